"""The look-ahead peak limiter (rc_engine_set_output_limiter; the definition is stated in include/rocoder_hip.h) in numpy,
in integers and f32 exactly as stated, the mutants the host tests must catch, and the ctypes binding of the test hook
rc_test_frames_limit (librocoder_hip_hooks.so) with guarded device buffers."""
import numpy as np

ONE = 1 << 24
MAX_LOOKAHEAD = 2048
ONE_BITS = 0x3F800000  # the bits of 1.0f: what the min-gain word holds in front of a job


def _f32(v):
    return np.float32(v)


def sliding_min(a, T):
    """out[j] = min a[j .. j + T), len(a) - T + 1 values, by log-step doubling"""
    a = np.asarray(a)
    assert 1 <= T <= a.size
    w, m = 1, a.copy()  # m[j] = min a[j .. j + w)
    while 2 * w <= T:
        m = np.minimum(m[:m.size - w], m[w:])
        w *= 2
    k = a.size - T + 1
    return np.minimum(m[:k], m[T - w:T - w + k])


def required_gain_q(v, ceiling):
    """rq[t] of the driven rows v[C, n]: the channel maximum over |v| < inf, ceiling / a where a > ceiling, times 2^24,
    truncated"""
    c = _f32(ceiling)
    av = np.abs(v)
    av = np.where(av < np.inf, av, _f32(0))  # (a NaN fails the test)
    a = av.max(axis=0) if v.shape[0] else np.zeros(v.shape[1], np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a > c, c / a, _f32(1)).astype(np.float32)
    return (r * _f32(16777216.0)).astype(np.float32).astype(np.uint32)


def gain_of(rq, L):
    """(g, S) of rq[n]: ONE outside, the minimum over |t - u| <= L, the 64-bit sum over |u - t| <= L, one f32 division"""
    n, T = rq.size, 2 * L + 1
    if n == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.uint64)
    padded = np.concatenate([np.full(2 * L, ONE, np.uint32), rq.astype(np.uint32), np.full(2 * L, ONE, np.uint32)])
    m = sliding_min(padded, T).astype(np.uint64)  # m[u], u in [-L, n + L)
    assert m.size == n + 2 * L
    P = np.concatenate([np.zeros(1, np.uint64), np.cumsum(m, dtype=np.uint64)])
    S = P[T:T + n] - P[:n]
    assert S.size == n and (S <= np.uint64(T * ONE)).all()
    g = (S.astype(np.float32) / _f32(T * ONE)).astype(np.float32)
    return g, S


def limit(rows, drive, ceiling, L, mutant=None):
    """rows float32 [C, n] -> (y float32 [C, n], g float32 [n], S uint64 [n]). mutant: None, or one of
    'half_window' (no minimum stage: the gain looks L, not 2 L, frames around),
    'unlinked' (the gain of each channel from its own r alone), 'no_clamp'."""
    x = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
    assert 0 <= L <= MAX_LOOKAHEAD and x.ndim == 2
    drive, c = _f32(drive), _f32(ceiling)
    T = 2 * L + 1
    with np.errstate(over="ignore", invalid="ignore"):
        v = (x * drive).astype(np.float32)
    if mutant == "unlinked":
        gs = [gain_of(required_gain_q(v[k:k + 1], c), L) for k in range(x.shape[0])]
        g = np.stack([q[0] for q in gs])
        S = np.minimum.reduce([q[1] for q in gs])
        with np.errstate(over="ignore", invalid="ignore"):
            y = (v * g).astype(np.float32)
        g = g.min(axis=0)
    else:
        rq = required_gain_q(v, c)
        if mutant == "half_window":
            n = rq.size
            padded = np.concatenate([np.full(L, ONE, np.uint64), rq.astype(np.uint64), np.full(L, ONE, np.uint64)])
            P = np.concatenate([np.zeros(1, np.uint64), np.cumsum(padded, dtype=np.uint64)])
            S = P[T:T + n] - P[:n]
            g = (S.astype(np.float32) / _f32(T * ONE)).astype(np.float32)
        else:
            g, S = gain_of(rq, L)
        with np.errstate(over="ignore", invalid="ignore"):
            y = (v * g[None, :]).astype(np.float32)
    if mutant != "no_clamp":
        y = np.where(y > c, c, np.where(y < -c, -c, y)).astype(np.float32)
    return y, g, S


def stats_of(g, S, L):
    """(the bits of the smallest g, 1.0f for no frame; the frames with S < T * ONE): what the two stats words hold"""
    T = 2 * L + 1
    bits = int(np.asarray(g, np.float32).view(np.uint32).min()) if g.size else ONE_BITS
    return min(bits, ONE_BITS), int((S < np.uint64(T * ONE)).sum())


# ---- the launcher on the GPU, through the test hook rc_test_frames_limit (librocoder_hip_hooks.so) -------------------------
GUARD_FLOATS = 8


def hook():
    import ctypes as C

    import frameskernelutil as K

    fn = K.hooks().rc_test_frames_limit
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_float, C.c_float, C.c_uint32,
                   C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    return fn


def gpu_limit(rows, drive, ceiling, L, n=None, src0=0, t0=0, t1=None, pad=0, ranges=None, halo_only=False, src_dev=None,
              src_stride=None):
    """launch_frames_limit on rows[:, i] = absolute frame src0 + i of a job of n frames. The frames [t0, t1) go to rows of a
    guard-filled block, dst_stride = t1 - t0 + pad, GUARD_FLOATS guard floats in front, behind and (pad) between the rows;
    `ranges` cuts [t0, t1) into the launches given (default: one), each with stats words of its own, joined on the host.
    halo_only: a launch is handed only the src frames [max(a - 2 L, 0), min(b + 2 L, n)) of its range [a, b).
    Returns (status of the last launch, y float32 [channels, t1 - t0], True where every guard float is unchanged,
    (min-gain bits, limited frames)). Every size is asserted before a launch."""
    import frameskernelutil as K

    rows = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
    ch, src_len = rows.shape
    n = src_len if n is None else n
    t1 = n if t1 is None else t1
    fn = hook()
    count = t1 - t0
    stride = max(count, 1) + pad
    total = GUARD_FLOATS + (ch - 1) * stride + max(count, 1) + GUARD_FLOATS
    host = np.full(total, K.GUARD_WORD, np.uint32)
    for c in range(ch):
        host[GUARD_FLOATS + c * stride:GUARD_FLOATS + c * stride + count] = 0
    dst = K.DevBuf(host)
    src = src_dev if src_dev is not None else K.DevBuf(rows if rows.size else np.zeros(ch, np.float32))
    row_stride = (max(src_len, 1) if src_stride is None else src_stride)
    assert src.nbytes >= 4 * ((ch - 1) * row_stride + src_len)
    status, bits, limited = 0, ONE_BITS, 0
    for a, b in (ranges if ranges is not None else [(t0, t1)]):
        assert t0 <= a <= b <= t1
        assert 4 * (GUARD_FLOATS + (ch - 1) * stride + (b - t0)) <= dst.nbytes - 4 * GUARD_FLOATS
        lo, length = src0, src_len
        if halo_only:
            lo = max(max(a - 2 * L, 0), src0)
            length = max(min(min(b + 2 * L, n), src0 + src_len) - lo, 0)
        # the launcher reads the floats c * row_stride + [lo - src0, lo - src0 + length) of src: inside the rows
        assert src0 <= lo and lo - src0 + length <= max(src_len, lo - src0)
        words = K.DevBuf(np.array([ONE_BITS, 0, 0, 0], np.uint32))
        status = fn(src.ptr(4 * (lo - src0)), lo, length, row_stride, ch, n, float(np.float32(drive)), float(np.float32(ceiling)), L,
                    dst.ptr(4 * (GUARD_FLOATS + (a - t0))), stride, a, b, None, 0, words.ptr())
        w = words.read().view(np.uint32)
        if status:
            assert w[0] == ONE_BITS and not w[1:].any()  # (a refused launch leaves the words alone)
            break
        bits = min(bits, int(w[0]))
        limited += int(w[2:4].view(np.uint64)[0])
    got = dst.read().view(np.uint32)
    y = np.empty((ch, count), np.float32)
    for c in range(ch):
        row = got[GUARD_FLOATS + c * stride:GUARD_FLOATS + c * stride + count]
        y[c] = row.view(np.float32)
        row[:] = K.GUARD_WORD
    return status, y, bool((got == K.GUARD_WORD).all()), (bits, limited)

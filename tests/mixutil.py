"""The mix bus (include/rocoder_hip_mix.h) in numpy: envelope, send and accumulate as the header states them, every step
ONE float32 operation (an explicit np.float32 array per operation; numpy fuses nothing). The send chain is the one place
where a fused multiply-add IS the definition: this Python (3.10) has no math.fma, so fmaf below forms the product exactly
in f64 (24 + 24 bits), adds with the error term of TwoSum and moves a sum that sits exactly on an f32 tie towards the
error before the one rounding to f32 - exact for finite operands whose result is a normal f32, which is what the send
cases use (`fmaf` asserts it).

Mutants of the definition, for the CPU proof in tests/test_mix_host.py: `mutant=` one of MUTANTS.

Also here: the ctypes binding of the launcher hook rc_test_frames_mix (librocoder_hip_hooks.so), over guarded device
blocks, and the cases tests/test_gpu_frames_mix_kernel.py and the CPU proof share."""
import ctypes as C
import math

import numpy as np

HAVE_MATH_FMA = hasattr(math, "fma")
MAX_KEYS = 4096
MUTANTS = ["bus_clock", "le_at_key", "contracted", "offset_sign", "drop_last", "send_transposed"]
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------- envelope
def sqrt_interp(a, b, r):
    """math::sqrt_interp(a, b, r) as written, float32 arrays, one rounding per operation"""
    a, b, r = (np.asarray(v, f32) for v in (a, b, r))
    inc = a < b
    c = (r * f32(2.0)).astype(f32)
    c = (c - f32(1.0)).astype(f32)
    pr = np.where(inc, c, -c).astype(f32)  # (c * +-1.0f)
    m = np.maximum(pr, f32(-1.0)).astype(f32)
    s = (f32(1.0) + m).astype(f32)
    h = (f32(0.5) * s).astype(f32)
    fct = np.sqrt(h).astype(f32)
    d = (b - a).astype(f32)
    w = np.abs(d).astype(f32)
    p = (w * fct).astype(f32)
    return (np.where(inc, a, b).astype(f32) + p).astype(f32)


def keys_of(keys):
    if keys is None or len(keys) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, f32)
    return np.array([int(k[0]) for k in keys], np.uint64), np.array([k[1] for k in keys], f32)


def envelope(keys, t, le_at_key=False):
    """amp(t) for the uint64 array t. le_at_key: the mutant that stays in segment i at t == key_frame[i + 1]."""
    kf, ka = keys_of(keys)
    t = np.asarray(t, np.uint64)
    K = kf.size
    if K == 0:
        return np.ones(t.shape, f32)
    if K == 1:
        return np.full(t.shape, ka[0], f32)
    with np.errstate(all="ignore"):
        idx = np.searchsorted(kf, t, side="left" if le_at_key else "right").astype(np.int64) - 1  # the last key <= t (mutant: < t)
        i = np.clip(idx, 0, K - 2)
        num = (t - kf[i]).astype(f32)  # (uint64 -> f32: round to nearest even)
        den = (kf[i + 1] - kf[i]).astype(f32)
        r = (num / den).astype(f32)
        amp = sqrt_interp(ka[i], ka[i + 1], r)
    amp = np.where(idx < 0, ka[0], amp)
    after = (t > kf[K - 1]) if le_at_key else (t >= kf[K - 1])
    return np.where(after, ka[K - 1], amp).astype(f32)


# ----------------------------------------------------------------------------------------------------------------- send
def fmaf(w, x, acc):
    """fmaf(w, x, acc) on float32 arrays with ONE rounding; exact for finite operands and a normal or zero result"""
    w, x, acc = (np.asarray(v, f32).astype(np.float64) for v in (w, x, acc))
    assert np.isfinite(w).all() and np.isfinite(x).all() and np.isfinite(acc).all()
    p = w * x  # exact
    s = p + acc
    bb = s - p
    e = (p - (s - bb)) + (acc - bb)  # TwoSum: p + acc = s + e exactly
    tie = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where(tie & (e != 0), np.nextafter(s, toward), s)
    out = s.astype(f32)
    assert ((out == 0) | (np.abs(out) >= np.finfo(f32).tiny)).all(), "fmaf: a denormal result is outside what this emulation covers"
    return out


def send_rows(x, send, transposed=False):
    """s[cb][t]: x itself where send is None, else one fmaf chain from +0 with cl ascending"""
    x = np.asarray(x, f32)
    if send is None:
        return x
    send = np.asarray(send, f32)
    CB, CL = send.shape
    assert x.shape[0] == CL
    out = np.zeros((CB, x.shape[1]), f32)
    for cb in range(CB):
        acc = np.zeros(x.shape[1], f32)
        for cl in range(CL):
            w = send.reshape(-1)[cl * CB + cb] if transposed else send[cb, cl]
            acc = fmaf(np.full(x.shape[1], w, f32), x[cl], acc)
        out[cb] = acc
    return out


# ------------------------------------------------------------------------------------------------------------ accumulate
def mix(bus, x, offset=0, keys=None, send=None, x0=0, mutant=None):
    """The bus after one layer: x[:, i] is layer frame x0 + i. Returns a new array; `bus` is not changed."""
    assert mutant is None or mutant in MUTANTS
    bus = np.array(bus, f32, copy=True)
    x = np.asarray(x, f32)
    CB, N = bus.shape
    n = x.shape[1]
    if mutant == "drop_last":
        n = max(n - 1, 0)
    if mutant == "offset_sign":
        offset = -offset
    with np.errstate(all="ignore"):
        s = send_rows(x, send, transposed=mutant == "send_transposed")
        assert s.shape[0] == CB
        t = np.arange(x0, x0 + n, dtype=np.int64)
        u = t + offset
        ok = (u >= 0) & (u < N)
        t, u = t[ok], u[ok]
        clock = (u if mutant == "bus_clock" else t).astype(np.uint64)
        amp = envelope(keys, clock, le_at_key=mutant == "le_at_key")
        for cb in range(CB):
            sv = s[cb, t - x0]
            if mutant == "contracted":
                fin = np.isfinite(sv) & np.isfinite(bus[cb, u])
                r = (bus[cb, u].astype(np.float64) + sv.astype(np.float64) * amp.astype(np.float64)).astype(f32)  # (one rounding, near enough)
                plain = (bus[cb, u] + (sv * amp).astype(f32)).astype(f32)
                bus[cb, u] = np.where(fin, r, plain)
            else:
                prod = (sv * amp).astype(f32)
                bus[cb, u] = (bus[cb, u] + prod).astype(f32)
    return bus, int(ok.sum())


# ---------------------------------------------------------------------------------------------------------------- values
def special_values():
    tiny = np.finfo(f32).tiny
    return np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, tiny / 2, -tiny / 4, np.float32(1e-45), tiny, 0.99999994, 3.4e38], f32)


def rows(channels, n, seed, specials=True):
    """white float32 rows in [-1, 1]; with `specials` every fourth frame from frame 5 on holds one of special_values()"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (channels, n)).astype(f32)
    if specials:
        sp = special_values()
        for c in range(channels):
            at = np.arange(5 + c, n, 4)
            x[c, at] = sp[(np.arange(at.size) + c) % sp.size]
    return x


def same(got, want):
    """bit for bit, but a NaN of `want` asks for a NaN of any payload (an IEEE operation made it)"""
    g = np.ascontiguousarray(got, f32).view(np.uint32).reshape(-1)
    w = np.ascontiguousarray(want, f32).view(np.uint32).reshape(-1)
    if g.shape != w.shape:
        return False
    wn, gn = (w & 0x7FFFFFFF) > 0x7F800000, (g & 0x7FFFFFFF) > 0x7F800000
    return bool((wn == gn).all() and (g[~wn] == w[~wn]).all())


# ---- the cases the kernel test runs and the CPU proof replays: (name, dict) ------------------------------------------------
# Amplitudes: 0.15 -> 0.7 and 0.15 -> 0.95 are pairs with a + fl(b - a) != b in f32, which is what shows `<=` for `<` at a
# rising key; keys sit on frames that are group, tile (1024) and workgroup edges of the launch and one off them.
RISE_FALL = [(0, 0.15), (1024, 0.7), (1025, 0.7), (2048, -0.25), (2051, 0.15), (3000, 0.95)]


def kernel_cases():
    cases = []
    for off in range(4):  # every offset mod 4 against every row alignment
        for align in range(4):
            cases.append((f"offset {off + 8} align {align}", dict(n=3001, N=3100, offset=off + 8, align=align, keys=RISE_FALL, CL=2, CB=2)))
    cases += [
        ("negative offset", dict(n=3001, N=3100, offset=-1027, keys=RISE_FALL, CL=2, CB=2)),
        ("partly past N", dict(n=3001, N=2000, offset=5, keys=RISE_FALL, CL=2, CB=2)),
        ("wholly past N", dict(n=3001, N=100, offset=100, keys=RISE_FALL, CL=2, CB=2)),
        ("wholly in front", dict(n=300, N=100, offset=-300, keys=RISE_FALL, CL=2, CB=2)),
        ("N = 0", dict(n=300, N=0, offset=0, keys=RISE_FALL, CL=2, CB=2)),
        ("N = 1", dict(n=300, N=1, offset=-7, keys=RISE_FALL, CL=2, CB=2)),
        ("N = 5", dict(n=300, N=5, offset=-2, keys=RISE_FALL, CL=2, CB=2)),
        ("no keys", dict(n=3001, N=3100, offset=3, keys=[], CL=2, CB=2)),
        ("one key", dict(n=3001, N=3100, offset=3, keys=[(77, -0.6)], CL=2, CB=2)),
        ("two keys", dict(n=3001, N=3100, offset=3, keys=[(1, 0.0), (2999, 1.0)], CL=2, CB=2)),
        ("equal amplitudes", dict(n=3001, N=3100, offset=0, keys=[(10, 0.4), (1500, 0.4), (2500, -0.4)], CL=2, CB=2)),
        ("mono into stereo", dict(n=3001, N=3100, offset=2, keys=RISE_FALL, CL=1, CB=2, send=[[0.75], [-0.5]], specials=False)),
        ("three into two", dict(n=3001, N=3100, offset=1, keys=RISE_FALL, CL=3, CB=2, send=[[0.5, 0.25, -0.125], [0.3, -0.7, 0.9]],
                                specials=False)),
    ]
    return cases


def case_inputs(kw, seed=11):
    x = rows(kw["CL"], kw["n"], seed, specials=kw.get("specials", True))
    bus = rows(kw["CB"], kw["N"], seed + 1, specials=False)  # pre-filled, not zero: the accumulation is seen
    send = None if kw.get("send") is None else np.array(kw["send"], f32)
    return x, bus, send


# ---- the launcher on the GPU, through the test hook rc_test_frames_mix (librocoder_hip_hooks.so) ------------------------
GUARD_FLOATS = 8
GUARD_NAN = 0x7FC0A5A5  # a quiet NaN


def gpu_mix(x, bus, offset=0, keys=None, send=None, x0=0, ranges=None, align=0, row_pad=3):
    """launch_frames_mix on x[:, i] = layer frame x0 + i, once per (t0, t1) of `ranges` (default: the whole of x). The rows
    start `align` floats behind a 16-byte boundary, row_pad floats apart; the bus rows lie in a block of quiet-NaN guard
    words - GUARD_FLOATS in front and behind, and the words [N, stride) of every row. Returns (status of the last launch,
    the bus as float32 [CB, N], True where every guard word is unchanged). Every size is asserted before a launch."""
    import frameskernelutil as K

    x = np.ascontiguousarray(np.atleast_2d(x), f32)
    bus = np.ascontiguousarray(np.atleast_2d(bus), f32)
    CL, n = x.shape
    CB, N = bus.shape
    kf, ka = keys_of(keys)
    H = K.hooks()
    fn = H.rc_test_frames_mix
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int64,
                   C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    stride = max(4, (N + 3) // 4 * 4 + (4 if N % 4 == 0 else 0))  # a multiple of 4 with at least one guard word behind every row
    host = np.full(2 * GUARD_FLOATS + CB * stride, GUARD_NAN, np.uint32)
    for c in range(CB):
        host[GUARD_FLOATS + c * stride:GUARD_FLOATS + c * stride + N] = bus[c].view(np.uint32)
    d_bus = K.DevBuf(host)
    row_stride = n + row_pad
    xh = np.zeros(align + CL * row_stride + 4, f32)
    for c in range(CL):
        xh[align + c * row_stride:align + c * row_stride + n] = x[c]
    d_x = K.DevBuf(xh)
    d_kf = K.DevBuf(kf.view(np.uint32)) if kf.size else None
    d_ka = K.DevBuf(ka) if ka.size else None
    d_send = None
    if send is not None:
        send = np.ascontiguousarray(send, f32)
        assert send.shape == (CB, CL)
        d_send = K.DevBuf(send)
    assert kf.size == ka.size and (d_kf is None or (d_kf.nbytes == 8 * kf.size and d_ka.nbytes == 4 * ka.size))
    assert d_bus.nbytes == 4 * host.size and (GUARD_FLOATS * 4) % 16 == 0 and stride % 4 == 0 and stride >= N
    status = 0
    for a, b in (ranges if ranges is not None else [(x0, x0 + n)]):
        assert x0 <= a and b <= x0 + n  # (a > b is the launcher's to refuse: it reads nothing then)
        assert 4 * (align + (CL - 1) * row_stride + (max(a, b) - x0)) <= d_x.nbytes
        status = fn(d_x.ptr(4 * (align + (a - x0))), row_stride, CL, a, b, d_bus.ptr(4 * GUARD_FLOATS), stride, CB, N, offset,
                    d_kf.ptr() if d_kf else None, d_ka.ptr() if d_ka else None, kf.size, d_send.ptr() if d_send else None)
        if status:
            break
    got = d_bus.read().view(np.uint32)
    out = np.empty((CB, N), f32)
    for c in range(CB):
        row = got[GUARD_FLOATS + c * stride:GUARD_FLOATS + c * stride + N]
        out[c] = row.view(f32)
        row[:] = GUARD_NAN
    return status, out, bool((got == GUARD_NAN).all())


# ---- the keys of the reference's Layer::fade_in_out (src/mixer.rs:179-190), placed as dur_to_sample places them ----------
def dur_to_sample(secs, rate):
    """(secs_f32 * rate as f32) as usize"""
    return int(f32(f32(secs) * f32(rate)))


def fade_keys(fade_secs, total_samples, rate):
    """(0, 0), (d(fade), 1), (d(T - fade), 1), (d(T), 0), T = total_samples as f32 / rate as f32 seconds; durations are whole
    nanoseconds, as the reference's are. A key that repeats the frame and amplitude of the one before it is dropped; a
    repeated frame with another amplitude is an error."""
    ns = lambda s: int(float(f32(s)) * 1e9)  # noqa: E731  (the f32 seconds times 1e9 in f64, truncated)
    secs = lambda n: f32(f32(n // 10 ** 9) + f32(f32(n % 10 ** 9) / f32(1e9)))  # noqa: E731  (Duration::as_secs_f32)
    T, F = ns(f32(f32(total_samples) / f32(rate))), ns(fade_secs)
    if F > T:
        raise ValueError("the fade is longer than the layer")
    raw = [(0, 0.0), (dur_to_sample(secs(F), rate), 1.0), (dur_to_sample(secs(T - F), rate), 1.0), (dur_to_sample(secs(T), rate), 0.0)]
    keys = []
    for k in raw:
        if keys and keys[-1] == k:
            continue
        if keys and keys[-1][0] >= k[0]:
            raise ValueError(f"keys {keys[-1]} and {k} share a frame")
        keys.append(k)
    return keys

"""The definition of the output warp (rc_engine_set_output_warp, include/rocoder_hip_warp.h) in numpy and Python integers:
the tier constants, the f64 filter tables, the positions, the f64 warp of given rows with given f32 tables and the error
bound the two f32 chains and the interpolation between them may reach, a CPU f32 implementation with its mutants, the
Python twin of rc_warp_curve, and the launcher on the GPU through its test hook. The tests of the host helpers, of the
kernel and of the engine hold the C and HIP code to it."""
import math
from fractions import Fraction

import numpy as np

import resampleutil as R

TIERS, BLOCK, PHASES, ROWS = 13, 64, 256, 257
D_MIN, D_MAX = 2 ** 35, 2 ** 41
# floor(2^(t/4) * 2^38) and ceil(32 * 2^(t/4)), as the header writes them
D = [274877906944, 326886762694, 388736063996, 462287693163, 549755813888, 653773525389, 777472127993, 924575386326,
     1099511627776, 1307547050779, 1554944255987, 1849150772653, 2199023255552]
W = [32, 39, 46, 54, 64, 77, 91, 108, 128, 153, 182, 216, 256]
QUARTER = [1.0, 0.8408964152537145, 0.7071067811865476, 0.5946035575013605]  # 2^(-k/4), the doubles the engine uses


def exact_D(t):
    """floor(2^(t/4) * 2^38) in exact arithmetic: the largest integer d with d^4 <= 2^t * 2^152"""
    target = 2 ** t * 2 ** 152
    d = int(round(2.0 ** (t / 4 + 38)))
    while d ** 4 > target:
        d -= 1
    while (d + 1) ** 4 <= target:
        d += 1
    return d


def exact_W(t):
    """ceil(32 * 2^(t/4)): the smallest integer w with w^4 >= 32^4 * 2^t"""
    target = 32 ** 4 * 2 ** t
    w = int(round(32 * 2.0 ** (t / 4)))
    while w ** 4 < target:
        w += 1
    while (w - 1) ** 4 >= target:
        w -= 1
    return w


def tier_of(d):
    assert D_MIN <= d <= D_MAX
    return next(t for t in range(TIERS) if d <= D[t])


def cutoff(t):
    return R.ROLLOFF * math.ldexp(QUARTER[t % 4], -(t // 4))


def prototype(t, u):
    """the tier's prototype filter at the float64 offsets u: c sinc(c u) I0(beta sqrt(1 - (u / W)^2)) / I0(beta), |u| < W"""
    u = np.asarray(u, np.float64)
    c, w = cutoff(t), W[t]
    inside = np.abs(u) < w
    r = np.where(inside, u / w, 0.0)
    h = c * np.sinc(c * u) * np.i0(R.BETA * np.sqrt(1.0 - r * r)) / np.i0(R.BETA)
    return np.where(inside, h, 0.0)


def table_f64(t):
    """float64 [257, T]: row p at u = j - (W - 1) - p / 256"""
    j = np.arange(2 * W[t], dtype=np.float64)[None, :]
    p = np.arange(ROWS, dtype=np.float64)[:, None]
    return prototype(t, j - (W[t] - 1) - p / PHASES)


def position(anchor, m, wrap32=False, next_shift=0):
    """(P(m), D_b); the mutants: D * i held in 32 bits, the step taken from the block behind"""
    b, i = divmod(m, BLOCK)
    nb = min(b + next_shift, len(anchor) - 2)
    prod = (int(anchor[nb + 1]) - int(anchor[nb])) * i
    if wrap32:
        prod &= 0xFFFFFFFF
    return int(anchor[b]) + (prod >> 6), int(anchor[b + 1]) - int(anchor[b])


def split(P):
    return P >> 32, (P >> 24) & 255, np.float32(P & 0xFFFFFF) * np.float32(2.0 ** -24)


def plan(anchor, m0, m1, **mut):
    """per output of [m0, m1): (tier, q, p, a)"""
    out = []
    for m in range(m0, m1):
        P, d = position(anchor, m, **mut)
        out.append((tier_of(d),) + split(P))
    return out


def warp_f64(rows, tables, anchor, n_out, n=None, src0=0, m0=0, m1=None):
    """(y, bound): float64 [channels, m1 - m0] each. y is the definition in f64 over the given f32 tables {tier: [257, T]}:
    (1 - a) y0 + a y1 of the exact dot products. bound = gamma_{T+3} * (sum |h_p||x| + sum |h_{p+1}||x|) + 1e-30 with
    gamma_k = k u / (1 - k u), u = 2^-24: each chain is a length-T f32 dot product (gamma_T of its own sum), the
    difference, the product with a and the last sum are three more roundings on values the two sums bound."""
    rows = np.atleast_2d(rows)
    n = rows.shape[1] if n is None else n
    m1 = n_out if m1 is None else m1
    y = np.zeros((rows.shape[0], m1 - m0))
    bound = np.zeros_like(y)
    u = 2.0 ** -24
    for o, (t, q, p, a) in enumerate(plan(anchor, m0, m1)):
        h = tables[t].astype(np.float64)
        T = h.shape[1]
        x = R.gather(rows, n, src0, [q - (W[t] - 1)], T)[:, 0, :]
        y0, y1 = x @ h[p], x @ h[p + 1]
        a = float(a)
        y[:, o] = y0 if a == 0.0 else y0 + a * (y1 - y0)
        g = (T + 3) * u / (1.0 - (T + 3) * u)
        bound[:, o] = g * (np.abs(x) @ np.abs(h[p]) + np.abs(x) @ np.abs(h[p + 1])) + 1e-30
    return y, bound


def warp_f32(rows, tables, anchor, n_out, n=None, src0=0, m0=0, m1=None, drop_a=False, tier_shift=0, wrap_row=False, wrap32=False,
             next_shift=0, k0_shift=0):
    """A CPU f32 implementation (two sequential f32 chains and the f32 interpolation), and its mutants: `a` dropped (the
    nearest lower phase), the tier off by one, row 256 read as row 0, D * i held in 32 bits, anchor[b + 1] taken from the
    wrong block, k0 shifted by one."""
    rows = np.atleast_2d(rows)
    n = rows.shape[1] if n is None else n
    m1 = n_out if m1 is None else m1
    y = np.zeros((rows.shape[0], m1 - m0), np.float32)
    for o, (t, q, p, a) in enumerate(plan(anchor, m0, m1, wrap32=wrap32, next_shift=next_shift)):
        t = min(max(t + tier_shift, 0), TIERS - 1)
        h = tables[t]
        T = h.shape[1]
        x = R.gather(rows, n, src0, [q - (W[t] - 1) + k0_shift], T)[:, 0, :].astype(np.float32)
        p1 = 0 if wrap_row and p + 1 == 256 else p + 1
        y0 = np.zeros(rows.shape[0], np.float32)
        y1 = np.zeros(rows.shape[0], np.float32)
        for j in range(T):
            y0 = (y0 + x[:, j] * h[p, j]).astype(np.float32)
            y1 = (y1 + x[:, j] * h[p1, j]).astype(np.float32)
        y[:, o] = y0 if (drop_a or a == 0) else (y0 + a * (y1 - y0).astype(np.float32)).astype(np.float32)
    return y


# ---- the Python twin of rc_warp_curve: the same IEEE double operations, one per statement -----------------------------
def ratio_at(at, ratio, q):
    n = len(at)
    if q <= at[0]:
        return ratio[0]
    if q >= at[n - 1]:
        return ratio[n - 1]
    seg = 0
    while seg + 2 < n and at[seg + 1] <= q:
        seg += 1
    dr = ratio[seg + 1] - ratio[seg]
    dq = q - at[seg]
    da = at[seg + 1] - at[seg]
    t = dq / da
    m = dr * t
    return ratio[seg] + m


def warp_curve(par, hop_pos, n_hops, at, ratio, n):
    """(anchors, n_out) for rc_params `par`; hop_pos None: the engine's grid"""
    at, ratio = [float(v) for v in at], [float(v) for v in ratio]
    hpw, wout, step = int(par.hops_per_window), int(par.window_out_len), int(par.sample_step_len)
    anchors, A, n_out = [0], 0, 0
    while (A >> 32) < n:
        k = min(n_hops - 1, (A >> 32) * hpw // wout)
        pos = float(int(hop_pos[k])) if hop_pos is not None else float(k * step)
        r = ratio_at(at, ratio, pos)
        scaled = r * 2.0 ** 38
        half = scaled + 0.5
        d = min(max(int(math.floor(half)), D_MIN), D_MAX)
        if (A + d) >> 32 >= n:
            i = 0
            while i < BLOCK and (A + ((d * i) >> 6)) >> 32 < n:
                i += 1
            n_out = (len(anchors) - 1) * BLOCK + i
        A += d
        anchors.append(A)
    return np.array(anchors, np.int64), n_out


def constant_anchors(num, den, n_out):
    """the anchors of the constant step num / den for n_out outputs"""
    d = Fraction(num * 2 ** 38, den)
    assert d.denominator == 1
    return np.arange(-(-n_out // BLOCK) + 1, dtype=np.int64) * int(d)


# ---- the launcher on the GPU, through the test hook rc_test_frames_warp (librocoder_hip_hooks.so) ----------------------
GUARD_FLOATS = R.GUARD_FLOATS


def device_tables(tables):
    """(float32 array, uint32 [13] offsets): the tiers given, tap-major, as the engine uploads them"""
    parts, off, at = [], np.full(TIERS, 0xFFFFFFFF, np.uint32), 0
    for t in sorted(tables):
        assert tables[t].shape == (ROWS, 2 * W[t]) and tables[t].dtype == np.float32
        off[t] = at
        parts.append(np.ascontiguousarray(tables[t].T).reshape(-1))
        at += parts[-1].size
    return np.concatenate(parts), off


def gpu_warp(rows, tables, anchor, n_out, n=None, src0=0, m0=0, m1=None, pad=0, ranges=None, host_anchor=None):
    """launch_frames_warp on rows[:, i] = absolute input frame src0 + i of a job of n frames. The outputs [m0, m1) go to
    rows of a guard-filled block, dst_stride = m1 - m0 + pad, GUARD_FLOATS guard floats in front, behind and (pad) between
    the rows; `ranges` cuts [m0, m1) into the launches given (default: one). Returns (status of the last launch, y as
    float32 [channels, m1 - m0], True where every guard float is unchanged). Every size is asserted before a launch."""
    import ctypes as C

    import frameskernelutil as K

    rows = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
    ch, src_len = rows.shape
    n = src_len if n is None else n
    m1 = n_out if m1 is None else m1
    anchor = np.ascontiguousarray(anchor, np.int64)
    host_anchor = anchor if host_anchor is None else np.ascontiguousarray(host_anchor, np.int64)
    assert host_anchor.size == anchor.size >= 2 and m1 <= BLOCK * (anchor.size - 1)
    # what the kernel reads of the device tables: every block's tier is one of those given, its step in range
    for b in range(anchor.size - 1):
        assert tier_of(int(anchor[b + 1]) - int(anchor[b])) in tables
    flat, off = device_tables(tables)
    H = K.hooks()
    fn = H.rc_test_frames_warp
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
    count = m1 - m0
    stride = max(count, 1) + pad
    total = GUARD_FLOATS + (ch - 1) * stride + max(count, 1) + GUARD_FLOATS
    host = np.full(total, K.GUARD_WORD, np.uint32)
    for c in range(ch):
        host[GUARD_FLOATS + c * stride:GUARD_FLOATS + c * stride + count] = 0
    dst = K.DevBuf(host)
    src = K.DevBuf(rows if rows.size else np.zeros(1, np.float32))
    tab = K.DevBuf(flat)
    anc = K.DevBuf(anchor.view(np.uint32))
    assert tab.nbytes == 4 * flat.size and anc.nbytes == 8 * anchor.size and src.nbytes >= 4 * ch * src_len
    assert all(int(o) + ROWS * 2 * W[t] <= flat.size for t, o in enumerate(off) if o != 0xFFFFFFFF)
    status = 0
    for a, b in (ranges if ranges is not None else [(m0, m1)]):
        assert m0 <= a <= b <= m1
        assert 4 * (GUARD_FLOATS + (ch - 1) * stride + (b - m0)) <= dst.nbytes - 4 * GUARD_FLOATS
        status = fn(src.ptr(), src0, src_len, max(src_len, 1), ch, n, tab.ptr(), off.ctypes.data, anc.ptr(), host_anchor.ctypes.data,
                    anchor.size, dst.ptr(4 * (GUARD_FLOATS + (a - m0))), stride, a, b)
        if status:
            break
    got = dst.read().view(np.uint32)
    y = np.empty((ch, count), np.float32)
    for c in range(ch):
        row = got[GUARD_FLOATS + c * stride:GUARD_FLOATS + c * stride + count]
        y[c] = row.view(np.float32)
        row[:] = K.GUARD_WORD
    return status, y, bool((got == K.GUARD_WORD).all())


# ---- the case the kernel test and the gate's own test share -------------------------------------------------------------
def white_rows(channels=2, n=3000, seed=2024):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (channels, n)).astype(np.float32)


def glide_case(n=3000, lo=0.5, hi=2.5, seed=7):
    """(anchors, n_out): a glide from `lo` to `hi` input frames per output frame over rows of n frames, every block's step
    jittered by up to 12 %, so that neighbouring blocks differ in tier and the positions take every phase and fraction"""
    rng = np.random.default_rng(seed)
    blocks = int(n / (BLOCK * (lo + hi) / 2)) + 2
    anchors = [0]
    for b in range(blocks):
        r = (lo + (hi - lo) * b / (blocks - 1)) * (1.0 + rng.uniform(-0.12, 0.12))
        anchors.append(anchors[-1] + min(max(int(r * 2 ** 38) | 1, D_MIN), D_MAX))
    anchors = np.array(anchors, np.int64)
    n_out = sum(1 for m in range(BLOCK * blocks) if position(anchors, m)[0] >> 32 < n)
    return anchors, n_out

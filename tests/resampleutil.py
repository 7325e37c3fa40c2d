"""The definition of the band-limited resampler (rc_engine_set_output_resample, include/rocoder_hip.h) in numpy and Python
integers: the f64 filter table, the f64 resample of given rows with a given f32 table, and the error bound a length-T f32
dot product may reach. The tests of the host helpers, of the kernel and of the engine hold the C and HIP code to it."""
from fractions import Fraction
from math import gcd

import numpy as np

Z, BETA, ROLLOFF = 32, 9.0, 0.9
MAX_DEN, MAX_STEP = 1024, 8
# the ratios the filter's figures were checked on
RATIOS = [(160, 147), (147, 160), (3, 2), (2, 3), (1024, 967), (967, 1024), (2, 1), (1, 2), (8, 1), (1, 8), (5, 1), (1, 3)]


def reduced(num, den):
    g = gcd(num, den)
    return num // g, den // g


def half_width(num, den):
    num, den = reduced(num, den)
    return Z if num <= den else -((-Z * num) // den)


def resample_len(n, num, den):
    """the m with m * num / den < n"""
    return 0 if n == 0 else (n * den - 1) // num + 1


def table_f64(num, den):
    """float64 [den, T] of the reduced step: h[p][j] = c sinc(c u) I0(beta sqrt(1 - (u / W)^2)) / I0(beta), |u| < W"""
    num, den = reduced(num, den)
    W = half_width(num, den)
    c = ROLLOFF * min(1.0, den / num)
    j = np.arange(2 * W, dtype=np.float64)[None, :]
    p = np.arange(den, dtype=np.float64)[:, None]
    u = j - (W - 1) - p / den
    inside = np.abs(u) < W
    r = np.where(inside, u / W, 0.0)
    h = c * np.sinc(c * u) * np.i0(BETA * np.sqrt(1.0 - r * r)) / np.i0(BETA)
    return np.where(inside, h, 0.0)


def positions(m0, m1, num, den, W):
    """(p, k0) of the outputs [m0, m1): Python integers, whatever their size"""
    ps, k0s = [], []
    for m in range(m0, m1):
        q, p = divmod(m * num, den)
        ps.append(p)
        k0s.append(q - (W - 1))
    return ps, k0s


def gather(rows, n, src0, k0s, T):
    """float64 [channels, outputs, T]: x[c][k0 + j], zero outside [0, n); rows[:, i] is absolute input frame src0 + i"""
    rows = np.atleast_2d(rows)
    out = np.zeros((rows.shape[0], len(k0s), T), np.float64)
    for i, k0 in enumerate(k0s):
        lo, hi = max(k0, 0, src0), min(k0 + T, n, src0 + rows.shape[1])
        if lo < hi:
            out[:, i, lo - k0:hi - k0] = rows[:, lo - src0:hi - src0]
    return out


def resample_f64(rows, table_f32, num, den, n=None, src0=0, m0=0, m1=None):
    """(y, bound): float64 [channels, m1 - m0] each. y is the definition in f64 over the given f32 table; bound is
    gamma * sum_j |h_j| |x_j| + 1e-30 with gamma = T u / (1 - T u), u = 2^-24: the standard bound of a length-T f32 dot
    product in any order, with or without fma."""
    rows = np.atleast_2d(rows)
    num, den = reduced(num, den)
    n = rows.shape[1] if n is None else n
    m1 = resample_len(n, num, den) if m1 is None else m1
    T = table_f32.shape[1]
    W = T // 2
    ps, k0s = positions(m0, m1, num, den, W)
    x = gather(rows, n, src0, k0s, T)
    h = table_f32.astype(np.float64)[ps] if ps else np.zeros((0, T))
    y = np.einsum("cmj,mj->cm", x, h)
    tu = T * 2.0 ** -24
    bound = tu / (1.0 - tu) * np.einsum("cmj,mj->cm", np.abs(x), np.abs(h)) + 1e-30
    return y, bound


def resample_f32(rows, table_f32, num, den, n=None, src0=0, m0=0, m1=None, k0_shift=0, p_shift=0, mirror=False, wrap32=False):
    """A CPU f32 implementation (sequential f32 accumulation), and its mutants: taps from k0 + k0_shift, row p + p_shift,
    rows mirrored, m * num held in 32 bits."""
    rows = np.atleast_2d(rows)
    num, den = reduced(num, den)
    n = rows.shape[1] if n is None else n
    m1 = resample_len(n, num, den) if m1 is None else m1
    T = table_f32.shape[1]
    W = T // 2
    ps, k0s = [], []
    for m in range(m0, m1):
        q, p = divmod((m * num) & 0xFFFFFFFF if wrap32 else m * num, den)
        ps.append((p + p_shift) % den)
        k0s.append(q - (W - 1) + k0_shift)
    x = gather(rows, n, src0, k0s, T).astype(np.float32)
    h = table_f32[:, ::-1] if mirror else table_f32
    acc = np.zeros(x.shape[:2], np.float32)
    for j in range(T):
        acc = (acc + x[:, :, j] * h[ps, j][None, :]).astype(np.float32)
    return acc


def response_db(table_f32, num, den, freqs):
    """|H| in dB at `freqs` (fractions of the INPUT's Nyquist frequency) of the prototype the table samples den times per
    input frame: H(f) = 1/den * sum over (p, j) of h[p][j] exp(-i pi f u(p, j)). Its own Nyquist frequency is den."""
    num, den = reduced(num, den)
    T = table_f32.shape[1]
    W = T // 2
    h = table_f32.astype(np.float64).reshape(-1)
    u = (np.arange(T)[None, :] - (W - 1) - np.arange(den)[:, None] / den).reshape(-1)
    out = []
    for f in np.asarray(freqs, np.float64).reshape(-1):
        out.append(abs(np.dot(h, np.exp(-1j * np.pi * f * u))) / den)
    return 20 * np.log10(np.maximum(np.array(out), 1e-300))


def best_ratio(step):
    f = Fraction(step).limit_denominator(MAX_DEN)
    return f.numerator, f.denominator


# ---- the launcher on the GPU, through the test hook rc_test_frames_resample (librocoder_hip_hooks.so) ----------------------
GUARD_FLOATS = 8


def gpu_resample(rows, table_f32, num, den, n=None, src0=0, m0=0, m1=None, pad=0, ranges=None, table_dev=None, src_dev=None):
    """launch_frames_resample on rows[:, i] = absolute input frame src0 + i of a job of n frames. The outputs [m0, m1) go to
    rows of a guard-filled block, dst_stride = m1 - m0 + pad, GUARD_FLOATS guard floats in front, behind and (pad) between
    the rows; `ranges` cuts [m0, m1) into the launches given (default: one). Returns (status of the last launch, y as
    float32 [channels, m1 - m0], True where every guard float is unchanged). Every size is asserted before a launch."""
    import ctypes as C

    import frameskernelutil as K

    rows = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
    ch, src_len = rows.shape
    num, den = reduced(num, den)
    n = src_len if n is None else n
    m1 = resample_len(n, num, den) if m1 is None else m1
    T = table_f32.shape[1]
    assert table_f32.shape == (den, T) and table_f32.dtype == np.float32 and T == 2 * half_width(num, den)
    H = K.hooks()
    fn = H.rc_test_frames_resample
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32,
                   C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
    count = m1 - m0
    stride = max(count, 1) + pad
    # guard floats | row 0 | pad | row 1 | ... | guard floats
    total = GUARD_FLOATS + (ch - 1) * stride + max(count, 1) + GUARD_FLOATS
    host = np.full(total, K.GUARD_WORD, np.uint32)
    for c in range(ch):
        host[GUARD_FLOATS + c * stride:GUARD_FLOATS + c * stride + count] = 0
    dst = K.DevBuf(host)
    src = src_dev if src_dev is not None else K.DevBuf(rows if rows.size else np.zeros(1, np.float32))
    tab = table_dev if table_dev is not None else K.DevBuf(table_f32)
    assert tab.nbytes == 4 * den * T and tab.base % 8 == 0 and src.nbytes >= 4 * ch * src_len
    status = 0
    for a, b in (ranges if ranges is not None else [(m0, m1)]):
        assert m0 <= a <= b <= m1
        # the launch writes floats GUARD + c * stride + [a - m0, b - m0) of dst: inside the rows laid out above
        assert 4 * (GUARD_FLOATS + (ch - 1) * stride + (b - m0)) <= dst.nbytes - 4 * GUARD_FLOATS
        status = fn(src.ptr(), src0, src_len, max(src_len, 1), ch, n, tab.ptr(), num, den, T // 2,
                    dst.ptr(4 * (GUARD_FLOATS + (a - m0))), stride, a, b)
        if status:
            break
    got = dst.read().view(np.uint32)
    y = np.empty((ch, count), np.float32)
    for c in range(ch):
        row = got[GUARD_FLOATS + c * stride:GUARD_FLOATS + c * stride + count]
        y[c] = row.view(np.float32)
        row[:] = K.GUARD_WORD
    return status, y, bool((got == K.GUARD_WORD).all())

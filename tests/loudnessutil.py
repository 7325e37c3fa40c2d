"""The definition of rc_engine_stretch_frames_loud's two measurements (include/rocoder_hip.h) in numpy: the K-weighting
coefficients, the f64 recurrence, the sub-block energies, the gate of BS.1770-4, the true peak as the resampler's fmaf chain
at the step 1/4, the gain - each with the mutants that tests/test_loudness_host.py proves the gates catch. The tests of the
host helpers, of the kernels and of the engine hold the C and HIP code to it. Also the test inputs the CPU and the GPU tests
share, and the two launchers through the test hooks rc_test_frames_kweight_energy / rc_test_frames_true_peak."""
import ctypes as C

import numpy as np

MIN_RATE, MAX_RATE = 8000, 768000
BS1770_48K = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
GATE_REL = 2.3e-3  # 0.01 dB of energy: 10^(0.01 / 10) - 1
ABS_GATE_ENERGY = 10.0 ** ((-70.0 + 0.691) / 10.0)  # the mean square of -70 LUFS


def coeffs_f64(rate):
    """b0 b1 b2 a1 a2 of the shelf, then of the high-pass, as the header states them"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
          (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return np.array(s1 + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)


def sub_frames(rate):
    return (rate + 5) // 10


def _biquad(b, a, x):
    try:
        from scipy.signal import lfilter
        return lfilter(b, np.concatenate([[1.0], a]), x, axis=-1)
    except ImportError:
        y = np.zeros_like(x)
        s1 = np.zeros(x.shape[:-1])
        s2 = np.zeros(x.shape[:-1])
        for t in range(x.shape[-1]):
            xt = x[..., t]
            yt = b[0] * xt + s1
            s1 = b[1] * xt - a[0] * yt + s2
            s2 = b[2] * xt - a[1] * yt
            y[..., t] = yt
        return y


def kweight(rows, rate, shelf=True, highpass=True):
    """k[c] in f64 (mutants: a stage left out)"""
    k = np.atleast_2d(np.asarray(rows, np.float64))
    c = coeffs_f64(rate)
    if shelf:
        k = _biquad(c[0:3], c[3:5], k)
    if highpass:
        k = _biquad(c[5:8], c[8:10], k)
    return k


def sub_energies(rows, rate, shelf=True, highpass=True, reset=False):
    """float64 [channels, nb] (mutant `reset`: the state zeroed at every sub-block, no warm-up)"""
    rows = np.atleast_2d(np.asarray(rows, np.float64))
    sub = sub_frames(rate)
    nb = rows.shape[1] // sub
    if reset:
        k = np.concatenate([kweight(rows[:, j * sub:(j + 1) * sub], rate, shelf, highpass) for j in range(nb)], axis=1) if nb else rows[:, :0]
    else:
        k = kweight(rows, rate, shelf, highpass)[:, :nb * sub]
    return (k.reshape(rows.shape[0], nb, sub) ** 2).sum(axis=2)


def lufs_of(x):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(x)


def block_loudness(e, sub, overlap=True, offset=True):
    """(l[i], L(l[i])) of the 400 ms blocks (mutants: blocks without overlap, -0.691 dropped)"""
    e = np.atleast_2d(np.asarray(e, np.float64))
    nb = e.shape[1]
    if nb < 4:
        return np.zeros(0), np.zeros(0)
    idx = np.arange(0, nb - 3, 1 if overlap else 4)
    z = (e[:, idx] + e[:, idx + 1] + e[:, idx + 2] + e[:, idx + 3]) / (4.0 * sub)
    l = z.sum(axis=0)
    return l, lufs_of(l) + (0.0 if offset else 0.691)


def integrated(e, sub, rel_gate=True, abs_gate=True, overlap=True, offset=True):
    """I in f64 from sub-block energies [channels, nb]; -inf where nothing passes"""
    l, L = block_loudness(e, sub, overlap, offset)
    keep = L > -70.0 if abs_gate else np.ones(l.size, bool)
    if not keep.any():
        return -np.inf
    off = 0.0 if offset else 0.691
    if rel_gate:
        gamma = lufs_of(l[keep].mean()) + off - 10.0
        keep = keep & (L > gamma)
        if not keep.any():
            return -np.inf
    return float(lufs_of(l[keep].mean()) + off)


def loudness(rows, rate, shelf=True, highpass=True, reset=False, tail=False, **gate):
    """I of rows [channels, n] at `rate` (mutant `tail`: the partial tail counted as one more sub-block)"""
    rows = np.atleast_2d(np.asarray(rows, np.float64))
    sub = sub_frames(rate)
    if tail and rows.shape[1] % sub:
        rows = np.concatenate([rows, np.zeros((rows.shape[0], sub - rows.shape[1] % sub))], axis=1)
    return integrated(sub_energies(rows, rate, shelf, highpass, reset), sub, **gate)


def gate_margin(rows, rate):
    """the smallest distance in LU of a block's loudness from the absolute gate and from the relative one"""
    sub = sub_frames(rate)
    l, L = block_loudness(sub_energies(rows, rate), sub)
    keep = L > -70.0
    d = np.abs(L + 70.0).min() if L.size else np.inf
    if keep.any():
        gamma = lufs_of(l[keep].mean()) - 10.0
        d = min(d, np.abs(L - gamma).min())
    return float(d)


# ---- true peak ---------------------------------------------------------------------------------------------------------------
def fma_f32(a, b, c):
    """fmaf(a, b, c), correctly rounded, on float32 arrays: the product is exact in f64; the f64 sum is rounded to odd (the
    error of the addition, recovered exactly, decides), which makes the second rounding to f32 the only one that counts"""
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
    toward = np.where(err > 0.0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    with np.errstate(over="ignore", invalid="ignore"):
        return s.astype(np.float32)


def table_1_4():
    """rc_resample_table(1, 4): float32 [4, 64], the engine's own table"""
    from rocoder_amd import _lib

    t = np.zeros(4 * 64, np.float32)
    ph, tp = C.c_uint32(0), C.c_uint32(0)
    rc = _lib.lib().rc_resample_table(1, 4, t.ctypes.data_as(C.POINTER(C.c_float)), t.size, C.byref(ph), C.byref(tp))
    assert rc == 0 and (ph.value, tp.value) == (4, 64)
    return t.reshape(4, 64)


def oversampled(rows, table, zero_extend=True):
    """u[c][m], m < 4 n, float32: the fmaf chain with j ascending (mutant: y held at its end values outside [0, n))"""
    rows = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
    ch, n = rows.shape
    if n == 0:
        return np.zeros((ch, 0), np.float32)
    pad = np.zeros((ch, n + 63), np.float32)
    pad[:, 31:31 + n] = rows
    if not zero_extend:
        pad[:, :31] = rows[:, :1]
        pad[:, 31 + n:] = rows[:, -1:]
    u = np.zeros((ch, n, 4), np.float32)
    for p in range(4):
        acc = np.zeros((ch, n), np.float32)
        for j in range(64):  # x[q - 31 + j] is pad[q + j]
            acc = fma_f32(np.broadcast_to(table[p, j], acc.shape), pad[:, j:j + n], acc)
        u[:, :, p] = acc
    return u.reshape(ch, 4 * n)


def finite_peak(v):
    a = np.abs(np.asarray(v, np.float32)).reshape(-1)
    a = a[np.isfinite(a)]
    return np.float32(a.max()) if a.size else np.float32(0.0)


def true_peak(rows, table, zero_extend=True, sample_peak=True):
    """tp as np.float32 (mutants: y not zero-extended, the sample peak left out)"""
    rows = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
    tp = finite_peak(oversampled(rows, table, zero_extend))
    return max(tp, finite_peak(rows)) if sample_peak else tp


def gain_of(lufs, tp, target_lufs, max_true_peak):
    """g as np.float32 from the REPORTED float32 loudness and true peak"""
    lufs, tp, max_true_peak = np.float32(lufs), np.float32(tp), np.float32(max_true_peak)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        gl = np.float32(1.0) if np.isinf(lufs) else np.float32(np.power(np.float64(10.0), (np.float64(np.float32(target_lufs)) - np.float64(lufs)) / 20.0))
        gc = np.float32(max_true_peak / tp) if max_true_peak > 0 and tp > 0 else np.float32(np.inf)
    g = min(gl, gc)
    return g if np.isfinite(g) and g > 0 else np.float32(1.0)


# ---- the inputs the kernel tests use (R = 8000: sub = 800) ----------------------------------------------------------------------
def test_input(kind, channels, n, rate=8000, seed=1):
    """float32 [channels, n]: 'white' noise; a 30 Hz 'tone'; 'dc' 1.0 with noise at 1e-3; a 'burst' after 2 s of exact zeros"""
    rng = np.random.default_rng(seed + 1000 * channels + n)
    t = np.arange(n, dtype=np.float64)[None, :]
    if kind == "white":
        x = 0.25 * rng.standard_normal((channels, n))
    elif kind == "tone":
        x = 0.5 * np.sin(2.0 * np.pi * 30.0 * t / rate + np.arange(channels)[:, None])
    elif kind == "dc":
        x = 1.0 + 1e-3 * rng.standard_normal((channels, n))
    else:
        assert kind == "burst"
        x = 0.3 * rng.standard_normal((channels, n))
        x[:, :2 * rate] = 0.0
    return x.astype(np.float32)


def programme(channels, rate=8000, scale=1.0, seed=5, tail=True):
    """float32 [channels, n], a programme on which every rule of the gate decides something: 3 s of near-silence (-80 dBFS,
    below the absolute gate), 1.5 s of noise 14 LU below the loud passage (out by the relative gate, in without the absolute
    one), 2 s of noise at 0.25 rms, and - `tail` - 799 louder frames that fill no sub-block. `scale` shortens the sections."""
    rng = np.random.default_rng(seed)
    parts = []
    for secs, amp in ((3.0, 1e-4), (1.5, 0.25 * 10.0 ** (-14.0 / 20.0)), (2.0, 0.25)):
        parts.append(amp * rng.standard_normal((channels, int(round(secs * scale * rate)))))
    if tail:
        parts.append(1.0 * rng.standard_normal((channels, sub_frames(rate) - 1)))
    return np.concatenate(parts, axis=1).astype(np.float32)


def energy_errors(got, want, sub):
    """(the largest relative error over the sub-blocks whose own loudness is above -70, the largest absolute error over the
    others as a fraction of the energy of -70 LUFS): both are held below GATE_REL"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    floor = ABS_GATE_ENERGY * sub
    loud = want > floor
    rel = float((np.abs(got - want)[loud] / want[loud]).max()) if loud.any() else 0.0
    quiet = float(np.abs(got - want)[~loud].max() / floor) if (~loud).any() else 0.0
    return rel, quiet


# ---- the launchers on the GPU, through the test hooks (librocoder_hip_hooks.so) ------------------------------------------------
GUARD_FLOATS = 8


def _hook(name, argtypes, restype=C.c_int):
    import frameskernelutil as K

    fn = getattr(K.hooks(), name)
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


def loud_span(channels, nb):
    return int(_hook("rc_test_frames_loud_span", [C.c_uint32, C.c_uint64], C.c_uint32)(channels, nb))


def _planar(rows, pad, base):
    """rows at floats base + c * (n + pad) of a guard-filled device block"""
    import frameskernelutil as K

    ch, n = rows.shape
    stride = max(n, 1) + pad
    host, _ = K.planar_host(rows, stride, base)
    return K.DevBuf(host), stride


def gpu_energies(rows, rate, pad=0, base=0, launches=1):
    """launch_frames_loud_energy on rows [channels, n] -> (float32 [launches, channels, nb], True where every guard word
    around the energy rows is unchanged). e_stride = nb + 3."""
    import frameskernelutil as K

    rows = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
    ch, n = rows.shape
    sub = sub_frames(rate)
    nb = n // sub
    fn = _hook("rc_test_frames_kweight_energy", [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                  C.c_void_p, C.c_uint64])
    src, stride = _planar(rows, pad, base)
    assert 4 * (base + (ch - 1) * stride + n) <= src.nbytes
    e_stride = nb + 3
    out, ok = [], True
    for _ in range(launches):
        host = np.full(GUARD_FLOATS + ch * e_stride + GUARD_FLOATS, K.GUARD_WORD, np.uint32)
        dst = K.DevBuf(host)
        assert 4 * (GUARD_FLOATS + (ch - 1) * e_stride + nb) <= dst.nbytes - 4 * GUARD_FLOATS
        K._done("rc_test_frames_kweight_energy", fn(src.ptr(4 * base), stride, n, ch, rate, sub, nb, dst.ptr(4 * GUARD_FLOATS), e_stride))
        got = dst.read().view(np.uint32)
        e = np.empty((ch, nb), np.float32)
        for c in range(ch):
            row = got[GUARD_FLOATS + c * e_stride:GUARD_FLOATS + c * e_stride + nb]
            e[c] = row.view(np.float32)
            row[:] = K.GUARD_WORD
        ok = ok and bool((got == K.GUARD_WORD).all())
        out.append(e)
    return np.stack(out), ok


def gpu_true_peak(rows, table, pad=0, base=0, table_dev=None):
    """launch_frames_true_peak on rows [channels, n] over zeroed words -> (tp as np.float32, the gain word's bits: untouched)"""
    import frameskernelutil as K

    rows = np.ascontiguousarray(np.atleast_2d(rows), np.float32)
    ch, n = rows.shape
    fn = _hook("rc_test_frames_true_peak", [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p])
    src, stride = _planar(rows, pad, base)
    assert 4 * (base + (ch - 1) * stride + n) <= src.nbytes
    tab = table_dev if table_dev is not None else K.DevBuf(np.ascontiguousarray(table, np.float32))
    assert tab.nbytes == 4 * 256
    words = K.DevBuf(np.array([0, K.GUARD_WORD], np.uint32))
    K._done("rc_test_frames_true_peak", fn(src.ptr(4 * base), stride, n, ch, tab.ptr(), words.ptr()))
    w = words.read().view(np.uint32)
    return w[:1].view(np.float32)[0], int(w[1])

"""The phase modes of include/rocoder_hip_phase.h stated in numpy float64 and Python integers: the sequential definition,
hop after hop, written from the header and not from the C - the yardstick of tests/test_phase_host.py and of the GPU
tests. Also here: the ctypes prototypes of the test-hook entries rc_test_phase_* (rc_phase_hooks.hip) and the cases the
host test admits for the GPU parity test."""
import ctypes as C

import numpy as np

from oracle import oracle_np as onp

RANDOM, PROPAGATE, LOCKED = 0, 1, 2
MASK = (1 << 32) - 1
TOL = 1.0e-4          # the project's gate: relative RMS against the twin
PERTURB = 2.0 ** -22  # the spectra's perturbation of the conditioning check ...
PERTURB_TOL = 1.0e-5  # ... and what it may move the output: a tenth of the gate


# ------------------------------------------------------------------------------------------------ the definition, per hop
def turns(X):
    """a[j] = llrint(atan2(im, re) / (2 pi) * 2^32) mod 2^32 of bins 0 ... H, as int64"""
    X = np.asarray(X, np.complex128)
    return np.rint(np.arctan2(X.imag, X.real) / (2.0 * np.pi) * 2.0 ** 32).astype(np.int64) & MASK


def increments(a_prev, a, N, step):
    """e_k[j] of bins 0 ... H from the two hops' turns"""
    H = N // 2
    j = np.arange(H + 1, dtype=np.int64)
    expect = ((j * step) % N) * ((1 << 32) // N)
    dev = (a - a_prev - expect) & MASK
    dev = dev - ((dev >> 31) << 32)  # the principal argument: int32
    d = ((j & 1) << 31) + (dev * H) // step  # (numpy's // floors)
    return (a_prev - a + d) & MASK


def peaks(m2):
    """bins 1 ... H - 1 strictly greater than both neighbours at distance 1 and 2; neighbours outside 0 ... H do not count"""
    m2 = np.asarray(m2, np.float64)
    H = m2.size - 1
    out = []
    for j in range(1, H):
        ok = m2[j] > m2[j - 1] and m2[j] > m2[j + 1]
        if ok and j - 2 >= 0:
            ok = m2[j] > m2[j - 2]
        if ok and j + 2 <= H:
            ok = m2[j] > m2[j + 2]
        if ok:
            out.append(j)
    return np.array(out, np.int64)


def owners(m2, locked):
    """P(j): j itself (PROPAGATE, or a hop without a peak), else the nearest peak, the lower one on a tie"""
    n = np.asarray(m2).size
    j = np.arange(n, dtype=np.int64)
    pk = peaks(m2) if locked else np.zeros(0, np.int64)
    if pk.size == 0:
        return j
    hi = np.searchsorted(pk, j, side="left")           # the first peak >= j
    lo = np.searchsorted(pk, j, side="right") - 1      # the last peak <= j
    below = np.where(lo >= 0, pk[np.maximum(lo, 0)], -1)
    above = np.where(hi < pk.size, pk[np.minimum(hi, pk.size - 1)], -1)
    own = np.where(below < 0, above, np.where(above < 0, below, np.where(j - below <= above - j, below, above)))
    return own.astype(np.int64)


def prep(X_prev, X, N, step, locked):
    """(P, e) of a hop from its spectrum and the one before it (bins 0 ... H); X_prev None: hop 0, the identity"""
    H = N // 2
    if X_prev is None:
        return np.arange(H + 1, dtype=np.int64), np.zeros(H + 1, np.int64)
    X = np.asarray(X, np.complex128)[:H + 1]
    e = increments(turns(np.asarray(X_prev)[:H + 1]), turns(X), N, step)
    return owners(X.real ** 2 + X.imag ** 2, locked), e


def advance(theta, P, e):
    """theta_k[j] = theta_{k-1}[P(j)] + e[P(j)]"""
    return (theta[P] + e[P]) & MASK


def scan_sequential(P, e, theta0):
    """[hops, H + 1] rows of P and e, the state in front of the first hop -> theta of every hop"""
    theta = np.asarray(theta0, np.int64) & MASK
    out = np.empty(np.asarray(P).shape, np.int64)
    for k in range(out.shape[0]):
        theta = advance(theta, np.asarray(P[k], np.int64), np.asarray(e[k], np.int64))
        out[k] = theta
    return out


def rotate(X, theta, N):
    """the N bins of Z: X cis(theta) for j <= H, the conjugates above"""
    H = N // 2
    Zh = np.asarray(X, np.complex128)[:H + 1] * np.exp(2j * np.pi * (np.asarray(theta, np.float64) / 2.0 ** 32))
    return np.concatenate([Zh, np.conj(Zh[1:H][::-1])])


def envelope(w):
    """env_c[i] = 1 / (w[i]^2 + w[i + H]^2) in float64 from the float32 window"""
    w = np.asarray(w, np.float32).astype(np.float64)
    H = w.size // 2
    return 1.0 / (w[:H] ** 2 + w[H:] ** 2)


# ------------------------------------------------------------------------------------------------ a whole channel
def stretch_channel(x, N, factor, pitch, mode, amplitude=1.0, window=None, perturb=None, rng=None):
    """One channel through the reference's loop (Stretcher::next_window as oracle_np.stretch_channel_literal walks it:
    hops at k * step, the input zero-padded once it runs out, windows of S samples resampled by the pitch multiple) with
    the coherent resynthesis in place of the random one. perturb = (kind, size), the conditioning check: every hop's
    spectrum gets complex Gaussian noise, "bin": of that size relative to each bin, X (1 + size g); "floor": of that size
    relative to the RMS magnitude of the hop's bins, X + size rms(|X|) g - the shape of an f32 transform's rounding, which
    does not shrink with the bin."""
    assert mode in (PROPAGATE, LOCKED)
    d = onp.derive(N, factor, amplitude, pitch)
    H, S, step, p = d["H"], d["S"], d["step"], d["p"]
    w = (onp.hanning(N) if window is None else np.asarray(window, np.float32)).astype(np.float64)
    env = envelope(w.astype(np.float32))
    inp = np.asarray(x, np.float64).copy()
    out_buf = np.zeros(H)
    theta = np.zeros(H + 1, np.int64)
    X_prev = None
    done = False
    chunks = []
    while not done:
        pos = 0
        while out_buf.size < S + H:
            if inp.size < N:
                inp = np.concatenate([inp, np.zeros(N - inp.size)])
                done = True
            X = np.fft.fft(inp[:N] * w)[:H + 1]
            if perturb:
                kind, size = perturb
                g = (rng.standard_normal(H + 1) + 1j * rng.standard_normal(H + 1)) / np.sqrt(2.0)
                X = X * (1.0 + size * g) if kind == "bin" else X + size * np.sqrt(np.mean(np.abs(X) ** 2)) * g
            P, e = prep(X_prev, X, N, step, mode == LOCKED)
            theta = advance(theta, P, e)
            y = np.fft.irfft(rotate(X, theta, N)[:H + 1], N) * w
            X_prev = X
            out_buf[pos:pos + H] = (y[:H] + out_buf[pos:pos + H]) * env * amplitude
            out_buf = np.concatenate([out_buf, y[H:]])
            pos += H
            inp = inp[step:]
        chunks.append(onp.resample(out_buf[:S], p))
        out_buf = out_buf[-H:]
    return np.concatenate(chunks)


def stretch(x, N, factor, pitch, mode, amplitude=1.0, window=None, perturb=None, seed=0):
    x = np.atleast_2d(x)
    return np.stack([stretch_channel(x[c], N, factor, pitch, mode, amplitude, window, perturb,
                                     np.random.default_rng([seed, c]) if perturb else None) for c in range(x.shape[0])])


def rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-300))


# ------------------------------------------------------------------------------------------------ inputs and cases
def tones(c, L, N, partials=((37.3, 0.4), (83.6, 0.25), (151.2, 0.15))):
    """a sum of sinusoids that are not bin-centred, more than 4 bins apart (the frequencies are in bins of an N-point
    transform); every channel its own phases and a slight detune"""
    t = np.arange(L, dtype=np.float64)
    x = np.zeros(L)
    for i, (b, a) in enumerate(partials):
        x += a * np.sin(2.0 * np.pi * (b * (1.0 + 0.013 * c)) / N * t + 0.7 * i + 1.3 * c)
    return x.astype(np.float32)


def tones_input(ch, L, N, partials=None):
    return np.stack([tones(c, L, N, *(() if partials is None else (partials,))) for c in range(ch)])


def small_partials(N):
    """three partials for a short window: the same rule (not bin-centred, more than 4 bins apart) inside N / 2 bins"""
    return ((2.3 * N / 32, 0.4), (7.6 * N / 32, 0.25), (12.7 * N / 32, 0.15))


# The GPU parity cases (tests/test_gpu_phase.py), admitted by tests/test_phase_host.py's conditioning check under both
# kinds of perturbation: PROPAGATE at factors with H % step == 0 only, LOCKED at any factor, tonal input. The caller's
# asymmetric window goes with PROPAGATE: its side lobes are peaks of their own, pairs of them tie within the "floor"
# noise, and LOCKED then moves by 3e-4. (N, factor, pitch, mode, window name or None)
PARITY_CASES = [
    (32, 2.0, 1, PROPAGATE, None),
    (32, 3.0, 1, LOCKED, None),
    (512, 2.0, 1, PROPAGATE, None),
    (512, 3.0, 1, LOCKED, None),
    (1024, 8.0, 1, LOCKED, None),
    (1024, 2.0, 2, PROPAGATE, None),
    (1024, 1.5, 2, LOCKED, None),
    (1024, 6.0, -2, LOCKED, None),
    (1024, 2.0, 1, PROPAGATE, "skew"),
    (16384, 8.0, 1, PROPAGATE, None),
    (16384, 1.5, 1, LOCKED, None),
]


def case_input(N, ch=2):
    """The stereo tonal input of a parity case: 12 windows long (8 from N = 4096 on), raised-cosine fades of two windows at both ends and half
    a window of zeros behind. Without the fades the last hops see the input cut off: a broadband spectrum in bins that
    held nothing but rounding noise one hop earlier, and the phase of such a bin, which e_k reads, is not a property of
    the signal (the f64 twin and an f32 transform disagree about it at any tolerance)."""
    L = (12 if N < 4096 else 8) * N
    x = tones_input(ch, L, N, small_partials(N) if N < 256 else None).astype(np.float64)
    g = np.ones(L)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(2 * N) + 0.5) / (2 * N))
    g[:2 * N] = ramp
    g[L - 2 * N - N // 2:L - N // 2] = ramp[::-1]
    g[L - N // 2:] = 0.0
    return (x * g).astype(np.float32)


def case_window(N, name):
    if name is None:
        return None
    import windowutil

    return windowutil.WINDOWS[name](N)


# ------------------------------------------------------------------------------------------------ the test-hook entries
_u32, _i64, _p = C.c_uint32, C.c_int64, C.c_void_p
PROTOTYPES = {
    "rc_test_phase_prep": (C.c_int, [_p, _p, _u32, _u32, _u32, _u32, _u32, _i64]),
    "rc_test_phase_scan": (C.c_int, [_p, _p, _p, _u32, _u32, _u32, _i64]),
    "rc_test_phase_apply": (C.c_int, [_p, _p, _p, _p, _u32, _u32, _u32, _u32, _i64]),
    "rc_test_phase_scan_block": (C.c_uint32, [_i64]),
    "rc_test_phase_chunk_hops": (C.c_int, [_p, C.c_uint64]),
}
_handle = None


def hooks():
    """the test-hook library with the prototypes of the phase entries set"""
    global _handle
    if _handle is None:
        from rocoder_amd import _lib

        with _lib.hooks_library() as H:
            for name, (res, args) in PROTOTYPES.items():
                fn = getattr(H, name)
                fn.restype = res
                fn.argtypes = args
            _handle = H
    return _handle


def done(name, rc):
    """Every call of these tests is a valid one, so a launcher that reports an error has met a device error. Nothing more
    is launched on a device in that state: the session ends there."""
    if rc != 0:
        import pytest

        pytest.exit(f"{name}: hipError_t {rc}; no further launches on this device", returncode=3)
    return rc

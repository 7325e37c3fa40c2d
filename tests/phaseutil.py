"""The phase modes of include/rocoder_hip_phase.h stated in numpy float64 and Python integers: the sequential definition,
hop after hop, written from the header and not from the C - the yardstick of tests/test_phase_host.py and of the GPU
tests. Also here: the ctypes prototypes of the test-hook entries rc_test_phase_* (rc_phase_hooks.hip, rc_engine.cpp), the
cases the host test admits for the GPU parity test, and the replay: the stage verifiers S1 ... S5, the staged twin and its
mutants, the replay cases and the host side of rc_test_phase_tap (tests/test_gpu_phase_replay.py)."""
import collections
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


def deviation(a_prev, a, N, step):
    """dev_k[j]: the principal argument (int32) of the turn's advance beyond the bin's own frequency"""
    j = np.arange(N // 2 + 1, dtype=np.int64)
    expect = ((j * step) % N) * ((1 << 32) // N)
    dev = (a - a_prev - expect) & MASK
    return dev - ((dev >> 31) << 32)


def increments(a_prev, a, N, step, odd_term=True, floor=True):
    """e_k[j] of bins 0 ... H from the two hops' turns (odd_term, floor: the mutants of tests/test_phase_host.py)"""
    H = N // 2
    j = np.arange(H + 1, dtype=np.int64)
    dev = deviation(a_prev, a, N, step)
    q = (dev * H) // step if floor else np.sign(dev) * ((np.abs(dev) * H) // step)  # (numpy's // floors)
    d = (((j & 1) << 31) if odd_term else 0) + q
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
    return owners_of_peaks(peaks(m2) if locked else np.zeros(0, np.int64), np.asarray(m2).size)


def owners_of_peaks(pk, n, upper_on_tie=False):
    """P(j) of n bins from the sorted peak indices (upper_on_tie: the mutant of tests/test_phase_host.py)"""
    j = np.arange(n, dtype=np.int64)
    pk = np.asarray(pk, np.int64)
    if pk.size == 0:
        return j
    hi = np.searchsorted(pk, j, side="left")           # the first peak >= j
    lo = np.searchsorted(pk, j, side="right") - 1      # the last peak <= j
    below = np.where(lo >= 0, pk[np.maximum(lo, 0)], -1)
    above = np.where(hi < pk.size, pk[np.minimum(hi, pk.size - 1)], -1)
    nearer = (j - below < above - j) if upper_on_tie else (j - below <= above - j)
    own = np.where(below < 0, above, np.where(above < 0, below, np.where(nearer, below, above)))
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
    # engine; spec, qs, base, z, y, chunks each with its capacity in elements; the chunk count
    "rc_test_phase_tap": (C.c_int, [_p, _p, C.c_size_t, _p, C.c_size_t, _p, C.c_size_t, _p, C.c_size_t, _p, C.c_size_t, _p, C.c_size_t, _p]),
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


# ------------------------------------------------------------------------------------------------ replay: the stages
# The rows a phase-mode job holds between its launches, each checked in float64 against the stage in front of it AS THE GPU
# LEFT IT ("Replay"). Every stage is then a continuous, or exactly integer, function of rows held bit for bit:
# the discontinuities of the definition no longer accumulate from hop to hop, and any input is admissible.
#   X      [ch, hops, N] complex64   the analysis spectra
#   theta  [ch, hops, H + 1] int64   the rotation of every bin, base[Q[j]] + s[j]
#   Z      [ch, hops, N] complex64   the rotated spectra
#   y      [ch, hops, N] float32     the windowed inverse transforms
#   out    [ch, n_out] float32       the job's output
Rows = collections.namedtuple("Rows", "X theta Z y out")

REG_TOL = 2.0e-6       # the project's regression gate (tests/test_gpu_parity.py): S1, S4, S5, relative RMS
BLOCK_TOL = 5.0e-6     # ... and its bound per block (assert_blocks), S5 on blocks of H
TURN_BOUND = 1 << 10   # a[j] of phase_prep against float64, in units of 2^-32 turn (tests/test_gpu_phase_kernels.py)
ROT_TOL = 2.0 ** -22   # the rotation, of the bin's magnitude (test_apply there)
TINY_M2 = 1.0e-30      # a bin below this and not exactly zero has no phase to speak of
EXCUSED_CAP = 1.0e-3   # of a case's bins: a condition on the inputs, not a measurement
MUTANTS = ("upper_on_tie", "no_odd_term", "truncate", "halo_ignored", "minus_theta", "no_conjugate", "plain_envelope", "channel0_theta")
OWNER_OF_MUTANT = {"upper_on_tie": "S2", "no_odd_term": "S2", "truncate": "S2", "halo_ignored": "S2", "minus_theta": "S3",
                   "no_conjugate": "S3", "plain_envelope": "S5", "channel0_theta": "S2"}


class StageError(AssertionError):
    """a verifier's finding; .stage names the stage, and with it the kernel"""

    def __init__(self, stage, text):
        super().__init__(f"{stage}: {text}")
        self.stage = stage


def _need(cond, stage, text):
    if not cond:
        raise StageError(stage, text() if callable(text) else text)


def geometry(N, f, p, L):
    """the job's step, hops per channel and samples per window (Stretcher::new and the loop of stretch_channel)"""
    d = onp.derive(N, f, 1.0, p)
    step, hpw = d["step"], (2 * p if p >= 1 else 1)
    assert step >= 1
    kd = (L - N) // step + 1 if L >= N else 0
    return dict(H=d["H"], S=d["S"], step=step, hpw=hpw, hops=hpw * (kd // hpw + 1))


def frames(x, N, step, hops):
    """[ch, hops, N] float64: the zero-padded input at k * step"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    n = (hops - 1) * step + N
    xp = np.zeros((x.shape[0], n))
    m = min(n, x.shape[1])
    xp[:, :m] = x[:, :m]
    return xp[:, np.arange(hops)[:, None] * step + np.arange(N)[None, :]]


def window_of(N, window):
    return onp.hanning(N) if window is None else np.asarray(window, np.float32)


def m2_f32(X, how):
    """re^2 + im^2 of complex64 bins as float32 arithmetic gives it: "unfused" rounds both products, "fma_re" / "fma_im"
    round one product and fuse the other into the sum (a product of two float32 is exact in float64)"""
    re, im = np.asarray(X.real, np.float64), np.asarray(X.imag, np.float64)
    rr, ii = re * re, im * im
    if how == "unfused":
        return rr.astype(np.float32) + ii.astype(np.float32)
    if how == "fma_re":
        return (rr + ii.astype(np.float32)).astype(np.float32)
    assert how == "fma_im"
    return (ii + rr.astype(np.float32)).astype(np.float32)


def peak_flags(m2):
    """peaks() on every row of [..., H + 1] at once: bool of the same shape"""
    m2 = np.asarray(m2)
    nb = m2.shape[-1]
    H = nb - 1
    c = m2[..., 1:H]
    ok = (c > m2[..., 0:H - 1]) & (c > m2[..., 2:H + 1])
    ok[..., 1:] &= c[..., 1:] > m2[..., 0:H - 2]    # bins 2 ... H - 1 against j - 2
    ok[..., :-1] &= c[..., :-1] > m2[..., 3:H + 1]  # bins 1 ... H - 2 against j + 2
    flags = np.zeros(m2.shape, bool)
    flags[..., 1:H] = ok
    return flags


def overlap_add_rows(y, N, p, S, env, amplitude):
    """one channel's [hops, N] rows through the reference's loop, as stretch_channel walks it"""
    H = N // 2
    out_buf = np.zeros(H)
    chunks, k = [], 0
    while k < y.shape[0]:
        pos = 0
        while out_buf.size < S + H:
            out_buf[pos:pos + H] = (y[k, :H] + out_buf[pos:pos + H]) * env * amplitude
            out_buf = np.concatenate([out_buf, y[k, H:]])
            pos += H
            k += 1
        chunks.append(onp.resample(out_buf[:S], p))
        out_buf = out_buf[-H:]
    return np.concatenate(chunks)


def _signed(d):
    d = d & MASK
    return d - ((d >> 31) << 32)


# ---- S1
def verify_analysis(x, X, N, step, window=None):
    """every X row against fft(w * x_hop) of the zero-padded input at k * step: relative RMS per (channel, hop) over all N
    bins - the upper half of the float64 transform is the conjugates - within REG_TOL; a hop of zeros exactly zero"""
    ch, hops, _ = X.shape
    w = window_of(N, window).astype(np.float64)
    ref = np.fft.fft(frames(x, N, step, hops) * w, axis=-1)
    err = np.sqrt(np.mean(np.abs(X - ref) ** 2, axis=-1))
    mag = np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1))
    zero = mag == 0
    _need(not X[zero].any(), "S1", "a hop of zeros has a spectrum that is not exactly zero")
    rel = np.where(zero, 0.0, err / np.where(zero, 1.0, mag))
    worst = float(rel.max()) if rel.size else 0.0
    _need(worst <= REG_TOL, "S1", lambda: f"analysis relative RMS {worst:.3e} > {REG_TOL:.1e} at (channel, hop) {np.unravel_index(rel.argmax(), rel.shape)}")
    H = N // 2
    herm = np.abs(X[..., N - 1:H:-1] - np.conj(X[..., 1:H])).max(initial=0.0)
    return dict(worst=worst, hermitian=float(herm))


# ---- S2
def lattice_ok(d_obs, a_prev, a, N, step):
    """Exact in integers: is the observed advance theta_k[j] - theta_(k-1)[j] a value the definition gives for SOME pair of
    turns whose difference lies within 2 TURN_BOUND of a - a_prev? With D = a1 - a0 and v = int32(D - expect):
    H % step == 0: e = D (r - 1) - expect r + odd, r = H / step: the residual is a multiple of r - 1;
    else: e + D - odd = floor(v H / step), that is floor(v (H - step) / step) = e + expect - odd, which has an integer
    solution v within the bound or has none - a truncated quotient, one unit up at negative v, has none where H / step - 1
    exceeds 1. Returns bool per bin, or None where |H / step - 1| < 0.2 and the search below would be too narrow."""
    H = N // 2
    j = np.arange(H + 1, dtype=np.int64)
    expect = ((j * step) % N) * ((1 << 32) // N)
    odd = (j & 1) << 31
    D = (a - a_prev) & MASK
    slack = 2 * TURN_BOUND
    if H % step == 0:
        r = H // step
        resid = _signed(d_obs - odd + expect * r - D * (r - 1))
        if r == 1:
            return resid == 0
        return (resid % (r - 1) == 0) & (np.abs(resid) <= slack * (r - 1))
    c = H - step
    if 5 * abs(c) < step:
        return None
    v_twin = _signed(D - expect)
    g0 = (v_twin * c) // step
    t = g0 + _signed(d_obs + expect - odd - g0)
    v0 = np.rint(t.astype(np.float64) * step / c).astype(np.int64)
    found = np.zeros(t.shape, bool)
    for dv in range(-6, 7):
        v = v0 + dv
        found |= ((v * c) // step == t) & (np.abs(v - v_twin) <= slack)
    return found


def verify_theta(X, theta, N, step, locked, what=""):
    """theta of every hop against the hop in front of it, both as given: (theta_k[j] - theta_(k-1)[P(j)]) mod 2^32 within
    2^11 (1 + H / step) + 2 units of e[P(j)] from the turns of the X bits, and on the lattice of lattice_ok. Exact: hop 0
    has theta 0, the bins of one owner share one theta. Excused, by the inputs alone: an owner that differs among the
    three float32 evaluations of m2, dev within 2^11 of half a turn where H % step != 0 (unless both bins lie on the real
    axis, where the turns are exact), 0 < |X|^2 < TINY_M2."""
    ch, hops, _ = X.shape
    H = N // 2
    nb = H + 1
    bound = (1 << 11) * (1.0 + H / step) + 2
    ident = np.arange(nb, dtype=np.int64)
    _need(not theta[:, 0].any(), "S2", "hop 0 has a theta that is not 0")
    Xh = X[:, :, :nb]
    a = turns(Xh)
    m2 = np.asarray(Xh.real, np.float64) ** 2 + np.asarray(Xh.imag, np.float64) ** 2
    tiny = (m2 < TINY_M2) & (m2 != 0)
    on_axis = Xh.imag == 0
    whole = H % step == 0
    worst, excused, off_lattice_checked = 0.0, 0, 0
    for c in range(ch):
        if locked:
            fl = [peak_flags(m2_f32(Xh[c], how)) for how in ("unfused", "fma_re", "fma_im")]
            same = (fl[0] == fl[1]).all(axis=-1) & (fl[0] == fl[2]).all(axis=-1)
        for k in range(1, hops):
            P, amb = ident, np.zeros(nb, bool)
            if locked:
                P = owners_of_peaks(np.flatnonzero(fl[0][k]), nb)
                if not same[k]:
                    for f in fl[1:]:
                        amb |= owners_of_peaks(np.flatnonzero(f[k]), nb) != P
            dev = deviation(a[c, k - 1], a[c, k], N, step)
            e = increments(a[c, k - 1], a[c, k], N, step)
            # (a bin on the real axis, zero included, has the same turn here and on the GPU - 0 or exactly half a turn,
            # which test_prep_turns_are_within_the_bound... asserts - so two such bins have the same dev, wherever it lies:
            # bins 0 and H of every hop, and every bin of a silent hop)
            near_half = np.zeros(nb, bool) if whole else (np.abs(dev) >= (1 << 31) - (1 << 11)) & ~(on_axis[c, k] & on_axis[c, k - 1])
            excuse = amb | (tiny[c, k] | tiny[c, k - 1] | near_half)[P]
            excused += int(excuse.sum())
            adv = (theta[c, k] - theta[c, k - 1][P]) & MASK
            d = np.abs(_signed(adv - e[P]))
            bad = (d > bound) & ~excuse
            _need(not bad.any(), "S2", lambda: f"{what} channel {c} hop {k}: theta is {int(d[bad].max())} units from the increment (bound {bound:.0f}) "
                                                f"at bins {np.flatnonzero(bad)[:6]} of {int(bad.sum())}")
            worst = max(worst, float(d[~excuse].max(initial=0)))
            share = (theta[c, k] != theta[c, k][P]) & ~amb
            _need(not share.any(), "S2", lambda: f"{what} channel {c} hop {k}: bins {np.flatnonzero(share)[:6]} do not share their owner's theta")
            on = None if locked else lattice_ok(adv, a[c, k - 1], a[c, k], N, step)
            if locked:  # the owners' own advance: bins that own themselves
                own = P == ident
                full = lattice_ok((theta[c, k] - theta[c, k - 1]) & MASK, a[c, k - 1], a[c, k], N, step)
                on = None if full is None else full | ~own
            if on is not None:
                off = ~on & ~excuse
                _need(not off.any(), "S2", lambda: f"{what} channel {c} hop {k}: the advance at bins {np.flatnonzero(off)[:6]} of {int(off.sum())} is no "
                                                    f"value the definition gives for turns within the bound")
                off_lattice_checked += int((~excuse).sum())
    bins = ch * max(hops - 1, 0) * nb
    return dict(worst=worst, bound=bound, excused=excused, bins=bins, share=excused / bins if bins else 0.0, lattice_bins=off_lattice_checked)


# ---- S3
def verify_rotation(X, theta, Z, N):
    """Z[j] against X[j] cis(theta[j]) within ROT_TOL of |X[j]|; theta == 0 gives the bits of X; exact conjugates above H"""
    H = N // 2
    nb = H + 1
    Xh = np.ascontiguousarray(X[..., :nb])
    Zh = np.ascontiguousarray(Z[..., :nb])
    still = theta == 0
    _need((Zh.view(np.uint64)[still] == Xh.view(np.uint64)[still]).all(), "S3", "a rotation of zero did not pass the bits through")
    want = Xh.astype(np.complex128) * np.exp(2j * np.pi * (theta.astype(np.float64) / 2.0 ** 32))
    err, mag = np.abs(Zh - want), np.abs(Xh.astype(np.complex128))
    bad = err > ROT_TOL * mag
    rel = np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), 0.0)
    worst = float(rel.max(initial=0.0))
    _need(not bad.any(), "S3", lambda: f"rotation error {worst:.3e} of the magnitude > 2^-22 at (channel, hop, bin) {np.argwhere(bad)[:3].tolist()}")
    up = np.ascontiguousarray(Z[..., N - 1:H:-1])  # bins N - 1 ... H + 1: the partners of bins 1 ... H - 1
    lo = np.ascontiguousarray(Z[..., 1:H])
    conj = (np.ascontiguousarray(up.real).view(np.uint32) == np.ascontiguousarray(lo.real).view(np.uint32)).all() and \
           (np.ascontiguousarray(up.imag).view(np.uint32) == np.ascontiguousarray(-lo.imag).view(np.uint32)).all()
    _need(conj, "S3", "the bins above H are not the exact conjugates")
    return dict(worst=worst)


# ---- S4
def oracle_synthesis_figure(Zrow, w32):
    """The S4 figure of one hop with the C oracle's float32 transform in the kernel's place: the folded spectrum
    Zs = A + i B, A even and B odd, through two of the oracle's real forward transforms (a window of ones),
    y = (Re fft(A) + Im fft(B)) / N, times the window in float32 - against the same float64 row."""
    from oracle import cbind as oc

    N = Zrow.size
    Z = Zrow.astype(np.complex128)
    Zs = 0.5 * (Z + np.conj(np.roll(Z[::-1], 1)))
    fft = oc.ReFFT(np.ones(N, np.float32))
    FA, FB = fft.forward_fft(Zs.real.astype(np.float32)), fft.forward_fft(Zs.imag.astype(np.float32))
    y32 = ((FA.real + FB.imag) / np.float32(N)).astype(np.float32) * np.asarray(w32, np.float32)
    return rel_rms(y32, np.fft.ifft(Z).real * np.asarray(w32, np.float64))


def verify_synthesis(Z, y, N, window=None):
    """every y row against the float64 inverse transform of the Z row as given, folded Zs[j] = (Z[j] + conj Z[N - j]) / 2
    as rc_phase.h states - the real part of ifft(Z), at hop_kernel's scale 1 / N - times the window: relative RMS per hop
    within REG_TOL. The figure is relative to the WINDOWED row while a float32 transform's error is relative to the row in
    front of the window: a hop whose output sits where the window vanishes (the last samples of a burst at the start of a
    frame: 1.5 % of the RMS survives the window) lies above the gate by construction. Such a hop is held to 4 times the
    same figure of the C oracle's float32 transform on the same row (oracle_synthesis_figure; 4 for hop_kernel's longer
    float32 chain), and both numbers are reported."""
    w32 = window_of(N, window)
    w = w32.astype(np.float64)
    ref = np.fft.ifft(Z.astype(np.complex128), axis=-1).real * w
    err = np.sqrt(np.mean((y - ref) ** 2, axis=-1))
    mag = np.sqrt(np.mean(ref ** 2, axis=-1))
    zero = mag == 0
    _need(not y[zero].any(), "S4", "a spectrum of zeros gave samples that are not exactly zero")
    rel = np.where(zero, 0.0, err / np.where(zero, 1.0, mag))
    lifted = []
    for c, k in np.argwhere(rel > REG_TOL).tolist():
        fig = oracle_synthesis_figure(Z[c, k], w32)
        _need(rel[c, k] <= 4.0 * fig, "S4", f"synthesis relative RMS {rel[c, k]:.3e} > {REG_TOL:.1e} at (channel, hop) {(c, k)}, where the C oracle's "
                                             f"float32 transform has {fig:.3e}")
        lifted.append((c, k, float(rel[c, k]), fig))
        rel[c, k] = 0.0
    return dict(worst=float(rel.max(initial=0.0)), lifted=lifted)


# ---- S5
def verify_overlap_add(y, out, N, p, S, window=None, amplitude=1.0, plain_envelope=False):
    """the job's output against the float64 overlap-add of the y rows as given, with the coherent envelope, the amplitude
    and the pitch's resampler: relative RMS per channel within REG_TOL, every block of H within BLOCK_TOL of the
    channel's RMS (assert_blocks of tests/test_gpu_parity.py); a channel of zeros exactly zero"""
    H = N // 2
    env = onp.hanning_crossfade_compensation(H).astype(np.float64) if plain_envelope else envelope(window_of(N, window))
    amp = float(np.float32(amplitude))
    ref = np.stack([overlap_add_rows(y[c].astype(np.float64), N, p, S, env, amp) for c in range(y.shape[0])])
    _need(ref.shape == out.shape, "S5", lambda: f"the output has shape {out.shape}, the overlap-add of its rows {ref.shape}")
    worst = worst_block = 0.0
    for c in range(ref.shape[0]):
        r = np.sqrt(np.mean(ref[c] ** 2)) if ref.shape[1] else 0.0
        if r == 0:
            _need(not out[c].any(), "S5", f"channel {c} of zeros is not exactly zero")
            continue
        d = out[c] - ref[c]
        worst = max(worst, float(np.sqrt(np.mean(d ** 2)) / r))
        nblk = d.size // H
        if nblk:
            worst_block = max(worst_block, float(np.sqrt((d[:nblk * H].reshape(nblk, H) ** 2).mean(axis=-1)).max() / r))
    _need(worst <= REG_TOL, "S5", lambda: f"overlap-add relative RMS {worst:.3e} > {REG_TOL:.1e}")
    _need(worst_block <= BLOCK_TOL, "S5", lambda: f"overlap-add: a block of H is {worst_block:.3e} of the channel's RMS > {BLOCK_TOL:.1e}")
    return dict(worst=worst, worst_block=worst_block)


def verify(rows, x, N, f, p, mode, window=None, amplitude=1.0, what="", stages=("S1", "S2", "S3", "S4", "S5")):
    """all five stages of a job's rows; prints the worst figure of each and returns them. Raises StageError."""
    x = np.atleast_2d(x)
    g = geometry(N, f, p, x.shape[1])
    assert rows.X.shape[1] == g["hops"], (rows.X.shape, g)
    fig = {}
    if "S1" in stages:
        fig["S1"] = verify_analysis(x, rows.X, N, g["step"], window)
    if "S2" in stages:
        fig["S2"] = verify_theta(rows.X, rows.theta, N, g["step"], mode == LOCKED, what)
    if "S3" in stages:
        fig["S3"] = verify_rotation(rows.X, rows.theta, rows.Z, N)
    if "S4" in stages:
        fig["S4"] = verify_synthesis(rows.Z, rows.y, N, window)
    if "S5" in stages:
        fig["S5"] = verify_overlap_add(rows.y, rows.out, N, p, g["S"], window, amplitude)
    s2 = fig.get("S2")
    if s2:
        _need(s2["share"] <= EXCUSED_CAP, "S2", lambda: f"{what}: {s2['excused']} of {s2['bins']} bins are excused, more than {EXCUSED_CAP:.1%}: the input is not admissible")
    print(f"REPLAY {what}: " + " ".join(
        f"{k} {v['worst']:.3e}" + (f" of {v['bound']:.0f} units, excused {v['share']:.2e}, lattice {v['lattice_bins']}" if k == "S2" else "")
        + (f" block {v['worst_block']:.3e}" if k == "S5" else "")
        + ("".join(f" [hop {lk} of channel {lc}: {lr:.3e}, the C oracle's float32 transform {lo:.3e}]" for lc, lk, lr, lo in v["lifted"]) if k == "S4" else "")
        for k, v in fig.items()))
    return fig


# ---- the twin, stage by stage, every stage from the float32 rows of the one before
def replay_twin(x, N, f, p, mode, window=None, amplitude=1.0, mutant=None, chunk=None):
    """Rows of the definition with every stage rounded to float32 before the next one reads it - what the verifiers must
    pass - or, with `mutant`, of one of the MUTANTS, which the stage that owns it must catch. m2 is the "unfused" float32
    evaluation. chunk: hops per chunk of the "halo_ignored" mutant."""
    assert mutant is None or mutant in MUTANTS
    x = np.atleast_2d(np.asarray(x, np.float32))
    ch = x.shape[0]
    g = geometry(N, f, p, x.shape[1])
    H, step, hops = g["H"], g["step"], g["hops"]
    nb = H + 1
    w32 = window_of(N, window)
    w = w32.astype(np.float64)
    X = np.fft.fft(frames(x, N, step, hops) * w, axis=-1).astype(np.complex64)
    Xh = X[:, :, :nb]
    a = turns(Xh)
    theta = np.zeros((ch, hops, nb), np.int64)
    ident = np.arange(nb, dtype=np.int64)
    for c in range(ch):
        flags = peak_flags(m2_f32(Xh[c], "unfused")) if mode == LOCKED else None
        for k in range(1, hops):
            e = increments(a[c, k - 1], a[c, k], N, step, odd_term=mutant != "no_odd_term", floor=mutant != "truncate")
            if mutant == "halo_ignored" and k % chunk == 0:
                e = np.zeros(nb, np.int64)
            P = ident if flags is None else owners_of_peaks(np.flatnonzero(flags[k]), nb, upper_on_tie=mutant == "upper_on_tie")
            theta[c, k] = advance(theta[c, k - 1], P, e)
    if mutant == "channel0_theta":
        theta[1:] = theta[0]
    rot = (-theta if mutant == "minus_theta" else theta).astype(np.float64) / 2.0 ** 32
    Zh = Xh.astype(np.complex128) * np.exp(2j * np.pi * rot)
    upper = Zh[..., 1:H][..., ::-1]
    Z = np.concatenate([Zh, upper if mutant == "no_conjugate" else np.conj(upper)], axis=-1).astype(np.complex64)
    y = (np.fft.ifft(Z.astype(np.complex128), axis=-1).real * w).astype(np.float32)
    env = onp.hanning_crossfade_compensation(H).astype(np.float64) if mutant == "plain_envelope" else envelope(w32)
    amp = float(np.float32(amplitude))
    out = np.stack([overlap_add_rows(y[c].astype(np.float64), N, p, g["S"], env, amp) for c in range(ch)]).astype(np.float32)
    return Rows(X, theta, Z, y, out)


# ---- the replay cases (tests/test_gpu_phase_replay.py; tests/test_phase_host.py holds the verifiers to them first)
ReplayCase = collections.namedtuple("ReplayCase", "group N f p mode ch L signal window")


def replay_id(c):
    return "%s-N%d-f%g-p%d-%s-ch%d-L%d-%s-%s" % (c.group, c.N, c.f, c.p, ("", "propagate", "locked")[c.mode], c.ch, c.L, c.signal, c.window)


def replay_input(c):
    """[ch, L] float32 of the case"""
    N, L, ch = c.N, c.L, c.ch
    import windowutil

    if c.signal == "parity":
        return case_input(N, ch)
    if c.signal == "white":
        return windowutil.white_input(ch, L)
    if c.signal == "white+tones":
        return (0.5 * windowutil.white_input(ch, L) + tones_input(ch, L, N, small_partials(N) if N < 256 else None)).astype(np.float32)
    if c.signal in ("white_full", "white_1e-6"):
        x = np.stack([np.random.default_rng(2000 + i).uniform(-1.0, 1.0, L) for i in range(ch)])
        return (x * (1.0 if c.signal == "white_full" else 1.0e-6)).astype(np.float32)
    if c.signal == "dc":
        return np.full((ch, L), 0.5, np.float32)
    x = np.zeros((ch, L), np.float32)
    if c.signal == "click":  # one sample, channel 0; the other channel is silent
        x[0, 3 * N + 5] = 0.75
    elif c.signal == "comb":  # two clicks a third of a window apart; another spacing and level in the other channel
        x[0, [3 * N + 5, 3 * N + 6 + N // 3]] = 0.75, 0.5
        x[-1, [2 * N + 1, 2 * N + 2 + N // 5]] = -0.6, 0.3
    else:
        assert c.signal == "bursts"  # two bursts of white with exact silence in front, between and behind
        wn = windowutil.white_input(ch, L)
        for lo, hi in ((N, 3 * N), (5 * N, 7 * N + 3)):
            x[:, lo:hi] = wn[:, lo:hi]
    return x


def _replay_cases():
    out = []
    sizes = [1 << n for n in range(5, 15)]
    # every window length under both modes; white for all, the tones on top for half; every factor and pitch
    fp = [(2.0, 1), (1.5, 1), (3.0, 2), (0.75, 1), (5.0, 1), (8.0, 1), (3.0, -2), (2.0, 3), (5.0, -3), (1.5, 2)]
    for i, N in enumerate(sizes):
        for m, mode in enumerate((PROPAGATE, LOCKED)):
            f, p = fp[(i + 3 * m) % len(fp)]
            L = (6 + (0 if N == 16384 else (i + m) % 7)) * N + 17
            out.append(ReplayCase("window", N, f, p, mode, 2, L, "white" if (i + m) % 2 else "white+tones", None))
    # every factor under both modes, the pitches in turn
    for i, f in enumerate((0.75, 1.5, 2.0, 3.0, 5.0, 8.0)):
        for m, mode in enumerate((PROPAGATE, LOCKED)):
            out.append(ReplayCase("factor", 1024, f, (1, 2, 3, -2, -3)[(i + 2 * m) % 5], mode, 2, 8 * 1024 + 5, "white", None))
    # channel counts: hop slots left empty, theta at ch_first (H + 1)
    for N in (64, 256):
        for i, ch in enumerate((1, 2, 3, 5)):
            out.append(ReplayCase("channels", N, 3.0, 1, (PROPAGATE, LOCKED)[(i + (N == 256)) % 2], ch, 8 * N + 3, "white+tones", None))
    out.append(ReplayCase("channels", 4096, 2.0, 1, LOCKED, 3, 6 * 4096 + 1, "white", None))
    # a caller's asymmetric windows
    for N, f in ((256, 2.0), (4096, 1.5)):
        for name in ("skew", "ramp"):
            for mode in (PROPAGATE, LOCKED):
                out.append(ReplayCase("caller", N, f, 1, mode, 2, 7 * N + 9, "white", name))
    # signal classes; clicks tie in 40 % of their bins, so they go with PROPAGATE only; DC at a factor with
    # H % step == 0, where its steady dev of exactly half a turn at bin H is no ambiguity
    for N, f in ((128, 1.5), (2048, 5.0)):
        for sig in ("click", "comb"):
            out.append(ReplayCase("class", N, f, 1, PROPAGATE, 2, 8 * N, sig, None))
        for sig in ("bursts", "dc", "white_full", "white_1e-6"):
            for mode in (PROPAGATE, LOCKED):
                out.append(ReplayCase("class", N, 2.0 if sig == "dc" else f, 1, mode, 2, 10 * N if sig == "bursts" else 8 * N, sig, None))
    # edge lengths
    for N, f in ((256, 2.0), (1024, 1.5)):
        step = onp.derive(N, f, 1.0, 1)["step"]
        for L in (0, 1, N - 1, N, N + 1, 5 * step):
            for mode in (PROPAGATE, LOCKED):
                out.append(ReplayCase("edge", N, f, 1, mode, 2, L, "white", None))
    # the parity cases of PARITY_CASES once more: the two methods meet
    for N, f, p, mode, wname in PARITY_CASES:
        out.append(ReplayCase("parity", N, f, p, mode, 2, case_input(N).shape[1], "parity", wname))
    return out


REPLAY_CASES = _replay_cases()


# ---- the tap (rc_test_phase_tap of the test-hook library)
TAP_COLS = 11  # hop_first, hop_count, block, ch_first, n_channels, halo, then the chunk's first element in spec, qs, base, z, y


class Tap:
    """Host arrays for the rows of one job of `hops` hops per channel cut into chunks of at least `min_chunk` hops"""

    def __init__(self, N, ch, hops, min_chunk):
        nb = N // 2 + 1
        n_chunks = (hops + min_chunk - 1) // min_chunk + 1
        self.N, self.ch, self.hops = N, ch, hops
        self.spec = np.full(ch * (hops + n_chunks) * N * 2, np.nan, np.float32)
        self.qs = np.full(ch * hops * 2 * nb, 0xA5A5A5A5, np.uint32)
        self.base = np.full(ch * (hops // 16 + n_chunks + 1) * nb, 0xA5A5A5A5, np.uint32)
        self.z = np.full(ch * hops * N * 2, np.nan, np.float32)
        self.y = np.full(ch * hops * N, np.nan, np.float32)
        self.chunks = np.full((n_chunks + 1) * TAP_COLS, -1, np.int64)
        self.count = np.zeros(1, np.uint64)

    def set(self, eng, caps=None):
        arrs = (self.spec, self.qs, self.base, self.z, self.y, self.chunks)
        caps = caps or [a.size for a in arrs[:5]] + [self.chunks.size // TAP_COLS]
        args = []
        for a, cap in zip(arrs, caps):
            args += [a.ctypes.data, cap]
        return hooks().rc_test_phase_tap(eng._h, *args, self.count.ctypes.data)

    @staticmethod
    def clear(eng):
        return hooks().rc_test_phase_tap(eng._h, *([None, 0] * 6), None)

    def table(self):
        return self.chunks[:int(self.count[0]) * TAP_COLS].reshape(-1, TAP_COLS)

    def rows(self, out):
        """place every chunk's rows by absolute hop: Rows; every (channel, hop) exactly once, and a chunk's halo hop is,
        bit for bit, the row the chunk in front of it analysed"""
        N, ch, hops = self.N, self.ch, self.hops
        nb = N // 2 + 1
        X = np.zeros((ch, hops, N), np.complex64)
        Z = np.zeros((ch, hops, N), np.complex64)
        y = np.zeros((ch, hops, N), np.float32)
        theta = np.zeros((ch, hops, nb), np.int64)
        seen = np.zeros((ch, hops), np.int64)
        for k0, kc, B, c0, nc, halo, o_spec, o_qs, o_base, o_z, o_y in self.table().tolist():
            assert 0 <= k0 and k0 + kc <= hops and c0 + nc <= ch and halo == (1 if k0 else 0) and B >= 1, (k0, kc, B, c0, nc, halo)
            blocks = (kc + B - 1) // B
            sp = self.spec[o_spec:o_spec + nc * (kc + halo) * N * 2].view(np.complex64).reshape(nc, kc + halo, N)
            if halo:
                assert (seen[c0:c0 + nc, k0 - 1] == 1).all()
                assert sp[:, 0].tobytes() == X[c0:c0 + nc, k0 - 1].tobytes(), f"the halo hop of the chunk at hop {k0} is not the hop the chunk before it analysed"
            X[c0:c0 + nc, k0:k0 + kc] = sp[:, halo:]
            Z[c0:c0 + nc, k0:k0 + kc] = self.z[o_z:o_z + nc * kc * N * 2].view(np.complex64).reshape(nc, kc, N)
            y[c0:c0 + nc, k0:k0 + kc] = self.y[o_y:o_y + nc * kc * N].reshape(nc, kc, N)
            qs = self.qs[o_qs:o_qs + nc * kc * 2 * nb].reshape(nc, kc, 2, nb).astype(np.int64)
            base = self.base[o_base:o_base + nc * blocks * nb].reshape(nc, blocks, nb).astype(np.int64)
            assert qs[:, :, 0].max() < nb
            blk = np.arange(kc) // B
            for c in range(nc):
                theta[c0 + c, k0:k0 + kc] = (np.take_along_axis(base[c][blk], qs[c, :, 0], axis=1) + qs[c, :, 1]) & MASK
            seen[c0:c0 + nc, k0:k0 + kc] += 1
        assert (seen == 1).all(), "the tap's chunks do not cover every (channel, hop) exactly once"
        return Rows(X, theta, Z, y, np.asarray(out))

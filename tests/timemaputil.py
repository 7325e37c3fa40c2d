"""Time maps in numpy and plain Python, for tests/test_time_map_host.py and tests/test_gpu_time_map.py (the definitions are in
include/rocoder_hip_timemap.h): `curve` is the twin of rc_time_map_curve in IEEE doubles, `gather` the rows V of a map,
`expected_map_job` the whole job from the oracle's own pieces. No device, no engine library."""
import math

import numpy as np

from oracle import oracle_np as onp


def hops_per_window(N: int, p: int) -> int:
    d = onp.derive(N, 1.0, 1.0, p)
    tail = N - N // 2
    return (d["S"] + tail - 1) // tail


def curve(N: int, p: int, in_len: int, at, factor):
    """rc_time_map_curve, operation for operation: Python floats are IEEE doubles and every line is one operation."""
    at = [float(a) for a in at]
    factor = [float(f) for f in factor]
    n = len(at)
    abs_p = float(abs(p))
    hpw = hops_per_window(N, p)

    def f_of(q):
        if q <= at[0]:
            return factor[0]
        if q >= at[n - 1]:
            return factor[n - 1]
        i = 0
        while i + 2 < n and at[i + 1] <= q:
            i += 1
        df = factor[i + 1] - factor[i]
        dq = q - at[i]
        da = at[i + 1] - at[i]
        t = dq / da
        m = df * t
        return factor[i] + m

    pos, q, K = [], 0.0, None
    while K is None or len(pos) < K:
        k = len(pos)
        here = int(math.floor(q))
        if K is None and here + N > in_len:
            K = hpw * (k // hpw + 1)
        pos.append(here)
        fq = f_of(q)
        psf = fq / abs_p if p < 0 else fq * abs_p
        den = 2.0 * psf
        step = float(N) / den
        q = q + step
    return np.array(pos[:K], np.int64)


def gather(x, pos, N: int, mutant: str = None) -> np.ndarray:
    """V[c, k * N + n] = x[c, pos[k] + n] inside the input, 0 elsewhere. `mutant` names a wrong gather (the tests prove that
    the definition of a map job tells each of them from the right one)."""
    x = np.atleast_2d(np.asarray(x))
    C, L = x.shape
    pos = [int(v) for v in pos]
    K = len(pos)
    V = np.zeros((C, K * N), x.dtype)
    for c in range(C):
        src = x[0] if mutant == "channel0" else x[c]
        for k in range(K):
            p = pos[K - 1 - k] if mutant == "reversed" else pos[k]
            if mutant == "off_by_one":
                p += 1
            j = p + np.arange(N)
            if mutant == "clamp":
                row = src[np.clip(j, 0, L - 1)] if L else np.zeros(N, x.dtype)
            else:
                ok = (j >= 0) & (j < L)
                row = np.zeros(N, x.dtype)
                row[ok] = src[j[ok]]
            if mutant == "drop_last":
                row[N - 1] = 0
            V[c, k * N:(k + 1) * N] = row
    return V


MUTANTS = ("off_by_one", "clamp", "reversed", "drop_last", "channel0")


def expected_map_job(x, pos, N: int, factor: float, amplitude: float, p: int, seed: int, window=None, mutant: str = None,
                     kernel=None) -> np.ndarray:
    """The definition of a map job in f64, [channels, K / hpw * window_out_len]: on the gathered windows
    O[k H + i] = (y_k[i] + y_{k-1}[H + i]) * env[i] * amp with y_k = resynth(V[k N : (k + 1) N], window, phase_key(seed, c, k)),
    y_{-1} = 0; then every window's S samples through the pitch resample (src/stretcher.rs:91-121)."""
    d = onp.derive(N, factor, amplitude, p)
    H, S, amp = d["H"], d["S"], float(d["amp"])
    hpw = hops_per_window(N, p)
    K = len(pos)
    assert K % hpw == 0
    w = onp.hanning(N) if window is None else np.asarray(window, np.float32)
    env = onp.hanning_crossfade_compensation(H).astype(np.float64)
    V = gather(np.asarray(x, np.float64), pos, N, mutant)
    rows = []
    for c in range(V.shape[0]):
        O = np.zeros(K * H)
        tail = np.zeros(H)
        for k in range(K):
            y = onp.resynth(V[c, k * N:(k + 1) * N], w, onp.phase_key(seed, c, k), kernel)
            O[k * H:(k + 1) * H] = (y[:H] + tail) * env * amp
            tail = y[H:]
        wins = [onp.resample(O[i * hpw * H:i * hpw * H + S], p) for i in range(K // hpw)]
        rows.append(np.concatenate(wins) if wins else np.zeros(0))
    return np.stack(rows)

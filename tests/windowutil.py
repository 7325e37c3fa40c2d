"""Helpers of the asymmetric-window parity tests (tests/test_window_parity_host.py, tests/test_gpu_window_parity.py):
caller windows that are not mirror-symmetric and do not vanish at the ends, white input, the oracle driven with a
caller's window, and the gates of tests/test_gpu_parity.py plus a per-frequency-band one. No GPU, no product import."""
import numpy as np

from conftest import rms
from oracle import cbind as oc
from oracle import oracle_np as onp

TOL = 1.0e-4        # the contract (tests/test_gpu_parity.py)
REG_TOL = 2.0e-6    # its regression gate
BLOCK_TOL = 5.0e-6  # its per-block bound
BAND_TOL = 5.0e-6


# ------------------------------------------------------------------ windows (f32 tables, built in f64)
def skew(N):
    """0.15 + 0.85 sin^2(pi ((n + 0.5) / N)^0.6): asymmetric (peak left of the centre), 0.15 .. 0.2 at both ends"""
    n = np.arange(N, dtype=np.float64)
    return (0.15 + 0.85 * np.sin(np.pi * ((n + 0.5) / N) ** 0.6) ** 2).astype(np.float32)


def ramp(N):
    """(n + 1) / N: the maximum is the LAST sample of the frame"""
    return ((np.arange(N, dtype=np.float64) + 1.0) / N).astype(np.float32)


def ramp_down(N):
    """ramp mirrored: the maximum is the FIRST sample of the frame"""
    return ramp(N)[::-1].copy()


def hann_but_last(N):
    """the default window with one sample changed, the last: w[N-1] = 0.5"""
    w = oc.hanning(N).copy()
    w[N - 1] = np.float32(0.5)
    return w


WINDOWS = {"skew": skew, "ramp": ramp, "ramp_down": ramp_down, "hann_but_last": hann_but_last}


# ------------------------------------------------------------------ input and references
def white(c, L):
    """white noise, uniform in +-0.9: every bin carries the same energy, so every bin weighs the same in an RMS"""
    return np.random.default_rng(1000 + c).uniform(-0.9, 0.9, L).astype(np.float32)


def white_input(ch, L):
    return np.stack([white(c, L) for c in range(ch)]) if ch else np.zeros((0, L), np.float32)


def oracle_with_window(x, N, f, p, w, seed, kernel=None):
    """[C, L] -> [C, n_out] of the reference path with the caller's window `w`: the C oracle (f32, one Stretcher per
    channel) for powers of two up to 65536, the f64 twin for every other length (the C oracle's transform there is the
    O(N^2) sum: 2.5 s at N = 1000, unusable at 24000) and above 65536."""
    x = np.atleast_2d(x)
    ch = x.shape[0]
    w = np.ascontiguousarray(w, np.float32)
    assert w.size == N
    chans = []
    for c in range(ch):
        if N & (N - 1) == 0 and N <= 65536:
            st = oc.Stretcher(channels=ch, factor=f, pitch_multiple=p, window=w, seed=seed, channel_index=c, kernel=kernel)
            st.send(x[c])
            st.close_input()
            wins = []
            while not st.is_done():
                wins.append(st.next_window())
            chans.append(np.concatenate(wins).astype(np.float64))
        else:
            chans.append(onp.stretch_channel_literal(x[c], N, f, 1.0, p, seed, c, kernel=kernel, window=w))
    return np.stack(chans)


# ------------------------------------------------------------------ gates
def assert_parity(got, ref, what="", reg=REG_TOL):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = rms(got - ref)
    r = rms(ref)
    assert err <= TOL and err <= TOL * r + 1e-9, f"{what}: rms_err={err:.3e} rms_ref={r:.3e}"  # the contract
    assert err <= reg * r + 1e-9, f"{what}: REGRESSION rms_err={err:.3e} = {err / max(r, 1e-30):.2e} of rms_ref"
    return err


def assert_blocks(got, ref, block, what="", bound=BLOCK_TOL):
    """No isolated bad stretch (one seam block, one run) hides inside a good global RMS: every block of `block`
    samples of every channel is within `bound` of the channel's RMS."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    nb = got.shape[-1] // block
    d = (got[..., :nb * block] - ref[..., :nb * block]).reshape(got.shape[:-1] + (nb, block))
    blk = np.sqrt((d * d).mean(axis=-1))
    scale = np.sqrt((ref * ref).mean(axis=-1, keepdims=True))
    worst = float((blk / scale).max())
    assert worst <= bound, (what, worst, np.unravel_index((blk / scale).argmax(), blk.shape))
    return worst


def band_errors(got, ref, nb=8):
    """[..., nb]: sqrt(sum |E|^2 / sum |R|^2) over each of nb equal bands of the rfft of every whole channel"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    E = np.abs(np.fft.rfft(got - ref, axis=-1)) ** 2
    R = np.abs(np.fft.rfft(ref, axis=-1)) ** 2
    m = E.shape[-1]
    edges = [i * m // nb for i in range(nb + 1)]
    e = np.stack([E[..., a:b].sum(axis=-1) for a, b in zip(edges[:-1], edges[1:])], axis=-1)
    r = np.stack([R[..., a:b].sum(axis=-1) for a, b in zip(edges[:-1], edges[1:])], axis=-1)
    return np.sqrt(e / np.maximum(r, 1e-300))


def assert_bands(got, ref, what="", nb=8, bound=BAND_TOL):
    """No band of the spectrum hides a bad error inside a good global RMS. Pitch 1 only: decimation folds the bands."""
    b = band_errors(got, ref, nb)
    worst = float(b.max())
    assert worst <= bound, (what, worst, np.unravel_index(b.argmax(), b.shape))
    return worst


def rel_err(got, ref):
    return rms(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / max(rms(ref), 1e-30)

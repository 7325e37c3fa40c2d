"""GPU parity tests (-m gpu) on the signals the dense-input tests do not have, through every kernel path with the
DEFAULT window (tests/signalutil.py: CASES): white input under the per-block and per-band gates; clicks, where the output
must be EXACTLY zero wherever no hop holding a click contributes; DC and Nyquist input, which put the energy into the
two bins every pair stage special-cases; and white input scaled by 2^-30 and 2^30, where the output must scale bit for bit.

tests/test_signal_classes_host.py shows on the CPU that the reference side satisfies all of this and which kernel errors
it catches that synth_input and white input at one level let through ("Parity on clicks, silence, DC, Nyquist
and scaled input")."""
import numpy as np
import pytest

import signalutil as su
import windowutil as wu
from test_gpu_window_parity import _check, _engine_mod, _half_window, _reg
from windowutil import REG_TOL

pytestmark = pytest.mark.gpu

_white = {}  # case -> the engine's output on white input: the parity test and the scaling test share it


def _run(ra, c, x):
    with ra.Engine(window_len=c.N, factor=c.f, pitch_multiple=c.p, channels=c.ch, seed=su.SEED, **su.engine_kwargs(c)) as e:
        return e.stretch_host(x)


def _white_output(ra, c):
    if c not in _white:
        _white[c] = _run(ra, c, su.make_input(c, "white"))
        _white[c].setflags(write=False)
    return _white[c]


def _assert_silent(got, mask, H, p, what):
    """exactly zero (-0.0 counts) outside the support; names the first sample that is not"""
    leak = su.first_leak(got, mask, H, p)
    if leak is not None:
        out = np.asarray(got)[~mask]
        raise AssertionError(f"{what}: nonzero outside the clicks' support, first at hop {leak[0]} offset {leak[1]}; "
                             f"{np.count_nonzero(out)} samples, largest {np.abs(out).max():.3e}")


# ------------------------------------------------------------------ white input, default window
@pytest.mark.parametrize("c", su.CASES, ids=su.case_id)
def test_default_window_on_white_input(c):
    """The instantiations that compute windows::hanning in registers (hop4, hopw* without a table, hop_kernel<HANN>,
    big5s / big5 HANN) and the chirp-z and long paths with the engine's own table, under the three gates of
    tests/test_gpu_window_parity.py: until now they met the oracle on synth_input alone."""
    ra = _engine_mod()
    _check(_white_output(ra, c), su.reference(c, "white"), c.N, c.f, c.p, su.case_id(c))


# ------------------------------------------------------------------ clicks
@pytest.mark.parametrize("c", su.CASES, ids=su.case_id)
def test_clicks_are_silent_outside_their_hops(c):
    """Zero frame -> zero spectrum -> sqrt(0) = 0 -> zero times a phasor, on every path: a sample outside the support that
    is not zero came from a neighbour's hop, run, channel or LDS region, or from behind the frame."""
    ra = _engine_mod()
    step, H, n_out = su.geometry(c)
    got = _run(ra, c, su.make_input(c, "clicks"))
    ref = su.reference(c, "clicks")
    mask = su.case_mask(c)
    assert got.shape == ref.shape == (c.ch, n_out)
    assert not got[1:].any(), f"a silent channel is not silent: {np.count_nonzero(got[1:])} samples"
    _assert_silent(got[0], mask, H, c.p, su.case_id(c))
    print(f"\nFIGURES clicks {su.case_id(c)}: rel {wu.rel_err(got[0], ref[0]):.2e} silent {1.0 - mask.mean():.2f}")
    wu.assert_parity(got[0], ref[0], su.case_id(c), reg=min(REG_TOL, _reg(c.N, c.f)))


def _boundary_clicks(N, step, L, sizes):
    """click_positions plus the last sample of every push and the first of the next"""
    pos = su.click_positions(N, step, L)
    edge = 0
    for sz in sizes:
        edge += sz
        pos += [edge - 1, edge]
    return sorted(set(pos))


@pytest.mark.parametrize("N,f", [(1024, 4.0), (16384, 8.0)])
def test_streaming_seam_is_silent_outside_the_clicks(N, f):
    """ragged pushes while the channels are open, then the closed rest (test_streaming_seam_with_a_caller_window_...'s
    sizes): the windows handed out are the offline job's bits, and silent outside the clicks' support"""
    ra = _engine_mod()
    L, sizes = 300_000, [50000, 1, 4095, 70000, 333, 40001]
    c = su.Case("stream", N, f, 1, 2, L, None)
    step, H, n_out = su.geometry(c)
    pos = _boundary_clicks(N, step, L, sizes)
    x = su.clicks(2, L, pos)
    mask = su.support_mask(N, step, H, 1, n_out, pos)
    assert 1.0 - mask.mean() >= 0.25
    offline = _run(ra, c, x)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=su.SEED) as e:
        wins = [[], []]

        def take(ch):
            got = e.next_window_view(ch) if (len(wins[ch]) & 1) else e.next_window(ch)
            if got is not None:
                wins[ch].append(np.array(got))
            return got is not None

        at = live = 0
        for sz in sizes:
            for ch in range(2):
                e.push_input(ch, x[ch, at:at + sz])
            at += sz
            while take(0):
                assert take(1)
                live += 1
        assert live > 0 and at < L
        for ch in range(2):
            e.push_input(ch, x[ch, at:])
            e.close_input(ch)
        while not e.is_done(0):
            for ch in range(2):
                assert take(ch)
        assert e.is_done(1)
    got = np.stack([np.concatenate(w) for w in wins])
    assert got.shape == offline.shape == (2, n_out)
    assert not got[1].any()
    _assert_silent(got[0], mask, H, 1, f"streaming N={N}")
    assert np.array_equal(got, offline)


def test_16384_long_job_is_silent_between_clicks_across_run_seams():
    """test_16384_runs_seams_and_ranges_bit_exact's geometry: 2441 hops per channel in runs of several hops, handed from
    workgroup to workgroup through the seam stash. The run length is the engine's own; one click every 37 hops puts the
    17 hops of a click at every offset inside a run for any run length that is no multiple of 37, and leaves 19 silent
    half-windows between two clicks: a stash, a flag or a tail taken from the wrong run is a nonzero sample there."""
    import torch

    ra = _engine_mod()
    N, f, L = 16384, 8.0, 2_500_000
    c = su.Case("16384", N, f, 1, 2, L, None)
    step, H, n_out = su.geometry(c)
    pos = list(range(step // 2 - 1, L - N, 37 * step))
    x = su.clicks(2, L, pos)
    mask = su.support_mask(N, step, H, 1, n_out, pos)
    assert len(pos) > 60 and 0.45 < 1.0 - mask.mean() < 0.6
    with ra.Engine(window_len=N, factor=f, channels=2, seed=su.SEED) as e:
        got = e.stretch_tensor(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (2, n_out)
    assert not got[1].any()
    _assert_silent(got[0], mask, H, 1, "long job")
    alive = (got[0].reshape(-1, H) != 0).any(axis=1)
    assert np.array_equal(alive, mask.reshape(-1, H)[:, 0]), "a half-window inside the support is all-zero"


# ------------------------------------------------------------------ DC and Nyquist
DC_CASES = ([c for c in su.CASES if c.p == 1 and c.spec is None and su.is_pow2(c.N)]
            + [c for c in su.CASES if c.p == 1 and c.N in (3000, 65538)])


@pytest.mark.parametrize("signal", ["dc", "nyquist"])
@pytest.mark.parametrize("c", DC_CASES, ids=su.case_id)
def test_dc_and_nyquist_input(c, signal):
    """All the energy sits in bins 0 and 1 (DC) or M - 1 and M (Nyquist): the `dc` lane of the pair stages, where bin 0
    pairs with itself and M - 0 is bin M. Parity and blocks; the eight bands are empty but one."""
    ra = _engine_mod()
    got = np.asarray(_run(ra, c, su.make_input(c, signal)), np.float64)
    ref = su.reference(c, signal)
    what = f"{signal} {su.case_id(c)}"
    assert got.shape == ref.shape
    block = _half_window(c.N, c.p)
    rel = max(wu.rel_err(got[ch], ref[ch]) for ch in range(c.ch))
    nb = got.shape[-1] // block
    d = (got[..., :nb * block] - ref[..., :nb * block]).reshape(c.ch, nb, block)
    blk = float((np.sqrt((d * d).mean(axis=-1)) / np.sqrt((ref * ref).mean(axis=-1, keepdims=True))).max())
    print(f"\nFIGURES {what}: rel {rel:.2e} block {blk:.2e}")
    for ch in range(c.ch):
        wu.assert_parity(got[ch], ref[ch], f"{what} ch{ch}", reg=min(REG_TOL, _reg(c.N, c.f)))
    wu.assert_blocks(got, ref, block, what)


# ------------------------------------------------------------------ level
@pytest.mark.parametrize("k", [-30, 30])
@pytest.mark.parametrize("c", su.CASES, ids=su.case_id)
def test_power_of_two_scaling_is_exact(c, k):
    """The path is homogeneous of degree 1 and every step of it scales exactly by a power of two: window products, FFT
    passes, v_sqrt_f32 of a value scaled by 4^k, phasors that do not depend on the data, the host kernel's f32 gains.
    An absolute epsilon, clamp, flush or threshold anywhere breaks the equality. No oracle: two GPU runs."""
    ra = _engine_mod()
    base = _white_output(ra, c)
    got = _run(ra, c, su.scaled(su.make_input(c, "white"), k))
    want = su.scaled(base, k)
    assert got.shape == want.shape and np.isfinite(got).all()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        ch, t = (int(v) for v in bad[0])
        raise AssertionError(f"{su.case_id(c)} k={k}: {len(bad)} of {got.size} samples differ, first at channel {ch} "
                             f"sample {t}: {got[ch, t]!r} against {want[ch, t]!r}")

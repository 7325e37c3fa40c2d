"""CPU proof that the asymmetric-window parity checks (tests/windowutil.py, used on the GPU by
tests/test_gpu_window_parity.py) bite, and that the reference side alone sits far inside their gates.

The mutants are the indexing errors a kernel can make when it reads a caller's window table, carries the tail of a frame
or pads the end of a frame - written as variations of oracle_np.resynth / oracle_np.stretch_channel_literal, compared
with the unmutated twin. With the new windows and white input every one of them trips assert_parity; with the window
and the input the older parity tests use (hanning**1.5, synth_input) most of them do not: the blind spot, pinned."""
import numpy as np
import pytest

import windowutil as wu
from oracle import cbind as oc
from oracle import oracle_np as onp


# ------------------------------------------------------------------ the windows
@pytest.mark.parametrize("N", [64, 1000, 16384])
def test_windows_are_asymmetric_bounded_and_alive_at_the_ends(N):
    for name, make in wu.WINDOWS.items():
        w = make(N)
        assert w.dtype == np.float32 and w.shape == (N,)
        assert np.abs(w - w[::-1]).max() > (0.4 if name == "hann_but_last" else 0.1), name
        assert np.abs(w).max() <= 1.0, name
        assert max(abs(w[0]), abs(w[N - 1])) >= 0.1, name  # an end sample of every frame carries weight
    # skew is alive at both ends; a ramp's far end is its maximum and its near end 1 / N; hann_but_last differs from the
    # default window in its last sample alone
    assert min(wu.skew(N)[0], wu.skew(N)[N - 1]) >= 0.1
    assert wu.ramp(N)[N - 1] == 1.0 and wu.ramp(N).argmax() == N - 1 and wu.ramp(N)[0] == np.float32(1.0 / N)
    assert np.array_equal(wu.ramp_down(N), wu.ramp(N)[::-1])
    hb = wu.hann_but_last(N)
    assert hb[0] == 0.0 and hb[N - 1] == np.float32(0.5) and np.array_equal(hb[:-1], oc.hanning(N)[:-1])


def test_white_is_flat_and_seeded():
    x = wu.white(2, 1 << 16)
    assert x.dtype == np.float32 and np.abs(x).max() <= 0.9 and np.array_equal(x, wu.white(2, 1 << 16))
    P = np.abs(np.fft.rfft(x.astype(np.float64))[1:]) ** 2
    bands = P[:32768].reshape(8, -1).sum(axis=1)
    assert bands.max() / bands.min() < 1.2  # (synth_input: one band holds 99 % of the energy)
    s = onp.synth_input(0, 1 << 16).astype(np.float64)
    Ps = (np.abs(np.fft.rfft(s)[1:]) ** 2)[:32768].reshape(8, -1).sum(axis=1)
    assert Ps.max() / Ps.sum() > 0.99


# ------------------------------------------------------------------ the reference side alone: C oracle (f32) against the f64 twin
def _half_window(N, p):
    wout = N if p > 0 else (-(-N // -p) - 1) * -p
    return max(1, wout // 2)


@pytest.mark.parametrize("N", [64, 256, 1024, 4096, 16384])
@pytest.mark.parametrize("name", list(wu.WINDOWS))
def test_c_oracle_equals_f64_twin_on_white_input_with_each_window(name, N):
    """Relative RMS, worst half-window block and worst of 8 bands all <= 1e-6 (measured: <= 3.0e-7), so the reference
    used on the GPU is 7x inside REG_TOL and 17x inside the block and band bounds by itself."""
    w = wu.WINDOWS[name](N)
    for f, p in ((4.0, 1), (2.0, 3), (3.0, -2), (0.3, 1)):
        L = 40 * N if f < 0.5 else 6 * N + 77
        x = wu.white_input(1, L)
        a = wu.oracle_with_window(x, N, f, p, w, seed=5)
        b = onp.stretch_channel_literal(x[0], N, f, 1.0, p, 5, 0, window=w)[None]
        what = f"{name} N={N} f={f} p={p}"
        assert a.shape == b.shape and b.shape[1] >= 2 * N // max(p, 1), what
        wu.assert_parity(a, b, what, reg=1e-6)
        wu.assert_blocks(a, b, _half_window(N, p), what, bound=1e-6)
        if p == 1:
            wu.assert_bands(a, b, what, bound=1e-6)


def test_oracle_with_window_takes_the_twin_off_the_power_of_two_path():
    x = wu.white_input(2, 3000)
    w = wu.skew(250)
    got = wu.oracle_with_window(x, 250, 2.0, 1, w, seed=9)
    for c in range(2):
        assert np.array_equal(got[c], onp.stretch_channel_literal(x[c], 250, 2.0, 1.0, 1, 9, c, window=w))
    # and a power of two gives the C oracle, channel index in the phase key: channels differ, and differ from the twin's bits
    w = wu.skew(256)
    got = wu.oracle_with_window(np.stack([x[0], x[0]]), 256, 2.0, 1, w, seed=9)
    assert wu.rel_err(got[1], got[0]) > 0.5
    tw = onp.stretch_channel_literal(x[0], 256, 2.0, 1.0, 1, 9, 1, window=w)
    assert 0 < wu.rel_err(got[1], tw) < 1e-6


# ------------------------------------------------------------------ mutants
def _resynth(samples, w_an, w_syn, key, drop_last=False):
    """onp.resynth with separate analysis / synthesis windows; drop_last: mutant (f)"""
    n = w_an.size
    X = np.fft.fft(samples[:n].astype(np.float64) * w_an.astype(np.float64))
    theta = onp.phase_theta(key, np.arange(n), n).astype(np.float64)
    y = np.fft.ifft(np.abs(X) * (np.cos(theta) + 1j * np.sin(theta))).real * w_syn.astype(np.float64)
    if drop_last:
        y[n - 1] = 0.0
    return y


def _literal(x, N, f, p, seed, c, w_an, w_syn, tail_shift=0, drop_last=False):
    """onp.stretch_channel_literal's loop; tail_shift = 1 carries y[H+1:] in place of y[H:]: mutant (e)"""
    d = onp.derive(N, f, 1.0, p)
    H, S, step, amp = d["H"], d["S"], d["step"], float(d["amp"])
    env = onp.hanning_crossfade_compensation(H).astype(np.float64)
    inp = np.asarray(x, np.float64).copy()
    out_buf = np.zeros(H)
    done, hop, chunks = False, 0, []
    while not done:
        pos = 0
        while out_buf.size < S + H:
            if inp.size < N:
                inp = np.concatenate([inp, np.zeros(N - inp.size)])
                done = True
            y = _resynth(inp[:N], w_an, w_syn, onp.phase_key(seed, c, hop), drop_last)
            hop += 1
            out_buf[pos:pos + H] = (y[:H] + out_buf[pos:pos + H]) * env * amp
            out_buf = np.concatenate([out_buf, y[H + tail_shift:], np.zeros(tail_shift)])
            pos += H
            inp = inp[step:]
        chunks.append(onp.resample(out_buf[:S], p))
        out_buf = out_buf[-H:]
    return np.concatenate(chunks)


def _mutants(w):
    m = w[::-1].copy()
    sw = w.reshape(-1, 2)[:, ::-1].reshape(-1).copy()
    return {"a_mirrored": dict(w_an=m, w_syn=m), "b_analysis_mirrored": dict(w_an=m, w_syn=w),
            "c_synthesis_mirrored": dict(w_an=w, w_syn=m), "d_pair_lanes_swapped": dict(w_an=sw, w_syn=sw),
            "e_tail_shifted": dict(w_an=w, w_syn=w, tail_shift=1), "f_last_sample_dropped": dict(w_an=w, w_syn=w, drop_last=True)}


MUTANTS = list(_mutants(np.zeros(2, np.float32)))
MN, MF, MSEED = 256, 4.0, 3


def test_unmutated_local_loop_is_the_twin_bit_for_bit():
    for p in (1, 3, -2):
        x = wu.white(0, 5000)
        w = wu.skew(MN)
        assert np.array_equal(_literal(x, MN, MF, p, MSEED, 0, w, w),
                              onp.stretch_channel_literal(x, MN, MF, 1.0, p, MSEED, 0, window=w))


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("name", list(wu.WINDOWS))
def test_every_mutant_trips_the_parity_gate_with_the_new_windows(name, mutant, p):
    x = wu.white(0, 6000)
    w = wu.WINDOWS[name](MN)
    base = _literal(x, MN, MF, p, MSEED, 0, w, w)
    bad = _literal(x, MN, MF, p, MSEED, 0, **_mutants(w)[mutant])
    with pytest.raises(AssertionError):
        wu.assert_parity(bad, base, f"{name} {mutant}")
    # far beyond the gate, not at its edge: the smallest (ramp_down with its last sample, 1 / N, dropped) is 3e-4
    assert wu.rel_err(bad, base) > 50 * wu.REG_TOL, (name, mutant, wu.rel_err(bad, base))


@pytest.mark.parametrize("N", [256, 16384])
def test_the_blind_spot_of_symmetric_windows_and_tonal_input(N):
    """hanning**1.5 (the caller's window of the older parity tests) with synth_input, against `ramp` with white input.

    (a) - (c), every mirrored read of the table, pass assert_parity unnoticed: windows::hanning in f32 is symmetric to
    3.6e-7 (not to the bit: cos of the f32 argument 2 pi i / (n - 1) near 2 pi is not cos near 0), and the outputs move
    by 1e-7 .. 3e-7 of their RMS, a tenth of REG_TOL. So they are not array_equal, as a first reading of the symmetry
    suggests; with the table symmetrised exactly they are, and that is asserted too.
    (d), the swapped pair lanes, is NOT in the blind spot: w[2n] <-> w[2n+1] moves a symmetric window as well (2e-2 of
    the output's RMS at N = 256, 4e-4 at 16384) and the older tests catch it. Pinned as it is.
    (e) moves the output 10x less than with ramp and white input, (f) not at all: the last sample of the frame is 0."""
    h = oc.hanning(N)
    assert 0 < np.abs(h - h[::-1]).max() < 5e-7
    w = (h.astype(np.float64) ** 1.5).astype(np.float32)
    L = 30 * N // 4
    xs, xw = onp.synth_input(0, L), wu.white(0, L)
    base = _literal(xs, N, MF, 1, MSEED, 0, w, w)
    mut = {k: _literal(xs, N, MF, 1, MSEED, 0, **kw) for k, kw in _mutants(w).items()}
    for k in MUTANTS[:3]:
        wu.assert_parity(mut[k], base, k)  # passes: unnoticed
        assert wu.rel_err(mut[k], base) < 5e-7, (k, wu.rel_err(mut[k], base))
    with pytest.raises(AssertionError):
        wu.assert_parity(mut[MUTANTS[3]], base, "pair lanes")
    ws = np.concatenate([w[:N // 2], w[:N // 2][::-1]])  # symmetric to the bit
    bs = _literal(xs, N, MF, 1, MSEED, 0, ws, ws)
    for k in MUTANTS[:3]:
        assert np.array_equal(_literal(xs, N, MF, 1, MSEED, 0, **_mutants(ws)[k]), bs), k
    r = wu.ramp(N)
    br = _literal(xw, N, MF, 1, MSEED, 0, r, r)
    for k, ratio in ((MUTANTS[4], 0.1), (MUTANTS[5], 1e-6)):
        moved_r = wu.rel_err(_literal(xw, N, MF, 1, MSEED, 0, **_mutants(r)[k]), br)
        moved_h = wu.rel_err(mut[k], base)
        print(f"N={N} {k}: hanning**1.5 + synth_input {moved_h:.2e}, ramp + white {moved_r:.2e}")
        assert moved_r > 1e-2 and moved_h <= ratio * moved_r, (k, moved_h, moved_r)


def test_mirrored_window_and_last_sample_move_the_output_as_far_as_the_issue_says():
    """the twin's figures the GPU file leans on: mirroring `skew` moves the output by 0.8 of its RMS; changing only
    w[N-1] of the default window to 0.5 moves it by 7e-3 at N = 16384 (so 1e-3 there separates the two runs safely)"""
    N, L = 16384, 40 * 1024 + 777
    x = wu.white(0, L)
    w = wu.skew(N)
    a = onp.stretch_channel_literal(x, N, 8.0, 1.0, 1, 3, 0, window=w)
    b = onp.stretch_channel_literal(x, N, 8.0, 1.0, 1, 3, 0, window=w[::-1].copy())
    assert 0.6 < wu.rel_err(b, a) < 1.0
    d0 = onp.stretch_channel_literal(x, N, 8.0, 1.0, 1, 3, 0)
    d1 = onp.stretch_channel_literal(x, N, 8.0, 1.0, 1, 3, 0, window=wu.hann_but_last(N))
    assert 5e-3 < wu.rel_err(d1, d0) < 1e-2


# ------------------------------------------------------------------ the band gate
def test_an_error_in_one_band_passes_the_global_gate_and_trips_the_band_gate():
    """A relative error of 1e-5 in one eighth of the bins. On synth_input (99.3 % of the energy in one bin) the global
    relative RMS sees it as 1e-5 * sqrt(the band's share of the energy) = 3e-7 and passes; assert_bands sees 1e-5 in
    that band and raises. (On white input the band holds an eighth of the energy, the global figure is
    1e-5 / sqrt(8) = 3.5e-6 and assert_parity itself raises: white input is what lets the global gate weigh every
    bin - also asserted.)"""
    N, f = 1024, 4.0
    w = wu.skew(N)
    for kind in ("synth", "white"):
        x = onp.synth_input(0, 20000) if kind == "synth" else wu.white(0, 20000)
        got = onp.stretch_channel_literal(x, N, f, 1.0, 1, 7, 0, window=w)
        R = np.fft.rfft(got)
        m = R.size
        for band in (3, 7):
            Rb = R.copy()
            Rb[band * m // 8:(band + 1) * m // 8] *= 1.0 + 1e-5
            ref = np.fft.irfft(Rb, n=got.size)
            b = wu.band_errors(got, ref)
            assert b.argmax() == band and 0.9e-5 < b[band] < 1.1e-5 and np.delete(b, band).max() < 1e-9
            with pytest.raises(AssertionError):
                wu.assert_bands(got, ref, kind)
            if kind == "synth":
                assert wu.assert_parity(got, ref, kind) < 1e-6 * np.sqrt(np.mean(ref * ref))
            else:
                with pytest.raises(AssertionError, match="REGRESSION"):
                    wu.assert_parity(got, ref, kind)
    wu.assert_bands(got, got, "identical")

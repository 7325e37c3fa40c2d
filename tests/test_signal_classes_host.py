"""CPU proof that the signal-class checks (tests/signalutil.py, used on the GPU by tests/test_gpu_signal_classes.py) are
sound on the reference side and catch what the dense-signal parity tests miss.

Sound: the C oracle is exactly zero outside the support of a set of clicks and alive in every hop inside it, it scales
bit for bit with a power of two, and it agrees with the f64 twin on clicks, DC, Nyquist and white input as closely as
on the older inputs. Biting: five mutants of the f64 twin's loop pass assert_parity, assert_blocks and assert_bands on
synth_input and on white input, and each fails exact silence, exact scaling or DC / Nyquist parity."""
import numpy as np
import pytest

import signalutil as su
import windowutil as wu
from oracle import cbind as oc
from oracle import oracle_np as onp

POSITIVE = [c for c in su.CASES if c.p >= 1]
NEGATIVE = [c for c in su.CASES if c.p < 0]
# what the C oracle runs in seconds: powers of two (its transform elsewhere is the O(N^2) sum)
ORACLE_CASES = [c for c in su.CASES if su.is_pow2(c.N) and c.N <= 65536]
SILENCE_CASES = [c for c in POSITIVE if su.is_pow2(c.N) and c.N <= 16384] + [c for c in POSITIVE if c.N == 1000]


# ------------------------------------------------------------------ the inputs
def test_inputs_are_what_they_say():
    x = su.clicks(3, 100, [0, 7, 99])
    assert x.dtype == np.float32 and x.shape == (3, 100)
    assert np.flatnonzero(x[0]).tolist() == [0, 7, 99] and (x[0, [0, 7, 99]] == np.float32(0.75)).all()
    assert not x[1:].any()
    assert (su.dc(2, 9) == np.float32(0.5)).all() and su.dc(2, 9).dtype == np.float32
    ny = su.nyquist(2, 9)
    assert ny.dtype == np.float32 and ny[1].tolist() == [0.5, -0.5] * 4 + [0.5]
    w = wu.white(0, 1000)
    for k in (-30, 30):
        s = su.scaled(w, k)
        assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), w.astype(np.float64) * 2.0 ** k)
        assert np.array_equal(su.scaled(s, -k), w)


def test_level_stays_far_from_overflow_at_the_largest_window():
    """No magnitude of x 2^30 reaches 2^60 at the largest window of CASES: |X[b]| <= sum |x w| <= 0.9 2^30 N. The long
    path's re re + im im of such a value, 2^121, is still finite in f32; and x 2^-30, 8e-10 at most, squares to 7e-19,
    twenty orders above the smallest normal number."""
    N = max(c.N for c in su.CASES)
    assert N == 131072
    top = 0.9 * 2.0 ** 30 * N
    assert top < 2.0 ** 60
    assert np.isfinite(np.float32(top) * np.float32(top) + np.float32(top) * np.float32(top))
    assert np.abs(su.scaled(wu.white(0, 4096), 30)).max() <= np.float32(0.9 * 2.0 ** 30)
    assert float(np.float32(0.9 * 2.0 ** -30)) ** 2 > 1e19 * np.finfo(np.float32).tiny


# ------------------------------------------------------------------ clicks: the support
def test_click_positions_and_support_arithmetic():
    N, step, L = 16384, 1024, su.L16
    pos = su.click_positions(N, step, L)
    k = (L // step) // 3
    assert pos[:4] == [0, k * step - 1, k * step, L - 1] and pos[4] == (k - 3) * step - step // 2
    past, before = pos[5:]
    assert past == (k + 4) * step + N and before % step == step - 1
    # `past` is the first sample behind hop k + 4 and `before` the last one in front of hop m; both hops hold no click
    hops = su.click_hops(N, step, pos)
    m = (before + 1) // step
    assert k + 4 not in hops and m not in hops and k + 5 in hops and m - 1 in hops
    assert su.click_hops(64, 16, [100]) == [3, 4, 5, 6]  # 48 <= 100 < 48 + 64 ... 96 <= 100
    assert su.click_hops(128, 213, [212]) == []          # step > window: between two frames
    # hop 3 .. 6 cover O[3 H, 6 H + N) = blocks 3 .. 7; at pitch 2 output sample t is O[2 t]
    m1 = su.support_mask(64, 16, 32, 1, 320, [100])
    assert np.flatnonzero(m1).tolist() == list(range(96, 256))
    m2 = su.support_mask(64, 16, 32, 2, 160, [100])
    assert np.flatnonzero(m2).tolist() == list(range(48, 128))
    assert su.first_leak(np.zeros(320), m1, 32, 1) is None
    leak = np.zeros(160)
    leak[130] = -1e-30
    assert su.first_leak(leak, m2, 32, 2) == (8, 4)
    assert su.first_leak(np.full(320, -0.0), m1, 32, 1) is None  # -0.0 is silence


@pytest.mark.parametrize("c", su.CASES, ids=su.case_id)
def test_every_case_holds_all_its_clicks(c):
    step, H, n_out = su.geometry(c)
    pos = su.click_positions(c.N, step, c.L)
    assert len(pos) == 6 + (c.N in (16384, 65536)) + (step > c.N) and len(set(pos)) == len(pos), pos
    assert su.clicks(c.ch, c.L, pos)[0].astype(bool).sum() == len(pos)
    if c.p >= 1:  # a condition on the inputs: at least a quarter of the output lies outside the support
        assert su.support_mask(c.N, step, H, c.p, n_out, pos).mean() <= 0.75


@pytest.mark.parametrize("c", SILENCE_CASES, ids=su.case_id)
def test_oracle_is_silent_outside_the_support_and_alive_inside(c):
    """Zero frame -> zero spectrum -> sqrt(0) = 0 -> zero times a phasor: outside the support the oracle's output is
    exactly zero, and so is every channel but the first. Inside, every hop that holds a click on a sample the window does
    not weigh with exactly 0 (windows::hanning: w[0] = 0, so hop 0 of the click at 0 and hop k of the one at k step are
    zero frames) leaves a nonzero sample in both half-windows it adds to: the mask is tight to the half-window."""
    step, H, n_out = su.geometry(c)
    pos = su.click_positions(c.N, step, c.L)
    ref = su.reference(c, "clicks")
    mask = su.case_mask(c)
    assert ref.shape == (c.ch, n_out) and mask.shape == (n_out,)
    assert 1.0 - mask.mean() >= 0.25, 1.0 - mask.mean()
    assert su.first_leak(ref[0], mask, H, c.p) is None
    assert not ref[1:].any()
    w = oc.hanning(c.N)
    blocks = n_out * c.p // H
    alive = np.zeros(blocks, bool)
    np.logical_or.at(alive, np.arange(n_out) * c.p // H, ref[0] != 0)
    checked = 0
    for k in su.click_hops(c.N, step, pos):
        if k < blocks and any(w[q - k * step] != 0 for q in pos if k * step <= q < k * step + c.N):
            assert alive[k] and (k + 1 == blocks or alive[k + 1]), k
            checked += 1
    assert checked >= (2 if step <= c.N else 1)


@pytest.mark.parametrize("c", NEGATIVE, ids=su.case_id)
def test_negative_pitch_support_is_whole_windows_of_the_oracle(c):
    ref = su.reference(c, "clicks")
    mask = su.case_mask(c)
    wout = su.window_out_len(c.N, c.p)
    assert mask.shape == (ref.shape[1],) and ref.shape[1] % wout == 0
    assert 1.0 - mask.mean() >= 0.25, 1.0 - mask.mean()
    assert mask.any() and not ref[0][~mask].any() and not ref[1:].any()


# ------------------------------------------------------------------ exact scaling
@pytest.mark.parametrize("c", ORACLE_CASES, ids=su.case_id)
def test_c_oracle_scales_bit_for_bit_with_a_power_of_two(c):
    """f32 throughout: products with the window, FFT passes, hypotf, the phasor product, the inverse and the
    overlap-add all scale exactly while nothing overflows or goes subnormal"""
    x = su.make_input(c, "white")
    base = su.reference(c, "white")
    for k in (-30, 30):
        got = wu.oracle_with_window(su.scaled(x, k), c.N, c.f, c.p, oc.hanning(c.N), su.SEED, kernel=su.oracle_kernel(c))
        assert np.array_equal(got.astype(np.float32), su.scaled(base, k)), k


# ------------------------------------------------------------------ the reference side alone on the new inputs
@pytest.mark.parametrize("N,f", [(1024, 4.0), (4096, 2.0)])
@pytest.mark.parametrize("signal", ["clicks", "dc", "nyquist", "white"])
def test_c_oracle_equals_f64_twin_on_each_signal(signal, N, f):
    """measured: 1.4e-7 .. 2.1e-7 of the RMS; held to 1e-6 as tests/test_window_parity_host.py holds its inputs"""
    c = su.Case("wave", N, f, 1, 1, 12 * N + 77, None)
    x = su.make_input(c, signal)
    a = wu.oracle_with_window(x, N, f, 1, oc.hanning(N), su.SEED)
    b = onp.stretch_channel_literal(x[0], N, f, 1.0, 1, su.SEED, 0, window=oc.hanning(N))[None]
    print(f"\nFIGURES oracle against twin N={N} {signal}: rel {wu.rel_err(a, b):.2e}")
    wu.assert_parity(a, b, f"{signal} N={N}", reg=1e-6)
    if signal != "clicks":  # (silent half-windows have no RMS to be relative to)
        wu.assert_blocks(a, b, N // 2, f"{signal} N={N}", bound=1e-6)


# ------------------------------------------------------------------ mutants
def _literal(x, N, f, p, seed, c, past=0.0, leak=0.0, eps=0.0, flush=0.0, swap_dc=False):
    """onp.stretch_channel_literal's loop with the default window, and five things a kernel can do wrong:
    past:    (a) the frame's last slot also takes `past` of the sample behind the frame
    leak:    (b) hop k adds `leak` of hop k - 1's windowed frame
    eps:     (c) |X| = sqrt(re^2 + im^2 + eps)
    flush:   (d) magnitudes below `flush` become 0
    swap_dc: (e) bin 0 takes bin M's phase and bin M bin 0's: the `dc` lane's wrap done wrong"""
    d = onp.derive(N, f, 1.0, p)
    H, S, step, amp = d["H"], d["S"], d["step"], float(d["amp"])
    w = onp.hanning(N).astype(np.float64)
    env = onp.hanning_crossfade_compensation(H).astype(np.float64)
    inp = np.asarray(x, np.float64).copy()
    out_buf = np.zeros(H)
    prev = np.zeros(N)
    done, hop, chunks = False, 0, []
    while not done:
        pos = 0
        while out_buf.size < S + H:
            if inp.size < N:
                inp = np.concatenate([inp, np.zeros(N - inp.size)])
                done = True
            clean = inp[:N] * w
            frame = clean + leak * prev
            if past and inp.size > N:
                frame[N - 1] += past * inp[N]
            prev = clean
            X = np.fft.fft(frame)
            theta = onp.phase_theta(onp.phase_key(seed, c, hop), np.arange(N), N).astype(np.float64)
            if swap_dc:
                theta[[0, H]] = theta[[H, 0]]
            mag = np.sqrt(X.real * X.real + X.imag * X.imag + eps) if eps else np.abs(X)
            if flush:
                mag = np.where(mag < flush, 0.0, mag)
            y = np.fft.ifft(mag * (np.cos(theta) + 1j * np.sin(theta))).real * w
            hop += 1
            out_buf[pos:pos + H] = (y[:H] + out_buf[pos:pos + H]) * env * amp
            out_buf = np.concatenate([out_buf, y[H:]])
            pos += H
            inp = inp[step:]
        chunks.append(onp.resample(out_buf[:S], p))
        out_buf = out_buf[-H:]
    return np.concatenate(chunks)


MN, MF, MSEED = 4096, 4.0, 3
ML = 16 * MN + 77
MUTANTS = {"a_one_past_the_frame": dict(past=1e-4), "b_previous_hop_leaks": dict(leak=1e-6),
           "c_epsilon_under_the_root": dict(eps=1e-20), "d_small_magnitudes_flushed": dict(flush=1e-12),
           "e_dc_and_nyquist_phases_swapped": dict(swap_dc=True)}


@pytest.fixture(scope="module")
def dense():
    """{input: (x, unmutated output)} of the two dense inputs, computed once"""
    out = {}
    for name, x in (("synth", onp.synth_input(0, ML)), ("white", wu.white(0, ML))):
        base = _literal(x, MN, MF, 1, MSEED, 0)
        base.setflags(write=False)
        out[name] = (x, base)
    return out


def _gates(bad, base, what, bands=True):
    """the three gates of the dense-signal tests; bands=False: the band gate must RAISE"""
    wu.assert_parity(bad, base, what)
    wu.assert_blocks(bad[None], base[None], MN // 2, what)
    if bands:
        wu.assert_bands(bad, base, what)
    else:
        with pytest.raises(AssertionError):
            wu.assert_bands(bad, base, what)
    return wu.rel_err(bad, base), float(wu.band_errors(bad, base).max())


def _click_case():
    c = su.Case("mutant", MN, MF, 1, 1, ML, None)
    step, H, n_out = su.geometry(c)
    pos = su.click_positions(MN, step, ML)
    return c, pos, su.support_mask(MN, step, H, 1, n_out, pos), H


def test_unmutated_local_loop_is_the_twin_bit_for_bit():
    for p in (1, 3, -2):
        x = wu.white(0, 5000)
        assert np.array_equal(_literal(x, 256, 4.0, p, MSEED, 0), onp.stretch_channel_literal(x, 256, 4.0, 1.0, p, MSEED, 0))
    c, pos, mask, H = _click_case()
    assert su.first_leak(_literal(su.clicks(1, ML, pos)[0], MN, MF, 1, MSEED, 0), mask, H, 1) is None
    x = wu.white(0, 20000)
    assert np.array_equal(_literal(su.scaled(x, -30), MN, MF, 1, MSEED, 0), _literal(x, MN, MF, 1, MSEED, 0) * 2.0 ** -30)


@pytest.mark.parametrize("mutant", ["a_one_past_the_frame", "b_previous_hop_leaks"])
def test_leak_mutants_pass_the_dense_gates_and_fail_exact_silence(mutant, dense):
    """Both pass assert_parity and assert_blocks on both dense inputs, (a) at 1.8e-6 of the 2e-6 gate, and assert_bands on
    white input. On synth_input (a) does NOT pass assert_bands: the stray sample is broadband and the tonal input's
    other bands are nearly empty, 2.2e-5 of band 2. No GPU test applies the band gate to synth_input, so the dense
    tests still miss it; asserted as it is."""
    kw = MUTANTS[mutant]
    for name, (x, base) in dense.items():
        caught = (mutant, name) == ("a_one_past_the_frame", "synth")
        moved, band = _gates(_literal(x, MN, MF, 1, MSEED, 0, **kw), base, f"{mutant} {name}", bands=not caught)
        print(f"\nFIGURES {mutant} on {name}: moved {moved:.2e} (gate {wu.REG_TOL:.0e}) worst band {band:.2e}")
    c, pos, mask, H = _click_case()
    bad = _literal(su.clicks(1, ML, pos)[0], MN, MF, 1, MSEED, 0, **kw)
    leak = su.first_leak(bad, mask, H, 1)
    print(f"first nonzero sample outside the support: hop {leak}, {np.count_nonzero(bad[~mask])} samples, "
          f"largest {np.abs(bad[~mask]).max():.2e}")
    assert leak is not None


def test_the_pair_of_clicks_alone_hides_a_read_one_past_the_frame():
    """why click_positions adds the two lone clicks: with 0, the pair and L - 1 alone, mutant (a) leaks only into hops
    that already hold a click (step divides N here: the hop that reads x[k step] behind its frame holds x[k step - 1])"""
    c, pos, mask, H = _click_case()
    step = su.geometry(c)[0]
    few = pos[:4]
    m4 = su.support_mask(MN, step, H, 1, mask.size, few)
    bad = _literal(su.clicks(1, ML, few)[0], MN, MF, 1, MSEED, 0, past=1e-4)
    assert su.first_leak(bad, m4, H, 1) is None


@pytest.mark.parametrize("mutant", ["c_epsilon_under_the_root", "d_small_magnitudes_flushed"])
def test_level_mutants_pass_the_dense_gates_and_fail_exact_scaling(mutant, dense):
    """(c) fails at k = -30: |X|^2 is 2e-17 there and the epsilon 1e-20. (d) with the threshold 1e-12 does NOT: the
    smallest of the 3e5 magnitudes of white input is 1e-2, 1e-11 after scaling, so nothing is flushed at k = -30 (it is
    from k = -34 on). What is true is asserted: 1e-12 passes at -30 and fails at -40; a threshold of 1e-10 fails at -30.
    Exact scaling at 2^-30 sees absolute thresholds down to about 1e-11 and none below."""
    for name, (x, base) in dense.items():
        moved, _ = _gates(_literal(x, MN, MF, 1, MSEED, 0, **MUTANTS[mutant]), base, f"{mutant} {name}")
        print(f"\nFIGURES {mutant} on {name}: moved {moved:.2e}")
    x = wu.white(0, ML)

    def scales(k, **kw):
        return np.array_equal(_literal(su.scaled(x, k), MN, MF, 1, MSEED, 0, **kw),
                              _literal(x, MN, MF, 1, MSEED, 0, **kw) * 2.0 ** k)

    if mutant == "c_epsilon_under_the_root":
        assert not scales(-30, eps=1e-20)
    else:
        assert scales(-30, flush=1e-12)
        assert not scales(-40, flush=1e-12)
        assert not scales(-30, flush=1e-10)


def test_swapped_dc_and_nyquist_phases_move_dc_and_nyquist_input_not_the_dense_ones(dense):
    """(e): bins 0 and M hold about 1 / N of the energy of both dense inputs, so a wholly wrong phase there is diluted by
    1 / sqrt(N): it moves white input by 4.1e-2 and synth_input by 2.6e-3 at N = 4096 (still caught: the swap is total;
    an error of d in those two bins alone shows as 0.04 d and 0.003 d). DC input has its largest bin at 0 and Nyquist
    input at M: the swap moves both by more than their RMS, so an error of d there shows as about d."""
    kw = MUTANTS["e_dc_and_nyquist_phases_swapped"]
    for name, (x, base) in dense.items():
        moved = wu.rel_err(_literal(x, MN, MF, 1, MSEED, 0, **kw), base)
        print(f"\nFIGURES (e) on {name}: moved {moved:.2e}")
        assert moved < 0.1, (name, moved)
    for name, x in (("dc", su.dc(1, ML)[0]), ("nyquist", su.nyquist(1, ML)[0])):
        moved = wu.rel_err(_literal(x, MN, MF, 1, MSEED, 0, **kw), _literal(x, MN, MF, 1, MSEED, 0))
        print(f"FIGURES (e) on {name}: moved {moved:.2e}")
        assert moved > 50 * wu.REG_TOL, (name, moved)

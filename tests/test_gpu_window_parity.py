"""GPU parity tests (-m gpu) with caller windows that are NOT mirror-symmetric and do not vanish at the ends of the
frame (tests/windowutil.py: skew, ramp, ramp_down, hann_but_last) on white input, through every kernel path that reads
a window table and every entry that runs hops.

Every other parity test uses windows with w[n] == w[N-1-n] that are ~0 at n = 0 and n = N-1, on an input with 99 % of
its energy in one bin: a kernel that reads the table mirrored, or is off by one at the ends of a frame, passes them
(tests/test_window_parity_host.py shows which mutants do). Here such a kernel is off by 0.01 .. 1 of the output's RMS.
Gates: the contract and the regression gate of tests/test_gpu_parity.py (assert_parity), its per-block bound over half
windows (assert_blocks), and at pitch 1 the same bound per eighth of the spectrum (assert_bands). Each case prints its
figures ("Parity on asymmetric windows and white input")."""
import numpy as np
import pytest

import windowutil as wu
from conftest import rms
from oracle import oracle_np as onp
from windowutil import REG_TOL, WINDOWS

pytestmark = pytest.mark.gpu


def _engine_mod():
    import rocoder_amd
    from rocoder_amd import _lib

    assert _lib.lib().rc_device_count() > 0, "no MI355X visible: GPU tests must not silently pass"
    return rocoder_amd


def _reg(N, f):
    """the project's own numbers: 5e-6 where step > window (factor below 0.5), 1.2e-6 on the long-window path"""
    return 5.0e-6 if f < 0.5 else 1.2e-6 if N > 65536 else REG_TOL


def _half_window(N, p):
    wout = N if p > 0 else (-(-N // -p) - 1) * -p  # (S - 1) |p| with S = ceil(N / |p|): src/stretcher.rs:47-51,108-113
    return max(1, wout // 2)


def _check(got, ref, N, f, p, what):
    """print the three figures, then: parity per channel, blocks over half windows, bands at pitch 1"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    block = _half_window(N, p)
    nb = got.shape[-1] // block
    d = (got[..., :nb * block] - ref[..., :nb * block]).reshape(got.shape[:-1] + (nb, block))
    blk = float((np.sqrt((d * d).mean(axis=-1)) / np.sqrt((ref * ref).mean(axis=-1, keepdims=True))).max()) if nb else 0.0
    band = float(wu.band_errors(got, ref).max()) if p == 1 else float("nan")
    rel = max(wu.rel_err(got[c], ref[c]) for c in range(got.shape[0]))
    print(f"\nFIGURES {what}: rel {rel:.2e} block {blk:.2e} band {band:.2e}")
    for c in range(got.shape[0]):
        wu.assert_parity(got[c], ref[c], f"{what} ch{c}", reg=_reg(N, f))
    if nb:
        wu.assert_blocks(got, ref, block, what)
    if p == 1:
        wu.assert_bands(got, ref, what)


def _run(ra, x, N, f, p, w, seed, **kw):
    with ra.Engine(window_len=N, factor=f, pitch_multiple=p, channels=x.shape[0], seed=seed, window=w, **kw) as e:
        return e.stretch_host(x)


# ------------------------------------------------------------------ offline job, kernel path by kernel path
GENERIC = [(64, 2.0, 1, 3, 5000, "skew"), (256, 4.0, 2, 2, 9999, "ramp"), (128, 0.3, 1, 2, 20000, "ramp_down")]
WAVE_LOCAL = [  # the TABW instantiations: pitch 1 at compile time, other pitches at run time, per length
    (512, 8.0, 1, 2, 20001, "ramp"), (512, 2.0, 5, 1, 9000, "skew"),
    (1024, 4.0, 3, 1, 33333, "ramp_down"), (1024, 8.0, 1, 2, 1025, "ramp"),
    (2048, 8.0, 1, 2, 30000, "skew"), (2048, 3.0, 2, 2, 50001, "ramp"),
    (4096, 0.25, 1, 2, 100000, "ramp"), (4096, 8.0, 1, 1, 4095, "ramp_down"),
    (8192, 2.0, 2, 3, 60001, "skew"), (8192, 8.0, 1, 2, 9000, "ramp")]
L16 = 40 * 1024 + 777  # several runs with seams at N = 16384 (test_band_mask_fused_into_the_16384_kernel's length)
N16384 = [(16384, 8.0, 1, 2, L16, "ramp"), (16384, 8.0, 1, 2, L16, "ramp_down"), (16384, 8.0, 1, 2, L16, "skew"),  # hop4, table
          (16384, 8.0, 3, 2, L16, "ramp"),   # hop2 table, decimating stores
          (16384, 8.0, 5, 2, L16, "skew"), (16384, 8.0, 1, 3, L16, "ramp")]
QUARTER = [(32768, 8.0, 2, 2, 3 * 32768 + 777, "ramp"), (65536, 16.0, 1, 2, 3 * 65536 + 777, "skew"),
           (65536, 16.0, 1, 1, 1000, "ramp_down")]
CHIRP_Z = [(1000, 4.0, 2, 2, 20000, "ramp"), (3000, 8.0, 1, 1, 12000, "skew"), (24000, 3.0, 1, 1, 130000, "ramp_down")]
LONG = [(131072, 4.0, 1, 2, 500000, "skew"), (65538, 4.0, 1, 1, 300000, "ramp")]
NEGATIVE = [(2048, 3.0, -2, 2, 40000, "ramp"), (16384, 8.0, -3, 1, 60000, "skew"), (3000, 3.0, -2, 1, 40000, "ramp_down")]


@pytest.mark.parametrize("N,f,p,ch,L,name", GENERIC + WAVE_LOCAL + N16384 + QUARTER + CHIRP_Z + LONG + NEGATIVE)
def test_caller_window_on_every_kernel_path(N, f, p, ch, L, name):
    """The generic slots kernel (N <= 256), the wave-local TABW kernels (512 .. 8192), hop4 / hop2 with a table (16384),
    big5s / big5 with a table (32768, 65536), the chirp-z kernels (lengths that are no power of two), rc_long.hip (above
    65536) and resample_slower behind them (negative pitch). Reference: the C oracle driven with the same window; the f64
    twin where the C oracle's transform is the O(N^2) sum and above 65536."""
    ra = _engine_mod()
    x = wu.white_input(ch, L)
    w = WINDOWS[name](N)
    got = _run(ra, x, N, f, p, w, seed=3)
    ref = wu.oracle_with_window(x, N, f, p, w, seed=3)
    _check(got, ref, N, f, p, f"N={N} f={f} p={p} ch={ch} L={L} {name}")


@pytest.mark.parametrize("p", [1, 3])
def test_16384_last_sample_of_the_window_alone(p):
    """hann_but_last is the default window in all samples but the last. The engine must not take it for the default
    (its detection compares all N samples) and the table kernels must honour w[N-1]: parity with the oracle driven with
    that window, and a result that differs from the window=None run by more than 1e-3 of its RMS (the f64 twin: 7e-3)."""
    ra = _engine_mod()
    N, f = 16384, 8.0
    x = wu.white_input(2, L16)
    w = wu.hann_but_last(N)
    got = _run(ra, x, N, f, p, w, seed=21)
    ref = wu.oracle_with_window(x, N, f, p, w, seed=21)
    _check(got, ref, N, f, p, f"N=16384 p={p} hann_but_last")
    default = _run(ra, x, N, f, p, None, seed=21)
    moved = min(wu.rel_err(got[c], default[c]) for c in range(2))
    print(f"hann_but_last against the default window: {moved:.2e}")
    assert moved > 1e-3, moved


# ------------------------------------------------------------------ spectrum pipelines with a caller window
def _hermitian_breaking(t, spec):  # test_spectral_kernel_matches_oracle's: depends on the bin index, all N bins matter
    n = spec.size
    g = np.linspace(0.2, 1.5, n).astype(np.float32)
    out = spec * g
    out[n // 3:] *= np.complex64(1j)
    return out


def _np_band(lo, hi, gi, go):
    def k(t, spec):
        n = spec.size
        f = np.minimum(np.arange(n), n - np.arange(n))
        g = np.where((f >= lo) & (f <= hi), np.float32(gi), np.float32(go)).astype(np.float32)
        return spec * g
    return k


def _np_shift(s):
    def k(t, spec):
        n = spec.size
        m = n // 2
        out = np.zeros(n, np.complex64)
        f = np.arange(m + 1)
        src = f - s
        ok = (src >= 0) & (src <= m)
        out[f[ok]] = spec[src[ok]]
        j = np.arange(m + 1, n)
        out[j] = np.conj(out[n - j])
        return out
    return k


@pytest.mark.parametrize("N,f,p", [(2048, 4.0, 2), (16384, 8.0, 1), (32768, 8.0, 1)])
def test_host_kernel_pipeline_with_a_caller_window(N, f, p):
    """analysis half, host kernel on the natural-order spectrum, synthesis half: both halves read the table"""
    ra = _engine_mod()
    x = wu.white_input(2, 3 * N + 777)
    w = wu.ramp(N)
    got = _run(ra, x, N, f, p, w, seed=11, kernel=_hermitian_breaking, kernel_time_ms=123)
    ref = wu.oracle_with_window(x, N, f, p, w, seed=11, kernel=_hermitian_breaking)
    _check(got, ref, N, f, p, f"host kernel N={N} p={p} ramp")


@pytest.mark.parametrize("N,f", [(4096, 4.0), (16384, 8.0)])
@pytest.mark.parametrize("dk", ["band", "shift"])
def test_device_kernels_with_a_caller_window(N, f, dk):
    ra = _engine_mod()
    x = wu.white_input(2, 3 * N + 777)
    w = wu.skew(N)
    if dk == "band":
        lo, hi = N // 64, N // 8
        got = _run(ra, x, N, f, 1, w, seed=17, device_kernel=("band", lo, hi, 1.25, 0.1))
        ref = wu.oracle_with_window(x, N, f, 1, w, seed=17, kernel=_np_band(lo, hi, 1.25, 0.1))
    else:
        got = _run(ra, x, N, f, 1, w, seed=17, device_kernel=("shift", 37))
        ref = wu.oracle_with_window(x, N, f, 1, w, seed=17, kernel=_np_shift(37))
    _check(got, ref, N, f, 1, f"device kernel {dk} N={N} skew")


# ------------------------------------------------------------------ the single-hop seam
@pytest.mark.parametrize("name", ["ramp", "skew"])
@pytest.mark.parametrize("N", [1024, 16384, 32768, 1000])
def test_refft_with_a_caller_window(N, name):
    """forward_fft is the only place a rotated or reversed ANALYSIS frame is visible (|X| forgets both): the complex
    spectrum against numpy's f64 FFT of x w, with test_refft_seam_on_large_window's gate; then one resynthesised hop."""
    ra = _engine_mod()
    x = wu.white(1, N)
    w = WINDOWS[name](N)
    r = ra.ReFFT(w, seed=3, channel_index=1)
    X = r.forward_fft(x).astype(np.complex128)
    Xo = np.fft.fft(x.astype(np.float64) * w.astype(np.float64))
    err, scale = rms(np.abs(X - Xo)), rms(np.abs(Xo))
    y = r.resynth(x, hop=5)
    yo = onp.resynth(x, w, onp.phase_key(3, 1, 5))
    print(f"\nFIGURES ReFFT N={N} {name}: fft rel {err / scale:.2e} resynth rel {wu.rel_err(y, yo):.2e}")
    assert err <= 2e-6 * scale + 1e-6, (N, name, err / scale)
    wu.assert_parity(y, yo, f"resynth N={N} {name}")


# ------------------------------------------------------------------ other entries: the offline job's bits
ENTRY_CASES = [(4096, 4.0), (16384, 8.0)]
ENTRY_L = 300_000


def _offline(ra, x, N, f, w):
    import torch

    with ra.Engine(window_len=N, factor=f, channels=x.shape[0], seed=11, window=w) as e:
        return e.stretch_tensor(torch.from_numpy(x).cuda()).cpu().numpy()


@pytest.mark.parametrize("N,f", ENTRY_CASES)
def test_streaming_seam_with_a_caller_window_equals_the_offline_job_bit_for_bit(N, f):
    """ragged pushes while the channels are open (windows drained as they become computable), then the closed rest;
    next_window and next_window_view in turn"""
    ra = _engine_mod()
    x = wu.white_input(2, ENTRY_L)
    w = wu.ramp(N)
    ref = _offline(ra, x, N, f, w)
    sizes = [50000, 1, 4095, 70000, 333, 40001]
    with ra.Engine(window_len=N, factor=f, channels=2, seed=11, window=w) as e:
        wins = [[], []]

        def take(c):
            got = e.next_window_view(c) if (len(wins[c]) & 1) else e.next_window(c)
            if got is not None:
                wins[c].append(np.array(got))
            return got is not None

        pos = live = 0
        for sz in sizes:
            for c in range(2):
                e.push_input(c, x[c, pos:pos + sz])
            pos += sz
            while take(0):
                assert take(1)
                live += 1
        assert live > 0 and pos < ENTRY_L
        for c in range(2):
            e.push_input(c, x[c, pos:])
            e.close_input(c)
        while not e.is_done(0):
            for c in range(2):
                assert take(c)
        assert e.is_done(1)
    for c in range(2):
        got = np.concatenate(wins[c])
        assert got.shape == ref[c].shape, (c, got.shape, ref[c].shape)
        assert np.array_equal(got, ref[c]), f"channel {c}"
    # (the offline job itself against the oracle on a prefix: the bits above are the right ones)
    Lp = 3 * N + 777
    _check(_offline(ra, np.ascontiguousarray(x[:, :Lp]), N, f, w), wu.oracle_with_window(x[:, :Lp], N, f, 1, w, seed=11),
           N, f, 1, f"offline prefix N={N} ramp")


@pytest.mark.parametrize("N,f", ENTRY_CASES)
def test_window_ranges_with_a_caller_window_concatenate_to_the_offline_job(N, f):
    import torch

    ra = _engine_mod()
    from rocoder_amd.distributed import engine_compute, shard_plan

    x = wu.white_input(2, ENTRY_L)
    xt = torch.from_numpy(x).cuda()
    with ra.Engine(window_len=N, factor=f, channels=2, seed=11, window=wu.ramp(N)) as e:
        full = e.stretch_tensor(xt).clone()
        torch.cuda.synchronize()
        wout = e.params.window_out_len
        nwin = full.shape[1] // wout
        comp = engine_compute(e, xt)
        for world in (2, 3):
            out = torch.zeros_like(full)
            for s in shard_plan(2, nwin, world):
                out[s.ch_first:s.ch_first + s.ch_count, s.win_first * wout:(s.win_first + s.win_count) * wout] = comp(s)
            torch.cuda.synchronize()
            assert torch.equal(out, full), f"world={world}"

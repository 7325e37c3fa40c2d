"""GPU tests (-m gpu) of the long-window path: window lengths 65538 .. 2^22 through the four-step
kernels of rc_long.hip, against the oracles, through every entry that runs hops: the transform alone, the single-hop
ReFFT seam, the offline job (plain, host frequency kernel, device kernels), the streaming seam (closed and live),
chunking, the multi-device entry and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rms
from oracle import cbind as oc
from oracle import oracle_np as onp
from wavutil import read_wav_f32, write_wav

pytestmark = pytest.mark.gpu

TOL = 1.0e-4  # the contract (tests/test_gpu_parity.py)
# Regression gate of the long-window path, measured on the first MI355X run with < 3x margin
REG_TOL = 1.2e-6    # worst measured: 4.6e-7 (single-hop resynth at 4194302)
BLOCK_TOL = 1.8e-6  # any one hop's block of output, relative to the channel's RMS (worst measured: 6.1e-7)
FFT_TOL = 1.0e-6    # the transform alone, relative RMS against numpy's f64 FFT


def _ra():
    import rocoder_amd
    from rocoder_amd import _lib

    assert _lib.lib().rc_device_count() > 0, "no MI355X visible: GPU tests must not silently pass"
    return rocoder_amd


def assert_parity(got, ref, what="", reg=REG_TOL):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = rms(got - ref)
    r = rms(ref)
    print(f"parity {what}: rel {err / max(r, 1e-30):.3e}")
    assert err <= TOL and err <= TOL * r + 1e-9, f"{what}: rms_err={err:.3e} rms_ref={r:.3e}"
    assert err <= reg * r + 1e-9, f"{what}: REGRESSION rms_err={err:.3e} = {err / max(r, 1e-30):.2e} of rms_ref"
    return err


def assert_blocks(got, ref, block, what="", bound=BLOCK_TOL):
    """one block per hop: no bad hop hides inside a good global RMS"""
    got = np.atleast_2d(np.asarray(got, np.float64))
    ref = np.atleast_2d(np.asarray(ref, np.float64))
    nb = got.shape[-1] // block
    if nb == 0:
        return 0.0
    d = (got[..., :nb * block] - ref[..., :nb * block]).reshape(got.shape[:-1] + (nb, block))
    blk = np.sqrt((d * d).mean(axis=-1))
    scale = np.sqrt((ref * ref).mean(axis=-1, keepdims=True)) + 1e-30
    worst = float((blk / scale).max())
    print(f"blocks {what}: worst {worst:.3e}")
    assert worst <= bound, (what, worst, np.unravel_index((blk / scale).argmax(), blk.shape))
    return worst


def _oracle(x, N, f, p, seed, kernel=None):
    """the C oracle (radix-2 f32 FFT) for powers of two, the f64 closed form otherwise"""
    if N & (N - 1) == 0:
        return oc.stretch_offline(x, N, f, 1.0, p, seed=seed, kernel=kernel).astype(np.float64)
    assert p >= 1
    return np.stack([onp.stretch_channel_closed(x[c], N, f, 1.0, p, seed, c, kernel=kernel) for c in range(x.shape[0])])


def _input(ch, L, N):
    """the BASELINE synthetic input (sines + noise) per channel"""
    return np.stack([onp.synth_input(c, L) for c in range(ch)]).astype(np.float32)


# ------------------------------------------------------------------ 1. the transform alone, 2. single-hop resynth
@pytest.mark.parametrize("N", [1 << 17, 1 << 20, 1 << 22, 65538, 100002, 4194302])
def test_forward_fft_and_resynth_against_numpy(N):
    ra = _ra()
    rng = np.random.default_rng(N)
    t = np.arange(N) / 44100.0
    x = (0.3 * rng.standard_normal(N) + 0.5 * np.sin(2 * np.pi * 441.0 * t)).astype(np.float32)
    w = oc.hanning(N)
    r = ra.ReFFT(w, seed=7, channel_index=1)
    X = r.forward_fft(x).astype(np.complex128)
    Xo = np.fft.fft(x.astype(np.float64) * w.astype(np.float64))
    rel = rms(np.abs(X - Xo)) / rms(np.abs(Xo))
    print(f"fft N={N}: rel {rel:.3e}")
    assert rel <= FFT_TOL, (N, rel)
    y = r.resynth(x, hop=3)
    yo = onp.resynth(x, w, onp.phase_key(7, 1, 3))
    assert_parity(y, yo, f"resynth {N}")


# ------------------------------------------------------------------ 3. every output sample against the oracle
CASES = [
    (131072, 1.5, 1, 2, 500_000), (131072, 8.0, 2, 1, 300_000), (131072, 4.0, 3, 2, 400_000),
    (131072, 2.0, -2, 1, 400_000),
    (262144, 8.0, 1, 2, 600_000), (262144, 3.0, 2, 1, 700_000), (262144, 4.0, -2, 2, 700_000),
    (1048576, 8.0, 1, 2, 1_600_000), (1048576, 6.0, 3, 1, 1_500_000), (1048576, 2.0, 1, 1, 2_000_000),
    (65538, 4.0, 1, 2, 300_000), (65538, 2.0, 2, 1, 250_000),
    (100000, 8.0, 1, 2, 350_000), (100000, 3.0, 2, 1, 300_000),
]


@pytest.mark.parametrize("N,f,p,ch,L", CASES)
def test_long_windows_match_oracle(N, f, p, ch, L):
    ra = _ra()
    x = _input(ch, L, N)
    got = ra.stretch(x, window_len=N, factor=f, pitch_multiple=p, seed=0x1F)
    ref = _oracle(x, N, f, p, 0x1F)
    assert got.shape == ref.shape
    for c in range(ch):
        assert_parity(got[c], ref[c], f"N={N} f={f} p={p} ch{c}")
    d = ra.derive_params(window_len=N, factor=f, pitch_multiple=p)
    assert_blocks(got, ref, d.window_out_len // d.hops_per_window if p > 0 else d.window_out_len, f"N={N} p={p}")


@pytest.mark.parametrize("N", [1 << 22, (1 << 22) - 2])
def test_longest_windows_match_oracle(N):
    ra = _ra()
    f = 8.0
    step = (N // 2) / f
    L = int(N + 4 * step)  # about six hops per channel
    x = _input(2, L, N)
    got = ra.stretch(x, window_len=N, factor=f, seed=0x22)
    ref = _oracle(x, N, f, 1, 0x22)
    for c in range(2):
        assert_parity(got[c], ref[c], f"N={N} ch{c}")
    assert_blocks(got, ref, N // 2, f"N={N}")


# ------------------------------------------------------------------ 4. edge cases (src/stretcher.rs:123-135)
@pytest.mark.parametrize("N", [131072, 100000])
def test_edge_lengths(N):
    ra = _ra()
    f = 2.0
    step = ra.derive_params(window_len=N, factor=f).sample_step_len
    for L in (N // 3, N, N + step - 1):
        x = _input(1, L, N)
        got = ra.stretch(x, window_len=N, factor=f, seed=9)
        assert_parity(got[0], _oracle(x, N, f, 1, 9)[0], f"N={N} L={L}")
    x = _input(1, 3 * N, N)  # factor < 0.5: step > N, samples between the windows are skipped
    got = ra.stretch(x, window_len=N, factor=0.4, seed=9)
    assert_parity(got[0], _oracle(x, N, 0.4, 1, 9)[0], f"N={N} f=0.4")


# ------------------------------------------------------------------ 5. host frequency kernel
@pytest.mark.parametrize("N", [131072, 100000])
def test_host_kernel_spectrum_order_time_and_panic(N):
    ra = _ra()
    x = _input(2, 3 * N, N)
    calls = []

    def k(t, spec):  # a natural-order N-bin spectrum: bins j and N - j are conjugates of a real frame
        calls.append((t, spec.size, round(float(np.abs(spec[:64]).sum()), 2),
                      float(abs(spec[7] - np.conj(spec[N - 7])) / (abs(spec[7]) + 1e-6))))
        out = spec.copy()
        out[: N // 8] *= np.float32(1.5)
        out[N - N // 8 + 1:] *= np.float32(1.5)
        return out

    got = ra.stretch(x, window_len=N, factor=4.0, seed=5, kernel=k, kernel_time_ms=777)
    ocalls = []

    def ko(t, spec):
        ocalls.append(round(float(np.abs(spec[:64]).sum()), 2))
        out = spec.copy()
        out[: N // 8] *= np.float32(1.5)
        out[N - N // 8 + 1:] *= np.float32(1.5)
        return out

    ref = _oracle(x, N, 4.0, 1, 5, kernel=ko)
    for c in range(2):
        assert_parity(got[c], ref[c], f"kernel N={N} ch{c}")
    assert all(c[0] == 777 and c[1] == N and c[3] <= 1e-3 for c in calls)
    if N & (N - 1):  # the f64 oracle runs channel after channel: put its calls in the reference's order
        K, hpw = len(ocalls) // 2, 2
        ocalls = [ocalls[c * K + h] for w0 in range(0, K, hpw) for c in range(2) for h in range(w0, w0 + hpw)]
    assert len(calls) == len(ocalls) and np.allclose([c[2] for c in calls], ocalls, rtol=1e-3)  # windows outer

    def bad(t, spec):
        raise RuntimeError("panic")  # src/fft.rs:100-106: identity

    a = ra.stretch(x, window_len=N, factor=4.0, seed=5, kernel=bad)
    b = ra.stretch(x, window_len=N, factor=4.0, seed=5)
    assert_parity(a, b, f"panic N={N}", reg=1e-6)


# ------------------------------------------------------------------ 6. device kernels
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


def test_device_kernels_at_262144():
    ra = _ra()
    N, f = 262144, 4.0
    x = _input(2, 700_000, N)
    g = ra.stretch(x, window_len=N, factor=f, seed=17, device_kernel=("gain", -1.5))
    assert_parity(g, _oracle(x, N, f, 1, 17, kernel=lambda t, s: s * np.float32(-1.5)), "gain")
    lo, hi = 2000, 30000
    band = ra.stretch(x, window_len=N, factor=f, seed=17, device_kernel=("band", lo, hi, 1.25, 0.1))
    assert_parity(band, _oracle(x, N, f, 1, 17, kernel=_np_band(lo, hi, 1.25, 0.1)), "band")
    for sh in (300, -120):
        got = ra.stretch(x, window_len=N, factor=f, seed=17, device_kernel=("shift", sh))
        assert_parity(got, _oracle(x, N, f, 1, 17, kernel=_np_shift(sh)), f"shift {sh}")


# ------------------------------------------------------------------ 7. streaming seam
ORDERS = ["round_robin", "channel_after_channel", "unequal_lengths"]
SEAM_CASES = [(131072, 4.0, 1, 2, 700_000, o) for o in ORDERS] + [(100000, 3.0, 2, 3, 500_000, o) for o in ORDERS] + \
    [(1 << 22, 8.0, 3, 2, (1 << 22) + 6 * (1 << 18), "round_robin")]


@pytest.mark.parametrize("N,f,p,ch,L,order", SEAM_CASES)
def test_seam_equals_offline_bit_for_bit(N, f, p, ch, L, order):
    import torch

    ra = _ra()
    x = _input(ch, L, N)
    lens = [L - (c * (L // 7) if order == "unequal_lengths" else 0) for c in range(ch)]
    with ra.Engine(window_len=N, factor=f, pitch_multiple=p, channels=ch, seed=11) as e:
        refs = []
        for c in range(ch):
            xt = torch.from_numpy(np.ascontiguousarray(x[:, :lens[c]])).cuda()
            refs.append(e.stretch_tensor(xt)[c].cpu().numpy())
    with ra.Engine(window_len=N, factor=f, pitch_multiple=p, channels=ch, seed=11) as e:
        if N == 1 << 22:
            assert e.params.window_out_len * 4 > 8 << 20  # one window is larger than the seam's 8 MiB group cap
        for c in range(ch):
            e.push_input(c, x[c, :lens[c]])
            e.close_input(c)
        wins = [[] for _ in range(ch)]
        if order == "channel_after_channel":
            for c in range(ch):
                while not e.is_done(c):
                    wins[c].append(e.next_window(c).copy())
        else:
            live = list(range(ch))
            while live:
                for c in list(live):
                    if e.is_done(c):
                        live.remove(c)
                        continue
                    w = e.next_window_view(c) if (len(wins[c]) & 1) else e.next_window(c)
                    wins[c].append(np.array(w))
        for c in range(ch):
            got = np.concatenate(wins[c])
            assert got.shape == refs[c].shape, (c, got.shape, refs[c].shape)
            assert np.array_equal(got, refs[c]), f"channel {c} ({order})"
        with pytest.raises(ra.RocoderError):  # as at every other length: no hand-out after is_done
            e.next_window(0)


@pytest.mark.parametrize("N", [131072, 100000])
def test_live_seam_equals_offline(N):
    ra = _ra()
    f, L = 4.0, 800_000
    x = _input(2, L, N)
    ref = ra.stretch(x, window_len=N, factor=f, seed=31)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=31) as e:
        wins = [[], []]
        pos = 0
        live = 0
        for chunk in (L // 4, L // 4, L // 4):
            for c in range(2):
                e.push_input(c, x[c, pos:pos + chunk])
            pos += chunk
            while True:
                w0 = e.next_window(0)
                if w0 is None:
                    break
                wins[0].append(w0)
                wins[1].append(e.next_window(1))
                live += 1
        assert live > 0
        for c in range(2):
            e.push_input(c, x[c, pos:])
            e.close_input(c)
        while not e.is_done(0):
            for c in range(2):
                wins[c].append(e.next_window(c))
        assert e.is_done(1)
        got = np.stack([np.concatenate(wins[0]), np.concatenate(wins[1])])
    assert got.shape == ref.shape and np.array_equal(got, ref)


# ------------------------------------------------------------------ 8. chunking and determinism
def test_chunks_and_seeds():
    """window ranges (each its own chunk, the tail recomputed from the hop before it) and a seam job in batches of
    two hops equal the one-chunk job bit for bit; the same seed reproduces it, another changes it"""
    import torch

    ra = _ra()
    N, f = 131072, 8.0
    x = _input(2, 1_000_000, N)
    a = ra.stretch(x, window_len=N, factor=f, seed=3)
    b = ra.stretch(x, window_len=N, factor=f, seed=3)
    c = ra.stretch(x, window_len=N, factor=f, seed=4)
    assert np.array_equal(a, b)
    assert rms(a - c) > 0.1 * rms(a)
    xt = torch.from_numpy(x).cuda()
    with ra.Engine(window_len=N, factor=f, channels=2, seed=3) as e:
        full = e.stretch_tensor(xt)
        torch.cuda.synchronize()
        wout = e.params.window_out_len
        nwin = full.shape[1] // wout
        from rocoder_amd.distributed import engine_compute, shard_plan

        comp = engine_compute(e, xt)
        for world in (2, 3, 5):
            out = torch.zeros_like(full)
            for sh in shard_plan(2, nwin, world):
                out[sh.ch_first:sh.ch_first + sh.ch_count,
                    sh.win_first * wout:(sh.win_first + sh.win_count) * wout] = comp(sh)
            torch.cuda.synchronize()
            assert torch.equal(out, full), f"world={world}"
    assert np.array_equal(full.cpu().numpy(), a)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=3, max_batch_hops=2) as e:
        for ch in range(2):
            e.push_input(ch, x[ch])
            e.close_input(ch)
        wins = [[], []]
        while not e.is_done(0):
            for ch in range(2):
                wins[ch].append(e.next_window(ch))
        assert np.array_equal(np.stack([np.concatenate(w) for w in wins]), a)


# ------------------------------------------------------------------ 9. several devices, one process
def test_multi_engine_equals_single_engine():
    import torch

    ra = _ra()
    N, f = 131072, 4.0
    x = _input(2, 900_000, N)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=99) as e:
        one = e.stretch_host(x)
    with ra.MultiEngine([0, 0], window_len=N, factor=f, channels=2, seed=99) as m:
        got_h = m.stretch_host(x)
        got_t = m.stretch_tensor(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(got_h, one)
    assert np.array_equal(got_t, one)


# ------------------------------------------------------------------ 10. CLI
def test_cli_long_window(tmp_path):
    ra = _ra()
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    x = _input(2, 700_000, 262144)
    wav, out = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    dec = write_wav(wav, x, 44100, "f32")
    r = subprocess.run([cli, "-i", wav, "-o", out, "-w", "262144", "-f", "4", "--seed", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rate, got = read_wav_f32(out)
    assert rate == 44100
    ref = ra.stretch(dec, window_len=262144, factor=4.0, seed=3)
    assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.float32))

"""User device kernels that read the spectra of earlier hops (RC_HISTORY, X.past(d)) on the MI355X. The oracle side is a
stateful host kernel, one closure per channel that keeps the last D analysis spectra it was handed (call i is hop i) and
accumulates in float32 in the order of the HIP source; every other check is an identity between GPU jobs, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from multi_devices import device_lists
from oracle import cbind as oc
from oracle import oracle_np as onp
from wavutil import read_wav_f32, write_wav

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "examples", "kernels")
TOL = 1e-4

X2 = ("__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
      "{ float2 x = X[j]; return make_float2(2.f * x.x, 2.f * x.y); }")

# (window, factor): Hop, Big, Gen and Long paths (tests/test_gpu_user_dk.py::PATHS)
PATHS = [(1024, 4.0), (65536, 8.0), (12288, 4.0), (131072, 4.0)]
W4 = [0.5, 0.25, -0.375, 0.125]  # blur, D = 3: four weights, exactly representable


def _ra():
    import rocoder_amd
    from rocoder_amd import _lib

    assert _lib.lib().rc_device_count() > 0, "no MI355X visible: GPU tests must not silently pass"
    return rocoder_amd


def example(name, depth=None):
    with open(os.path.join(EXAMPLES, name)) as f:
        src = f.read()
    return src if depth is None else f"#define RC_HISTORY {depth}\n" + src


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a)))


def assert_close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, r = rms(got.astype(np.float64) - ref), rms(ref)
    print(f"{what}: rms_err={err:.3e} rms_ref={r:.3e}")
    assert err <= TOL and err <= TOL * r + 1e-9, f"{what}: rms_err={err:.3e} rms_ref={r:.3e}"


def _job(ra, x, N, f, p, seed, src=None, params=None, **kw):
    with ra.Engine(window_len=N, factor=f, pitch_multiple=p, channels=x.shape[0], seed=seed, **kw) as e:
        if src is not None:
            e.set_device_kernel_source(src)
        if params is not None:
            e.set_device_kernel_params(params)
        return e.stretch_host(x).copy()


def delay_fn(D):
    def make():
        past = []

        def k(t, spec):
            past.append(spec.copy())
            return past[-1 - D].copy() if len(past) > D else np.zeros_like(spec)

        return k

    return make


def blur_fn(weights):
    D = len(weights) - 1

    def make():
        past = []

        def k(t, spec):
            past.append(spec.copy())
            del past[:-(D + 1)]
            y = np.zeros_like(spec)
            for d in range(min(D + 1, len(past))):  # y += w_d * X_{k-d}, as examples/kernels/blur.hip
                y = y + np.float32(weights[d]) * past[-1 - d]
            return y.astype(np.complex64)

        return k

    return make


def _oracle_stateful(x, N, f, p, seed, make):
    """Per-channel oracle Stretchers, each with its own stateful host kernel: call i of a channel is its hop i."""
    n_out = oc.offline_output_len(x.shape[1], N, f, p)
    out = np.zeros((x.shape[0], n_out), np.float32)
    for c in range(x.shape[0]):
        st = oc.Stretcher(channels=x.shape[0], factor=f, pitch_multiple=p, window=oc.hanning(N), seed=seed,
                          channel_index=c, kernel=make())
        st.send(x[c])
        st.close_input()
        parts = []
        while not st.is_done():
            parts.append(st.next_window())
        y = np.concatenate(parts)[:n_out]
        out[c, :y.size] = y
    return out


# ---- 1. paths and pitches -------------------------------------------------------------------------------------------
KERNELS = {"delay1": (lambda: example("delay.hip", 1), None, delay_fn(1)),
           "delay8": (lambda: example("delay.hip", 8), None, delay_fn(8)),
           "blur3": (lambda: example("blur.hip", 3), W4, blur_fn(W4))}


@pytest.mark.parametrize("N,f", PATHS)
@pytest.mark.parametrize("p", [1, 3, -2])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_history_kernels_match_the_stateful_oracle(N, f, p, kernel):
    ra = _ra()
    src, params, make = KERNELS[kernel]
    L = 5 * N + 333
    if N & (N - 1):  # (the oracle's transform of such a length is slow: 21 whole hops at every pitch, and the short ones)
        L = N + 20 * int(ra.derive_params(window_len=N, factor=f, pitch_multiple=p).sample_step_len) + 333
    x = np.stack([onp.synth_input(c + 1, L) for c in range(2)])
    got = _job(ra, x, N, f, p, 23, src=src(), params=params)
    ref = _oracle_stateful(x, N, f, p, 23, make)
    assert rms(ref) > 1e-3, "the case must not be silence"
    assert_close(got, ref, f"{kernel} N={N} p={p}")


# ---- 2. identities between GPU jobs ---------------------------------------------------------------------------------
def test_past_zero_is_the_hop_itself():
    ra = _ra()
    x = np.stack([onp.synth_input(c, 9 * 4096) for c in range(2)])
    base = _job(ra, x, 4096, 4.0, 1, 3, src=X2)
    assert np.array_equal(_job(ra, x, 4096, 4.0, 1, 3, src=X2.replace("X[j]", "X.past(0)[j]")), base)
    deep = "#define RC_HISTORY 2\n" + X2.replace("X[j]", "X.past(0)[j]")
    assert np.array_equal(_job(ra, x, 4096, 4.0, 1, 3, src=deep), base)
    assert np.array_equal(_job(ra, x, 4096, 4.0, 1, 3, src=X2.replace("X[j]", "X.past(1).past(0)[j]")), 0 * base)


def test_reads_past_the_declared_history_are_zero():
    ra = _ra()
    body = """#define RC_HISTORY 2
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 a = X[j], b = X.past(2)[j + 1];
    float2 y = make_float2(a.x + 0.5f * b.x, a.y + 0.5f * b.y);
    EXTRA
    return y;
}
"""
    extra = "const float2 c = X.past(3)[j], d = X.past(1).past(2)[j]; y.x += c.x + d.x; y.y += c.y + d.y;"
    for N, f in ((4096, 4.0), (12288, 4.0)):
        x = np.stack([onp.synth_input(c, 9 * N) for c in range(2)])
        without = _job(ra, x, N, f, 1, 5, src=body.replace("EXTRA", ""))
        clamped = _job(ra, x, N, f, 1, 5, src=body.replace("EXTRA", extra))
        assert np.array_equal(clamped, without), N
        assert not np.array_equal(without, _job(ra, x, N, f, 1, 5, src=X2.replace("2.f", "1.f"))), "past(2) is read"


@pytest.mark.parametrize("D", [1, 8])
def test_delay_starts_with_silence(D):
    ra = _ra()
    N, H = 2048, 1024
    x = np.stack([onp.synth_input(c, 40 * N) for c in range(2)])
    y = _job(ra, x, N, 4.0, 1, 8, src=example("delay.hip", D))
    # pitch 1: hop k adds to output samples [k H, k H + N), so [0, D H) hears hops < D only
    assert np.all(y[:, :D * H] == 0.0)
    assert rms(y[:, D * H:(D + 1) * H]) > 1e-4


# ---- 3. seams of the computation: all equal the offline job, blur at D = 3 -------------------------------------------
def _blur_engine(ra, N, f, ch, seed, **kw):
    e = ra.Engine(window_len=N, factor=f, channels=ch, seed=seed, **kw)
    e.load_device_kernel(ra.compile_device_kernel(example("blur.hip", 3)))
    e.set_device_kernel_params(W4)
    return e


def _pull_all(e, x, close_first):
    outs = [[] for _ in range(x.shape[0])]
    for c in range(x.shape[0]):
        e.push_input(c, x[c])
        if close_first:
            e.close_input(c)
    done = [False] * x.shape[0]
    while not all(done):
        for c in range(x.shape[0]):
            if done[c]:
                continue
            w = e.next_window(c)
            if w is None:
                e.close_input(c)
                continue
            outs[c].append(w.copy())
            done[c] = e.is_done(c)
    return outs


def test_streaming_seam_equals_offline():
    ra = _ra()
    N, f = 4096, 4.0
    x = np.stack([onp.synth_input(c, 30 * N) for c in range(2)])
    with _blur_engine(ra, N, f, 2, 9) as e:
        ref = e.stretch_host(x).copy()
    for close_first in (True, False):
        with _blur_engine(ra, N, f, 2, 9, max_batch_hops=1) as e:  # batches of one window
            outs = _pull_all(e, x, close_first)
        for c in range(2):
            y = np.concatenate(outs[c])
            n = min(y.size, ref.shape[1])
            assert n >= ref.shape[1] - N and np.array_equal(y[:n], ref[c, :n]), ("seam", close_first, c)


def _ranges_equal_whole(ra, e, x, cuts):
    import torch

    xt = torch.from_numpy(x).cuda()
    whole = e.stretch_tensor(xt)
    torch.cuda.synchronize()
    e.synchronize()
    wout = e.output_len(x.shape[1]) // cuts[-1]
    parts = torch.zeros_like(whole)
    for w0, w1 in zip(cuts[:-1], cuts[1:]):
        e.stretch_device_range_ptr(xt.data_ptr(), xt.stride(0), xt.shape[1], 0, x.shape[0], w0, w1 - w0,
                                   parts[:, w0 * wout:].data_ptr(), parts.stride(0), (w1 - w0) * wout)
    e.synchronize()
    return whole.cpu().numpy(), parts.cpu().numpy()


def test_device_ranges_equal_offline():
    ra = _ra()
    N, f = 4096, 4.0
    x = np.stack([onp.synth_input(c, 30 * N) for c in range(2)])
    with _blur_engine(ra, N, f, 2, 9) as e:
        wins = e.output_len(x.shape[1]) // int(e.params.window_out_len)
        whole, parts = _ranges_equal_whole(ra, e, x, [0, 1, wins // 3 + 2, wins])
        ref = e.stretch_host(x).copy()
    assert np.array_equal(whole, ref) and np.array_equal(parts, ref)


def test_host_pipeline_chunks_equal_the_device_job():
    import torch

    ra = _ra()
    N, f = 4096, 4.0
    # a host-pipeline chunk is 16 MiB of output per channel: 13 M output samples are four of them
    L = 3_300_000
    x = np.random.default_rng(5).uniform(-0.5, 0.5, (2, L)).astype(np.float32)
    with _blur_engine(ra, N, f, 2, 11) as e:
        n_out = e.output_len(L)
        assert n_out * 4 > 3 * (16 << 20)
        ref = e.stretch_tensor(torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.array_equal(e.stretch_host(x), ref), "pageable rows"
        xp, yp = ra.pinned_empty((2, L)), ra.pinned_empty((2, n_out))
        xp[:] = x
        assert np.array_equal(e.stretch_host(xp, out=yp), ref), "pinned rows"


def test_multi_engine_equals_offline():
    import torch

    ra = _ra()
    N, f = 4096, 4.0
    x = np.stack([onp.synth_input(c, 30 * N) for c in range(2)])
    with _blur_engine(ra, N, f, 2, 9) as e:
        ref = e.stretch_host(x).copy()
    code = ra.compile_device_kernel(example("blur.hip", 3))
    n_have = ra._lib.lib().rc_device_count()
    lists = [[0, 0]]
    first = device_lists(max(2, min(n_have, 3)), n_have)[-1]  # the spread list where the box has several GPUs
    if first not in lists:
        lists.append(first)
    for devs in lists:
        with ra.MultiEngine(devs, window_len=N, factor=f, channels=2, seed=9) as m:
            m.load_device_kernel(code)
            m.set_device_kernel_params(W4)
            assert np.array_equal(m.stretch_host(x), ref), ("multi host", devs)
            xt = torch.from_numpy(x).cuda(0)
            assert np.array_equal(m.stretch_tensor(xt).cpu().numpy(), ref), ("multi device", devs)
            m.set_staging(True)
            assert np.array_equal(m.stretch_tensor(xt).cpu().numpy(), ref), ("multi device, staged", devs)


def test_a_call_of_several_chunks_equals_its_ranges():
    """Long path, N = 131072, stereo: the engine's 1 GiB of scratch holds about 170 hops per chunk
    (1 GiB / (2 x (20 N + 8 x 65536) bytes)), so 400 hops per channel cross two chunk boundaries inside one call.
    Ranges of 70 windows (140 hops) are single chunks whose halos are recomputed at other hops."""
    ra = _ra()
    N, f = 131072, 4.0
    L = 400 * (N // 8) + N
    x = np.random.default_rng(7).uniform(-0.5, 0.5, (2, L)).astype(np.float32)
    with _blur_engine(ra, N, f, 2, 13) as e:
        hpw = int(e.params.hops_per_window)
        wins = e.output_len(L) // int(e.params.window_out_len)
        assert wins * hpw >= 400 and 70 * hpw <= 160
        cuts = list(range(0, wins, 70)) + [wins]
        whole, parts = _ranges_equal_whole(ra, e, x, cuts)
    assert rms(whole) > 1e-3
    assert np.array_equal(whole, parts)


# ---- 4. hot swap in an open stream ------------------------------------------------------------------------------------
def test_hot_swap_of_the_depth_in_an_open_stream():
    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c, 60 * N) for c in range(2)])
    blur = ra.compile_device_kernel(example("blur.hip", 3))
    x2 = ra.compile_device_kernel(X2)
    assert ra.device_kernel_history(blur) == 3 and ra.device_kernel_history(x2) == 0
    ref_blur = _job(ra, x, N, f, 1, 4, src=example("blur.hip", 3), params=W4)
    ref_x2 = _job(ra, x, N, f, 1, 4, src=X2)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=4, max_batch_hops=1) as e:
        wout = int(e.params.window_out_len)
        e.load_device_kernel(x2)
        e.set_device_kernel_params(W4)
        for c in range(2):
            e.push_input(c, x[c])  # the stream stays open
        w = 0
        for code, ref, count in ((x2, ref_x2, 7), (blur, ref_blur, 9), (x2, ref_x2, 5), (blur, ref_blur, 6)):
            e.load_device_kernel(code)
            for _ in range(count):
                for c in range(2):
                    got = e.next_window(c)
                    assert got is not None, w
                    assert np.array_equal(got, ref[c, w * wout:(w + 1) * wout]), (w, c)
                w += 1


# ---- 5. single frame ---------------------------------------------------------------------------------------------------
def test_single_frame_has_no_past():
    ra = _ra()
    N = 4096
    s = onp.synth_input(1, N)
    with ra.Engine(window_len=N, channels=2, seed=3) as e:
        e.set_device_kernel_source(example("delay.hip", 1))
        assert np.all(e.resynth(1, 7, s) == 0.0)
        e.set_device_kernel_source(example("blur.hip", 3))
        e.set_device_kernel_params(W4)
        y = e.resynth(1, 7, s)
    yo = oc.ReFFT(oc.hanning(N)).resynth(s, oc.phase_key(3, 1, 7), kernel=lambda t, sp: sp * np.float32(W4[0]))
    assert rms(yo) > 1e-3
    assert_close(y, yo, "resynth, weight 0 only")


# ---- 6. launch count ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,f", PATHS)
def test_the_halo_adds_no_launch(N, f):
    import torch

    ra = _ra()
    x = np.stack([onp.synth_input(c, 12 * N) for c in range(2)])
    xt = torch.from_numpy(x).cuda()
    launches = {}
    for name, src in (("x2", X2), ("blur3", example("blur.hip", 3))):
        with ra.Engine(window_len=N, factor=f, channels=2, seed=1) as e:
            e.set_device_kernel_source(src)
            e.set_device_kernel_params(W4)
            e.stretch_tensor(xt)
            torch.cuda.synchronize()
            e.synchronize()
            launches[name] = e.last_kernel_stats()[2]
    assert launches["blur3"] == launches["x2"] > 0, launches


# ---- 7. CLI --------------------------------------------------------------------------------------------------------------
def test_cli_blur_equals_python(tmp_path):
    ra = _ra()
    x = np.stack([onp.synth_input(c, 120_000) for c in range(2)])
    wav_in, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    write_wav(wav_in, x, 44100, "f32")
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    r = subprocess.run([cli, "-i", wav_in, "-o", wav_out, "-w", "4096", "-f", "4", "--seed", "6", "--device-kernel-src",
                        os.path.join(EXAMPLES, "blur.hip"), "--dk-params", ",".join(str(w) for w in W4)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    _, got = read_wav_f32(wav_out)
    want = _job(ra, x, 4096, 4.0, 1, 6, src=example("blur.hip"), params=W4)
    assert rms(want) > 1e-3
    assert np.array_equal(got[:, :want.shape[1]], want)

"""User device kernels on the MI355X (include/rocoder_hip.h, rc_dk_compile / rc_engine_load_device_kernel): HIP source
compiled at run time and run between analysis and synthesis. Every check is against the oracle driven by the same
function as a host kernel, against the curated device kernels bit for bit, or against another entry point bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from oracle import cbind as oc
from oracle import oracle_np as onp
from wavutil import read_wav_f32, write_wav

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4

X2 = ("__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
      "{ float2 x = X[j]; return make_float2(2.f * x.x, 2.f * x.y); }")


def shift_src(s):  # RC_DK_SHIFT written as a user kernel
    return f"""
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {{
    const uint32_t M = h.n / 2;
    const uint32_t f = j <= M ? j : h.n - j;
    const int64_t src = (int64_t)f - ({s});
    float2 y = make_float2(0.f, 0.f);
    if (src >= 0 && src <= (int64_t)M) {{
        y = X[src];
        if (j > M) y.y = -y.y;
    }}
    return y;
}}
"""


def band_src(lo, hi, gi, go):  # RC_DK_BAND written as a user kernel
    return f"""
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {{
    const uint32_t M = h.n / 2;
    const uint32_t f = j <= M ? j : h.n - j;
    const float g = (f >= {lo}u && f <= {hi}u) ? {gi!r}f : {go!r}f;
    const float2 x = X[j];
    return make_float2(x.x * g, x.y * g);
}}
"""


# gain from the hop index, the channel and param 0 (all three exactly representable)
HOP_CH_PARAM = """
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float g = h.param(0) * (1.0f + 0.25f * (float)h.channel) * (1.0f + 0.125f * (float)(h.hop % 5));
    const float2 x = X[j];
    return make_float2(x.x * g, x.y * g);
}
"""


def _ra():
    import rocoder_amd
    from rocoder_amd import _lib

    assert _lib.lib().rc_device_count() > 0, "no MI355X visible: GPU tests must not silently pass"
    return rocoder_amd


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a)))


def assert_close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, r = rms(got.astype(np.float64) - ref), rms(ref)
    assert err <= TOL and err <= TOL * r + 1e-9, f"{what}: rms_err={err:.3e} rms_ref={r:.3e}"


def _job(ra, x, N, f, p, seed, src=None, params=None, **kw):
    with ra.Engine(window_len=N, factor=f, pitch_multiple=p, channels=x.shape[0], seed=seed, **kw) as e:
        if src is not None:
            e.set_device_kernel_source(src)
        if params is not None:
            e.set_device_kernel_params(params)
        return e.stretch_host(x).copy()


# (window, factor, pitch): Hop, Big, Gen and Long paths
PATHS = [(1024, 4.0, 1), (65536, 8.0, 1), (12288, 4.0, 1), (131072, 4.0, 1)]


def test_readme_x2_is_c4_at_gpu_speed():
    ra = _ra()
    x = np.stack([onp.synth_input(c, 400_000) for c in range(2)])
    got = ra.stretch(x, window_len=16384, factor=8.0, seed=5, device_kernel_source=X2)
    ref = oc.stretch_offline(x, 16384, 8.0, 1.0, 1, seed=5, kernel=lambda t, s: s * np.float32(2.0))
    assert_close(got, ref, "x2 user kernel vs oracle")
    plain = ra.stretch(x, window_len=16384, factor=8.0, seed=5)
    assert rms(got - 2.0 * plain) <= 2e-6 * rms(plain) + 1e-9


@pytest.mark.parametrize("N,f,_p", PATHS)
@pytest.mark.parametrize("p", [1, 3, -2])
def test_user_shift_and_band_equal_curated_bit_for_bit(N, f, _p, p):
    ra = _ra()
    x = np.stack([onp.synth_input(c, 5 * N + 333) for c in range(2)])
    for s in (7, -5):
        cur = _job(ra, x, N, f, p, 17, device_kernel=("shift", s))
        usr = _job(ra, x, N, f, p, 17, src=shift_src(s))
        assert np.array_equal(cur, usr), (N, p, "shift", s)
    lo, hi = N // 64, N // 5
    cur = _job(ra, x, N, f, p, 17, device_kernel=("band", lo, hi, 1.25, 0.1))
    usr = _job(ra, x, N, f, p, 17, src=band_src(lo, hi, 1.25, 0.1))
    assert np.array_equal(cur, usr), (N, p, "band")


def _oracle_per_channel(x, N, f, p, seed, param0):
    """Per-channel oracle Stretchers whose host kernel counts its calls: call i of channel c is hop i."""
    n_out = oc.offline_output_len(x.shape[1], N, f, p)
    out = np.zeros((x.shape[0], n_out), np.float32)
    for c in range(x.shape[0]):
        calls = [0]

        def k(t, spec, c=c):
            hop = calls[0]
            calls[0] += 1
            g = np.float32(param0) * (np.float32(1.0) + np.float32(0.25) * np.float32(c)) * \
                (np.float32(1.0) + np.float32(0.125) * np.float32(hop % 5))
            return spec * np.float32(g)

        st = oc.Stretcher(channels=x.shape[0], factor=f, pitch_multiple=p, window=oc.hanning(N), seed=seed,
                          channel_index=c, kernel=k)
        st.send(x[c])
        st.close_input()
        parts = []
        while not st.is_done():
            parts.append(st.next_window())
        y = np.concatenate(parts)[:n_out]
        out[c, :y.size] = y
    return out


@pytest.mark.parametrize("N,f,p", PATHS)
def test_hop_channel_and_param_inputs(N, f, p):
    ra = _ra()
    x = np.stack([onp.synth_input(c + 3, 4 * N + 111) for c in range(2)])
    got = _job(ra, x, N, f, p, 29, src=HOP_CH_PARAM, params=[1.5])
    ref = _oracle_per_channel(x, N, f, p, 29, 1.5)
    assert_close(got, ref, f"hop/channel/param N={N}")


def test_index_reduction_is_modulo_n():
    ra = _ra()
    x = np.stack([onp.synth_input(c, 5 * 4096) for c in range(2)])
    base = _job(ra, x, 4096, 4.0, 1, 3, src=X2)
    for expr in ("(int64_t)j + 3 * (int64_t)h.n", "(int64_t)j - (int64_t)h.n"):
        src = X2.replace("X[j]", f"X[{expr}]")
        assert np.array_equal(_job(ra, x, 4096, 4.0, 1, 3, src=src), base), expr
    xg = np.stack([onp.synth_input(c, 5 * 12288) for c in range(2)])  # not a power of two: the modulo path
    base = _job(ra, xg, 12288, 4.0, 1, 3, src=X2)
    for expr in ("(int64_t)j + 3 * (int64_t)h.n", "(int64_t)j - (int64_t)h.n"):
        assert np.array_equal(_job(ra, xg, 12288, 4.0, 1, 3, src=X2.replace("X[j]", f"X[{expr}]")), base), expr


def test_single_hop_resynth_matches_oracle():
    ra = _ra()
    N = 4096
    w = oc.hanning(N)
    s = onp.synth_input(1, N)
    with ra.Engine(window_len=N, channels=2, seed=3) as e:
        e.set_device_kernel_source(HOP_CH_PARAM)
        e.set_device_kernel_params([0.75])
        y = e.resynth(1, 7, s)
    g = np.float32(0.75) * np.float32(1.25) * (np.float32(1.0) + np.float32(0.125) * np.float32(7 % 5))
    yo = oc.ReFFT(w).resynth(s, oc.phase_key(3, 1, 7), kernel=lambda t, sp: sp * np.float32(g))
    assert_close(y, yo, "resynth")


def test_seam_and_multi_equal_offline():
    import torch

    ra = _ra()
    N, f = 4096, 4.0
    x = np.stack([onp.synth_input(c, 30 * N) for c in range(2)])
    ref = _job(ra, x, N, f, 1, 9, src=HOP_CH_PARAM, params=[1.25])
    code = ra.compile_device_kernel(HOP_CH_PARAM)
    for close_first in (True, False):
        with ra.Engine(window_len=N, factor=f, channels=2, seed=9) as e:
            e.load_device_kernel(code)
            e.set_device_kernel_params([1.25])
            outs = [[], []]
            for c in range(2):
                e.push_input(c, x[c])
                if close_first:
                    e.close_input(c)
            done = [False, False]
            while not all(done):
                for c in range(2):
                    if done[c]:
                        continue
                    w = e.next_window(c)
                    if w is None:
                        e.close_input(c)
                        continue
                    outs[c].append(w)
                    done[c] = e.is_done(c)
        for c in range(2):
            y = np.concatenate(outs[c])
            n = min(y.size, ref.shape[1])
            assert n >= ref.shape[1] - N and np.array_equal(y[:n], ref[c, :n]), ("seam", close_first, c)
    n_dev = _ra()._lib.lib().rc_device_count()
    devs = [0, 0] if n_dev < 2 else [0, 1, 0]
    with ra.MultiEngine(devs, window_len=N, factor=f, channels=2, seed=9) as m:
        m.load_device_kernel(code)
        m.set_device_kernel_params([1.25])
        assert np.array_equal(m.stretch_host(x), ref), "multi host"
        xt = torch.from_numpy(x).cuda(0)
        assert np.array_equal(m.stretch_tensor(xt).cpu().numpy(), ref), "multi device"


def test_hot_swap_and_lifetime():
    import torch

    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c, 200 * N) for c in range(2)])
    A, B = X2, shift_src(3)
    fresh_a, fresh_b = _job(ra, x, N, f, 1, 4, src=A), _job(ra, x, N, f, 1, 4, src=B)
    ca, cb = ra.compile_device_kernel(A), ra.compile_device_kernel(B)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=4) as e:
        for code, want in ((ca, fresh_a), (cb, fresh_b), (ca, fresh_a)):
            e.load_device_kernel(code)
            assert np.array_equal(e.stretch_host(x), want)
        # bad bytes are refused before the runtime sees them; A stays loaded
        for bad in (b"\x00" * 4096, ca[:18] + b"\x00\x00" + ca[20:], ca[:48] + bytes([0x4c]) + ca[49:]):
            with pytest.raises(ra.RocoderError) as ei:
                e.load_device_kernel(bad)
            assert ei.value.code == -1
        assert np.array_equal(e.stretch_host(x), fresh_a)
        # B loaded right after an asynchronous call on a side stream: that call still runs A
        xt = torch.from_numpy(x).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = e.stretch_tensor(xt, stream=side.cuda_stream)
        e.load_device_kernel(cb)
        side.synchronize()
        assert np.array_equal(out.cpu().numpy(), fresh_a)
        assert np.array_equal(e.stretch_host(x), fresh_b)
        # params from the next call on, equal to the constants written in
        e.load_device_kernel(ra.compile_device_kernel(HOP_CH_PARAM))
        e.set_device_kernel_params([0.5])
        p05 = e.stretch_host(x).copy()
        e.set_device_kernel_params([2.0])
        p2 = e.stretch_host(x).copy()
        with pytest.raises(ra.RocoderError):
            e.set_device_kernel_params([1.0] * 17)
    assert np.array_equal(p05, _job(ra, x, N, f, 1, 4, src=HOP_CH_PARAM.replace("h.param(0)", "0.5f")))
    assert np.array_equal(p2, _job(ra, x, N, f, 1, 4, src=HOP_CH_PARAM.replace("h.param(0)", "2.0f")))
    for kw in (dict(kernel=lambda t, s: s), dict(device_kernel=("gain", 2.0))):
        with ra.Engine(window_len=N, factor=f, channels=2, seed=4, **kw) as e:
            with pytest.raises(ra.RocoderError) as ei:
                e.load_device_kernel(ca)
            assert ei.value.code == -1


def test_cli_device_kernel_src(tmp_path):
    ra = _ra()
    x = np.stack([onp.synth_input(c, 120_000) for c in range(2)])
    wav_in, wav_out, k = str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), tmp_path / "k.hip"
    write_wav(wav_in, x, 44100, "f32")
    k.write_text(HOP_CH_PARAM)
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    base = [cli, "-i", wav_in, "-o", wav_out, "-w", "4096", "-f", "4", "--seed", "6"]
    r = subprocess.run(base + ["--device-kernel-src", str(k), "--dk-params", "2"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    _, got = read_wav_f32(wav_out)
    want = _job(ra, x, 4096, 4.0, 1, 6, src=HOP_CH_PARAM, params=[2.0])
    assert np.array_equal(got[:, :want.shape[1]], want)
    k.write_text("int x\n" + HOP_CH_PARAM)  # does not compile: the log is printed, the run goes on without a kernel
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    _, plain = read_wav_f32(wav_out)
    r = subprocess.run(base + ["--device-kernel-src", str(k)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "k.hip:2" in r.stderr and "error" in r.stderr
    _, got = read_wav_f32(wav_out)
    assert np.array_equal(got, plain)

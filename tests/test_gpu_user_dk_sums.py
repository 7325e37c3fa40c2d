"""User device kernels with whole-hop sums (RC_SUMS, rc_sum_term, X.sum(i)) on the MI355X.

1. The value of a sum on single frames (rc_engine_resynth): two sums whose double accumulation is exact, two against the
   value computed in float64 from rc_engine_forward_fft of the same frame. 2. Smooth kernels against the oracle by the
   two-pass method of tests/test_gpu_user_dk_channels.py. 3. Bit-for-bit identities between GPU jobs (seam, ranges,
   rc_multi, hot swap). 4. The zero rules. 5. More than 32768 rows in one pass. 6. The CLI.

Every test here compiles a source that declares RC_SUMS (or, for the undeclared zero rule, calls X.sum), which the code
before this feature rejects."""
import os
import subprocess
import sys

import numpy as np
import pytest

from multi_devices import device_lists
from oracle import oracle_np as onp
from test_gpu_user_dk_channels import (EXAMPLES, HEAD, IDENT, ROOT, X2, ZERO, _case_input, _job, _oracle_cross, _pull_all, _ra,
                                       assert_close, example, rms)
from wavutil import read_wav_f32, write_wav

pytestmark = pytest.mark.gpu

TERM = "__device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i) "
ENERGY = TERM + "{ float2 x = X[j]; return x.x * x.x + x.y * x.y; }\n"
GAIN = HEAD + "{ float2 x = X[j]; float g = EXPR; return make_float2(g * x.x, g * x.y); }"

# own, previous hop's and the other channel's energy in one smooth gain (tests 2 and 3)
MIX = ("#define RC_SUMS 1\n#define RC_HISTORY 1\n#define RC_CROSS_CHANNEL 1\n" + ENERGY + HEAD +
       "{ float2 x = X[j]; float s0 = X.sum(0), sp = X.past(1).sum(0), sc = X.channel(1 - h.channel).sum(0), p = h.param(0);\n"
       "  float g = (s0 + p) / (((s0 + sp) + sc) + p); return make_float2(g * x.x, g * x.y); }")


# ---- 1. the value of a sum, on single frames -------------------------------------------------------------------------
# sum i passes X[j] where |X.sum(i) - param(0)| <= param(1), i = param(2)
CHECK = ("#define RC_SUMS 4\n" + TERM +
         "{ float2 x = X[j]; float e = x.x * x.x + x.y * x.y;\n"
         "  return i == 0 ? 1.f : i == 1 ? (float)j : i == 2 ? e : (float)j * e; }\n" + HEAD +
         "{ float s = X.sum((uint32_t)h.param(2));\n"
         "  return fabsf(s - h.param(0)) <= h.param(1) ? X[j] : make_float2(0.f, 0.f); }")


@pytest.mark.parametrize("N", [32, 256, 1000, 1024, 16384, 32768, 131072])
def test_the_value_of_a_sum_on_a_single_frame(N):
    ra = _ra()
    frame = onp.synth_input(3, N)
    with ra.Engine(window_len=N, channels=2, seed=3) as e:
        X = e.forward_fft(frame).astype(np.complex128)
        e.set_device_kernel_source(IDENT)
        ident = e.resynth(1, 5, frame)
        assert rms(ident) > 1e-3
        energy = X.real * X.real + X.imag * X.imag
        j = np.arange(N, dtype=np.float64)
        # (expected value, tolerance): exact where the double accumulation is exact, else 1e-5 of the sum of |term|: a
        # fused multiply-add in the term and the float32 rounding of the spectra
        want = [(float(np.float32(N)), 0.0), (float(np.float32(N * (N - 1) // 2)), 0.0),
                (float(energy.sum()), 1e-5 * float(energy.sum())), (float((j * energy).sum()), 1e-5 * float((j * energy).sum()))]
        e.set_device_kernel_source(CHECK)
        for i, (value, tol) in enumerate(want):
            e.set_device_kernel_params([value, tol, float(i)])
            got = e.resynth(1, 5, frame)
            print(f"N={N} sum {i}: expected {value!r} tol {tol!r} equal={np.array_equal(got, ident)}")
            assert np.array_equal(got, ident), (N, i, value)
            # negative control: the expected value off by 1e-3 relative
            e.set_device_kernel_params([value * (1.0 + 1e-3), tol, float(i)])
            assert np.all(e.resynth(1, 5, frame) == 0.0), (N, i, "control")


# ---- 2. against the oracle ----------------------------------------------------------------------------------------------
def _sum32(terms):
    """The sum as the pass forms it: float32 terms, float64 accumulation, one rounding."""
    return np.float32(np.sum(np.asarray(terms, np.float32).astype(np.float64)))


def _energy(x):
    return x.real * x.real + x.imag * x.imag  # float32


def auto_gain_fn(p0, p1):
    p0, p1 = np.float32(p0), np.float32(p1)

    def fn(rec, c, i):  # examples/kernels/auto_gain.hip
        x = rec[c][i]
        g = p0 / np.sqrt(_sum32(_energy(x)) / np.float32(x.size) + p1)
        return np.float32(g) * x

    return fn


def centroid_tilt_fn(p0):
    p0 = np.float32(p0)

    def fn(rec, c, i):  # examples/kernels/centroid_tilt.hip
        x = rec[c][i]
        n = x.size
        jf = np.minimum(np.arange(n), n - np.arange(n)).astype(np.float32)
        e = _energy(x)
        s0, s1 = _sum32(e), _sum32(jf * e)
        cen = s1 / s0 if s0 > 0 else np.float32(0)
        u = jf / (p0 * cen + np.float32(1))
        return (np.float32(1) / (np.float32(1) + u * u)) * x

    return fn


def mix_fn(p):
    p = np.float32(p)

    def fn(rec, c, i):  # MIX
        s0 = _sum32(_energy(rec[c][i]))
        sp = _sum32(_energy(rec[c][i - 1])) if i >= 1 else np.float32(0)
        sc = _sum32(_energy(rec[1 - c][i])) if 0 <= 1 - c < len(rec) else np.float32(0)
        return ((s0 + p) / (((s0 + sp) + sc) + p)) * rec[c][i]

    return fn


# (source, params(N), host twin(N)); a windowed hop of the test signal has magnitudes of the order N / 4
SMOOTH = {"auto_gain": (lambda: example("auto_gain.hip"), lambda N: [N / 8.0, 1.0], lambda N: auto_gain_fn(N / 8.0, 1.0)),
          "centroid_tilt": (lambda: example("centroid_tilt.hip"), lambda N: [2.0], lambda N: centroid_tilt_fn(2.0)),
          "mix": (lambda: MIX, lambda N: [float(N)], lambda N: mix_fn(float(N)))}


@pytest.mark.parametrize("kernel", sorted(SMOOTH))  # (varies fastest: the kernels of a case share pass 1)
@pytest.mark.parametrize("p", [1, -2])
@pytest.mark.parametrize("N,f", [(1024, 4.0), (32768, 8.0), (1000, 4.0), (131072, 4.0)])
def test_smooth_kernels_with_sums_match_the_oracle(N, f, p, kernel):
    ra = _ra()
    src, params, make = SMOOTH[kernel]
    x = _case_input(ra, N, f, p, 2)
    got = _job(ra, x, N, f, p, 23, src=src(), params=params(N))
    ref = _oracle_cross(x, N, f, p, 23, make(N))
    assert rms(ref) > 1e-3, "the case must not be silence"
    assert_close(got, ref, f"{kernel} N={N} p={p}")
    assert not np.array_equal(got, _job(ra, x, N, f, p, 23, src=IDENT))


# ---- 3. bit-for-bit identities between GPU jobs ----------------------------------------------------------------------
N3, F3 = 2048, 4.0
SEAMS = {"level_gate": (lambda: example("level_gate.hip"), [1.0]), "mix": (lambda: MIX, [float(N3)])}


def _engine3(ra, kernel, ch, **kw):
    src, params = SEAMS[kernel]
    e = ra.Engine(window_len=N3, factor=F3, channels=ch, seed=9, **kw)
    e.load_device_kernel(ra.compile_device_kernel(src()))
    e.set_device_kernel_params(params)
    return e


def _x3(ch):
    return np.stack([onp.synth_input(c + 1, 30 * N3) for c in range(ch)])


@pytest.mark.parametrize("kernel", sorted(SEAMS))
def test_streaming_seam_equals_offline(kernel):
    ra = _ra()
    x = _x3(2)
    with _engine3(ra, kernel, 2) as e:
        ref = e.stretch_host(x).copy()
    assert rms(ref) > 1e-3 and not np.array_equal(ref, _job(ra, x, N3, F3, 1, 9, src=IDENT))
    for close_first in (True, False):
        with _engine3(ra, kernel, 2, max_batch_hops=1) as e:  # batches of one window
            outs = _pull_all(e, x, close_first)
        for c in range(2):
            y = np.concatenate(outs[c])
            n = min(y.size, ref.shape[1])
            assert n >= ref.shape[1] - N3 and np.array_equal(y[:n], ref[c, :n]), ("seam", close_first, c)


@pytest.mark.parametrize("kernel", sorted(SEAMS))
def test_channel_subsets_and_window_cuts_equal_offline(kernel):
    import torch

    ra = _ra()
    x = _x3(3)
    with _engine3(ra, kernel, 3) as e:
        ref = e.stretch_host(x).copy()
        assert rms(ref) > 1e-3
        xt = torch.from_numpy(x).cuda()
        wout = int(e.params.window_out_len)
        wins = ref.shape[1] // wout
        cuts = [0, 1, wins // 3 + 2, wins]
        for ch_first, ch_count in ((0, 3), (1, 1), (0, 2), (2, 1)):
            parts = torch.zeros((3, ref.shape[1]), device="cuda")
            for w0, w1 in zip(cuts[:-1], cuts[1:]):
                e.stretch_device_range_ptr(xt.data_ptr(), xt.stride(0), xt.shape[1], ch_first, ch_count, w0, w1 - w0,
                                           parts[ch_first:, w0 * wout:].data_ptr(), parts.stride(0), (w1 - w0) * wout)
            e.synchronize()
            got = parts.cpu().numpy()
            assert np.array_equal(got[ch_first:ch_first + ch_count], ref[ch_first:ch_first + ch_count]), (ch_first, ch_count)


@pytest.mark.parametrize("kernel", sorted(SEAMS))
def test_multi_engine_equals_offline(kernel):
    import torch

    ra = _ra()
    x = _x3(2)
    with _engine3(ra, kernel, 2) as e:
        ref = e.stretch_host(x).copy()
    src, params = SEAMS[kernel]
    code = ra.compile_device_kernel(src())
    n_have = ra._lib.lib().rc_device_count()
    lists = [[0, 0], [0, 0, 0]]
    first = device_lists(max(2, min(n_have, 3)), n_have)[-1]  # the spread list where the box has several GPUs
    if first not in lists:
        lists.append(first)
    for devs in lists:
        with ra.MultiEngine(devs, window_len=N3, factor=F3, channels=2, seed=9) as m:
            m.load_device_kernel(code)
            m.set_device_kernel_params(params)
            assert np.array_equal(m.stretch_host(x), ref), ("multi host", devs)
            xt = torch.from_numpy(x).cuda(0)
            assert np.array_equal(m.stretch_tensor(xt).cpu().numpy(), ref), ("multi device", devs)
            m.set_staging(True)
            assert np.array_equal(m.stretch_tensor(xt).cpu().numpy(), ref), ("multi device, staged", devs)


def test_hot_swap_between_an_undeclared_and_a_declared_kernel():
    ra = _ra()
    x = np.stack([onp.synth_input(c, 60 * N3) for c in range(2)])
    gate = ra.compile_device_kernel(example("level_gate.hip"))
    x2 = ra.compile_device_kernel(X2)
    assert ra.device_kernel_sums(gate) == 1 and ra.device_kernel_history(gate) == 1 and ra.device_kernel_sums(x2) == 0
    ref_gate = _job(ra, x, N3, F3, 1, 4, src=example("level_gate.hip"), params=[1.0])
    ref_x2 = _job(ra, x, N3, F3, 1, 4, src=X2)
    with ra.Engine(window_len=N3, factor=F3, channels=2, seed=4, max_batch_hops=1) as e:
        wout = int(e.params.window_out_len)
        e.load_device_kernel(x2)
        e.set_device_kernel_params([1.0])
        for c in range(2):
            e.push_input(c, x[c])  # the stream stays open
        w = 0
        for code, ref, count in ((x2, ref_x2, 7), (gate, ref_gate, 9), (x2, ref_x2, 5), (gate, ref_gate, 6)):
            e.load_device_kernel(code)
            for _ in range(count):
                for c in range(2):
                    got = e.next_window(c)
                    assert got is not None, w
                    assert np.array_equal(got, ref[c, w * wout:(w + 1) * wout]), (w, c)
                w += 1


# ---- 4. zero rules -------------------------------------------------------------------------------------------------------
ZEROS = {
    "sum_beyond_S": "#define RC_SUMS 1\n" + ENERGY + GAIN.replace("EXPR", "X.sum(1)"),
    "past_beyond_history": "#define RC_SUMS 1\n#define RC_HISTORY 1\n" + ENERGY + GAIN.replace("EXPR", "X.past(2).sum(0)"),
    "hop_before_the_stream": "#define RC_SUMS 1\n#define RC_HISTORY 1\n" + ENERGY +
                             GAIN.replace("EXPR", "h.hop == 0 ? X.past(1).sum(0) : 0.f"),
    "channel_outside": "#define RC_SUMS 1\n#define RC_CROSS_CHANNEL 1\n" + ENERGY +
                       GAIN.replace("EXPR", "X.channel(h.channels + 3).sum(0)"),
    "undeclared": GAIN.replace("EXPR", "X.sum(0)"),
    "sum_inside_the_term": "#define RC_SUMS 1\n" + TERM + "{ return X.sum(0); }\n" + GAIN.replace("EXPR", "X.sum(0)"),
}
CONTROLS = {
    "own": "#define RC_SUMS 1\n" + ENERGY + GAIN.replace("EXPR", "1e-9f * X.sum(0)"),
    "past": "#define RC_SUMS 1\n#define RC_HISTORY 1\n" + ENERGY + GAIN.replace("EXPR", "h.hop == 1 ? 1e-9f * X.past(1).sum(0) : 0.f"),
    "channel": "#define RC_SUMS 1\n#define RC_CROSS_CHANNEL 1\n" + ENERGY +
               GAIN.replace("EXPR", "1e-9f * X.channel(1 - h.channel).sum(0)"),
}


def test_sums_outside_the_declaration_are_zero():
    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c + 1, 9 * N) for c in range(2)])
    zero = _job(ra, x, N, f, 1, 5, src=ZERO)
    for name, src in sorted(ZEROS.items()):
        assert np.array_equal(_job(ra, x, N, f, 1, 5, src=src), zero), name
    for name, src in sorted(CONTROLS.items()):
        y = _job(ra, x, N, f, 1, 5, src=src)
        assert np.all(np.isfinite(y)) and not np.array_equal(y, zero), name


# ---- 5. more than 32768 rows in one pass ---------------------------------------------------------------------------------
def test_more_than_32768_rows_in_one_pass():
    ra = _ra()
    N, f = 32, 4.0
    x = np.stack([onp.synth_input(c + 1, 80_000) for c in range(2)])
    gain = "1.f / sqrtf(SUM / 32.f + 1.f)"
    declared = "#define RC_SUMS 1\n" + ENERGY + GAIN.replace("EXPR", gain.replace("SUM", "X.sum(0)"))
    loop = HEAD + ("{ double s = 0.0; for (uint32_t b = 0; b < 32u; ++b) { float2 q = X[b]; s += (double)(q.x * q.x + q.y * q.y); }\n"
                   "  float2 x = X[j]; float g = EXPR; return make_float2(g * x.x, g * x.y); }").replace(
                       "EXPR", gain.replace("SUM", "(float)s"))
    with ra.Engine(window_len=N, factor=f, channels=2, seed=11) as e:
        rows = 2 * (x.shape[1] // int(e.params.sample_step_len))
        assert rows > 32768, rows
    got = _job(ra, x, N, f, 1, 11, src=declared)
    ref = _job(ra, x, N, f, 1, 11, src=loop)
    assert rms(ref) > 1e-3 and rms(got) > 1e-3
    assert not np.array_equal(ref, _job(ra, x, N, f, 1, 11, src=IDENT))
    worst = float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref.astype(np.float64)), 1e-300)))
    print(f"rows={rows} worst relative difference {worst:.3e} equal={np.array_equal(got, ref)}")
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 1e-6 * np.abs(ref.astype(np.float64)))


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------
def _compile_as_the_cli_does(path):
    """The code object of a kernel file from the compiler the CLI uses. The CLI compiles with the hiprtc that lies next to
    the system's HIP runtime; this process has PyTorch loaded and compiles with the hiprtc PyTorch bundles (rocoder_amd/
    _lib.py), another build, which lowers sqrtf to other instructions: the two code objects of auto_gain.hip differ, and
    their gains differ by one ulp in a few hops. The identity under test is between two runs of ONE code object, so the
    Python job takes its code object from a child interpreter that, like the CLI, never loads PyTorch."""
    child = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, sys.argv[1]); import rocoder_amd as ra; "
             "sys.stdout.buffer.write(ra.compile_device_kernel(open(sys.argv[2]).read()))")
    r = subprocess.run([sys.executable, "-c", child, ROOT, path], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout[:4] == b"\x7fELF", r.stderr[-2000:]
    return r.stdout


def test_cli_auto_gain_equals_python(tmp_path):
    ra = _ra()
    x = np.stack([onp.synth_input(c, 120_000) for c in range(2)])
    wav_in, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    write_wav(wav_in, x, 44100, "f32")
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    src = os.path.join(EXAMPLES, "auto_gain.hip")
    r = subprocess.run([cli, "-i", wav_in, "-o", wav_out, "-w", "4096", "-f", "4", "--seed", "6", "--device-kernel-src", src,
                        "--dk-params", "8,1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "INFO Got new device kernel (history: 0 earlier hops, 1 whole-hop sums)" in r.stderr, r.stderr[-2000:]
    _, got = read_wav_f32(wav_out)
    code = _compile_as_the_cli_does(src)
    assert ra.device_kernel_sums(code) == 1
    with ra.Engine(window_len=4096, factor=4.0, channels=2, seed=6) as e:
        e.load_device_kernel(code)
        e.set_device_kernel_params([8.0, 1.0])
        want = e.stretch_host(x).copy()
    assert rms(want) > 1e-3 and not np.array_equal(want, _job(ra, x, 4096, 4.0, 1, 6, src=IDENT))
    assert np.array_equal(got[:, :want.shape[1]], want)

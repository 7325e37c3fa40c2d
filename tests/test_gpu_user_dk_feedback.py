"""User device kernels that read their own earlier outputs (RC_FEEDBACK, X.out(d)) on the MI355X.

1. Bit for bit against a history kernel that computes the same thing from the analysis spectra. 2. Smooth recursions against
the oracle with a stateful Python kernel per channel (tests/test_gpu_user_dk_channels.py: _oracle_channel, assert_close).
3. Bit-for-bit identities between GPU jobs (seam, ranges, channel subsets, the host-form entries, the two launch shapes,
a repeated job). 4. The order rule and the refusals. 5. The zero rules. 6. The CLI.

Every test here compiles a source that declares RC_FEEDBACK or calls X.out, which the code before this feature rejects."""
import os
import subprocess

import numpy as np
import pytest

from oracle import cbind as oc
from oracle import oracle_np as onp
from test_gpu_user_dk_channels import (EXAMPLES, HEAD, IDENT, ROOT, X2, ZERO, _case_input, _job, _oracle_channel, _pull_all, _ra,
                                       assert_close, example, rms)
from test_gpu_user_dk_sums import _compile_as_the_cli_does
from wavutil import read_wav_f32, write_wav

pytestmark = pytest.mark.gpu

# 0.5 X[j] + 0.3 out(1)[j + 1] - 0.2 out(2)[j - 1]
TWO_TAP = ("#define RC_FEEDBACK 2\n" + HEAD +
           "{ float2 x = X[j]; float2 a = X.out(1)[(int64_t)j + 1]; float2 b = X.out(2)[(int64_t)j - 1];\n"
           "  return make_float2(0.5f * x.x + 0.3f * a.x - 0.2f * b.x, 0.5f * x.y + 0.3f * a.y - 0.2f * b.y); }")


# ---- 1. bit for bit against a history kernel ---------------------------------------------------------------------------
def _pair(F, which):
    r = f"uint32_t r = (uint32_t)(h.hop % {F + 1}u); "
    if which == "A":  # a chain of out(1): hop k reads hop k - 1, shifted by a bin each time
        fb = "{ " + r + "if (r == 0) return X[j]; return X.out(1)[(int64_t)j + 1]; }"
        hist = "{ " + r + "return X.past(r)[(int64_t)j + r]; }"
    else:  # out(r): straight back to the hop that passed
        fb = "{ " + r + "if (r == 0) return X[j]; return X.out(r)[j]; }"
        hist = "{ " + r + "return X.past(r)[j]; }"
    return f"#define RC_FEEDBACK {F}\n" + HEAD + fb, f"#define RC_HISTORY {F}\n" + HEAD + hist


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("p", [1, -2])
@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("N", [32, 1024, 1000, 32768, 131072])
def test_feedback_equals_its_history_twin_bit_for_bit(N, F, p, which):
    ra = _ra()
    x = _case_input(ra, N, 4.0, p, 2)
    fb, hist = _pair(F, which)
    got = _job(ra, x, N, 4.0, p, 17, src=fb)
    ref = _job(ra, x, N, 4.0, p, 17, src=hist)
    assert rms(ref) > 1e-3 and not np.array_equal(ref, _job(ra, x, N, 4.0, p, 17, src=IDENT))
    assert np.array_equal(got, ref)


def test_feedback_across_a_chunk_edge_of_a_job():
    """N = 131072, two channels: run_hops cuts the job into chunks of at most 1 GiB of scratch, at 20 N bytes of spectra and
    samples per hop and channel and the path's work buffer - fewer than 205 hops. 260 hops cross an edge; the launch count
    says so: a chunk costs a fixed number of launches beside one per hop (the per-hop shape at this N), which a one-chunk
    job of 8 hops gives."""
    import torch

    ra = _ra()
    N, f, F = 131072, 4.0, 4
    fb, hist = _pair(F, "A")
    step = int(ra.derive_params(window_len=N, factor=f).sample_step_len)
    chunk_bound = (1024 << 20) // (N * 20 * 2)
    assert chunk_bound < 260

    def run(src, hops):
        L = N + (hops - 1) * step
        xt = torch.from_numpy(np.stack([onp.synth_input(c + 1, L) for c in range(2)])).cuda()
        with ra.Engine(window_len=N, factor=f, channels=2, seed=17) as e:
            e.set_device_kernel_source(src)
            y = e.stretch_tensor(xt)
            e.synchronize()
            _, n_hops, launches = e.last_kernel_stats()
            return y.cpu().numpy(), n_hops // 2, launches

    _, h_small, l_small = run(fb, 8)
    per_chunk = l_small - h_small
    assert per_chunk > 0
    got, h_big, l_big = run(fb, 260)
    ref, _, _ = run(hist, 260)
    chunks = (l_big - h_big) / per_chunk
    print(f"hops {h_small} -> {l_small} launches; hops {h_big} -> {l_big} launches: {chunks} chunks")
    assert h_big >= 260 and chunks == int(chunks) and chunks >= 2
    assert rms(ref) > 1e-3 and np.array_equal(got, ref)


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------
def smooth_kernel(a):
    a = np.float32(a)
    b = np.float32(1) - a
    prev = [None]

    def k(t, spec):  # examples/kernels/smooth.hip
        x = np.asarray(spec, np.complex64)
        y = x * b if prev[0] is None else (prev[0] * a + x * b).astype(np.complex64)
        prev[0] = y.astype(np.complex64)
        return prev[0]

    return k


def two_tap_kernel():
    outs = []

    def k(t, spec):  # TWO_TAP
        x = np.asarray(spec, np.complex64)
        y = np.float32(0.5) * x
        if len(outs) >= 1:
            y = y + np.float32(0.3) * np.roll(outs[-1], -1)
        if len(outs) >= 2:
            y = y - np.float32(0.2) * np.roll(outs[-2], 1)
        outs.append(y.astype(np.complex64))
        del outs[:-2]
        return outs[-1]

    return k


RECURSIONS = {"smooth_0.5": (lambda: example("smooth.hip"), [0.5], lambda: smooth_kernel(0.5)),
              "smooth_0.9": (lambda: example("smooth.hip"), [0.9], lambda: smooth_kernel(0.9)),
              "two_tap": (lambda: TWO_TAP, None, two_tap_kernel)}
_IDENT = {}


@pytest.mark.parametrize("kernel", sorted(RECURSIONS))
@pytest.mark.parametrize("p", [1, -2])
@pytest.mark.parametrize("N,f", [(1024, 4.0), (32768, 8.0), (1000, 4.0), (131072, 4.0)])
def test_recursions_match_the_oracle(N, f, p, kernel):
    ra = _ra()
    src, params, make = RECURSIONS[kernel]
    x = _case_input(ra, N, f, p, 2)
    got = _job(ra, x, N, f, p, 23, src=src(), params=params)
    n_out = oc.offline_output_len(x.shape[1], N, f, p)
    ref = np.zeros((2, n_out), np.float32)
    for c in range(2):
        y = _oracle_channel(x, c, N, f, p, 23, make())[:n_out]  # (a fresh state per channel)
        ref[c, :y.size] = y
    assert rms(ref) > 1e-3, "the case must not be silence"
    assert_close(got, ref, f"{kernel} N={N} p={p}")
    if (N, f, p) not in _IDENT:
        _IDENT.clear()
        _IDENT[(N, f, p)] = _job(ra, x, N, f, p, 23, src=IDENT)
    assert not np.array_equal(got, _IDENT[(N, f, p)])


# ---- 3. bit-for-bit identities between GPU jobs ------------------------------------------------------------------------
N3, F3 = 2048, 4.0
SEAMS = {"decay": (lambda: example("decay.hip"), [0.8]), "two_tap": (lambda: TWO_TAP, [])}


def _engine3(ra, kernel, ch, **kw):
    src, params = SEAMS[kernel]
    kw.setdefault("window_len", N3)
    e = ra.Engine(factor=F3, channels=ch, seed=9, **kw)
    e.load_device_kernel(ra.compile_device_kernel(src()))
    e.set_device_kernel_params(params)
    return e


def _x3(ch, N=N3):
    return np.stack([onp.synth_input(c + 1, 30 * N) for c in range(ch)])


@pytest.mark.parametrize("kernel", sorted(SEAMS))
def test_streaming_seam_equals_offline(kernel):
    ra = _ra()
    x = _x3(2)
    with _engine3(ra, kernel, 2) as e:
        ref = e.stretch_host(x).copy()
    assert rms(ref) > 1e-3 and not np.array_equal(ref, _job(ra, x, N3, F3, 1, 9, src=IDENT))
    # closed first: the look-ahead batches of a closed job
    with _engine3(ra, kernel, 2, max_batch_hops=1) as e:
        outs = _pull_all(e, x, True)
    for c in range(2):
        y = np.concatenate(outs[c])
        n = min(y.size, ref.shape[1])
        assert n >= ref.shape[1] - N3 and np.array_equal(y[:n], ref[c, :n]), ("closed", c)
    # open, pushed in odd-sized pieces, the channels at different windows
    with _engine3(ra, kernel, 2, max_batch_hops=1) as e:
        got = [[], []]
        at = [0, 0]
        piece = [3001, 1777]
        while at[0] < x.shape[1] or at[1] < x.shape[1]:
            for c in range(2):
                if at[c] < x.shape[1]:
                    e.push_input(c, x[c, at[c]:at[c] + piece[c]])
                    at[c] += piece[c]
                while True:
                    w = e.next_window(c)
                    if w is None:
                        break
                    got[c].append(w.copy())
        for c in range(2):
            y = np.concatenate(got[c])
            assert y.size > ref.shape[1] // 2 and np.array_equal(y, ref[c, :y.size]), ("open", c)


@pytest.mark.parametrize("kernel", sorted(SEAMS))
def test_consecutive_ranges_and_channel_subsets_equal_offline(kernel):
    import torch

    ra = _ra()
    x = _x3(3)
    with _engine3(ra, kernel, 3) as e:
        ref = e.stretch_host(x).copy()
        assert rms(ref) > 1e-3
        xt = torch.from_numpy(x).cuda()
        wout = int(e.params.window_out_len)
        wins = ref.shape[1] // wout
        cuts = [0, 1, wins // 3 + 2, wins - 3, wins]  # three cuts
        for ch_first, ch_count in ((0, 3), (1, 1), (0, 2), (2, 1)):
            parts = torch.zeros((3, ref.shape[1]), device="cuda")
            for w0, w1 in zip(cuts[:-1], cuts[1:]):
                e.stretch_device_range_ptr(xt.data_ptr(), xt.stride(0), xt.shape[1], ch_first, ch_count, w0, w1 - w0,
                                           parts[ch_first:, w0 * wout:].data_ptr(), parts.stride(0), (w1 - w0) * wout)
            e.synchronize()
            got = parts.cpu().numpy()
            assert np.array_equal(got[ch_first:ch_first + ch_count], ref[ch_first:ch_first + ch_count]), (ch_first, ch_count)


@pytest.mark.parametrize("kernel", sorted(SEAMS))
def test_the_whole_job_entries_agree_and_a_restart_zeroes_the_state(kernel):
    import torch

    ra = _ra()
    x = _x3(2)
    with _engine3(ra, kernel, 2) as e:
        host = e.stretch_host(x).copy()
        assert rms(host) > 1e-3
        dev = e.stretch_tensor(torch.from_numpy(x).cuda())
        e.synchronize()
        assert np.array_equal(dev.cpu().numpy(), host), "stretch_device"
        frames = e.stretch_frames(np.ascontiguousarray(x.T))
        assert np.array_equal(frames.T, host), "frames"
        assert np.array_equal(e.stretch_host(x), host), "a second job starts from zero state"


@pytest.mark.parametrize("kernel", sorted(SEAMS))
def test_the_per_hop_shape_equals_the_loop_shape(kernel, monkeypatch):
    import torch

    from rocoder_amd import _lib

    ra = _ra()
    N = 1024
    x = _x3(2, N)
    xt = torch.from_numpy(x).cuda()
    out = {}
    with _lib.hooks_library():
        for name, diag in (("loop", None), ("per_hop", "16")):
            if diag is None:
                monkeypatch.delenv("ROCODER_DIAG", raising=False)
            else:
                monkeypatch.setenv("ROCODER_DIAG", diag)
            with _engine3(ra, kernel, 2, window_len=N) as e:
                y = e.stretch_tensor(xt)
                e.synchronize()
                out[name] = (y.cpu().numpy(), e.last_kernel_stats())
        monkeypatch.delenv("ROCODER_DIAG", raising=False)
    (loop, (_, hops, l_loop)), (per_hop, (_, hops2, l_hop)) = out["loop"], out["per_hop"]
    assert hops == hops2 and l_hop - l_loop == hops // 2 - 1, (hops, l_loop, l_hop)  # one launch per hop instead of one
    assert rms(loop) > 1e-3 and np.array_equal(loop, per_hop)
    with _engine3(ra, kernel, 2, window_len=N) as e:  # the product library, which never reads the variable
        assert np.array_equal(e.stretch_host(x), loop)


# ---- 4. order and refusals -----------------------------------------------------------------------------------------------
def test_a_range_out_of_order_is_refused_and_the_in_order_range_still_runs():
    import torch

    ra = _ra()
    x = _x3(2)
    with _engine3(ra, "two_tap", 2) as e:
        ref = e.stretch_host(x).copy()
        xt = torch.from_numpy(x).cuda()
        wout = int(e.params.window_out_len)
        wins = ref.shape[1] // wout
        parts = torch.zeros((2, ref.shape[1]), device="cuda")

        def run(w0, w1):
            e.stretch_device_range_ptr(xt.data_ptr(), xt.stride(0), xt.shape[1], 0, 2, w0, w1 - w0,
                                       parts[:, w0 * wout:].data_ptr(), parts.stride(0), (w1 - w0) * wout)

        run(0, 4)
        for w0 in (5, 3, wins - 1):
            with pytest.raises(ra.RocoderError) as ei:
                run(w0, w0 + 1)
            assert ei.value.code == ra._lib.RC_EINVAL and f"at hop {4 * int(e.params.hops_per_window)} " in str(ei.value), str(ei.value)
        run(4, wins)
        e.synchronize()
        assert np.array_equal(parts.cpu().numpy(), ref)


def test_a_hot_swap_into_an_open_stream_starts_from_zero_state_one_hop_early():
    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c, 40 * N) for c in range(2)])
    smooth = example("smooth.hip")
    with ra.Engine(window_len=N, factor=f, channels=2, seed=4, max_batch_hops=1) as e:
        wout, hpw = int(e.params.window_out_len), int(e.params.hops_per_window)
        w_swap = 6
        k0 = w_swap * hpw
        # the offline twin: the identity before hop k0 - 1, the recursion from there on, its out zero before. It holds
        # for the windows from the swap on: hop k0 - 1 runs again under the new kernel for its tail alone, as the hop in
        # front of every range start does, and the windows handed out before the swap are the old kernel's.
        twin = ("#define RC_FEEDBACK 1\n" + HEAD +
                "{ const float a = h.param(0), b = 1.f - a; const float2 x = X[j];\n"
                "  if ((float)h.hop < h.param(1)) return x;\n"
                "  const float2 y = (float)h.hop == h.param(1) ? make_float2(0.f, 0.f) : X.out(1)[j];\n"
                "  return make_float2(a * y.x + b * x.x, a * y.y + b * x.y); }")
        ref = _job(ra, x, N, f, 1, 4, src=twin, params=[0.7, float(k0 - 1)])
        before = _job(ra, x, N, f, 1, 4, src=IDENT)
        e.set_device_kernel_source(IDENT)
        e.set_device_kernel_params([0.7])
        for c in range(2):
            e.push_input(c, x[c])  # the stream stays open
        for w in range(w_swap + 8):
            if w == w_swap:
                e.set_device_kernel_source(smooth)
            for c in range(2):
                got = e.next_window(c)
                want = (before if w < w_swap else ref)[c, w * wout:(w + 1) * wout]
                assert got is not None and np.array_equal(got, want), (w, c)
    tail = slice(w_swap * wout, (w_swap + 8) * wout)
    assert not np.array_equal(ref[:, tail], before[:, tail])
    assert not np.array_equal(ref[:, tail], _job(ra, x, N, f, 1, 4, src=smooth, params=[0.7])[:, tail])


def test_rc_multi_refuses_a_feedback_kernel_and_keeps_the_loaded_one():
    ra = _ra()
    x = _x3(2)
    ref = _job(ra, x, N3, F3, 1, 9, src=X2)
    with ra.MultiEngine([0, 0], window_len=N3, factor=F3, channels=2, seed=9) as m:
        m.set_device_kernel_source(X2)
        with pytest.raises(ra.RocoderError) as ei:
            m.set_device_kernel_source(example("smooth.hip"))
        assert ei.value.code == ra._lib.RC_EUNSUPPORTED and "in order" in str(ei.value)
        assert np.array_equal(m.stretch_host(x), ref)


# ---- 5. zero rules: a kernel that passes X[j] where the read is (0, 0) and returns zero otherwise -----------------------
def _pass_if_zero(expr, head="#define RC_FEEDBACK 2\n", cond="true"):
    return (head + HEAD + "{ if (!(" + cond + ")) return X[j]; const float2 q = " + expr +
            "; return (q.x == 0.f && q.y == 0.f) ? X[j] : make_float2(0.f, 0.f); }")


ZEROS = {
    "d_is_0": _pass_if_zero("X.out(0)[j]"),
    "d_beyond_F": _pass_if_zero("X.out(3)[j]"),
    "before_hop_0": _pass_if_zero("X.out(2)[j]", cond="h.hop < 2"),
    "undeclared": _pass_if_zero("X.out(1)[j]", head=""),
    "other_channel": _pass_if_zero("X.channel(1 - h.channel).out(1)[j]", head="#define RC_FEEDBACK 2\n#define RC_CROSS_CHANNEL 1\n"),
    "past_of_out": _pass_if_zero("X.out(1).past(1)[j]", head="#define RC_FEEDBACK 2\n#define RC_HISTORY 2\n"),
    "channel_of_out": _pass_if_zero("X.out(1).channel(1 - h.channel)[j]", head="#define RC_FEEDBACK 2\n#define RC_CROSS_CHANNEL 1\n"),
}
SUM_TERM = "__device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i) "
SUM_ZEROS = {
    # the sum of |out(1)[j]| inside the term is 0, so X.sum(0) is
    "out_inside_the_term": ("#define RC_FEEDBACK 1\n#define RC_SUMS 1\n" + SUM_TERM +
                            "{ const float2 q = X.out(1)[j]; return fabsf(q.x) + fabsf(q.y); }\n" + HEAD +
                            "{ return X.sum(0) == 0.f ? X[j] : make_float2(0.f, 0.f); }"),
    "sum_of_out": ("#define RC_FEEDBACK 1\n#define RC_SUMS 1\n" + SUM_TERM + "{ return 1.f; }\n" + HEAD +
                   "{ return (X.out(1).sum(0) == 0.f && X.sum(0) == (float)h.n) ? X[j] : make_float2(0.f, 0.f); }"),
}
# the controls: the same trick where the read is NOT zero gives silence from the second hop on
CONTROL = _pass_if_zero("X.out(1)[j]", cond="h.hop >= 1")


def test_reads_outside_the_rules_are_zero():
    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c + 1, 9 * N) for c in range(2)])
    ident = _job(ra, x, N, f, 1, 5, src=IDENT)
    assert rms(ident) > 1e-3
    for name, src in sorted({**ZEROS, **SUM_ZEROS}.items()):
        assert np.array_equal(_job(ra, x, N, f, 1, 5, src=src), ident), name
    assert not np.array_equal(_job(ra, x, N, f, 1, 5, src=CONTROL), ident)


def test_a_single_frame_reads_zero():
    ra = _ra()
    N = 2048
    frame = onp.synth_input(3, N)
    with ra.Engine(window_len=N, channels=2, seed=3) as e:
        e.set_device_kernel_source(IDENT)
        ident = e.resynth(1, 5, frame)
        assert rms(ident) > 1e-3
        e.set_device_kernel_source(_pass_if_zero("X.out(1)[j]"))
        assert np.array_equal(e.resynth(1, 5, frame), ident)
        assert np.array_equal(e.resynth(1, 6, frame), e.resynth(1, 6, frame))
        # ... also behind a job that has left outputs in the ring, and without disturbing the job's order
        x = np.stack([onp.synth_input(c + 1, 9 * N) for c in range(2)])
        e.set_device_kernel_source(example("smooth.hip"))
        e.set_device_kernel_params([0.5])
        first = e.stretch_host(x).copy()
        e.set_device_kernel_params([0.0])  # Y = 0 * out(1) + X
        assert np.array_equal(e.resynth(1, 5, frame), ident)
        e.set_device_kernel_params([0.5])
        assert np.array_equal(e.stretch_host(x), first)


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------
def test_cli_decay_equals_python(tmp_path):
    ra = _ra()
    x = np.stack([onp.synth_input(c, 120_000) for c in range(2)])
    wav_in, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    write_wav(wav_in, x, 44100, "f32")
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    src = os.path.join(EXAMPLES, "decay.hip")
    r = subprocess.run([cli, "-i", wav_in, "-o", wav_out, "-w", "4096", "-f", "4", "--seed", "6", "--device-kernel-src", src,
                        "--dk-params", "0.8"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "1 earlier outputs" in r.stderr, r.stderr[-2000:]
    _, got = read_wav_f32(wav_out)
    code = _compile_as_the_cli_does(src)
    assert ra.device_kernel_feedback(code) == 1
    with ra.Engine(window_len=4096, factor=4.0, channels=2, seed=6) as e:
        e.load_device_kernel(code)
        e.set_device_kernel_params([0.8])
        want = e.stretch_host(x).copy()
    assert rms(want) > 1e-3 and not np.array_equal(want, _job(ra, x, 4096, 4.0, 1, 6, src=IDENT))
    assert np.array_equal(got[:, :want.shape[1]], want)

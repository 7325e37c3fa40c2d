"""User device kernels that read the other channels' spectra (RC_CROSS_CHANNEL, X.channel(c)) on the MI355X.

The oracle side takes two passes of per-channel oracle Stretchers: the first, with a recording identity kernel, collects
every channel's analysis spectra (call i of a channel is its hop i); the second runs each channel again with a host kernel
that computes, in float32 and in the order of the HIP source, what the device kernel computes from the recorded spectra
of all channels at that call index. Every other check is an identity between GPU jobs, bit for bit. The undeclared
kernels' outputs are held to values recorded from the parent commit's build (tests/golden/user_dk_parent_samples.npz).

The sizes follow tests/test_gpu_user_dk_history.py (L = 5 N + 333; 21 whole hops where N is not a power of two). The two
oracle passes, timed on a CPU: N = 1024 under 0.1 s; N = 65536 and 131072 0.4 - 2.3 s for pass 1 and 0.5 - 2.7 s for pass
2 of a kernel, so all three pitches stay; N = 12288 (the oracle's transform of such a length is the slow one) 52 - 58 s a
pass, so a kernel's case is about a minute and the first kernel of each pitch, which also records pass 1, about two."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "user_dk_parent_samples.npz")
TOL = 1e-4

HEAD = "__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
X2 = HEAD + "{ float2 x = X[j]; return make_float2(2.f * x.x, 2.f * x.y); }"
IDENT = HEAD + "{ return X[j]; }"
ZERO = HEAD + "{ return make_float2(0.f, 0.f); }"
SWAP = "#define RC_CROSS_CHANNEL 1\n" + HEAD + "{ return X.channel((h.channel + 1) % h.channels)[j]; }"

# (window, factor): Hop, Big, Gen and Long paths (tests/test_gpu_user_dk_history.py::PATHS)
PATHS = [(1024, 4.0), (65536, 8.0), (12288, 4.0), (131072, 4.0)]
W4 = [0.5, 0.25, -0.375, 0.125]  # blur, D = 3 (the parent-sample cases)


def _ra():
    import rocoder_amd
    from rocoder_amd import _lib

    assert _lib.lib().rc_device_count() > 0, "no MI355X visible: GPU tests must not silently pass"
    return rocoder_amd


def example(name):
    with open(os.path.join(EXAMPLES, name)) as f:
        return f.read()


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


# ---- the oracle: two passes ------------------------------------------------------------------------------------------
def _oracle_channel(x, c, N, f, p, seed, kernel):
    st = oc.Stretcher(channels=x.shape[0], factor=f, pitch_multiple=p, window=oc.hanning(N), seed=seed, channel_index=c,
                      kernel=kernel)
    st.send(x[c])
    st.close_input()
    parts = []
    while not st.is_done():
        parts.append(st.next_window())
    return np.concatenate(parts)


_RECORDED = {}


def _recorded(x, N, f, p, seed):
    """Pass 1: rec[c][i] = the analysis spectrum of hop i of channel c, and the identity kernel's output."""
    key = (x.shape, N, f, p, seed)
    if key not in _RECORDED:
        _RECORDED.clear()  # (one case's spectra at a time)
        rec, out = [], []
        for c in range(x.shape[0]):
            mine = []

            def k(t, spec, mine=mine):
                mine.append(np.array(spec, np.complex64))
                return spec

            out.append(_oracle_channel(x, c, N, f, p, seed, k))
            rec.append(mine)
        _RECORDED[key] = (rec, out)
    return _RECORDED[key]


def _oracle_cross(x, N, f, p, seed, fn):
    """Pass 2: channel c's call i returns fn(rec, c, i), computed from the recorded spectra of all channels."""
    rec, _ = _recorded(x, N, f, p, seed)
    n_out = oc.offline_output_len(x.shape[1], N, f, p)
    out = np.zeros((x.shape[0], n_out), np.float32)
    for c in range(x.shape[0]):
        calls = [0]

        def k(t, spec, c=c, calls=calls):
            i = calls[0]
            calls[0] += 1
            return np.asarray(fn(rec, c, i), np.complex64)

        y = _oracle_channel(x, c, N, f, p, seed, k)[:n_out]
        assert calls[0] == len(rec[c])
        out[c, :y.size] = y
    return out


def swap_fn(rec, c, i):
    return rec[(c + 1) % len(rec)][i]


def mid_side_fn(width):
    w = np.float32(width)
    half = np.float32(0.5)

    def fn(rec, c, i):  # examples/kernels/mid_side.hip
        if len(rec) < 2 or c > 1:
            return rec[c][i]
        l, r = rec[0][i], rec[1][i]
        m, s = half * (l + r), half * (l - r)
        return m + (w if c == 0 else -w) * s

    return fn


def duck_fn(key, sens, depth=2):
    s = np.float32(sens)

    def fn(rec, c, i):  # examples/kernels/duck.hip
        loud = np.zeros(rec[c][i].shape, np.float32)
        for d in range(depth + 1):
            if i - d >= 0:
                k = rec[key][i - d]
                loud = np.maximum(loud, k.real * k.real + k.imag * k.imag)
        g = np.float32(1.0) / (np.float32(1.0) + s * s * loud)
        return g * rec[c][i]

    return fn


def _duck_params(N):
    # magnitudes of a windowed hop of the test signal are of the order N / 4: the gain moves between about 0.5 and 1
    return [1.0, 4.0 / N]


KERNELS = {"swap": (lambda: SWAP, lambda N: None, lambda N: swap_fn),
           "mid_side": (lambda: example("mid_side.hip"), lambda N: [0.5], lambda N: mid_side_fn(0.5)),
           "duck": (lambda: example("duck.hip"), _duck_params, lambda N: duck_fn(1, 4.0 / N))}


def _case_input(ra, N, f, p, channels):
    L = 5 * N + 333
    if N & (N - 1):  # (the oracle's transform of such a length is slow: 21 whole hops at every pitch, and the short ones)
        L = N + 20 * int(ra.derive_params(window_len=N, factor=f, pitch_multiple=p).sample_step_len) + 333
    return np.stack([onp.synth_input(c + 1, L) for c in range(channels)])


def _against_the_oracle(N, f, p, kernel, channels):
    ra = _ra()
    src, params, make = KERNELS[kernel]
    x = _case_input(ra, N, f, p, channels)
    got = _job(ra, x, N, f, p, 23, src=src(), params=params(N))
    ref = _oracle_cross(x, N, f, p, 23, make(N))
    assert rms(ref) > 1e-3, "the case must not be silence"
    assert_close(got, ref, f"{kernel} N={N} p={p} C={channels}")
    if kernel == "swap":
        ident = np.stack([y[:ref.shape[1]] for y in _recorded(x, N, f, p, 23)[1]])
        assert not np.array_equal(ref, ident) and not np.array_equal(got, _job(ra, x, N, f, p, 23, src=IDENT))


# ---- 1. paths and pitches against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))  # (varies fastest: the three kernels of a case share pass 1)
@pytest.mark.parametrize("p", [1, 3, -2])
@pytest.mark.parametrize("N,f", PATHS)
def test_cross_channel_kernels_match_the_oracle(N, f, p, kernel):
    _against_the_oracle(N, f, p, kernel, 2)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_three_channels_match_the_oracle(kernel):
    _against_the_oracle(1024, 4.0, 1, kernel, 3)


# ---- 2. identities between GPU jobs ----------------------------------------------------------------------------------
def test_own_channel_is_the_hop_itself():
    ra = _ra()
    x = np.stack([onp.synth_input(c, 9 * 4096) for c in range(2)])
    base = _job(ra, x, 4096, 4.0, 1, 3, src=X2)
    own = X2.replace("X[j]", "X.channel(h.channel)[j]")
    assert np.array_equal(_job(ra, x, 4096, 4.0, 1, 3, src=own), base)
    assert np.array_equal(_job(ra, x, 4096, 4.0, 1, 3, src="#define RC_CROSS_CHANNEL 1\n" + own), base)
    assert np.array_equal(_job(ra, x, 4096, 4.0, 1, 3, src="#define RC_CROSS_CHANNEL 1\n" + X2), base)


def test_reads_outside_the_declaration_are_zero():
    ra = _ra()
    for N, f in ((4096, 4.0), (12288, 4.0)):
        x = np.stack([onp.synth_input(c, 9 * N) for c in range(2)])
        zero = _job(ra, x, N, f, 1, 5, src=ZERO)
        undeclared = HEAD + "{ return X.channel(1 - h.channel)[j]; }"
        assert np.array_equal(_job(ra, x, N, f, 1, 5, src=undeclared), zero), N
        beyond = "#define RC_CROSS_CHANNEL 1\n" + HEAD + "{ return X.channel(h.channels + 3)[j]; }"
        assert np.array_equal(_job(ra, x, N, f, 1, 5, src=beyond), zero), N
        assert not np.array_equal(_job(ra, x, N, f, 1, 5, src=SWAP), zero)


def test_swap_moves_the_magnitudes_and_keeps_the_phases():
    ra = _ra()
    N, f = 4096, 4.0
    a, b = onp.synth_input(1, 9 * N), onp.synth_input(2, 9 * N)
    # equal channels: the other channel's magnitudes are the own ones, the phases are the channel's own either way
    same = np.stack([b, b])
    ident_bb = _job(ra, same, N, f, 1, 7, src=IDENT)
    assert np.array_equal(_job(ra, same, N, f, 1, 7, src=SWAP), ident_bb)
    # (a, b) under swap: channel 0 carries b's magnitudes with channel 0's phases, as identity on (b, b) does
    ab = _job(ra, np.stack([a, b]), N, f, 1, 7, src=SWAP)
    assert np.array_equal(ab[0], ident_bb[0])
    assert not np.array_equal(ab[0], _job(ra, np.stack([a, b]), N, f, 1, 7, src=IDENT)[0])


def test_composition_with_history_commutes():
    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c + 1, 12 * N) for c in range(2)])
    body = "#define RC_CROSS_CHANNEL 1\n#define RC_HISTORY 2\n" + HEAD + "{ return EXPR; }"
    one = _job(ra, x, N, f, 1, 2, src=body.replace("EXPR", "X.channel(1 - h.channel).past(2)[j]"))
    two = _job(ra, x, N, f, 1, 2, src=body.replace("EXPR", "X.past(2).channel(1 - h.channel)[j]"))
    assert rms(one) > 1e-3 and np.array_equal(one, two)
    deep = _job(ra, x, N, f, 1, 2, src=body.replace("EXPR", "X.channel(1 - h.channel).past(3)[j]"))
    assert np.all(deep == 0.0)


# ---- 3. seams of the computation: all equal the offline job, duck (declared + history) ---------------------------------
DUCK_PARAMS = [1.0, 1e-3]


def _duck_engine(ra, N, f, ch, seed, **kw):
    e = ra.Engine(window_len=N, factor=f, channels=ch, seed=seed, **kw)
    e.load_device_kernel(ra.compile_device_kernel(example("duck.hip")))
    e.set_device_kernel_params(DUCK_PARAMS)
    return e


def _pull_all(e, x, close_first):
    outs = [[] for _ in range(len(x))]
    for c in range(len(x)):
        e.push_input(c, x[c])
        if close_first:
            e.close_input(c)
    done = [False] * len(x)
    while not all(done):
        for c in range(len(x)):
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
    with _duck_engine(ra, N, f, 2, 9) as e:
        ref = e.stretch_host(x).copy()
    assert rms(ref) > 1e-3 and not np.array_equal(ref, _job(ra, x, N, f, 1, 9, src=IDENT))
    for close_first in (True, False):
        with _duck_engine(ra, N, f, 2, 9, max_batch_hops=1) as e:  # batches of one window
            outs = _pull_all(e, x, close_first)
        for c in range(2):
            y = np.concatenate(outs[c])
            n = min(y.size, ref.shape[1])
            assert n >= ref.shape[1] - N and np.array_equal(y[:n], ref[c, :n]), ("seam", close_first, c)


def test_channel_subsets_and_window_cuts_equal_offline():
    import torch

    ra = _ra()
    N, f = 4096, 4.0
    x = np.stack([onp.synth_input(c, 30 * N) for c in range(3)])
    with _duck_engine(ra, N, f, 3, 9) as e:
        ref = e.stretch_host(x).copy()
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


def test_multi_engine_equals_offline():
    import torch

    ra = _ra()
    N, f = 4096, 4.0
    x = np.stack([onp.synth_input(c, 30 * N) for c in range(2)])
    with _duck_engine(ra, N, f, 2, 9) as e:
        ref = e.stretch_host(x).copy()
    code = ra.compile_device_kernel(example("duck.hip"))
    n_have = ra._lib.lib().rc_device_count()
    lists = [[0, 0], [0, 0, 0]]  # parts of ONE channel per shard, on any box
    first = device_lists(max(2, min(n_have, 3)), n_have)[-1]  # the spread list where the box has several GPUs
    if first not in lists:
        lists.append(first)
    for devs in lists:
        with ra.MultiEngine(devs, window_len=N, factor=f, channels=2, seed=9) as m:
            m.load_device_kernel(code)
            m.set_device_kernel_params(DUCK_PARAMS)
            assert np.array_equal(m.stretch_host(x), ref), ("multi host", devs)
            xt = torch.from_numpy(x).cuda(0)
            assert np.array_equal(m.stretch_tensor(xt).cpu().numpy(), ref), ("multi device", devs)
            m.set_staging(True)
            assert np.array_equal(m.stretch_tensor(xt).cpu().numpy(), ref), ("multi device, staged", devs)


def test_hot_swap_between_rounds_in_an_open_stream():
    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c, 60 * N) for c in range(2)])
    duck = ra.compile_device_kernel(example("duck.hip"))
    x2 = ra.compile_device_kernel(X2)
    assert ra.device_kernel_cross_channel(duck) and not ra.device_kernel_cross_channel(x2)
    ref_duck = _job(ra, x, N, f, 1, 4, src=example("duck.hip"), params=DUCK_PARAMS)
    ref_x2 = _job(ra, x, N, f, 1, 4, src=X2)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=4, max_batch_hops=1) as e:
        wout = int(e.params.window_out_len)
        e.load_device_kernel(x2)
        e.set_device_kernel_params(DUCK_PARAMS)
        for c in range(2):
            e.push_input(c, x[c])  # the stream stays open
        w = 0
        for code, ref, count in ((x2, ref_x2, 7), (duck, ref_duck, 9), (x2, ref_x2, 5), (duck, ref_duck, 6)):
            e.load_device_kernel(code)
            for _ in range(count):
                for c in range(2):
                    got = e.next_window(c)
                    assert got is not None, w
                    assert np.array_equal(got, ref[c, w * wout:(w + 1) * wout]), (w, c)
                w += 1


# ---- 4. the stream rules -----------------------------------------------------------------------------------------------
def test_a_window_waits_for_the_open_siblings_input():
    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c, 20 * N) for c in range(2)])
    ref = _job(ra, x, N, f, 1, 4, src=SWAP)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=4, max_batch_hops=1) as e:
        wout = int(e.params.window_out_len)
        e.set_device_kernel_source(SWAP)
        e.push_input(0, x[0])
        e.push_input(1, x[1][:N // 2])  # open, and short of the first hop
        assert e.next_window(0) is None, "channel 0 alone has enough; channel 1 is open and has not"
        e.push_input(1, x[1][N // 2:])
        for c in range(2):
            got = e.next_window(c)
            assert got is not None and np.array_equal(got, ref[c, :wout]), c


def test_a_closed_shorter_channel_reads_as_zero_padded():
    ra = _ra()
    N, f = 2048, 4.0
    L, Ls = 30 * N, 17 * N + 123
    x = np.stack([onp.synth_input(c + 1, L) for c in range(2)])
    padded = x.copy()
    padded[1, Ls:] = 0.0
    ref = _job(ra, padded, N, f, 1, 4, src=SWAP)
    for close_first in (True, False):
        with ra.Engine(window_len=N, factor=f, channels=2, seed=4, max_batch_hops=1) as e:
            e.set_device_kernel_source(SWAP)
            outs = _pull_all(e, [x[0], x[1][:Ls]], close_first)
        y0, y1 = np.concatenate(outs[0]), np.concatenate(outs[1])
        n = min(y0.size, ref.shape[1])
        assert n >= ref.shape[1] - N and np.array_equal(y0[:n], ref[0, :n]), close_first  # late windows included
        assert y1.size < y0.size and np.array_equal(y1, ref[1, :y1.size]), close_first


def test_a_declared_kernel_loads_only_between_rounds():
    ra = _ra()
    N, f = 2048, 4.0
    x = np.stack([onp.synth_input(c, 20 * N) for c in range(2)])
    ref_x2 = _job(ra, x, N, f, 1, 4, src=X2)
    ref_swap = _job(ra, x, N, f, 1, 4, src=SWAP)
    swap = ra.compile_device_kernel(SWAP)
    with ra.Engine(window_len=N, factor=f, channels=2, seed=4, max_batch_hops=1) as e:
        wout = int(e.params.window_out_len)
        e.set_device_kernel_source(X2)
        for c in range(2):
            e.push_input(c, x[c])
        assert np.array_equal(e.next_window(0), ref_x2[0, :wout])
        with pytest.raises(ra.RocoderError) as ei:  # channel 0 stands one window ahead of channel 1
            e.load_device_kernel(swap)
        assert ei.value.code == ra._lib.RC_EINVAL and "RC_CROSS_CHANNEL" in str(ei.value)
        assert np.array_equal(e.next_window(1), ref_x2[1, :wout]), "the old kernel keeps running"
        e.load_device_kernel(swap)  # the round is over
        for c in range(2):
            assert np.array_equal(e.next_window(c), ref_swap[c, wout:2 * wout]), c


def test_single_frame_has_no_other_channel():
    ra = _ra()
    N = 4096
    s = onp.synth_input(1, N)
    with ra.Engine(window_len=N, channels=2, seed=3) as e:
        e.set_device_kernel_source(SWAP)
        assert np.all(e.resynth(1, 7, s) == 0.0)
        e.set_device_kernel_source("#define RC_CROSS_CHANNEL 1\n" + IDENT.replace("X[j]", "X.channel(h.channel)[j]"))
        y = e.resynth(1, 7, s)
        e.set_device_kernel_source(IDENT)
        assert rms(y) > 1e-3 and np.array_equal(y, e.resynth(1, 7, s))


# ---- 5. undeclared kernels are untouched: values recorded from the parent commit's build --------------------------------
PARENT_CASES = {f"{k}_{N}_{p}": (k, N, f, p) for N, f, p in ((4096, 4.0, 1), (12288, 4.0, -2), (65536, 8.0, 1))
                for k in ("x2", "blur")}


def parent_sample_case(name):
    """(source, params, N, f, p, seed, input) of a case; shared with the script that recorded the parent's values."""
    k, N, f, p = PARENT_CASES[name]
    x = np.stack([onp.synth_input(c + 1, 7 * N + 55) for c in range(2)])
    return (X2, None, N, f, p, 31, x) if k == "x2" else (example("blur.hip"), W4, N, f, p, 31, x)


def parent_sample_indices(size):
    return np.sort(np.random.default_rng(20261016).choice(size, size=min(size, 4096), replace=False))


@pytest.mark.parametrize("name", sorted(PARENT_CASES))
def test_undeclared_kernels_give_the_parents_values(name):
    ra = _ra()
    src, params, N, f, p, seed, x = parent_sample_case(name)
    y = _job(ra, x, N, f, p, seed, src=src, params=params).ravel()
    with np.load(GOLDEN) as g:
        want, size = g[name], int(g[name + "_size"])
    assert y.size == size and rms(want) > 1e-3
    assert np.array_equal(y[parent_sample_indices(size)], want)


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------
def test_cli_mid_side_equals_python(tmp_path):
    ra = _ra()
    x = np.stack([onp.synth_input(c, 120_000) for c in range(2)])
    wav_in, wav_out = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    write_wav(wav_in, x, 44100, "f32")
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    r = subprocess.run([cli, "-i", wav_in, "-o", wav_out, "-w", "4096", "-f", "4", "--seed", "6", "--device-kernel-src",
                        os.path.join(EXAMPLES, "mid_side.hip"), "--dk-params", "0.5"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    _, got = read_wav_f32(wav_out)
    want = _job(ra, x, 4096, 4.0, 1, 6, src=example("mid_side.hip"), params=[0.5])
    assert rms(want) > 1e-3 and not np.array_equal(want, _job(ra, x, 4096, 4.0, 1, 6, src=IDENT))
    assert np.array_equal(got[:, :want.shape[1]], want)

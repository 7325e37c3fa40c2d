"""Time maps on the MI355X (include/rocoder_hip_timemap.h).

1. The gather launcher by itself, bit for bit against numpy (timemaputil.gather), through rc_test_time_map_gather of the
   test-hook library: every position class, all four load phases, odd strides and an odd float base, a poisoned and guarded
   destination, hop_first > 0, and the float-per-thread kernel (N % 4 == 2, a destination off 16 bytes).
2. Engine equivalence with no tolerance: engine A runs a map of K hops on x; engine B is a plain engine whose step is
   exactly N (factor 0.5 / 0.25 / 1.0 for p = 1 / 2 / -2) and is given numpy's gathered rows V[: K N - 1]. Both have
   corrected_amp_factor = 4 amplitude. A's output equals B's on every entry, every window path, under every stage, with
   host and device frequency kernels, whatever the chunk size.
3. Parity with the numpy definition (timemaputil.expected_map_job) under the project's contract: RMS error at most 1e-4
   absolute and at most 1e-4 of the reference's RMS.
4. Behaviour: the refusals while a map is set, clearing it, the capacity check."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_np as onp

import timemaputil as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
B_FACTOR = {1: 0.5, 2: 0.25, -2: 1.0}  # the plain engine whose sample_step_len is exactly N
A_FACTOR = 2.0                         # nominal, at most 16: corrected_amp_factor = 4 amplitude on both sides


def _ra():
    import rocoder_amd
    from rocoder_amd import _lib

    assert _lib.lib().rc_device_count() > 0, "no MI355X visible: GPU tests must not silently pass"
    return rocoder_amd


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the launcher
_hooks = None


def hooks():
    global _hooks
    if _hooks is None:
        from rocoder_amd import _lib

        with _lib.hooks_library() as H:
            H.rc_test_time_map_gather.restype = C.c_int
            H.rc_test_time_map_gather.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                                  C.c_uint32, C.c_void_p, C.c_uint64]
            H.rc_test_time_map_chunk_windows.restype = C.c_int
            H.rc_test_time_map_chunk_windows.argtypes = [C.c_void_p, C.c_uint64]
            _hooks = H
    return _hooks


def launch_gather(x_host, pos, N, hop_first=3, v_offset=0, channels=2):
    """x_host [channels, in_len] float32 -> (the gathered rows [channels, K * N] as the launcher wrote them, the whole
    destination block with its guards). The input rows sit at an odd float base with an odd stride; the destination is
    filled with quiet NaNs, 4 guard floats on either side and 4 between the rows."""
    import torch

    _ra()
    H = hooks()
    in_len = x_host.shape[1]
    K = len(pos)
    in_stride = in_len | 1
    src = np.full(1 + channels * in_stride + 1, np.float32(777.0), np.float32)
    for c in range(channels):
        src[1 + c * in_stride:1 + c * in_stride + in_len] = x_host[c]
    d_src = torch.from_numpy(src).cuda()
    table = np.concatenate([np.full(hop_first, 1 << 40, np.int64), np.asarray(pos, np.int64)])
    d_table = torch.from_numpy(table).cuda()
    v_stride = K * N + 4
    total = 4 + v_offset + channels * v_stride + 4
    d_v = torch.full((total,), float("nan"), dtype=torch.float32, device="cuda")
    assert d_v.data_ptr() % 16 == 0 and d_src.data_ptr() % 16 == 0
    x_ptr = d_src.data_ptr() + 4 if in_len else None  # (no input: a null pointer is valid)
    v_ptr = d_v.data_ptr() + 4 * (4 + v_offset)
    # every float the launcher may touch lies inside the two blocks: asserted before the launch
    assert 1 + (channels - 1) * in_stride + in_len <= src.size
    assert 4 + v_offset + (channels - 1) * v_stride + K * N <= total - 4
    rc = H.rc_test_time_map_gather(x_ptr, in_stride, in_len, d_table.data_ptr(), hop_first, K, channels, N, v_ptr, v_stride)
    assert rc == 0, rc
    block = d_v.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy().view(np.uint32), src.view(np.uint32))  # the input is only read
    rows = np.stack([block[4 + v_offset + c * v_stride:4 + v_offset + c * v_stride + K * N] for c in range(channels)])
    mask = np.ones(total, bool)
    for c in range(channels):
        mask[4 + v_offset + c * v_stride:4 + v_offset + c * v_stride + K * N] = False
    assert np.isnan(block[mask]).all(), "a guard word was written"
    return rows


def positions(N, in_len):
    big = 1 << 40
    return [-big, -N - 3, -N, -N + 1, -1, 0, 1, 2, 3, in_len - N - 1, in_len - N, in_len - N + 1, in_len - 1, in_len, in_len + 7, big,
            5, 5, 3, 2]  # ... repeated and decreasing entries


def special_input(in_len, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, in_len)).astype(np.float32)
    sp = np.array([0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC00123, 0x807FFFFF], np.uint32).view(np.float32)
    n = min(in_len, sp.size)
    x[1, :n] = sp[:n]  # -0.0, denormals, infinities, a NaN with a payload: a gather moves bits
    return x


@pytest.mark.parametrize("N", [4, 64, 1000, 16384])
@pytest.mark.parametrize("which", ["0", "1", "N/2", "N", "3N+5"])
def test_gather_launcher_bit_for_bit(N, which):
    in_len = {"0": 0, "1": 1, "N/2": N // 2, "N": N, "3N+5": 3 * N + 5}[which]
    x = special_input(in_len, N + in_len)
    pos = positions(N, in_len)
    got = launch_gather(x, pos, N)
    want = tm.gather(x, pos, N)
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:8]


@pytest.mark.parametrize("N,v_offset,hop_first", [(6, 0, 3), (10, 0, 0), (1002, 0, 1), (64, 1, 3), (16384, 2, 0), (1000, 3, 5)])
def test_gather_launcher_float_kernel_and_first_hop(N, v_offset, hop_first):
    """N % 4 == 2, or a destination off 16 bytes: the float-per-thread kernel writes the same values."""
    in_len = 3 * N + 5
    x = special_input(in_len, 99 + N)
    pos = positions(N, in_len)
    got = launch_gather(x, pos, N, hop_first=hop_first, v_offset=v_offset)
    assert np.array_equal(bits(got), bits(tm.gather(x, pos, N)))


def test_gather_launcher_one_channel_and_many_blocks():
    """More than one block per row and a tail block that is not full (16-byte groups: 4096 per block)."""
    N, in_len = 4096, 30000
    x = special_input(in_len, 5)
    pos = [int(v) for v in np.random.default_rng(1).integers(-N, in_len, 37)]
    got = launch_gather(x[:1], pos, N, channels=1)
    assert np.array_equal(bits(got), bits(tm.gather(x[:1], pos, N)))


# ------------------------------------------------------------------------------------------------ 2. engine equivalence
def make_maps(ra, N, p, K):
    """name -> (positions, in_len). Every map's last window ends past the input: the last sample of V is 0."""
    maps = {}
    curve = ra.stretcher.time_map_curve(40 * N, [0.0, 6.0 * N], [1.0, 12.0], window_len=N, factor=A_FACTOR, pitch_multiple=p)
    assert curve.size >= K
    ramp = curve[:K].copy()
    maps["ramp"] = (ramp, int(ramp[-1]) + N // 2)
    L = 4 * N + 37
    hold_n = min(10, K - 2)
    hold = np.concatenate([np.arange(K - hold_n - 1) * (N // 3), np.full(hold_n, N + 11), [L - N // 2]]).astype(np.int64)
    maps["hold"] = (hold, L)
    rev = np.linspace(L - N // 2, -N // 4, K).astype(np.int64)[::1]
    rev[-1] = L - 1  # (the last window: one sample inside)
    maps["reversed"] = (rev, L)
    mixed = np.array([-2 * N, -N + 1, -5, 0, 3, L - N + 1, L, L + 9, 1, 2, N // 2, L - 1] * ((K + 11) // 12), np.int64)[:K]
    mixed[-1] = L - 3
    maps["mixed"] = (mixed, L)
    for name, (pos, in_len) in maps.items():
        assert pos.size == K and pos[-1] + N - 1 >= in_len, name
    return maps


def input_rows(L, channels=2):
    return np.stack([onp.synth_input(c + 1, L) for c in range(channels)]).astype(np.float32)


def pair(ra, N, p, **kw):
    a = ra.Engine(window_len=N, factor=A_FACTOR, pitch_multiple=p, channels=2, seed=0x5EED, **kw)
    b = ra.Engine(window_len=N, factor=B_FACTOR[p], pitch_multiple=p, channels=2, seed=0x5EED, **kw)
    assert int(b.params.sample_step_len) == N
    assert float(a.params.corrected_amp_factor) == float(b.params.corrected_amp_factor) == 4.0
    return a, b


def check_lengths(ra, N, p, K):
    kw = dict(window_len=N, pitch_multiple=p)
    n_map = ra.stretcher.time_map_output_len(K, factor=A_FACTOR, **kw)
    assert n_map > 0 and ra.offline_output_len(K * N - 1, factor=B_FACTOR[p], **kw) == n_map
    return n_map


def device_out(e, x):
    import torch

    out = e.stretch_tensor(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    e.synchronize()
    return out.cpu().numpy()


PATHS = [("generic", 64, 24), ("hopw9", 512, 24), ("hopw10", 1024, 24), ("hopw11", 2048, 24), ("hopw", 4096, 24), ("hopw2", 8192, 24),
         ("hop4", 16384, 24), ("big5s", 32768, 8), ("big5", 65536, 8), ("chirp-z", 1000, 12), ("long", 131072, 4)]


@pytest.mark.parametrize("path,N,K", PATHS, ids=[p[0] for p in PATHS])
def test_map_job_equals_the_plain_engine_on_the_gathered_rows(path, N, K):
    ra = _ra()
    n_out = check_lengths(ra, N, 1, K)
    a, b = pair(ra, N, 1)
    with a, b:
        for name, (pos, L) in make_maps(ra, N, 1, K).items():
            x = input_rows(L)
            V = tm.gather(x, pos, N)[:, :K * N - 1]
            a.set_time_map(pos)
            assert a.output_len(L) == n_out
            want = b.stretch_host(V).copy()
            assert want.shape == (2, n_out)
            got = a.stretch_host(x)
            assert np.array_equal(bits(got), bits(want)), (path, name, "host")
            assert np.array_equal(bits(device_out(a, x)), bits(device_out(b, V))), (path, name, "device")
            assert np.array_equal(bits(device_out(a, x)), bits(want)), (path, name, "device == host")


@pytest.mark.parametrize("N", [16384, 64])
@pytest.mark.parametrize("p", [1, 2, -2])
def test_map_job_at_every_pitch_and_chunk_size(N, p):
    ra = _ra()
    from rocoder_amd import _lib

    hooks()
    hpw = int(ra.derive_params(window_len=N, pitch_multiple=p).hops_per_window)
    K = 24 if hpw != 1 else 12
    check_lengths(ra, N, p, K)
    with _lib.hooks_library():
        a, b = pair(ra, N, p)
    with a, b:
        for name, (pos, L) in make_maps(ra, N, p, K).items():
            x = input_rows(L)
            V = tm.gather(x, pos, N)[:, :K * N - 1]
            a.set_time_map(pos)
            want = b.stretch_host(V).copy()
            for chunk in (0, 1, 3):  # windows per chunk: the 256 MiB bound, then forced small
                assert hooks().rc_test_time_map_chunk_windows(a._h, chunk) == 0
                assert np.array_equal(bits(a.stretch_host(x)), bits(want)), (name, chunk, "host")
                assert np.array_equal(bits(device_out(a, x)), bits(want)), (name, chunk, "device")


@pytest.mark.parametrize("N", [16384, 4096])
def test_map_job_with_a_callers_window(N):
    ra = _ra()
    K = 24
    w = (0.25 + 0.75 * onp.hanning(N) * np.linspace(0.6, 1.0, N)).astype(np.float32)  # asymmetric, ends not zero
    a, b = pair(ra, N, 1, window=w)
    with a, b:
        for name, (pos, L) in make_maps(ra, N, 1, K).items():
            x = input_rows(L)
            V = tm.gather(x, pos, N)[:, :K * N - 1]
            a.set_time_map(pos)
            want = b.stretch_host(V).copy()
            assert np.array_equal(bits(a.stretch_host(x)), bits(want)), name
            assert np.array_equal(bits(device_out(a, x)), bits(want)), name


def to_i16(x):
    return np.ascontiguousarray(np.clip(np.rint(x.T * 32767.0), -32768, 32767).astype(np.int16))  # [frames, channels]


@pytest.mark.parametrize("N", [16384, 64])
def test_map_job_on_every_entry_and_under_every_stage(N):
    """A's frames are the caller's; B's are the gathered frames (a gather commutes with the decode: 0 decodes to 0.0)."""
    ra = _ra()
    from rocoder_amd import _lib

    hooks()
    K = 24
    n_out = check_lengths(ra, N, 1, K)
    with _lib.hooks_library():
        a, b = pair(ra, N, 1)
    maps = make_maps(ra, N, 1, K)
    with a, b:
        for name in ("ramp", "mixed"):
            pos, L = maps[name]
            x = input_rows(L)
            a.set_time_map(pos)
            fr_a = {"i16": to_i16(x), "f32": np.ascontiguousarray(x.T)}
            fr_b = {k: np.ascontiguousarray(tm.gather(v.T, pos, N)[:, :K * N - 1].T) for k, v in fr_a.items()}
            for chunk in (0, 3):
                assert hooks().rc_test_time_map_chunk_windows(a._h, chunk) == 0
                for fmt in ("i16", "f32"):
                    want = b.stretch_frames(fr_b[fmt]).copy()
                    assert want.shape == (n_out, 2)
                    assert np.array_equal(bits(a.stretch_frames(fr_a[fmt])), bits(want)), (name, fmt, "frames")
                for e in (a, b):
                    e.set_output_dither("tpdf", 11)
                want = b.stretch_frames(fr_b["i16"], out_fmt="i16").copy()
                assert np.array_equal(a.stretch_frames(fr_a["i16"], out_fmt="i16"), want), (name, "pcm")
                assert a.last_clipped == b.last_clipped
                want = b.stretch_frames(fr_b["i16"], out_fmt="i16", normalize=0.9).copy()
                assert np.array_equal(a.stretch_frames(fr_a["i16"], out_fmt="i16", normalize=0.9), want), (name, "norm")
                assert (bits(a.last_peak), bits(a.last_gain), a.last_clipped) == (bits(b.last_peak), bits(b.last_gain), b.last_clipped)
                want = b.stretch_frames_loud(fr_b["f32"], -23.0, 0.8, out_fmt="i16").copy()
                assert np.array_equal(a.stretch_frames_loud(fr_a["f32"], -23.0, 0.8, out_fmt="i16"), want), (name, "loud")
                assert (bits(a.last_lufs), bits(a.last_true_peak), bits(a.last_gain)) == (bits(b.last_lufs), bits(b.last_true_peak), bits(b.last_gain))
                # fade, resample 3 / 2, limiter and a channel map all set
                n_rs = ra.stretcher.resample_len(n_out, 3, 2)
                for e in (a, b):
                    e.set_output_resample(3, 2)
                    e.set_output_fade(n_rs // 5, n_rs - n_rs // 4, n_rs // 4 - 3)
                    e.set_output_limiter(1.5, 0.5, 64)
                    e.set_channel_map([1, 0])
                want = b.stretch_frames(fr_b["i16"], out_fmt="i16").copy()
                assert want.shape == (n_rs, 2)
                assert np.array_equal(a.stretch_frames(fr_a["i16"], out_fmt="i16"), want), (name, "all stages")
                assert a.last_limiter_stats == b.last_limiter_stats and a.last_clipped == b.last_clipped
                want = b.stretch_host(tm.gather(x, pos, N)[:, :K * N - 1]).copy()
                assert np.array_equal(bits(a.stretch_host(x)), bits(want)), (name, "all stages, host rows")
                for e in (a, b):
                    e.set_output_resample(0, 0)
                    e.set_output_fade()
                    e.set_output_limiter()
                    e.set_channel_map(None)
                    e.set_output_dither("none")


@pytest.mark.parametrize("N", [1024, 1000])
def test_map_job_under_frequency_kernels(N):
    """A host frequency kernel (x 2) and examples/kernels/blur.hip (RC_HISTORY 3: X.past(d) is hop k - d of the map): the
    output equals the plain engine's with the same kernel, whatever the chunk size."""
    ra = _ra()
    from rocoder_amd import _lib

    hooks()
    K = 24
    maps = make_maps(ra, N, 1, K)
    blur = "#define RC_HISTORY 3\n" + open(os.path.join(ROOT, "examples", "kernels", "blur.hip")).read()
    code = ra.compile_device_kernel(blur)

    def times2(_t, spec):
        return (2.0 * spec).astype(np.complex64)

    for kind in ("host x2", "blur"):
        kw = dict(kernel=times2, kernel_time_ms=1) if kind == "host x2" else {}
        with _lib.hooks_library():
            a, b = pair(ra, N, 1, **kw)
        with a, b:
            if kind == "blur":
                for e in (a, b):
                    e.load_device_kernel(code)
                    e.set_device_kernel_params([0.5, 0.25, -0.375, 0.125])
            for name in ("ramp", "reversed"):
                pos, L = maps[name]
                x = input_rows(L)
                V = tm.gather(x, pos, N)[:, :K * N - 1]
                a.set_time_map(pos)
                want = b.stretch_host(V).copy()
                for chunk in (0, 1, 3):
                    assert hooks().rc_test_time_map_chunk_windows(a._h, chunk) == 0
                    assert np.array_equal(bits(a.stretch_host(x)), bits(want)), (kind, name, chunk)
                    assert np.array_equal(bits(device_out(a, x)), bits(want)), (kind, name, chunk, "device")


def test_map_job_under_a_feedback_kernel_at_every_chunk_size():
    """examples/kernels/smooth.hip (RC_FEEDBACK 1: X.out(1) is what the kernel returned for hop k - 1 of the map) and a two-tap
    recursion with RC_FEEDBACK 2. A feedback kernel runs its hops in order and carries its state and its tail from chunk to
    chunk: the job equals the plain engine's, which runs the same hops in one piece, at every forced chunk size, twice in a
    row (the second job restarts at hop 0)."""
    ra = _ra()
    from rocoder_amd import _lib

    hooks()
    N, K = 1024, 24
    maps = make_maps(ra, N, 1, K)
    smooth = open(os.path.join(ROOT, "examples", "kernels", "smooth.hip")).read()
    two_tap = ("#define RC_FEEDBACK 2\n__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {\n"
               "    const float2 x = X[j], a = X.out(1)[j], b = X.out(2)[j];\n"
               "    return make_float2(0.5f * x.x + 0.25f * a.x - 0.125f * b.x, 0.5f * x.y + 0.25f * a.y - 0.125f * b.y);\n}\n")
    for kind, src, params in (("smooth", smooth, [0.75]), ("two_tap", two_tap, [])):
        code = ra.compile_device_kernel(src)
        assert ra.device_kernel_feedback(code) == (1 if kind == "smooth" else 2)
        with _lib.hooks_library():
            a, b = pair(ra, N, 1)
        with a, b:
            for e in (a, b):
                e.load_device_kernel(code)
                e.set_device_kernel_params(params)
            for name in ("ramp", "reversed", "hold"):
                pos, L = maps[name]
                x = input_rows(L)
                V = tm.gather(x, pos, N)[:, :K * N - 1]
                a.set_time_map(pos)
                want = b.stretch_host(V).copy()
                assert np.abs(want).max() > 0
                for chunk in (0, 1, 3):
                    assert hooks().rc_test_time_map_chunk_windows(a._h, chunk) == 0
                    assert np.array_equal(bits(a.stretch_host(x)), bits(want)), (kind, name, chunk)
                    assert np.array_equal(bits(device_out(a, x)), bits(want)), (kind, name, chunk, "device")


# ------------------------------------------------------------------------------------------------ 3. parity with the definition
def assert_close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = got.astype(np.float64) - ref
    err, r = float(np.sqrt(np.mean(d * d))), float(np.sqrt(np.mean(ref * ref)))
    print(f"{what}: rms_err={err:.3e} rms_ref={r:.3e}")
    assert err <= TOL and err <= TOL * r, f"{what}: rms_err={err:.3e} rms_ref={r:.3e}"


@pytest.mark.parametrize("N,K,which", [(16384, 24, "ramp"), (16384, 24, "reversed"), (1000, 12, "ramp"), (1000, 12, "reversed")])
def test_map_job_matches_the_numpy_definition(N, K, which):
    ra = _ra()
    pos, L = make_maps(ra, N, 1, K)[which]
    x = input_rows(L)
    ref = tm.expected_map_job(x, pos, N, A_FACTOR, 0.9, 1, 0x5EED)
    with ra.Engine(window_len=N, factor=A_FACTOR, amplitude=0.9, channels=2, seed=0x5EED) as e:
        e.set_time_map(pos)
        for c in range(2):
            assert_close(e.stretch_host(x)[c], ref[c], f"N={N} {which} host ch{c}")
            assert_close(device_out(e, x)[c], ref[c], f"N={N} {which} device ch{c}")


def test_map_job_matches_the_numpy_definition_where_every_mutant_shows():
    """The case of test_time_map_host.py's mutants: white input, a caller's window whose ends are not zero, a map that
    crosses both ends, holds and reverses - and p = 2 and -2 on the same map."""
    ra = _ra()
    from test_time_map_host import mutant_case

    N, x, w, pos = mutant_case()
    for p in (1, 2, -2):
        hpw = int(ra.derive_params(window_len=N, pitch_multiple=p).hops_per_window)
        pp = pos[:len(pos) // hpw * hpw]
        ref = tm.expected_map_job(x, pp, N, A_FACTOR, 1.0, p, 7, window=w)
        with ra.Engine(window_len=N, factor=A_FACTOR, pitch_multiple=p, channels=2, seed=7, window=w) as e:
            e.set_time_map(pp)
            got = e.stretch_host(x)
            for c in range(2):
                assert_close(got[c], ref[c], f"p={p} ch{c}")


# ------------------------------------------------------------------------------------------------ 4. behaviour
def test_refusals_clearing_and_capacity():
    import torch

    ra = _ra()
    from rocoder_amd import _lib

    N, K = 1024, 8
    x = input_rows(5 * N + 3)
    xt = torch.from_numpy(x).cuda()
    with ra.Engine(window_len=N, factor=4.0, channels=2, seed=3) as fresh:
        plain = fresh.stretch_host(x).copy()
    with ra.Engine(window_len=N, factor=4.0, channels=2, seed=3) as e:
        with pytest.raises(ra.RocoderError) as err:
            e.set_time_map([0, 1, 2])  # not a multiple of hops_per_window
        assert err.value.code == _lib.RC_EINVAL
        with pytest.raises(ra.RocoderError):
            e.set_time_map([0, (1 << 48) + 1])
        assert np.array_equal(bits(e.stretch_host(x)), bits(plain))  # a refused map sets nothing
        e.set_time_map(np.arange(K) * 100)
        n_out = e.output_len(x.shape[1])
        assert n_out == K // 2 * N
        out = torch.empty((2, n_out), dtype=torch.float32, device="cuda")
        for call, named in ((lambda: e.stretch_device_range_ptr(xt.data_ptr(), xt.stride(0), x.shape[1], 0, 2, 0, 1, out.data_ptr(), n_out, n_out),
                             "rc_engine_stretch_device_range"),
                            (lambda: e.push_input(0, x[0]), "rc_engine_push_input"),
                            (lambda: e.next_window(0), "rc_engine_next_window"),
                            (lambda: e.next_window_view(0), "rc_engine_next_window_view")):
            with pytest.raises(ra.RocoderError) as err:
                call()
            assert err.value.code == _lib.RC_EINVAL and "time map" in str(err.value) and named in str(err.value)
        got = C.c_size_t(0)
        rc = e._L.rc_engine_stretch_device(e._h, C.c_void_p(xt.data_ptr()), xt.stride(0), x.shape[1], C.c_void_p(out.data_ptr()), n_out,
                                           n_out - 1, C.byref(got), None)
        assert rc == _lib.RC_ECAPACITY
        fp = C.POINTER(C.c_float)
        small = np.empty((2, n_out - 1), np.float32)
        ins = (fp * 2)(*[x[c].ctypes.data_as(fp) for c in range(2)])
        outs = (fp * 2)(*[small[c].ctypes.data_as(fp) for c in range(2)])
        assert e._L.rc_engine_stretch_host(e._h, ins, x.shape[1], outs, n_out - 1, C.byref(got)) == _lib.RC_ECAPACITY
        assert e.stretch_host(x).shape == (2, n_out)
        # the map reads no input at all where there is none: silence in, silence out
        silent = e.stretch_host(np.zeros((2, 0), np.float32))
        assert silent.shape == (2, n_out) and not silent.any()
        e.set_time_map(None)
        assert e.output_len(x.shape[1]) == plain.shape[1]
        assert np.array_equal(bits(e.stretch_host(x)), bits(plain))
        assert np.array_equal(bits(device_out(e, x)), bits(plain))
        e.push_input(0, x[0])  # the streaming seam is open again


def test_kernel_id_is_the_kernel_sources_hash():
    """No hop kernel changed: the library's id is still the hash of the kernel families' sources (tools/kernel_id.py), and
    the gather's translation unit belongs to none of them."""
    import subprocess
    import sys

    ra = _ra()
    from rocoder_amd import _lib

    flags = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rocoder_amd", "csrc"), "print-flags"], capture_output=True, text=True,
                           check=True).stdout.strip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_id

    assert _lib.lib().rc_kernel_id().decode() == kernel_id.id_string(kernel_id.family_ids(os.path.join(ROOT, "rocoder_amd", "csrc"), flags))
    assert not any("timemap" in f for files in kernel_id.FAMILIES.values() for f in files)
    assert not any("timemap" in f for f in kernel_id.SHARED)

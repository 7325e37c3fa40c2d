"""GPU tests of the phase modes end to end (rc_engine_set_phase_mode / Engine.set_phase_mode): factor 1 returns
the input, parity with the numpy twin (tests/phaseutil.py) on the cases tests/test_phase_host.py admits, independence of
the chunking, repeatability, the master chain behind a phase mode, and every refusal."""
import numpy as np
import pytest

import phaseutil as pu
import windowutil

import rocoder_amd
from rocoder_amd import _lib

pytestmark = pytest.mark.gpu

MODES = {"propagate": pu.PROPAGATE, "locked": pu.LOCKED}


def _engine(N, f=1.0, p=1, ch=2, mode=None, **kw):
    eng = rocoder_amd.Engine(window_len=N, factor=f, pitch_multiple=p, channels=ch, seed=7, **kw)
    if mode is not None:
        eng.set_phase_mode(mode)
    return eng


# ------------------------------------------------------------------------------------------------ factor 1: the input
@pytest.mark.parametrize("mode", ["propagate", "locked"])
@pytest.mark.parametrize("N", [32, 1024, 16384])
def test_factor_one_returns_the_input(N, mode):
    """step == H: every e_k is 0, theta is exactly 0 and Z == X, so only the two transforms' rounding separates the output
    from the input - outside the first H samples, which one window covers, and the last window, which runs out of input"""
    H, L = N // 2, 8 * N
    x = windowutil.white_input(2, L)
    eng = _engine(N, mode=mode)
    y = eng.stretch_host(x)
    eng.close()
    assert y.shape[1] >= L
    a, b = H, L - N
    err = pu.rel_rms(y[:, a:b], x[:, a:b])
    print(f"N={N} {mode}: relative rms {err:.3e}")
    assert err <= 1e-5
    assert np.abs(y[:, a:b].astype(np.float64) - x[:, a:b]).max() <= 1e-4


# ------------------------------------------------------------------------------------------------ parity with the twin
_REFS = {}


def _case_ref(case):
    """the twin's output of a parity case, computed once"""
    if case not in _REFS:
        N, f, p, mode, wname = case
        ref = pu.stretch(pu.case_input(N), N, f, p, mode, window=pu.case_window(N, wname))
        ref.setflags(write=False)
        _REFS[case] = ref
    return _REFS[case]


def _case_id(c):
    return "N%d-f%g-p%d-%s-%s" % (c[0], c[1], c[2], ("", "propagate", "locked")[c[3]], c[4])


@pytest.mark.parametrize("case", pu.PARITY_CASES, ids=_case_id)
def test_parity_with_the_twin(case):
    N, f, p, mode, wname = case
    x = pu.case_input(N)
    eng = _engine(N, f, p, mode=mode, window=pu.case_window(N, wname))
    got = eng.stretch_host(x)
    eng.close()
    ref = _case_ref(case)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = pu.rel_rms(got, ref)
    print(f"{_case_id(case)}: relative rms {err:.3e}")
    assert err <= pu.TOL


# ------------------------------------------------------------------------------------------------ chunks, calls, modes
@pytest.mark.parametrize("N,f,p,mode,chunk", [(1024, 3.0, 1, "locked", 7), (1024, 2.0, 2, "propagate", 64), (32, 8.0, 1, "locked", 1),
                                               (1024, 6.0, -2, "locked", 5), (16384, 1.5, 1, "locked", 3)])
def test_small_chunks_are_bit_identical_to_one_chunk(N, f, p, mode, chunk):
    """integer phases are associative: the carried state and the one-hop halo make the chunking invisible, bit for bit"""
    x = pu.case_input(N)
    with _lib.hooks_library():
        H = pu.hooks()
        eng = _engine(N, f, p, mode=mode)
        whole = eng.stretch_host(x).copy()
        assert H.rc_test_phase_chunk_hops(eng._h, chunk) == 0
        cut = eng.stretch_host(x).copy()
        assert H.rc_test_phase_chunk_hops(eng._h, 0) == 0
        again = eng.stretch_host(x).copy()
        eng.close()
    assert np.isfinite(whole).all() and np.abs(whole).max() > 0.01
    assert cut.tobytes() == whole.tobytes()
    assert again.tobytes() == whole.tobytes()


def test_calls_repeat_and_random_is_untouched_by_a_mode_in_between():
    N = 1024
    x = pu.case_input(N)
    eng = _engine(N, 3.0)
    before = eng.stretch_host(x).copy()
    assert eng.phase_mode == rocoder_amd.RC_PHASE_RANDOM
    eng.set_phase_mode("locked")
    assert eng.phase_mode == rocoder_amd.RC_PHASE_LOCKED
    a = eng.stretch_host(x).copy()
    b = eng.stretch_host(x).copy()
    assert a.tobytes() == b.tobytes()  # every call restarts at hop 0
    eng.set_phase_mode(rocoder_amd.RC_PHASE_PROPAGATE)
    c = eng.stretch_host(x).copy()
    assert c.tobytes() != a.tobytes()
    eng.set_phase_mode("random")
    after = eng.stretch_host(x).copy()
    eng.close()
    assert after.tobytes() == before.tobytes()  # the reference's envelope and amplitude are back
    assert pu.rel_rms(a, before) > 0.1  # ... and a mode is another resynthesis
    fresh = _engine(N, 3.0, mode="locked")
    assert fresh.stretch_host(x).tobytes() == a.tobytes()
    fresh.close()


def test_device_form_equals_host_form():
    import torch

    N = 512
    x = pu.case_input(N)
    eng = _engine(N, 2.0, mode="propagate")
    want = eng.stretch_host(x)
    got = eng.stretch_tensor(torch.from_numpy(x).to("cuda")).cpu().numpy()
    eng.close()
    assert got.tobytes() == want.tobytes()


def test_a_host_job_of_several_pipeline_chunks_continues_where_it_stands():
    """rc_engine_stretch_host cuts a long job into window chunks of about 4 Mi output samples per channel, each its own
    range of hops: under a mode they continue at the channels' next hop with theta and the tail carried. The device form
    runs the same job as one range: the same bits."""
    import torch

    N, f = 1024, 8.0
    L = 1_200_000  # 9.6 M output samples per channel: three chunks
    x = windowutil.white_input(2, L)
    eng = _engine(N, f, mode="locked")
    want = eng.stretch_tensor(torch.from_numpy(x).to("cuda")).cpu().numpy()
    got = eng.stretch_host(x)
    eng.close()
    assert got.shape[1] > 2 * (4 << 20) and np.abs(want).max() > 0.01
    assert got.tobytes() == want.tobytes()


def _bus_of(planar):
    """a bus that holds the planar rows as they are: written into its device rows from the host, past every frames entry"""
    import ctypes as C

    L = _lib.lib()  # (dlsym on the engine library's handle also finds the HIP runtime it is linked against)
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipMemcpy.restype = C.c_int
    planar = np.ascontiguousarray(planar, np.float32)
    ch, n = planar.shape
    bus = rocoder_amd.Bus(ch, n)
    ptr, stride = bus.device_rows()
    assert ptr and stride >= n
    for c in range(ch):
        assert L.hipMemcpy(ptr + 4 * c * stride, planar[c].ctypes.data, 4 * n, 1) == 0  # hipMemcpyHostToDevice
    return bus


def test_the_frames_entries_behind_a_phase_mode_are_the_planar_result_through_the_master_chain():
    """The planar LOCKED result of rc_engine_stretch_host is the yardstick (parity with the twin holds it). Every frames
    entry under the same mode, bit for bit: _frames is its transpose; _mix_frames puts it on a bus; _frames_pcm with a fade,
    the limiter and dither set, and _frames_norm on top of them, are that planar result - written into a bus from the host,
    past every frames entry - through the same stages (rc_engine_bus_frames); _frames_loud is it times the gain it reports."""
    N, f = 1024, 2.0
    x = pu.case_input(N)
    frames = np.ascontiguousarray(x.T)
    eng = _engine(N, f, mode="locked", amplitude=2.5)  # (loud enough for the limiter to work)
    planar = eng.stretch_host(x).copy()
    n = planar.shape[1]
    assert pu.rel_rms(planar, 2.5 * pu.stretch(x, N, f, 1, pu.LOCKED)) <= pu.TOL
    assert eng.stretch_frames(frames).tobytes() == np.ascontiguousarray(planar.T).tobytes()
    mixed = rocoder_amd.Bus(2, n)
    assert eng.mix_frames(frames, mixed) == n
    rows, _ = eng.bus_frames(mixed, "f32")
    assert rows.tobytes() == np.ascontiguousarray(planar.T).tobytes()
    mixed.close()
    loud = eng.stretch_frames_loud(frames, -23.0, out_fmt="f32", sample_rate=8000)
    assert np.isfinite(eng.last_lufs) and eng.last_gain > 0 and eng.last_gain != 1
    assert loud.tobytes() == (np.ascontiguousarray(planar.T) * np.float32(eng.last_gain)).astype(np.float32).tobytes()
    bus = _bus_of(planar)
    eng.set_output_fade(300, n - 500, 500)
    eng.set_output_limiter(1.0, 0.7, 64)
    eng.set_output_dither("tpdf", 99)
    want, _stats = eng.bus_frames(bus, "i16")
    got = eng.stretch_frames(frames, out_fmt="i16")
    stats = eng.last_limiter_stats
    want_norm, norm_stats = eng.bus_frames(bus, "i16", target_peak=0.9)
    got_norm = eng.stretch_frames(frames, out_fmt="i16", normalize=0.9)
    peak, gain = eng.last_peak, eng.last_gain
    eng.close()
    bus.close()
    assert stats is not None and stats[1] > 0  # the limiter did turn frames down
    assert got.shape == (n, 2) and got.tobytes() == want.tobytes() and got.any()
    assert got_norm.tobytes() == want_norm.tobytes() and got_norm.tobytes() != got.tobytes()
    assert peak == norm_stats["peak"] and gain == norm_stats["gain"] and peak > 0


# ------------------------------------------------------------------------------------------------ refusals
def _raises(code, fn, *a, word=None, **kw):
    with pytest.raises(rocoder_amd.RocoderError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value
    if word:
        assert word in str(ei.value), ei.value


IDENTITY_DK = "__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) { return X[j]; }"


@pytest.mark.parametrize("mode", ["propagate", "locked"])
def test_unsupported_entries_are_refused_by_name(mode):
    import torch

    N = 256
    eng = _engine(N, 2.0, mode=mode)
    x = pu.case_input(N)
    U = _lib.RC_EUNSUPPORTED
    _raises(U, eng.push_input, 0, x[0], word=mode)
    _raises(U, eng.next_window, 0, word=mode)
    _raises(U, eng.resynth, 0, 0, x[0, :N], word=mode)
    t = torch.from_numpy(x).to("cuda")
    out = torch.empty((2, 4 * eng.params.window_out_len), dtype=torch.float32, device="cuda")
    _raises(U, eng.stretch_device_range_ptr, t.data_ptr(), t.stride(0), t.shape[1], 0, 2, 0, 1, out.data_ptr(), out.stride(0), out.shape[1], word=mode)
    eng.set_phase_mode("random")
    eng.stretch_device_range_ptr(t.data_ptr(), t.stride(0), t.shape[1], 0, 2, 0, 1, out.data_ptr(), out.stride(0), out.shape[1])
    eng.close()


def test_windows_off_the_hop_path_are_unsupported():
    for N in (1000, 32768):
        eng = _engine(N, 2.0)
        _raises(_lib.RC_EUNSUPPORTED, eng.set_phase_mode, "locked", word="locked")
        assert eng.phase_mode == 0
        eng.set_phase_mode("random")
        eng.close()
    eng = _engine(64, 2.0)
    _raises(_lib.RC_EINVAL, eng.set_phase_mode, 3)
    with pytest.raises(ValueError):
        eng.set_phase_mode("coherent")
    eng.close()


def test_kernels_maps_and_warps_are_refused_in_either_order():
    N, E = 256, _lib.RC_EINVAL
    x = pu.case_input(N)
    # the mode first
    eng = _engine(N, 2.0, mode="locked")
    hop_pos = np.arange(eng.params.hops_per_window * 4, dtype=np.int64) * eng.params.sample_step_len
    _raises(E, eng.set_time_map, hop_pos, word="locked")
    anchors = (np.arange(3, dtype=np.int64) * 100) << 32
    _raises(E, eng.set_output_warp, anchors, 100, word="locked")
    code = rocoder_amd.compile_device_kernel(IDENTITY_DK)
    _raises(E, eng.load_device_kernel, code, word="locked")
    eng.load_device_kernel(None)  # clearing is no kernel
    eng.set_time_map(None)
    eng.set_output_warp(None)
    want = eng.stretch_host(x).copy()
    # ... and the mode second
    eng.set_phase_mode("random")
    eng.load_device_kernel(code)
    _raises(E, eng.set_phase_mode, "propagate", word="propagate")
    eng.load_device_kernel(None)
    eng.set_time_map(hop_pos)
    _raises(E, eng.set_phase_mode, "locked", word="time map")
    eng.set_time_map(None)
    eng.set_output_warp(anchors, 100)
    _raises(E, eng.set_phase_mode, "locked", word="warp")
    eng.set_output_warp(None)
    assert eng.phase_mode == 0
    eng.set_phase_mode("locked")
    assert eng.stretch_host(x).tobytes() == want.tobytes()  # nothing of the refused calls stuck
    eng.close()
    for kw in (dict(device_kernel=("gain", 2.0)), dict(device_kernel=("band", 2, 9, 1.0, 0.0)), dict(device_kernel=("shift", 3)),
               dict(kernel=lambda t, X: X)):
        eng = _engine(N, 2.0, **kw)
        _raises(E, eng.set_phase_mode, "locked", word="kernel")
        eng.close()


def test_a_window_without_a_coherent_envelope_is_refused():
    N = 256
    w = np.ones(N, np.float32)
    w[5] = w[5 + N // 2] = 0.0
    eng = _engine(N, 2.0, window=w)
    _raises(_lib.RC_EINVAL, eng.set_phase_mode, "locked", word="2^-10")
    eng.close()

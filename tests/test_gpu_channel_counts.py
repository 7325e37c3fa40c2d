"""Parity across channel counts on every window path (-m gpu): the table of tests/channelutil.py, every channel by itself
against the oracle under the project's gates (assert_parity with TOL / REG_TOL, assert_blocks over half a window at 5e-6).

The fused jobs run on the test-hook library, which alone tells the plan of the last launch (rc_test_last_run_plan): the
plan must be the one the planner gives for the device's CUs (rc_test_plan), and over the cases of every fused path every
regime of tests/channelutil.py must occur - all runs one hop, longer runs in more than a round, hop4_kernel's taper with
more than 3 channels, the resident share clamped to 1. Everything else runs on the shipped library. Each case prints its
worst channel (`channels: ...`): DESIGN "Parity across channel counts" tabulates those figures; none of them is a gate."""
import ctypes as C

import numpy as np
import pytest

import channelutil as cu
from test_channel_counts_host import RC_MAX_CHANNELS, hook_plan_fn
from test_gpu_parity import _engine_mod, _np_band, _np_shift

pytestmark = pytest.mark.gpu


def _n_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _last_plan(e):
    from rocoder_amd import _lib

    with _lib.hooks_library() as Lh:
        fn = Lh.rc_test_last_run_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint32)] * 3
    r, b, s = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert fn(e._h, C.byref(r), C.byref(b), C.byref(s)) == 0
    return r.value, b.value, s.value


def _engine_kw(case):
    kw = dict(window_len=case.N, factor=case.f, pitch_multiple=case.p, channels=case.channels, seed=cu.SEED)
    if case.window:
        kw["window"] = cu.window_of(case)
    return kw


def _report(what, worst_rms, worst_blk):
    print(f"channels: {what} worst_rel_rms={worst_rms:.3e} worst_block={worst_blk:.3e}")


# ------------------------------------------------------------------ fused paths: every count, the plan, every channel
@pytest.mark.parametrize("case", cu.FUSED_CASES, ids=cu.case_id)
def test_fused_path_every_channel_matches_the_oracle(case):
    import torch

    from rocoder_amd import _lib

    ra = _engine_mod()
    n_cu = _n_cu()
    want = cu.plan_of(hook_plan_fn(), n_cu, case)
    x = cu.case_input(case)
    with _lib.hooks_library(), ra.Engine(**_engine_kw(case)) as e:
        got = e.stretch_tensor(torch.from_numpy(x).cuda()).cpu().numpy()
        runs, body, shortest = _last_plan(e)
    assert body == want.run_len, (runs, body, shortest, want)
    if want.tapered:
        assert shortest < body and runs > want.runs_per_channel * case.channels, (runs, body, shortest, want)
    else:
        assert runs == want.runs_per_channel * case.channels and shortest == min(body, cu.hop_count(case)), (runs, body, shortest, want)
    if case.channels > cu.FUSED_BY_NAME[case.path].resident:
        assert case.channels > want.resident and want.share == 0, "more channels than the engine's resident workgroups"
    ref = cu.reference(x, case.N, case.f, case.p, window=cu.window_of(case))
    _report(cu.case_id(case) + f" regimes={sorted(cu.regimes(case, want))}", *cu.assert_every_channel(got, ref, case.N, cu.case_id(case)))


@pytest.mark.parametrize("path", cu.FUSED, ids=lambda p: p.name)
def test_the_cases_of_a_fused_path_hit_every_regime_on_this_device(path):
    """with the device's own CU count: the cases above assert that each launch ran the plan counted here"""
    _engine_mod()
    plan_fn, n_cu = hook_plan_fn(), _n_cu()
    hit = set()
    for case in cu.FUSED_CASES:
        if case.path == path.name:
            hit |= cu.regimes(case, cu.plan_of(plan_fn, n_cu, case))
    assert cu.required_regimes(path) <= hit, (path.name, n_cu, cu.required_regimes(path) - hit)


# ------------------------------------------------------------------ plan independence
@pytest.mark.parametrize("channels", [8, 65])
@pytest.mark.parametrize("path", cu.FUSED, ids=lambda p: p.name)
def test_a_channel_alone_equals_its_row_of_the_full_job(path, channels):
    """The full job's plan depends on the channel count, a single channel's does not know it: channel c run alone through
    rc_engine_stretch_device_range, and a block of three channels in the middle, equal the full job's rows bit for bit."""
    import torch

    from rocoder_amd.distributed import Shard, engine_compute

    ra = _engine_mod()
    case = next(c for c in cu.FUSED_CASES if c.path == path.name and c.channels == channels)
    xt = torch.from_numpy(cu.case_input(case)).cuda()
    with ra.Engine(**_engine_kw(case)) as e:
        full = e.stretch_tensor(xt).clone()
        torch.cuda.synchronize()
        nwin = full.shape[1] // int(e.params.window_out_len)
        comp = engine_compute(e, xt)
        mid = channels // 2
        for c in (0, mid, channels - 1):
            alone = comp(Shard(0, c, 1, 0, nwin))
            torch.cuda.synchronize()
            assert torch.equal(alone[0], full[c]), (case, c)
        block = comp(Shard(0, mid - 1, 3, 0, nwin))
        torch.cuda.synchronize()
        assert torch.equal(block, full[mid - 1:mid + 2]), case
        assert float(full.abs().max()) > 1e-3


# ------------------------------------------------------------------ unfused, chirp-z and long-window paths
def _host_band(N):
    return _np_band(N // 64, N // 8, 1.25, 0.1)


@pytest.mark.parametrize("name,kind,case", cu.other_cases(), ids=lambda v: cu.case_id(v) if isinstance(v, cu.Case) else None)
def test_unfused_chirpz_and_long_paths_every_channel(name, kind, case):
    ra = _engine_mod()
    N = case.N
    x = cu.case_input(case)
    kw = dict(window_len=N, factor=case.f, pitch_multiple=case.p, seed=cu.SEED)
    kernel = None
    if kind == "host":
        kernel = _host_band(N)
        kw.update(kernel=kernel, kernel_threads=2)
    elif kind == "band":
        kernel = _host_band(N)
        kw.update(device_kernel=("band", N // 64, N // 8, 1.25, 0.1))
    elif kind == "shift":
        kernel = _np_shift(37)
        kw.update(device_kernel=("shift", 37))
    got = ra.stretch(x, **kw)
    ref = cu.reference(x, N, case.f, case.p, kernel=kernel)
    _report(cu.case_id(case), *cu.assert_every_channel(got, ref, N, cu.case_id(case)))


# ------------------------------------------------------------------ a kernel that reads the next channel
@pytest.mark.parametrize("channels", [17, 65])
@pytest.mark.parametrize("N", [1024, 16384])
def test_cross_channel_kernel_every_channel_equals_the_rotated_oracle(N, channels):
    from test_gpu_user_dk_channels import SWAP, _oracle_cross, swap_fn

    ra = _engine_mod()
    f = 4.0
    x = np.stack([cu.onp.synth_input(c + 1, 2 * N + 333) for c in range(channels)])
    with ra.Engine(window_len=N, factor=f, channels=channels, seed=cu.SEED) as e:
        e.set_device_kernel_source(SWAP)
        got = e.stretch_host(x).copy()
    ref = _oracle_cross(x, N, f, 1, cu.SEED, swap_fn)
    what = f"swap N={N} C={channels}"
    _report(what, *cu.assert_every_channel(got, ref, N, what))
    own = cu.oracle_rows(x, N, f, 1)  # channel c carries channel c + 1's magnitudes, not its own
    assert all(cu.rel_err(got[c], own[c]) > 1e-2 for c in range(channels))


# ------------------------------------------------------------------ negative pitch
@pytest.mark.parametrize("channels", [8, 65])
@pytest.mark.parametrize("N", [2048, 16384])
def test_negative_pitch_every_channel(N, channels):
    ra = _engine_mod()
    f, p = 4.0, -2
    hops = max(4, min(24, (6_000_000 // N) // channels))
    x = np.stack([cu.onp.synth_input(c, cu.length_for(N, f, p, hops)) for c in range(channels)])
    got = ra.stretch(x, window_len=N, factor=f, pitch_multiple=p, seed=cu.SEED)
    ref = cu.reference(x, N, f, p)
    what = f"pitch -2 N={N} C={channels}"
    _report(what, *cu.assert_every_channel(got, ref, N, what))


# ------------------------------------------------------------------ whole channels dealt unevenly to three engines
@pytest.mark.parametrize("channels", [7, 16])
def test_multi_engine_of_three_equals_the_single_engine(channels):
    ra = _engine_mod()
    N, f = 16384, 8.0
    x = np.stack([cu.onp.synth_input(c, cu.length_for(N, f, 1, 30)) for c in range(channels)])
    with ra.Engine(window_len=N, factor=f, channels=channels, seed=cu.SEED) as e:
        want = e.stretch_host(x).copy()
    with ra.MultiEngine([0, 0, 0], window_len=N, factor=f, channels=channels, seed=cu.SEED) as m:
        got = m.stretch_host(x)
    assert np.array_equal(got, want)
    ref = cu.reference(x, N, f, 1)
    _report(f"multi C={channels}", *cu.assert_every_channel(want, ref, N, f"single engine C={channels}"))


# ------------------------------------------------------------------ the upper end
def test_a_count_above_the_limit_is_refused_at_the_creation():
    """no engine, no launch, no allocation: RC_EUNSUPPORTED names RC_MAX_CHANNELS on every window path"""
    ra = _engine_mod()
    for N in (256, 16384, 65536, 1000, 131072):
        with pytest.raises(ra.RocoderError) as err:
            ra.Engine(window_len=N, factor=2.0, channels=RC_MAX_CHANNELS + 1, seed=1)
        assert err.value.code == -3 and "RC_MAX_CHANNELS = 65535" in str(err.value), str(err.value)

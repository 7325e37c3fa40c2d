"""Channel counts without a GPU: the table of tests/channelutil.py against the run planner (the test-hook library's
rc_test_plan, no device needed) - every plan regime is hit by a listed case of every fused path - the refusal above
RC_MAX_CHANNELS through rc_derive_params, and the thread pool of oracle Stretchers against stretch_offline. The refusals
of rc_engine_create and of a job of more than RC_MAX_JOB_HOPS hops run in tests/c/engine_host_driver.cpp
(tests/test_engine_host_sanitized.py)."""
import ctypes as C

import numpy as np
import pytest

import channelutil as cu
from oracle import cbind as oc
from oracle import oracle_np as onp
from rocoder_amd import _lib

RC_EUNSUPPORTED = -3
RC_MAX_CHANNELS = 65535


@pytest.fixture(scope="module")
def plan_fn():
    return hook_plan_fn()


def hook_plan_fn():
    with _lib.hooks_library() as H:
        fn = H.rc_test_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]

    def plan(n_cu, window_len, pitch, table_window, hop_count, channels):
        out = (C.c_uint32 * 5)()
        assert fn(n_cu, window_len, pitch, table_window, hop_count, channels, out) == 0
        return tuple(out)

    return plan


def test_the_table_walks_every_count_on_every_fused_path():
    for path in cu.FUSED:
        counts = {c.channels for c in cu.FUSED_CASES if c.path == path.name}
        assert set(cu.COUNTS) <= counts and path.resident + 1 in counts, path.name
    names = {p.name for p in cu.FUSED}
    assert {64, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536} == {p.N for p in cu.FUSED}
    assert {p.p for p in cu.FUSED if p.N == 16384 and not p.window} == {1, 2, 3, 4} and "hop4_window" in names


@pytest.mark.parametrize("path", cu.FUSED, ids=lambda p: p.name)
def test_every_regime_is_hit_on_every_fused_path(plan_fn, path):
    hit = {}
    for case in cu.FUSED_CASES:
        if case.path != path.name:
            continue
        plan = cu.plan_of(plan_fn, cu.N_CU, case)
        assert plan.resident == path.resident, "the table's count above the resident workgroups is written for this"
        assert plan.runs_per_channel * plan.run_len >= cu.hop_count(case) > (plan.runs_per_channel - 1) * plan.run_len
        for r in cu.regimes(case, plan):
            hit.setdefault(r, []).append(cu.case_id(case))
    missing = cu.required_regimes(path) - set(hit)
    assert not missing, (path.name, missing)
    # the clamp is reached by the count above the resident workgroups, and by no count of the ordinary ones
    assert all(f"-c{path.resident + 1}-" in i for i in hit[cu.CLAMPED])
    # a plan of more than a round that is not the clamped one, wherever the oracle's cost allows a case for it
    if path.N <= 1024 or path.hop4:
        assert any(f"-c{path.resident + 1}-" not in i for i in hit[cu.MULTI_ROUND]), path.name


def test_hop_count_is_the_engines(plan_fn):
    L = _lib.lib()
    for case in cu.FUSED_CASES[::7]:
        cfg = _config(case.N, case.f, case.p, case.channels)
        n_out = L.rc_offline_output_len(C.byref(cfg), C.c_size_t(case.L))
        par = _lib.rc_params()
        assert L.rc_derive_params(C.byref(cfg), C.byref(par)) == 0
        assert n_out == cu.hop_count(case) // par.hops_per_window * par.window_out_len, cu.case_id(case)
        assert par.hops_per_window == cu.hops_per_window(case.p) and par.sample_step_len == cu.step_of(case.N, case.f, case.p)


def _config(N, f, p, channels):
    cfg = _lib.rc_config()
    C.memset(C.byref(cfg), 0, C.sizeof(cfg))
    cfg.struct_size = C.sizeof(cfg)
    cfg.window_len, cfg.factor, cfg.amplitude, cfg.pitch_multiple = N, f, 1.0, p
    cfg.sample_rate, cfg.channels, cfg.buffer_secs = 44100, channels, 1.0
    return cfg


@pytest.mark.parametrize("N", [64, 1024, 16384, 65536, 1000, 131072])
def test_more_than_65535_channels_are_refused_by_name(N):
    L = _lib.lib()
    L.rc_last_error.restype = C.c_char_p
    par = _lib.rc_params()
    ok = _config(N, 2.0, 1, RC_MAX_CHANNELS)
    assert L.rc_derive_params(C.byref(ok), C.byref(par)) == 0
    assert L.rc_offline_output_len(C.byref(ok), C.c_size_t(10 * N)) > 0
    for channels in (RC_MAX_CHANNELS + 1, 70_000, 2 ** 32 - 1):
        bad = _config(N, 2.0, 1, channels)
        assert L.rc_derive_params(C.byref(bad), C.byref(par)) == RC_EUNSUPPORTED
        msg = L.rc_last_error().decode()
        assert "RC_MAX_CHANNELS" in msg and "65535" in msg and str(channels) in msg, msg
        assert L.rc_offline_output_len(C.byref(bad), C.c_size_t(10 * N)) == 0
        eng = C.c_void_p()
        assert L.rc_engine_create(C.byref(bad), C.byref(eng)) == RC_EUNSUPPORTED and not eng.value  # (before the device is asked for)


def test_the_header_states_the_limits():
    import os

    from conftest import ROOT

    with open(os.path.join(ROOT, "include", "rocoder_hip.h")) as f:
        text = f.read()
    assert "#define RC_MAX_CHANNELS 65535u" in text and "#define RC_MAX_JOB_HOPS 4294967295ull" in text


@pytest.mark.parametrize("N,f,p,ch,L,window", [(256, 4.0, 1, 5, 3000, None), (1024, 2.0, 3, 3, 9001, None),
                                               (16384, 8.0, 1, 2, 60000, None), (2048, 4.0, -2, 3, 20000, None),
                                               (1024, 2.0, 1, 4, 700, None)])
def test_the_pool_of_stretchers_is_stretch_offline(N, f, p, ch, L, window):
    x = np.stack([onp.synth_input(c, L) for c in range(ch)])
    want = oc.stretch_offline(x, N, f, 1.0, p, seed=cu.SEED)
    assert np.array_equal(cu.oracle_rows(x, N, f, p), want)
    assert np.array_equal(cu.oracle_rows(x, N, f, p, threads=1), want)

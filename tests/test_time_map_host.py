"""CPU tests (-m "not gpu") of time maps (include/rocoder_hip_timemap.h): rc_time_map_curve against its Python twin, the
curve's properties against rc_derive_params and rc_offline_output_len, the capacity idiom, hand-written maps, the numpy
definition of a map job (timemaputil.expected_map_job) against the oracle's own literal loop, the mutants of the gather
that definition must catch, and the new header held to the ctypes table and the Rust stub. The setter needs an engine,
and an engine needs a device: its validation runs in tests/c/engine_host_driver_timemap.cpp (test_time_map_sanitized.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle_np as onp

import rocoder_amd  # noqa: E402,F401  (a broken import of the package fails here, loudly)
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import (derive_params, make_config, offline_output_len, time_map_curve,  # noqa: E402
                                   time_map_output_len)

import timemaputil as tm  # noqa: E402


def _raw_curve(cfg, in_len, at, factor, cap, buf=None):
    L = _lib.lib()
    a = (C.c_double * max(1, len(at)))(*at)
    f = (C.c_double * max(1, len(factor)))(*factor)
    n = C.c_size_t(12345)
    rc = L.rc_time_map_curve(C.byref(cfg), in_len, a, f, len(at), buf, cap, C.byref(n))
    return rc, n.value


# ---------------------------------------------------------------------------------------------- the twin
CURVES = [
    ("one point", [0.0], [8.0]),
    ("one point, late", [5000.0], [3.0]),
    ("ramp 8 to 64", [0.0, 40000.0], [8.0, 64.0]),
    ("down and up", [100.5, 9000.25, 30000.0], [4.0, 0.75, 17.3]),
    ("points past in_len", [60000.0, 90000.0], [2.0, 9.0]),
    ("speed up", [0.0, 20000.0], [0.3, 0.001953125]),
]


@pytest.mark.parametrize("p", [1, 2, -2])
@pytest.mark.parametrize("N,in_len", [(1024, 50000), (1000, 50001), (16384, 50000), (64, 31), (1024, 0), (4, 7)])
@pytest.mark.parametrize("name,at,factor", CURVES, ids=[c[0] for c in CURVES])
def test_curve_equals_the_python_twin(name, at, factor, N, in_len, p):
    got = time_map_curve(in_len, at, factor, window_len=N, pitch_multiple=p)
    want = tm.curve(N, p, in_len, at, factor)
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    par = derive_params(window_len=N, pitch_multiple=p)
    assert got.size % par.hops_per_window == 0 and got.size >= par.hops_per_window
    assert got[0] == 0 and np.all(np.diff(got) >= 0)
    # kd is the first hop whose window runs past the input, and the map ends with the window that holds it
    kd = int(np.flatnonzero(got + N > in_len)[0])
    assert got.size == par.hops_per_window * (kd // par.hops_per_window + 1)


# ---------------------------------------------------------------------------------------------- the curve's properties
@pytest.mark.parametrize("N,f,p,L", [(16384, 8.0, 1, 200000), (1024, 2.0, 2, 30001), (1024, 4.0, -2, 30001), (64, 0.5, 1, 1000),
                                     (4096, 0.25, 1, 100000), (1024, 1.0, 1, 1023), (1024, 1.0, 1, 0)])
def test_one_point_with_an_integer_step_is_the_engines_own_grid(N, f, p, L):
    par = derive_params(window_len=N, factor=f, pitch_multiple=p)
    assert N / (2.0 * float(par.pitch_shifted_factor)) == par.sample_step_len  # the step is an integer: nothing is truncated
    pos = time_map_curve(L, [0.0], [f], window_len=N, factor=f, pitch_multiple=p)
    assert np.array_equal(pos, np.arange(pos.size, dtype=np.int64) * par.sample_step_len)
    n_out = offline_output_len(L, window_len=N, factor=f, pitch_multiple=p)
    assert pos.size == n_out // par.window_out_len * par.hops_per_window
    assert time_map_output_len(pos.size, window_len=N, factor=f, pitch_multiple=p) == n_out


def test_factor_3_at_16384_is_no_longer_truncated():
    par = derive_params(window_len=16384, factor=3.0)
    assert par.sample_step_len == 2730
    pos = time_map_curve(10_000_000, [0.0], [3.0], window_len=16384, factor=3.0)
    mean = (pos[-1] - pos[0]) / (pos.size - 1)
    assert abs(mean - 16384 / 6) < 1e-3, mean  # 2730.67 a hop; the steps are 2730 and 2731
    assert set(np.diff(pos).tolist()) == {2730, 2731}


def test_output_len():
    for N, p in ((1024, 1), (1024, 2), (1024, -2), (1000, 3), (64, -4)):
        par = derive_params(window_len=N, pitch_multiple=p)
        hpw, wout = par.hops_per_window, par.window_out_len
        assert time_map_output_len(0, window_len=N, pitch_multiple=p) == 0
        assert time_map_output_len(5 * hpw, window_len=N, pitch_multiple=p) == 5 * wout
        if hpw > 1:
            assert time_map_output_len(5 * hpw + 1, window_len=N, pitch_multiple=p) == 0
    cfg, _keep = make_config(window_len=1024)
    cfg.pitch_multiple = 0
    assert _lib.lib().rc_time_map_output_len(C.byref(cfg), 4) == 0
    assert _lib.lib().rc_time_map_output_len(None, 4) == 0


def test_capacity_idiom_and_rejected_arguments():
    cfg, _keep = make_config(window_len=64, factor=2.0)
    at, fac = [0.0], [2.0]
    rc, K = _raw_curve(cfg, 100, at, fac, 0)
    assert (rc, K) == (_lib.RC_ECAPACITY, 4)
    buf = (C.c_int64 * 6)(*[-7] * 6)
    rc, K = _raw_curve(cfg, 100, at, fac, 3, buf)
    assert (rc, K) == (_lib.RC_ECAPACITY, 4) and list(buf) == [-7] * 6  # too small: nothing written
    rc, K = _raw_curve(cfg, 100, at, fac, 6, buf)
    assert (rc, K) == (_lib.RC_OK, 4) and list(buf) == [0, 16, 32, 48, -7, -7]
    E = _lib.RC_EINVAL
    assert _raw_curve(cfg, 100, [], [], 0)[0] == E  # no point
    assert _raw_curve(cfg, 100, [-1.0], [2.0], 0)[0] == E  # a point in front of the input
    assert _raw_curve(cfg, 100, [5.0, 5.0], [2.0, 2.0], 0)[0] == E  # not strictly increasing
    assert _raw_curve(cfg, 100, [5.0, 4.0], [2.0, 2.0], 0)[0] == E
    assert _raw_curve(cfg, 100, [float("nan")], [2.0], 0)[0] == E
    assert _raw_curve(cfg, 100, [float("inf")], [2.0], 0)[0] == E
    for bad in (0.0, -2.0, 2.0 ** -11, 2.0 ** 20 + 1, float("nan"), float("inf")):
        assert _raw_curve(cfg, 100, [0.0], [bad], 0)[0] == E, bad
    for ok in (2.0 ** -10, 2.0 ** 20):
        assert _raw_curve(cfg, 100, [0.0], [ok], 0)[0] == _lib.RC_ECAPACITY, ok
    L = _lib.lib()
    one = (C.c_double * 1)(2.0)
    n = C.c_size_t(0)
    assert L.rc_time_map_curve(C.byref(cfg), 100, None, one, 1, None, 0, C.byref(n)) == E
    assert L.rc_time_map_curve(C.byref(cfg), 100, one, None, 1, None, 0, C.byref(n)) == E
    assert L.rc_time_map_curve(C.byref(cfg), 100, one, one, 1, None, 0, None) == E
    assert L.rc_time_map_curve(C.byref(cfg), 100, one, one, 1, None, 5, C.byref(n)) == E  # a capacity and no table
    assert L.rc_time_map_curve(None, 100, one, one, 1, None, 0, C.byref(n)) == E
    bad_cfg, _k = make_config(window_len=64)
    bad_cfg.pitch_multiple = -1
    assert L.rc_time_map_curve(C.byref(bad_cfg), 100, one, one, 1, None, 0, C.byref(n)) == E


# typed in, not computed: (N, p, in_len, at, factor) -> the map
BY_HAND = [
    (4, 1, 7, [0.0], [1.0], [0, 2, 4, 6]),                        # step 2; hop 2 at 4 runs out (4 + 4 > 7): kd 2, K = 2 (2 / 2 + 1)
    (8, 1, 16, [0.0], [1.25], [0, 3, 6, 9]),                      # step 3.2: q = 0, 3.2, 6.4, 9.6; kd 3
    (8, 1, 18, [0.0, 8.0], [1.0, 2.0], [0, 4, 6, 8, 10, 12]),     # f = 1, 1.5, 1.83, then 2: q = 0, 4, 6.67, 8.85, 10.85, 12.85; kd 5
    (4, 2, 5, [0.0], [0.5], [0, 2, 4, 6]),                        # psf 1, step 2, four hops a window; kd 1
    (8, -2, 10, [0.0], [2.0], [0, 4]),                            # psf 1, step 4, one hop a window; kd 1, K = 2
    (8, 1, 0, [0.0], [1.0], [0, 4]),                              # no input: kd 0, the first window is finished
    (8, 1, 3, [2.0], [0.5], [0, 8]),                              # in_len < N; step 8
]


@pytest.mark.parametrize("N,p,in_len,at,factor,want", BY_HAND)
def test_maps_written_out_by_hand(N, p, in_len, at, factor, want):
    assert len(want) <= 8
    assert time_map_curve(in_len, at, factor, window_len=N, pitch_multiple=p).tolist() == want
    assert tm.curve(N, p, in_len, at, factor).tolist() == want


def test_gather_written_out_by_hand():
    x = np.array([[1, 2, 3, 4, 5], [10, 20, 30, 40, 50]], np.float32)
    V = tm.gather(x, [-2, 3, 0, 7], 4)
    assert V.tolist() == [[0, 0, 1, 2, 4, 5, 0, 0, 1, 2, 3, 4, 0, 0, 0, 0],
                          [0, 0, 10, 20, 40, 50, 0, 0, 10, 20, 30, 40, 0, 0, 0, 0]]
    assert tm.gather(np.zeros((1, 0), np.float32), [0, -5], 4).tolist() == [[0] * 8]


# ---------------------------------------------------------------------------------------------- the definition of a map job
@pytest.mark.parametrize("p,f", [(1, 2.0), (2, 2.0), (-2, 2.0)])
def test_definition_equals_the_oracles_literal_loop_on_a_uniform_map(p, f):
    N, L, seed = 64, 700, 0x5EED
    par = derive_params(window_len=N, factor=f, pitch_multiple=p)
    assert N / (2.0 * float(par.pitch_shifted_factor)) == par.sample_step_len
    pos = time_map_curve(L, [0.0], [f], window_len=N, factor=f, pitch_multiple=p)
    assert pos.size >= 3 * par.hops_per_window
    for c in range(2):
        x = onp.synth_input(c, L)
        want = onp.stretch_channel_literal(x, N, f, 0.9, p, seed, c)
        got = tm.expected_map_job(np.stack([onp.synth_input(0, L), onp.synth_input(1, L)]), pos, N, f, 0.9, p, seed)[c]
        assert got.shape == want.shape == (time_map_output_len(pos.size, window_len=N, factor=f, pitch_multiple=p),)
        assert np.array_equal(got, want), float(np.max(np.abs(got - want)))


def mutant_case():
    """White input and a caller's window whose ends are not zero: under the Hann window w[0] = w[N - 1] = 0, so a hop's last
    sample never reaches the output and dropping it cannot be seen."""
    N, L = 64, 500
    x = np.random.default_rng(5).uniform(-1, 1, (2, L)).astype(np.float32)
    w = (0.25 + 0.75 * onp.hanning(N) * np.linspace(0.6, 1.0, N)).astype(np.float32)
    pos = [-40, -3, 0, 17, 200, 200, 430, 470, 300, 120, 499, 520]  # both ends crossed, a hold, a reversed stretch
    return N, x, w, pos


@pytest.mark.parametrize("mutant", tm.MUTANTS)
def test_definition_catches_the_mutants_of_the_gather(mutant):
    """The parity bound of the GPU tests (RMS error <= 1e-4 of the reference's RMS) tells every wrong gather from the right
    one: the error of each mutant is more than 50 times either bound."""
    N, x, w, pos = mutant_case()
    want = tm.expected_map_job(x, pos, N, 2.0, 1.0, 1, 7, window=w)
    got = tm.expected_map_job(x, pos, N, 2.0, 1.0, 1, 7, window=w, mutant=mutant)
    for c in ((1,) if mutant == "channel0" else (0, 1)):
        err = float(np.sqrt(np.mean((got[c] - want[c]) ** 2)))
        rms = float(np.sqrt(np.mean(want[c] ** 2)))
        assert err > 50 * 1e-4 * rms and err > 50 * 1e-4, (mutant, c, err, rms)


# ---------------------------------------------------------------------------------------------- the new header, held to its mirrors
def _timemap_prototypes():
    h = open(os.path.join(ROOT, "include", "rocoder_hip_timemap.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    base = {"int": "c_int", "size_t": "usize", "int64_t": "i64", "double": "f64", "rc_config": "RcConfig", "rc_engine": "RcEngine"}
    protos = {}
    for ret, name, args in re.findall(r"^([A-Za-z_][\w \*]*?)\b(rc_\w+)\s*\(([^;{]*?)\)\s*;", h, flags=re.M | re.S):
        params = []
        for a in " ".join(args.split()).split(","):
            toks = re.sub(r"\b\w+$", "", a.strip()).replace("*", " * ").split()
            const = "const" in toks
            ty = base[[t for t in toks if t not in ("const", "*")][0]]
            params.append(("*const " if const else "*mut ") + ty if "*" in toks else ty)
        protos[name] = (base[ret.strip()], params)
    return protos


def test_time_map_header_matches_the_library_the_ctypes_table_and_the_rust_stub():
    protos = _timemap_prototypes()
    assert sorted(protos) == ["rc_engine_set_time_map", "rc_time_map_curve", "rc_time_map_output_len"]
    assert sorted(_lib.TIME_MAP_SYMBOLS) == sorted(protos)
    main = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    assert '#include "rocoder_hip_timemap.h"' in main and "#define RC_ABI_VERSION 5" in main
    L = _lib.lib()
    for name, (_res, args) in _lib.TIME_MAP_SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(args) == len(protos[name][1]), name
    with _lib.hooks_library() as H:
        for name in list(protos) + ["rc_test_time_map_gather", "rc_test_time_map_chunk_windows"]:
            assert hasattr(H, name), name
    assert b"rc_test_time_map" not in open(_lib.LIB_PATH, "rb").read()  # the product library gains no hook
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read())
    blocks = re.findall(r"extern \"C\" \{(.*?)\n\}", rust, flags=re.S)
    assert len(blocks) == 2
    fns = {}
    for name, args, ret in re.findall(r"pub fn (\w+)\((.*?)\)\s*(?:->\s*([^;]+?))?\s*;", blocks[1], flags=re.S):
        fns[name] = (ret.strip(), [a.split(":", 1)[1].strip() for a in " ".join(args.split()).split(",")])
    assert fns == protos
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in protos:
        assert f"`{name}(" in md, name

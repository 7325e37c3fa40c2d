"""CPU tests (-m "not gpu") of the mix bus's host side (include/rocoder_hip_mix.h): the numpy definition of tests/mixutil.py
against hand-written answers (tests/golden/mix_known_answers.json) and against rc_mix_envelope bit for bit, the validation
statuses that need no GPU - and the proof that the cases of tests/test_gpu_frames_mix_kernel.py catch seven mutants of the
definition. Which inputs catch which mutant is asserted in test_the_kernel_cases_catch_the_mutants and stated there."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rocoder_amd = pytest.importorskip("rocoder_amd")
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import mix_envelope  # noqa: E402

import mixutil as M  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "mix_known_answers.json")))
u64p, f32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float)


def test_symbols_agree_in_header_ctypes_and_libraries():
    h = open(os.path.join(ROOT, "include", "rocoder_hip_mix.h")).read()
    main = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    assert '#include "rocoder_hip_mix.h"' in main
    declared = set(re.findall(r"\n(?:int|void)\s+(rc_\w+)\(", h))
    assert declared == set(_lib.MIX_SYMBOLS) and len(declared) == 8
    assert "typedef struct rc_bus rc_bus;" in h and "#define RC_MIX_MAX_KEYS 4096" in h
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert not re.search(r"\n(?:int|void)\s+" + name + r"\(", main), name  # (declared in the mix header alone)
    assert _lib.lib().rc_abi_version() == 5
    assert b"rc_test_frames_mix" not in open(_lib.LIB_PATH, "rb").read()
    with _lib.hooks_library() as H:
        assert hasattr(H, "rc_test_frames_mix")
    assert not M.HAVE_MATH_FMA or hasattr(__import__("math"), "fma")


def close(got, want):
    return abs(float(got) - want) <= GOLDEN["rel_tol"] * max(abs(want), 1e-30) or float(got) == want


def test_numpy_definition_gives_the_hand_written_answers():
    for c in GOLDEN["sqrt_interp"]:
        assert close(M.sqrt_interp(c["a"], c["b"], c["r"]), c["want"]), c
    for c in GOLDEN["envelope"]:
        got = M.envelope(c["keys"], np.array(c["t"], np.uint64))
        assert got.dtype == np.float32 and all(close(g, w) for g, w in zip(got, c["want"])), (c, got)
    for c in GOLDEN["fade_in_out"]:
        if "dur_to_sample" in c:
            assert all(M.dur_to_sample(s, c["rate"]) == d for s, d in c["dur_to_sample"])
        elif c.get("error"):
            with pytest.raises(ValueError):
                M.fade_keys(c["fade_secs"], c["total_samples"], c["rate"])
        else:
            assert M.fade_keys(c["fade_secs"], c["total_samples"], c["rate"]) == [tuple(k) for k in c["want"]]


def test_fade_in_keys_are_the_output_fades_up():
    """with the keys (0, 0), (F, 1) the envelope on [0, F) is up(t, F) of the output fade, bit for bit"""
    import fadeutil

    for F in (1, 7, 1000, 44100):
        t = np.arange(F, dtype=np.uint64)
        want = fadeutil.sq(t, F, False)
        got = M.envelope([(0, 0.0), (F, 1.0)], t)
        r = (t.astype(np.float32) / np.float32(F)).astype(np.float32)
        b = ((r * np.float32(2)).astype(np.float32) - np.float32(1)).astype(np.float32)
        mine = np.sqrt((np.float32(0.5) * (np.float32(1) + np.maximum(b, np.float32(-1))).astype(np.float32)).astype(np.float32))
        assert M.same(got, mine)
        if want is not None:
            assert M.same(got, np.asarray(want, np.float32))


def random_keys(rng, K, span):
    kf = np.unique(rng.integers(0, span, 4 * K + 8, dtype=np.uint64))
    kf = np.sort(rng.permutation(kf)[:K]) if span > 10 ** 6 else np.sort(rng.choice(np.arange(span, dtype=np.uint64), K, replace=False))
    ka = rng.uniform(-2.0, 2.0, K).astype(np.float32)
    if K > 3:
        ka[2] = ka[1]  # an equal pair
    return list(zip(kf.tolist(), ka.tolist()))


@pytest.mark.parametrize("K,span", [(0, 10), (1, 10), (2, 50), (3, 5), (17, 4000), (400, 5000), (4096, 5000), (9, 2 ** 40)])
def test_numpy_envelope_is_rc_mix_envelope_bit_for_bit(K, span):
    rng = np.random.default_rng(K + 1)
    keys = random_keys(rng, K, span)
    first = keys[0][0] if keys else 0
    for t0, n in ((0, min(span, 5000) + 50), (max(0, span - 70), 140), (span // 3, 1), (max(first, 3) - 3, 2000)):
        got = mix_envelope(keys, t0, n)
        want = M.envelope(keys, np.arange(t0, t0 + n, dtype=np.uint64))
        assert got.dtype == np.float32 and M.same(got, want) and not np.isnan(got).any()
    if K == 9:  # frame differences beyond 2^24: the conversion to f32 rounds
        kf = [k[0] for k in keys]
        for t0 in kf[1:-1]:
            assert M.same(mix_envelope(keys, t0 - 3, 7), M.envelope(keys, np.arange(t0 - 3, t0 + 4, dtype=np.uint64)))


def test_validation_statuses_without_a_gpu():
    L = _lib.lib()
    kf = (C.c_uint64 * 3)(1, 5, 9)
    ka = (C.c_float * 3)(0.0, 1.0, 0.5)
    out = (C.c_float * 4)(7, 7, 7, 7)
    env = L.rc_mix_envelope
    assert env(kf, ka, 3, 0, 4, out) == _lib.RC_OK
    assert env(kf, ka, 3, 0, 0, None) == _lib.RC_OK
    assert env(None, None, 0, 0, 4, out) == _lib.RC_OK and list(out) == [1.0] * 4
    out[:] = [7, 7, 7, 7]
    assert env(kf, ka, 3, 0, 4, None) == _lib.RC_EINVAL
    assert env(None, ka, 3, 0, 4, out) == _lib.RC_EINVAL and env(kf, None, 3, 0, 4, out) == _lib.RC_EINVAL
    assert env((C.c_uint64 * 3)(1, 5, 5), ka, 3, 0, 4, out) == _lib.RC_EINVAL
    assert env((C.c_uint64 * 3)(1, 5, 4), ka, 3, 0, 4, out) == _lib.RC_EINVAL
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert env(kf, (C.c_float * 3)(0.0, bad, 0.5), 3, 0, 4, out) == _lib.RC_EINVAL
    big = np.arange(_lib.RC_MIX_MAX_KEYS + 1, dtype=np.uint64)
    amp = np.zeros(big.size, np.float32)
    assert env(big.ctypes.data_as(u64p), amp.ctypes.data_as(f32p), big.size, 0, 4, out) == _lib.RC_EINVAL
    assert env(big.ctypes.data_as(u64p), amp.ctypes.data_as(f32p), big.size - 1, 0, 4, out) == _lib.RC_OK
    out[:] = [7, 7, 7, 7]
    assert env(kf, (C.c_float * 3)(0.0, float("nan"), 0.5), 3, 0, 4, out) == _lib.RC_EINVAL and list(out) == [7.0] * 4
    # the engine and bus entries: what is refused before any device is looked at
    h = C.c_void_p()
    assert L.rc_bus_create(0, 0, 16, C.byref(h)) == _lib.RC_EINVAL and not h.value
    assert L.rc_bus_create(0, 33, 16, C.byref(h)) == _lib.RC_EINVAL and not h.value
    assert L.rc_bus_create(0, 2, 16, None) == _lib.RC_EINVAL
    assert L.rc_bus_clear(None) == _lib.RC_EINVAL and L.rc_bus_info(None, None, None, None) == _lib.RC_EINVAL
    assert L.rc_bus_device_rows(None, None, None) == _lib.RC_EINVAL
    L.rc_bus_destroy(None)
    mixed = C.c_uint64(99)
    assert L.rc_engine_mix_frames(None, None, 0, 5, None, 0, None, None, 0, None, C.byref(mixed)) == _lib.RC_EINVAL and mixed.value == 99
    got = C.c_size_t(99)
    assert L.rc_engine_bus_frames(None, None, None, 0, 5, 0.0, C.byref(got), None, None, None) == _lib.RC_EINVAL and got.value == 99
    assert b"null" in L.rc_last_error()


# ---- the CPU proof: the cases of the GPU kernel test, replayed on the numpy definition and on its mutants ----------------
def replay(kw, mutant=None, order=None):
    x, bus, send = M.case_inputs(kw)
    return M.mix(bus, x, kw["offset"], kw["keys"], send, mutant=mutant)[0]


CASES = dict(M.kernel_cases())
# mutant -> the cases that must show it, and why those inputs do
CAUGHT_BY = {
    # offset != 0 puts bus frame u = t + offset in another place of a segment than layer frame t
    "bus_clock": ["offset 9 align 0", "negative offset", "two keys"],
    # a rising pair with a + fl(b - a) != b (0.15 -> 0.7 at frame 1024, 0.15 -> 0.95 at frame 3000), read exactly at the key
    "le_at_key": ["offset 8 align 0", "mono into stereo"],
    # a pre-filled bus and products that are not exact: white values under amplitudes like 0.1 ... 0.9
    "contracted": ["offset 8 align 0", "one key", "negative offset"],
    # an offset that is not 0
    "offset_sign": ["offset 8 align 0", "negative offset", "N = 5"],
    # a last frame that lands on the bus with a non-zero amplitude
    "drop_last": ["offset 8 align 0", "no keys", "three into two"],
    # a send matrix that is not symmetric under the wrong indexing: 3 -> 2 and 1 -> 2 (the latter is its own transpose:
    # NOT caught there, so only the 3 -> 2 case is listed)
    "send_transposed": ["three into two"],
}


def test_the_definition_is_deterministic_and_the_cases_are_not_trivial():
    for name, kw in CASES.items():
        x, bus, send = M.case_inputs(kw)
        a, landed = M.mix(bus, x, kw["offset"], kw["keys"], send)
        b, _ = M.mix(bus, x, kw["offset"], kw["keys"], send)
        assert M.same(a, b)
        lo, hi = max(0, kw["offset"]), min(kw["N"], kw["offset"] + kw["n"])
        assert landed == max(0, hi - lo), name
        if landed:
            assert not M.same(a, bus), name
        else:
            assert M.same(a, bus), name


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_kernel_cases_catch_the_mutants(mutant):
    for name in CAUGHT_BY[mutant]:
        kw = CASES[name]
        assert not M.same(replay(kw, mutant), replay(kw)), (mutant, name)


def test_the_summation_order_is_seen():
    """the seventh mutant: layers summed in another order. Three layers of white values with different amplitudes: f32
    addition does not associate, so the orders differ in some bits - the three-layer C-ABI test relies on that."""
    N = 1024
    bus = np.zeros((2, N), np.float32)
    layers = [(M.rows(2, 900, s, specials=False), off, keys) for s, off, keys in
              ((1, 10, [(0, 0.0), (300, 1.0)]), (2, 0, None), (3, -200, [(100, 0.9), (700, 0.2)]))]

    def run(order):
        b = bus
        for i in order:
            b, _ = M.mix(b, *layers[i])
        return b

    assert M.same(run([0, 1, 2]), run([0, 1, 2]))
    assert not M.same(run([0, 1, 2]), run([2, 1, 0])) and not M.same(run([0, 1, 2]), run([0, 2, 1]))


def test_fmaf_emulation_on_chosen_values():
    """products that need 48 bits, sums on f32 ties with a non-zero tail, cancellation"""
    f = np.float32
    one_ulp = f(2.0 ** -23)
    # (1 + u)(1 - u) - 1 = -u^2: an f32 fma keeps it, a multiplication followed by an addition gives 0
    got = M.fmaf(f(1) + one_ulp, f(1) - one_ulp, f(-1))
    assert float(got) == -(2.0 ** -46)
    assert float(f((f(1) + one_ulp) * (f(1) - one_ulp)) + f(-1)) == 0.0
    # a tie: 1 + 2^-24 + (a product of 2^-60): rounds up with the tail, to even (down) without
    assert float(M.fmaf(f(2.0 ** -30), f(2.0 ** -30), f(1))) == 1.0
    x = M.fmaf(f(2.0 ** -12), f(2.0 ** -12), f(1))  # 1 + 2^-24 exactly: the tie, to even
    assert float(x) == 1.0
    y = M.fmaf(f(2.0 ** -12) + f(2.0 ** -35), f(2.0 ** -12), f(1))  # a hair above the tie
    assert float(y) == 1.0 + 2.0 ** -23

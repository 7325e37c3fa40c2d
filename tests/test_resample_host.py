"""CPU tests (-m "not gpu") of the band-limited resampler's host side (rc_engine_set_output_resample and its pure helpers
rc_resample_len, rc_resample_table, rc_resample_ratio): the table against the f64 definition of tests/resampleutil.py, the
filter it is, the lengths, the ratios, every refusal, the symbols in the two libraries - and the gate of the GPU tests
itself, asserted on a CPU f32 implementation and refused for four mutants."""
import ctypes as C
import math
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
from rocoder_amd.stretcher import resample_len, resample_ratio, resample_table  # noqa: E402

import resampleutil as R  # noqa: E402

u32p = C.POINTER(C.c_uint32)


def test_symbols_agree_in_header_ctypes_rust_and_integration_md():
    h = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.SYMBOLS["rc_engine_set_output_resample"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32])
    assert _lib.SYMBOLS["rc_resample_len"] == (C.c_size_t, [C.c_size_t, C.c_uint32, C.c_uint32])
    assert _lib.SYMBOLS["rc_resample_ratio"] == (C.c_int, [C.c_float, u32p, u32p])
    assert re.search(r"\nint rc_engine_set_output_resample\(rc_engine \*e, uint32_t num, uint32_t den\);", h)
    assert re.search(r"\nsize_t rc_resample_len\(size_t n, uint32_t num, uint32_t den\);", h)
    assert re.search(r"\nint rc_resample_table\(uint32_t num, uint32_t den, float \*table, size_t cap, uint32_t \*phases, uint32_t \*taps\);", h)
    assert re.search(r"\nint rc_resample_ratio\(float step, uint32_t \*num, uint32_t \*den\);", h)
    assert re.search(r"pub fn rc_engine_set_output_resample\(e: \*mut RcEngine, num: u32, den: u32\) -> c_int;", rust)
    assert re.search(r"pub fn rc_resample_ratio\(step: f32, num: \*mut u32, den: \*mut u32\) -> c_int;", rust)
    for name in ("rc_engine_set_output_resample", "rc_resample_len", "rc_resample_table", "rc_resample_ratio"):
        assert hasattr(_lib.lib(), name) and name in md, name
    assert _lib.lib().rc_abi_version() == 5


def test_hook_is_in_the_hooks_library_alone():
    assert b"rc_test_frames_" not in open(_lib.LIB_PATH, "rb").read()
    assert not hasattr(_lib.lib(), "rc_test_frames_resample")
    with _lib.hooks_library() as H:
        assert hasattr(H, "rc_test_frames_resample")


@pytest.mark.parametrize("num,den", R.RATIOS)
def test_table_is_the_f64_definition_rounded_once(num, den):
    """every coefficient within 2^-24 absolute: an f32 rounding of a value <= 1, plus one flip at a rounding boundary where
    libm and numpy differ in the last f64 bit; sizes den x 2 W"""
    t = resample_table(num, den)
    ref = R.table_f64(num, den)
    W = R.half_width(num, den)
    assert t.shape == (den, 2 * W) == ref.shape and t.dtype == np.float32
    err = np.abs(t.astype(np.float64) - ref).max()
    print(f"{num}/{den}: T = {2 * W}, max |h - h64| = {err * 2 ** 24:.3f} * 2^-24")
    assert err <= 2.0 ** -24


@pytest.mark.parametrize("num,den", R.RATIOS)
def test_table_is_the_filter_the_header_states(num, den):
    """measured in numpy on the f32 table: +-0.00025 dB up to 0.8 s, 91 dB down from s, row sums within 8e-6; asserted with
    a margin for a table that differs by the rounding the test above allows"""
    t = resample_table(num, den)
    s = min(1.0, den / num)
    pb = np.abs(R.response_db(t, num, den, np.linspace(0.0, 0.8 * s, 161))).max()
    sb = R.response_db(t, num, den, np.linspace(s, min(float(den), 4.0), 401)).max()
    if den > 4:  # the images further up, to the prototype's own Nyquist frequency
        sb = max(sb, R.response_db(t, num, den, np.linspace(4.0, float(den), 97)).max())
    rows = np.abs(t.astype(np.float64).sum(axis=1) - 1.0).max()
    l1 = np.abs(t.astype(np.float64)).sum(axis=1).max()
    print(f"{num}/{den}: passband {pb:.6f} dB, stopband {sb:.2f} dB, row sums {rows:.2e}, sum |h| {l1:.4f}")
    assert pb <= 0.001
    assert sb <= -90.0
    assert rows <= 2e-5
    assert l1 <= 2.24


def test_table_sizes_only_capacity_and_refusals():
    L = _lib.lib()
    ph, tp = C.c_uint32(0), C.c_uint32(0)
    assert L.rc_resample_table(320, 294, None, 0, C.byref(ph), C.byref(tp)) == _lib.RC_OK  # reduced: 160/147
    assert (ph.value, tp.value) == (147, 70)
    buf = np.full(147 * 70 + 1, 7.0, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rc_resample_table(160, 147, fp, 147 * 70 - 1, C.byref(ph), C.byref(tp)) == _lib.RC_ECAPACITY
    assert (buf == 7.0).all()
    assert L.rc_resample_table(160, 147, fp, 147 * 70, C.byref(ph), C.byref(tp)) == _lib.RC_OK
    assert buf[-1] == 7.0 and np.array_equal(buf[:-1].reshape(147, 70), resample_table(160, 147))
    assert L.rc_resample_table(160, 147, fp, buf.size, None, C.byref(tp)) == _lib.RC_EINVAL
    assert L.rc_resample_table(160, 147, fp, buf.size, C.byref(ph), None) == _lib.RC_EINVAL
    for num, den in ((0, 0), (0, 1), (1, 0), (1026, 1025), (1024, 1025), (9, 1), (1, 9), (8193, 1024), (127, 1024)):
        assert L.rc_resample_table(num, den, None, 0, C.byref(ph), C.byref(tp)) == _lib.RC_EINVAL, (num, den)
    assert L.rc_resample_table(8192, 1024, None, 0, C.byref(ph), C.byref(tp)) == _lib.RC_OK and (ph.value, tp.value) == (1, 512)
    assert L.rc_resample_table(2050, 2048, None, 0, C.byref(ph), C.byref(tp)) == _lib.RC_OK and ph.value == 1024


def test_resample_len_is_the_definition():
    cases = [(0, 3, 2), (1, 3, 2), (1, 2, 3), (1, 8, 1), (1, 1, 8), (2 ** 40, 160, 147), (2 ** 40, 147, 160), (2 ** 40, 8, 1), (2 ** 40, 1, 8)]
    for num, den in ((160, 147), (147, 160), (3, 2), (2, 3), (1069, 1009), (8, 1)):
        inv = pow(den, -1, num)  # n = r * inv mod num: n * den = r mod num
        for r in (0, num - 1, 1):  # n * den at exactly, one below and one above a multiple of num
            for k in (1, 40):
                n = (r * inv) % num + k * num
                assert (n * den) % num == r
                cases.append((n, num, den))
    for n, num, den in cases:
        want = R.resample_len(n, num, den)
        assert resample_len(n, num, den) == want, (n, num, den)
        if n:  # the m with m * num / den < n: the last one is inside, the next is not
            assert (want - 1) * num < n * den <= want * num
    assert [resample_len(n, 3, 1) for n in (5, 6, 7)] == [2, 2, 3]  # n * den = 5, 6, 7 around 6 = 2 * 3


def test_resample_ratio_is_the_best_rational():
    assert resample_ratio(48000 / 44100) == (160, 147)
    assert resample_ratio(1.5) == (3, 2)
    assert resample_ratio(2 ** (1 / 12)) == (1069, 1009)
    assert resample_ratio(2 ** (7 / 12)) == (1329, 887)
    assert resample_ratio(2 ** (-1 / 12)) == (824, 873)
    assert resample_ratio(8.0) == (8, 1) and resample_ratio(0.125) == (1, 8) and resample_ratio(1.0) == (1, 1)
    rng = np.random.default_rng(5)
    for step in np.exp(rng.uniform(math.log(0.125), math.log(8.0), 200)):
        num, den = resample_ratio(float(step))
        assert (num, den) == R.best_ratio(float(np.float32(step))), step  # (the C-ABI takes an f32)
        assert den <= 1024 and num <= 8 * den and den <= 8 * num and math.gcd(num, den) == 1
    L = _lib.lib()
    a, b = C.c_uint32(11), C.c_uint32(13)
    for bad in (0.0, -1.5, 0.1249, 8.001, 1e30, float("inf"), float("-inf"), float("nan")):
        assert L.rc_resample_ratio(bad, C.byref(a), C.byref(b)) == _lib.RC_EINVAL, bad
        assert (a.value, b.value) == (11, 13)
    assert L.rc_resample_ratio(1.5, None, C.byref(b)) == _lib.RC_EINVAL
    assert L.rc_resample_ratio(1.5, C.byref(a), None) == _lib.RC_EINVAL


def test_setter_refuses_a_null_engine():
    L = _lib.lib()
    for num, den in ((3, 2), (0, 0), (1, 1), (0, 1)):
        assert L.rc_engine_set_output_resample(None, num, den) == _lib.RC_EINVAL
    assert b"null engine" in L.rc_last_error()


# ---- the gate of the GPU tests, on the CPU ------------------------------------------------------------------------------

def _noise(channels, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (channels, n)).astype(np.float32)


@pytest.mark.parametrize("num,den", [(3, 2), (2, 3), (160, 147), (8, 1), (1, 8)])
def test_gate_passes_an_f32_implementation_and_refuses_the_mutants(num, den):
    """|y - y_f64| <= gamma * sum |h_j| |x_j| + 1e-30 on white noise: a sequential f32 implementation passes; taps from
    k0 + 1, row p + 1 and mirrored rows move the result by O(0.1) against a bound of about 1e-5"""
    t = resample_table(num, den)
    x = _noise(2, 600, 17)
    y, bound = R.resample_f64(x, t, num, den)
    assert y.shape[1] == R.resample_len(600, num, den)
    got = R.resample_f32(x, t, num, den)
    assert (np.abs(got - y) <= bound).all()
    assert bound.max() < 1e-4
    mutants = {"k0 + 1": dict(k0_shift=1), "mirrored rows": dict(mirror=True)}
    if den > 1:  # (one row: p + 1 is p)
        mutants["p + 1"] = dict(p_shift=1)
    for name, kw in mutants.items():
        bad = R.resample_f32(x, t, num, den, **kw)
        frac = (np.abs(bad - y) > bound).mean()
        print(f"{num}/{den} mutant {name}: {frac:.3f} of the outputs outside the bound, worst {np.abs(bad - y).max():.3f}")
        # (a row of phase 1/2 is its own mirror image: at den == 2 the mirrored table moves every other output only)
        assert frac > (0.4 if name == "mirrored rows" and den == 2 else 0.5), name


def test_gate_refuses_a_32_bit_position():
    """m * num held in 32 bits at m >= 2^32 / num: positions are 64-bit all the way"""
    num, den = 160, 147
    t = resample_table(num, den)
    W = t.shape[1] // 2
    m0 = 2 ** 32 // num + 5
    src0 = m0 * num // den - W - 3
    x = _noise(1, 400, 23)
    n = src0 + x.shape[1]
    y, bound = R.resample_f64(x, t, num, den, n=n, src0=src0, m0=m0, m1=m0 + 100)
    good = R.resample_f32(x, t, num, den, n=n, src0=src0, m0=m0, m1=m0 + 100)
    assert (np.abs(good - y) <= bound).all() and np.abs(y).max() > 0.1
    bad = R.resample_f32(x, t, num, den, n=n, src0=src0, m0=m0, m1=m0 + 100, wrap32=True)
    assert (np.abs(bad - y) > bound).mean() > 0.5


def test_engine_frames_resample_is_clean_under_asan():
    """The engine's lag bookkeeping over the HIP stub, as a stand-alone program under ASan + UBSan (nothing is loaded into
    python): the resample launches of multi-chunk jobs tile [0, n_rs) once and in order, none reads a row frame its chunk
    has not finished, the fade, pack and download ranges are the resampled ones, and a cleared state is no state."""
    import subprocess

    from test_engine_host_sanitized import _build

    exe = _build("engine_frames_resample_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_frames_resample: ok"

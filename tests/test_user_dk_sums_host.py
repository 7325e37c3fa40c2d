"""User device kernels with whole-hop sums (RC_SUMS, rc_sum_term, X.sum(i)), without a GPU: the source compiles for
gfx950, the code object carries the number of sums where pure Python finds it, independent of the other two markers, a
value outside 0 ... 4 and a declaration without rc_sum_term do not compile, the example kernels build, the arithmetic of
a sum has a numpy twin with known answers, and the engine's host code around the pass is clean under ASan + UBSan in a
stand-alone program (nothing is loaded into python)."""
import os
import subprocess

import numpy as np
import pytest

from test_engine_host_sanitized import _build
from test_user_dk_channels_host import _symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "examples", "kernels")

TERM = """__device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i) {
    const float2 x = X[j];
    return i == 0 ? x.x * x.x + x.y * x.y : (float)j;
}
"""
APPLY = """__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 a = X[j];
    const float g = X.sum(0) + X.past(1).sum(1) + X.channel(1 - h.channel).sum(0);
    return make_float2(g * a.x, g * a.y);
}
"""
DECLARED = "#define RC_SUMS 2\n" + TERM + APPLY


def test_a_declared_source_compiles_and_carries_the_marker():
    import rocoder_amd as ra

    code = ra.compile_device_kernel(DECLARED)
    assert code[:4] == b"\x7fELF"
    syms = _symbols(code)
    assert syms["rc_user_dk_sums"] == 3 and "rc_user_dk_sums_pass" in syms and "rc_user_dk" in syms
    assert ra.device_kernel_sums(code) == 2
    for s in (1, 4):
        code = ra.compile_device_kernel(f"#define RC_SUMS {s}\n" + TERM + APPLY)
        assert _symbols(code)["rc_user_dk_sums"] == s + 1 and ra.device_kernel_sums(code) == s
    with pytest.raises(ValueError):
        ra.device_kernel_sums(b"\x00" * 128)


@pytest.mark.parametrize("head", ["", "#define RC_SUMS 0\n"])
def test_no_sums_leave_no_marker_and_the_call_still_compiles(head):
    import rocoder_amd as ra

    # (X.sum(i) in an undeclared source compiles, as X.channel(c) does, and reads 0; rc_sum_term is not asked for)
    code = ra.compile_device_kernel(head + APPLY)
    syms = _symbols(code)
    assert "rc_user_dk_sums" not in syms and "rc_user_dk_sums_pass" not in syms and "rc_user_dk" in syms
    assert ra.device_kernel_sums(code) == 0


@pytest.mark.parametrize("sums", [0, 3])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("depth", [0, 2])
def test_the_three_markers_are_independent(depth, cross, sums):
    import rocoder_amd as ra

    src = TERM + APPLY
    if sums:
        src = f"#define RC_SUMS {sums}\n" + src
    if cross:
        src = "#define RC_CROSS_CHANNEL 1\n" + src
    if depth:
        src = f"#define RC_HISTORY {depth}\n" + src
    code = ra.compile_device_kernel(src)
    assert ra.device_kernel_history(code) == depth
    assert ra.device_kernel_cross_channel(code) is cross
    assert ra.device_kernel_sums(code) == sums
    syms = _symbols(code)
    assert syms["rc_user_dk_history"] == depth + 1
    assert ("rc_user_dk_channels" in syms) is cross
    assert syms.get("rc_user_dk_sums", 1) == sums + 1 and ("rc_user_dk_sums_pass" in syms) is bool(sums)


@pytest.mark.parametrize("value", ["5", "-1"])
def test_a_number_of_sums_outside_the_range_does_not_compile(value):
    import rocoder_amd as ra

    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel(f"#define RC_SUMS {value}\n" + TERM + APPLY)
    assert ei.value.code == -1
    assert "RC_SUMS" in ei.value.log and "error" in ei.value.log
    assert "RC_SUMS" in str(ei.value).splitlines()[0]  # rc_last_error: the log's first error line


def test_a_declaration_without_the_term_does_not_compile():
    import rocoder_amd as ra

    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel("#define RC_SUMS 1\n" + APPLY)
    assert "rc_sum_term" in ei.value.log and "error" in ei.value.log


def test_compile_errors_in_a_declared_kernel_point_at_the_users_lines():
    import rocoder_amd as ra

    bad = DECLARED.replace("const float2 x = X[j];", "const float2 x = X.bin(j);")  # line 3 of the user's text
    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel(bad, name="sums.hip")
    assert "sums.hip:3" in ei.value.log and "error" in ei.value.log
    # the sums are read-only: writing through the spectrum's pointer to them does not compile
    ro = DECLARED.replace("const float2 a = X[j];", "X.sums_[0] = 1.f; const float2 a = X[j];")  # line 7
    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel(ro, name="sums.hip")
    assert "sums.hip:7" in ei.value.log


@pytest.mark.parametrize("name,sums,depth", [("auto_gain.hip", 1, 0), ("centroid_tilt.hip", 2, 0), ("level_gate.hip", 1, 1)])
def test_example_kernels_compile(name, sums, depth):
    import rocoder_amd as ra

    with open(os.path.join(EXAMPLES, name)) as f:
        src = f.read()
    code = ra.compile_device_kernel(src, name=name)
    assert ra.device_kernel_sums(code) == sums and ra.device_kernel_history(code) == depth
    assert not ra.device_kernel_cross_channel(code)


def test_cli_help_names_the_sums_define():
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "RC_SUMS" in r.stderr and "RC_CROSS_CHANNEL" in r.stderr and "RC_HISTORY" in r.stderr


# ---- the arithmetic of a sum: a numpy twin -------------------------------------------------------------------------------
def hop_sum(terms):
    """X.sum(i) from the N float32 terms of a hop, in the order of rc_user_dk_sums_pass: lane t of 256 adds the terms of
    bins t, t + 256, ... ascending in float64; each wave of 64 lanes is folded by down-shuffles of 32, 16, ... 1 (lane l
    takes lane l + off's value); wave 0's lane 0 adds the four wave partials in wave order; one rounding to float32."""
    t = np.asarray(terms, np.float32).astype(np.float64)
    lanes = np.zeros(256, np.float64)
    with np.errstate(all="ignore"):
        for first in range(0, t.size, 256):
            part = t[first:first + 256]
            lanes[:part.size] += part
        waves = lanes.reshape(4, 64).copy()
        for off in (32, 16, 8, 4, 2, 1):
            waves[:, :off] += waves[:, off:2 * off]
        return np.float32(((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0])


def test_the_numpy_twin_of_a_sum_on_three_tiny_spectra():
    # 1. three bins, idle lanes add exact zeros: 1 + 2 + 4
    assert hop_sum([1.0, 2.0, 4.0]) == np.float32(7.0)
    # 2. float32 terms, float64 accumulation: 2^24 + 1 + 1 is 2^24 + 2 in float64 (in float32 each + 1 would be lost),
    #    and the one rounding to float32 keeps it
    assert hop_sum([2.0 ** 24, 1.0, 1.0]) == np.float32(16777218.0)
    assert np.float32(np.float32(np.float32(2.0 ** 24) + np.float32(1.0)) + np.float32(1.0)) == np.float32(2.0 ** 24)
    # 3. 300 bins, more than one term per lane: the terms 0.1f are float32 values, the sum is rounded once
    want = np.float32(300 * np.float64(np.float32(0.1)))
    assert hop_sum(np.full(300, 0.1, np.float32)) == want
    # (a float32 accumulator, bin after bin, drifts off that value)
    drift = np.float32(0)
    for _ in range(300):
        drift = np.float32(drift + np.float32(0.1))
    assert drift != want
    # NaN and Inf propagate
    assert np.isnan(hop_sum([1.0, np.nan])) and np.isinf(hop_sum([1.0, np.inf])) and np.isnan(hop_sum([np.inf, -np.inf]))


# ---- the engine's host code around the pass ------------------------------------------------------------------------------
def test_engine_host_code_with_sums_is_clean_under_asan_ubsan():
    """tests/c/engine_host_driver_dk_sums.cpp over tests/c/hip_stub_rtc_sums.cpp (rocoder_amd/csrc/host/sanitize.mk builds
    it as engine_dk_sums_asan): the scratch holds every row's sums and no more than reserve's slack; the pass covers
    in_ch_count x (halo + hops) rows in grid chunks of 32768, with a halo, with cross-channel blocks, for channel-subset
    ranges, a single frame, the seam, rc_multi shards and a job of more than 32768 rows; it precedes the kernel on the
    same stream and is counted in the launch statistics; an undeclared module causes one lookup and gets no sums; every
    rejected code object leaves the loaded kernel running."""
    exe = _build("engine_dk_sums_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_dk_sums: ok"

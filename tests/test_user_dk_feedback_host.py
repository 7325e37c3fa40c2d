"""User device kernels that read their own earlier outputs (RC_FEEDBACK, X.out(d)), without a GPU: the source compiles for
gfx950, the code object carries the depth where pure Python finds it, independent of the other three markers, a value
outside 0 ... 4 does not compile, an undeclared source that calls X.out compiles and carries no marker, nothing can be
written through an out spectrum, the example kernels build, the CLI's help names the define, and the engine's host code
around the feature is clean under ASan + UBSan in a stand-alone program (nothing is loaded into python)."""
import os
import subprocess

import pytest

from test_engine_host_sanitized import _build
from test_user_dk_channels_host import _symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "examples", "kernels")

TERM = """__device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i) {
    const float2 x = X[j];
    return x.x * x.x + x.y * x.y;
}
"""
APPLY = """__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 a = X[j];
    const float2 y = X.out(1)[(int64_t)j - 1];
    const float g = X.sum(0) + X.past(1).sum(0) + X.channel(1 - h.channel).sum(0) + (float)h.feedback;
    return make_float2(g * a.x + y.x, g * a.y + y.y);
}
"""
DECLARED = "#define RC_FEEDBACK 2\n" + APPLY


def test_a_declared_source_compiles_and_carries_the_marker():
    import rocoder_amd as ra

    code = ra.compile_device_kernel(DECLARED)
    assert code[:4] == b"\x7fELF"
    syms = _symbols(code)
    assert syms["rc_user_dk_feedback"] == 3 and "rc_user_dk" in syms
    assert ra.device_kernel_feedback(code) == 2
    for f in (1, 4):
        code = ra.compile_device_kernel(f"#define RC_FEEDBACK {f}\n" + APPLY)
        assert _symbols(code)["rc_user_dk_feedback"] == f + 1 and ra.device_kernel_feedback(code) == f
    with pytest.raises(ValueError):
        ra.device_kernel_feedback(b"\x00" * 128)


@pytest.mark.parametrize("head", ["", "#define RC_FEEDBACK 0\n"])
def test_no_feedback_leaves_no_marker_and_the_call_still_compiles(head):
    import rocoder_amd as ra

    code = ra.compile_device_kernel(head + APPLY)  # (calls X.out(1))
    syms = _symbols(code)
    assert "rc_user_dk_feedback" not in syms and "rc_user_dk" in syms
    assert ra.device_kernel_feedback(code) == 0


@pytest.mark.parametrize("feedback", [0, 3])
@pytest.mark.parametrize("sums", [0, 2])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("depth", [0, 2])
def test_the_four_markers_are_independent(depth, cross, sums, feedback):
    import rocoder_amd as ra

    src = TERM + APPLY
    if feedback:
        src = f"#define RC_FEEDBACK {feedback}\n" + src
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
    assert ra.device_kernel_feedback(code) == feedback
    syms = _symbols(code)
    assert syms["rc_user_dk_history"] == depth + 1
    assert ("rc_user_dk_channels" in syms) is cross
    assert syms.get("rc_user_dk_sums", 1) == sums + 1 and ("rc_user_dk_sums_pass" in syms) is bool(sums)
    assert syms.get("rc_user_dk_feedback", 1) == feedback + 1


@pytest.mark.parametrize("value", ["5", "-1"])
def test_a_depth_outside_the_range_does_not_compile(value):
    import rocoder_amd as ra

    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel(f"#define RC_FEEDBACK {value}\n" + APPLY)
    assert ei.value.code == -1
    assert "RC_FEEDBACK" in ei.value.log and "error" in ei.value.log
    assert "RC_FEEDBACK" in str(ei.value).splitlines()[0]  # rc_last_error: the log's first error line


def test_nothing_is_written_through_an_out_spectrum():
    import rocoder_amd as ra

    for member in ("p_", "fb_"):  # the bins of the out spectrum, and the ring behind X itself
        ro = DECLARED.replace("const float2 a = X[j];", f"X.out(1).{member}[0].x = 1.f; const float2 a = X[j];")  # line 3
        with pytest.raises(ra.DeviceKernelCompileError) as ei:
            ra.compile_device_kernel(ro, name="fb.hip")
        assert "fb.hip:3" in ei.value.log and "error" in ei.value.log


@pytest.mark.parametrize("name", ["decay.hip", "freeze.hip", "smooth.hip"])
def test_example_kernels_compile(name):
    import rocoder_amd as ra

    with open(os.path.join(EXAMPLES, name)) as f:
        src = f.read()
    code = ra.compile_device_kernel(src, name=name)
    assert ra.device_kernel_feedback(code) == 1
    assert ra.device_kernel_history(code) == 0 and ra.device_kernel_sums(code) == 0 and not ra.device_kernel_cross_channel(code)


def test_cli_help_names_the_feedback_define():
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "RC_FEEDBACK" in r.stderr and "X.out(" in r.stderr


def test_engine_host_code_with_feedback_is_clean_under_asan_ubsan():
    """tests/c/engine_host_driver_dk_fb.cpp over tests/c/hip_stub_rtc_fb.cpp (rocoder_amd/csrc/host/sanitize.mk builds it as
    engine_dk_fb_asan): the launches of a chunk in the loop and the per-hop shape, in hop order, on every window path, with
    a halo, cross-channel blocks and a sums pass; the state of exactly channels x (F + 1) x 8 N bytes; restart, continue,
    the first call after a load and the refusal of anything else, which enqueues nothing and leaves the ring as it was;
    channels in different cases; a single frame without state; the seam; rc_multi's refusal; every rejected code object
    leaves the loaded kernel and its books in place. The stub checks every ring row it is handed against the block."""
    exe = _build("engine_dk_fb_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_dk_fb: ok"

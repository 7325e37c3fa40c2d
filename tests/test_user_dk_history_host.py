"""User device kernels that read earlier hops (RC_HISTORY, X.past(d)), without a GPU: the source compiles for gfx950, the
code object carries the declared depth where pure Python finds it, too deep a history does not compile, and the example
kernels build."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "examples", "kernels")

X2 = ("__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
      "{ float2 x = X[j]; return make_float2(2.f * x.x, 2.f * x.y); }")

PAST2 = """#define RC_HISTORY 2
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 a = X[j], b = X.past(1)[j], c = X.past(2)[j + 1];
    return make_float2(a.x + b.x + c.x + (float)h.history, a.y + b.y + c.y);
}
"""


def test_history_source_compiles_and_declares_its_depth():
    import rocoder_amd as ra

    code = ra.compile_device_kernel(PAST2)
    assert code[:4] == b"\x7fELF"
    assert ra.device_kernel_history(code) == 2


def test_source_without_history_declares_zero():
    import rocoder_amd as ra

    assert ra.device_kernel_history(ra.compile_device_kernel(X2)) == 0
    with pytest.raises(ValueError):
        ra.device_kernel_history(b"\x00" * 128)


@pytest.mark.parametrize("depth", [0, 1, 8])
def test_every_allowed_depth_compiles(depth):
    import rocoder_amd as ra

    assert ra.device_kernel_history(ra.compile_device_kernel(f"#define RC_HISTORY {depth}\n" + X2)) == depth


def test_history_above_the_maximum_does_not_compile():
    import rocoder_amd as ra

    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel("#define RC_HISTORY 9\n" + X2)
    assert ei.value.code == -1
    assert "RC_HISTORY" in ei.value.log and "error" in ei.value.log
    assert "RC_HISTORY" in str(ei.value).splitlines()[0]  # rc_last_error: the log's first error line


def test_compile_errors_in_a_history_kernel_point_at_the_users_lines():
    import rocoder_amd as ra

    bad = PAST2.replace("const float2 a = X[j]", "const float2 a = X.before(1)[j]")  # line 3 of the user's text
    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel(bad, name="hist.hip")
    assert "hist.hip:3" in ei.value.log and "error" in ei.value.log
    # the user gets no pointer through past() either: writing through it does not compile
    ro = PAST2.replace("const float2 a = X[j]", "X.past(1).p_[0].x = 1.f; const float2 a = X[j]")
    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel(ro, name="hist.hip")
    assert "hist.hip:3" in ei.value.log


@pytest.mark.parametrize("name,depth", [("blur.hip", 3), ("delay.hip", 1), ("flux_gate.hip", 1)])
def test_example_kernels_compile(name, depth):
    import rocoder_amd as ra

    with open(os.path.join(EXAMPLES, name)) as f:
        src = f.read()
    assert ra.device_kernel_history(ra.compile_device_kernel(src, name=name)) == depth
    if name != "flux_gate.hip":  # blur and delay take another depth from a define in front of the file
        assert ra.device_kernel_history(ra.compile_device_kernel("#define RC_HISTORY 8\n" + src, name=name)) == 8


def test_cli_help_names_the_history_define():
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "RC_HISTORY" in r.stderr


def test_engine_host_code_with_history_is_clean_under_asan_ubsan():
    """The halo bookkeeping of a depth-3 kernel (chunks, ranges, streaming batches, rc_multi spans) over the HIP stub,
    whose device memory is host memory: tests/c/engine_host_driver_dk.cpp under ASan + UBSan."""
    host = os.path.join(ROOT, "rocoder_amd", "csrc", "host")
    r = subprocess.run(["make", "-C", host, "-f", "sanitize.mk", "../../bin/engine_dk_asan"], capture_output=True,
                       text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "rocoder_amd", "bin", "engine_dk_asan")], capture_output=True, text=True,
                       timeout=1800, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "engine_host_driver_dk: ok" in out

"""User device kernels that read the other channels' spectra (RC_CROSS_CHANNEL, X.channel(c)), without a GPU: the source
compiles for gfx950, the code object carries the declaration where pure Python finds it, independent of the history
depth, any value but 0 and 1 does not compile, and the example kernels build."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "examples", "kernels")

X2 = ("__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
      "{ float2 x = X[j]; return make_float2(2.f * x.x, 2.f * x.y); }")

OTHER = """__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const float2 a = X[j], b = X.channel(1 - h.channel)[j];
    return make_float2(a.x + b.x + (float)h.channels, a.y + b.y);
}
"""
DECLARED = "#define RC_CROSS_CHANNEL 1\n" + OTHER


def _symbols(code):
    """name -> size of the code object's ELF symbols (the way the sibling history test reads the depth)."""
    import struct

    b = bytes(code)
    assert b[:4] == b"\x7fELF" and b[4] == 2 and b[5] == 1
    shoff, = struct.unpack_from("<Q", b, 40)
    shentsize, shnum = struct.unpack_from("<HH", b, 58)
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _n, typ, _f, _a, off, size, link, _i, _al, ent in secs:
        if typ not in (2, 11) or ent != 24:
            continue
        strtab = b[secs[link][4]:secs[link][4] + secs[link][5]]
        for s in range(off, off + size - 23, 24):
            st_name, _i2, _o, _sh, _v, st_size = struct.unpack_from("<IBBHQQ", b, s)
            out[strtab[st_name:strtab.index(b"\0", st_name)].decode()] = st_size
    return out


def test_cross_channel_source_compiles_and_carries_the_marker():
    import rocoder_amd as ra

    code = ra.compile_device_kernel(DECLARED)
    assert code[:4] == b"\x7fELF"
    assert "rc_user_dk_channels" in _symbols(code) and "rc_user_dk" in _symbols(code)
    assert ra.device_kernel_cross_channel(code) is True
    # the same source without the define compiles too (the other channel reads zero) and reports none
    plain = ra.compile_device_kernel(OTHER)
    assert "rc_user_dk_channels" not in _symbols(plain)
    assert ra.device_kernel_cross_channel(plain) is False
    assert ra.device_kernel_cross_channel(ra.compile_device_kernel("#define RC_CROSS_CHANNEL 0\n" + OTHER)) is False
    with pytest.raises(ValueError):
        ra.device_kernel_cross_channel(b"\x00" * 128)


def test_any_other_value_of_the_define_does_not_compile():
    import rocoder_amd as ra

    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel("#define RC_CROSS_CHANNEL 2\n" + OTHER)
    assert ei.value.code == -1
    assert "RC_CROSS_CHANNEL" in ei.value.log and "error" in ei.value.log
    assert "RC_CROSS_CHANNEL" in str(ei.value).splitlines()[0]  # rc_last_error: the log's first error line


def test_compile_errors_in_a_declared_kernel_point_at_the_users_lines():
    import rocoder_amd as ra

    bad = DECLARED.replace("const float2 a = X[j]", "const float2 a = X.chan(0)[j]")  # line 3 of the user's text
    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel(bad, name="xch.hip")
    assert "xch.hip:3" in ei.value.log and "error" in ei.value.log
    # the user gets no pointer through channel() either: writing through it does not compile
    ro = DECLARED.replace("const float2 a = X[j]", "X.channel(1).p_[0].x = 1.f; const float2 a = X[j]")
    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel(ro, name="xch.hip")
    assert "xch.hip:3" in ei.value.log


@pytest.mark.parametrize("depth", [None, 3])
@pytest.mark.parametrize("declared", [False, True])
def test_the_two_markers_are_independent(depth, declared):
    import rocoder_amd as ra

    src = OTHER.replace("X.channel(1 - h.channel)[j]", "X.channel(1 - h.channel).past(1)[j]")
    if depth is not None:
        src = f"#define RC_HISTORY {depth}\n" + src
    if declared:
        src = "#define RC_CROSS_CHANNEL 1\n" + src
    code = ra.compile_device_kernel(src)
    assert ra.device_kernel_history(code) == (depth or 0)
    assert ra.device_kernel_cross_channel(code) is declared
    assert _symbols(code)["rc_user_dk_history"] == (depth or 0) + 1


@pytest.mark.parametrize("name,depth", [("cross_synth.hip", 0), ("mid_side.hip", 0), ("duck.hip", 2)])
def test_example_kernels_compile(name, depth):
    import rocoder_amd as ra

    with open(os.path.join(EXAMPLES, name)) as f:
        src = f.read()
    code = ra.compile_device_kernel(src, name=name)
    assert ra.device_kernel_cross_channel(code) and ra.device_kernel_history(code) == depth


def test_cli_help_names_the_cross_channel_define():
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "RC_CROSS_CHANNEL" in r.stderr and "RC_HISTORY" in r.stderr


def test_engine_host_code_with_a_declared_kernel_is_clean_under_asan_ubsan():
    """The all-channel bookkeeping of a declared kernel (chunks, channel-subset ranges, the stream rules with channels of
    unequal length, rc_multi spans over four devices) on one window length of each path, over the HIP stub, whose device
    memory is host memory: tests/c/engine_host_driver_xch.cpp under ASan + UBSan."""
    host = os.path.join(ROOT, "rocoder_amd", "csrc", "host")
    r = subprocess.run(["make", "-C", host, "-f", "sanitize.mk", "../../bin/engine_xch_asan"], capture_output=True,
                       text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "rocoder_amd", "bin", "engine_xch_asan")], capture_output=True, text=True,
                       timeout=1800, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "engine_host_driver_xch: ok" in out

"""User device kernels without a GPU: rc_dk_compile is pure host (hiprtc cross-compiles for gfx950), the code object it
returns is checked here with a small ELF reader, and the CLI lists the new flags."""
import ctypes as C
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

X2 = ("__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
      "{ float2 x = X[j]; return make_float2(2.f * x.x, 2.f * x.y); }")


def _L():
    from rocoder_amd import _lib

    return _lib.lib()


def _compile(src: bytes, cap=None):
    L = _L()
    n = C.c_size_t(0)
    log = C.create_string_buffer(1 << 16)
    buf = None if cap is None else C.create_string_buffer(cap)
    rc = L.rc_dk_compile(src, len(src), buf, 0 if cap is None else cap, C.byref(n), log, len(log))
    return rc, n.value, (buf.raw[:n.value] if buf is not None and rc == 0 else None), log.value.decode()


def _elf_symbols(b: bytes):
    """Names in the ELF64 symbol tables of b (SHT_SYMTAB / SHT_DYNSYM)."""
    shoff, = struct.unpack_from("<Q", b, 40)
    shentsize, shnum = struct.unpack_from("<HH", b, 58)
    assert shentsize == 64
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * 64) for i in range(shnum)]
    names = set()
    for _name, typ, _fl, _addr, off, size, link, _info, _al, ent in secs:
        if typ not in (2, 11):
            continue
        stroff, strsize = secs[link][4], secs[link][5]
        for s in range(off, off + size, ent):
            st_name, = struct.unpack_from("<I", b, s)
            end = b.index(b"\0", stroff + st_name)
            names.add(b[stroff + st_name:end].decode())
    return names


def test_compile_readme_x2_gives_a_gfx950_code_object():
    from rocoder_amd import _lib

    src = X2.encode()
    rc, n, _, _ = _compile(src)  # size query
    assert rc == _lib.RC_ECAPACITY and n > 0
    rc, n2, code, log = _compile(src, n - 1)
    assert rc == _lib.RC_ECAPACITY and n2 == n
    rc, n3, code, log = _compile(src, n)
    assert rc == _lib.RC_OK and n3 == n, log
    assert code[:4] == b"\x7fELF" and code[4] == 2 and code[5] == 1
    e_machine, = struct.unpack_from("<H", code, 18)
    e_flags, = struct.unpack_from("<I", code, 48)
    assert e_machine == 224 and e_flags & 0xFF == 0x4F
    assert "rc_user_dk" in _elf_symbols(code)


def test_compile_errors_point_at_the_users_lines():
    from rocoder_amd import _lib

    L = _L()
    src = b'#line 1 "my_kernel.hip"\n// line 1\n// line 2\n  this is not c++;\n' + X2.encode()
    rc, _, _, log = _compile(src, 1 << 16)
    assert rc == _lib.RC_EINVAL
    assert "my_kernel.hip:3" in log, log
    assert "my_kernel.hip:3" in L.rc_last_error().decode()
    rc, _, _, log = _compile(b"// nothing here\n__device__ float2 f(float2 x) { return x; }\n", 1 << 16)
    assert rc == _lib.RC_EINVAL and "rc_apply" in log


def test_python_wrapper_raises_with_the_log():
    import rocoder_amd as ra

    code = ra.compile_device_kernel(X2)
    assert code[:4] == b"\x7fELF"
    with pytest.raises(ra.DeviceKernelCompileError) as ei:
        ra.compile_device_kernel("int x\n" + X2, name="k.hip")
    assert "k.hip:2" in ei.value.log and "error" in ei.value.log
    assert ei.value.code == -1


def test_load_and_params_validate_without_an_engine():
    from rocoder_amd import _lib

    L = _L()
    assert L.rc_engine_load_device_kernel(None, b"x", 1) == _lib.RC_EINVAL
    assert L.rc_engine_set_device_kernel_params(None, None, 0) == _lib.RC_EINVAL
    assert L.rc_multi_load_device_kernel(None, b"x", 1) == _lib.RC_EINVAL


def test_cli_help_lists_the_device_kernel_flags():
    cli = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--device-kernel-src" in r.stderr and "--dk-params" in r.stderr
    r = subprocess.run([cli, "-i", "x.wav", "-o", "y.wav", "--device-kernel-src", "k.hip", "--freq-kernel", "k.c"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0


def test_sanitizer_builds_still_link():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "rocoder_amd", "csrc", "host"), "-f", "sanitize.mk"],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]

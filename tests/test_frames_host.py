"""CPU tests (-m "not gpu") of the interleaved-frames entry point (rc_engine_stretch_frames, --frames-on-gpu): status
codes without a device, the CLI's excluded options, and the engine's arithmetic on the raw frame block under
AddressSanitizer over the HIP stub (tests/c/engine_host_driver_frames.cpp + tests/c/hip_stub_frames.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rocoder_amd import _lib
from wavutil import write_wav

CLI = os.environ.get("ROCODER_CLI") or os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")


def test_entry_point_returns_status_codes_without_an_engine():
    """No crash and no silent success: a null engine, source or target is RC_EINVAL for every format, and so is a
    format outside 1 ... 5 (without a GPU no engine can exist; tests/test_gpu_frames.py repeats this on a real one)."""
    L = _lib.lib()
    assert "rc_engine_stretch_frames" in _lib.SYMBOLS
    assert [_lib.PCM_FORMATS[k] for k in ("u8", "i16", "i24", "i32", "f32")] == [1, 2, 3, 4, 5]
    src = np.zeros(64, np.uint8)
    out = np.zeros(64, np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    n = C.c_size_t(7)
    for fmt in (0, 1, 2, 3, 4, 5, 6):
        assert L.rc_engine_stretch_frames(None, src.ctypes.data, 4, fmt, fp, 16, C.byref(n)) == _lib.RC_EINVAL
        assert L.rc_engine_stretch_frames(None, None, 4, fmt, fp, 16, None) == _lib.RC_EINVAL
        assert L.rc_engine_stretch_frames(None, src.ctypes.data, 0, fmt, None, 0, None) == _lib.RC_EINVAL
    assert n.value == 7 and not out.any()
    assert L.rc_last_error()
    h = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    for name, val in _lib.PCM_FORMATS.items():
        assert f"#define RC_PCM_{name.upper()} {val}\n" in h
    rust = open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read()
    for name, val in _lib.PCM_FORMATS.items():
        assert f"pub const RC_PCM_{name.upper()}: u32 = {val};" in rust


@pytest.mark.parametrize("extra,named", [(["--freq-kernel", "k.c"], "--freq-kernel"),
                                         (["--device-kernel-src", "k.hip"], "--device-kernel-src"),
                                         (["--devices", "0,0"], "--devices"),
                                         (["--rotate-channels"], "--rotate-channels")])
def test_cli_frames_on_gpu_refuses_the_options_it_cannot_serve(tmp_path, extra, named):
    wav, out = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    write_wav(wav, np.zeros((2, 3000)), 44100, "i16")
    r = subprocess.run([CLI, "-i", wav, "-o", out, "--frames-on-gpu", *extra], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and "--frames-on-gpu" in lines[0] and named in lines[0], r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".part")


def test_usage_names_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--frames-on-gpu" in r.stderr


def test_engine_frames_arithmetic_is_clean_under_asan():
    """i24 x 3 channels and u8 x 1, a job of several chunks, sources at odd addresses, 0 and 1 frames, every buffer
    exactly as long as the call says."""
    from test_engine_host_sanitized import _build

    exe = _build("engine_frames_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("engine_host_driver_frames: ok")

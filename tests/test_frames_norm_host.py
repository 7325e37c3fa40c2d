"""CPU tests (-m "not gpu") of peak-normalised PCM output (rc_engine_stretch_frames_norm, --normalize): the symbol in the
header, the ctypes table and the Rust block; status codes without a device; the engine's two-phase bookkeeping under
AddressSanitizer over the HIP stub (tests/c/engine_host_driver_frames_norm.cpp + tests/c/hip_stub_frames_norm.cpp); the
CLI's argument checks. `normalise` is the numpy statement of the definition in include/rocoder_hip.h, which the GPU
tests (tests/test_gpu_frames_norm.py) hold the device to bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rocoder_amd import _lib

CLI = os.environ.get("ROCODER_CLI") or os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
NAME = "rc_engine_stretch_frames_norm"


def normalise(ref, target):
    """The definition: peak = the largest |y| among the samples with |y| < inf (0 where there is none), gain = target /
    peak in ONE f32 division where peak > 0 and the quotient is finite, else 1, z = y * gain in ONE f32 multiplication.
    Returns (z, peak, gain), peak and gain as np.float32."""
    y = np.asarray(ref, np.float32)
    mag = np.abs(y)
    with np.errstate(invalid="ignore"):
        finite = mag < np.float32(np.inf)  # (False for NaN)
    peak = np.float32(mag[finite].max()) if finite.any() else np.float32(0)
    gain = np.float32(1)
    if peak > 0:
        with np.errstate(over="ignore"):
            q = np.float32(target) / peak
        if np.isfinite(q):
            gain = np.float32(q)
    with np.errstate(invalid="ignore", over="ignore"):
        z = (y * gain).astype(np.float32)  # (f32 x f32 in numpy: one IEEE multiplication, denormals kept)
    return z, peak, gain


def test_normalise_follows_the_definition_on_edge_values():
    y = np.array([0.25, -2.0, np.nan, np.inf, -np.inf, 1e-40], np.float32)
    z, peak, gain = normalise(y, 1.0)
    assert peak == np.float32(2) and gain == np.float32(0.5)
    assert z[0] == np.float32(0.125) and z[1] == -1 and np.isnan(z[2]) and z[3] == np.inf and z[4] == -np.inf
    assert z[5] == np.float32(1e-40) * np.float32(0.5) and z[5] != 0, "denormals are kept"
    for dead in (np.zeros(4, np.float32), np.array([np.nan, np.inf], np.float32), np.zeros(0, np.float32)):
        z, peak, gain = normalise(dead, 0.5)
        assert peak == 0 and gain == 1 and z.tobytes() == dead.tobytes()
    z, peak, gain = normalise(np.array([1e-45], np.float32), 1.0)  # the quotient overflows: no gain
    assert peak > 0 and gain == 1
    z, peak, gain = normalise(np.array([3.0, -0.7], np.float32), 1.0)  # peak * gain may round above the target by an ulp
    assert gain == np.float32(1) / np.float32(3) and abs(float(z[0]) - 1) <= 2.0 ** -23


def test_the_symbol_is_declared_in_every_binding():
    assert NAME in _lib.SYMBOLS
    assert len(_lib.SYMBOLS[NAME][1]) == 12
    assert _lib.SYMBOLS[NAME][1][7] is C.c_float
    h = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    m = re.search(r"\nint " + NAME + r"\(([^;]*)\);", h)
    assert m and m.group(1).count(",") == 11, "header: twelve arguments"
    for s in ("float target_peak", "float *peak", "float *gain", "uint64_t *clipped", "uint32_t out_format", "void *out_frames"):
        assert s in m.group(1), s
    for s in ("ONE IEEE f32 division", "ONE IEEE f32 multiplication", "one ulp above target_peak", "|y| < inf", "!(|z| <= 1)",
              "not contracted", "denormals"):
        assert s in h, s
    rust = open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read()
    m = re.search(r"pub fn " + NAME + r"\(([^;]*)\) -> c_int;", rust)
    assert m and m.group(1).count(",") == 11
    for s in ("target_peak: f32", "peak: *mut f32", "gain: *mut f32", "clipped: *mut u64"):
        assert s in m.group(1), s
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.lib().rc_abi_version() == 5


def test_entry_point_returns_status_codes_without_an_engine():
    L = _lib.lib()
    src = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    n, clipped, peak, gain = C.c_size_t(7), C.c_uint64(9), C.c_float(3), C.c_float(4)
    tail = (C.byref(n), C.byref(peak), C.byref(gain), C.byref(clipped))
    for fmt in range(7):
        for ofmt in range(7):
            assert L.rc_engine_stretch_frames_norm(None, src.ctypes.data, 4, fmt, out.ctypes.data, 16, ofmt, 1.0, *tail) == _lib.RC_EINVAL
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.rc_engine_stretch_frames_norm(None, src.ctypes.data, 4, 2, out.ctypes.data, 16, 2, bad, *tail) == _lib.RC_EINVAL
    assert L.rc_engine_stretch_frames_norm(None, None, 4, 2, out.ctypes.data, 16, 2, 1.0, None, None, None, None) == _lib.RC_EINVAL
    assert L.rc_engine_stretch_frames_norm(None, src.ctypes.data, 0, 2, None, 0, 2, 1.0, None, None, None, None) == _lib.RC_EINVAL
    assert (n.value, clipped.value, peak.value, gain.value) == (7, 9, 3.0, 4.0) and not out.any()
    assert L.rc_last_error()


def test_engine_frames_norm_bookkeeping_is_clean_under_asan():
    """Every output format, targets at all four byte phases, several chunks whose edges fall inside a dword, a host
    kernel, 0 and 1 frames. The driver holds the engine to: every output sample through the peak launcher once, all of
    them in front of the first pack launch, the gain stored once, one readback, nothing written on an error."""
    from test_engine_host_sanitized import _build

    exe = _build("engine_frames_norm_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("engine_host_driver_frames_norm: ok")


def test_python_wrapper_refuses_a_bad_level_before_it_touches_an_engine():
    from rocoder_amd.stretcher import Engine

    eng = object.__new__(Engine)  # (no engine behind it: the check comes first)
    for bad in (0, -0.5, float("nan"), float("inf"), 1e-60, 1e60):
        with pytest.raises(ValueError, match="normalize"):
            Engine.stretch_frames(eng, np.zeros((4, 2), np.int16), normalize=bad)


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def test_cli_names_the_flag_and_checks_its_arguments(tmp_path):
    r = run("--help")
    assert r.returncode == 0 and "--normalize" in r.stderr and "--frames-on-gpu" in r.stderr
    out = str(tmp_path / "o.wav")
    r = run("-i", "a.wav", "-o", out, "--normalize", "0.9")
    assert r.returncode != 0 and "--normalize" in r.stderr and "--frames-on-gpu" in r.stderr, r.stderr
    for bad in ("0", "nan", "-1", "inf", "loud"):
        r = run("-i", "a.wav", "-o", out, "--frames-on-gpu", "--normalize", bad)
        assert r.returncode != 0 and "--normalize" in r.stderr, (bad, r.stderr)
    assert not os.path.exists(out)
    assert "--normalize" in open(os.path.join(ROOT, "README.md")).read()

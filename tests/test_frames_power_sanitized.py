"""CPU test (-m "not gpu"): the engine's host code of rc_engine_frames_power, and rc_autocrop_points, under AddressSanitizer
and UndefinedBehaviorSanitizer in a stand-alone program over the HIP stub (tests/c/engine_host_driver_frames_power.cpp +
tests/c/hip_stub_frames_power.cpp; rocoder_amd/csrc/host/sanitize.mk builds it as engine_frames_power_asan). Nothing is
loaded into python."""
import os
import subprocess

from test_engine_host_sanitized import _build


def test_engine_frames_power_asan_runs_clean():
    """Every frame through the launcher exactly once, in launches that follow each other; the bins zeroed in front of the
    first launch and read back once behind the last; nothing written on an error; pageable and page-locked sources at
    every byte phase; 0, 1 and a few frames; rc_autocrop_points' and rc_frames_power_bins' answers and status codes."""
    exe = _build("engine_frames_power_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_frames_power: ok"

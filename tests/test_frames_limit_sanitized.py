"""CPU test (-m "not gpu"): the engine's host code of rc_engine_set_output_limiter under AddressSanitizer and
UndefinedBehaviorSanitizer in a stand-alone program over the HIP stub (tests/c/engine_host_driver_frames_limit.cpp +
tests/c/hip_stub_frames_limit.cpp; rocoder_amd/csrc/host/sanitize.mk builds it as engine_frames_limit_asan). Nothing is
loaded into python."""
import os
import subprocess

from test_engine_host_sanitized import _build


def test_engine_frames_limit_asan_runs_clean():
    """On multi-chunk jobs with and without a resample step and a fade, on all four whole-job host-form entries and under a
    host frequency kernel: the limit launches tile [0, n) once and in order; none reads an input frame its chunk has not
    finished (the stub refuses such a range as the real launcher does) and none waits longer than 2 L frames; the fade
    launches precede the limit launch that reads their frames; the peak, pack and download ranges are the limit launches'
    ranges; the stats words are reset in front of every job and read back; a rejected setter leaves the previous state; a
    cleared engine logs what an engine that never set a limiter logs, and writes the same bytes."""
    exe = _build("engine_frames_limit_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_frames_limit: ok"

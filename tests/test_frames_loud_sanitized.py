"""CPU test (-m "not gpu"): the engine's host code of rc_engine_stretch_frames_loud and its host helpers under
AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program over the HIP stub
(tests/c/engine_host_driver_frames_loud.cpp + tests/c/hip_stub_frames_loud.cpp; rocoder_amd/csrc/host/sanitize.mk builds it as
engine_frames_loud_asan). Nothing is loaded into python."""
import os
import subprocess

from test_engine_host_sanitized import _build


def test_engine_frames_loud_asan_runs_clean():
    """On multi-chunk and tiny jobs, with and without a limiter and a resample step, under a host frequency kernel, at the
    engine's rate and at an explicit one: phase one launches no peak kernel; each measuring launcher runs once, over all
    frames of the rows the job would pack (the limiter's, the resampler's or the hops'), with the coefficients of the
    rate; the loudness, the true peak and the gain are the header's formulas on what the stub measured, a binding ceiling
    included; the pack launches store that gain once and write every byte of the block and nothing else; every rejected
    call leaves the out-pointers and the block untouched; _pcm and _norm behind it run as before; the three host helpers
    read exactly the words they are given."""
    exe = _build("engine_frames_loud_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_frames_loud: ok"

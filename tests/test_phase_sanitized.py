"""CPU tests (-m "not gpu"): the engine's host code of rc_engine_set_phase_mode under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer, in a stand-alone program over the HIP stub
(tests/c/engine_host_driver_phase.cpp + tests/c/hip_stub_phase.cpp; rocoder_amd/csrc/host/sanitize.mk builds it as
engine_phase_asan / engine_phase_tsan). Nothing is loaded into python."""
import os
import subprocess

import pytest

from test_engine_host_sanitized import TSAN, _build


@pytest.mark.parametrize("target,env,marker", [
    ("engine_phase_asan", {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"}, "Sanitizer"),
    ("engine_phase_tsan", TSAN, "WARNING: ThreadSanitizer"),
])
def test_engine_phase_host_code_runs_clean(target, env, marker):
    """Against numbers written out by hand: the launches of every chunk of a three-chunk job in order - analysis with the
    halo hop, prep, scan, walk, apply, the phase-keeping synthesis, the overlap-add; theta zeroed at hop 0 and carried from
    chunk to chunk, call after call; the coherent envelope and the plain amplitude under a mode, the reference's bits again
    behind RANDOM; every refusal in both orders of the two calls; the rows and the chunk table rc_test_phase_tap copies
    out, into arrays of exactly their size, and its refusal of a job that does not fit."""
    exe = _build(target)
    r = subprocess.run([exe], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert marker not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_phase: ok"

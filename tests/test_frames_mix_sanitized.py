"""CPU tests (-m "not gpu"): the engine's host code of rc_engine_mix_frames and rc_engine_bus_frames under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer, in a stand-alone program over the HIP stub
(tests/c/engine_host_driver_frames_mix.cpp + tests/c/hip_stub_frames_mix.cpp; rocoder_amd/csrc/host/sanitize.mk builds it as
engine_frames_mix_asan / engine_frames_mix_tsan). Nothing is loaded into python."""
import os
import subprocess

import pytest

from test_engine_host_sanitized import TSAN, _build


@pytest.mark.parametrize("target,env,marker", [
    ("engine_frames_mix_asan", {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"}, "Sanitizer"),
    ("engine_frames_mix_tsan", TSAN, "WARNING: ThreadSanitizer"),
])
def test_engine_mix_host_code_runs_clean(target, env, marker):
    """Against numbers written out by hand: the mix launches of a three-chunk job tile [0, n) once and in order and cover
    every bus word of the landing range once; the job asks for no copy to the host; under a resampler and a limiter the
    launches end where the two lags say; rc_engine_bus_frames leaves the bus words as they were; every refusal of the
    three entries and of the bus, with the bus untouched; create / destroy of bus and engine in both orders."""
    exe = _build(target)
    r = subprocess.run([exe], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert marker not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_frames_mix: ok"

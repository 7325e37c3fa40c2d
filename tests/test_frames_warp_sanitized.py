"""CPU tests (-m "not gpu"): the engine's host code of rc_engine_set_output_warp under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer, in a stand-alone program over the HIP stub
(tests/c/engine_host_driver_frames_warp.cpp + tests/c/hip_stub_frames_warp.cpp; rocoder_amd/csrc/host/sanitize.mk builds it
as engine_frames_warp_asan / engine_frames_warp_tsan). Nothing is loaded into python."""
import os
import subprocess

import pytest

from test_engine_host_sanitized import TSAN, _build


@pytest.mark.parametrize("target,env,marker", [
    ("engine_frames_warp_asan", {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"}, "Sanitizer"),
    ("engine_frames_warp_tsan", TSAN, "WARNING: ThreadSanitizer"),
])
def test_engine_output_warp_host_code_runs_clean(target, env, marker):
    """Against numbers written out by hand: need[] with a tier that drops between blocks; the warp launches of a
    multi-chunk job tile [0, n_out) once and in order, and each ends at the block the lag names; none reads a row frame
    its chunk has not finished; a block at a step of 8 at a chunk's edge holds the blocks behind it back; the fade, pack
    and download ranges are the warp launches' ranges on all four whole-job entries; the setter's validation and the
    mutual refusal of the two resamplers; a cleared engine logs what an engine that never set a warp logs;
    rc_warp_curve's capacity idiom."""
    exe = _build(target)
    r = subprocess.run([exe], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert marker not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_frames_warp: ok"

"""CPU tests (-m "not gpu"): the engine's host code of rc_engine_set_time_map under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer, in a stand-alone program over the HIP stub
(tests/c/engine_host_driver_timemap.cpp + tests/c/hip_stub_timemap.cpp + tests/c/hip_stub_timemap_hops.cpp; rocoder_amd/csrc/host/sanitize.mk builds it as
engine_timemap_asan / engine_timemap_tsan). Nothing is loaded into python."""
import os
import subprocess

import pytest

from test_engine_host_sanitized import TSAN, _build


@pytest.mark.parametrize("target,env,marker", [
    ("engine_timemap_asan", {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"}, "Sanitizer"),
    ("engine_timemap_tsan", TSAN, "WARNING: ThreadSanitizer"),
])
def test_engine_time_map_host_code_runs_clean(target, env, marker):
    """Against launches written out by hand: the hops every chunk of a map job gathers (the recomputed hop, a history
    kernel's halo, none under a host frequency kernel that carries its tail, the inner passes of a negative pitch); what
    run_hops hands the hop launchers per chunk - in_origin, in_len, a step of N, the rows of that chunk's gather, no padded
    tail - seen through link-time wrappers of rc::launch_hop and rc::launch_prep (tests/c/hip_stub_timemap_hops.cpp); the
    uploads of the host pipeline per chunk for a forward map (each chunk's share, up to its bound) and a reversed one (all
    of it first), and what the stub gathered from them; every whole-job entry's length and capacity check, the setter's validation, the refusal of the range and
    streaming entries while a map is set, and the plain launches once it is cleared; rc_time_map_curve's capacity idiom."""
    exe = _build(target)
    r = subprocess.run([exe], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert marker not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_timemap: ok"

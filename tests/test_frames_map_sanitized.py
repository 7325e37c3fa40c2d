"""CPU test (-m "not gpu"): the engine's host code of rc_engine_set_channel_map and rc_engine_frames_channel_peaks, and
rc_split_mono_map, under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program over the HIP stub
(tests/c/engine_host_driver_frames_map.cpp + tests/c/hip_stub_frames_map.cpp; rocoder_amd/csrc/host/sanitize.mk builds it as
engine_frames_map_asan). Nothing is loaded into python."""
import os
import subprocess

from test_engine_host_sanitized import _build


def test_engine_frames_map_asan_runs_clean():
    """The unmapped launcher with no map and with an identity map - the launches of the engine as it was; with a map, the
    table on the device in front of the first mapped launch and every frame through the mapped launcher exactly once across
    the chunks, on all three frames entries and under a host frequency kernel; a rejected map leaves the previous one. Every
    frame through the channel-peaks launcher exactly once, its words zeroed in front of the first launch and read back once;
    nothing written on an error; pageable and page-locked sources at every byte phase; 0, 1 and a few frames;
    rc_split_mono_map's answers and status codes."""
    exe = _build("engine_frames_map_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_frames_map: ok"

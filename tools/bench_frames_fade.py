"""The output fade (rc_engine_set_output_fade) end to end (PCIe included) on the C2-shaped job of tools/bench_frames_norm.py
(stereo, N = 16384, f = 8, L = 2 646 000 i16 frames in, i16 out), page-locked memory on both sides. 3 warm-ups, then 10
rounds in which the legs take turns in one process; medians and the min-max spread per leg.

  a   rc_engine_stretch_frames_pcm, the fade cleared            (the path as it was: the floor)
  b   rc_engine_stretch_frames_pcm with fades of the CLI's default length: 44 100 frames in, 44 100 out in front of
      min(L * f, the output's length) - this job's output is shorter than L * f, where the CLI would leave the fade-out out
  c0  rc_engine_stretch_frames_norm, the fade cleared
  c1  rc_engine_stretch_frames_norm with those fades            (recorded, not gated)

GATE: the median of b is no slower than the median of a by more than the spread (max - min) of a's ten calls. The fade
launches cover 88 200 of the job's 21 million frames and sit on the engine's stream beside the copies.
From a run of its own under `rocprofv3 --kernel-trace --stats` (a fresh child process, 3 calls of leg b): the time per
launch of the fade kernel.
usage: python tools/bench_frames_fade.py [--no-trace] [out.json]"""
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rocoder_amd  # noqa: E402
from rocoder_amd import _lib  # noqa: E402

CH, N, F, L = 2, 16384, 8.0, 2_646_000
WARM, ROUNDS = 3, 10
TARGET = 0.9
FADE = 44_100


def job():
    eng = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
    n_out = eng.output_len(L)
    i16 = rocoder_amd.pinned_empty((L, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (L, CH), dtype=np.int64)
    yb = rocoder_amd.pinned_empty(n_out * CH * 2, np.uint8)
    end = min(int(np.float32(L) * np.float32(F)), n_out)  # (the CLI's expected_total_samples, where the output has them)
    assert 2 * FADE <= end
    return eng, n_out, i16, yb, (FADE, end - FADE, FADE)


def call_legs():
    eng, n_out, i16, yb, fade = job()

    def leg(faded, normalize):
        def run():
            eng.set_output_fade(*(fade if faded else ()))
            return eng.stretch_frames(i16, out=yb, out_fmt="i16", normalize=normalize)
        return run

    legs = [("a_pcm_fade_cleared", leg(False, None)), ("b_pcm_faded", leg(True, None)),
            ("c0_norm_fade_cleared", leg(False, TARGET)), ("c1_norm_faded", leg(True, TARGET))]
    times = {name: [] for name, _ in legs}
    for r in range(WARM + ROUNDS):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[name].append(dt)
    plain = legs[0][1]().copy()
    faded = legs[1][1]().copy()
    # the fade changed the first and the last frames it covers, and nothing in between
    mid = slice(fade[0] * CH * 2, fade[1] * CH * 2)
    sane = bool(np.array_equal(plain[mid], faded[mid]) and not np.array_equal(plain[:mid.start], faded[:mid.start])
                and not faded[(fade[1] + fade[2]) * CH * 2:].any())
    eng.close()
    return dict(frames=L, out_frames=n_out, fade=dict(in_len=fade[0], out_start=fade[1], out_len=fade[2]), ms=times,
                faded_bytes_differ_only_inside_the_fades=sane)


def traced_child():
    eng, n_out, i16, yb, fade = job()
    eng.set_output_fade(*fade)
    for _ in range(3):
        eng.stretch_frames(i16, out=yb, out_fmt="i16")
    eng.close()


def kernel_times():
    if not shutil.which("rocprofv3"):
        return {"error": "no rocprofv3 on PATH: not measured"}
    d = tempfile.mkdtemp(prefix="rc_fade_trace_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                            os.path.abspath(__file__), "--traced-child"], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": f"rocprofv3 exited {r.returncode}: {r.stderr[-400:]}"}
        rows = {}
        for f in glob.glob(d + "/**/*kernel_stats.csv", recursive=True):
            for row in csv.DictReader(open(f)):
                if "frames_" in row["Name"]:
                    rows[row["Name"]] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3,
                                             min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
        return rows or {"error": "no frames kernel in the stats file"}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    if "--traced-child" in sys.argv[1:]:
        traced_child()
        return 0
    args = [a for a in sys.argv[1:] if a != "--no-trace"]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r13_frames_fade.json")
    res = {"job": dict(channels=CH, window_len=N, factor=F, target_peak=TARGET), "warmups": WARM, "rounds": ROUNDS}
    if "--no-trace" not in sys.argv[1:]:  # (first: its child is the only process with the GPU open while it runs)
        res["kernel_us_per_launch"] = kernel_times()
        print("kernel times:", json.dumps(res["kernel_us_per_launch"], indent=1), flush=True)
    res["kernel_id"] = _lib.lib().rc_kernel_id().decode()
    res.update(call_legs())
    summ = res["summary"] = {}
    for k, v in res["ms"].items():
        summ[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:24s} median {summ[k]['median']:9.3f} ms   min {summ[k]['min']:9.3f}   max {summ[k]['max']:9.3f}", flush=True)
    a, b = summ["a_pcm_fade_cleared"], summ["b_pcm_faded"]
    res["gate"] = dict(b_minus_a_ms=b["median"] - a["median"], spread_of_a_ms=a["max"] - a["min"],
                       passed=bool(b["median"] - a["median"] <= a["max"] - a["min"]))
    res["norm_faded_over_cleared"] = summ["c1_norm_faded"]["median"] / summ["c0_norm_fade_cleared"]["median"]
    print("gate:", res["gate"], "  bytes differ only inside the fades:", res["faded_bytes_differ_only_inside_the_fades"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    return 0 if res["gate"]["passed"] and res["faded_bytes_differ_only_inside_the_fades"] else 1


if __name__ == "__main__":
    sys.exit(main())

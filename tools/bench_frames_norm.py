"""rc_engine_stretch_frames_norm end to end (PCIe included) on the C2-shaped job of tools/bench_frames.py (stereo,
N = 16384, f = 8, L = 2 646 000 i16 frames in; --long: the full C2 length, ten times that), page-locked memory on both
sides. 3 warm-ups, then 10 rounds in which the legs take turns in one process; medians and the min-max spread per leg.

  a  rc_engine_stretch_frames_norm, i16 out                    (two phases: compute + peak, then pack with the gain + download)
  b  rc_engine_stretch_frames_pcm, i16 out                     (the floor: the same bytes moved, no second phase)
  c  rc_engine_stretch_frames, f32 out, then peak, scale and quantise in numpy on the host
     (what a caller has to do without the new entry; both pieces exist unchanged on the parent commit)

and, from a run of its own under `rocprofv3 --kernel-trace --stats` (a fresh child process, 3 calls of leg a), the time
per launch of the peak kernel and of the pack kernel with and without the gain. Recorded: the ratios a / b and a / c of
the medians, and whether a's bytes equal c's.
usage: python tools/bench_frames_norm.py [--long] [--no-trace] [out.json]"""
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


def job(n_in):
    eng = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
    n_out = eng.output_len(n_in)
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    yf = rocoder_amd.pinned_empty((n_out, CH))
    yb = rocoder_amd.pinned_empty(n_out * CH * 2, np.uint8)
    return eng, n_out, i16, yf, yb


def host_normalise(eng, i16, yf):
    """leg c: the floats to the host, then what the definition says, in numpy"""
    y = eng.stretch_frames(i16, out=yf)
    mag = np.abs(y)
    peak = mag[np.isfinite(mag)].max()
    gain = np.float32(TARGET) / peak
    z = y * gain
    z *= np.float32(32767)
    np.rint(z, out=z)
    np.clip(z, -32768, 32767, out=z)
    return z.astype("<i2")


def call_legs(n_in, rounds):
    eng, n_out, i16, yf, yb = job(n_in)
    legs = [("a_stretch_frames_norm_i16_out", lambda: eng.stretch_frames(i16, out=yb, out_fmt="i16", normalize=TARGET)),
            ("b_stretch_frames_pcm_i16_out", lambda: eng.stretch_frames(i16, out=yb, out_fmt="i16")),
            ("c_stretch_frames_f32_out_then_numpy", lambda: host_normalise(eng, i16, yf))]
    times = {name: [] for name, _ in legs}
    for r in range(WARM + rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[name].append(dt)
    got = eng.stretch_frames(i16, out=yb, out_fmt="i16", normalize=TARGET)
    peak, gain, clipped = float(eng.last_peak), float(eng.last_gain), eng.last_clipped
    equal = bool(np.array_equal(got, host_normalise(eng, i16, yf)))
    eng.close()
    return dict(frames=n_in, out_frames=n_out, ms=times, norm_bytes_equal_the_host_route=equal, peak=peak, gain=gain, clipped=clipped)


def traced_child():
    eng, n_out, i16, yf, yb = job(L)
    for _ in range(3):
        eng.stretch_frames(i16, out=yb, out_fmt="i16", normalize=TARGET)
        eng.stretch_frames(i16, out=yb, out_fmt="i16")
    eng.close()


def kernel_times():
    """per-launch times of the frames kernels, from rocprofv3's stats of a fresh child that runs legs a and b three times"""
    if not shutil.which("rocprofv3"):
        return {"error": "no rocprofv3 on PATH: not measured"}
    d = tempfile.mkdtemp(prefix="rc_norm_trace_")
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


def summarise(times):
    summ = {}
    for k, v in times.items():
        summ[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:40s} median {summ[k]['median']:9.3f} ms   min {summ[k]['min']:9.3f}   max {summ[k]['max']:9.3f}", flush=True)
    return summ


def ratios(summ):
    a, b, c = (summ[k]["median"] for k in ("a_stretch_frames_norm_i16_out", "b_stretch_frames_pcm_i16_out", "c_stretch_frames_f32_out_then_numpy"))
    return dict(a_over_b=a / b, a_over_c=a / c)


def main():
    if "--traced-child" in sys.argv[1:]:
        traced_child()
        return 0
    flags = ("--long", "--no-trace")
    args = [a for a in sys.argv[1:] if a not in flags]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r12_frames_norm.json")
    res = {"job": dict(channels=CH, window_len=N, factor=F, target_peak=TARGET), "warmups": WARM, "rounds": ROUNDS}
    if "--no-trace" not in sys.argv[1:]:  # (first: its child is the only process with the GPU open while it runs)
        res["kernel_us_per_launch"] = kernel_times()
        print("kernel times:", json.dumps(res["kernel_us_per_launch"], indent=1), flush=True)
    res["kernel_id"] = _lib.lib().rc_kernel_id().decode()
    short = res["short"] = call_legs(L, ROUNDS)
    short["summary"] = summarise(short["ms"])
    short["ratios"] = ratios(short["summary"])
    print("ratios:", short["ratios"], "  bytes equal the host route:", short["norm_bytes_equal_the_host_route"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    if "--long" in sys.argv[1:]:
        print("the full C2 length:", flush=True)
        long_ = res["long"] = call_legs(10 * L, 5)
        long_["summary"] = summarise(long_["ms"])
        long_["ratios"] = ratios(long_["summary"])
        print("ratios:", long_["ratios"], flush=True)
        json.dump(res, open(out_path, "w"), indent=1)
    return 0 if short["norm_bytes_equal_the_host_route"] else 1


if __name__ == "__main__":
    sys.exit(main())

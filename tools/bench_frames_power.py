"""rc_engine_frames_power end to end (PCIe included): the per-bin peaks of an i16 stereo block of 2 646 000 frames (--long:
the C2 length, 26 460 000) in bins of 100 ms (4 410 frames), the block in page-locked memory. 3 warm-ups, then 10 rounds in
which the legs take turns in one process; median [min - max] per leg.

  a  rc_engine_frames_power                                    (chunked uploads, the power kernel of a chunk under the next upload)
  b  one hipMemcpy of the same bytes from the same page-locked block to the device        (the floor: nothing is computed)
  c  decode, abs and np.maximum.reduceat in numpy on the host  (what a caller has without the entry: the parent commit's offer)

Recorded: a / b and a / c of the medians, a - b beside the spread (max - min) of b's ten calls, whether a's bins equal c's
bit for bit, and, from a run of its own under `rocprofv3 --kernel-trace --stats` (a fresh child process, 3 calls of leg a),
the time per launch of frames_power_kernel and the bytes per second that gives.
usage: python tools/bench_frames_power.py [--long] [--no-trace] [out.json]"""
import csv
import ctypes as C
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

CH, L, BIN = 2, 2_646_000, 4410
WARM, ROUNDS = 3, 10


def job(n_in):
    eng = rocoder_amd.Engine(window_len=1024, factor=2.0, channels=CH, seed=1)
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    return eng, i16


def host_bins(i16):
    """leg c: the reader's decode, abs, a maximum per frame and per bin"""
    x = i16.astype(np.float32)
    x /= np.float32(32767)
    np.abs(x, out=x)
    return np.maximum.reduceat(x.max(axis=1), np.arange(0, i16.shape[0], BIN))


class Floor:
    """leg b: hipMalloc once, then one blocking hipMemcpy per call"""

    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.d = C.c_void_p()
        self.nbytes = nbytes
        assert self.hip.hipMalloc(C.byref(self.d), C.c_size_t(nbytes)) == 0

    def __call__(self, host):
        assert self.hip.hipMemcpy(self.d, C.c_void_p(host.ctypes.data), C.c_size_t(self.nbytes), 1) == 0  # hipMemcpyHostToDevice

    def close(self):
        self.hip.hipFree(self.d)


def call_legs(n_in, rounds):
    eng, i16 = job(n_in)
    floor = Floor(i16.nbytes)
    legs = [("a_frames_power", lambda: eng.frames_power(i16, bin_frames=BIN)),
            ("b_one_hipMemcpy", lambda: floor(i16)),
            ("c_numpy_on_the_host", lambda: host_bins(i16))]
    times = {name: [] for name, _ in legs}
    for r in range(WARM + rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[name].append(dt)
    equal = bool(np.array_equal(eng.frames_power(i16, bin_frames=BIN).view(np.uint32), host_bins(i16).view(np.uint32)))
    floor.close()
    eng.close()
    return dict(frames=n_in, bytes=int(i16.nbytes), bins=-(-n_in // BIN), ms=times, bins_equal_the_host_route=equal)


def traced_child():
    eng, i16 = job(L)
    for _ in range(3):
        eng.frames_power(i16, bin_frames=BIN)
    eng.close()


def kernel_times():
    if not shutil.which("rocprofv3"):
        return {"error": "no rocprofv3 on PATH: not measured"}
    d = tempfile.mkdtemp(prefix="rc_power_trace_")
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
        for name, row in rows.items():
            if "frames_power" in name:  # a launch: one upload chunk of 16 MiB (the last one shorter: the average reads low)
                chunk = min(16 << 20, L * CH * 2)
                row["chunk_bytes"] = chunk
                row["gb_per_s_at_min_us"] = chunk / row["min_us"] / 1e3
        return rows or {"error": "no frames kernel in the stats file"}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def summarise(times):
    summ = {}
    for k, v in times.items():
        summ[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:24s} median {summ[k]['median']:9.3f} ms   [{summ[k]['min']:9.3f} - {summ[k]['max']:9.3f}]", flush=True)
    return summ


def ratios(summ):
    a, b, c = (summ[k]["median"] for k in ("a_frames_power", "b_one_hipMemcpy", "c_numpy_on_the_host"))
    fb = summ["b_one_hipMemcpy"]
    return dict(a_over_b=a / b, a_over_c=a / c, a_minus_b_ms=a - b, spread_of_b_ms=fb["max"] - fb["min"])


def main():
    if "--traced-child" in sys.argv[1:]:
        traced_child()
        return 0
    flags = ("--long", "--no-trace")
    args = [a for a in sys.argv[1:] if a not in flags]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r15_frames_power.json")
    res = {"job": dict(channels=CH, format="i16", bin_frames=BIN), "warmups": WARM, "rounds": ROUNDS}
    if "--no-trace" not in sys.argv[1:]:  # (first: its child is the only process with the GPU open while it runs)
        res["kernel_us_per_launch"] = kernel_times()
        print("kernel times:", json.dumps(res["kernel_us_per_launch"], indent=1), flush=True)
    res["kernel_id"] = _lib.lib().rc_kernel_id().decode()
    short = res["short"] = call_legs(L, ROUNDS)
    short["summary"] = summarise(short["ms"])
    short["ratios"] = ratios(short["summary"])
    print("ratios:", short["ratios"], "  bins equal the host route:", short["bins_equal_the_host_route"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    if "--long" in sys.argv[1:]:
        print("the C2 length:", flush=True)
        long_ = res["long"] = call_legs(10 * L, ROUNDS)
        long_["summary"] = summarise(long_["ms"])
        long_["ratios"] = ratios(long_["summary"])
        print("ratios:", long_["ratios"], "  bins equal the host route:", long_["bins_equal_the_host_route"], flush=True)
        json.dump(res, open(out_path, "w"), indent=1)
    return 0 if short["bins_equal_the_host_route"] else 1


if __name__ == "__main__":
    sys.exit(main())

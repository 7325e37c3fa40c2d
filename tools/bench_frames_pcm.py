"""rc_engine_stretch_frames_pcm against rc_engine_stretch_frames, end to end (PCIe included), on the job of
tools/bench_frames.py (stereo, N = 16384, f = 8, L = 2 646 000 i16 frames in), page-locked memory on both sides. 3
warm-ups, then 10 rounds in which the legs take turns in one process; medians and the min-max spread per leg.

  a  rc_engine_stretch_frames, f32 out                         (the merged code: the yardstick)
  b  rc_engine_stretch_frames_pcm, f32 out
  c  the same, i16 out (half the download)
  d  the same, i24 out (three quarters of it)
  e  HIP-event time of one pack launch per output format on the job's buffers, next to the f32 pack kernel and a
     device-to-device hipMemcpyAsync of the bytes they all read

Gate: median(b) and median(c) each <= median(a) + (max(a) - min(a)). The gain of c and d over a is recorded,
not gated. With --long the full C2 length (26 460 000 frames in, 1.69 GB of f32 out) is measured as well, where the
download is what the call waits for.
usage: python tools/bench_frames_pcm.py [--long] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rocoder_amd  # noqa: E402
from bench_frames import PackParams, launcher  # noqa: E402
from rocoder_amd import _lib  # noqa: E402

CH, N, F, L = 2, 16384, 8.0, 2_646_000
WARM, ROUNDS = 3, 10
BYTES = {"u8": 1, "i16": 2, "i24": 3, "i32": 4, "f32": 4}


class PackPcmParams(C.Structure):  # rc::FramesPackPcmParams (rocoder_amd/csrc/rc_frames.h)
    _fields_ = [("planar", C.c_void_p), ("stride", C.c_uint64), ("target", C.c_void_p), ("phase", C.c_uint32),
                ("channels", C.c_uint32), ("n_frames", C.c_uint64), ("clipped", C.c_void_p)]


def kernel_legs(Lib, n_out):
    hip = Lib  # (dlsym on the engine library's handle also searches the HIP runtime it is linked against)
    for f, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                    ("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                    ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
                    ("hipMemcpyAsync", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
                    ("hipMemset", [C.c_void_p, C.c_int, C.c_size_t]), ("hipDeviceSynchronize", [])):
        getattr(hip, f).argtypes = args
        getattr(hip, f).restype = C.c_int

    def dmalloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        assert hip.hipMemset(p, 0, nbytes) == 0
        return p

    pack = launcher(Lib, "launch_frames_pack")
    pack.argtypes = [C.POINTER(PackParams), C.c_void_p]
    pack_pcm = launcher(Lib, "launch_frames_pack_pcm")
    pack_pcm.argtypes = [C.c_uint32, C.POINTER(PackPcmParams), C.c_void_p]
    d_out, d_frames, d_clip = dmalloc(n_out * CH * 4), dmalloc(n_out * CH * 4 + 16), dmalloc(8)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def timed(fn):
        ts = []
        for i in range(WARM + ROUNDS):
            assert hip.hipEventRecord(ev0, None) == 0
            assert fn() == 0
            assert hip.hipEventRecord(ev1, None) == 0 and hip.hipEventSynchronize(ev1) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
            if i >= WARM:
                ts.append(ms.value)
        return ts

    pk = PackParams(d_out.value, n_out, d_frames.value, n_out, CH)
    legs = {"pack_f32_kernel_ms": timed(lambda: pack(C.byref(pk), None))}
    for name, code in _lib.PCM_FORMATS.items():
        for phase in (0, 1):
            q = PackPcmParams(d_out.value, n_out, d_frames.value, phase, CH, n_out, d_clip.value)
            legs[f"pack_pcm_{name}_phase{phase}_ms"] = timed(lambda: pack_pcm(code, C.byref(q), None))
    legs["d2d_of_the_bytes_read_ms"] = timed(lambda: hip.hipMemcpyAsync(d_frames, d_out, n_out * CH * 4, 3, None))
    hip.hipDeviceSynchronize()
    for p in (d_out, d_frames, d_clip):
        hip.hipFree(p)
    return legs


def call_legs(n_in, rounds):
    eng = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
    n_out = eng.output_len(n_in)
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    yf = rocoder_amd.pinned_empty((n_out, CH))
    yb = rocoder_amd.pinned_empty(n_out * CH * 4, np.uint8)
    legs = [("a_stretch_frames_f32_out", lambda: eng.stretch_frames(i16, out=yf)),
            ("b_stretch_frames_pcm_f32_out", lambda: eng.stretch_frames(i16, out=yb, out_fmt="f32")),
            ("c_stretch_frames_pcm_i16_out", lambda: eng.stretch_frames(i16, out=yb, out_fmt="i16")),
            ("d_stretch_frames_pcm_i24_out", lambda: eng.stretch_frames(i16, out=yb, out_fmt="i24"))]
    times = {name: [] for name, _ in legs}
    for r in range(WARM + rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[name].append(dt)
    ref = eng.stretch_frames(i16, out=yf)
    equal = bool(np.array_equal(eng.stretch_frames(i16, out=yb, out_fmt="f32").view(np.uint32), ref.view(np.uint32)))
    clipped = eng.last_clipped
    eng.close()
    return dict(frames=n_in, out_frames=n_out, ms=times, f32_out_equals_the_f32_entry=equal, clipped=clipped)


def summarise(times):
    summ = {}
    for k, v in times.items():
        summ[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:36s} median {summ[k]['median']:9.3f} ms   min {summ[k]['min']:9.3f}   max {summ[k]['max']:9.3f}", flush=True)
    return summ


def main():
    args = [a for a in sys.argv[1:] if a != "--long"]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r11_frames_pcm.json")
    Lib = _lib.lib()
    short = call_legs(L, ROUNDS)
    res = {"job": dict(channels=CH, window_len=N, factor=F), "warmups": WARM, "rounds": ROUNDS,
           "kernel_id": Lib.rc_kernel_id().decode(), "short": short}
    summ = short["summary"] = summarise(short["ms"])
    res["kernel_ms"] = kernel_legs(Lib, short["out_frames"])
    res["kernel_summary"] = summarise(res["kernel_ms"])
    a, b, c = (summ[k] for k in ("a_stretch_frames_f32_out", "b_stretch_frames_pcm_f32_out", "c_stretch_frames_pcm_i16_out"))
    spread = a["max"] - a["min"]
    res["gate"] = dict(a_median=a["median"], a_spread=spread, b_median=b["median"], c_median=c["median"],
                       passed=b["median"] <= a["median"] + spread and c["median"] <= a["median"] + spread)
    print("f32 out == the f32 entry:", short["f32_out_equals_the_f32_entry"], "  gate:", res["gate"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    if "--long" in sys.argv[1:]:
        print("the full C2 length:", flush=True)
        long_ = call_legs(10 * L, 5)
        long_["summary"] = summarise(long_["ms"])
        res["long"] = long_
        json.dump(res, open(out_path, "w"), indent=1)
    return 0 if res["gate"]["passed"] and short["f32_out_equals_the_f32_entry"] else 1


if __name__ == "__main__":
    sys.exit(main())

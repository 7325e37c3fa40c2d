"""rc_engine_set_output_resample against the unresampled rc_engine_stretch_frames_pcm, end to end (PCIe included), on the job
and by the protocol of tools/bench_frames_pcm.py: stereo, N = 16384, f = 8, L = 2 646 000 i16 frames in, page-locked memory on
both sides; 3 warm-ups, then 10 rounds in which the legs take turns in one process; medians and the min-max spread per leg.

  a  i16 out, no step set                                      (the merged code: the yardstick)
  b  160/147   (48 kHz material delivered at 44.1 kHz)
  c  147/160   (the other way)
  d  1069/1009 (a semitone: 1009 table rows)
  e  2/1       (an octave: one row of 128 taps)
  f  HIP-event time of one resample launch per ratio on the job's rows, next to a device-to-device hipMemcpyAsync of the
     bytes it reads plus writes

Gates (read next to the parent commit's tools/bench_frames_pcm.py i16 leg of the same visit): median(a) inside that leg's
min - max - the cleared state costs nothing. The resampled legs are recorded as ratios to (a) and to their copy, not gated.
usage: python tools/bench_frames_resample.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rocoder_amd  # noqa: E402
from bench_frames import launcher  # noqa: E402
from bench_frames_pcm import CH, F, L, N, ROUNDS, WARM, summarise  # noqa: E402
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import resample_len, resample_table  # noqa: E402

LEGS = [("a_none", None), ("b_160_147", (160, 147)), ("c_147_160", (147, 160)), ("d_1069_1009", (1069, 1009)), ("e_2_1", (2, 1))]


class ResampleParams(C.Structure):  # rc::FramesResampleParams (rocoder_amd/csrc/rc_frames.h)
    _fields_ = [("src", C.c_void_p), ("src0", C.c_uint64), ("src_len", C.c_uint64), ("stride", C.c_uint64), ("channels", C.c_uint32),
                ("n", C.c_uint64), ("table", C.c_void_p), ("num", C.c_uint32), ("den", C.c_uint32), ("W", C.c_uint32),
                ("dst", C.c_void_p), ("dst_stride", C.c_uint64), ("m0", C.c_uint64), ("m1", C.c_uint64)]


def kernel_legs(Lib, n):
    hip = Lib  # (dlsym on the engine library's handle also searches the HIP runtime it is linked against)
    for f, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                    ("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                    ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
                    ("hipMemcpyAsync", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
                    ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
                    ("hipMemset", [C.c_void_p, C.c_int, C.c_size_t]), ("hipDeviceSynchronize", [])):
        getattr(hip, f).argtypes = args
        getattr(hip, f).restype = C.c_int

    def dmalloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        assert hip.hipMemset(p, 0, nbytes) == 0
        return p

    resample = launcher(Lib, "launch_frames_resample")
    resample.argtypes = [C.POINTER(ResampleParams), C.c_void_p]
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

    d_rows = dmalloc(n * CH * 4)
    legs = {}
    for name, step in LEGS[1:]:
        num, den = step
        table = resample_table(num, den)
        n_rs = resample_len(n, num, den)
        d_table, d_rs, d_copy = dmalloc(table.nbytes), dmalloc(n_rs * CH * 4), dmalloc((n + n_rs) * CH * 4)
        assert hip.hipMemcpy(d_table, table.ctypes.data, table.nbytes, 1) == 0
        q = ResampleParams(d_rows.value, 0, n, n, CH, n, d_table.value, num, den, table.shape[1] // 2, d_rs.value, n_rs, 0, n_rs)
        legs[f"resample_{name[2:]}_ms"] = timed(lambda: resample(C.byref(q), None))
        # the bytes the launch reads plus writes, as one device-to-device copy moves them (a copy reads and writes each byte)
        half = (n + n_rs) * CH * 4 // 2
        legs[f"d2d_{name[2:]}_ms"] = timed(lambda: hip.hipMemcpyAsync(d_copy, C.c_void_p(d_copy.value + half), half, 3, None))
        hip.hipDeviceSynchronize()
        for p in (d_table, d_rs, d_copy):
            hip.hipFree(p)
    hip.hipFree(d_rows)
    return legs


def call_legs(n_in, rounds):
    """an engine per leg, so that the legs take turns without a setter call inside the timed region"""
    engs = {}
    for name, step in LEGS:
        engs[name] = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
        if step:
            engs[name].set_output_resample(*step)
    n_rows = engs["a_none"].output_len(n_in)
    n_max = max(resample_len(n_rows, *step) if step else n_rows for _, step in LEGS)
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    yb = rocoder_amd.pinned_empty(n_max * CH * 2, np.uint8)
    times = {name: [] for name, _ in LEGS}
    frames = {}
    for r in range(WARM + rounds):
        for name, _ in LEGS:
            t0 = time.perf_counter()
            got = engs[name].stretch_frames(i16, out=yb, out_fmt="i16")
            dt = (time.perf_counter() - t0) * 1e3
            frames[name] = int(got.shape[0])
            if r >= WARM:
                times[name].append(dt)
    for e in engs.values():
        e.close()
    return dict(frames=n_in, row_frames=n_rows, out_frames=frames, ms=times)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18_frames_resample.json")
    Lib = _lib.lib()
    short = call_legs(L, ROUNDS)
    res = {"job": dict(channels=CH, window_len=N, factor=F), "warmups": WARM, "rounds": ROUNDS,
           "kernel_id": Lib.rc_kernel_id().decode(), "short": short}
    summ = short["summary"] = summarise(short["ms"])
    res["kernel_ms"] = kernel_legs(Lib, short["row_frames"])
    ks = res["kernel_summary"] = summarise(res["kernel_ms"])
    a = summ["a_none"]
    res["ratios"] = {name: dict(to_a=summ[name]["median"] / a["median"],
                                launch_to_its_copy=ks[f"resample_{name[2:]}_ms"]["median"] / ks[f"d2d_{name[2:]}_ms"]["median"])
                     for name, step in LEGS if step}
    res["a_spread"] = a["max"] - a["min"]
    print("ratios:", res["ratios"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

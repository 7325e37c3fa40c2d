"""rc_engine_set_output_limiter against the unlimited rc_engine_stretch_frames_pcm, end to end (PCIe included), on the job
and by the protocol of tools/bench_frames_pcm.py: stereo, N = 16384, f = 8, L = 2 646 000 i16 frames in, page-locked memory on
both sides; 3 warm-ups, then 10 rounds in which the legs take turns in one process; medians and the min-max spread per leg.

  a  i16 out, the limiter cleared                              (the merged code: the yardstick)
  b  the limiter set, a look-ahead of 64 frames
  c  the limiter set, a look-ahead of 2048 frames
  d  HIP-event time of one limit launch on the job's rows at both look-aheads, next to a device-to-device hipMemcpyAsync
     of the bytes it reads plus writes

Gate (read next to the parent commit's tools/bench_frames_pcm.py i16 leg of the same visit): median(a) inside that leg's
min - max - the cleared state costs nothing. The limited legs are recorded as ratios to (a) and to the copy, not gated.
usage: python tools/bench_frames_limiter.py [out.json]"""
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

LEGS = [("a_none", None), ("b_L64", 64), ("c_L2048", 2048)]
DRIVE, CEILING = 1.0, 0.25  # (the input is noise of +-0.49: about a third of the frames are turned down)


class LimitParams(C.Structure):  # rc::FramesLimitParams (rocoder_amd/csrc/rc_frames.h)
    _fields_ = [("src", C.c_void_p), ("src0", C.c_uint64), ("src_len", C.c_uint64), ("stride", C.c_uint64), ("channels", C.c_uint32),
                ("n", C.c_uint64), ("drive", C.c_float), ("ceiling", C.c_float), ("L", C.c_uint32), ("dst", C.c_void_p),
                ("dst_stride", C.c_uint64), ("t0", C.c_uint64), ("t1", C.c_uint64), ("scratch", C.c_void_p), ("scratch_words", C.c_uint64),
                ("stats", C.c_void_p)]


def kernel_legs(Lib, n, rows_host):
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

    limit = launcher(Lib, "launch_frames_limit")
    limit.argtypes = [C.POINTER(LimitParams), C.c_void_p]
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

    d_rows, d_out, d_copy, d_words = dmalloc(n * CH * 4), dmalloc(n * CH * 4), dmalloc(2 * n * CH * 4), dmalloc(16)
    assert rows_host.shape == (CH, n) and rows_host.dtype == np.float32 and rows_host.flags.c_contiguous
    assert hip.hipMemcpy(d_rows, rows_host.ctypes.data, rows_host.nbytes, 1) == 0
    legs = {}
    for name, look in LEGS[1:]:
        q = LimitParams(d_rows.value, 0, n, n, CH, n, DRIVE, CEILING, look, d_out.value, n, 0, n, None, 0, d_words.value)
        legs[f"limit_{name[2:]}_ms"] = timed(lambda: limit(C.byref(q), None))
    # the bytes a launch reads plus writes, as one device-to-device copy moves them (a copy reads and writes each byte)
    half = n * CH * 4
    legs["d2d_ms"] = timed(lambda: hip.hipMemcpyAsync(d_copy, C.c_void_p(d_copy.value + half), half, 3, None))
    hip.hipDeviceSynchronize()
    for p in (d_rows, d_out, d_copy, d_words):
        hip.hipFree(p)
    return legs


def call_legs(n_in, rounds):
    """an engine per leg, so that the legs take turns without a setter call inside the timed region"""
    engs = {}
    for name, look in LEGS:
        engs[name] = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
        if look is not None:
            engs[name].set_output_limiter(DRIVE, CEILING, look)
    n_out = engs["a_none"].output_len(n_in)
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    yb = rocoder_amd.pinned_empty(n_out * CH * 2, np.uint8)
    times = {name: [] for name, _ in LEGS}
    stats = {}
    for r in range(WARM + rounds):
        for name, look in LEGS:
            t0 = time.perf_counter()
            engs[name].stretch_frames(i16, out=yb, out_fmt="i16")
            dt = (time.perf_counter() - t0) * 1e3
            if look is not None:
                g, f = engs[name].last_limiter_stats
                stats[name] = dict(min_gain=float(g), limited_frames=f)
            if r >= WARM:
                times[name].append(dt)
    rows = np.ascontiguousarray(engs["a_none"].stretch_frames(i16).T)  # the job's unlimited rows, for the launch legs
    for e in engs.values():
        e.close()
    return dict(frames=n_in, out_frames=n_out, ms=times, stats=stats), rows


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r19_frames_limiter.json")
    Lib = _lib.lib()
    short, rows = call_legs(L, ROUNDS)
    res = {"job": dict(channels=CH, window_len=N, factor=F, drive=DRIVE, ceiling=CEILING), "warmups": WARM, "rounds": ROUNDS,
           "kernel_id": Lib.rc_kernel_id().decode(), "short": short}
    summ = short["summary"] = summarise(short["ms"])
    res["kernel_ms"] = kernel_legs(Lib, short["out_frames"], rows)
    ks = res["kernel_summary"] = summarise(res["kernel_ms"])
    a = summ["a_none"]
    res["ratios"] = {name: dict(to_a=summ[name]["median"] / a["median"],
                                launch_to_the_copy=ks[f"limit_{name[2:]}_ms"]["median"] / ks["d2d_ms"]["median"])
                     for name, look in LEGS if look is not None}
    res["a_spread"] = a["max"] - a["min"]
    print("ratios:", res["ratios"], "stats:", short["stats"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

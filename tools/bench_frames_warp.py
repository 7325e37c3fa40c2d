"""rc_engine_set_output_warp against the rational resampler and the unresampled rc_engine_stretch_frames_pcm, end to end (PCIe
included), on the job and by the protocol of tools/bench_frames_resample.py: stereo, N = 16384, f = 8, L = 2 646 000 i16 frames
in, page-locked memory on both sides; 3 warm-ups, then 10 rounds in which the legs take turns in one process; medians and the
min-max spread per leg.

  a   i16 out, neither set                                     (the merged code: the yardstick)
  b/c the warp at a constant 160/147 (anchors of round(160/147 * 2^38)), and the rational step 160/147
  d/e the warp at a constant 2/1, and the rational step 2/1
  f   the warp on a glide from 0.5 to 2 along the input
  g   HIP-event time of one warp launch per leg on the job's rows, next to the rational resampler's launch at the same step
      and next to a device-to-device hipMemcpyAsync of the bytes the warp launch reads plus writes

No gate on the ratios: they are recorded.
usage: python tools/bench_frames_warp.py [out.json]"""
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
from bench_frames_resample import ResampleParams  # noqa: E402
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import resample_len, resample_table, warp_curve, warp_table  # noqa: E402

KW = dict(window_len=N, factor=F, channels=CH, seed=1)
D_LIST = [274877906944, 326886762694, 388736063996, 462287693163, 549755813888, 653773525389, 777472127993, 924575386326,
          1099511627776, 1307547050779, 1554944255987, 1849150772653, 2199023255552]
W_LIST = [32, 39, 46, 54, 64, 77, 91, 108, 128, 153, 182, 216, 256]
NO_TIER = 0xFFFFFFFF


class WarpParams(C.Structure):  # rc::FramesWarpParams (rocoder_amd/csrc/rc_warp.h)
    _fields_ = [("src", C.c_void_p), ("src0", C.c_uint64), ("src_len", C.c_uint64), ("stride", C.c_uint64), ("channels", C.c_uint32),
                ("n", C.c_uint64), ("table", C.c_void_p), ("tier_off", C.c_uint32 * 13), ("anchor", C.c_void_p), ("h_anchor", C.c_void_p),
                ("n_anchors", C.c_uint64), ("dst", C.c_void_p), ("dst_stride", C.c_uint64), ("m0", C.c_uint64), ("m1", C.c_uint64)]


def warps(n_rows, n_hops):
    """{leg: (anchors, n_out, the rational step or None)}"""
    out = {}
    for name, step in (("b_warp_160_147", (160, 147)), ("d_warp_2_1", (2, 1))):
        a, n_out = warp_curve(n_rows, [0.0], [step[0] / step[1]], n_hops=n_hops, **KW)
        out[name] = (a, n_out, step)
    a, n_out = warp_curve(n_rows, [0.0, float(L)], [0.5, 2.0], n_hops=n_hops, **KW)
    out["f_warp_glide"] = (a, n_out, None)
    return out


def device_tables(anchors):
    tiers = sorted({next(t for t in range(13) if d <= D_LIST[t]) for d in np.unique(np.diff(anchors)).tolist()})
    off, parts, at = [NO_TIER] * 13, [], 0
    for t in tiers:
        off[t] = at
        parts.append(np.ascontiguousarray(warp_table(t).T).reshape(-1))
        at += parts[-1].size
    return np.concatenate(parts), off, tiers


def kernel_legs(Lib, n, legs_in):
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

    warp = launcher(Lib, "launch_frames_warp")
    warp.argtypes = [C.POINTER(WarpParams), C.c_void_p]
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
    legs, tiers_used = {}, {}
    for name, (anchors, n_out, step) in legs_in.items():
        flat, off, tiers = device_tables(anchors)
        tiers_used[name] = tiers
        anchors = np.ascontiguousarray(anchors, np.int64)
        d_table, d_anchor, d_out, d_copy = dmalloc(flat.nbytes), dmalloc(anchors.nbytes), dmalloc(n_out * CH * 4), dmalloc((n + n_out) * CH * 4)
        assert hip.hipMemcpy(d_table, flat.ctypes.data, flat.nbytes, 1) == 0 and hip.hipMemcpy(d_anchor, anchors.ctypes.data, anchors.nbytes, 1) == 0
        q = WarpParams(d_rows.value, 0, n, n, CH, n, d_table.value, (C.c_uint32 * 13)(*off), d_anchor.value, anchors.ctypes.data, anchors.size,
                       d_out.value, n_out, 0, n_out)
        legs[f"{name[2:]}_ms"] = timed(lambda: warp(C.byref(q), None))
        half = (n + n_out) * CH * 4 // 2
        legs[f"d2d_{name[2:]}_ms"] = timed(lambda: hip.hipMemcpyAsync(d_copy, C.c_void_p(d_copy.value + half), half, 3, None))
        if step:
            table = resample_table(*step)
            n_rs = resample_len(n, *step)
            d_rt, d_rs = dmalloc(table.nbytes), dmalloc(n_rs * CH * 4)
            assert hip.hipMemcpy(d_rt, table.ctypes.data, table.nbytes, 1) == 0
            r = ResampleParams(d_rows.value, 0, n, n, CH, n, d_rt.value, step[0], step[1], table.shape[1] // 2, d_rs.value, n_rs, 0, n_rs)
            legs[f"resample_{step[0]}_{step[1]}_ms"] = timed(lambda: resample(C.byref(r), None))
            hip.hipDeviceSynchronize()
            hip.hipFree(d_rt), hip.hipFree(d_rs)
        hip.hipDeviceSynchronize()
        for p in (d_table, d_anchor, d_out, d_copy):
            hip.hipFree(p)
    hip.hipFree(d_rows)
    return legs, tiers_used


def call_legs(n_in, rounds):
    """an engine per leg, so that the legs take turns without a setter call inside the timed region"""
    base = rocoder_amd.Engine(**KW)
    n_rows = base.output_len(n_in)
    n_hops = n_rows // base.params.window_out_len * base.params.hops_per_window
    w = warps(n_rows, n_hops)
    engs = {"a_none": base}
    for name, (anchors, n_out, step) in w.items():
        engs[name] = rocoder_amd.Engine(**KW)
        engs[name].set_output_warp(anchors, n_out)
        if step:
            rname = f"{chr(ord(name[0]) + 1)}_step_{step[0]}_{step[1]}"
            engs[rname] = rocoder_amd.Engine(**KW)
            engs[rname].set_output_resample(*step)
    order = sorted(engs)
    n_max = max([n_rows] + [v[1] for v in w.values()] + [resample_len(n_rows, 160, 147), resample_len(n_rows, 2, 1)])
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    yb = rocoder_amd.pinned_empty(n_max * CH * 2, np.uint8)
    times = {name: [] for name in order}
    frames = {}
    for r in range(WARM + rounds):
        for name in order:
            t0 = time.perf_counter()
            got = engs[name].stretch_frames(i16, out=yb, out_fmt="i16")
            dt = (time.perf_counter() - t0) * 1e3
            frames[name] = int(got.shape[0])
            if r >= WARM:
                times[name].append(dt)
    for e in engs.values():
        e.close()
    return dict(frames=n_in, row_frames=n_rows, out_frames=frames, ms=times), w


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r24_frames_warp.json")
    Lib = _lib.lib()
    short, w = call_legs(L, ROUNDS)
    res = {"job": dict(channels=CH, window_len=N, factor=F), "warmups": WARM, "rounds": ROUNDS,
           "kernel_id": Lib.rc_kernel_id().decode(), "short": short}
    summ = short["summary"] = summarise(short["ms"])
    res["kernel_ms"], res["tiers"] = kernel_legs(Lib, short["row_frames"], w)
    ks = res["kernel_summary"] = summarise(res["kernel_ms"])
    a = summ["a_none"]
    res["ratios"] = {name: dict(to_a=summ[name]["median"] / a["median"]) for name in summ if name != "a_none"}
    for name, (_a, _n, step) in w.items():
        r = res["ratios"][name]
        r["launch_to_its_copy"] = ks[f"{name[2:]}_ms"]["median"] / ks[f"d2d_{name[2:]}_ms"]["median"]
        if step:
            r["launch_to_the_rational_launch"] = ks[f"{name[2:]}_ms"]["median"] / ks[f"resample_{step[0]}_{step[1]}_ms"]["median"]
    res["a_spread"] = a["max"] - a["min"]
    print("ratios:", json.dumps(res["ratios"]), flush=True)
    print("kernel medians (ms):", json.dumps({k: round(v["median"], 4) for k, v in ks.items()}), flush=True)
    print("end to end medians (ms):", json.dumps({k: round(v["median"], 3) for k, v in summ.items()}), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

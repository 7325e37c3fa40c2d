"""What a time map costs (rc_engine_set_time_map), by the protocol of tools/bench_frames_pcm.py: 3 warm-ups, then
10 rounds in which the legs take turns in one process; medians and the min-max spread per leg; bench.py's box calibration
(rc_calib_valu) alongside.

  a  the C2-shaped device-form job (stereo, N = 16384, f = 8, L = 2 646 000), event time of the launches on the stream:
     no map / the uniform map of the same hops (one point, f = 8: hop k at k * sample_step_len) / a ramp from 8 to 64
  b  the C5-shaped job (8 channels, N = 65536, f = 32, L = 5 292 000), the same three
  c  one gather launch of (a) - a chunk's rows, as the engine sizes it - through the test hook, by HIP events, next to a
     device-to-device hipMemcpyAsync of the bytes it writes
  d  rc_engine_stretch_frames_pcm to i16 with and without the uniform map, end to end (PCIe included, page-locked memory)

The uniform-map job computes the no-map job's hops (its output is checked to be the same bits), so its extra time is the
gather's. A ramp has more hops: its time is recorded per hop as well. Nothing here is a gate; the one condition - the
no-map job against the parent commit's library - is tools/ab_libs.py's.
usage: python tools/bench_time_map.py [out.json] [--no-c5]"""
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
from bench_frames_pcm import ROUNDS, WARM, summarise  # noqa: E402
from rocoder_amd import _lib  # noqa: E402

JOBS = {"a_c2": dict(channels=2, window_len=16384, factor=8.0, length=2_646_000),
        "b_c5": dict(channels=8, window_len=65536, factor=32.0, length=5_292_000)}


def device_legs(job):
    import torch

    ch, N, f, L = job["channels"], job["window_len"], job["factor"], job["length"]
    kw = dict(window_len=N, factor=f, channels=ch, seed=1)
    x = torch.rand((ch, L), device="cuda") - 0.5
    uniform = rocoder_amd.time_map_curve(L, [0.0], [f], **kw)
    ramp = rocoder_amd.time_map_curve(L, [0.0, float(L)], [8.0, 64.0], **kw)
    engines = {"no_map": rocoder_amd.Engine(**kw), "uniform_map": rocoder_amd.Engine(**kw), "ramp_8_to_64": rocoder_amd.Engine(**kw)}
    engines["uniform_map"].set_time_map(uniform)
    engines["ramp_8_to_64"].set_time_map(ramp)
    outs = {k: torch.empty((ch, e.output_len(L)), dtype=torch.float32, device="cuda") for k, e in engines.items()}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()  # (not the null stream: the engine's launches go onto this one, between the two events)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in engines}
    with torch.cuda.stream(stream):
        for r in range(WARM + ROUNDS):
            for k, e in engines.items():
                ev0.record(stream)
                e.stretch_tensor(x, out=outs[k])
                ev1.record(stream)
                ev1.synchronize()
                if r >= WARM:
                    times[k].append(ev0.elapsed_time(ev1))
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["no_map"], outs["uniform_map"]))
    hops = {"no_map": int(uniform.size), "uniform_map": int(uniform.size), "ramp_8_to_64": int(ramp.size)}
    for e in engines.values():
        e.close()
    return dict(job=job, hops=hops, uniform_map_equals_no_map_bit_for_bit=same, ms=times)


def gather_leg(job):
    """one chunk of job's gather, as run_map_hops sizes it: the rows of all channels within 256 MiB, one hop in front"""
    import torch

    ch, N, f, L = job["channels"], job["window_len"], job["factor"], job["length"]
    hpw = int(rocoder_amd.derive_params(window_len=N, factor=f).hops_per_window)
    pos = rocoder_amd.time_map_curve(L, [0.0], [f], window_len=N, factor=f)
    rows = min(int(pos.size), (((256 << 20) // (ch * N * 4) - 1) // hpw * hpw) + 1)
    with _lib.hooks_library() as H:
        H.rc_test_time_map_gather.restype = C.c_int
        H.rc_test_time_map_gather.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_uint64]
        hip = H
        for fn, args in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                         ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
                         ("hipMemcpyAsync", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]), ("hipDeviceSynchronize", [])):
            getattr(hip, fn).argtypes = args
            getattr(hip, fn).restype = C.c_int
        x = torch.rand((ch, L), device="cuda") - 0.5
        d_pos = torch.from_numpy(pos).cuda()
        v = torch.empty(ch * rows * N, dtype=torch.float32, device="cuda")
        w = torch.empty_like(v)
        torch.cuda.synchronize()
        ev0, ev1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
        calls = {"gather_ms": lambda: H.rc_test_time_map_gather(x.data_ptr(), L, L, d_pos.data_ptr(), 0, rows, ch, N, v.data_ptr(), rows * N),
                 "d2d_ms": lambda: hip.hipMemcpyAsync(w.data_ptr(), v.data_ptr(), v.numel() * 4, 3, None)}
        times = {k: [] for k in calls}
        for r in range(WARM + ROUNDS):
            for k, fn in calls.items():
                assert hip.hipEventRecord(ev0, None) == 0
                assert fn() == 0
                assert hip.hipEventRecord(ev1, None) == 0 and hip.hipEventSynchronize(ev1) == 0
                ms = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                if r >= WARM:
                    times[k].append(ms.value)
        hip.hipDeviceSynchronize()
    return dict(hops=rows, channels=ch, bytes_written=int(v.numel() * 4), ms=times)


def frames_legs(job):
    ch, N, f, L = job["channels"], job["window_len"], job["factor"], job["length"]
    kw = dict(window_len=N, factor=f, channels=ch, seed=1)
    plain, mapped = rocoder_amd.Engine(**kw), rocoder_amd.Engine(**kw)
    mapped.set_time_map(rocoder_amd.time_map_curve(L, [0.0], [f], **kw))
    n_out = plain.output_len(L)
    assert mapped.output_len(L) == n_out
    i16 = rocoder_amd.pinned_empty((L, ch), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (L, ch), dtype=np.int64)
    ya, yb = (rocoder_amd.pinned_empty(n_out * ch * 2, np.uint8) for _ in range(2))
    calls = {"pcm_no_map": lambda: plain.stretch_frames(i16, out=ya, out_fmt="i16"),
             "pcm_uniform_map": lambda: mapped.stretch_frames(i16, out=yb, out_fmt="i16")}
    times = {k: [] for k in calls}
    for r in range(WARM + ROUNDS):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if r >= WARM:
                times[k].append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(ya, yb))
    plain.close()
    mapped.close()
    return dict(frames=L, out_frames=n_out, same_bytes=same, ms=times)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r21_time_map.json")
    L = _lib.lib()
    res = {"warmups": WARM, "rounds": ROUNDS, "kernel_id": L.rc_kernel_id().decode()}
    ms_l, ns_i = C.c_float(0), C.c_float(0)
    if L.rc_calib_valu(0, None, 48, C.byref(ms_l), C.byref(ns_i)) == 0:
        res["calib_valu"] = {"ms_per_launch": float(ms_l.value), "ns_per_inst": float(ns_i.value)}
    for name, job in JOBS.items():
        if name == "b_c5" and "--no-c5" in sys.argv:
            continue
        print(name, job, flush=True)
        leg = res[name] = device_legs(job)
        s = leg["summary"] = summarise(leg["ms"])
        leg["uniform_to_no_map"] = s["uniform_map"]["median"] / s["no_map"]["median"]
        leg["us_per_hop_and_channel"] = {k: 1e3 * s[k]["median"] / (leg["hops"][k] * job["channels"]) for k in s}
        json.dump(res, open(out_path, "w"), indent=1)
    print("c_gather", flush=True)
    g = res["c_gather"] = gather_leg(JOBS["a_c2"])
    s = g["summary"] = summarise(g["ms"])
    g["gather_to_the_copy"] = s["gather_ms"]["median"] / s["d2d_ms"]["median"]
    g["gather_GBps_read_plus_written"] = 2 * g["bytes_written"] / s["gather_ms"]["median"] / 1e6
    print("d_frames", flush=True)
    d = res["d_frames_pcm"] = frames_legs(JOBS["a_c2"])
    s = d["summary"] = summarise(d["ms"])
    d["uniform_to_no_map"] = s["pcm_uniform_map"]["median"] / s["pcm_no_map"]["median"]
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k in ("kernel_id", "calib_valu")}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

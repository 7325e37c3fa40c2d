"""rc_engine_set_output_dither against the undithered rc_engine_stretch_frames_pcm, end to end (PCIe included), on the job
and by the protocol of tools/bench_frames_pcm.py: stereo, N = 16384, f = 8, L = 2 646 000 i16 frames in, page-locked memory on
both sides; 3 warm-ups, then 10 rounds in which the legs take turns in one process; medians and the min-max spread per leg.

  a  i16 out, no dither set                                    (the merged code: the yardstick)
  b  i16 out, TPDF
  c  i16 out, TPDF_HP
  d  the same three on u8
  e  HIP-event time of one pack launch per mode and format on the job's buffers, next to the undithered launch and a
     device-to-device hipMemcpyAsync of the bytes they read

Gate: median(b) and median(c) each <= median(a) + (max(a) - min(a)): the call is bound by PCIe, and the dither
has to stay hidden under it. The u8 legs and the per-launch figures of (e) are recorded, not gated.
usage: python tools/bench_frames_dither.py [out.json]"""
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
from bench_frames import launcher  # noqa: E402
from bench_frames_pcm import CH, F, L, N, ROUNDS, WARM, PackPcmParams, summarise  # noqa: E402
from rocoder_amd import _lib  # noqa: E402

SEED = 1
MODES = ["none", "tpdf", "tpdf-hp"]


class DitherParams(C.Structure):  # rc::FramesDitherParams (rocoder_amd/csrc/rc_frames.h)
    _fields_ = [("mode", C.c_uint32), ("channel0", C.c_uint32), ("t0", C.c_uint64), ("keys", C.c_void_p)]


class PackPcmDitherParams(C.Structure):  # rc::FramesPackPcmDitherParams
    _fields_ = [("pack", PackPcmParams), ("dither", DitherParams)]


def kernel_legs(Lib, n_out):
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

    pack_pcm = launcher(Lib, "launch_frames_pack_pcm")
    pack_pcm.argtypes = [C.c_uint32, C.POINTER(PackPcmParams), C.c_void_p]
    pack_dither = launcher(Lib, "launch_frames_pack_pcm_dither")
    pack_dither.argtypes = [C.c_uint32, C.POINTER(PackPcmDitherParams), C.c_void_p]
    d_out, d_frames, d_clip, d_keys = dmalloc(n_out * CH * 4), dmalloc(n_out * CH * 4 + 16), dmalloc(8), dmalloc(8 * CH)
    keys = (C.c_uint64 * CH)(*[Lib.rc_phase_key(SEED, c, 0xFFFFFFFFFF) for c in range(CH)])
    assert hip.hipMemcpy(d_keys, keys, 8 * CH, 1) == 0
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

    legs = {}
    for name in ("i16", "u8", "i24"):
        code = _lib.PCM_FORMATS[name]
        q = PackPcmParams(d_out.value, n_out, d_frames.value, 0, CH, n_out, d_clip.value)
        legs[f"pack_pcm_{name}_none_ms"] = timed(lambda: pack_pcm(code, C.byref(q), None))
        for mode in (1, 2):
            qd = PackPcmDitherParams(q, DitherParams(mode, 0, 0, d_keys.value))
            legs[f"pack_pcm_{name}_{MODES[mode]}_ms"] = timed(lambda: pack_dither(code, C.byref(qd), None))
    legs["d2d_of_the_bytes_read_ms"] = timed(lambda: hip.hipMemcpyAsync(d_frames, d_out, n_out * CH * 4, 3, None))
    hip.hipDeviceSynchronize()
    for p in (d_out, d_frames, d_clip, d_keys):
        hip.hipFree(p)
    return legs


def call_legs(n_in, rounds):
    """an engine per mode, so that the legs take turns without a setter call inside the timed region"""
    engs = {}
    for mode in MODES:
        engs[mode] = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
        engs[mode].set_output_dither(mode, SEED)
    n_out = engs["none"].output_len(n_in)
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    yb = rocoder_amd.pinned_empty(n_out * CH * 2, np.uint8)
    legs = []
    for letter, fmt in (("abc", "i16"), ("d d d", "u8")):
        for k, mode in enumerate(MODES):
            tag = letter[k] if fmt == "i16" else "d"
            legs.append((f"{tag}_{fmt}_{mode}", (lambda m, f: lambda: engs[m].stretch_frames(i16, out=yb[:n_out * CH * (2 if f == 'i16' else 1)], out_fmt=f))(mode, fmt)))
    times = {name: [] for name, _ in legs}
    for r in range(WARM + rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[name].append(dt)
    # what was timed is what the definition says: the codes differ from the undithered ones by at most one step, and do differ
    plain = engs["none"].stretch_frames(i16, out_fmt="i16").astype(np.int32)
    differ = {}
    for mode in MODES[1:]:
        d = engs[mode].stretch_frames(i16, out_fmt="i16").astype(np.int32) - plain
        differ[mode] = dict(max_abs_code_difference=int(np.abs(d).max()), share_of_codes_changed=float((d != 0).mean()))
    for e in engs.values():
        e.close()
    return dict(frames=n_in, out_frames=n_out, ms=times, dithered_against_undithered_i16=differ)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_frames_dither.json")
    Lib = _lib.lib()
    short = call_legs(L, ROUNDS)
    res = {"job": dict(channels=CH, window_len=N, factor=F), "warmups": WARM, "rounds": ROUNDS,
           "kernel_id": Lib.rc_kernel_id().decode(), "short": short}
    summ = short["summary"] = summarise(short["ms"])
    res["kernel_ms"] = kernel_legs(Lib, short["out_frames"])
    res["kernel_summary"] = summarise(res["kernel_ms"])
    a, b, c = (summ[k] for k in ("a_i16_none", "b_i16_tpdf", "c_i16_tpdf-hp"))
    spread = a["max"] - a["min"]
    res["gate"] = dict(a_median=a["median"], a_spread=spread, b_median=b["median"], c_median=c["median"],
                       passed=b["median"] <= a["median"] + spread and c["median"] <= a["median"] + spread)
    print("dithered against undithered i16:", short["dithered_against_undithered_i16"], "  gate:", res["gate"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    return 0 if res["gate"]["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())

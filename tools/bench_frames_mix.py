"""The mix bus (rc_engine_mix_frames / rc_engine_bus_frames) on the job and by the protocol of
tools/bench_frames_pcm.py: stereo, N = 16384, f = 8, L = 2 646 000 i16 frames in, page-locked memory on the host side; 3
warm-ups, then 10 rounds in which the legs take turns in one process; medians and the min-max spread per leg.

  1  HIP-event time of one mix launch on the job's rows into a bus of the same length (two keys, no send, offset 1), next to
     a device-to-device hipMemcpyAsync of the same bytes. The launch moves 3 words per sample (row in, bus in, bus out), the
     copy 2 (in, out): about 1.5 x the copy's time is what a memory-bound launch costs.
  2  rc_engine_mix_frames end to end next to rc_engine_stretch_frames (f32 out) on the same job: the mix saves the download.
  3  three layers (factors 8, 8 and 4, offsets and fades of their own) through the bus into i16 with a target peak, next to
     three rc_engine_stretch_frames calls plus numpy's sum under the same envelopes, peak and quantiser.

Nothing is gated: these are the first numbers of this path. usage: python tools/bench_frames_mix.py [out.json]"""
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
from rocoder_amd.stretcher import Bus, mix_envelope  # noqa: E402


class MixParams(C.Structure):  # rc::FramesMixParams (rocoder_amd/csrc/rc_frames.h)
    _fields_ = [("rows", C.c_void_p), ("stride", C.c_uint64), ("channels", C.c_uint32), ("t0", C.c_uint64), ("t1", C.c_uint64),
                ("bus", C.c_void_p), ("bus_stride", C.c_uint64), ("bus_channels", C.c_uint32), ("bus_frames", C.c_uint64),
                ("offset", C.c_int64), ("key_frame", C.c_void_p), ("key_amp", C.c_void_p), ("n_keys", C.c_uint32), ("send", C.c_void_p)]


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

    mix = launcher(Lib, "launch_frames_mix")
    mix.argtypes = [C.POINTER(MixParams), C.c_void_p]
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

    stride = (n + 4 + 3) // 4 * 4
    d_rows, d_bus, d_copy, d_keys = dmalloc(n * CH * 4), dmalloc(stride * CH * 4), dmalloc(2 * n * CH * 4), dmalloc(64)
    kf, ka = np.array([0, n], np.uint64), np.array([0.0, 1.0], np.float32)
    assert hip.hipMemcpy(d_keys, kf.ctypes.data, 16, 1) == 0 and hip.hipMemcpy(C.c_void_p(d_keys.value + 16), ka.ctypes.data, 8, 1) == 0
    legs = {}
    for name, keys in (("mix_2keys_ms", 2), ("mix_nokeys_ms", 0)):
        q = MixParams(d_rows.value, n, CH, 0, n, d_bus.value, stride, CH, n + 1, 1, d_keys.value, d_keys.value + 16, keys, None)
        legs[name] = timed(lambda: mix(C.byref(q), None))
    half = n * CH * 4  # the same samples as one device-to-device copy moves them (a copy reads and writes each byte once)
    legs["d2d_ms"] = timed(lambda: hip.hipMemcpyAsync(d_copy, C.c_void_p(d_copy.value + half), half, 3, None))
    hip.hipDeviceSynchronize()
    for p in (d_rows, d_bus, d_copy, d_keys):
        hip.hipFree(p)
    return legs


def quantise_i16(x):
    return np.clip(np.rint(x * np.float32(32767.0)), -32768, 32767).astype("<i2")


def call_legs(n_in):
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    e8 = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
    e8b = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=2)
    e4 = rocoder_amd.Engine(window_len=N, factor=F / 2, channels=CH, seed=3)
    n8, n4 = e8.output_len(n_in), e4.output_len(n_in)
    layers = [(e8, 0, [(0, 0.0), (44100, 1.0), (n8 - 44100, 1.0), (n8, 0.0)]), (e8b, 22050, [(0, 0.7)]),
              (e4, 44100, [(0, 0.0), (88200, 0.5)])]
    n_bus = max(o + e.output_len(n_in) for e, o, _ in layers)
    y8 = rocoder_amd.pinned_empty((n8, CH), np.float32)
    y4 = rocoder_amd.pinned_empty((n4, CH), np.float32)
    out = rocoder_amd.pinned_empty(n_bus * CH * 2, np.uint8)
    times = {k: [] for k in ("stretch_f32", "mix_frames", "three_layers_bus_i16", "three_stretch_numpy_i16", "bus_frames_i16_alone")}
    with Bus(CH, n8) as one, Bus(CH, n_bus) as bus:
        for r in range(WARM + ROUNDS):
            t = {}
            t0 = time.perf_counter()
            e8.stretch_frames(i16, out=y8)
            t["stretch_f32"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            e8.mix_frames(i16, one, keys=layers[0][2])
            t["mix_frames"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            bus.clear()
            for e, off, keys in layers:
                e.mix_frames(i16, bus, offset=off, keys=keys)
            t1 = time.perf_counter()
            e8.bus_frames(bus, "i16", target_peak=0.9, out=out)
            t["three_layers_bus_i16"] = time.perf_counter() - t0
            t["bus_frames_i16_alone"] = time.perf_counter() - t1
            t0 = time.perf_counter()
            acc = np.zeros((n_bus, CH), np.float32)
            for e, off, keys in layers:
                y = e.stretch_frames(i16, out=y8 if e is not e4 else y4)
                acc[off:off + y.shape[0]] += y * mix_envelope(keys, 0, y.shape[0])[:, None]
            peak = np.abs(acc).max()
            host = quantise_i16(acc * (np.float32(0.9) / peak))
            t["three_stretch_numpy_i16"] = time.perf_counter() - t0
            if r >= WARM:
                for k, v in t.items():
                    times[k].append(v * 1e3)
        del host
    for e in (e8, e8b, e4):
        e.close()
    return dict(frames=n_in, out_frames=n8, bus_frames=n_bus, ms=times)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r25_frames_mix.json")
    Lib = _lib.lib()
    res = {"job": dict(channels=CH, window_len=N, factor=F), "warmups": WARM, "rounds": ROUNDS, "kernel_id": Lib.rc_kernel_id().decode()}
    from boxclock import ClockSampler
    with ClockSampler(0) as clk:
        calls = res["calls"] = call_legs(L)
        cs = calls["summary"] = summarise(calls["ms"])
        res["kernel_ms"] = kernel_legs(Lib, calls["out_frames"])
    ks = res["kernel_summary"] = summarise(res["kernel_ms"])
    res["box"] = dict(device="MI355X (gfx950)", median_sclk_mhz=clk.median_mhz())
    res["ratios"] = dict(mix_launch_to_the_copy=ks["mix_2keys_ms"]["median"] / ks["d2d_ms"]["median"],
                         mix_launch_no_keys_to_the_copy=ks["mix_nokeys_ms"]["median"] / ks["d2d_ms"]["median"],
                         mix_frames_to_stretch_f32=cs["mix_frames"]["median"] / cs["stretch_f32"]["median"],
                         bus_to_numpy=cs["three_layers_bus_i16"]["median"] / cs["three_stretch_numpy_i16"]["median"])
    print("ratios:", res["ratios"], "box:", res["box"], flush=True)
    print("medians (ms):", {k: round(v["median"], 3) for k, v in {**cs, **ks}.items()}, flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The channel map and the channel peaks end to end (PCIe included), on an i16 stereo block of 2 646 000 frames in
page-locked memory, N = 1024, f = 2. 3 warm-ups, then 10 rounds in which the legs take turns in one process; median
[min - max] per leg.

  a0  stretch_frames(out_fmt="i16"), no map                       (the parent commit's call: the unmapped launches)
  a1  the same call on the same job with the swap map [1, 0]      (the mapped unpack kernel)
  b   permute the interleaved block in numpy (a[:, [1, 0]]), then a0's call   (what a caller has without the entry)
  c0  frames_channel_peaks                                        (chunked uploads, a chunk's kernel under the next upload)
  c1  one hipMemcpy of the same bytes from the same page-locked block to the device   (the floor: nothing is computed)
  c2  decode, abs and max(axis=0) in numpy on the host

Recorded: a1 / a0, b / a1, c0 / c1 and c0 / c2 of the medians, a1 - a0 beside the spread (max - min) of a0's ten calls,
and whether a1's bytes equal b's and c0's peaks equal c2's bit for bit.
usage: python tools/bench_frames_map.py [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rocoder_amd  # noqa: E402
from rocoder_amd import _lib  # noqa: E402

CH, L = 2, 2_646_000
WARM, ROUNDS = 3, 10
SWAP = [1, 0]


class Floor:
    """leg c1: hipMalloc once, then one blocking hipMemcpy per call"""

    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.d = C.c_void_p()
        self.nbytes = nbytes
        assert self.hip.hipMalloc(C.byref(self.d), C.c_size_t(nbytes)) == 0

    def __call__(self, host):
        assert self.hip.hipMemcpy(self.d, C.c_void_p(host.ctypes.data), C.c_size_t(self.nbytes), 1) == 0  # hipMemcpyHostToDevice

    def close(self):
        self.hip.hipFree(self.d)


def host_peaks(i16):
    """leg c2: the reader's decode, abs, a maximum per channel"""
    x = i16.astype(np.float32)
    x /= np.float32(32767)
    np.abs(x, out=x)
    return x.max(axis=0)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16_frames_map.json")
    eng = rocoder_amd.Engine(window_len=1024, factor=2.0, channels=CH, seed=1)
    i16 = rocoder_amd.pinned_empty((L, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (L, CH), dtype=np.int64)
    floor = Floor(i16.nbytes)

    def unmapped():
        eng.set_channel_map(None)
        return eng.stretch_frames(i16, out_fmt="i16")

    def mapped():
        eng.set_channel_map(SWAP)
        return eng.stretch_frames(i16, out_fmt="i16")

    def permuted_on_the_host():
        eng.set_channel_map(None)
        return eng.stretch_frames(np.ascontiguousarray(i16[:, SWAP]), out_fmt="i16")

    legs = [("a0_no_map", unmapped), ("a1_swap_map", mapped), ("b_numpy_permute_then_no_map", permuted_on_the_host),
            ("c0_frames_channel_peaks", lambda: eng.frames_channel_peaks(i16)), ("c1_one_hipMemcpy", lambda: floor(i16)),
            ("c2_numpy_on_the_host", lambda: host_peaks(i16))]
    times = {name: [] for name, _ in legs}
    for r in range(WARM + ROUNDS):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[name].append(dt)
    bytes_equal = mapped().tobytes() == permuted_on_the_host().tobytes()
    peaks_equal = bool(np.array_equal(eng.frames_channel_peaks(i16).view(np.uint32), host_peaks(i16).view(np.uint32)))
    summ = {}
    for k, v in times.items():
        summ[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:30s} median {summ[k]['median']:9.3f} ms   [{summ[k]['min']:9.3f} - {summ[k]['max']:9.3f}]", flush=True)
    m = {k: v["median"] for k, v in summ.items()}
    ratios = dict(a1_over_a0=m["a1_swap_map"] / m["a0_no_map"], b_over_a1=m["b_numpy_permute_then_no_map"] / m["a1_swap_map"],
                  a1_minus_a0_ms=m["a1_swap_map"] - m["a0_no_map"], spread_of_a0_ms=summ["a0_no_map"]["max"] - summ["a0_no_map"]["min"],
                  c0_over_c1=m["c0_frames_channel_peaks"] / m["c1_one_hipMemcpy"], c0_over_c2=m["c0_frames_channel_peaks"] / m["c2_numpy_on_the_host"])
    res = {"job": dict(channels=CH, format="i16", frames=L, bytes=int(i16.nbytes), window_len=1024, factor=2.0, out_fmt="i16", map=SWAP),
           "warmups": WARM, "rounds": ROUNDS, "kernel_id": _lib.lib().rc_kernel_id().decode(), "ms": times, "summary": summ,
           "ratios": ratios, "mapped_bytes_equal_the_host_permuted_route": bytes_equal, "peaks_equal_the_host_route": peaks_equal}
    print("ratios:", ratios, " equal:", bytes_equal, peaks_equal, flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    floor.close()
    eng.close()
    return 0 if bytes_equal and peaks_equal else 1


if __name__ == "__main__":
    sys.exit(main())

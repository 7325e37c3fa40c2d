"""rc_engine_stretch_frames_loud against rc_engine_stretch_frames_norm and rc_engine_stretch_frames_pcm, end to end (PCIe
included), on the job and by the protocol of tools/bench_frames_pcm.py: stereo, N = 16384, f = 8, L = 2 646 000 i16 frames in,
i16 out, page-locked memory on both sides; 3 warm-ups, then 10 rounds in which the legs take turns in one process; medians and
the min-max spread per leg.

  a  rc_engine_stretch_frames_pcm                                (the merged code: the yardstick)
  b  rc_engine_stretch_frames_norm, target 0.9
  c  rc_engine_stretch_frames_loud, -16 LUFS under a ceiling of 0.9, at 44.1 kHz
  d  HIP-event time of each measuring launch on the job's rows (through the test hooks: the launch and its synchronise),
     next to a device-to-device hipMemcpyAsync of the bytes it reads (a copy reads and writes: half as many bytes copied)
  e  what is left of (c) - (b) once the two launches are taken off and the peak launches of (b), unmeasured here, are
     ignored: the wait of the host round trip between the two phases, the readback and the gate

The energy words of the last launch are also held against the f64 definition: the largest relative error goes into the file.

Gate (read next to the parent commit's tools/bench_frames_pcm.py i16 leg of the same visit): median(a) inside that leg's
min - max - the new entry costs the old ones nothing. Everything else is recorded as ratios, not gated.
usage: python tools/bench_frames_loud.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rocoder_amd  # noqa: E402
from bench_frames_pcm import CH, F, L, N, ROUNDS, WARM, summarise  # noqa: E402
from rocoder_amd import _lib  # noqa: E402

RATE, TARGET, CEILING = 44100, -16.0, 0.9
LEGS = ["a_pcm", "b_norm", "c_loud"]


def kernel_legs(rows):
    """the two launchers on rows [CH, n] already on the device, by HIP events on the null stream"""
    import torch

    import loudnessutil as U

    hip = _lib.lib()
    for f, args in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                    ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
                    ("hipMemcpyAsync", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]), ("hipDeviceSynchronize", [])):
        getattr(hip, f).argtypes = args
        getattr(hip, f).restype = C.c_int
    energy = U._hook("rc_test_frames_kweight_energy", [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                       C.c_void_p, C.c_uint64])
    peak = U._hook("rc_test_frames_true_peak", [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p])
    ch, n = rows.shape
    sub = U.sub_frames(RATE)
    nb = n // sub
    d_rows = torch.from_numpy(rows).to("cuda")
    d_e = torch.zeros(ch * nb, dtype=torch.float32, device="cuda")
    d_tab = torch.from_numpy(U.table_1_4().copy()).to("cuda")
    d_words = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_copy = torch.zeros(ch * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
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

    legs = {"energy_ms": timed(lambda: energy(d_rows.data_ptr(), n, n, ch, RATE, sub, nb, d_e.data_ptr(), nb)),
            "true_peak_ms": timed(lambda: peak(d_rows.data_ptr(), n, n, ch, d_tab.data_ptr(), d_words.data_ptr()))}
    half = ch * n * 2  # bytes: half the rows copied onto the other half moves as many bytes as a launch reads
    legs["d2d_ms"] = timed(lambda: hip.hipMemcpyAsync(d_copy.data_ptr(), d_copy.data_ptr() + half, half, 3, None))
    hip.hipDeviceSynchronize()
    # the words of the last energy launch against the f64 definition (tests/loudnessutil.py): the largest errors on this job
    rel, quiet = U.energy_errors(d_e.cpu().numpy().reshape(ch, nb), U.sub_energies(rows, RATE), sub)
    return legs, dict(span=U.loud_span(ch, nb), sub_blocks=nb, largest_relative_energy_error=rel, largest_error_below_the_gate=quiet)


def call_legs(n_in, rounds):
    eng = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1, sample_rate=RATE)
    n_out = eng.output_len(n_in)
    i16 = rocoder_amd.pinned_empty((n_in, CH), np.int16)
    i16[:] = np.random.default_rng(0).integers(-16000, 16000, (n_in, CH), dtype=np.int64)
    yb = rocoder_amd.pinned_empty(n_out * CH * 2, np.uint8)
    calls = {"a_pcm": lambda: eng.stretch_frames(i16, out=yb, out_fmt="i16"),
             "b_norm": lambda: eng.stretch_frames(i16, out=yb, out_fmt="i16", normalize=0.9),
             "c_loud": lambda: eng.stretch_frames_loud(i16, TARGET, CEILING, out=yb, out_fmt="i16", sample_rate=RATE)}
    times = {name: [] for name in LEGS}
    for r in range(WARM + rounds):
        for name in LEGS:
            t0 = time.perf_counter()
            calls[name]()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[name].append(dt)
    found = dict(lufs=float(eng.last_lufs), true_peak=float(eng.last_true_peak), gain=float(eng.last_gain), clipped=eng.last_clipped)
    rows = np.ascontiguousarray(eng.stretch_frames(i16).T)
    eng.close()
    return dict(frames=n_in, out_frames=n_out, ms=times, found=found), rows


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r20_frames_loud.json")
    short, rows = call_legs(L, ROUNDS)
    res = {"job": dict(channels=CH, window_len=N, factor=F, rate=RATE, target_lufs=TARGET, max_true_peak=CEILING), "warmups": WARM,
           "rounds": ROUNDS, "kernel_id": _lib.lib().rc_kernel_id().decode(), "short": short}
    summ = short["summary"] = summarise(short["ms"])
    with _lib.hooks_library():
        res["kernel_ms"], res["geometry"] = kernel_legs(rows)
    ks = res["kernel_summary"] = summarise(res["kernel_ms"])
    a, b, c = (summ[k]["median"] for k in LEGS)
    res["ratios"] = dict(loud_to_pcm=c / a, loud_to_norm=c / b, norm_to_pcm=b / a,
                         energy_to_the_copy=ks["energy_ms"]["median"] / ks["d2d_ms"]["median"],
                         true_peak_to_the_copy=ks["true_peak_ms"]["median"] / ks["d2d_ms"]["median"])
    res["round_trip_ms"] = (c - b) - ks["energy_ms"]["median"] - ks["true_peak_ms"]["median"]
    res["a_spread"] = summ["a_pcm"]["max"] - summ["a_pcm"]["min"]
    print("ratios:", res["ratios"], "round trip:", res["round_trip_ms"], "found:", short["found"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""rc_engine_stretch_frames against the host form, end to end (PCIe included), on the C2-shaped job the other tools use
(stereo, N = 16384, f = 8, L = 2 646 000 frames). 3 warm-ups, then 10 rounds in which the legs take turns (one process,
interleaved, so that clock and link drift hit all of them alike); medians and the min-max spread per leg.

  1  rc_engine_stretch_host on page-locked planar f32 rows                       (the yardstick)
  2  leg 1 + the conversion and the interleave the CLI does on the host today: a C transcription of read_wav's loop
     (i16 -> f32, de-interleaved by push_back) and of WavStreamWriter::append's (4096 frames at a time), compiled here
  3  rc_engine_stretch_frames, f32 frames, page-locked on both sides
  4  the same with i16 frames
  5  HIP-event time of the unpack launch (f32, i16) and of the pack launch alone on the job's buffers, next to a
     device-to-device hipMemcpyAsync of the bytes each one writes

Acceptance: median(3) <= median(1) + (max(1) - min(1)). Everything else is recorded, not gated.
usage: python tools/bench_frames.py [out.json]"""
import ctypes as C
import json
import os
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

CH, N, F, L = 2, 16384, 8.0, 2_646_000
WARM, ROUNDS = 3, 10

HOST_LOOPS = r"""
#include <cstdint>
#include <cstring>
#include <vector>
// host/rocoder_cli.cpp read_wav: i16 -> float, de-interleaved with a push_back per sample
extern "C" void decode_i16(const unsigned char *raw, size_t n, unsigned ch, float *const *rows) {
    std::vector<std::vector<float>> data(ch);
    for (auto &c : data) c.reserve(n / ch + 1);
    for (size_t i = 0; i < n; ++i) {
        const unsigned char *p = raw + i * 2;
        data[i % ch].push_back((float)(int16_t)(uint16_t)(p[0] | (p[1] << 8)) / 32767.0f);
    }
    for (unsigned c = 0; c < ch; ++c) memcpy(rows[c], data[c].data(), data[c].size() * sizeof(float));  // (into the pinned rows)
}
// WavStreamWriter::append: 4096 frames at a time into a row buffer, the row to the sink (here memory, not a file)
extern "C" void interleave(const float *const *chans, size_t n, unsigned ch, float *sink) {
    std::vector<float> row((size_t)ch * 4096);
    for (size_t i0 = 0; i0 < n; i0 += 4096) {
        const size_t k = n - i0 < 4096 ? n - i0 : 4096;
        for (size_t i = 0; i < k; ++i)
            for (unsigned c = 0; c < ch; ++c) row[i * ch + c] = chans[c][i0 + i];
        memcpy(sink + i0 * ch, row.data(), k * ch * sizeof(float));
    }
}
"""


def build_host_loops(tmp):
    src, so = os.path.join(tmp, "host_loops.cpp"), os.path.join(tmp, "host_loops.so")
    open(src, "w").write(HOST_LOOPS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src], check=True)
    return C.CDLL(so)


class UnpackParams(C.Structure):  # rc::FramesUnpackParams (rocoder_amd/csrc/rc_frames.h)
    _fields_ = [("raw", C.c_void_p), ("raw_dwords", C.c_uint64), ("phase", C.c_uint32), ("channels", C.c_uint32),
                ("frame0", C.c_uint64), ("n_frames", C.c_uint64), ("planar", C.c_void_p), ("stride", C.c_uint64)]


class PackParams(C.Structure):  # rc::FramesPackParams
    _fields_ = [("planar", C.c_void_p), ("stride", C.c_uint64), ("frames", C.c_void_p), ("n_frames", C.c_uint64),
                ("channels", C.c_uint32)]


def launcher(Lib, name):
    """The C++ launchers are no part of the C-ABI: found by their mangled names in the library's dynamic symbols."""
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    sym = [ln.split()[-1] for ln in out.splitlines() if f"{len(name)}{name}E" in ln]  # (the whole name: not launch_frames_pack_pcm)
    assert len(sym) == 1, (name, sym)
    fn = getattr(Lib, sym[0])
    fn.restype = C.c_int
    return fn


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

    unpack, pack = launcher(Lib, "launch_frames_unpack"), launcher(Lib, "launch_frames_pack")
    unpack.argtypes = [C.c_uint32, C.POINTER(UnpackParams), C.c_void_p]
    pack.argtypes = [C.POINTER(PackParams), C.c_void_p]
    raw_bytes = (L * CH * 4 + 15) // 16 * 16 + 16
    d_raw, d_in = dmalloc(raw_bytes), dmalloc(L * CH * 4)
    d_out, d_frames = dmalloc(n_out * CH * 4), dmalloc(n_out * CH * 4)
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

    up = UnpackParams(d_raw.value, raw_bytes // 4, 0, CH, 0, L, d_in.value, L)
    pk = PackParams(d_out.value, n_out, d_frames.value, n_out, CH)
    D2D = 3  # hipMemcpyDeviceToDevice
    legs = {
        "unpack_f32_ms": timed(lambda: unpack(_lib.RC_PCM_F32, C.byref(up), None)),
        "unpack_i16_ms": timed(lambda: unpack(_lib.RC_PCM_I16, C.byref(up), None)),
        "d2d_input_bytes_ms": timed(lambda: hip.hipMemcpyAsync(d_in, d_raw, L * CH * 4, D2D, None)),
        "pack_ms": timed(lambda: pack(C.byref(pk), None)),
        "d2d_output_bytes_ms": timed(lambda: hip.hipMemcpyAsync(d_frames, d_out, n_out * CH * 4, D2D, None)),
    }
    hip.hipDeviceSynchronize()
    for p in (d_raw, d_in, d_out, d_frames):
        hip.hipFree(p)
    return legs


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_frames.json")
    Lib = _lib.lib()
    eng = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
    n_out = eng.output_len(L)
    rng = np.random.default_rng(0)
    q = rng.integers(-16000, 16000, (L, CH), dtype=np.int64)
    i16 = rocoder_amd.pinned_empty((L, CH), np.int16)
    i16[:] = q
    x = rocoder_amd.pinned_empty((CH, L))
    x[:] = (q.astype(np.float32) / np.float32(32767.0)).T
    f32 = rocoder_amd.pinned_empty((L, CH))
    f32[:] = x.T
    y = rocoder_amd.pinned_empty((CH, n_out))
    yf = rocoder_amd.pinned_empty((n_out, CH))
    sink = np.empty((n_out, CH), np.float32)
    sink[:] = 0
    with tempfile.TemporaryDirectory() as tmp:
        host = build_host_loops(tmp)
        fpp = C.POINTER(C.c_float)
        rows_in = (fpp * CH)(*[x[c].ctypes.data_as(fpp) for c in range(CH)])
        rows_out = (fpp * CH)(*[y[c].ctypes.data_as(fpp) for c in range(CH)])
        host.decode_i16.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, C.POINTER(fpp)]
        host.interleave.argtypes = [C.POINTER(fpp), C.c_size_t, C.c_uint, C.c_void_p]

        def leg2():
            host.decode_i16(i16.ctypes.data, L * CH, CH, rows_in)
            eng.stretch_host(x, out=y)
            host.interleave(rows_out, n_out, CH, sink.ctypes.data)

        legs = [("1_stretch_host_pinned_f32_rows", lambda: eng.stretch_host(x, out=y)),
                ("2_host_loops_plus_stretch_host", leg2),
                ("3_stretch_frames_f32", lambda: eng.stretch_frames(f32, out=yf)),
                ("4_stretch_frames_i16", lambda: eng.stretch_frames(i16, out=yf))]
        times = {name: [] for name, _ in legs}
        for r in range(WARM + ROUNDS):
            for name, fn in legs:
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if r >= WARM:
                    times[name].append(dt)
        ref = eng.stretch_host(x, out=y).T
        equal = bool(np.array_equal(eng.stretch_frames(i16, out=yf), ref)) and bool(np.array_equal(eng.stretch_frames(f32, out=yf), ref))
    res = {"job": dict(channels=CH, window_len=N, factor=F, frames=L, out_frames=n_out), "warmups": WARM, "rounds": ROUNDS,
           "kernel_id": Lib.rc_kernel_id().decode(), "frames_equal_host_form": equal, "ms": times, "kernel_ms": kernel_legs(Lib, n_out)}
    summ = {}
    for k, v in list(times.items()) + list(res["kernel_ms"].items()):
        summ[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{k:36s} median {summ[k]['median']:9.3f} ms   min {summ[k]['min']:9.3f}   max {summ[k]['max']:9.3f}", flush=True)
    one, three = summ["1_stretch_host_pinned_f32_rows"], summ["3_stretch_frames_f32"]
    res["summary"] = summ
    res["acceptance"] = dict(leg1_median=one["median"], leg1_spread=one["max"] - one["min"], leg3_median=three["median"],
                             passed=three["median"] <= one["median"] + (one["max"] - one["min"]))
    print("frames == host form:", equal, "  acceptance:", res["acceptance"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    return 0 if res["acceptance"]["passed"] and equal else 1


if __name__ == "__main__":
    sys.exit(main())

"""The phase modes (rc_engine_set_phase_mode) on the stereo f = 8, L = 2 646 000 job at N = 1024 / 4096 / 16384,
device-resident input and output; 3 warm-ups, then 10 rounds in which the variants take turns in one process; medians and
the min-max spread per leg, HIP-event times throughout.

  1  the whole job's launches (rc_engine_last_kernel_stats): PROPAGATE and LOCKED next to the same job through an identity
     user device kernel - the same analysis, synthesis and overlap-add launches with a copy kernel in the stage's place -
     and next to RANDOM (the fused kernel: no spectrum in HBM at all).
  2  each launch of the stage (prep in both modes, scan, walk, apply) on one chunk of the job's hops, next to a
     device-to-device copy that moves the bytes the launch reads and writes.
  3  scan and walk on the same chunk at B = 16 ... 256 hops per block, the values taking turns behind a fresh prep: what
     the shipped block size is held against.

Nothing is gated: there is no target number. usage: python tools/bench_phase.py [out.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rocoder_amd  # noqa: E402
from bench_frames import launcher  # noqa: E402
from bench_frames_pcm import summarise  # noqa: E402
from rocoder_amd import _lib  # noqa: E402

CH, F, L = 2, 8.0, 2_646_000
WINDOWS = (1024, 4096, 16384)
WARM, ROUNDS = 3, 10


def shipped_block(hops):  # rc::phase_scan_block (rocoder_amd/csrc/rc_phase.h)
    b = 16
    while b < 256 and 6 * b * b < hops:
        b *= 2
    return b

SWEEP = (16, 32, 64, 128, 256)  # the block sizes scan + walk are timed at, beside the shipped one
IDENTITY = "__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) { return X[j]; }"


class PrepParams(C.Structure):  # rc::PhasePrepParams (rocoder_amd/csrc/rc_phase.h)
    _fields_ = [("spec", C.c_void_p), ("pe", C.c_void_p), ("n", C.c_uint32), ("step", C.c_uint32), ("locked", C.c_uint32),
                ("n_channels", C.c_uint32), ("halo", C.c_uint32), ("hop_count", C.c_int64)]


class ScanParams(C.Structure):
    _fields_ = [("pe", C.c_void_p), ("n", C.c_uint32), ("n_channels", C.c_uint32), ("block", C.c_uint32), ("hop_count", C.c_int64)]


class WalkParams(C.Structure):
    _fields_ = [("pe", C.c_void_p), ("base", C.c_void_p), ("theta", C.c_void_p), ("n", C.c_uint32), ("n_channels", C.c_uint32),
                ("block", C.c_uint32), ("hop_count", C.c_int64)]


class ApplyParams(C.Structure):
    _fields_ = [("spec", C.c_void_p), ("out", C.c_void_p), ("pe", C.c_void_p), ("base", C.c_void_p), ("n", C.c_uint32),
                ("n_channels", C.c_uint32), ("halo", C.c_uint32), ("block", C.c_uint32), ("hop_count", C.c_int64)]


def job_legs(N):
    """kernel time of the whole job per variant, the variants taking turns"""
    import torch

    x = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, (CH, L)).astype(np.float32)).to("cuda")
    engines = {}
    for name in ("random", "identity_kernel", "propagate", "locked"):
        e = rocoder_amd.Engine(window_len=N, factor=F, channels=CH, seed=1)
        if name == "identity_kernel":
            e.set_device_kernel_source(IDENTITY)
        elif name != "random":
            e.set_phase_mode(name)
        engines[name] = e
    out = torch.empty((CH, engines["random"].output_len(L)), dtype=torch.float32, device="cuda")
    times = {k: [] for k in engines}
    launches = {}
    for r in range(WARM + ROUNDS):
        for name, e in engines.items():
            e.stretch_tensor(x, out=out)
            torch.cuda.synchronize()
            e.synchronize()
            ms, hops, n_launch = e.last_kernel_stats()
            launches[name] = n_launch
            if r >= WARM:
                times[name].append(ms)
    step, hops = engines["random"].params.sample_step_len, hops // CH
    for e in engines.values():
        e.close()
    return dict(ms=times, launches=launches, hops_per_channel=hops, step=step)


def launch_legs(Lib, N, step, hops):
    """event time of each launch of the stage on `hops` hops per channel of random spectra, and of the copies"""
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

    fns = {}
    for name, ty in (("launch_phase_prep", PrepParams), ("launch_phase_scan", ScanParams), ("launch_phase_walk", WalkParams),
                     ("launch_phase_apply", ApplyParams)):
        fns[name] = launcher(Lib, name)
        fns[name].argtypes = [C.POINTER(ty), C.c_void_p]
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def once(fn):
        assert hip.hipEventRecord(ev0, None) == 0
        assert fn() == 0
        assert hip.hipEventRecord(ev1, None) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value

    nb, rows, BLOCK = N // 2 + 1, hops + 1, shipped_block(hops)
    n_blocks = (hops + BLOCK - 1) // BLOCK
    spec_bytes, pe_bytes, out_bytes = CH * rows * N * 8, CH * hops * 2 * nb * 4, CH * hops * N * 8
    base_bytes = CH * ((hops + min(SWEEP) - 1) // min(SWEEP)) * nb * 4  # (the most blocks of the sweep)
    d_spec, d_pe, d_out, d_base, d_theta = dmalloc(spec_bytes), dmalloc(pe_bytes), dmalloc(out_bytes), dmalloc(base_bytes), dmalloc(CH * nb * 4)
    host = np.random.default_rng(1).standard_normal(CH * rows * N * 2).astype(np.float32)
    assert hip.hipMemcpy(d_spec, host.ctypes.data, spec_bytes, 1) == 0
    # the bytes a launch reads and writes (the bins 0 ... H of a spectrum row: half of it)
    touched = dict(prep_locked=spec_bytes // 2 + pe_bytes, prep_propagate=spec_bytes // 2 + pe_bytes, scan=2 * pe_bytes,
                   walk=3 * CH * n_blocks * nb * 4, apply=spec_bytes // 2 + pe_bytes + out_bytes)
    d_copy = dmalloc(max(touched.values()))  # (a copy of half of them, source and target side by side)
    prep_l = PrepParams(d_spec.value, d_pe.value, N, step, 1, CH, 1, hops)
    prep_p = PrepParams(d_spec.value, d_pe.value, N, step, 0, CH, 1, hops)
    scan = ScanParams(d_pe.value, N, CH, BLOCK, hops)
    walk = WalkParams(d_pe.value, d_base.value, d_theta.value, N, CH, BLOCK, hops)
    app = ApplyParams(d_spec.value, d_out.value, d_pe.value, d_base.value, N, CH, 1, BLOCK, hops)
    legs = {
        "prep_propagate": lambda: fns["launch_phase_prep"](C.byref(prep_p), None),
        "prep_locked": lambda: fns["launch_phase_prep"](C.byref(prep_l), None),
        "scan": lambda: fns["launch_phase_scan"](C.byref(scan), None),
        "walk": lambda: fns["launch_phase_walk"](C.byref(walk), None),
        "apply": lambda: fns["launch_phase_apply"](C.byref(app), None),
    }
    for k, b in list(touched.items()):
        half = b // 2 // 16 * 16  # a copy reads and writes each byte once
        legs["copy_of_" + k] = (lambda h: lambda: hip.hipMemcpyAsync(d_copy, C.c_void_p(d_copy.value + h), h, 3, None))(half)
    times = {k: [] for k in legs}
    for r in range(WARM + ROUNDS):
        # (scan rewrites the rows prep made: the order prep_locked -> scan -> walk -> apply is the engine's, every round)
        for k in ("prep_propagate", "prep_locked", "scan", "walk", "apply") + tuple(k for k in legs if k.startswith("copy_of_")):
            ms = once(legs[k])
            if r >= WARM:
                times[k].append(ms)
    sweep = {f"B{b}_{k}": [] for b in SWEEP for k in ("scan", "walk")}
    for r in range(WARM + ROUNDS):
        for b in SWEEP:
            scan_b, walk_b = ScanParams(d_pe.value, N, CH, b, hops), WalkParams(d_pe.value, d_base.value, d_theta.value, N, CH, b, hops)
            once(legs["prep_locked"])  # (scan rewrites the rows in place: fresh ones for every value)
            t_scan = once(lambda: fns["launch_phase_scan"](C.byref(scan_b), None))
            t_walk = once(lambda: fns["launch_phase_walk"](C.byref(walk_b), None))
            if r >= WARM:
                sweep[f"B{b}_scan"].append(t_scan)
                sweep[f"B{b}_walk"].append(t_walk)
    hip.hipDeviceSynchronize()
    for p in (d_spec, d_pe, d_out, d_base, d_theta, d_copy):
        hip.hipFree(p)
    return dict(ms=times, hops_per_channel=hops, scan_block=BLOCK, bytes_touched=touched, block_sweep_ms=sweep)


def next_profile():
    prof = os.path.join(ROOT, "profiles")
    used = {int(f[1:3]) for f in os.listdir(prof) if len(f) > 3 and f[0] == "r" and f[1:3].isdigit()}
    return os.path.join(prof, "r%02d_phase.json" % (max(used) + 1))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else next_profile()
    Lib = _lib.lib()
    res = {"job": dict(channels=CH, factor=F, frames=L), "warmups": WARM, "rounds": ROUNDS,
           "kernel_id": Lib.rc_kernel_id().decode(), "windows": {}}
    from boxclock import ClockSampler
    with ClockSampler(0) as clk:
        for N in WINDOWS:
            print(f"--- N = {N}", flush=True)
            job = job_legs(N)
            job["summary"] = summarise({f"N{N} job {k}": v for k, v in job["ms"].items()})
            # one chunk of run_unfused: 1 GiB of spectra, y and (P, e) rows, whole windows (two hops each at pitch 1), the
            # halo hop off, at most 32 767
            budget = (1 << 30) // ((N * 28 + (N + 2) * 4) * CH) - 1
            chunk = min(job["hops_per_channel"], max(2, min(budget // 2 * 2, 32767)))
            lau = launch_legs(Lib, N, job["step"], chunk)
            lau["summary"] = summarise({f"N{N} launch {k}": v for k, v in lau["ms"].items()})
            lau["block_sweep_summary"] = summarise({f"N{N} sweep {k}": v for k, v in lau["block_sweep_ms"].items()})
            res["windows"][str(N)] = dict(job=job, launches=lau)
    res["box"] = dict(device="MI355X (gfx950)", median_sclk_mhz=clk.median_mhz())
    print("box:", res["box"], flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""What whole-hop sums (RC_SUMS, X.sum(i)) cost a user device kernel, on one GPU, on the C2-shaped job: stereo,
L = 2 646 000 per channel, window 16384, factor 8, device-resident input and output. The engine's event time of the
kernel launches (rc_engine_kernel_times), --reps timed calls after --warmup, the variants interleaved:
  (a) identity            an undeclared user kernel, Y = X: the path this feature leaves alone;
      identity_with_pass  the same rc_apply under RC_SUMS 1 (term |X|^2, the sum unused): (a) plus the pass alone;
  (b) auto_gain           examples/kernels/auto_gain.hip;
  (c) centroid_tilt       examples/kernels/centroid_tilt.hip (two sums).
The pass's own time is identity_with_pass - identity (medians); next to it, a device-to-device copy of the bytes the
pass reads, rows x N x 8 (torch events, same reps). `spread_ms` is max - min over the reps of a variant: two builds agree
on (a) when their medians differ by less than that.
`--root <tree of another build> --only-identity` measures (a) with another build, for a comparison in the same visit.
Prints one JSON line.   python tools/bench_user_dk_sums.py [--root DIR] [--only-identity] [--reps 10] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
IDENT = HEAD + "{ return X[j]; }"
IDENT_WITH_PASS = ("#define RC_SUMS 1\n"
                   "__device__ float rc_sum_term(const rc_spectrum &X, uint32_t j, const rc_hop &h, uint32_t i) "
                   "{ float2 x = X[j]; return x.x * x.x + x.y * x.y; }\n" + IDENT)
JOB = dict(window_len=16384, factor=8.0, channels=2, L=2_646_000)


def example(name):
    with open(os.path.join(HERE, "examples", "kernels", name)) as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--only-identity", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch

    import rocoder_amd

    C, L, N = JOB["channels"], JOB["L"], JOB["window_len"]
    xd = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, (C, L)).astype(np.float32)).cuda()
    variants = {"identity": (IDENT, None)}
    if not a.only_identity:
        variants["identity_with_pass"] = (IDENT_WITH_PASS, None)
        variants["auto_gain"] = (example("auto_gain.hip"), [N / 8.0, 1.0])
        variants["centroid_tilt"] = (example("centroid_tilt.hip"), [2.0])
    engines, outs = {}, {}
    for name, (src, params) in variants.items():
        e = rocoder_amd.Engine(window_len=N, factor=JOB["factor"], channels=C, seed=1)
        e.set_device_kernel_source(src)
        if params:
            e.set_device_kernel_params(params)
        engines[name] = e
        outs[name] = torch.empty((C, e.output_len(L)), device="cuda")
    hops = (engines["identity"].output_len(L) // int(engines["identity"].params.window_out_len)) * \
        int(engines["identity"].params.hops_per_window)
    rows = C * hops
    pass_bytes = rows * N * 8
    src_buf = torch.empty(pass_bytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst_buf = torch.empty_like(src_buf)
    times = {n: [] for n in variants}
    copy_ms, launches = [], {}
    for rep in range(a.warmup + a.reps):
        for n, e in engines.items():
            e.stretch_tensor(xd, out=outs[n])
            torch.cuda.synchronize()
            e.synchronize()
            launches[n] = e.last_kernel_stats()[2]
            if rep >= a.warmup:
                times[n].append(round(float(e.kernel_times(1)[-1]), 4))
        if not a.only_identity:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            dst_buf.copy_(src_buf)
            t1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                copy_ms.append(round(float(t0.elapsed_time(t1)), 4))
    res = {n: dict(median_ms=round(statistics.median(t), 4), min_ms=min(t), max_ms=max(t), spread_ms=round(max(t) - min(t), 4),
                   ms=t, launches=launches[n]) for n, t in times.items()}
    out = dict(bench="user_dk_sums", kernel_id=rocoder_amd._lib.lib().rc_kernel_id().decode(),
               root=os.path.basename(os.path.abspath(a.root)), reps=a.reps, warmup=a.warmup, job=JOB, rows=rows, results=res)
    if not a.only_identity:
        silent = [n for n in variants if not bool(torch.any(outs[n] != 0))]
        pass_ms = res["identity_with_pass"]["median_ms"] - res["identity"]["median_ms"]
        out["pass"] = dict(bytes_read=pass_bytes, own_ms=round(pass_ms, 4), copy_of_those_bytes_ms=round(statistics.median(copy_ms), 4),
                           copy_ms=copy_ms, gb_per_s=round(pass_bytes / max(pass_ms, 1e-6) / 1e6, 1),
                           ratio_to_copy=round(pass_ms / statistics.median(copy_ms), 3))
        out["silent_outputs"] = silent
    for e in engines.values():
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

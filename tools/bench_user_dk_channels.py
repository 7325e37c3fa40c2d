"""What a user device kernel that reads the other channels (RC_CROSS_CHANNEL, X.channel(c)) costs, on one GPU:
  C2-shaped job: stereo, L = 2 646 000 per channel, window 16384, factor 8;
  C5-shaped job: 8 channels, L = 5 292 000 per channel, window 65536, factor 32;
device-resident input and output, the engine's event time of the kernel launches (rc_engine_kernel_times), 10 timed
calls after 3 warm-ups, the variants interleaved. Per job:
  (a) `swap` (Y = X of the next channel) against the undeclared x2 kernel, whole job;
  (b) the same pair for channel 0 only, through rc_engine_stretch_device_range;
  (c) the x2 kernel alone is also what `--root <tree of another build> --only-x2` measures, for a comparison of builds
      in the same visit.
Prints one JSON line with the medians and the raw timings.
   python tools/bench_user_dk_channels.py [--root DIR] [--only-x2] [--reps 10] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HEAD = "__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
X2 = HEAD + "{ float2 x = X[j]; return make_float2(2.f * x.x, 2.f * x.y); }"
SWAP = "#define RC_CROSS_CHANNEL 1\n" + HEAD + "{ return X.channel((h.channel + 1) % h.channels)[j]; }"
JOBS = {"c2": dict(window_len=16384, factor=8.0, channels=2, L=2_646_000),
        "c5": dict(window_len=65536, factor=32.0, channels=8, L=5_292_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only-x2", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch

    import rocoder_amd

    res = {}
    for job, spec in JOBS.items():
        C, L = spec["channels"], spec["L"]
        xd = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, (C, L)).astype(np.float32)).cuda()
        kernels = {"x2": X2} if a.only_x2 else {"x2": X2, "swap": SWAP}
        engines, calls = {}, {}
        for name, src in kernels.items():
            e = rocoder_amd.Engine(window_len=spec["window_len"], factor=spec["factor"], channels=C, seed=1)
            e.set_device_kernel_source(src)
            engines[name] = e
            out = torch.empty((C, e.output_len(L)), device="cuda")
            wins = e.output_len(L) // int(e.params.window_out_len)
            calls[f"{name}_whole"] = (e, lambda e=e, out=out: e.stretch_tensor(xd, out=out))
            calls[f"{name}_one_channel"] = (e, lambda e=e, out=out, wins=wins: e.stretch_device_range_ptr(
                xd.data_ptr(), xd.stride(0), L, 0, 1, 0, wins, out.data_ptr(), out.stride(0), out.shape[1]))
        times = {n: [] for n in calls}
        launches = {}
        for rep in range(a.warmup + a.reps):
            for n, (e, call) in calls.items():
                call()
                torch.cuda.synchronize()
                e.synchronize()
                launches[n] = e.last_kernel_stats()[2]
                if rep >= a.warmup:
                    times[n].append(round(float(e.kernel_times(1)[-1]), 4))
        res[job] = {n: dict(median_ms=round(statistics.median(t), 4), min_ms=min(t), max_ms=max(t), ms=t,
                            launches=launches[n]) for n, t in times.items()}
        for e in engines.values():
            e.close()
        del xd
    print(json.dumps(dict(bench="user_dk_channels", kernel_id=rocoder_amd._lib.lib().rc_kernel_id().decode(),
                          root=os.path.basename(os.path.abspath(a.root)), reps=a.reps, warmup=a.warmup, results=res)))


if __name__ == "__main__":
    main()

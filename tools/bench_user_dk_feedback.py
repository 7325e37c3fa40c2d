"""What a feedback kernel (RC_FEEDBACK, X.out(d)) costs, and where its two launch shapes cross, on one GPU: stereo,
L = 2 646 000 per channel, factor 8, device-resident input and output, at the window lengths of --windows. The engine's
event time of the kernel launches (rc_engine_kernel_times), --reps timed calls after --warmup, the variants of a window
length interleaved:
  identity        an undeclared user kernel, Y = X: the path this feature leaves alone (product library);
  smooth          examples/kernels/smooth.hip, a = 0.5, in the shape the engine picks (product library);
  smooth_per_hop  the same, one launch per hop     } the test-hook library, ROCODER_DIAG bit 16 / bit 32: both shapes at
  smooth_loop     the same, one launch per chunk   } every window length, whatever kFeedbackLoopMaxN says
`spread_ms` is max - min over the reps of a variant: two builds agree on identity when their medians differ by less.
`--root <tree of another build> --only-identity` measures identity with another build, for a comparison in the same visit.
Prints one JSON line.
  python tools/bench_user_dk_feedback.py [--root DIR] [--only-identity] [--windows 1024,4096,16384,65536] [--reps 10] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
IDENT = HEAD + "{ return X[j]; }"
JOB = dict(factor=8.0, channels=2, L=2_646_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--only-identity", action="store_true")
    ap.add_argument("--windows", default="1024,4096,16384,65536")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch

    import rocoder_amd
    from rocoder_amd import _lib

    C, L = JOB["channels"], JOB["L"]
    xd = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, (C, L)).astype(np.float32)).cuda()
    with open(os.path.join(HERE, "examples", "kernels", "smooth.hip")) as f:
        smooth = f.read()
    results = {}
    for N in [int(w) for w in a.windows.split(",")]:
        engines = {}

        def engine(src, params=None):
            e = rocoder_amd.Engine(window_len=N, factor=JOB["factor"], channels=C, seed=1)
            e.set_device_kernel_source(src)
            if params:
                e.set_device_kernel_params(params)
            return e

        engines["identity"] = engine(IDENT)
        if not a.only_identity:
            engines["smooth"] = engine(smooth, [0.5])
            with _lib.hooks_library():
                for name, bit in (("smooth_per_hop", "16"), ("smooth_loop", "32")):
                    os.environ["ROCODER_DIAG"] = bit
                    engines[name] = engine(smooth, [0.5])
                del os.environ["ROCODER_DIAG"]
        out = torch.empty((C, engines["identity"].output_len(L)), device="cuda")
        times = {n: [] for n in engines}
        launches, hops = {}, 0
        for rep in range(a.warmup + a.reps):
            for n, e in engines.items():
                e.stretch_tensor(xd, out=out)
                torch.cuda.synchronize()
                e.synchronize()
                _, hops, launches[n] = e.last_kernel_stats()
                if rep >= a.warmup:
                    times[n].append(round(float(e.kernel_times(1)[-1]), 4))
        silent = not bool(torch.any(out != 0))
        res = {n: dict(median_ms=round(statistics.median(t), 4), min_ms=min(t), max_ms=max(t), spread_ms=round(max(t) - min(t), 4),
                       ms=t, launches=launches[n]) for n, t in times.items()}
        if not a.only_identity:
            res["faster_shape"] = "loop" if res["smooth_loop"]["median_ms"] < res["smooth_per_hop"]["median_ms"] else "per_hop"
        results[str(N)] = dict(hops_per_channel=hops // C, silent=silent, **res)
        for e in engines.values():
            e.close()
    print(json.dumps(dict(bench="user_dk_feedback", kernel_id=rocoder_amd._lib.lib().rc_kernel_id().decode(),
                          root=os.path.basename(os.path.abspath(a.root)), reps=a.reps, warmup=a.warmup, job=JOB, results=results)))


if __name__ == "__main__":
    main()

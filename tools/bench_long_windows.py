#!/usr/bin/env python3
"""Long-window path on one GPU: stereo, factor 8, input resident in HBM, one warm-up and the median of
>= 5 stretch_tensor launches per window length. One JSON line per length: ms per launch (host wall clock around a
synchronised launch, and the engine's own kernel time), hops/s, output Msamples/s, rc_engine_create time, the traffic
model (bytes per hop of every pass, from the shapes) and the GB/s it implies for the whole job next to a device copy
measured in the same run.

usage: python tools/bench_long_windows.py [--lengths 131072,262144,...] [--launches 5] [--hops 64]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def traffic(N, pitch=1):
    """HBM bytes per hop of each pass of the plain stretch (launch_long stage 3 + launch_long_ola): 8 B per complex
    point of the work buffer, 4 B per sample; tables are not counted (they stay in the caches)."""
    M = N // 2
    if N & (N - 1) == 0:
        P = M
        passes = {
            "col_fwd": 4 * N + 8 * P,      # samples in, work buffer out
            "row_fwd": 16 * P,
            "pair": 16 * P,
            "row_inv": 16 * P,
            "col_inv": 8 * P + 4 * N,      # work buffer in, y out
        }
    else:
        P = 1
        while P < 2 * M - 1:
            P *= 2
        passes = {
            "col_fwd": 4 * N + 8 * P,
            "row_conv_fwd": 24 * P,        # row in / out + FFT_L(conj chirp)
            "col_post": 8 * P + 8 * M,
            "pair": 16 * M,
            "col_pre": 8 * M + 8 * P,
            "row_conv_inv": 24 * P,
            "col_inv": 8 * P + 4 * N,
        }
    passes["ola"] = 4 * N + 4 * (N // 2) // pitch  # y_k and y_{k-1}'s tail in, H / p samples out
    return P, passes


def copy_gbs(torch, mib=1024, reps=5):
    a = torch.empty(mib << 18, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 2 * a.numel() * 4 / statistics.median(ts) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="131072,262144,1048576,4194304,100000,4194302")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--hops", type=int, default=64, help="hops per channel (at least)")
    ap.add_argument("--factor", type=float, default=8.0)
    a = ap.parse_args()
    import numpy as np
    import torch

    import rocoder_amd as ra

    gbs_copy = copy_gbs(torch)
    for N in [int(v) for v in a.lengths.split(",")]:
        d = ra.derive_params(window_len=N, factor=a.factor)
        L = N + (a.hops - 1) * d.sample_step_len
        x = np.stack([np.sin(np.arange(L) * (0.01 + 0.003 * c)).astype(np.float32) for c in range(2)])
        xt = torch.from_numpy(x).cuda()
        t0 = time.perf_counter()
        e = ra.Engine(window_len=N, factor=a.factor, channels=2, seed=1)
        create_ms = (time.perf_counter() - t0) * 1e3
        try:
            out = torch.empty((2, e.output_len(L)), dtype=torch.float32, device="cuda")
            e.stretch_tensor(xt, out=out)
            torch.cuda.synchronize()
            wall, kern = [], []
            for _ in range(max(5, a.launches)):
                t0 = time.perf_counter()
                e.stretch_tensor(xt, out=out)
                torch.cuda.synchronize()
                e.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(e.last_kernel_stats()[0])
            ms = statistics.median(wall)
            kms, hops, launches = statistics.median(kern), e.last_kernel_stats()[1], e.last_kernel_stats()[2]
        finally:
            e.close()
        P, passes = traffic(N)
        per_hop = sum(passes.values())
        print(json.dumps({
            "window_len": N, "channels": 2, "factor": a.factor, "hops": hops, "launches": launches,
            "ms_per_stretch": round(ms, 3), "kernel_ms": round(kms, 3),
            "hops_per_s": round(hops / (ms / 1e3), 1), "out_msamples_per_s": round(2 * out.shape[1] / (ms / 1e3) / 1e6, 1),
            "create_ms": round(create_ms, 1), "fft_points": P, "bytes_per_hop": passes, "bytes_per_hop_total": per_hop,
            "model_gbs": round(per_hop * hops / (kms / 1e3) / 1e9, 1), "copy_gbs": round(gbs_copy, 1),
            "model_share_of_copy": round(per_hop * hops / (kms / 1e3) / 1e9 / gbs_copy, 3),
        }), flush=True)


if __name__ == "__main__":
    main()

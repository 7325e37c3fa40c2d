"""User device kernels (rc_dk_compile / rc_engine_load_device_kernel) against what they replace, on the BASELINE C2/C4
job (stereo, L = 2 646 000 per channel, window 16384, factor 8), device-resident input and output:
  * a user SHIFT kernel against the curated RC_DK_SHIFT (the same pipeline: analysis -> kernel -> synthesis -> OLA);
  * the README's x2 kernel as a user device kernel (C4 at GPU speed) against the plain stretch (C2);
  * examples/kernels/blur.hip at RC_HISTORY 1, 3 and 8 (a weighted sum over the hop and the D hops before it) against
    the x2 kernel of the same run: what reading earlier hops costs;
  * hiprtc compile time: cold (first compile in a fresh process) and warm.
Wall time per call (median of --reps after one warm-up, the variants interleaved) and the engine's event time of the
kernel launches. Prints one JSON line.   python tools/bench_user_dk.py [--reps 7]
(The host-kernel C4 figure to compare with is tools/bench_c4.py's.)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

X2 = ("__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) "
      "{ float2 x = X[j]; return make_float2(2.f * x.x, 2.f * x.y); }")
SHIFT = """
__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h) {
    const uint32_t M = h.n / 2;
    const uint32_t f = j <= M ? j : h.n - j;
    const int64_t src = (int64_t)f - 7;
    float2 y = make_float2(0.f, 0.f);
    if (src >= 0 && src <= (int64_t)M) {
        y = X[src];
        if (j > M) y.y = -y.y;
    }
    return y;
}
"""

COMPILE_CHILD = r"""
import json, sys, time
sys.path.insert(0, sys.argv[1])
import rocoder_amd
src = sys.argv[2]
t0 = time.perf_counter(); rocoder_amd.compile_device_kernel(src); t1 = time.perf_counter()
rocoder_amd.compile_device_kernel(src + "\n// warm"); t2 = time.perf_counter()
print(json.dumps(dict(cold_ms=(t1 - t0) * 1e3, warm_ms=(t2 - t1) * 1e3)))
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch

    import rocoder_amd

    xh = np.random.default_rng(0).uniform(-0.5, 0.5, (2, 2_646_000)).astype(np.float32)
    xd = torch.from_numpy(xh).cuda()
    job = dict(window_len=16384, factor=8.0, channels=2, seed=1)
    variants = {"plain_c2": dict(), "curated_shift": dict(device_kernel=("shift", 7)),
                "user_shift": dict(src=SHIFT), "user_x2_c4": dict(src=X2)}
    with open(os.path.join(ROOT, "examples", "kernels", "blur.hip")) as f:
        blur = f.read()
    for depth in (1, 3, 8):
        variants[f"user_blur_d{depth}"] = dict(src=f"#define RC_HISTORY {depth}\n" + blur,
                                               params=[1.0 / (depth + 1)] * (depth + 1))
    engines, outs = {}, {}
    for name, v in variants.items():
        kw = dict(job)
        kw.update({k: val for k, val in v.items() if k not in ("src", "params")})
        e = rocoder_amd.Engine(**kw)
        if "src" in v:
            e.set_device_kernel_source(v["src"])
        if "params" in v:
            e.set_device_kernel_params(v["params"])
        engines[name] = e
        outs[name] = torch.empty((2, e.output_len(xd.shape[1])), device="cuda")
        e.stretch_tensor(xd, out=outs[name])
        torch.cuda.synchronize()
        e.synchronize()
    wall = {n: [] for n in variants}
    ev = {n: [] for n in variants}
    for _ in range(a.reps):
        for n, e in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.stretch_tensor(xd, out=outs[n])
            torch.cuda.synchronize()
            e.synchronize()
            wall[n].append((time.perf_counter() - t0) * 1e3)
            ev[n].append(e.kernel_times(1)[-1])
    same = bool(torch.equal(outs["user_shift"], outs["curated_shift"]))
    res = {n: dict(wall_ms=round(statistics.median(wall[n]), 3), kernel_ms=round(statistics.median(ev[n]), 3),
                   launches=engines[n].last_kernel_stats()[2]) for n in variants}
    for e in engines.values():
        e.close()
    child = subprocess.run([sys.executable, "-c", COMPILE_CHILD, ROOT, X2], capture_output=True, text=True, timeout=600)
    comp = json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0 else dict(error=child.stderr[-500:])
    print(json.dumps(dict(bench="user_dk", kernel_id=rocoder_amd._lib.lib().rc_kernel_id().decode(), reps=a.reps,
                          user_shift_equals_curated=same, results=res,
                          compile_ms={k: round(v, 1) for k, v in comp.items()} if "error" not in comp else comp)))


if __name__ == "__main__":
    main()

"""A/B of the run plan's taper of the N = 16384 kernel inside ONE process, interleaved (cancels clock / thermal drift),
on the C2 job:
python tools/ab_taper.py "-1" "-1,1" "0" "0,1" "2" "3" ...   (one engine of the test-hook build per configuration: it
reads ROCODER_TAPER once, at create: -1 no taper = the plan of round 6, 0 the shipped shape, n > 0 build_run_table's
taper_div2. A second number only tells two engines of one configuration apart: the spread of same-configuration repeats.)
Every configuration's output must equal the first one's bit for bit.
Prints per configuration the kernel time (the engine's event pair) and the time per step of 12 back-to-back calls."""
import os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rocoder_amd
from rocoder_amd import _lib
cfgs = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(-1,), (0,)]
REPS = int(os.environ.get("ROCODER_AB_REPS", "12"))
dev = torch.device("cuda", 0)
x = (torch.rand((2, 26_460_000), device=dev) - 0.5)
stream = torch.cuda.Stream(dev)
res = {c: [] for c in cfgs}
step = {c: [] for c in cfgs}
with torch.cuda.stream(stream):
    eng = {}
    with _lib.hooks_library():
        for c in cfgs:
            os.environ["ROCODER_TAPER"] = str(c[0])
            eng[c] = rocoder_amd.Engine(window_len=16384, factor=8.0, channels=2, seed=1)
    e = eng[cfgs[0]]
    ref = torch.empty((2, e.output_len(x.shape[1])), device=dev)
    out = torch.empty_like(ref)
    e.stretch_tensor(x, out=ref)
    for c in cfgs[1:]:
        out.zero_()
        eng[c].stretch_tensor(x, out=out)
        stream.synchronize()
        print(f"taper {c}: output bit-equal to the first configuration's: {torch.equal(out, ref)}")
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 3.0:
        for _ in range(16):
            e.stretch_tensor(x, out=out)
        stream.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(REPS):
        for c in cfgs:
            e = eng[c]
            e.stretch_tensor(x, out=out)
            ev0.record(stream)
            for _ in range(12):
                e.stretch_tensor(x, out=out)
            ev1.record(stream)
            stream.synchronize()
            res[c] += e.kernel_times(10)
            step[c].append(ev0.elapsed_time(ev1) / 12)
for c in cfgs:
    v, s = res[c], step[c]
    print(f"taper {str(c):8s}: kernel median {statistics.median(v):.4f} ms  min {min(v):.4f}  n={len(v)}   "
          f"step median {statistics.median(s):.4f} ms  min {min(s):.4f}  max {max(s):.4f}")

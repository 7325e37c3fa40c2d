"""A/B of engine LIBRARIES on the C2 job inside ONE process, interleaved (cancels clock / thermal drift):
python tools/ab_libs.py rocoder_amd/lib_parent.so rocoder_amd/librocoder_hip.so ...
(variants: tools/build_variant.sh, or a copy of another commit's librocoder_hip.so). A path may be given twice: two
engines of one library, whose difference is the spread of same-library repeats. Every library's output must equal the
first one's bit for bit. Prints per engine the kernel time (the engine's event pair around the kernel) and the time per
step of 12 back-to-back calls (events on the stream: prep dispatch, kernel and the gaps between them)."""
import os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rocoder_amd
from rocoder_amd import _lib
paths = sys.argv[1:]
REPS = int(os.environ.get("ROCODER_AB_REPS", "12"))
dev = torch.device("cuda", 0)
x = (torch.rand((2, 26_460_000), device=dev) - 0.5)
stream = torch.cuda.Stream(dev)
with torch.cuda.stream(stream):
    eng = []
    for p in paths:
        prev, _lib._lib = _lib._lib, _lib._load(os.path.abspath(p))  # (what hooks_library() does, for any library)
        try:
            eng.append(rocoder_amd.Engine(window_len=16384, factor=8.0, channels=2, seed=1))
        finally:
            _lib._lib = prev
    res, step = [[] for _ in eng], [[] for _ in eng]
    ref = torch.empty((2, eng[0].output_len(x.shape[1])), device=dev)
    out = torch.empty_like(ref)
    eng[0].stretch_tensor(x, out=ref)
    for i in range(1, len(eng)):
        out.zero_()
        eng[i].stretch_tensor(x, out=out)
        stream.synchronize()
        print(f"{paths[i]}: output bit-equal to {paths[0]}'s: {torch.equal(out, ref)}")
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 3.0:
        for _ in range(16):
            eng[0].stretch_tensor(x, out=out)
        stream.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(REPS):
        for i, e in enumerate(eng):
            e.stretch_tensor(x, out=out)
            ev0.record(stream)
            for _ in range(12):
                e.stretch_tensor(x, out=out)
            ev1.record(stream)
            stream.synchronize()
            res[i] += e.kernel_times(10)
            step[i].append(ev0.elapsed_time(ev1) / 12)
for i, p in enumerate(paths):
    v, s = res[i], step[i]
    print(f"{p:40s} kernel median {statistics.median(v):.4f} ms  min {min(v):.4f}  n={len(v)}   "
          f"step median {statistics.median(s):.4f} ms  min {min(s):.4f}  max {max(s):.4f}  ({REPS} alternations)")

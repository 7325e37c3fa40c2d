"""dev: the drain of a hop4_kernel launch, C2 shape. Needs the drain build
(tools/build_variant.sh drain -DRC_DRAIN=1 -DRC_DRAIN_DUMP, ROCODER_HIP_LIB=rocoder_amd/lib_drain.so): every workgroup
leaves the 100 MHz clock (s_memrealtime) at its ticket and on its way out. From them: the resident workgroups over time,
the moment the first XCD stops getting workgroups (its ticket counter and its neighbour's are dry), and the area above
the curve from there to the last exit, in slot-us and as a fraction of the launch's slots x time.
The drain build reads ROCODER_TAPER like the test-hook build (-1: the plan of round 6, 0: the shipped taper)."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, '.')
import rocoder_amd
dev = torch.device("cuda", 0)
x = (torch.rand((2, 26_460_000), device=dev) - 0.5)
path = os.environ.pop("ROCODER_DRAIN", "/tmp/rocoder_drain.txt")
e = rocoder_amd.Engine(window_len=16384, factor=8.0, channels=2, seed=1)
out = torch.empty((2, e.output_len(x.shape[1])), device=dev)
t_start = time.perf_counter()
while time.perf_counter() - t_start < 2.0:  # steady clocks first; the dump (a host synchronisation) only for the last launch
    for _ in range(16):
        e.stretch_tensor(x, out=out)
    torch.cuda.synchronize()
warm = float(np.median(e.kernel_times(16)))
os.environ["ROCODER_DRAIN"] = path
e.stretch_tensor(x, out=out)
torch.cuda.synchronize()
ms = e.kernel_times(1)[0]
lines = open(path).read().splitlines()
print(lines[0], f"| kernel {ms:.4f} ms, median of the 16 launches before it {warm:.4f} ms")
d = np.array([[int(v) for v in l.split()] for l in lines[1:]], dtype=np.int64)
d = d[d[:, 1] > 0]
base = d[:, 0].min()
t0, t1, xcd = (d[:, 0] - base) * 0.01, (d[:, 1] - base) * 0.01, d[:, 2]  # us
span = t1.max()
SLOTS, SLOTS_X = 768, 96
last_start = {xx: t0[xcd == xx].max() for xx in range(8)}
last_exit = {xx: t1[xcd == xx].max() for xx in range(8)}
dry = min(last_start.values())
grid = np.linspace(0, span, 2001)
resident = np.array([np.count_nonzero((t0 <= g) & (t1 > g)) for g in grid])
print(f"launch span {span:.1f} us (first ticket to last exit); the first XCD to get no more workgroups: at {dry:.1f} us; last ticket at {t0.max():.1f} us")
print("resident workgroups over time (of 768 slots), every 5 % of the launch and every 1 % of its last 20 %:")
for i in list(range(0, 1600, 100)) + list(range(1600, 2001, 20)):
    print(f"  {grid[i]:8.1f} us  {resident[i]:4d}")
m = grid >= dry
area = float(np.sum(SLOTS - np.minimum(resident[m], SLOTS))) * (grid[1] - grid[0])
print(f"idle area from {dry:.1f} us to the last exit: {area:.0f} slot-us = {area / (SLOTS * span) * 100:.2f} % of the launch's slots x time "
      f"({area / SLOTS:.1f} us of the whole chip)")
for xx in range(8):
    mx = xcd == xx
    gx = grid >= last_start[xx]
    rx = np.array([np.count_nonzero((t0[mx] <= g) & (t1[mx] > g)) for g in grid[gx]])
    ax = float(np.sum(SLOTS_X - np.minimum(rx, SLOTS_X))) * (grid[1] - grid[0])
    print(f"XCD {xx}: {np.count_nonzero(mx)} workgroups, last ticket {last_start[xx]:.1f} us, last exit {last_exit[xx]:.1f} us, "
          f"idle from its last ticket to the launch's end {ax:.0f} slot-us")
dur = t1 - t0
print(f"workgroup life: median {np.median(dur):.1f} us, 5 % {np.percentile(dur, 5):.1f}, 95 % {np.percentile(dur, 95):.1f}")

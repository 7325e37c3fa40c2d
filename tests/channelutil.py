"""Helpers of the channel-count parity tests (tests/test_channel_counts_host.py, tests/test_gpu_channel_counts.py): the
one table of cases (path, N, f, p, channels, L), the input, the references and the plan regimes. No GPU, no product
import: the planner is reached through a function the caller passes in (the test-hook library's rc_test_plan).

Sizes. A hop of the C oracle costs about N x 60 ns (1 ms at 16384, 8 ms at 65536), so a case holds about 1e7 / N hops
over all its channels: a few dozen hops per channel at the small counts, a handful at the large ones. The counts
above a path's resident workgroups (32769 channels at N = 64 ... 257 at 65536) run three windows; the last hop of every
job is a ragged one that the tail staging zero-pads. The references of the power-of-two windows are the C oracle's Stretchers,
one per channel as stretch_offline runs them, dealt to a pool of threads (the calls release the GIL);
tests/test_channel_counts_host.py holds the pool to stretch_offline bit for bit."""
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import windowutil
from oracle import cbind as oc
from oracle import oracle_np as onp
from windowutil import BLOCK_TOL, assert_blocks, assert_parity, rel_err  # noqa: F401  (the project's gates, unchanged)

SEED = 0xC4A27
N_CU = 256  # an MI355X; the table's counts "above the resident workgroups" are written for it
COUNTS = (1, 2, 3, 4, 5, 6, 8, 16, 17, 33, 64, 65)
THREADS = max(1, min(16, os.cpu_count() or 1))
BASELINE_ABOVE = 50_000_000  # output samples from which the reference is oc.cpu_baseline_stretch

# a fused path: window, factor, pitch multiple, the caller's window (a name of windowutil.WINDOWS) or None, the
# workgroups (hop slots below 512) that stay resident on N_CU CUs, and whether the kernel is hop4_kernel
Path = namedtuple("Path", "name N f p window resident hop4")
FUSED = [
    Path("slots64", 64, 2.0, 1, None, 128 * N_CU, False),
    Path("slots256", 256, 4.0, 1, None, 32 * N_CU, False),
    Path("wave512", 512, 2.0, 1, None, 16 * N_CU, False),
    Path("wave1024", 1024, 4.0, 2, None, 16 * N_CU, False),
    Path("wave2048", 2048, 2.0, 1, None, 12 * N_CU, False),
    Path("wave4096", 4096, 2.0, 1, None, 12 * N_CU, False),
    Path("wave8192", 8192, 2.0, 1, None, 6 * N_CU, False),
    Path("hop4_p1", 16384, 8.0, 1, None, 3 * N_CU, True),
    Path("hop4_p2", 16384, 4.0, 2, None, 3 * N_CU, True),
    Path("hop4_p3", 16384, 2.0, 3, None, 3 * N_CU, True),
    Path("hop4_p4", 16384, 2.0, 4, None, 3 * N_CU, True),  # (the run-time pitch instantiation)
    Path("hop4_window", 16384, 8.0, 1, "skew", 3 * N_CU, True),
    Path("big5s", 32768, 2.0, 1, None, N_CU, False),
    Path("big5", 65536, 2.0, 1, None, N_CU, False),
]
FUSED_BY_NAME = {p.name: p for p in FUSED}

Case = namedtuple("Case", "path N f p channels L window")

ONE_HOP, MULTI_ROUND, TAPER_GT3, CLAMPED = "all runs one hop", "longer runs, more than a round", "taper, > 3 channels", "resident clamped to 1"


def required_regimes(path):
    return {ONE_HOP, MULTI_ROUND, CLAMPED} | ({TAPER_GT3} if path.hop4 else set())


def step_of(N, f, p):
    return int(onp.derive(N, f, 1.0, p)["step"])


def hops_per_window(p):
    return 2 * p if p >= 1 else 2


def length_for(N, f, p, hops, ragged=7):
    """an input whose last whole hop is hop `hops` - 1, with a few samples more (the ragged hop behind it)"""
    return N + (hops - 1) * step_of(N, f, p) + ragged


def hop_count(case):
    """the hops per channel of the whole job (offline_windows x hops_per_window: rc_engine.cpp)"""
    step, hpw = step_of(case.N, case.f, case.p), hops_per_window(case.p)
    kd = (case.L - case.N) // step + 1 if case.L >= case.N else 0
    return (kd // hpw + 1) * hpw


def _fused_cases():
    cases = []
    for path in FUSED:
        N, f, p = path.N, path.f, path.p
        budget = max(2 * hops_per_window(p), 10_000_000 // N)
        for ch in COUNTS:
            hops = max(hops_per_window(p), min(40, budget // ch))
            cases.append(Case(path.name, N, f, p, ch, length_for(N, f, p, hops), path.window))
        # one count above the resident workgroups: three windows per channel. (Not one: the output of a single window
        # of a steady tone hangs on a few bins' random phases, and where they cancel - channel 397 of 769 at N = 16384,
        # output RMS 0.03 against 0.13 ... 0.22 beside it - every error is divided by that small RMS: the f32 oracle is
        # 1.2e-6 from its f64 twin there, against 1.5e-7 ... 3e-7 on the other channels.)
        cases.append(Case(path.name, N, f, p, path.resident + 1, length_for(N, f, p, 3 * hops_per_window(p)), path.window))
    # plans of more than a round whose resident share is not clamped, where the oracle stays in seconds: 64 channels
    # of a few hundred hops on the small windows
    for name, hops in (("slots64", 4800), ("slots256", 1200), ("wave512", 600), ("wave1024", 600)):
        path = FUSED_BY_NAME[name]
        cases.append(Case(name, path.N, path.f, path.p, 64, length_for(path.N, path.f, path.p, hops), path.window))
    # hop4_kernel's taper needs more than a round and a half of runs of at least 8 hops: 5 channels of 2 500 hops
    for path in FUSED:
        if path.hop4:
            cases.append(Case(path.name, path.N, path.f, path.p, 5, length_for(path.N, path.f, path.p, 2500), path.window))
    return cases


FUSED_CASES = _fused_cases()


def case_id(case):
    return f"{case.path}-c{case.channels}-L{case.L}"


# ------------------------------------------------------------------ plans and regimes
Plan = namedtuple("Plan", "runs_per_channel run_len tapered resident share")


def regimes(case, plan):
    """the regimes of the issue that `plan` (rc_test_plan's five words) is in"""
    hit = set()
    if plan.run_len == 1 and plan.runs_per_channel > 1:
        hit.add(ONE_HOP)
    if plan.run_len > 1 and plan.runs_per_channel * case.channels > plan.resident:
        hit.add(MULTI_ROUND)
    if plan.tapered and case.channels > 3:
        hit.add(TAPER_GT3)
    if plan.share == 0:
        hit.add(CLAMPED)
    return hit


def plan_of(plan_fn, n_cu, case):
    """plan_fn(n_cu, window_len, pitch, table_window, hop_count, channels) -> five words"""
    return Plan(*plan_fn(n_cu, case.N, case.p, 1 if case.window else 0, hop_count(case), case.channels))


# ------------------------------------------------------------------ input and references
def window_of(case):
    return windowutil.WINDOWS[case.window](case.N) if case.window else None


def case_input(case):
    return np.stack([onp.synth_input(c, case.L) for c in range(case.channels)])


def _one_channel(x, c, N, f, p, w, seed, kernel=None):
    st = oc.Stretcher(channels=x.shape[0], factor=f, pitch_multiple=p, window=w, seed=seed, channel_index=c, kernel=kernel)
    st.send(x[c])
    st.close_input()
    wins = []
    while not st.is_done():
        wins.append(st.next_window())
    return np.concatenate(wins)


def oracle_rows(x, N, f, p, seed=SEED, window=None, kernel=None, threads=THREADS):
    """[C, L] -> [C, n_out]: the C oracle, one Stretcher per channel (channel_index = the row), on a pool of threads"""
    w = oc.hanning(N) if window is None else np.ascontiguousarray(window, np.float32)
    n_out = oc.offline_output_len(x.shape[1], N, f, p)
    out = np.zeros((x.shape[0], n_out), np.float32)

    def run(c):
        y = _one_channel(x, c, N, f, p, w, seed, kernel)[:n_out]
        out[c, :y.size] = y

    if threads > 1 and x.shape[0] > 1 and kernel is None:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(run, range(x.shape[0])))
    else:
        for c in range(x.shape[0]):
            run(c)
    return out


def reference(x, N, f, p, seed=SEED, window=None, kernel=None):
    """The reference of one job: the C oracle for powers of two up to 65536 (oc.cpu_baseline_stretch from BASELINE_ABOVE
    output samples on, where it can run the job: default window, no kernel), the f64 twin everywhere else."""
    if N & (N - 1) == 0 and N <= 65536:
        n_out = oc.offline_output_len(x.shape[1], N, f, p)
        if x.shape[0] * n_out > BASELINE_ABOVE and window is None and kernel is None and p >= 1:
            return oc.cpu_baseline_stretch(x, N, f, 1.0, p, seed=seed, threads=THREADS, ch_first=0)
        return oracle_rows(x, N, f, p, seed, window, kernel)
    w = oc.hanning(N) if window is None else window
    return windowutil.oracle_with_window(x, N, f, p, w, seed, kernel=kernel)


def assert_every_channel(got, ref, N, what):
    """assert_parity (TOL, REG_TOL) and assert_blocks (half a window, 5e-6) on each channel by itself; returns the worst
    relative RMS and the worst block over the channels"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    worst_rms = worst_blk = 0.0
    for c in range(ref.shape[0]):
        err = assert_parity(got[c], ref[c], f"{what} ch={c}")
        worst_rms = max(worst_rms, err / max(windowutil.rms(ref[c]), 1e-30))
        if ref.shape[1] >= N // 2:
            worst_blk = max(worst_blk, assert_blocks(got[c], ref[c], N // 2, f"{what} ch={c}"))
    return worst_rms, worst_blk


# ------------------------------------------------------------------ the other paths
# unfused, chirp-z and long-window jobs: (name, N, f, p, kind); every one at OTHER_COUNTS channels (the long path: <= 17)
OTHER_COUNTS = (1, 4, 17, 65)
OTHER = [
    ("host_kernel", 1024, 4.0, 1, "host"),
    ("band", 4096, 2.0, 1, "band"),
    ("shift", 2048, 4.0, 1, "shift"),
    ("chirpz1000", 1000, 2.0, 1, None),
    ("chirpz24000", 24000, 2.0, 1, None),
    ("long131072", 131072, 2.0, 1, None),
]


def other_cases():
    out = []
    for name, N, f, p, kind in OTHER:
        for ch in OTHER_COUNTS:
            if N > 65536 and ch > 17:
                continue
            if N > 65536:
                L = 3 * N  # three windows' worth of input
            elif N & (N - 1):
                L = length_for(N, f, p, 6 if ch <= 4 else 3)  # (the f64 twin is the cost)
            else:
                L = length_for(N, f, p, max(4, min(24, 400 // ch)))
            out.append((name, kind, Case(name, N, f, p, ch, L, None)))
    return out

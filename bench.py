#!/usr/bin/env python3
"""Benchmark of the stretch hot path on MI355X.

A "step" is one whole pass of the hot path over one synthetic job already resident in HBM: BASELINE.json
configs[1] - stereo 44.1 kHz, window 16384, factor 8, pitch 1, L = 26 460 000 samples per channel (600 s):
51 652 hops -> 423 133 184 output samples per step. The metric names that FIXED job "@1/2/4/8 GPU", so at N > 1
the SAME job is cut by rocoder_amd.distributed.shard_plan into (channel, hop range) shards, one rank per GPU
(N = 2: a channel per GPU; N = 4, 8: half / quarter channels; every rank recomputes the single hop before its
range) - `"scaling": "strong"`, total work fixed. `value` = output samples of the whole job / max-rank time of
the timed steps, outputs left sharded in HBM, no data-path collective. N = 1 is the one-GPU job itself, so a
scaling sweep's N = 1 point equals the single-GPU bench line.

Launching: under torch.distributed.run (RANK / WORLD_SIZE in the environment) this process is one rank. Without
a launcher, `python bench.py --gpus N` (N > 1) starts its own ranks: BEFORE torch is imported or the GPU is
touched it starts N fresh child processes of this file with the environment a launcher would give them (RANK,
LOCAL_RANK, WORLD_SIZE, MASTER_ADDR=127.0.0.1, a free MASTER_PORT), relays rank 0's one JSON line and exits
with the first non-zero exit code of a rank (never exec). A box with fewer than N GPUs gets a JSON line with an
"error" field and a non-zero exit code, no traceback.

A plain run sets up, warms up (the W warm-up steps, then --preheat-s seconds of back-to-back steps for steady clocks),
times the --steps steps, writes the last step's output with --dump-outputs DIR and prints the line: the headline
fields and a roofline block priced on the engine's own event times of the timed steps. Everything below that takes
runs of its own (the extras, the post-measurement legs at N > 1, the box calibration kernel, the shader-clock
sampling, the CPU baselines) runs with --full only.

--dump-outputs DIR: DIR/output_sample.npy is a fixed seeded sample of the output of the last timed step, the
[channels, windows x window_out_len] f32 layout a caller of the path receives (at N > 1 gathered from the ranks'
shards onto rank 0), at the positions in DIR/output_positions.npy (f64, the same for every run and build).

With --full, after the main line is complete, under a watchdog (they can never cost the measurement), every leg
agreeing across ranks that its set-up succeeded before any timed collective is entered:
  config.weak        - ONE stereo job of N x L samples per channel cut the same way (per-GPU work that of N = 1)
  config.ref_1gpu    - the fixed job on every rank's own GPU alone, in this run (max over ranks)
  config.c5_sharded  - BASELINE configs[4] (8 channels, window 65536) cut over the same ranks
  config.concat      - the path's one optional collective: the RCCL concat of the shards on rank 0

The same JSON line carries (box calibration, clock under load and measured copy bandwidth with --full only)
  roofline     - the dominant kernel (the N = 16384 fused hop kernel) priced on SURVEY 8(d4)'s
                 algorithmic READ bytes 4*N per hop of rank 0's launch against the 8 TB/s HBM peak; its duration
                 is the MEDIAN of the per-launch HIP-event times the engine records around the kernel itself
                 (rc_engine_kernel_times), after >= 2 s of back-to-back launches (steady clocks);
                 also against the copy bandwidth measured on this very device, and the total-traffic,
                 compulsory and LDS-traffic figures of SURVEY 8 d3/d4;
  cpu_baseline - the CPU path of the reference algorithm written for speed (oracle/
                 rocoder_cpu_baseline.c, "port": the Rust reference cannot be built here), one DSP thread
                 as in src/stretcher_processor.rs:55-71, on a bounded sample of the same workload;
  cpu_baseline_all_cores - the same code on every core this process may use (rank 0, N = 1 only).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WINDOW = 16384
FACTOR = 8.0
PITCH = 1
CHANNELS = 2
SAMPLE_RATE = 44100
L_IN = 26_460_000
SEED = 0x5EED
CONCAT_TIMEOUT_S = float(os.environ.get("ROCODER_BENCH_CONCAT_TIMEOUT", "120"))  # watchdog of the post-measurement concat region (N > 1)
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec
LDS_READ_PEAK_GBS = 150e3    # MI355X_MICROARCH.md §LDS: ds_read_b64/b128, every CU streaming
LDS_WRITE_PEAK_GBS = 45e3    # same: 38-51 TB/s for ds_write_b32..b128
# rc_calib_valu on the reference box of profiles/README.md's normalised table (ns per packed-FMA wave instruction per
# SIMD, eight waves per SIMD): kernel_ms_normalised = kernel_ms * REF / this box's value
BOX_CALIB_REF_NS = 1.74
# reference shader clock for kernel_ms_at_ref_clock (MHz): what a typical box of the pool holds under the hop kernel
SCLK_REF_MHZ = 2100.0


def synth_on_device(torch, device, channels, length):
    """BASELINE.md §3 signal shape: 0.5 sin(2 pi 220 (c+1) t) + 0.05 u_c[t] (device-generated
    uniform noise; the parity tests use the documented splitmix64 stream, throughput does not
    depend on the noise bits)."""
    g = torch.Generator(device=device)
    g.manual_seed(0xC0DEC0DE)
    rows = []
    for c in range(channels):
        t = torch.arange(length, device=device, dtype=torch.float64) / SAMPLE_RATE
        s = 0.5 * torch.sin(2 * torch.pi * 220.0 * (c + 1) * t)
        del t
        u = torch.rand(length, device=device, generator=g, dtype=torch.float64) * 2 - 1
        rows.append((s + 0.05 * u).to(torch.float32))
        del s, u
    return torch.stack(rows).contiguous()


def pmc_counters(family_id, section=None):
    """Mean counter values per launch from the committed rocprofv3 PMC passes (profiles/r*_pmc_summary.txt, separate
    --pmc runs) of the kernel family `family_id` ("hop4=<hash>", "big4=<hash>": rc_kernel_id() hashes each family's
    sources at build time). Only a summary headed by exactly this id is quoted: counters of another build of the
    kernel say nothing about this one. `section`: the "## ..." block of a summary that holds several kernels.
    Returns (dict, relative path) or (None, reason)."""
    import glob
    import re

    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary.txt")), reverse=True):
        txt = open(path).read()
        kid = re.search(r"^#?\s*kernel_id:\s*(\S+)", txt, re.M)
        if not kid or kid.group(1) != family_id:
            continue
        if section is not None:
            parts = re.split(r"^## ", txt, flags=re.M)
            txt = next((p for p in parts if p.startswith(section)), "")
        g = {k: float(v) for k, v in re.findall(r"^(\w+)\s+n=\s*\d+\s+mean=([0-9.e+]+)", txt, re.M)}
        if g:
            return g, os.path.relpath(path, ROOT)
    return None, f"no profiles/r*_pmc_summary.txt headed by kernel_id {family_id}"


def pmc_traffic(family_id, section=None):
    """HBM-side bytes per launch: FETCH_SIZE, WRITE_SIZE in KiB. Per MI355X_MICROARCH.md (HBM / rocprofv3),
    FETCH_SIZE on gfx950 tallies 128-B read requests at 64 B, so the read side is doubled; WRITE_SIZE is exact."""
    g, src = pmc_counters(family_id, section)
    if g and "FETCH_SIZE" in g and "WRITE_SIZE" in g:
        return (2.0 * g["FETCH_SIZE"] + g["WRITE_SIZE"]) * 1024.0, src
    return None, src if g is None else f"{src}: no FETCH_SIZE / WRITE_SIZE"


def pmc_valu(family_id, section=None):
    """VALU occupancy and instruction count from the same summary (or None): SQ_ACTIVE_INST_VALU counts quad-cycles
    summed over all waves; 1024 SIMDs x the launch's busy cycles is what the chip offers. GRBM_GUI_ACTIVE is summed
    over the 8 XCDs."""
    g, src = pmc_counters(family_id, section)
    if g and {"SQ_ACTIVE_INST_VALU", "GRBM_GUI_ACTIVE", "SQ_INSTS_VALU"} <= set(g):
        simd_cycles = g["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0
        return {"valu_busy": round(4.0 * g["SQ_ACTIVE_INST_VALU"] / simd_cycles, 3),
                "valu_insts_per_launch": g["SQ_INSTS_VALU"], "source": src}
    return None


def family_id(full_id, family):
    """'hop4=<hash>' out of rc_kernel_id()'s 'hop4=<hash> big4=<hash> ...'."""
    import re

    m = re.search(r"\b%s=([0-9a-f]+)" % family, full_id)
    return f"{family}={m.group(1)}" if m else full_id


def cpu_baselines(all_cores=True):
    """Time oracle/rocoder_cpu_baseline.c (the reference's per-hop work with an optimised FFT) on
    bounded samples of the workload: one thread for all channels, then every core available."""
    import numpy as np

    from oracle import cbind as oc
    from oracle import oracle_np as onp

    def run(length, threads):
        x = np.stack([onp.synth_input(c, length) for c in range(CHANNELS)])
        t0 = time.perf_counter()
        y = oc.cpu_baseline_stretch(x, WINDOW, FACTOR, 1.0, PITCH, seed=SEED, threads=threads)
        dt = time.perf_counter() - t0
        return y.size, dt

    what = ("CPU path of rocoder's algorithm written for speed (oracle/rocoder_cpu_baseline.c: full N-point "
            "complex FFTs as src/fft.rs:59,69 with a radix-4 Stockham FFT, scalar libm hypotf/sincosf per bin "
            "as src/fft.rs:65-68), not the rocoder binary (no Rust toolchain)")
    n1, t1 = run(8_000_000, 1)
    one = {
        "value": round(n1 / t1 / 1e6, 3), "unit": "Msamples/s", "cores": 1, "kind": "port",
        "sample": f"stereo L=8000000/ch window={WINDOW} factor={FACTOR:g} -> {n1} output samples in {t1:.1f}s; "
                  f"one DSP thread for all channels like src/stretcher_processor.rs:55-71; {what}",
    }
    many = None
    if all_cores:
        cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        cores = max(1, min(cores, 64))
        length = 8_000_000 if cores < 8 else 24_000_000
        nm, tm = run(length, cores)
        many = {
            "value": round(nm / tm / 1e6, 3), "unit": "Msamples/s", "cores": cores, "kind": "port",
            "sample": f"stereo L={length}/ch -> {nm} output samples in {tm:.1f}s; OpenMP, one task per (channel, "
                      f"hop range), the hop before a range recomputed; host reports {os.cpu_count()} logical cores",
        }
    return one, many


METRIC = "output Msamples/s, 16384-win f=8 stereo (x CPU-realtime in config)"


def error_line(args, msg):
    """The bench contract's one JSON line when no measurement could be made (the caller exits non-zero)."""
    return {"metric": METRIC, "value": None, "unit": "Msamples/s", "n_gpus": args.gpus, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "error": str(msg)[:600]}


def gpus_on_this_box():
    """GPU agents the kernel driver lists (KFD topology nodes with SIMDs), read from sysfs: no HIP call, no torch
    import - this runs in the launcher process, which must never touch the GPU. None when the tree is not there."""
    import glob

    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not nodes:
        return None
    n = 0
    for path in nodes:
        try:
            for ln in open(path):
                k, _, v = ln.partition(" ")
                if k == "simd_count" and int(v) > 0:
                    n += 1
        except (OSError, ValueError):
            return None
    return n


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as FRESH child processes (never exec: this
    process has not touched the GPU and never will) with the environment torch.distributed.run would give them
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT), relay rank 0's one JSON line and return
    the first non-zero exit code of a rank."""
    import signal
    import socket
    import subprocess

    rehearsal = os.environ.get("ROCODER_BENCH_REHEARSAL") in ("1", "hang")
    have = gpus_on_this_box()
    if have is not None and have < args.gpus and not rehearsal:
        print(json.dumps(error_line(args, f"--gpus {args.gpus} but this box has {have} GPU(s) "
                                          "(ROCODER_BENCH_REHEARSAL=1 walks the N-rank code on one GPU over gloo)")))
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []

    def kill_all(sig=signal.SIGKILL):
        """Exactly the process groups started below (each rank is the leader of its own session)."""
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, sig)
                except (ProcessLookupError, PermissionError):
                    pass

    # the ranks live in their own sessions, so a SIGTERM / SIGINT / SIGHUP that reaches only this launcher
    # (an outer `timeout`, gpurun's limit, Ctrl-C) must be passed on - otherwise GPU-initialised ranks are orphaned
    # inside a collective. The launcher never touches the GPU, so handling signals here is safe.
    class _Stopped(Exception):
        pass

    def on_signal(signum, _frame):
        kill_all()
        raise _Stopped(signum)

    previous = {sg: signal.signal(sg, on_signal) for sg in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP)}

    def die_with_parent():
        # a SIGKILLed launcher runs no handler: the kernel then signals the rank itself (PR_SET_PDEATHSIG = 1)
        try:
            import ctypes

            ctypes.CDLL(None, use_errno=True).prctl(1, int(signal.SIGKILL), 0, 0, 0)
        except Exception:  # noqa: BLE001  (best effort; the handlers above cover the ordinary cases)
            pass

    for r in range(args.gpus):
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "1")
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr.fileno(),
                                      start_new_session=True, preexec_fn=die_with_parent))
    limit = float(os.environ.get("ROCODER_BENCH_SPAWN_TIMEOUT", "1500"))
    t_end = time.monotonic() + limit
    out = b""
    rc = 0

    def reap(grace):
        """Wait for the ranks; once one has failed the others get `grace` seconds (a rank that lost its peers sits in
        a collective for ever), then exactly the process groups started above are killed."""
        nonlocal rc
        deadline = None
        while any(p.poll() is None for p in procs):
            for p in procs:
                if p.poll() not in (None, 0) and rc == 0:
                    rc = p.returncode
                    deadline = time.monotonic() + grace
            now = time.monotonic()
            if (deadline is not None and now > deadline) or now > t_end:
                if rc == 0:
                    rc = 124
                kill_all()
                break
            time.sleep(0.1)
        for p in procs:
            p.wait()
            if p.returncode and rc == 0:
                rc = p.returncode

    import threading

    reaper = threading.Thread(target=reap, args=(30.0,), daemon=True)
    stopped = None
    try:
        reaper.start()
        out = procs[0].stdout.read()  # ends when rank 0 exits (or is killed by the reaper)
        reaper.join()
    except _Stopped as ex:
        stopped = int(ex.args[0])
    finally:
        kill_all()  # whatever ended the wait (a signal, KeyboardInterrupt, an error): no rank outlives the launcher
        for p in procs:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                pass
        for sg, h in previous.items():
            signal.signal(sg, h)
    if stopped is not None:
        print(json.dumps(error_line(args, f"launcher stopped by signal {stopped}; its {args.gpus} ranks were killed")),
              flush=True)
        return 128 + stopped
    line = None
    for ln in out.decode(errors="replace").splitlines():
        if ln.startswith("{"):
            line = ln
    if line is None:
        line = json.dumps(error_line(args, f"the {args.gpus} ranks printed no result line (exit code {rc})"))
        rc = rc or 1
    print(line, flush=True)
    return rc if 0 <= rc < 256 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preheat-s", type=float, default=2.0,
                    help="seconds of back-to-back launches before the timed steps (steady DVFS state)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: box calibration, clock under load, the extras, "
                         "the post-measurement legs (N > 1) and the CPU baselines (N = 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write a fixed seeded sample of the last timed step's output to DIR/*.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the copy microbench, the PCIe-inclusive runs and the post-measurement legs")
    args = ap.parse_args()
    if args.gpus < 1 or args.steps < 1:
        print(json.dumps(error_line(args, "--gpus and --steps must be >= 1")))
        return 2
    if args.gpus > 1 and "RANK" not in os.environ:
        return spawn_ranks(args, sys.argv[1:])  # torch not imported, GPU not touched in this process
    if "RANK" in os.environ and os.environ.get("ROCODER_BENCH_TEST_RANK_PIDDIR"):
        # test hook (tests/test_bench_host.py): a rank that only records its pid and waits - what a rank stuck in a
        # collective looks like to the launcher - so the launcher's signal handling can be tested without a GPU
        open(os.path.join(os.environ["ROCODER_BENCH_TEST_RANK_PIDDIR"], os.environ["RANK"]), "w").write(str(os.getpid()))
        time.sleep(600)
        return 0

    # Exactly ONE line on stdout (the JSON): RCCL / the HIP runtime print banners to fd 1, so park
    # the real stdout and point fd 1 at stderr until the result is ready.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))

    def say(obj):
        os.write(real_stdout, (json.dumps(obj) + "\n").encode())

    try:
        return worker(args, say)
    except SystemExit:
        raise
    except BaseException as ex:  # noqa: BLE001  (a failed measurement still owes the caller its one line)
        import traceback

        traceback.print_exc(file=sys.stderr)
        if rank == 0:
            say(error_line(args, f"{type(ex).__name__}: {ex}"))
        return 1


def worker(args, say):
    import threading

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # ROCODER_BENCH_REHEARSAL=1 (dev only, never the driver's command): every rank on cuda:0 over gloo, to walk the
    # N > 1 shard plan / timing code on a one-GPU box. RCCL refuses two ranks on one device, so the concat region
    # is skipped there; the JSON line is marked "rehearsal" and is not a measurement.
    rehearsal = os.environ.get("ROCODER_BENCH_REHEARSAL") in ("1", "hang")  # "hang": stall the concat region (watchdog test)
    if world != args.gpus:
        if rank == 0:
            say(error_line(args, f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world} rank(s)"))
        return 2
    n_dev = torch.cuda.device_count()  # (does not initialise the GPU)
    if n_dev < 1 or (n_dev < world and not rehearsal):
        if rank == 0:
            say(error_line(args, f"--gpus {world} but this box has {n_dev} GPU(s): the engine has no CPU fallback"))
        return 2
    dev_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist = None
    if world > 1 or "RANK" in os.environ:  # launched by torch.distributed.run: RCCL barrier/all-reduce
        import torch.distributed as dist

        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
    red_device = "cpu" if rehearsal else device

    def note(msg):  # progress on stderr in rehearsals only
        if rehearsal:
            print(f"[bench rank {rank}] {msg}", file=sys.stderr, flush=True)

    def max_over_ranks(v):
        if dist is None:
            return v
        tt = torch.tensor([v], dtype=torch.float64, device=red_device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    def all_ranks_ok(ok):
        """Every rank calls this once per leg, whatever happened in its own set-up: the timed collectives of a leg
        are entered by all ranks or by none (a rank that skips its barriers hangs the others)."""
        if dist is None:
            return ok
        tt = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=red_device)
        dist.all_reduce(tt, op=dist.ReduceOp.MIN)
        return float(tt.item()) > 0.5

    import rocoder_amd
    from rocoder_amd import _lib
    from rocoder_amd.distributed import engine_compute, shard_plan, stretch_sharded

    kernel_ids = _lib.lib().rc_kernel_id().decode()
    kernel_id = family_id(kernel_ids, "hop4")  # the bench kernel's family
    # ONE job for all ranks, the same at every N: same seed, same (replicated, device-generated) input
    eng = rocoder_amd.Engine(window_len=WINDOW, factor=FACTOR, pitch_multiple=PITCH,
                             sample_rate=SAMPLE_RATE, channels=CHANNELS, seed=SEED, device=dev_index)
    x = synth_on_device(torch, device, CHANNELS, L_IN)
    wout = eng.params.window_out_len
    n_out = eng.output_len(L_IN)          # per channel, whole job
    nwin = n_out // wout
    plan = shard_plan(CHANNELS, nwin, world)
    mine = [s for s in plan if s.rank == rank]
    compute = engine_compute(eng, x)
    # this rank's shards stay in its own HBM (no collective in the timed steps)
    bufs = {s: torch.empty((s.ch_count, s.win_count * wout), dtype=torch.float32, device=device) for s in mine}
    my_samples = sum(b.numel() for b in bufs.values())
    hops_mine = my_samples * PITCH // (WINDOW // 2)

    def step():
        for s in mine:
            compute(s, out=bufs[s])

    def barrier():
        torch.cuda.synchronize(device)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(device)

    # a real (non-default) stream: the engine launches its kernels on exactly this stream
    stream = torch.cuda.Stream(device)
    note(f"plan {[(s.rank, s.ch_first, s.ch_count, s.win_first, s.win_count) for s in plan]}")
    barrier()
    note("first barrier passed")
    # shader clock under THIS load, sampled by a host thread while the PRE-HEAT runs and stopped before the timed
    # steps (an SMI query every 50 ms has no place inside the measurement it annotates). Boxes of the pool
    # hold 2.0 - 2.15 GHz under the hop kernel; the calibration kernel below alone does not show it.
    clk_samples, clk_stop = [], threading.Event()

    def clk_sampler():
        while not clk_stop.is_set():
            try:
                clk_samples.append((time.perf_counter(), float(torch.cuda.clock_rate(dev_index))))
            except Exception:  # noqa: BLE001  (no SMI library on the box: the field stays null)
                return
            time.sleep(0.05)

    clk_thread = threading.Thread(target=clk_sampler, daemon=True)
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            step()
        # pre-heat: >= preheat_s of back-to-back launches so the timed steps run at the clock the chip
        # holds under this load (MI355X_MICROARCH.md, DVFS), not at the boost clock of an idle chip
        if args.full:
            clk_thread.start()
        t_heat = time.perf_counter()
        n_heat = 0
        while time.perf_counter() - t_heat < args.preheat_s:
            for _ in range(32):
                step()
            n_heat += 32
            stream.synchronize()
        t_heat_end = time.perf_counter()
        clk_stop.set()
        if args.full:
            clk_thread.join(timeout=2.0)
        for _ in range(8):  # the join above left the chip idle for a moment
            step()
        barrier()
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record(stream)
        for _ in range(args.steps):
            step()
        ev1.record(stream)
        barrier()
        dt = time.perf_counter() - t0
        # a kernel that gave up inside the timed region (seam wait expired: output incomplete) reports through the
        # engine's device error word; synchronize() raises it. A line measured on such a run must not be printed.
        eng.synchronize()
        step_event_ms = ev0.elapsed_time(ev1) / args.steps
        # per-launch kernel durations of exactly those steps (the engine brackets each kernel launch); a step of a
        # rank that holds several shards is the sum of its launches
        per_step = max(1, len(mine))
        k_steps = max(1, min(64 // per_step, args.steps))
        per_call = eng.kernel_times(k_steps * per_step)
        per_call = per_call[len(per_call) % per_step:]
        per_step_ms = [sum(per_call[i:i + per_step]) for i in range(0, len(per_call), per_step)]
        kernel_ms_median = statistics.median(per_step_ms)
        kernel_ms_mean = sum(per_step_ms) / len(per_step_ms)
    note(f"timed region done: {dt:.4f} s")
    clk_under_load = [c for (tt, c) in clk_samples if t_heat_end - 1.0 <= tt <= t_heat_end]
    sclk_mhz = statistics.median(clk_under_load) if clk_under_load else None
    dt = max_over_ranks(dt)

    if args.dump_outputs:
        def sum_over_ranks(t):
            if dist is None:
                return t
            t = t.to(red_device)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return t

        dump_outputs(torch, args.dump_outputs, rank, mine, bufs, wout, nwin, device, sum_over_ranks)

    # ---- box calibration: a fixed pure-VALU kernel on the same stream right after the timed
    # steps, ~50 ms, so that a slow box shows in the JSON line itself
    calib = None
    if args.full:
        try:
            import ctypes as C

            ms_l, ns_i = C.c_float(0), C.c_float(0)
            rc = _lib.lib().rc_calib_valu(dev_index, C.c_void_p(stream.cuda_stream), 48, C.byref(ms_l), C.byref(ns_i))
            if rc == 0:
                calib = {"ms_per_launch": float(ms_l.value), "ns_per_inst": float(ns_i.value)}
        except Exception as ex:  # noqa: BLE001
            calib = {"error": f"{type(ex).__name__}: {ex}"[:200]}

    extras = {}
    if args.full and not args.no_extras:
        with torch.cuda.stream(stream):
            # device copy microbench on this very GPU: the measured bandwidth the roofline is also priced on
            n_copy = 1 << 28  # 1 GiB of f32
            a = torch.empty(n_copy, dtype=torch.float32, device=device).normal_()
            b = torch.empty_like(a)
            for _ in range(3):
                b.copy_(a)
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record(stream)
            for _ in range(10):
                b.copy_(a)
            c1.record(stream)
            stream.synchronize()
            extras["copy_GBs"] = 2.0 * 4.0 * n_copy * 10 / (c0.elapsed_time(c1) * 1e-3) / 1e9
            del a, b
        if world == 1:
            extras["e2e_pcie"] = e2e_host(eng, x, torch)
            extras["other_configs"] = other_configs(torch, device, dev_index, stream, x, threading, kernel_ids)
            extras["shard_sizes"] = shard_sizes(torch, device, stream, eng, x, wout, nwin)
            extras["c5_share"] = c5_share(torch, device, dev_index, stream)
            extras["seam"] = seam_numbers()

    res = None
    if rank == 0:
        total_samples = float(n_out) * CHANNELS * args.steps
        value = total_samples / dt / 1e6
        H = WINDOW // 2
        step_len = eng.params.sample_step_len
        read_b, write_b = 4.0 * WINDOW, 4.0 * H / PITCH
        algo_bytes = hops_mine * read_b  # 4N read bytes per hop, one step's launches of this rank
        sec = kernel_ms_median * 1e-3
        achieved = algo_bytes / sec / 1e9
        traffic, traffic_src = pmc_traffic(kernel_id) if world == 1 else (None, "counters were taken on the N = 1 job")
        # LDS bytes per hop: four exchanges of N/2 complex points (8 B each), written once and read once
        lds_w = lds_r = 4 * (WINDOW // 2) * 8.0
        roof = {
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": traffic,
            "traffic_source": traffic_src,
            "kernel": f"N=16384 fused hop kernel ({kernel_id})" + ("" if world == 1 else f", rank 0's shard of the job ({hops_mine} hops)"),
            "kernel_id": kernel_id,
            "kernel_ms": round(kernel_ms_median, 4),
            "kernel_ms_mean": round(kernel_ms_mean, 4),
            "kernel_ms_min": round(min(per_step_ms), 4),
            "kernel_ms_max": round(max(per_step_ms), 4),
            "kernel_launches_timed": len(per_call),
            "step_event_ms": round(step_event_ms, 4),
            "preheat_launches": n_heat,
            "hops_per_s": round(hops_mine / sec, 1),
            "algorithmic_bytes_per_launch": algo_bytes,
            "frac_total_traffic": round(hops_mine * (read_b + write_b) / sec / 1e9 / HBM_PEAK_GBS, 4),
            "frac_compulsory": round(hops_mine * (4.0 * step_len + write_b) / sec / 1e9 / HBM_PEAK_GBS, 4),
            "lds_GBs": round(hops_mine * (lds_w + lds_r) / sec / 1e9, 1),
            "lds_time_frac": round(hops_mine * (lds_w / (LDS_WRITE_PEAK_GBS * 1e9) + lds_r / (LDS_READ_PEAK_GBS * 1e9)) / sec, 4),
            "note": "achieved = algorithmic READ bytes 4*N per hop (SURVEY §8 d4) / median per-launch kernel time; "
                    "frac_total_traffic adds the 4*H/p write bytes, frac_compulsory counts each input sample once "
                    "(4*step + 4*H/p); lds_time_frac = LDS exchange bytes priced at the measured LDS store/load rates "
                    "of MI355X_MICROARCH.md. The kernel is VALU-pipe bound (FFT butterflies + per-bin hash/sincos), "
                    "see DESIGN.md §5",
        }
        pv = pmc_valu(kernel_id) if world == 1 else None
        if pv:
            # the counter-backed ceiling of this kernel: its VALU instruction stream at full
            # occupancy of the VALU pipe - what the kernel would run at if nothing but VALU issue ever stalled
            roof["valu_busy"] = pv["valu_busy"]
            roof["valu_insts_per_hop"] = round(pv["valu_insts_per_launch"] / max(1, hops_mine), 1)
            roof["frac_at_full_valu_occupancy"] = round(achieved / HBM_PEAK_GBS / max(pv["valu_busy"], 1e-9), 4)
            roof["note"] += (f". CEILING: PMC ({pv['source']}) has the VALU pipes {pv['valu_busy']:.0%} busy for "
                             f"{roof['valu_insts_per_hop']:.0f} VALU instructions per hop; the same instruction stream "
                             f"with the pipes 100 % busy would reach frac {roof['frac_at_full_valu_occupancy']} - the "
                             "0.40 target needs fewer VALU cycles per hop (the frozen phase spec's hash + sincos, the "
                             "butterflies at 1.5 packed FMAs per point and stage), not more overlap")
        roof["counters_box"] = "builder"  # traffic / valu_busy come from the committed PMC summary, not from this box
        if calib and "ns_per_inst" in calib:
            # kernel_ms scaled to the reference box speed: boxes of the pool differ by +-3..5 % on the same binary
            roof["box_calib_ns"] = round(calib["ns_per_inst"], 4)
            roof["box_calib_ms_per_launch"] = round(calib["ms_per_launch"], 4)
            roof["box_calib_ref_ns"] = BOX_CALIB_REF_NS
            roof["kernel_ms_normalised"] = round(kernel_ms_median * BOX_CALIB_REF_NS / calib["ns_per_inst"], 4)
            roof["frac_normalised"] = round(achieved / HBM_PEAK_GBS * calib["ns_per_inst"] / BOX_CALIB_REF_NS, 4)
        elif calib:
            roof["box_calib_error"] = calib.get("error")
        # the shader clock this box held under the load of the hop kernel (median of the SMI samples of the last second
        # of the pre-heat) and the kernel time scaled to the reference clock
        roof["sclk_mhz_under_load"] = sclk_mhz
        roof["sclk_samples"] = len(clk_under_load)
        if sclk_mhz:
            roof["sclk_ref_mhz"] = SCLK_REF_MHZ
            roof["kernel_ms_at_ref_clock"] = round(kernel_ms_median * sclk_mhz / SCLK_REF_MHZ, 4)
            roof["frac_at_ref_clock"] = round(achieved / HBM_PEAK_GBS * SCLK_REF_MHZ / sclk_mhz, 4)
        if "copy_GBs" in extras:
            roof["measured_copy_GBs"] = round(extras["copy_GBs"], 1)
            roof["frac_measured_peak"] = round(achieved / extras["copy_GBs"], 4)
        res = {
            "metric": METRIC,
            "value": round(value, 1),
            "unit": "Msamples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic" if not rehearsal else "synthetic (REHEARSAL: all ranks on one GPU over gloo, not a measurement)",
            "config": {
                "workload": f"BASELINE configs[1]: stereo 44.1 kHz, window=16384, factor=8, pitch=1, "
                            f"L={L_IN}/ch (the same fixed job at every N), inputs resident in HBM; signal = BASELINE.md "
                            "§3's 0.5 sin(2 pi 220 (c+1) t) + 0.05 u_c[t] with u_c from torch.rand on the device "
                            "(seed 0xC0DEC0DE), NOT SURVEY d2's splitmix64 stream (the parity tests use that one; "
                            "throughput does not depend on the noise bits)",
                "hops_per_step": n_out * CHANNELS * PITCH // H,
                "hops_per_rank": hops_mine,
                "output_samples_per_step": n_out * CHANNELS,
                "x_realtime": round(value * 1e6 / CHANNELS / SAMPLE_RATE, 1),
                "kernel_ids": kernel_ids,
                "parallelism": (f"{world} rank(s): one job cut into (channel, hop range) shards by shard_plan "
                                f"{[(s.rank, s.ch_first, s.ch_count, s.win_first, s.win_count) for s in plan]}, "
                                "outputs left sharded in HBM, no data-path collective; one kernel launch per shard and "
                                "step, wall time between barriers, max over ranks"),
            },
            "roofline": roof,
        }
        if "e2e_pcie" in extras:
            res["config"]["e2e_pcie"] = extras["e2e_pcie"]
            best = extras["e2e_pcie"].get("pinned_Msamples_s") or extras["e2e_pcie"].get("pageable_reused_Msamples_s")
            if best:
                res["config"]["e2e_pcie_Msamples_s"] = best
        if "shard_sizes" in extras:
            res["config"]["shard_sizes_on_one_gpu"] = extras["shard_sizes"]
        if "other_configs" in extras:  # not the metric's config: BASELINE configs[2..4] on this one GPU
            res["config"]["other_configs"] = extras["other_configs"]
        if "c5_share" in extras:
            res["config"]["c5_share_on_one_gpu"] = extras["c5_share"]
        if "seam" in extras:
            res["config"]["streaming_seam"] = extras["seam"].get("streaming_seam")
            res["config"]["live_latency_us"] = extras["seam"].get("live_latency_us")
        if args.full and world == 1 and not args.no_cpu_baseline:
            one, many = cpu_baselines()
            res["cpu_baseline"] = one
            res["config"]["x_cpu"] = round(value / one["value"], 1)
            if many:
                res["cpu_baseline_all_cores"] = many
                res["config"]["x_cpu_all_cores"] = round(value / many["value"], 1)

    # ---- post-measurement legs (N > 1 only): the main line is complete; everything below runs under a watchdog that
    # prints the line and exits non-zero if a collective hangs, and every leg agrees across the ranks on its set-up
    # before it enters a timed collective.
    lock = threading.Lock()
    emitted = [False]
    legs = {}

    def emit():
        with lock:
            if rank == 0 and not emitted[0]:
                res["config"].update(legs)
                say(res)
            emitted[0] = True

    def watchdog():
        # The main line is printed (it is complete), then the process exits NON-ZERO: a collective that hung on
        # GPU-initialised processes must be visible to the launcher, not look like a clean run.
        with lock:
            if rank == 0 and not emitted[0]:
                res["config"].update(legs)
                res["config"]["legs_error"] = (f"the post-measurement legs did not finish within {CONCAT_TIMEOUT_S} s "
                                               f"(finished: {sorted(legs)}); the main line is unaffected")
                say(res)
            emitted[0] = True
        os._exit(3)

    timer = threading.Timer(CONCAT_TIMEOUT_S, watchdog)
    timer.daemon = True
    broken = [False]

    def leg(name, setup, body):
        """setup() -> state on every rank (local work only: allocation, engines); then ONE agreement collective; then
        body(state) -> dict with the leg's timed collectives, entered by every rank or by none."""
        if broken[0]:
            return
        state, err = None, None
        try:
            if rehearsal and os.environ.get("ROCODER_BENCH_REHEARSAL_FAIL") == f"{name}:{rank}":
                raise RuntimeError("rehearsal: injected set-up failure")  # (exercises the agreement below; dev only)
            with torch.cuda.stream(stream):
                state = setup()
                torch.cuda.synchronize(device)
        except Exception as ex:  # noqa: BLE001
            err = f"{type(ex).__name__}: {ex}"[:300]
        if not all_ranks_ok(err is None):
            legs[name] = {"error": err or "set-up failed on another rank; leg skipped on all ranks"}
            note(f"{name}: skipped ({legs[name]['error']})")
            return
        try:
            with torch.cuda.stream(stream):
                legs[name] = body(state)
        except Exception as ex:  # noqa: BLE001
            # past the agreement point: the other ranks may be inside a barrier this rank will never reach. No further
            # collective is entered here; the watchdog of the ranks left behind ends the job non-zero.
            legs[name] = {"error": f"{type(ex).__name__}: {ex}"[:300]}
            broken[0] = True
        note(f"{name}: {legs.get(name)}")

    def timed(fn, k, warm=3):
        for _ in range(warm):
            fn()
        barrier()
        t = time.perf_counter()
        for _ in range(k):
            fn()
        barrier()
        return max_over_ranks(time.perf_counter() - t) / k

    if world > 1 and args.full and not args.no_extras:
        timer.start()
        ks = max(args.steps, 20)

        # (1) the fixed job on ONE GPU, in this run: every rank runs the whole job on its own GPU
        def ref_setup():
            return torch.empty((CHANNELS, n_out), dtype=torch.float32, device=device)

        def ref_body(full_f):
            one_f = shard_plan(CHANNELS, nwin, 1)
            t_1 = timed(lambda: [compute(s, out=full_f[s.ch_first:s.ch_first + s.ch_count]) for s in one_f], ks)
            t_n = dt / args.steps
            return {"workload": "the fixed job on every rank's own GPU alone (max over ranks), same run",
                    "steps": ks, "ms_per_step_1gpu": round(t_1 * 1e3, 4),
                    "value_1gpu_Msamples_s": round(float(n_out) * CHANNELS / t_1 / 1e6, 1),
                    "efficiency_vs_1gpu": round(t_1 / (world * t_n), 4)}

        leg("ref_1gpu", ref_setup, ref_body)

        # (2) weak scaling: ONE stereo job of N x L samples per channel, per-GPU work that of N = 1
        def weak_setup():
            xw = synth_on_device(torch, device, CHANNELS, L_IN * world)
            n_out_w = eng.output_len(L_IN * world)
            plan_w = shard_plan(CHANNELS, n_out_w // wout, world)
            mine_w = [s for s in plan_w if s.rank == rank]
            bufs_w = {s: torch.empty((s.ch_count, s.win_count * wout), dtype=torch.float32, device=device) for s in mine_w}
            return xw, n_out_w, plan_w, mine_w, bufs_w, engine_compute(eng, xw)

        def weak_body(st):
            xw, n_out_w, plan_w, mine_w, bufs_w, comp_w = st
            t_w = timed(lambda: [comp_w(s, out=bufs_w[s]) for s in mine_w], ks)
            return {"scaling": "weak",
                    "workload": f"one stereo job of L={L_IN * world}/ch ({world} x {L_IN}) cut over {world} rank(s)",
                    "steps": ks, "ms_per_step": round(t_w * 1e3, 4),
                    "value_Msamples_s": round(float(n_out_w) * CHANNELS / t_w / 1e6, 1),
                    "hops_per_rank": sum(s.ch_count * s.win_count for s in mine_w) * eng.params.hops_per_window,
                    "plan": [(s.rank, s.ch_first, s.ch_count, s.win_first, s.win_count) for s in plan_w]}

        leg("weak", weak_setup, weak_body)

        # (3) BASELINE configs[4] (C5: 8 channels, window 65536, factor 32, L = 5 292 000 per channel) cut over the
        # ranks by the same shard_plan (8 ranks: one channel per GPU, no halo). Not the metric's config.
        C5 = dict(window=65536, factor=32.0, channels=8, length=5_292_000)

        def c5_setup():
            eng5 = rocoder_amd.Engine(window_len=C5["window"], factor=C5["factor"], pitch_multiple=1,
                                      sample_rate=SAMPLE_RATE, channels=C5["channels"], seed=SEED, device=dev_index)
            x5 = synth_on_device(torch, device, C5["channels"], C5["length"])
            wout5 = eng5.params.window_out_len
            n_out5 = eng5.output_len(C5["length"])
            plan5 = shard_plan(C5["channels"], n_out5 // wout5, world)
            mine5 = [s for s in plan5 if s.rank == rank]
            bufs5 = {s: torch.empty((s.ch_count, s.win_count * wout5), dtype=torch.float32, device=device) for s in mine5}
            return eng5, x5, n_out5, plan5, mine5, bufs5, engine_compute(eng5, x5)

        def c5_body(st):
            eng5, x5, n_out5, plan5, mine5, bufs5, comp5 = st
            k5 = max(3, min(10, args.steps))
            t5 = timed(lambda: [comp5(s, out=bufs5[s]) for s in mine5], k5)
            r = {"workload": "BASELINE configs[4]: 8 ch, window=65536, factor=32, L=5292000/ch, one job cut by shard_plan",
                 "steps": k5, "ms_per_step": round(t5 * 1e3, 4),
                 "value_Msamples_s": round(float(n_out5) * C5["channels"] / t5 / 1e6, 1),
                 "plan": [(s.rank, s.ch_first, s.ch_count, s.win_first, s.win_count) for s in plan5]}
            eng5.close()
            return r

        leg("c5_sharded", c5_setup, c5_body)

        # (4) the one collective of the path: concat of the shards on rank 0, straight into the final layout
        # (stretch_sharded). Timed as compute + concat per step.
        if rehearsal:
            legs["concat"] = {"skipped": "rehearsal: gloo has no device-to-device send/recv"}
            if os.environ.get("ROCODER_BENCH_REHEARSAL") == "hang":
                del legs["concat"]
                time.sleep(1e6)
        else:
            def concat_setup():
                return torch.empty((CHANNELS, n_out), dtype=torch.float32, device=device) if rank == 0 else None

            def concat_body(full):
                k2 = max(2, min(5, args.steps))
                tc = timed(lambda: stretch_sharded(compute, CHANNELS, nwin, wout, dst=0, full=full), k2, warm=1)
                return {"steps": k2, "ms_per_step_with_concat": round(tc * 1e3, 4),
                        "value_with_concat": round(float(n_out) * CHANNELS / tc / 1e6, 1),
                        "bytes_moved_to_rank0": int((n_out * CHANNELS - (my_samples if rank == 0 else 0)) * 4),
                        "how": "grouped RCCL send/recv of each shard into its view of the final [channels, n_out] "
                               "tensor on rank 0 (root-inbound-bound); no pad, no staging copy"}

            leg("concat", concat_setup, concat_body)
    emit()
    if broken[0]:
        os._exit(4)  # a leg failed past its agreement point: no further collective, the main line is out
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    timer.cancel()
    return 0


DUMP_PER_CHANNEL = 1 << 21  # sampled output positions per channel: 2 x 8 MiB of f32 values + 16 MiB of positions
DUMP_SEED = 0xD0D0


def dump_outputs(torch, out_dir, rank, mine, bufs, wout, nwin, device, sum_over_ranks):
    """--dump-outputs: the output of the last timed step at a fixed seeded sample of positions of the
    [CHANNELS, nwin * wout] layout, the same positions in every channel. Each rank fills the positions its shards hold;
    the ranks' parts are summed (each position lies in exactly one shard, the others add zeros) and rank 0 writes
    output_sample.npy (f32 [CHANNELS, k]) and output_positions.npy (f64 [k])."""
    import numpy as np

    n = nwin * wout
    k = min(DUMP_PER_CHANNEL, n)
    pos = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=k, replace=False))
    pos_d = torch.from_numpy(pos).to(device)
    vals = torch.zeros((CHANNELS, k), dtype=torch.float32, device=device)
    for s in mine:
        lo, hi = s.win_first * wout, (s.win_first + s.win_count) * wout
        a, b = int(np.searchsorted(pos, lo)), int(np.searchsorted(pos, hi))
        if b > a:
            vals[s.ch_first:s.ch_first + s.ch_count, a:b] = bufs[s][:, pos_d[a:b] - lo]
    vals = sum_over_ranks(vals)
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, "output_sample.npy"), vals.cpu().numpy())
        np.save(os.path.join(out_dir, "output_positions.npy"), pos.astype(np.float64))


def e2e_host(eng, x, torch):
    """PCIe-inclusive C2 (host arrays in and out through rc_engine_stretch_host; never `value`): input
    upload, compute and output download as one pipelined call. Three forms of the same job, median of 3 calls each:
      pinned           rows from rc_host_alloc on both sides (DMA straight from / into the caller's memory)
      pageable_reused  ordinary numpy arrays, the output array allocated once and reused (its pages exist)
      pageable_fresh   a new output array per call (np.empty inside the call: every page is faulted in on the way; the
                       previous result is released before the clock starts)"""
    import numpy as np

    import rocoder_amd

    xh = x.cpu().numpy()
    n_out = eng.output_len(xh.shape[1])
    total = float(n_out) * xh.shape[0]
    r = {"what": "rc_engine_stretch_host on the C2 job, host arrays in and out, wall time of the blocking call",
         "pcie_bound_Msamples_s_at_54GBs": round(54e9 / 4 / 1e6, 0)}

    def med(fn, reps=3):
        fn()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return statistics.median(ts)

    try:
        xp = rocoder_amd.pinned_empty(xh.shape)
        xp[:] = xh
        yp = rocoder_amd.pinned_empty((xh.shape[0], n_out))
        t = med(lambda: eng.stretch_host(xp, out=yp))
        r["pinned_Msamples_s"] = round(total / t / 1e6, 1)
        r["pinned_ms"] = round(t * 1e3, 2)
        del xp, yp
    except Exception as ex:  # noqa: BLE001
        r["pinned_error"] = f"{type(ex).__name__}: {ex}"[:200]
    try:
        yh = np.empty((xh.shape[0], n_out), np.float32)
        t = med(lambda: eng.stretch_host(xh, out=yh))
        r["pageable_reused_Msamples_s"] = round(total / t / 1e6, 1)
        del yh
        # a new output array per call; the previous one is released BEFORE the clock starts (unmapping 1.7 GB of touched
        # pages costs tens of milliseconds and is not part of the call)
        ts, keep = [], eng.stretch_host(xh)
        for _ in range(2):
            keep = None
            t0 = time.perf_counter()
            keep = eng.stretch_host(xh)
            ts.append(time.perf_counter() - t0)
        del keep
        r["pageable_fresh_Msamples_s"] = round(total / statistics.median(ts) / 1e6, 1)
    except Exception as ex:  # noqa: BLE001
        r["pageable_error"] = f"{type(ex).__name__}: {ex}"[:200]
    return r


def shard_sizes(torch, device, stream, eng, x, wout, nwin):
    """What ONE rank of an N-way cut of the fixed job costs, measured on this one GPU (N = 2, 4, 8: rank 0's shard
    of shard_plan, the launch bench.py --gpus N times on every rank). It is the per-rank compute of the strong-scaling
    run - run length quantisation, the recomputed hop, launch overhead at 6 456 hops per rank - and says nothing about
    a node's fabric (the data path has no collective). NOT a multi-GPU measurement."""
    from rocoder_amd.distributed import engine_compute, shard_plan

    out = {}
    try:
        comp = engine_compute(eng, x)
        with torch.cuda.stream(stream):
            for n in (2, 4, 8):
                mine = [s for s in shard_plan(CHANNELS, nwin, n) if s.rank == 0]
                bufs = {s: torch.empty((s.ch_count, s.win_count * wout), dtype=torch.float32, device=device) for s in mine}
                for _ in range(50):
                    for s in mine:
                        comp(s, out=bufs[s])
                stream.synchronize()
                k = 200
                t = time.perf_counter()
                for _ in range(k):
                    for s in mine:
                        comp(s, out=bufs[s])
                stream.synchronize()
                wall = (time.perf_counter() - t) / k
                kms = statistics.median(eng.kernel_times(32))
                hops = sum(s.ch_count * s.win_count for s in mine) * eng.params.hops_per_window
                out[f"1_of_{n}"] = {"hops": hops, "kernel_ms": round(kms, 4), "step_wall_ms": round(wall * 1e3, 4),
                                    "frac_hbm_read": round(hops * 4.0 * WINDOW / kms / 1e6 / HBM_PEAK_GBS, 4),
                                    "job_Msamples_s_if_all_ranks_alike": round(float(nwin) * wout * CHANNELS / wall / 1e6, 1)}
                del bufs
    except Exception as ex:  # noqa: BLE001
        out["error"] = f"{type(ex).__name__}: {ex}"[:300]
    return out


def c5_share(torch, device, dev_index, stream):
    """BASELINE configs[4] is DEFINED as an 8-GPU job (8 channels, window 65536, factor 32, one channel per GPU): what one
    rank of it costs, measured on this one GPU - rank 0's shard of shard_plan(8 channels, n windows, 8 ranks) = one whole
    channel (5 106 hops over the 256 one-per-CU workgroups of big5_kernel), through the launch `bench.py --gpus 8` issues
    per rank (config.c5_sharded). NOT a multi-GPU measurement (the data path has no collective)."""
    import rocoder_amd
    from rocoder_amd.distributed import engine_compute, shard_plan

    out = {}
    try:
        with torch.cuda.stream(stream):
            x5 = synth_on_device(torch, device, 8, 5_292_000)
            e5 = rocoder_amd.Engine(window_len=65536, factor=32.0, sample_rate=SAMPLE_RATE, channels=8, seed=SEED, device=dev_index)
            wout5, nwin5 = e5.params.window_out_len, e5.output_len(x5.shape[1]) // e5.params.window_out_len
            comp = engine_compute(e5, x5)
            whole = torch.empty((8, nwin5 * wout5), dtype=torch.float32, device=device)
            for _ in range(3):
                e5.stretch_tensor(x5, out=whole)
            stream.synchronize()
            for _ in range(12):
                e5.stretch_tensor(x5, out=whole)
            stream.synchronize()
            whole_ms = statistics.median(e5.kernel_times(10))
            del whole
            mine = [sh for sh in shard_plan(8, nwin5, 8) if sh.rank == 0]
            bufs = {sh: torch.empty((sh.ch_count, sh.win_count * wout5), dtype=torch.float32, device=device) for sh in mine}
            for _ in range(20):
                for sh in mine:
                    comp(sh, out=bufs[sh])
            stream.synchronize()
            k = 100
            t = time.perf_counter()
            for _ in range(k):
                for sh in mine:
                    comp(sh, out=bufs[sh])
            stream.synchronize()
            wall = (time.perf_counter() - t) / k
            kms = statistics.median(e5.kernel_times(32))
            hops = sum(sh.ch_count * sh.win_count for sh in mine) * e5.params.hops_per_window
            out = {"shards_of_rank0": [(sh.ch_first, sh.ch_count, sh.win_first, sh.win_count) for sh in mine],
                   "hops": hops, "kernel_ms": round(kms, 4), "step_wall_ms": round(wall * 1e3, 4),
                   "frac_hbm_read": round(hops * 4.0 * 65536 / kms / 1e6 / HBM_PEAK_GBS, 4),
                   "whole_job_kernel_ms_on_this_gpu": round(whole_ms, 4),
                   "percent_of_linear": round(100.0 * whole_ms / 8.0 / kms, 1),
                   "job_Msamples_s_if_all_ranks_alike": round(float(nwin5) * wout5 * 8 / wall / 1e6, 1)}
            e5.close()
            del bufs, x5
    except Exception as ex:  # noqa: BLE001
        out["error"] = f"{type(ex).__name__}: {ex}"[:300]
    return out


def seam_numbers():
    """The literal drop-in seam (rc_engine_push_input / close_input / next_window(_view): what INTEGRATION.md tells a
    maintainer to bind), driven from C in the processor's order (tools/seam_bench.c, built by build() into
    rocoder_amd/bin/libseam_bench.so) on the engine library this process has loaded:
      streaming_seam  - the C2 job as a CLOSED stereo job (`-o` mode), output samples/s of the hand-out loop with the
                        copying call and with the pointer-returning one; host buffers, PCIe inside (never `value`);
      live_latency_us - OPEN channels (live mode), window 16384, stereo: each round pushes the input one output window
                        consumes to every channel and asks every channel for its window; first = until the first
                        next_window returns, round = until all have; --buffer 1 s and 0.1 s."""
    import ctypes as C

    from rocoder_amd import _lib

    out = {}
    try:
        so = os.path.join(ROOT, "rocoder_amd", "bin", "libseam_bench.so")
        sb = C.CDLL(so)
        sb.seam_bench_closed.argtypes = [C.c_char_p, C.c_uint32, C.c_float, C.c_uint32, C.c_size_t, C.c_int,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        sb.seam_bench_live.argtypes = [C.c_char_p, C.c_uint32, C.c_float, C.c_uint32, C.c_float, C.c_uint32,
                                       C.POINTER(C.c_double)]
        lib = _lib.LIB_PATH.encode()
        # what `numactl --cpunodebind` does for a host program: the hand-out thread (this one) on the CPUs next to the GPU,
        # for the seam legs only (the engine prefers that node's memory for its pinned blocks by itself)
        affinity = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None
        node = sb.seam_bench_pin_near_gpu()
        seam = {}
        for name, view in (("copy", 0), ("view", 1)):
            best, push = 0.0, 0.0
            for _ in range(2):
                sps, pms, n = C.c_double(0), C.c_double(0), C.c_uint64(0)
                rc = sb.seam_bench_closed(lib, WINDOW, FACTOR, CHANNELS, L_IN, view, C.byref(sps), C.byref(pms), C.byref(n))
                if rc != 0:
                    raise RuntimeError(f"seam_bench_closed({name}) returned {rc}")
                if sps.value > best:
                    best, push = sps.value, pms.value
            seam[f"{name}_Msamples_s"] = round(best / 1e6, 1)
            seam[f"{name}_push_ms"] = round(push, 1)
        seam["job"] = (f"closed stereo job, L={L_IN}/ch, window {WINDOW}, factor {FACTOR:g}; round-robin over the channels; best of 2; "
                       f"calling thread on the CPUs of the GPU's NUMA node ({node})" + ("" if node >= 0 else ": not found, unpinned"))
        out["streaming_seam"] = seam
        live = {}
        for buf in (1.0, 0.1):
            o = (C.c_double * 6)()
            rc = sb.seam_bench_live(lib, WINDOW, FACTOR, CHANNELS, buf, 1000, o)
            if rc != 0:
                raise RuntimeError(f"seam_bench_live({buf}) returned {rc}")
            live[f"buffer_{buf:g}s"] = {"first_window_median": round(o[0], 1), "first_window_p99": round(o[1], 1),
                                       "first_window_mean": round(o[2], 1), "first_window_max": round(o[3], 1),
                                       "round_median": round(o[4], 1), "round_p99": round(o[5], 1)}
        live["what"] = ("open stereo channels, window 16384, factor 8: push of one window's input advance (2048 samples) per "
                        "channel -> rc_engine_next_window returns; 1000 rounds after 8 untimed ones")
        out["live_latency_us"] = live
        if affinity is not None:
            os.sched_setaffinity(0, affinity)
    except Exception as ex:  # noqa: BLE001
        out.setdefault("streaming_seam", {})["error"] = f"{type(ex).__name__}: {ex}"[:300]
    return out


def other_configs(torch, device, dev_index, stream, x, threading, kernel_ids=""):
    """The other single-GPU BASELINE configs, timed the same way (pre-heated, median of the engine's per-launch
    event times) so that the driver's own run carries them: C3 (pitch 3) and C5 (8 ch, window 65536, f = 32)."""
    import rocoder_amd

    other = {}
    try:
        with torch.cuda.stream(stream):
            def timed_config(xx, **kw):
                e2 = rocoder_amd.Engine(sample_rate=SAMPLE_RATE, channels=xx.shape[0], seed=SEED, device=dev_index, **kw)
                o2 = torch.empty((xx.shape[0], e2.output_len(xx.shape[1])), dtype=torch.float32, device=device)
                e2.stretch_tensor(xx, out=o2)
                clk2, stop2 = [], threading.Event()

                def samp():
                    while not stop2.is_set():
                        try:
                            clk2.append(float(torch.cuda.clock_rate(dev_index)))
                        except Exception:  # noqa: BLE001
                            return
                        time.sleep(0.05)

                t2 = threading.Thread(target=samp, daemon=True)
                t2.start()
                th = time.perf_counter()
                while time.perf_counter() - th < 0.7:
                    for _ in range(4):
                        e2.stretch_tensor(xx, out=o2)
                    stream.synchronize()
                stop2.set()
                t2.join(timeout=2.0)
                for _ in range(40):
                    e2.stretch_tensor(xx, out=o2)
                stream.synchronize()
                ms2 = statistics.median(e2.kernel_times(10))
                _, hops2, _ = e2.last_kernel_stats()
                nwin = kw["window_len"]
                r2 = {"kernel_ms": round(ms2, 4), "hops": int(hops2),
                      "out_Msamples_s": round(o2.numel() / ms2 / 1e3, 1),
                      "frac_hbm_read": round(hops2 * 4.0 * nwin / ms2 / 1e6 / HBM_PEAK_GBS, 4),
                      "sclk_mhz_under_load": round(statistics.median(clk2), 1) if clk2 else None}
                e2.close()
                del o2
                return r2

            other["C3_pitch3"] = timed_config(x, window_len=WINDOW, factor=FACTOR, pitch_multiple=3)
            x5 = synth_on_device(torch, device, 8, 5_292_000)
            c5 = timed_config(x5, window_len=65536, factor=32.0)
            # HBM traffic / VALU occupancy of big4_kernel<64> from the committed C5 counter passes of THIS kernel build
            fam = family_id(kernel_ids, "big4")
            c5["kernel_id"] = fam
            c5["traffic"], c5["traffic_source"] = pmc_traffic(fam, "R64")
            pv = pmc_valu(fam, "R64")
            if pv:
                c5["valu_busy"] = pv["valu_busy"]
                c5["valu_insts_per_hop"] = round(pv["valu_insts_per_launch"] / max(1, c5["hops"]), 1)
            other["C5_8ch_window65536_f32"] = c5
            del x5
    except Exception as ex:  # noqa: BLE001
        other["error"] = f"{type(ex).__name__}: {ex}"[:300]
    try:
        other["C4_host_kernel_x2"] = c4_config(torch, device, dev_index, stream, x)
    except Exception as ex:  # noqa: BLE001
        other["C4_host_kernel_x2"] = {"error": f"{type(ex).__name__}: {ex}"[:300]}
    return other


def c4_config(torch, device, dev_index, stream, x):
    """BASELINE configs[3] at its own size: the C2 job with the README's x2.0 apply() (README.md:121-128) as a compiled
    C-ABI host kernel, two kernel threads. Input and output resident in HBM as for `value`; every hop's N-bin spectrum
    crosses PCIe both ways (2 x 6.77 GB) and passes through the host callback: PCIe- and callback-bound, not on the
    roofline line."""
    import shutil
    import subprocess
    import tempfile

    import rocoder_amd

    tmp = tempfile.mkdtemp(prefix="rocoder_c4_")
    try:
        src, so = os.path.join(tmp, "gain2.c"), os.path.join(tmp, "libgain2.so")
        with open(src, "w") as fh:
            fh.write("#include <stddef.h>\n#include <stdint.h>\n"
                     "int apply(uint64_t t, const float *in, float *out, size_t n, void *u) {\n"
                     "    (void)t; (void)u;\n    for (size_t i = 0; i < 2 * n; ++i) out[i] = in[i] * 2.0f;\n    return 0;\n}\n")
        subprocess.run(["gcc", "-O3", "-shared", "-fPIC", "-o", so, src], check=True, timeout=120)
        k = rocoder_amd.load_kernel_library(so)
        with torch.cuda.stream(stream):
            e4 = rocoder_amd.Engine(window_len=WINDOW, factor=FACTOR, pitch_multiple=PITCH, sample_rate=SAMPLE_RATE,
                                    channels=x.shape[0], seed=SEED, device=dev_index, kernel=k, kernel_threads=2)
            o4 = torch.empty((x.shape[0], e4.output_len(x.shape[1])), dtype=torch.float32, device=device)
            e4.stretch_tensor(x[:, :1_000_000].contiguous(), out=o4)  # pinned sets, scratch
            stream.synchronize()
            ts = []
            for _ in range(2):
                t0 = time.perf_counter()
                e4.stretch_tensor(x, out=o4)
                stream.synchronize()
                e4.synchronize()
                ts.append(time.perf_counter() - t0)
            _, hops4, _ = e4.last_kernel_stats()
            r = {"ms": round(min(ts) * 1e3, 1), "hops": int(hops4), "kernel_threads": 2,
                 "out_Msamples_s": round(o4.numel() / min(ts) / 1e6, 1),
                 "spectrum_GB_each_way": round(hops4 * WINDOW * 8 / 1e9, 2),
                 "note": "device-resident in / out; spectra over PCIe both ways + host apply(); best of 2 calls"}
            e4.close()
            del o4
        return r
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())

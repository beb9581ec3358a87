"""Headline benchmark: OFDM symbols/s through the fused GPU modem path.

Metric (BASELINE.json): OFDM symbols/sec at N_FFT=1024, 64-QAM.  Workload = BASELINE config
(b): N_FFT=1024, 64-QAM, flat channel (flat_fading.npy, cp=0), no equaliser, AWGN at 24 dB
(BER ~1e-4), Philox bits and noise generated on the device, in complex128 -- the reference's
arithmetic (np.fft / np.convolve on complex128, modulation/models.py:32,46-48).  One step = one
complete Simulation-run of the hot path over `--symbols` OFDM symbols per GPU (TX kernel, power
exchange, RX kernel, counter reduction, counts on the host).  Default 10 steps x 1e6 symbols =
the "1e7 symbols at one SNR" of config (b).  `value` is measured after exactly `--warmup`
untimed steps.  A plain run does no more than that: set-up, warmup, the K timed steps, the
result line (and `--dump-outputs DIR`: what the last timed step returned, as DIR/<field>.npy).
With `--full` the same path in complex64 is reported beside it (`c64_variant`), and so is a
second complex128 measurement after a clock-ramp warmup (`value_after_ramp`); rank 0 also
reports the BER Delta dB of the timed run against the reference-stream path (the second half of
the BASELINE metric) and the CPU baseline, and a `--sweep` adds its per-kernel roofline step.

Multi-GPU: `--gpus N` without a torch.distributed environment re-launches this script as N
ranks (torch.distributed.run, one process per GPU, before anything touches a GPU); each rank
simulates its contiguous share of every step's global symbol range with a fixed share per GPU
(weak scaling); the exchanges are one all-gather of the 40-byte ofdm_stats record (exact
fixed-point power) and one all-reduce of the error counters per step (RCCL).
"""

from __future__ import annotations

import argparse
import importlib
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "ofdm-based-systems_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {
    # name: (N, M, channel, ratio, eq, snr_db, description)
    "b": (1024, 64, "flat_fading", 1.0, "NONE", 24.0,
          "config (b): N_FFT=1024, 64-QAM, flat channel (flat_fading.npy, cp=0), no equaliser, AWGN 24 dB"),
    "c": (1024, 64, "severe_multipath", 1.0, "MMSE", 27.75,
          "config (c): N_FFT=1024, 64-QAM, severe_multipath.npy (8 taps, cp=7), MMSE, AWGN 27.75 dB"),
    # M = 0: CAPACITY_BASED adaptive bit loading (per-subcarrier square-QAM orders from the
    # water-filling allocation at the SNR, simulation/models.py:289-395)
    "d": (2048, 0, "Lin-Phoong_P1", 1.0, "MMSE", 20.0,
          "config (d): N_FFT=2048, adaptive bit loading (water-filling, desired SER 1e-3), Lin-Phoong_P1.npy "
          "(4 taps, cp=3), MMSE, AWGN 20 dB"),
    # 38.75 dB: the BER 1e-4 crossing of this config (profiles/r02g_ber_curve_e.json: 38.67 dB)
    # (deliberately above the reference's 10..30 dB sweep of config/simulation_settings_waterfilling
    # .json, where 256-QAM never reaches BER 1e-4; the kernels' cost does not depend on the SNR)
    "e": (4096, 256, "Lin-Phoong_P1", 1.0, "MMSE", 38.75,
          "config (e): N_FFT=4096, 256-QAM, Lin-Phoong_P1.npy (4 taps, cp=3), MMSE, AWGN 38.75 dB (its BER 1e-4 "
          "crossing, above the reference's 10..30 dB sweep)"),
}
# BASELINE configs[2] / SURVEY 8(d): config (c) as an SNR sweep, 0..30 dB in 1 dB steps plus 0.25 dB
# steps over 26..29 dB around the BER 1e-4 crossing (~27.7 dB) -- 40 points
SWEEP_GRID = sorted(set([float(x) for x in range(0, 31)] + [26 + 0.25 * i for i in range(13)]))
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
PRECISIONS = {"f64": ("c128 (f64)", 16), "f32": ("c64 (f32)", 8)}


def make_engine(cfg, precision):
    """LinkEngine of a bench config; the constellation tables as Simulation builds them
    (QAMConstellationMapper, or the adaptive mapper over the water-filling orders)."""
    from ofdm_based_systems import _backend as B
    from ofdm_based_systems.constellation.adaptive import AdaptiveConstellationMapper
    from ofdm_based_systems.constellation.models import QAMConstellationMapper
    from ofdm_based_systems.engine import LinkEngine
    from ofdm_based_systems.power_allocation.models import WaterfillingPowerAllocation

    N, M, ch, ratio, eq_name, snr, _ = cfg
    h = np.load(os.path.join(ROOT, "config", "channel_models", ch + ".npy"))
    cp = int(ratio * (len(h) - 1))
    eq = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}[eq_name]
    sc = None
    if M == 0:
        gains = np.abs(np.fft.fft(h, N)) ** 2
        noise_power = 10 ** (-snr / 10)
        alloc = WaterfillingPowerAllocation(N, gains, noise_power).allocate()
        orders = np.array([QAMConstellationMapper.calculate_bit_loading_order(ser=1e-3, snr=p * g / noise_power)
                           for p, g in zip(alloc, gains)], dtype=np.int64)
        luts, sc = AdaptiveConstellationMapper(orders, QAMConstellationMapper, N).lut_tables()
    else:
        luts = [QAMConstellationMapper(M).constellation]
    prec = B.OFDM_F32 if precision == "f32" else B.OFDM_F64
    return LinkEngine(N, cp, h, eq, luts, sc, prec)


def kernel_bytes_per_symbol(N: int, bps: int, cp: int, w: int = 8) -> int:
    """Algorithmic bytes one OFDM symbol moves in ONE of the two kernels:
    B_alg = 2*ceil(bps/8) + 2*(N+cp)*w per symbol (bps = N*b, or sum b_k with adaptive loading;
    w = 16 bytes per complex128 sample, 8 per complex64) is split evenly: each kernel touches the
    tx bits once (map / comparator) and the channel stream once (write / read)."""
    return math.ceil(bps / 8) + (N + cp) * w


# ---------------------------------------------------------------------------- CPU baseline
def host_cpus():
    """(affinity-set size, cgroup CPU quota or None): on the GPU box os.cpu_count() and the
    affinity set report every CPU of the machine, while the job's share is the cgroup quota."""
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        aff = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, period = f.read().split()[:2]
        if q != "max":
            quota = max(1, int(int(q) / int(period)))
    except (OSError, ValueError):
        pass
    return aff, quota


def host_cores() -> int:
    """CPUs this process may use: min(affinity set, cgroup quota)."""
    aff, quota = host_cpus()
    return min(aff, quota) if quota else aff


def _cpu_worker(job, barrier, results):
    """One CPU worker: imports and set-up first, then a shared barrier, then the timed sample --
    the oracle run over `S` OFDM symbols in chunks (each chunk a complete run with its own
    reference streams, so memory stays bounded), stream generation included as the GPU leg
    generates its streams."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ofdm_oracle as O

    idx, seed, S, chunk, N, M, ch, cp, eq, snr = job
    h = np.load(os.path.join(ROOT, "config", "channel_models", ch + ".npy"))
    orders = bps = None
    if M == 0:  # CAPACITY_BASED: orders from water-filling, the adaptive data path
        orders, _, _ = O.adaptive_orders(N, h, snr, 1e-3, True)
        bps = int(sum(int(np.log2(o)) for o in orders if o > 0))
    barrier.wait()
    t0 = time.perf_counter()
    done = 0
    while done < S:
        n = min(chunk, S - done)
        if M == 0:
            tx, nz = O.reference_streams(seed + done, n * bps, n * (N + cp))
            O.run_adaptive(tx, orders, N, h, cp, eq, snr, nz)
        else:
            b = int(np.log2(M))
            tx, nz = O.reference_streams(seed + done, n * N * b, n * (N + cp))
            O.run_fixed(tx, n * N * b, N, M, h, cp, eq, snr, nz)
        done += n
    results.put((idx, S, t0, time.perf_counter()))


def literal_reference(config: str):
    """The literal reference's own CPU rate for this config (profiles/literal_reference_cpu.json:
    its Simulation.run timed in the build container by the golden generators, tools/ref_cpu_rate.py),
    reported beside the oracle port the box times; None when absent."""
    path = os.path.join(ROOT, "profiles", "literal_reference_cpu.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        rec = json.load(f).get(config)
    if not rec:
        return None
    return {"per_core_symbols_per_s": rec["per_core_symbols_per_s"], "cores": rec["cores"], "kind": "reference",
            "measured": rec["measured"], "source": "profiles/literal_reference_cpu.json"}


def cpu_baseline(cfg, per_worker: int):
    """The NumPy oracle (a port of the reference path, complex128 like the reference) on every
    CPU of this process's share, one worker process per core, bounded sample.  The workers start,
    import and set up, then meet at a barrier; each times its own sample from there, and value =
    all symbols / the slowest worker's compute time (process start-up is reported beside it as
    wall_incl_spawn_s, never in value)."""
    import multiprocessing as mp

    N, M, ch, ratio, eq, snr, _ = cfg
    h = np.load(os.path.join(ROOT, "config", "channel_models", ch + ".npy"))
    cp = int(ratio * (len(h) - 1))
    chunk = max(8, 2000 * 1024 // N)
    if M == 0:  # whole-byte runs: the adaptive decode needs S * sum(b_k) % 8 == 0
        per_worker = 8 * math.ceil(per_worker / 8)
        chunk = 8 * math.ceil(chunk / 8)
    aff, quota = host_cpus()
    # (at most 32 workers: each spawned worker re-imports this module, torch included, ~0.4 GB; on a
    # whole 8-GPU node the cgroup share can be 8x a 1-GPU box's 16 CPUs)
    workers = min(host_cores(), 32)
    ctx = mp.get_context("spawn")
    barrier, results = ctx.Barrier(workers + 1), ctx.Queue()
    w0 = time.perf_counter()
    procs = [ctx.Process(target=_cpu_worker, args=((i, 100 + 7919 * i, per_worker, chunk, N, M, ch, cp, eq, snr),
                                                   barrier, results)) for i in range(workers)]
    for p in procs:
        p.start()
    barrier.wait()
    out = [results.get() for _ in procs]
    for p in procs:
        p.join()
    wall = time.perf_counter() - w0
    syms = sum(o[1] for o in out)
    durs = [o[3] - o[2] for o in out]
    slowest = max(durs)
    return {
        "value": syms / slowest, "unit": "OFDM symbols/s", "cores": workers, "kind": "port",
        "affinity_cpus": aff, "cgroup_quota_cpus": quota, "host_cpu_count": os.cpu_count(),
        "sample": f"{workers} worker processes (min(affinity set {aff}, cgroup quota {quota}, 32) CPUs; the machine "
                  f"reports {os.cpu_count()}) x {per_worker} OFDM symbols of the same config through the NumPy "
                  f"oracle in complex128, in runs of {chunk} symbols with the reference's PCG64 bits + legacy-normal "
                  f"noise generated inside the timing; clock started per worker after a shared barrier (start-up "
                  f"excluded), value = all symbols / slowest worker ({slowest:.1f} s; fastest {min(durs):.1f} s)",
        "per_core_symbols_per_s": syms / sum(durs),
        "slowest_worker_s": slowest,
        "wall_incl_spawn_s": wall,
    }


# ---------------------------------------------------------------------------- accuracy check
def ber_vs_reference(engine64, N, cp, snr, ber_phx, bits_phx, symbols=16000, seed=1):
    """BER Delta dB of the timed throughput run against the reference-stream path at the same SNR.

    The reference-stream path is the drop-in's default mode: the reference's own PCG64 bytes and
    legacy normal draws (real array first, noise/models.py:19-21) through the complex128 kernels,
    bit-exact with the reference NumPy code (tests/test_gpu_parity.py).  Delta dB is the
    horizontal distance between the two BER curves at the throughput run's BER, through the
    reference curve's local slope from a second point 0.5 dB higher; positive = the throughput
    run needs more SNR.  Outside the timed region."""
    def ref_ber(snr_db, sd):
        bits = np.random.Generator(np.random.PCG64(sd)).bytes(math.ceil(symbols * engine64.bps / 8))
        rs = np.random.RandomState(sd)  # = np.random.seed(sd) + np.random.normal (the reference's draws)
        nr = rs.normal(size=symbols * (N + cp))
        ni = rs.normal(size=symbols * (N + cp))
        r = engine64.run(symbols, snr_db, bits=np.frombuffer(bits, np.uint8), normals=(nr, ni))
        return r.bit_errors, engine64.valid_bits(symbols)

    e0, n0 = ref_ber(snr, seed)
    e1, n1 = ref_ber(snr + 0.5, seed + 1)
    if min(e0, e1, ber_phx * bits_phx) <= 0:
        return {"snr_db": snr, "ber": ber_phx, "ber_reference_streams": e0 / n0, "delta_db": None}
    slope = (math.log10(e1 / n1) - math.log10(e0 / n0)) / 0.5  # decades per dB (< 0)
    delta = (math.log10(ber_phx) - math.log10(e0 / n0)) / slope
    sd_db = 0.4343 * math.sqrt(1.0 / e0 + 1.0 / (ber_phx * bits_phx)) / abs(slope)
    return {"snr_db": snr, "ber": ber_phx, "ber_reference_streams": e0 / n0,
            "reference_symbols": symbols, "slope_decades_per_db": slope,
            "delta_db": delta, "delta_db_stderr": sd_db, "bar_db": 0.05}


def pmc_traffic(key: str, symbols_per_launch: int):
    """HBM bytes per launch of each kernel from a committed rocprofv3 --pmc summary
    (profiles/pmc_summary.json, produced by tools/pmc_summary.py), or None."""
    path = os.path.join(ROOT, "profiles", "pmc_summary.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        pm = json.load(f)
    rec = pm.get(key)
    if not rec:
        return None
    from ofdm_based_systems import _backend as B

    if rec.get("build_id") != B.build_id():  # profiled on other kernel sources: not this build's traffic
        return None
    return {k: v * symbols_per_launch / rec["symbols_per_launch"] for k, v in rec["bytes_per_launch"].items()}


def pmc_issue(key: str):
    """Issue fractions of the fused kernels from committed rocprofv3 SQ counters
    (profiles/pmc_summary.json[key]['issue'], tools/pmc_summary.py --counters), or None when they
    were measured on other kernel sources."""
    path = os.path.join(ROOT, "profiles", "pmc_summary.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        rec = json.load(f).get(key, {}).get("issue")
    if not rec:
        return None
    from ofdm_based_systems import _backend as B

    if rec.get("build_id") != B.build_id():
        return None
    return rec


def build_id_or_none():
    try:
        from ofdm_based_systems import _backend as B

        return B.build_id()
    except OSError:  # pragma: no cover
        return None


# ---------------------------------------------------------------------------- ranks
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(nproc: int) -> int:
    """Run this script as `nproc` ranks under torch.distributed.run (a child process started
    before anything here touches a GPU) and return its exit code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


class Runtime:
    """Device, stream-synchronisation and collective helpers for one rank (GPU, or the CPU when
    a test engine factory runs the bench without a GPU)."""

    def __init__(self, backend: str, cpu: bool):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local = int(os.environ.get("LOCAL_RANK", "0"))
        self.cpu = cpu
        self.group = self.host_group = None
        # OFDM_BENCH_DEVICE pins every rank to one device: a multi-rank rehearsal on a 1-GPU box
        # (with --backend gloo; RCCL refuses two ranks on one GPU)
        self.dev = int(os.environ.get("OFDM_BENCH_DEVICE", self.local))
        self.backend = None
        if not cpu:
            torch.cuda.set_device(self.dev)
        # launched by torch.distributed.run (WORLD_SIZE set): the process group even for one rank, so
        # that a one-GPU rehearsal runs every collective and barrier of a node's N-rank run -- RCCL
        # bound with device_id plus the gloo host group (tests/test_gpu_multirank.py)
        if "WORLD_SIZE" in os.environ:
            import torch.distributed as dist

            if backend == "nccl" and not cpu:
                dist.init_process_group("nccl", device_id=torch.device("cuda", self.dev))
            else:
                dist.init_process_group(backend)
            self.group = dist.group.WORLD
            self.world = dist.get_world_size()
            self.backend = dist.get_backend()
            # host-side group for the closing barrier: while rank 0 times the CPU baseline, the other
            # ranks wait on a socket (gloo) instead of a device collective whose host thread spins
            self.host_group = dist.new_group(backend="gloo") if dist.get_backend() != "gloo" else self.group

    def sync(self):
        if not self.cpu:
            torch.cuda.synchronize()

    def barrier(self):
        if self.group is not None:
            import torch.distributed as dist

            dist.barrier()

    def max_over_ranks(self, x: float) -> float:
        if self.group is None:
            return x
        import torch.distributed as dist

        t = torch.tensor([x], dtype=torch.float64, device="cpu" if self.cpu else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def gather(self, obj):
        if self.group is None:
            return [obj]
        import torch.distributed as dist

        out = [None] * self.world
        dist.all_gather_object(out, obj)
        return out

    def finish(self):
        if self.group is not None:
            import torch.distributed as dist

            dist.barrier(group=self.host_group)
            dist.destroy_process_group()


def timed_steps(rt: Runtime, engine, total: int, snr: float, steps: int, seed0: int, events, lanes: int = 1):
    """K complete runs (one per step), enqueued as LinkEngine.run_pipelined schedules them and
    read back inside the timed region, bracketed by barrier + device synchronisation; the
    elapsed time is the maximum over ranks."""
    rt.sync()
    rt.barrier()
    rt.sync()
    t0 = time.perf_counter()
    pending = engine.run_pipelined(total, snr, range(seed0, seed0 + steps), group=rt.group, events=events,
                                   lanes=lanes)
    results = [p.result() for p in pending]
    rt.sync()
    rt.barrier()
    rt.sync()
    return rt.max_over_ranks(time.perf_counter() - t0), results


# what a caller of the timed path receives per run (engine.LinkStats), as --dump-outputs writes it
OUTPUT_FIELDS = ("bit_errors", "symbol_errors", "power_sum", "x_power_sum", "x_peak", "papr_db")


def dump_outputs(path: str, runs) -> None:
    """--dump-outputs: the LinkStats of the last timed step's runs (one run, or one per point of a
    sweep, in point order) as `path`/<field>.npy, one float64 per run (the counts are exact in
    float64).  The seeds of the timed steps are fixed, so the same arguments give the same inputs."""
    os.makedirs(path, exist_ok=True)
    for name in OUTPUT_FIELDS:
        np.save(os.path.join(path, name + ".npy"), np.array([getattr(r, name) for r in runs], dtype=np.float64))


def roofline(events, N: int, bps: int, cp: int, w: int, traffic, issue=None):
    """The dominant kernel's algorithmic bytes per launch over its average launch time (HIP
    events recorded on the launch stream around every ofdm_tx / ofdm_rx).

    issue (pmc_issue): the committed SQ counters of this build -- then roofline.issue carries the
    dominant kernel's VALU / LDS issue fractions of the SIMDs' time, and `bound` names whichever
    ceiling is closer: "hbm" (achieved / peak, the HBM fraction) or "valu" (the SIMDs' VALU issue
    fraction).  achieved / peak / frac stay the HBM figures either way."""
    if not events:
        return None
    durs = {}
    for name, n, e0, e1 in events:
        durs.setdefault(name, []).append((e0.elapsed_time(e1) * 1e-3, n))
    avg = {k: sum(d for d, _ in v) / len(v) for k, v in durs.items()}
    dom = max(avg, key=avg.get)
    per_launch = durs[dom][0][1]
    alg = kernel_bytes_per_symbol(N, bps, cp, w)
    achieved = alg * per_launch / avg[dom] / 1e9
    out = {
        "bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": None if traffic is None else traffic.get(dom),
        "alg_bytes_per_symbol": alg, "symbols_per_launch": per_launch,
        "avg_launch_ms": {k: v * 1e3 for k, v in avg.items()},
    }
    kd = (issue or {}).get("kernels", {})
    if dom in kd:
        k = kd[dom]
        out["issue"] = {
            "valu": k.get("valu"), "lds": k.get("lds"), "any": k.get("any"),
            "waves_per_simd": k.get("waves_per_simd"),
            "valu_insts_per_symbol": k.get("per_symbol", {}).get("SQ_INSTS_VALU"),
            "other_kernel": {n: {"valu": v.get("valu"), "lds": v.get("lds")} for n, v in kd.items() if n != dom},
            "source": f"profiles/{issue['tag']}_issue.json (rocprofv3 SQ counters of build {issue['build_id']}; "
                      "fraction of the SIMDs' time issuing, GRBM_GUI_ACTIVE as the kernel's duration)",
        }
        if (k.get("valu") or 0.0) > out["frac"]:
            out["bound"] = "valu"
    return out


def measure(rt: Runtime, args, cfg, precision: str, per_gpu: int, factory, ramp: bool):
    """W untimed warmup steps, then K timed steps; optionally a clock-ramp warmup and K more
    timed steps (value_after_ramp)."""
    N, M, ch, ratio, eq_name, snr, _ = cfg
    engine = factory(cfg, precision)
    cp, bps = engine.cp, engine.bps
    total = per_gpu * rt.world
    # the two runs' channel-sample buffers the pipelined schedule keeps alive, allocated before
    # the warmup (a first-time hipMalloc of 2 x 16.4 GB would otherwise land in the timed steps)
    lanes = args.lanes or 1
    engine.reserve(total, 2, group=rt.group, lanes=lanes)
    for i in range(args.warmup):
        engine.run(total, snr, seed=10_000 + i, group=rt.group)
    events = None if rt.cpu else []
    elapsed, results = timed_steps(rt, engine, total, snr, args.steps, 0, events, lanes)
    bit_errors = sum(r.bit_errors for r in results)
    w = PRECISIONS[precision][1]
    key = args.config if precision == "f32" else f"{args.config}_{precision}"
    rec = {
        "value": total * args.steps / elapsed,
        "ms_per_step": elapsed / args.steps * 1e3,
        "dtype": PRECISIONS[precision][0],
        "roofline": roofline(events, N, bps, cp, w, None if rt.cpu else pmc_traffic(key, per_gpu),
                             None if rt.cpu else pmc_issue(key)),
        "ber": bit_errors / (engine.valid_bits(total) * args.steps),
        "bits": engine.valid_bits(total) * args.steps,
        "last_step": results[-1:],
    }
    rec["path_hbm_fraction"] = rec["value"] * 2 * kernel_bytes_per_symbol(N, bps, cp, w) / (
        HBM_PEAK_GBS * 1e9 * rt.world)
    if ramp and args.ramp_seconds > 0:
        # a fresh box idles at low clocks and needs ~40 ms of load to reach the steady state its
        # power cap sets (profiles/r02_ramp_b.json): keep running untimed steps for --ramp-seconds,
        # then time K more
        extra, t_ramp = 0, time.perf_counter()
        while True:
            done = torch.tensor([time.perf_counter() - t_ramp >= args.ramp_seconds], dtype=torch.int32,
                                device="cpu" if rt.cpu else "cuda")
            if rt.group is not None:
                import torch.distributed as dist

                dist.all_reduce(done, op=dist.ReduceOp.MIN)  # every rank runs the same number of steps
            if int(done.item()):
                break
            engine.run(total, snr, seed=20_000 + extra, group=rt.group)
            extra += 1
        e2, _ = timed_steps(rt, engine, total, snr, args.steps, 30_000, None, lanes)
        rec["value_after_ramp"] = {"value": total * args.steps / e2, "ms_per_step": e2 / args.steps * 1e3,
                                   "extra_untimed_steps": extra, "ramp_seconds": args.ramp_seconds}
    return engine, rec


def crossing(snrs, bers, target=1e-4):
    """SNR where a BER curve crosses `target` (log10 BER linear in dB between grid points)."""
    pts = sorted((q, b) for q, b in zip(snrs, bers) if b > 0)
    for (s0, b0), (s1, b1) in zip(pts[:-1], pts[1:]):
        if b0 >= target > b1:
            l0, l1, lt = math.log10(b0), math.log10(b1), math.log10(target)
            return s0 + (s1 - s0) * (l0 - lt) / (l0 - l1)
    return None


def reference_sweep(engine64, N, cp, snrs, symbols):
    """BER of the reference-stream path (the reference's PCG64 bits and legacy normals through the
    complex128 kernels, bit-exact with the reference NumPy code) at each SNR; outside any timing."""
    out = []
    for i, q in enumerate(snrs):
        bits = np.random.Generator(np.random.PCG64(500 + i)).bytes(math.ceil(symbols * engine64.bps / 8))
        rs = np.random.RandomState(500 + i)
        nr = rs.normal(size=symbols * (N + cp))
        ni = rs.normal(size=symbols * (N + cp))
        r = engine64.run(symbols, q, bits=np.frombuffer(bits, np.uint8), normals=(nr, ni))
        out.append(r.bit_errors / engine64.valid_bits(symbols))
    return out


# The sweeps of BASELINE configs[2..4] as the reference's settings files run them: one
# engine (plan) per group, each group's SNR points pipelined through LinkEngine.run_pipelined.
#   c: config/simulation_settings_custom_channel.json's channel at N = 1024 / 64-QAM over SWEEP_GRID;
#   d: config/simulation_settings_adaptive.json's SNRs 15 / 20 / 25 dB (the bit loading is derived
#      per SNR, simulation/models.py:289-395, so every point has its own plan);
#   e: config/simulation_settings_waterfilling.json's SNRs 10..30 dB by 5 at 16-, 64- and 256-QAM
#      (BASELINE configs[4]: "up to 256-QAM").
SWEEP_SNRS_D = [15.0, 20.0, 25.0]
SWEEP_SNRS_E = [10.0, 15.0, 20.0, 25.0, 30.0]
SWEEP_ORDERS_E = [16, 64, 256]


def sweep_groups(name: str, cfg):
    """[(config tuple of the group's engine, its SNR points)] of the --sweep of config `name`."""
    N, M, ch, ratio, eq_name, snr, desc = cfg
    if name == "d":
        return [((N, M, ch, ratio, eq_name, q, desc), [q]) for q in SWEEP_SNRS_D]
    if name == "e":
        return [((N, m, ch, ratio, eq_name, snr, desc), list(SWEEP_SNRS_E)) for m in SWEEP_ORDERS_E]
    if M == 0:
        raise SystemExit("--sweep of an adaptive config other than (d)")
    return [(cfg, list(SWEEP_GRID))]


def measure_sweep(rt: Runtime, args, groups, precision: str, per_gpu: int, factory):
    """The SNR sweep as the bench step: every step runs all points of every group, `per_gpu`
    OFDM symbols per GPU each (one complete run per point, new seed per point and step), each
    group's points pipelined through its engine's LinkEngine.run_pipelined (all groups enqueued
    before any result is read) and symbol-sharded across ranks; W untimed steps, K timed."""
    engines = [factory(g, precision) for g, _ in groups]
    total = per_gpu * rt.world
    # four lanes (HIP streams, one hardware queue each): the short launches of one point's TX overlap
    # the others' RX and fill their start / drain bubbles -- config c's sweep 1.219-1.236e8 at two
    # lanes against 1.243-1.251e8 at four, same box (profiles/r06p_sweep_lanes_c.txt)
    lanes = args.lanes or 4
    for eng in engines:
        eng.reserve(total, 2, group=rt.group, lanes=lanes)
    npts = sum(len(q) for _, q in groups)

    for i in range(args.warmup):  # one untimed sweep per warmup step, every group enqueued first
        pend = [eng.run_pipelined(total, snrs, [50_000 + 1000 * gi + 100 * i + k for k in range(len(snrs))],
                                  group=rt.group, lanes=lanes)
                for gi, (eng, (_, snrs)) in enumerate(zip(engines, groups))]
        for ps in pend:
            for p in ps:
                p.result()
    rt.sync()
    rt.barrier()
    rt.sync()
    t0 = time.perf_counter()
    # per group one pipelined call over all K steps' points (step-major), every group enqueued
    # before any count is read back
    pend = []
    for gi, (eng, (_, snrs)) in enumerate(zip(engines, groups)):
        pend.append(eng.run_pipelined(total, snrs * args.steps,
                                      [1_000_000 * gi + 1000 * st + k for st in range(args.steps)
                                       for k in range(len(snrs))], group=rt.group, lanes=lanes))
    results = [[p.result() for p in ps] for ps in pend]
    errs = [[r.bit_errors for r in rs] for rs in results]
    rt.sync()
    rt.barrier()
    rt.sync()
    elapsed = rt.max_over_ranks(time.perf_counter() - t0)
    w = PRECISIONS[precision][1]
    points = []
    for gi, ((gcfg, snrs), eng) in enumerate(zip(groups, engines)):
        nbits = eng.valid_bits(total) * args.steps
        for k, q in enumerate(snrs):
            e = sum(errs[gi][k::len(snrs)])
            points.append({"snr_db": q, "qam_order": gcfg[1] if gcfg[1] else "adaptive", "bits_per_ofdm_symbol": eng.bps,
                           "ber": e / nbits, "bits": nbits})
    # --full: the kernels' launch times for the roofline: one more sweep step after the timed region, on
    # ONE lane with HIP events around every launch -- on two lanes a kernel's events would also span the
    # other lane's overlapping kernel (round 4's sweep line reported that bound, not a measurement);
    # the group whose symbols carry the most bits stands for the sweep
    roof = None
    if args.full and not rt.cpu:
        gi = max(range(len(engines)), key=lambda j: engines[j].bps)
        events = []
        for p in engines[gi].run_pipelined(total, groups[gi][1], [90_000 + k for k in range(len(groups[gi][1]))],
                                           group=rt.group, events=events, lanes=1):
            p.result()
        roof = roofline(events, groups[gi][0][0], engines[gi].bps, engines[gi].cp, w, None)
        if roof is not None:
            roof["measured"] = ("one untimed sweep step of the group with the most bits per symbol, on one HIP stream "
                                "after the timed region (HIP events around every launch; no overlap between kernels)")
    rec = {
        "value": total * npts * args.steps / elapsed,
        "ms_per_step": elapsed / args.steps * 1e3,
        "dtype": PRECISIONS[precision][0],
        "lanes": lanes,
        "roofline": roof,
        # the last timed step's runs, in point order
        "last_step": [r for (_, snrs), rs in zip(groups, results) for r in rs[len(rs) - len(snrs):]],
        "sweep": {"snr_db": [pt["snr_db"] for pt in points], "ber": [pt["ber"] for pt in points],
                  # one value when every group's symbols carry the same bits, else one per group (in
                  # group order; per_point[*].bits holds every point's own)
                  "bits_per_point": (points[0]["bits"] if len({pt["bits"] for pt in points}) == 1
                                     else [eng.valid_bits(total) * args.steps for eng in engines]),
                  "points": npts, "symbols_per_point_per_step": total,
                  "per_point": points},
    }
    return engines, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10,
                    help="untimed steps before the K timed ones (default 10, ~0.1 s of config (b): past the "
                         "first launches' code-object loads, workspace allocations and the clock's first transient)")
    ap.add_argument("--symbols", type=int, default=0,
                    help="OFDM symbols per GPU per step (default 1e6 x 1024/N)")
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS),
                    help="BASELINE config (default b; with --sweep, c: the sweep BASELINE configs[2] names)")
    ap.add_argument("--precision", default="f64", choices=sorted(PRECISIONS),
                    help="arithmetic of the headline line (f64 = complex128, the reference's)")
    ap.add_argument("--no-variant", action="store_true", help="skip the complex64 companion run")
    ap.add_argument("--cpu-sample", type=int, default=0,
                    help="OFDM symbols per CPU worker (default 30000 x 1024/N: ~15 s of work per core)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ber-check", action="store_true", help="skip the BER Delta-dB check vs the reference streams")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL)")
    ap.add_argument("--ramp-seconds", type=float, default=0.25,
                    help="clock-ramp warmup before the value_after_ramp measurement (0: skip it)")
    ap.add_argument("--engine-factory", default=None, help=argparse.SUPPRESS)  # tests: module:function
    ap.add_argument("--sweep", action="store_true",
                    help="one step = the SNR sweep of BASELINE configs[2] (0..30 dB by 1 dB + 26..29 dB by 0.25 dB); "
                         "with --config d / e the reference settings' SNR lists of configs[3] / [4] (15/20/25 dB "
                         "adaptive; 10..30 dB by 5 at 16/64/256-QAM); --symbols per GPU per point (default 1e5 x 1024/N)")
    ap.add_argument("--lanes", type=int, default=None,
                    help="HIP streams the timed runs alternate over (LinkEngine.run_pipelined); default 1, "
                         "--sweep 4 (its 1e5-symbol points overlap receivers with the next transmitters: "
                         "1.02 -> 1.08e8 symbols/s at 2, profiles/r04c_sweep_c*.json; 2 -> 4: +1.4 %, "
                         "profiles/r06p_sweep_lanes_c.txt)")
    ap.add_argument("--ref-symbols", type=int, default=12000,
                    help="--sweep: reference-stream OFDM symbols per point near the BER 1e-4 crossing (26..29 dB)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the other precision's companion run, the "
                         "value_after_ramp measurement, the BER check against the reference streams, the CPU "
                         "baseline and a sweep's per-kernel roofline step (each still has its own --no-... switch)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (its run's LinkStats "
                         "fields; one entry per point with --sweep) as DIR/<field>.npy in float64")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.config is None:
        args.config = "c" if args.sweep else "b"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))

    factory = make_engine
    if args.engine_factory:
        mod, fn = args.engine_factory.split(":")
        factory = getattr(importlib.import_module(mod), fn)
    rt = Runtime(args.backend, cpu=bool(args.engine_factory) and not torch.cuda.is_available())
    if args.gpus > 1 and rt.world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={rt.world}")

    cfg = CONFIGS[args.config]
    N, M, ch, ratio, eq_name, snr, desc = cfg
    if args.sweep:
        return sweep_main(rt, args, cfg, factory)
    per_gpu = args.symbols if args.symbols else 1_000_000 // max(1, N // 1024)
    total = per_gpu * rt.world
    engine, head = measure(rt, args, cfg, args.precision, per_gpu, factory, ramp=args.full)
    if args.dump_outputs and rt.rank == 0:
        dump_outputs(args.dump_outputs, head["last_step"])
    variant = None
    if args.full and not args.no_variant:
        other = "f32" if args.precision == "f64" else "f64"
        _, variant = measure(rt, args, cfg, other, per_gpu, factory, ramp=False)
    devices = rt.gather(rt.dev if not rt.cpu else "cpu")

    out = {
        "metric": "OFDM symbols/sec (1/2/4/8 GPU) at N_FFT=1024 64-QAM; BER ΔdB vs ref",
        "value": head["value"],
        "unit": "OFDM symbols/s",
        "n_gpus": rt.world,
        "devices": devices,
        "process_group": rt.backend,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": head["ms_per_step"],
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": head["dtype"],
        "data": "synthetic: Philox4x32-10 / MWC64X bits and Box-Muller AWGN (64-point phase table) generated "
                "on the GPU per (seed, symbol), stream version 3: the noise radius is the Rayleigh quantile at "
                "the midpoints of 2^31 equiprobable cells (its tail exact at every cell boundary down to "
                "6.555 sigma), the component tail within 2^-33 of the Gaussian",
        "config": {
            "workload": f"{desc}; {per_gpu} OFDM symbols per GPU per step",
            "n_fft": N, "qam_order": M if M else "adaptive", "bits_per_ofdm_symbol": engine.bps, "cp": engine.cp,
            "channel": ch, "equalizer": eq_name, "snr_db": snr,
            "symbols_per_step": total, "parallelism": f"symbol-sharded x{rt.world}",
        },
        "roofline": head["roofline"],
        "build_id": build_id_or_none(),
        "path_hbm_fraction": head["path_hbm_fraction"],
        "ber": head["ber"],
    }
    if "value_after_ramp" in head:
        out["value_after_ramp"] = head["value_after_ramp"]
    if variant is not None:
        out[("c64" if variant["dtype"].startswith("c64") else "c128") + "_variant"] = {
            k: variant[k] for k in ("value", "ms_per_step", "dtype", "roofline", "path_hbm_fraction", "ber")}
    if rt.rank == 0 and args.full and not args.no_ber_check and not rt.cpu:
        eng64 = make_engine(cfg, "f64")
        out["ber_vs_reference"] = ber_vs_reference(eng64, N, engine.cp, snr, head["ber"], head["bits"],
                                                   symbols=max(2000, 16000 * 1024 // N))
    if rt.rank == 0 and args.full and not args.no_cpu_baseline:
        # on rank 0 after every GPU measurement, for any number of ranks (the other ranks wait at
        # rt.finish()): the reference CPU path on the node's host cores, in the same run
        out["cpu_baseline"] = cpu_baseline(cfg, args.cpu_sample or max(100, 30000 * 1024 // N))
        lit = literal_reference(args.config)
        if lit is not None:
            out["cpu_baseline"]["literal_reference"] = lit
    if rt.rank == 0:
        print(json.dumps(out), flush=True)
    rt.finish()


def sweep_main(rt: Runtime, args, cfg, factory):
    """--sweep: BASELINE configs[2] (config (c), the default) -- symbols/s over the whole SNR sweep and
    the BER 1e-4 crossing of the timed runs against the reference-stream path's; with --config d / e
    the reference's own SNR lists of configs[3] / [4] (sweep_groups)."""
    N, M, ch, ratio, eq_name, snr, desc = cfg
    groups = sweep_groups(args.config, cfg)
    per_gpu = args.symbols if args.symbols else 100_000 // max(1, N // 1024)
    engines, head = measure_sweep(rt, args, groups, args.precision, per_gpu, factory)
    if args.dump_outputs and rt.rank == 0:
        dump_outputs(args.dump_outputs, head["last_step"])
    engine = engines[0]
    total = per_gpu * rt.world
    devices = rt.gather(rt.dev if not rt.cpu else "cpu")
    sw = head["sweep"]
    if args.config == "d":
        what = (f"{desc.split(',')[0]} as config/simulation_settings_adaptive.json runs it: SNR 15 / 20 / 25 dB, the "
                f"bit loading derived per SNR")
    elif args.config == "e":
        what = (f"{desc.split(',')[0]} as config/simulation_settings_waterfilling.json runs it: SNR 10..30 dB by 5 at "
                f"16-, 64- and 256-QAM")
    else:
        what = f"{desc.split(',')[0]} as the BASELINE configs[2] SNR sweep: 0..30 dB by 1 dB, 26..29 dB by 0.25 dB"
    out = {
        "metric": "OFDM symbols/sec (1/2/4/8 GPU) at N_FFT=1024 64-QAM; BER ΔdB vs ref",
        "value": head["value"], "unit": "OFDM symbols/s", "n_gpus": rt.world, "devices": devices, "process_group": rt.backend,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": head["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": head["dtype"],
        "data": "synthetic: Philox4x32-10 / MWC64X bits and Box-Muller AWGN generated on the GPU per (seed, symbol)",
        "config": {
            "workload": f"{what}; {sw['points']} points x {per_gpu} OFDM symbols per GPU per point; one step = the "
                        f"whole sweep",
            "n_fft": N, "qam_order": SWEEP_ORDERS_E if args.config == "e" else (M if M else "adaptive"),
            "bits_per_ofdm_symbol": engine.bps if len(engines) == 1 else [e.bps for e in engines],
            "cp": engine.cp, "channel": ch, "equalizer": eq_name, "snr_db": "sweep",
            "symbols_per_step": total * sw["points"], "parallelism": f"symbol-sharded x{rt.world}",
        },
        "roofline": head["roofline"],
        "build_id": build_id_or_none(),
        "sweep": sw,
    }
    if args.config == "c" or (args.config not in ("d", "e") and M):
        c_phx = crossing(sw["snr_db"], sw["ber"])
        out["ber_1e-4_crossing_db"] = {"throughput": c_phx}
        if rt.rank == 0 and args.full and not args.no_ber_check and not rt.cpu:
            near = [q for q in sw["snr_db"] if 26.0 <= q <= 29.0]
            eng64 = make_engine(cfg, "f64")
            ref = reference_sweep(eng64, N, engine.cp, near, max(1000, args.ref_symbols * 1024 // N))
            c_ref = crossing(near, ref)
            out["ber_1e-4_crossing_db"]["reference_streams"] = c_ref
            out["ber_1e-4_crossing_db"]["reference_symbols_per_point"] = max(1000, args.ref_symbols * 1024 // N)
            out["ber_1e-4_crossing_db"]["reference_ber"] = dict(zip(near, ref))
            out["delta_db_at_1e-4"] = None if c_phx is None or c_ref is None else c_phx - c_ref
            out["bar_db"] = 0.05
    else:
        # (d) / (e): no BER 1e-4 crossing inside the reference's SNR list (the adaptive loading holds
        # SER ~1e-3 at every SNR; 256-QAM stays above 1e-4 to 30 dB) -- the single-point bench lines
        # carry the BER check of these configs (ber_vs_reference)
        out["ber_1e-4_crossing_db"] = None
    if rt.rank == 0 and args.full and not args.no_cpu_baseline:
        cpu_cfg = (N, M, ch, ratio, eq_name, 27.75 if args.config == "c" else snr, desc)
        out["cpu_baseline"] = cpu_baseline(cpu_cfg, args.cpu_sample or max(100, 30000 * 1024 // N))
        if args.config == "e":
            out["cpu_baseline"]["sample"] += (" (the 256-QAM group's engine only, at %s dB -- the sweep's other groups are "
                                              "16- and 64-QAM, whose CPU cost per symbol is lower)" % cpu_cfg[5])
        elif args.config == "d":
            out["cpu_baseline"]["sample"] += (" (the %s dB point's bit loading only: every point of the sweep has its "
                                              "own plan)" % cpu_cfg[5])
        else:
            out["cpu_baseline"]["sample"] += (" (at one point of the sweep, %s dB: the CPU cost does not depend on the "
                                              "SNR)" % cpu_cfg[5])
    if rt.rank == 0:
        print(json.dumps(out), flush=True)
    rt.finish()


if __name__ == "__main__":
    main()

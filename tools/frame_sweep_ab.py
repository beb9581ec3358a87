#!/usr/bin/env python3
"""An FER-versus-SNR curve three ways, in one process on one GPU in complex128, steps alternating:

  (i)   LinkEngine.run_frame_sweep(n, snrs, F)          one transmit, ofdm_rx_sweep_frames over every point
  (ii)  [run(n, q, frame_symbols=F) for q in snrs]      the way without the sweep: a transmit and an
                                                        ofdm_rx_frames per point
  (iii) LinkEngine.run_sweep(n, snrs)                   the sweep without the record (ofdm_rx_sweep)

over bench.py's SNR lists (config c: the 40-point grid; config e: its 256-QAM list), n symbols per point,
at F = 14 and F = 1.  Reported: the step's wall time (launch to results) as median and interquartile range,
the receivers' HIP-event time, (ii) / (i) -- the gain of the sweep with the record -- and (i) / (iii) -- the
record's cost inside the sweep -- and that the three ways count the same errors.

    python tools/frame_sweep_ab.py [--steps 20] [--warmup 2] [--symbols 100000] > profiles/frame_sweep_ab.txt
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ofdm-based-systems_amd")]

import numpy as np  # noqa: E402


def timed(fn):
    """(wall ms, receiver event ms, results) of one step."""
    import torch

    ev = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn(ev)
    wall = (time.perf_counter() - t0) * 1e3
    rx = sum(e0.elapsed_time(e1) for k, _, e0, e1 in ev if k != "ofdm_tx")
    return wall, rx, res


def summary(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25))


def case(name, snrs, n, F, steps, warmup):
    import bench

    eng = bench.make_engine(bench.CONFIGS[name], "f64")
    eng.reserve(n, 1)
    ways = {
        "i": lambda seed: lambda ev: eng.run_frame_sweep(n, snrs, F, seed=seed, events=ev),
        "ii": lambda seed: lambda ev: [eng.run(n, q, seed=seed, frame_symbols=F, events=ev) for q in snrs],
        "iii": lambda seed: lambda ev: eng.run_sweep(n, snrs, seed=seed, events=ev),
    }
    for k in range(warmup):
        for w in ways.values():
            timed(w(100 + k))
    rows = {w: [] for w in ways}
    order = list(ways)
    for k in range(steps):
        got = {}
        for w in order[k % 3:] + order[:k % 3]:   # rotate which goes first
            wall, rx, got[w] = timed(ways[w](1000 + k))
            rows[w].append((wall, rx))
        # the three ways count the same errors, and (i)'s records are (ii)'s
        cnt = {w: [(r.bit_errors, r.symbol_errors) for r in res] for w, res in got.items()}
        assert cnt["i"] == cnt["ii"] == cnt["iii"], (name, F, k)
        assert all(np.array_equal(a.frames.bit_errors, b.frames.bit_errors) and int(a.frames.bit_errors.sum()) == a.bit_errors
                   for a, b in zip(got["i"], got["ii"])), (name, F, k)
        fer = [r.frames.fer for r in got["i"]]
    out = {w: (summary([r[0] for r in v]), summary([r[1] for r in v])) for w, v in rows.items()}
    K = len(snrs)
    print(f"config {name}, {K} points x {n} symbols, F = {F} ({steps} alternating steps, medians [iqr], ms):")
    label = {"i": "(i)   run_frame_sweep        ", "ii": "(ii)  run(frame_symbols) x K ", "iii": "(iii) run_sweep              "}
    for w in ways:
        (sm, si), (rm, ri) = out[w]
        print(f"  {label[w]} step {sm:9.3f} [{si:6.3f}]   receivers {rm:9.3f} [{ri:6.3f}]   "
              f"{K * n / sm * 1e3:.4g} point-symbols/s")
    print(f"  (ii) / (i) = {out['ii'][0][0] / out['i'][0][0]:.3f} (step), {out['ii'][1][0] / out['i'][1][0]:.3f} (receivers);  "
          f"(i) / (iii) = {out['i'][0][0] / out['iii'][0][0]:.3f} (step), {out['i'][1][0] / out['iii'][1][0]:.3f} (receivers)")
    print(f"  FER at the points with 0 < FER < 1: "
          + ", ".join(f"{q:g} dB {f:.4g}" for q, f in zip(snrs, fer) if f is not None and 0 < f < 1), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--symbols", type=int, default=100_000, help="OFDM symbols per point at N = 1024 (N = 4096: a quarter)")
    args = ap.parse_args()
    import torch

    import bench

    torch.cuda.set_device(0)
    print(f"# tools/frame_sweep_ab.py on {torch.cuda.get_device_name(0)}, complex128")
    for name, snrs in (("c", list(bench.SWEEP_GRID)), ("e", list(bench.SWEEP_SNRS_E))):
        n = args.symbols * 1024 // bench.CONFIGS[name][0]
        for F in (14, 1):
            case(name, snrs, n, F, args.steps, args.warmup)


if __name__ == "__main__":
    main()

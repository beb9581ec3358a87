#!/usr/bin/env python3
"""Rate of an SNR sweep two ways, in one process on one GPU:

  A  LinkEngine.run_pipelined(total, snrs, seeds, lanes=4): one complete run (ofdm_tx + ofdm_rx) per
     point, four lanes -- the way bench.py --sweep and tools/ber_curve.py run sweeps;
  B  LinkEngine.run_sweep(total, snrs): one transmit, every point from one ofdm_rx_sweep pass.

    python tools/sweep_rate.py --config b|c|e [--pairs 3] [--symbols N] [--out profiles/sweep_rate_<config>.json]

The SNR lists are bench.py's (sweep_groups: config c the 40-point grid; config e its three orders x five
SNRs, one engine per order), 1e5 * 1024 / N OFDM symbols per point.  Both paths are warmed up, then
alternate A B A B ...; each repetition is timed by the host clock around work that ends in a device
synchronise.  Prints symbols x points per second of every repetition, the medians' ratio B / A and
the spread, checks that B's counts equal single-point runs at three points of the first group, and
writes the JSON record DESIGN.md section 6 quotes.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ofdm-based-systems_amd")]

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=["b", "c", "e"], required=True)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--symbols", type=int, default=None, help="OFDM symbols per point (default 1e5 * 1024 / N)")
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pairs < 3:
        ap.error("at least three A/B pairs")
    cfg = bench.CONFIGS[args.config]
    groups = bench.sweep_groups(args.config, cfg)
    total = args.symbols or 100_000 * 1024 // cfg[0]
    engines = [bench.make_engine(g, args.precision) for g, _ in groups]
    npts = sum(len(q) for _, q in groups)
    for eng in engines:
        eng.reserve(total, 2, lanes=4)

    def path_a(rep):
        pend = [eng.run_pipelined(total, snrs, [7000 + 100 * rep + k for k in range(len(snrs))], lanes=4)
                for eng, (_, snrs) in zip(engines, groups)]
        return [[p.result() for p in ps] for ps in pend]

    def path_b(rep):
        pend = [eng.run_sweep_async(total, snrs, seed=7000 + rep) for eng, (_, snrs) in zip(engines, groups)]
        return [p.result() for p in pend]

    def timed(fn, rep):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(rep)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    path_a(-1), path_b(-1)  # warm-up of both
    ta, tb, last_b = [], [], None
    for rep in range(args.pairs):
        ta.append(timed(path_a, rep)[0])
        dt, last_b = timed(path_b, rep)
        tb.append(dt)
    rate = lambda t: total * npts / t
    for name, ts in (("A run_pipelined", ta), ("B run_sweep", tb)):
        print(f"{name:16s} symbols x points / s: " + "  ".join(f"{rate(t):.4e}" for t in ts))
    ma, mb = statistics.median(ta), statistics.median(tb)
    spread = lambda ts: (max(ts) - min(ts)) / statistics.median(ts)
    print(f"ratio of medians B / A: {ma / mb:.3f}  (spread A {spread(ta):.1%}, B {spread(tb):.1%})")

    # B's counts against single-point runs: first, middle and last point of the first group
    eng, snrs = engines[0], groups[0][1]
    seed = 7000 + args.pairs - 1
    checked = []
    for k in sorted({0, len(snrs) // 2, len(snrs) - 1}):
        one = eng.run(total, snrs[k], seed=seed)
        got = last_b[0][k]
        assert (got.bit_errors, got.symbol_errors) == (one.bit_errors, one.symbol_errors), (snrs[k], got, one)
        checked.append({"snr_db": snrs[k], "bit_errors": got.bit_errors, "symbol_errors": got.symbol_errors})
    print("counts equal single-point runs at", [c["snr_db"] for c in checked], "dB")

    rec = {"config": args.config, "precision": args.precision, "device": torch.cuda.get_device_name(0),
           "symbols_per_point": total, "points": npts, "groups": [{"qam_order": g[1], "snr_db": q} for g, q in groups],
           "seconds_A_run_pipelined_lanes4": ta, "seconds_B_run_sweep": tb,
           "rate_A": [rate(t) for t in ta], "rate_B": [rate(t) for t in tb],
           "ratio_of_medians_B_over_A": ma / mb, "spread_A": spread(ta), "spread_B": spread(tb),
           "counts_checked": checked}
    out = args.out or os.path.join(ROOT, "profiles", f"sweep_rate_{args.config}.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()

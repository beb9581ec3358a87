#!/usr/bin/env python3
"""Cost of the constellation-density record (ofdm_rx_density, LinkEngine.run(density=128)) on one GPU in
complex128, against the two receivers it is read beside: ofdm_rx_profile, the nearest existing receiver
of the same one-wave-per-SIMD workgroup shape, and the plain two-kernel run.  Bench configs (b) -- the
two-kernel path, fused=False -- (c) and (e) at the bench's symbols per step, each at 24 dB and with the
noise off: without noise every point of a 64-QAM run falls on one of 64 cells, the worst same-address case
of the LDS adds.  In one process, after a warm-up, steps rotate over

    plain    run(n, snr, fused=False)                  ofdm_tx + ofdm_rx
    profile  run(n, snr, fused=False, profile=True)    ofdm_tx + ofdm_rx_profile
    density  run(n, snr, fused=False, density=128)     ofdm_tx + ofdm_rx_density

and the receiver's HIP-event time is reported as a median with its spread.  (ofdm_rx and ofdm_rx_profile
are the parent commit's kernels, machine code for machine code: profiles/density_kernel_audit.txt.)

    python tools/density_ab.py [--steps 10] [--warmup 2] > profiles/density_ab.txt   # on the GPU
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ofdm-based-systems_amd")]

import numpy as np  # noqa: E402

# (config, symbols per step: bench.py's 1e6 // (N / 1024))
CASES = (("b", 1_000_000), ("c", 1_000_000), ("e", 250_000))
SNR_DB = 24.0
# kind: (run's keywords, the receiver's event name, the entry point)
KINDS = {"plain": ({}, "ofdm_rx", "ofdm_rx"), "profile": ({"profile": True}, "ofdm_rx", "ofdm_rx_profile"),
         "density": ({"density": 128}, "ofdm_rx_density", "ofdm_rx_density")}


def step(eng, n, seed, noise_on, kind):
    """(receiver event ms, bit errors, LinkStats) of one run."""
    kw, event, _ = KINDS[kind]
    ev = []
    res = eng.run(n, SNR_DB, seed=seed, fused=False, noise_on=noise_on, events=ev, **kw)
    rx = sum(e0.elapsed_time(e1) for k, _, e0, e1 in ev if k == event)
    return rx, res.bit_errors, res


def case(name, n, noise_on, steps, warmup):
    import bench

    eng = bench.make_engine(bench.CONFIGS[name], "f64")
    eng.reserve(n, 1)
    for k in range(warmup):
        for kind in KINDS:
            step(eng, n, 100 + k, noise_on, kind)
    rows = {kind: [] for kind in KINDS}
    order = list(KINDS)
    for k in range(steps):
        for kind in order[k % 3:] + order[:k % 3]:   # rotate which goes first
            rx, be, res = step(eng, n, 1000 + k, noise_on, kind)
            rows[kind].append((rx, be))
            if kind == "density":
                d = res.density
                assert d.n_points == int(d.counts.sum()) + d.outside == n * int(np.count_nonzero(eng.bits_per_subcarrier))
                cells = int(np.count_nonzero(d.counts))
    assert len({tuple(r[1] for r in rows[kind]) for kind in KINDS}) == 1   # the same counts, seed by seed
    med = {kind: float(np.median([r[0] for r in rows[kind]])) for kind in KINDS}
    iqr = {kind: float(np.subtract(*np.percentile([r[0] for r in rows[kind]], [75, 25]))) for kind in KINDS}
    print(f"config {name}, N = {eng.n_fft}, {n} symbols, {'24 dB' if noise_on else 'noise off'}, {cells} non-empty cells "
          f"of 16384: " + ", ".join(f"{KINDS[kind][2]} {med[kind]:.3f} [{iqr[kind]:.3f}] ms" for kind in KINDS)
          + f"; density / profile {med['density'] / med['profile']:.3f}, density / plain "
          f"{med['density'] / med['plain']:.3f}; {n * eng.n_fft / med['density'] / 1e6:.2f} G points/s binned", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    print(f"# tools/density_ab.py on {torch.cuda.get_device_name(0)}: the receiver's HIP-event time, complex128, "
          f"{args.steps} rotating steps each after {args.warmup} warm-up rounds; medians, iqr in brackets")
    for name, n in CASES:
        for noise_on in (True, False):
            case(name, n, noise_on, args.steps, args.warmup)


if __name__ == "__main__":
    main()

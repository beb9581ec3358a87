"""Reference runs above 256 points per constellation: 1024/4096-QAM, wide PSK, and CAPACITY_BASED
loading at SNRs where the reference itself loads 1024- and 4096-QAM.

Run ONLY where the reference is importable, with the environment make_golden.py's docstring gives
(the reference's src on PYTHONPATH, no bytecode, the Agg backend):

    python tests/golden/make_golden_wide.py

Writes ``runs_wide.json`` (the record format of runs.json), the stage fixture
``stage_n64_m1024_severe_cp_mmse.npz`` and its record ``stages_wide.json``; runs.json and stages.json
are not touched.  Seeded exactly like make_golden.run_sim.  Every case must pin something: the
generator refuses to write a run with fewer than 10 bit errors or a BER of 0.1 or more.
"""

from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (imports the reference)

STAGE = ("n64_m1024_severe_cp_mmse", 64, 1024, "severe_multipath", "CP", 1.0, "MMSE", 34.0, 16, 14)


def main() -> None:
    cases, weak = [], []

    def add(tag, seed, ch, **kw):
        h = G.channel(ch)
        res = G.run_sim(seed, channel_impulse_response=h, **kw)
        params = {k: (v.value if hasattr(v, "value") else v) for k, v in kw.items()}
        cases.append(dict(tag=tag, seed=seed, channel=ch, params=params, result=res))
        orders = res["constellation_order_per_subcarrier"]
        hist = {o: orders.count(o) for o in sorted(set(orders))}
        print(f"  {tag} seed={seed} snr={kw['snr_db']} be={res['bit_errors']} se={res['symbol_errors']} "
              f"bits={res['total_bits']} orders={hist} t={res['_ref_seconds']:.1f}s", file=sys.stderr, flush=True)
        if res["bit_errors"] < 10 or res["bit_errors"] >= 0.1 * res["total_bits"]:
            weak.append(f"{tag}: {res['bit_errors']} bit errors in {res['total_bits']} bits")

    CP, NP, ZP = G.PrefixType.CYCLIC, G.PrefixType.NONE, G.PrefixType.ZERO
    MM, NE = G.EqualizationMethod.MMSE, G.EqualizationMethod.NONE
    base = dict(constellation_scheme=G.ConstellationType.QAM, modulator_type=G.ModulationType.OFDM,
                noise_scheme=G.NoiseType.AWGN, power_allocation_type=G.PowerAllocationType.UNIFORM,
                adaptive_modulation_mode=G.AdaptiveModulationMode.FIXED, prefix_length_ratio=1.0)
    psk = dict(base, constellation_scheme=G.ConstellationType.PSK)
    ad = dict(base, power_allocation_type=G.PowerAllocationType.WATERFILLING,
              adaptive_modulation_mode=G.AdaptiveModulationMode.CAPACITY_BASED)

    # FIXED 1024- and 4096-QAM (num_symbols counts constellation symbols in FIXED mode)
    add("wide_n64_m1024_flat_none", 3, "flat_fading", num_symbols=4096, num_subcarriers=64,
        constellation_order=1024, prefix_scheme=NP, equalizator_type=NE, snr_db=30.0, **base)
    add("wide_n64_m4096_flat_none", 3, "flat_fading", num_symbols=4096, num_subcarriers=64,
        constellation_order=4096, prefix_scheme=NP, equalizator_type=NE, snr_db=38.0, **base)
    add("wide_n64_m1024_severe_mmse", 4, "severe_multipath", num_symbols=4096, num_subcarriers=64,
        constellation_order=1024, prefix_scheme=CP, equalizator_type=MM, snr_db=36.0, **base)
    # CAPACITY_BASED + water-filling on Lin-Phoong P1 at SER 1e-3: 35 dB loads 1024-QAM, 40 dB 4096-QAM
    # (num_symbols counts OFDM symbols here; multiples of 8 keep the bit stream in whole bytes)
    for n, nsym, snr in ((64, 512, 35.0), (64, 512, 40.0), (2048, 64, 35.0)):
        add(f"wide_n{n}_adaptive_p1", 5, "Lin-Phoong_P1", num_symbols=nsym, num_subcarriers=n,
            constellation_order=16, prefix_scheme=CP, equalizator_type=MM, snr_db=snr,
            desired_symbol_error_rate=1e-3, **ad)
    # PSK: 64 and 128 points (regression cover below the old limit), 1024 points above it
    for m, snr in ((64, 30.0), (128, 36.0), (1024, 50.0)):
        add(f"wide_n64_psk{m}_flat_none", 6, "flat_fading", num_symbols=4096, num_subcarriers=64,
            constellation_order=m, prefix_scheme=NP, equalizator_type=NE, snr_db=snr, **psk)
    # the largest accepted shape: 4096-QAM at N = 4096, 4 OFDM symbols
    add("wide_n4096_m4096_p1_mmse", 7, "Lin-Phoong_P1", num_symbols=4096 * 4, num_subcarriers=4096,
        constellation_order=4096, prefix_scheme=CP, equalizator_type=MM, snr_db=44.0, **base)
    # SC-OFDM with zero padding
    add("wide_scofdm_zp_n64_m1024_severe_mmse", 8, "severe_multipath", num_symbols=4096, num_subcarriers=64,
        constellation_order=1024, prefix_scheme=ZP, equalizator_type=MM, snr_db=35.0,
        **dict(base, modulator_type=G.ModulationType.SC_OFDM))

    stage = G.make_stage(*STAGE)
    print(f"  stage {stage['name']} be={stage['bit_errors']} se={stage['symbol_errors']}", file=sys.stderr)
    if stage["bit_errors"] < 10:
        weak.append(f"stage {stage['name']}: {stage['bit_errors']} bit errors")
    if weak:
        raise SystemExit("these cases pin nothing, move their SNR:\n  " + "\n  ".join(weak))
    with open(os.path.join(G.OUT, "stages_wide.json"), "w") as f:
        json.dump([stage], f, indent=1)
    with open(os.path.join(G.OUT, "runs_wide.json"), "w") as f:
        json.dump(cases, f, indent=1, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))


if __name__ == "__main__":
    main()

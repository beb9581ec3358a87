"""Reference runs over channels with an exact spectral null or one deep fade.

``[1, -1]`` (null at DC), ``[1, 1]`` (null at N/2) and ``[1, -1j]`` (null at N/4) have a frequency
response that is exactly ``0j`` on one subcarrier; ``[1, -(1 - 2**-12)]`` has ``|H_0|`` about 2.4e-4
and no exact zero.  On a null bin the reference's MMSE output is an exact (signed) zero, a four-way
tie of every square QAM that its first-index argmin decides; its ZF output there is the noise divided
by 1e-10.

Run ONLY where the reference is importable, with the environment make_golden.py's docstring gives:

    python tests/golden/make_golden_nulls.py

Writes ``runs_nulls.json`` (the record format of runs.json plus ``taps``, ``k0`` and, for ZF, what the
null bin held), ``stages_nulls.json`` and ``stage_null_*.npz``; no other fixture is touched.  Seeded
exactly like make_golden.run_sim.  Every null case asserts ``np.fft.fft(h, N)[k0] == 0``.  ZF cases
take the first seed from their base seed upwards at which (a) every real and imaginary part of the
pre-equaliser spectrum on the null bin is above 1e-3 in modulus, so the noise's sign decides the
symbol and no precision can flip it, and (b) more than half of those components, divided by 1e-10
and scaled to level units, exceed 2^31 (the share is recorded).
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (imports the reference)

TAPS = {
    "null_dc": np.array([1, -1], dtype=np.complex128),
    "null_half": np.array([1, 1], dtype=np.complex128),
    "null_quarter": np.array([1, -1j], dtype=np.complex128),
    "fade_dc": np.array([1, -(1 - 2.0 ** -12)], dtype=np.complex128),
}
K0 = {"null_dc": lambda n: 0, "null_half": lambda n: n // 2, "null_quarter": lambda n: n // 4}

_files = G.channel
G.channel = lambda name: TAPS[name].copy() if name in TAPS else _files(name)

STAGES = [
    # name, N, M, channel, prefix, ratio, eq, snr, S, base seed
    ("null_n8_m16_half_zf", 8, 16, "null_half", "CP", 1.0, "ZF", 5.0, 16, 21),
    ("null_n64_m64_dc_mmse", 64, 64, "null_dc", "CP", 1.0, "MMSE", 30.0, 8, 22),
    ("null_n64_m64_quarter_zf", 64, 64, "null_quarter", "CP", 1.0, "ZF", 10.0, 8, 23),
    ("null_n1024_m64_dc_mmse", 1024, 64, "null_dc", "CP", 1.0, "MMSE", 30.0, 4, 24),
]
# ZF: low enough that most null-bin samples pass 2^31 level units (fewer levels need more noise)
ZF_SNR = {4: 0.0, 16: 5.0, 64: 10.0, 256: 10.0, 1024: 10.0, 4096: 10.0}
MMSE_SNR = {4: 10.0, 16: 18.0, 64: 30.0, 256: 32.0, 1024: 38.0, 4096: 44.0}
SEED_TRIES = 64


def null_bin(ch: str, n: int):
    if ch not in K0:
        return None
    k0 = K0[ch](n)
    assert np.fft.fft(TAPS[ch], n)[k0] == 0, (ch, n)
    return k0


def level_scale(m: int) -> float:
    """Level units per unit of amplitude of square m-QAM: (side - 1) / (max level - min level)."""
    lev = np.unique(G.QAMConstellationMapper(m).constellation.real)
    return (len(lev) - 1) / (lev[-1] - lev[0])


def zf_bin_facts(Yk: np.ndarray, m: int) -> dict:
    """Yk: the pre-equaliser spectrum on the null bin, one entry per OFDM symbol."""
    comp = np.concatenate([Yk.real, Yk.imag])
    t = np.abs(comp) / 1e-10 * level_scale(m)
    return dict(min_abs_component=float(np.min(np.abs(comp))), share_above_2p31=float(np.mean(t > 2.0 ** 31)))


def zf_ok(facts: dict) -> bool:
    return facts["min_abs_component"] > 1e-3 and facts["share_above_2p31"] > 0.5


class ZFCapture:
    """Records what ZeroForcingEqualizator.equalize is handed (one row per OFDM symbol)."""

    def __enter__(self):
        self.rows = []
        self.orig = G.ZeroForcingEqualizator.equalize
        rows, orig = self.rows, self.orig

        def equalize(eqz, received_symbols):
            rows.append(np.array(received_symbols))
            return orig(eqz, received_symbols)

        G.ZeroForcingEqualizator.equalize = equalize
        return self

    def __exit__(self, *exc):
        G.ZeroForcingEqualizator.equalize = self.orig


def main() -> None:
    cases = []

    def add(tag, seed0, ch, **kw):
        n = kw["num_subcarriers"]
        k0 = null_bin(ch, n)
        zf = kw["equalizator_type"] == G.EqualizationMethod.ZF and k0 is not None
        for seed in range(seed0, seed0 + (SEED_TRIES if zf else 1)):
            with ZFCapture() as cap:
                res = G.run_sim(seed, channel_impulse_response=TAPS[ch].copy(), **kw)
            facts = zf_bin_facts(np.array(cap.rows)[:, k0], kw["constellation_order"]) if zf else None
            if not zf or zf_ok(facts):
                break
        else:
            raise SystemExit(f"{tag}: no seed in {seed0}..{seed0 + SEED_TRIES - 1} meets the ZF conditions")
        params = {k: (v.value if hasattr(v, "value") else v) for k, v in kw.items()}
        rec = dict(tag=tag, seed=seed, channel=ch, taps=[[float(t.real), float(t.imag)] for t in TAPS[ch]],
                   k0=k0, params=params, result=res)
        if zf:
            rec["zf_null_bin"] = facts
        cases.append(rec)
        print(f"  {tag} seed={seed} snr={kw['snr_db']} be={res['bit_errors']} se={res['symbol_errors']} "
              f"bits={res['total_bits']} zf={facts} t={res['_ref_seconds']:.1f}s", file=sys.stderr, flush=True)

    CP, ZP = G.PrefixType.CYCLIC, G.PrefixType.ZERO
    MM, ZF = G.EqualizationMethod.MMSE, G.EqualizationMethod.ZF
    base = dict(constellation_scheme=G.ConstellationType.QAM, modulator_type=G.ModulationType.OFDM,
                noise_scheme=G.NoiseType.AWGN, power_allocation_type=G.PowerAllocationType.UNIFORM,
                adaptive_modulation_mode=G.AdaptiveModulationMode.FIXED, prefix_length_ratio=1.0,
                prefix_scheme=CP, num_subcarriers=64)
    nsym = 64 * 40  # FIXED mode counts constellation symbols: 40 OFDM symbols

    def snr(eq, m):
        return ZF_SNR[m] if eq == ZF else MMSE_SNR[m]

    for eq in (MM, ZF):
        for ch in ("null_dc", "null_half", "null_quarter"):
            for m in (4, 16, 64, 256):
                add(f"null_n64_m{m}_{ch[5:]}_{eq.value.lower()}", 30, ch, num_symbols=nsym,
                    constellation_order=m, equalizator_type=eq, snr_db=snr(eq, m), **base)
        for m in (1024, 4096):
            add(f"null_n64_m{m}_dc_{eq.value.lower()}", 31, "null_dc", num_symbols=nsym,
                constellation_order=m, equalizator_type=eq, snr_db=snr(eq, m), **base)
    psk = dict(base, constellation_scheme=G.ConstellationType.PSK)
    add("null_n64_psk4_dc_mmse", 32, "null_dc", num_symbols=nsym, constellation_order=4,
        equalizator_type=MM, snr_db=10.0, **psk)
    add("null_n64_psk8_dc_mmse", 32, "null_dc", num_symbols=nsym, constellation_order=8,
        equalizator_type=MM, snr_db=18.0, **psk)
    add("null_scofdm_n64_m16_half_mmse", 33, "null_half", num_symbols=nsym, constellation_order=16,
        equalizator_type=MM, snr_db=18.0, **dict(base, modulator_type=G.ModulationType.SC_OFDM))
    add("null_zp_n64_m16_dc_mmse", 34, "null_dc", num_symbols=nsym, constellation_order=16,
        equalizator_type=MM, snr_db=18.0, **dict(base, prefix_scheme=ZP))
    for eq in (ZF, MM):
        add(f"fade_n64_m64_dc_{eq.value.lower()}", 35, "fade_dc", num_symbols=nsym, constellation_order=64,
            equalizator_type=eq, snr_db=30.0, **base)
    # CAPACITY_BASED with UNIFORM power (water-filling refuses a zero gain): num_symbols counts OFDM
    # symbols here; the null bin, and the bins about it whose SNR loads nothing, get order 0
    add("null_n64_adaptive_uniform_dc", 36, "null_dc", num_symbols=40, constellation_order=16,
        equalizator_type=MM, snr_db=25.0, desired_symbol_error_rate=1e-3,
        **dict(base, adaptive_modulation_mode=G.AdaptiveModulationMode.CAPACITY_BASED))
    # the shapes whose reference-stream runs take the throughput kernels
    add("null_n1024_m64_dc_mmse", 37, "null_dc", num_symbols=1024 * 8, constellation_order=64,
        equalizator_type=MM, snr_db=30.0, **dict(base, num_subcarriers=1024))
    add("null_n4096_m256_dc_mmse", 38, "null_dc", num_symbols=4096 * 2, constellation_order=256,
        equalizator_type=MM, snr_db=32.0, **dict(base, num_subcarriers=4096))

    ad = next(c for c in cases if c["tag"] == "null_n64_adaptive_uniform_dc")
    assert ad["result"]["constellation_order_per_subcarrier"][0] == 0
    try:
        G.WaterfillingPowerAllocation(64.0, np.abs(np.fft.fft(TAPS["null_dc"], 64)) ** 2, 1e-2).allocate()
    except ValueError as e:
        waterfilling_error = str(e)
    else:
        raise SystemExit("the reference's water-filling accepted a zero gain")

    stages = []
    for name, n, m, ch, prefix, ratio, eq, snr_db, s, seed0 in STAGES:
        k0 = null_bin(ch, n)
        for seed in range(seed0, seed0 + (SEED_TRIES if eq == "ZF" else 1)):
            st = G.make_stage(name, n, m, ch, prefix, ratio, eq, snr_db, s, seed)
            a = np.load(os.path.join(G.OUT, f"stage_{name}.npz"))
            Y = np.fft.fft(a["y"].reshape(-1, n + st["cp"])[:, st["cp"]:], axis=1, norm="ortho")
            facts = zf_bin_facts(Y[:, k0], m) if eq == "ZF" else None
            if eq != "ZF" or zf_ok(facts):
                break
        else:
            raise SystemExit(f"stage {name}: no seed meets the ZF conditions")
        assert a["H"][k0] == 0
        if eq == "MMSE":
            assert np.all(a["Z"][:, k0] == 0)
        st["k0"] = k0
        if facts:
            st["zf_null_bin"] = facts
        stages.append(st)
        print(f"  stage {name} seed={seed} be={st['bit_errors']} se={st['symbol_errors']} zf={facts}", file=sys.stderr)

    with open(os.path.join(G.OUT, "stages_nulls.json"), "w") as f:
        json.dump(dict(stages=stages, waterfilling_error=waterfilling_error), f, indent=1)
    for c in cases:
        for k in ("_ref_seconds", "transmission_time_ms"):  # wall times: the fields that would not regenerate
            c["result"].pop(k, None)
    with open(os.path.join(G.OUT, "runs_nulls.json"), "w") as f:
        json.dump(cases, f, indent=1, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))


if __name__ == "__main__":
    main()

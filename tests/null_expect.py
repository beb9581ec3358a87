"""Loaders and expectations for the spectral-null fixtures (tests/golden/make_golden_nulls.py): channels
whose frequency response is exactly 0 on one subcarrier, k0.  What tests/test_null_bins_cpu.py and
tests/test_gpu_null_bins.py share.

On a null bin the reference's MMSE output is an exact zero -- a four-way tie of every square QAM, which
its first-index argmin decides (ORIGIN_INDEX) -- and its ZF output is the noise divided by 1e-10, far
beyond the profile's cap of 2^20 and any density extent.
"""

import json
import os

import numpy as np
from conftest import GOLDEN
from numpy.random import PCG64, Generator

import ofdm_oracle as O

# argmin_m |0 - C_m| (first index) of the reference's LUTs.  Square QAM: the four central points tie;
# the first of them is (-1, +1) * scale -- on I the lower of the two central levels, on Q the upper.
ORIGIN_INDEX = {4: 0, 16: 5, 64: 18, 256: 85, 1024: 330, 4096: 1365}
# the same decision per axis: (I level, Q level) counted from the most negative level
ORIGIN_LEVELS = {m: (int(np.sqrt(m)) // 2 - 1, int(np.sqrt(m)) // 2) for m in ORIGIN_INDEX}
PSK_ORIGIN_INDEX = {2: 0, 4: 0}

CAP = 2.0 ** 20  # the profile's cap on |z - c|^2 (profile_expect.CAP)


def load_runs():
    with open(os.path.join(GOLDEN, "runs_nulls.json")) as f:
        return json.load(f)


def _stage_file():
    with open(os.path.join(GOLDEN, "stages_nulls.json")) as f:
        return json.load(f)


def load_stages():
    return _stage_file()["stages"]


def waterfilling_error():
    """The message of the ValueError the reference's water-filling raises on a zero gain."""
    return _stage_file()["waterfilling_error"]


def taps(case):
    return np.array([complex(re, im) for re, im in case["taps"]], np.complex128)


def run_id(c):
    return f"{c['tag']}-s{c['seed']}-{c['params']['snr_db']}"


def stage(name):
    return next(s for s in load_stages() if s["name"] == name)


def null_taps(kind):
    """The impulse responses of the fixtures by name."""
    return {"null_dc": np.array([1, -1], np.complex128), "null_half": np.array([1, 1], np.complex128),
            "null_quarter": np.array([1, -1j], np.complex128),
            "fade_dc": np.array([1, -(1 - 2.0 ** -12)], np.complex128)}[kind]


def fx_limbs(power):
    """(low, high) limbs of an error power that is a whole multiple of 2^-40, in the profile's
    fixed-point format (rows 2 and 3: units of 2^-40 and 2^-8)."""
    units = int(power) << 40
    return units & 0xFFFFFFFF, units >> 32


def seeded_run(case, **extra):
    """The reference's seeding recipe applied to this package, as
    test_gpu_parity.seeded_run, with the case's own taps as the channel."""
    import ofdm_based_systems.bits_generation.models as bg
    from ofdm_based_systems.configuration.enums import (
        AdaptiveModulationMode,
        ConstellationType,
        EqualizationMethod,
        ModulationType,
        NoiseType,
        PowerAllocationType,
        PrefixType,
    )
    from ofdm_based_systems.simulation.models import Simulation

    enums = {
        "constellation_scheme": ConstellationType, "modulator_type": ModulationType, "prefix_scheme": PrefixType,
        "equalizator_type": EqualizationMethod, "noise_scheme": NoiseType,
        "power_allocation_type": PowerAllocationType, "adaptive_modulation_mode": AdaptiveModulationMode,
    }
    seed = case["seed"]
    bg.RandomBitsGenerator.__init__.__defaults__ = (Generator(PCG64(seed)),)
    bg.AdaptiveBitsGenerator.__init__.__defaults__ = (Generator(PCG64(seed)),)
    np.random.seed(seed)
    kw = {}
    for k, v in case["params"].items():
        if k in enums:
            v = enums[k]("SC-OFDM" if v == "SC_OFDM" else v)
        kw[k] = v
    return Simulation(verbose=False, channel_impulse_response=taps(case), make_plot=False, **kw, **extra).run()


def oracle_fixed_run(case):
    """ofdm_oracle.run_reference_fixed of a FIXED, square-QAM, OFDM, cyclic-prefix case."""
    p = case["params"]
    return O.run_reference_fixed(case["seed"], p.get("num_symbols"), p.get("num_bits"), p["num_subcarriers"],
                                 p["constellation_order"], taps(case), p["prefix_length_ratio"], "CP",
                                 p["equalizator_type"], p["snr_db"])


def is_plain_fixed_qam(case):
    p = case["params"]
    return (p["adaptive_modulation_mode"] == "FIXED" and p["modulator_type"] == "OFDM"
            and p["prefix_scheme"] == "CYCLIC" and p["constellation_scheme"] == "QAM")

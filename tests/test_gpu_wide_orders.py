"""Constellations above 256 points (1024/4096-QAM, PSK up to 1024) on the GPU against the reference:
seeded Simulation.run results (tests/golden/runs_wide.json, bit-exact counts), the 1024-QAM stage
fixture through the fused engine and the operators, and the limits that stay (throughput streams
carry at most 8 bits per subcarrier).

On the commit before wide orders every test here that builds a plan with an order above 256 fails
with ValueError "constellation order must be a power of two in [2, 256]"; the 64/128-PSK runs and
test_narrow_throughput_still_runs pass there too and are regression cover.
"""

import io
import json
import math
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN, channel, stage_arrays
from numpy.random import PCG64, Generator

import ofdm_oracle as O
import ofdm_based_systems.bits_generation.models as bg
from ofdm_based_systems import _backend as B
from ofdm_based_systems.configuration.enums import (
    AdaptiveModulationMode,
    ConstellationType,
    EqualizationMethod,
    ModulationType,
    NoiseType,
    PowerAllocationType,
    PrefixType,
)
from ofdm_based_systems.constellation.models import PSKConstellationMapper, QAMConstellationMapper
from ofdm_based_systems.engine import LinkEngine
from ofdm_based_systems.simulation.models import Simulation

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "runs_wide.json")) as _f:
    RUNS = json.load(_f)
with open(os.path.join(GOLDEN, "stages_wide.json")) as _f:
    STAGE = json.load(_f)[0]
EQ = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}
ENUMS = {
    "constellation_scheme": ConstellationType, "modulator_type": ModulationType, "prefix_scheme": PrefixType,
    "equalizator_type": EqualizationMethod, "noise_scheme": NoiseType,
    "power_allocation_type": PowerAllocationType, "adaptive_modulation_mode": AdaptiveModulationMode,
}


def seeded_run(case, **extra):
    """The reference's seeding recipe applied to this package, as
    test_gpu_parity.seeded_run."""
    seed = case["seed"]
    bg.RandomBitsGenerator.__init__.__defaults__ = (Generator(PCG64(seed)),)
    bg.AdaptiveBitsGenerator.__init__.__defaults__ = (Generator(PCG64(seed)),)
    np.random.seed(seed)
    kw = {}
    for k, v in case["params"].items():
        if k in ENUMS:
            v = ENUMS[k]("SC-OFDM" if v == "SC_OFDM" else v)
        kw[k] = v
    return Simulation(verbose=False, channel_impulse_response=channel(case["channel"]), make_plot=False,
                      **kw, **extra).run()


def _id(c):
    return f"{c['tag']}-s{c['seed']}-{c['params']['snr_db']}"


def case(tag, snr=None):
    return next(c for c in RUNS if c["tag"] == tag and (snr is None or c["params"]["snr_db"] == snr))


@pytest.mark.parametrize("c", RUNS, ids=_id)
def test_simulation_run_matches_reference(gpu, c):
    """The assertions of test_gpu_parity.test_simulation_run_matches_reference on the wide cases."""
    r = c["result"]
    got = seeded_run(c)
    assert got["bit_errors"] == r["bit_errors"]
    assert got["symbol_errors"] == r["symbol_errors"]
    assert got["total_bits"] == r["total_bits"]
    assert math.isclose(got["papr_db"], r["papr_db"], rel_tol=1e-9)
    assert got["constellation_order_per_subcarrier"] == r["constellation_order_per_subcarrier"]
    np.testing.assert_allclose(got["allocated_power"], r["allocated_power"], rtol=1e-12, atol=1e-300)
    if r["water_level"] is None:
        assert got["water_level"] is None
    else:
        assert math.isclose(got["water_level"], r["water_level"], rel_tol=1e-9)
    for key in ("title", "subtitle", "prefix_acronym", "power_allocation_acronym", "num_subcarriers",
                "constellation_scheme", "modulator_type", "equalizator_type"):
        assert got[key] == r[key], key
    assert set(r) - {"_ref_seconds", "_received_symbols_len"} <= set(got)


def stage_engine(precision=B.OFDM_F64):
    a = stage_arrays(STAGE["name"])
    eng = LinkEngine(STAGE["N"], STAGE["cp"], a["h_raw"], EQ[STAGE["eq"]], [O.qam_lut(STAGE["M"])],
                     precision=precision)
    return a, eng


def test_fused_engine_stage_parity(gpu):
    """ofdm_tx / ofdm_rx on the 1024-QAM stage fixture: counts, received symbols, PAPR, power."""
    a, eng = stage_engine()
    S = STAGE["S"]
    res = eng.run(S, STAGE["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]), keep_symbols=S)
    assert res.bit_errors == STAGE["bit_errors"]
    assert res.symbol_errors == STAGE["symbol_errors"]
    assert math.isclose(res.papr_db, STAGE["papr_db"], rel_tol=1e-12)
    np.testing.assert_allclose(res.received, a["Z"].ravel(), rtol=1e-9, atol=1e-9)
    assert math.isclose(res.power_sum, float(np.sum(np.abs(a["y_clean"]) ** 2)), rel_tol=1e-12)


def test_operators_on_stage_fixture(gpu):
    """ofdm_map / ofdm_demap / ofdm_demap_count at 10 bits per subcarrier on the reference's own
    bytes and symbols."""
    a = stage_arrays(STAGE["name"])
    N, M = STAGE["N"], STAGE["M"]
    mapper = QAMConstellationMapper(M)
    X = mapper.encode(io.BytesIO(a["tx_bytes"].tobytes()))
    assert np.array_equal(X.reshape(-1, N), a["X"])
    assert mapper.decode(a["X"].ravel()).read() == a["tx_bytes"].tobytes()
    assert mapper.decode(a["Z"].ravel()).read() == a["rx_bytes"].tobytes()
    for precision in (B.OFDM_F64, B.OFDM_F32):
        plan = B.Plan(n_fft=N, precision=precision, luts=[O.qam_lut(M)])
        Z = torch.from_numpy(a["Z"]).to(plan.cdtype).to(gpu)
        tx = torch.from_numpy(a["tx_bytes"].copy()).to(gpu)
        cnt = torch.zeros(2, dtype=torch.int64, device=gpu)
        B.check(B.lib().ofdm_demap_count(plan.handle, B.stream_ptr(), B.ptr(Z), B.ptr(tx), Z.shape[0], B.ptr(cnt)))
        assert tuple(cnt.cpu().tolist()) == (STAGE["bit_errors"], STAGE["symbol_errors"])


def test_qam1024_decode_matches_argmin(gpu):
    """Every point of the LUT displaced by less than 0.3 of half a level step per axis (off every
    decision boundary), the outer rows and columns also pushed outwards past the last level."""
    lut = O.qam_lut(1024)
    rng = np.random.default_rng(1024)
    half = (np.unique(lut.real)[1] - np.unique(lut.real)[0]) / 2
    idx = np.concatenate([np.arange(1024), rng.integers(0, 1024, size=1024)])
    z = lut[idx] + 0.3 * half * (rng.uniform(-1, 1, len(idx)) + 1j * rng.uniform(-1, 1, len(idx)))
    edge = np.abs(lut[idx].real) == np.abs(lut.real).max()
    z[edge] += 5 * half * np.sign(lut[idx][edge].real)
    edge = np.abs(lut[idx].imag) == np.abs(lut.imag).max()
    z[edge] += 5j * half * np.sign(lut[idx][edge].imag)
    want = O.nn_demap(z, lut)
    assert np.array_equal(want, idx)
    assert QAMConstellationMapper(1024).decode(z).read() == O.indices_to_bytes(want, 10)


def test_psk1024_decode_matches_argmin(gpu):
    """1024-PSK (not separable: the nearest-point search): points rotated by less than 0.3 of half
    the angular spacing and scaled radially."""
    lut = O.psk_lut(1024)
    rng = np.random.default_rng(1025)
    idx = np.concatenate([np.arange(1024), rng.integers(0, 1024, size=512)])
    z = lut[idx] * rng.uniform(0.7, 1.3, len(idx)) * np.exp(1j * 0.3 * (np.pi / 1024) * rng.uniform(-1, 1, len(idx)))
    want = O.nn_demap(z, lut)
    assert np.array_equal(want, idx)
    mapper = PSKConstellationMapper(1024)
    assert mapper.decode(z).read() == O.indices_to_bytes(want, 10)
    data = rng.integers(0, 256, size=160, dtype=np.uint8).tobytes()
    assert np.array_equal(mapper.encode(io.BytesIO(data)), lut[O.bits_to_indices(O.bytes_to_bits(data), 10)])


def test_fused_tail_mask_matches_operators(gpu):
    """n_valid_bits 13 bits short of the run -- the last subcarrier and 3 bits of the one before --
    in the fused receiver against the operators on the symbols it kept: ofdm_demap_count over all
    bits, less the errors ofdm_demap's bytes show in the 13 masked bits.  (ofdm_demap_count takes
    whole OFDM symbols, so the mask itself is applied to the demapped bytes here.)"""
    a, eng = stage_engine()  # (run at 15 dB: most symbols decide wrongly, far outside the grid too)
    S, N, b = STAGE["S"], STAGE["N"], 10
    total = S * N * b
    res = eng.run(S, 15.0, bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]),
                  keep_symbols=S, n_valid_bits=total - 13)
    plan = B.Plan(n_fft=N, luts=[O.qam_lut(1024)])
    Z = torch.from_numpy(res.received.reshape(S, N)).to(gpu)
    tx = torch.from_numpy(a["tx_bytes"].copy()).to(gpu)
    cnt = torch.zeros(2, dtype=torch.int64, device=gpu)
    B.check(B.lib().ofdm_demap_count(plan.handle, B.stream_ptr(), B.ptr(Z), B.ptr(tx), S, B.ptr(cnt)))
    be_all, se = cnt.cpu().tolist()
    rx = np.frombuffer(QAMConstellationMapper(1024).decode(res.received).read(), np.uint8)
    diff = np.unpackbits(rx) != np.unpackbits(a["tx_bytes"])
    assert int(diff.sum()) == be_all
    tail = int(diff[total - 13:].sum())
    assert tail > 0, "the masked bits must hold errors for the mask to show"
    assert (res.bit_errors, res.symbol_errors) == (be_all - tail, se)


@pytest.mark.parametrize("batch", [1, 3])
def test_batched_schedule_is_identical(gpu, batch):
    c = case("wide_n64_m1024_severe_mmse")
    r = c["result"]
    got = seeded_run(c, batch_symbols=batch)
    assert (got["bit_errors"], got["symbol_errors"]) == (r["bit_errors"], r["symbol_errors"])
    assert math.isclose(got["papr_db"], r["papr_db"], rel_tol=1e-9)


@pytest.mark.parametrize("tag", ["wide_n64_m1024_flat_none", "wide_n64_m1024_severe_mmse"])
def test_f32_tracks_reference(gpu, tag):
    """complex64 with the reference's streams: the project's rule for counts, PAPR to 1e-5."""
    c = case(tag)
    r = c["result"]
    got = seeded_run(c, precision="f32")
    assert abs(got["bit_errors"] - r["bit_errors"]) <= max(2, 2e-3 * r["bit_errors"])
    assert abs(got["symbol_errors"] - r["symbol_errors"]) <= max(2, 2e-3 * r["symbol_errors"])
    assert math.isclose(got["papr_db"], r["papr_db"], rel_tol=1e-5)


def test_throughput_mode_refuses_wide_orders(gpu):
    a, eng = stage_engine()
    with pytest.raises(ValueError, match="at most 8 bits per subcarrier"):
        eng.run(STAGE["S"], STAGE["snr_db"])


def test_narrow_throughput_still_runs(gpu):
    a = stage_arrays(STAGE["name"])
    eng = LinkEngine(STAGE["N"], STAGE["cp"], a["h_raw"], EQ[STAGE["eq"]], [O.qam_lut(256)])
    res = eng.run(64, 30.0, seed=5)
    assert res.num_ofdm_symbols == 64 and 0 <= res.bit_errors < 0.1 * 64 * STAGE["N"] * 8

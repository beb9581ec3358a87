"""The per-subcarrier profile of the fused receiver (ofdm_rx_profile, LinkEngine.run(profile=True),
Simulation(subcarrier_profile=True)) on the GPU against tests/profile_expect.py: the expected rows
restated with the oracle's demapper from equalised symbols and transmitted indices.

Integer rows (bit errors, symbol errors, clipped) are compared exactly.  The error power is compared
within profile_expect.power_bound: with every device symbol within delta_k = delta (1 + max |Z_sk|) of
the symbols the expectation is computed from (delta = 1e-9, the project's complex128 tolerance on Z;
1e-4 for complex64), |dEP_k| <= 2 delta_k sqrt(S EP_k) + S delta_k^2 + S 2^-41, twice that between
two device runs.

On the commit before the profile every test here fails: LinkEngine.run has no ``profile`` argument.
"""

import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
from conftest import GOLDEN, ROOT, channel, load_runs, load_stages, stage_arrays
from numpy.random import PCG64, Generator

import ofdm_oracle as O
import philox_streams as P
import profile_expect as PE
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
from ofdm_based_systems.constellation.adaptive import AdaptiveConstellationMapper
from ofdm_based_systems.constellation.models import QAMConstellationMapper
from ofdm_based_systems.engine import LinkEngine
from ofdm_based_systems.simulation.models import Simulation

pytestmark = pytest.mark.gpu

EQ = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}
ENUMS = {
    "constellation_scheme": ConstellationType, "modulator_type": ModulationType, "prefix_scheme": PrefixType,
    "equalizator_type": EqualizationMethod, "noise_scheme": NoiseType,
    "power_allocation_type": PowerAllocationType, "adaptive_modulation_mode": AdaptiveModulationMode,
}
INT_ROWS = ("bit_errors", "symbol_errors", "clipped")


def rows_of(prof):
    return {k: getattr(prof, k) for k in INT_ROWS + ("error_power",)}


def assert_rows(got, exp, Z, delta, factor=1.0, what=""):
    for k in INT_ROWS:
        assert np.array_equal(got[k], exp[k]), (what, k, np.flatnonzero(got[k] != exp[k])[:8])
    bound = PE.power_bound(Z, exp["error_power"], delta, factor)
    err = np.abs(got["error_power"] - exp["error_power"])
    worst = int(np.argmax(err - bound))
    print(f"{what}: error power max |diff| {err.max():.3e}, at the worst subcarrier {err[worst]:.3e} "
          f"against the bound {bound[worst]:.3e}")
    assert np.all(err <= bound), (what, worst, err[worst], bound[worst])


def assert_identical(p, q, what=""):
    for k in INT_ROWS + ("error_power_fx",):
        assert np.array_equal(getattr(p, k), getattr(q, k)), (what, k)


def assert_sums(res):
    assert int(res.profile.bit_errors.sum()) == res.bit_errors
    assert int(res.profile.symbol_errors.sum()) == res.symbol_errors


# ---------------------------------------------------------------- 1. reference streams, complex128
def stage_run(st, precision=B.OFDM_F64, **kw):
    a = stage_arrays(st["name"])
    eng = LinkEngine(st["N"], st["cp"], a["h_raw"], EQ[st["eq"]], [O.qam_lut(st["M"])], precision=precision)
    S = st["S"]
    res = eng.run(S, st["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]), profile=True,
                  keep_symbols=S, **kw)
    return a, eng, res


def stage_expect(st, a, Z, n_valid=None):
    N, S, b = st["N"], st["S"], int(np.log2(st["M"]))
    bk = np.full(N, b, np.int64)
    idx = PE.tx_indices(a["tx_bytes"], bk, S)
    return PE.expected_rows(Z, idx, bk, S * N * b if n_valid is None else n_valid)


@pytest.mark.parametrize("st", load_stages(), ids=lambda s: s["name"])
def test_stage_fixtures_generic_kernel(gpu, st):
    a, eng, res = stage_run(st)
    S, N = st["S"], st["N"]
    # as test_fused_engine_stage_parity
    assert res.bit_errors == st["bit_errors"]
    assert res.symbol_errors == st["symbol_errors"]
    np.testing.assert_allclose(res.received, a["Z"].ravel(), rtol=1e-9, atol=1e-9)
    assert math.isclose(res.power_sum, float(np.sum(np.abs(a["y_clean"]) ** 2)), rel_tol=1e-12)
    assert_sums(res)
    assert res.profile.n_symbols == S and np.all(res.profile.bits_per_subcarrier == int(np.log2(st["M"])))
    assert_rows(rows_of(res.profile), stage_expect(st, a, a["Z"]), a["Z"], 1e-9, what=st["name"])
    for batch in (1, 3):
        rb = eng.run(S, st["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]), profile=True,
                     keep_symbols=S, batch=batch)
        assert (rb.bit_errors, rb.symbol_errors) == (res.bit_errors, res.symbol_errors)
        assert_identical(rb.profile, res.profile, f"batch {batch}")


# ---------------------------------------------------------------- 2. modem variants through Simulation
with open(os.path.join(GOLDEN, "runs_wide.json")) as _f:
    _WIDE = json.load(_f)
VARIANTS = [("cfg_d_n64_adaptive", 15.0), ("adaptive_psk_n64_p1_mmse", 15.0), ("next_scofdm_n64_qpsk_p1_zf", None),
            ("next_zp_n64_m16_p2_mmse", None), ("next_psk8_zp_scofdm_n64_p1_mmse", None),
            ("wide_n64_m1024_severe_mmse", None), ("wide_n64_adaptive_p1", 35.0)]


def golden_case(tag, snr):
    return next(c for c in load_runs() + _WIDE
                if c["tag"] == tag and (snr is None or c["params"]["snr_db"] == snr))


def seeded_simulation(case, **extra):
    """The reference's seeding recipe, as test_gpu_parity.seeded_run."""
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


@pytest.mark.parametrize("tag,snr", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_simulation_variants(gpu, tag, snr):
    case = golden_case(tag, snr)
    p, r = case["params"], case["result"]
    plain = seeded_simulation(case)
    got = seeded_simulation(case, subcarrier_profile=True, received_symbols_keep=1 << 30)
    keys = {"bit_errors_per_subcarrier", "symbol_errors_per_subcarrier", "error_power_per_subcarrier",
            "mer_db_per_subcarrier"}
    assert set(got) - set(plain) == keys and not keys & set(plain)
    assert (got["bit_errors"], got["symbol_errors"]) == (r["bit_errors"], r["symbol_errors"])
    be, se = got["bit_errors_per_subcarrier"], got["symbol_errors_per_subcarrier"]
    assert (int(be.sum()), int(se.sum())) == (r["bit_errors"], r["symbol_errors"])
    N = p["num_subcarriers"]
    scheme = p["constellation_scheme"]
    adaptive = p["adaptive_modulation_mode"] == "CAPACITY_BASED"
    orders = np.asarray(got["constellation_order_per_subcarrier"], np.int64)
    bk = np.array([int(o).bit_length() - 1 if o > 0 else 0 for o in orders], np.int64)
    total_bits = got["total_bits"]
    S = total_bits // int(bk.sum())
    Z = got["received_symbols"].reshape(S, N)
    tx = O.generate_bits(total_bits, Generator(PCG64(case["seed"])))
    idx = PE.tx_indices(np.frombuffer(tx, np.uint8), bk, S)
    # adaptive runs do not compare a trailing partial byte
    n_valid = (total_bits // 8) * 8 if adaptive else total_bits
    exp = PE.expected_rows(Z, idx, bk, n_valid, scheme)
    assert np.array_equal(be, exp["bit_errors"]) and np.array_equal(se, exp["symbol_errors"])
    ep = got["error_power_per_subcarrier"]
    assert np.all(np.abs(ep - exp["error_power"]) <= PE.power_bound(Z, exp["error_power"], 1e-9))
    off = bk == 0
    assert not be[off].any() and not se[off].any() and not ep[off].any()
    assert np.all(np.isnan(got["mer_db_per_subcarrier"][off]))
    np.testing.assert_allclose(got["mer_db_per_subcarrier"][~off], -10 * np.log10(ep[~off] / S), rtol=1e-12)


# ---------------------------------------------------------------- 3. n_valid_bits
def test_n_valid_bits_masks_the_profile_as_the_total(gpu):
    st = next(s for s in load_stages() if s["name"] == "n64_m16_severe_cp_mmse")
    total = st["S"] * st["N"] * int(np.log2(st["M"]))
    a, eng, res = stage_run(st, n_valid_bits=total - 5)
    assert_sums(res)
    exp = stage_expect(st, a, a["Z"], total - 5)
    assert res.bit_errors == int(exp["bit_errors"].sum())
    assert_rows(rows_of(res.profile), exp, a["Z"], 1e-9, what="n_valid_bits")


# ---------------------------------------------------------------- 4. complex64, generic kernel
def test_complex64_generic_kernel(gpu):
    st = next(s for s in load_stages() if s["name"] == "n64_m16_severe_cp_mmse")
    a, eng, res = stage_run(st, precision=B.OFDM_F32)
    assert_sums(res)
    Z = res.received.reshape(st["S"], st["N"]).astype(np.complex128)
    exp = stage_expect(st, a, Z)
    # complex64 policy of test_f32_hot_path_tracks_reference: decision flips only at near-ties
    for k, tot in (("bit_errors", res.bit_errors), ("symbol_errors", res.symbol_errors)):
        l1 = int(np.abs(getattr(res.profile, k) - exp[k]).sum())
        print(f"complex64 {k}: L1 difference {l1} of {tot}")
        assert l1 <= max(2, 2e-3 * tot)
    assert np.array_equal(res.profile.clipped, exp["clipped"])
    assert np.all(np.abs(res.profile.error_power - exp["error_power"]) <= PE.power_bound(Z, exp["error_power"], 1e-4))


# ---------------------------------------------------------------- 5. throughput streams, bench shapes
def throughput_engine(case):
    h, cp, orders = PE.case_channel(case)
    N = case["N"]
    if orders is None:
        luts, sc = [O.qam_lut(case["M"])], None
        bk = np.full(N, int(np.log2(case["M"])), np.int64)
    else:
        luts, sc = AdaptiveConstellationMapper(orders, QAMConstellationMapper, N).lut_tables()
        bk = np.array([int(o).bit_length() - 1 if o > 0 else 0 for o in orders], np.int64)
    return LinkEngine(N, cp, h, EQ[case["eq"]], luts, sc, B.OFDM_F64), bk


@pytest.mark.parametrize("case", PE.THROUGHPUT_CASES, ids=lambda c: c["id"])
def test_throughput_streams_on_the_bench_shapes(gpu, case):
    eng, bk = throughput_engine(case)
    N, S, snr = case["N"], case["S"], case["snr"]
    plain = eng.run(S, snr, seed=PE.SEED)                                  # (i) the throughput receiver
    prof = eng.run(S, snr, seed=PE.SEED, profile=True)                     # (ii)
    tap = eng.run(S, snr, seed=PE.SEED, profile=True, keep_symbols=S)      # (iii) with the received symbols
    print(f"{case['id']}: {plain.bit_errors} / {plain.symbol_errors} (oracle {case['bit_errors']} / "
          f"{case['symbol_errors']})")
    assert plain.profile is None
    assert (prof.bit_errors, prof.symbol_errors) == (plain.bit_errors, plain.symbol_errors)
    assert plain.bit_errors > 100
    assert_sums(prof)
    assert_sums(tap)
    Z = tap.received.reshape(S, N)
    # (ii) against (iii): a wrong element-to-subcarrier map shows here
    assert_rows(rows_of(prof.profile), rows_of(tap.profile), Z, 1e-9, 2.0, what="profile against tapped run")
    idx = P.tx_indices(P.lane_generators(PE.SEED, np.arange(S), N), S, N, bk if case["M"] == 0 else int(bk[0]))
    exp = PE.expected_rows(Z, idx, bk, eng.valid_bits(S))
    assert_rows(rows_of(tap.profile), exp, Z, 1e-9, what="tapped run against the helper")
    off = bk == 0
    assert not prof.profile.error_power_fx[:, off].any() and not prof.profile.bit_errors[off].any()
    batched = eng.run(S, snr, seed=PE.SEED, profile=True, batch=50)
    assert (batched.bit_errors, batched.symbol_errors) == (prof.bit_errors, prof.symbol_errors)
    assert_identical(batched.profile, prof.profile, "batch 50")


# ---------------------------------------------------------------- 6. two gloo ranks on device 0
def test_two_ranks_hold_the_one_rank_profile(gpu, tmp_path):
    case = PE.THROUGHPUT_CASES[1]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OFDM_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = tmp_path / "profile"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(ROOT, "tests", "profile_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    eng, _ = throughput_engine(case)
    one = eng.run(case["S"], case["snr"], seed=PE.SEED, profile=True)
    rec = np.concatenate([np.stack([one.profile.bit_errors, one.profile.symbol_errors]), one.profile.error_power_fx,
                          one.profile.clipped[None]])
    for rank in (0, 1):
        got = json.loads((tmp_path / f"profile.{rank}.json").read_text())
        assert got["world"] == 2 and got["shard"] == [[0, 81], [81, 163]][rank]
        assert got["totals"] == [one.bit_errors, one.symbol_errors]
        assert np.array_equal(np.asarray(got["record"], np.int64), rec), rank

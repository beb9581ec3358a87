"""Receiver decisions on spectral-null and deep-fade subcarriers, on the GPU against the reference
(tests/golden/make_golden_nulls.py; the expectations are grounded in tests/test_null_bins_cpu.py).

A channel such as [1, -1] has a frequency response that is exactly 0 on one subcarrier, k0.  There
the reference's MMSE output is an exact zero -- a four-way tie of every square QAM that its
first-index argmin decides (null_expect.ORIGIN_INDEX: the lower central level on I, the upper on Q)
-- and its ZF output is the noise divided by 1e-10: level coordinates beyond 2^31, an error power at
the profile's cap, a point outside every density grid.  Every receiver form is held to the reference's
decision on that subcarrier: Simulation.run in both precisions, the fused engine and the operators on
the stage fixtures, the profile, frame and density records of the generic kernels, and the throughput
forms (Philox streams, the bench shapes with the channel swapped for [1, -1]) against
oracle/philox_streams.py.

On the commit before the zero-component rule 51 of the tests here fail, every one
on an MMSE null bin: the Simulation.run cases by 2 to 10 bits, ofdm_demap_count at every order, the
profile and frame records of the MMSE stage fixtures, and the N = 1024 64-QAM throughput forms.  The
ZF cases pass there too and are the pin.
"""

import math

import numpy as np
import pytest
import torch
from conftest import stage_arrays

import density_expect as DE
import frames_expect as FE
import null_expect as NE
import ofdm_oracle as O
import operator_expect as OE
import philox_streams as P
import profile_expect as PE
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.constellation.adaptive import AdaptiveConstellationMapper
from ofdm_based_systems.constellation.models import QAMConstellationMapper
from ofdm_based_systems.engine import LinkEngine

pytestmark = pytest.mark.gpu

RUNS = NE.load_runs()
STAGES = NE.load_stages()
EQ = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}
PRECS = pytest.mark.parametrize("prec", [B.OFDM_F64, B.OFDM_F32], ids=["complex128", "complex64"])
STAGE_IDS = dict(ids=lambda s: s["name"])


def popcount_sum(v):
    return int(sum(bin(int(x)).count("1") for x in np.asarray(v).ravel()))


# ---------------------------------------------------------------- 1. Simulation.run
@pytest.mark.parametrize("c", RUNS, ids=NE.run_id)
def test_simulation_run_matches_reference(gpu, c):
    """The assertions of test_gpu_parity.test_simulation_run_matches_reference."""
    r = c["result"]
    got = NE.seeded_run(c)
    print(f"{c['tag']}: {got['bit_errors']} / {got['symbol_errors']} (reference {r['bit_errors']} / {r['symbol_errors']})")
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


@pytest.mark.parametrize("c", RUNS, ids=NE.run_id)
def test_f32_tracks_reference(gpu, c):
    """complex64 with the reference's streams: test_gpu_parity.test_f32_hot_path_tracks_reference's rule.
    A null bin decided otherwise than the reference decides it moves the counts by tens of bits."""
    r = c["result"]
    got = NE.seeded_run(c, precision="f32")
    print(f"{c['tag']} complex64: {got['bit_errors']} / {got['symbol_errors']} "
          f"(reference {r['bit_errors']} / {r['symbol_errors']})")
    assert abs(got["bit_errors"] - r["bit_errors"]) <= max(2, 2e-3 * r["bit_errors"])
    assert abs(got["symbol_errors"] - r["symbol_errors"]) <= max(2, 2e-3 * r["symbol_errors"])
    assert math.isclose(got["papr_db"], r["papr_db"], rel_tol=1e-5)


def test_waterfilling_run_refuses_the_null_channel(gpu):
    c = dict(next(c for c in RUNS if c["tag"] == "null_n64_adaptive_uniform_dc"))
    c["params"] = dict(c["params"], power_allocation_type="WATERFILLING")
    with pytest.raises(ValueError, match="All channel gains must be positive"):
        NE.seeded_run(c)


# ---------------------------------------------------------------- 2. the plan's response
@PRECS
@pytest.mark.parametrize("kind", ["null_dc", "null_half", "null_quarter"])
def test_plan_response_is_exactly_zero_on_the_null_bin(gpu, kind, prec):
    """Without an exact zero in the plan's own H no case here would test a null bin."""
    h = NE.null_taps(kind)
    for N in (8, 64, 1024, 4096):
        k0 = {"null_dc": 0, "null_half": N // 2, "null_quarter": N // 4}[kind]
        plan = B.Plan(n_fft=N, cp=1, precision=prec, equalizer=B.EQ_MMSE, luts=[O.qam_lut(4)], h_raw=h)
        H = torch.empty(N, dtype=torch.complex128, device=gpu)
        B.check(B.lib().ofdm_plan_response(plan.handle, B.stream_ptr(), B.ptr(H), None))
        H = H.cpu().numpy()
        want = np.fft.fft(h, N)
        assert want[k0] == 0 and H[k0].real == 0 and H[k0].imag == 0, (kind, N, H[k0])
        assert np.count_nonzero(H == 0) == 1
        np.testing.assert_allclose(H, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("c", [c for c in RUNS if c["k0"] is not None and c["params"]["num_subcarriers"] == 64][:3]
                         + [c for c in RUNS if c["params"]["num_subcarriers"] > 64], ids=NE.run_id)
def test_plan_response_zero_on_the_recorded_bins(gpu, c):
    N = c["params"]["num_subcarriers"]
    plan = B.Plan(n_fft=N, cp=1, equalizer=B.EQ_MMSE, luts=[O.qam_lut(4)], h_raw=NE.taps(c))
    H = torch.empty(N, dtype=torch.complex128, device=gpu)
    B.check(B.lib().ofdm_plan_response(plan.handle, B.stream_ptr(), B.ptr(H), None))
    assert H.cpu().numpy()[c["k0"]] == 0


# ---------------------------------------------------------------- 3. stage fixtures, the fused engine
def stage_engine(st, prec=B.OFDM_F64):
    a = stage_arrays(st["name"])
    return a, LinkEngine(st["N"], st["cp"], a["h_raw"], EQ[st["eq"]], [O.qam_lut(st["M"])], precision=prec)


def stage_run(st, prec=B.OFDM_F64, **kw):
    a, eng = stage_engine(st, prec)
    S = st["S"]
    res = eng.run(S, st["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]), keep_symbols=S, **kw)
    return a, eng, res


def stage_indices(st, a):
    N, S, b = st["N"], st["S"], int(np.log2(st["M"]))
    bk = np.full(N, b, np.int64)
    return bk, PE.tx_indices(a["tx_bytes"], bk, S)


def null_bin_counts(st, a):
    """(bit errors, symbol errors) of the null bin's S symbols as the reference decides them."""
    _, idx = stage_indices(st, a)
    k0 = st["k0"]
    diff = O.nn_demap(a["Z"][:, k0], O.qam_lut(st["M"])) ^ idx[:, k0]
    return popcount_sum(diff), int(np.count_nonzero(diff))


@pytest.mark.parametrize("st", STAGES, **STAGE_IDS)
def test_fused_engine_stage_parity(gpu, st):
    """test_gpu_parity.test_fused_engine_stage_parity's assertions, and the null bin itself."""
    a, eng, res = stage_run(st)
    S, N, k0 = st["S"], st["N"], st["k0"]
    print(f"{st['name']}: {res.bit_errors} / {res.symbol_errors} (reference {st['bit_errors']} / {st['symbol_errors']})")
    Z = res.received.reshape(S, N)
    if st["eq"] == "MMSE":
        assert np.all(Z[:, k0].real == 0) and np.all(Z[:, k0].imag == 0)
    np.testing.assert_allclose(res.received, a["Z"].ravel(), rtol=1e-9, atol=1e-9)
    assert math.isclose(res.papr_db, st["papr_db"], rel_tol=1e-12)
    assert math.isclose(res.power_sum, float(np.sum(np.abs(a["y_clean"]) ** 2)), rel_tol=1e-12)
    assert res.bit_errors == st["bit_errors"]
    assert res.symbol_errors == st["symbol_errors"]


@pytest.mark.parametrize("st", STAGES, **STAGE_IDS)
def test_fused_engine_stage_complex64(gpu, st):
    """complex64: an exact zero on an MMSE null bin too, the noise's signs on a ZF one, and the counts
    under the project's complex64 rule."""
    a, eng, res = stage_run(st, B.OFDM_F32)
    S, N, k0 = st["S"], st["N"], st["k0"]
    Z = res.received.reshape(S, N)
    assert Z.dtype == np.complex64
    if st["eq"] == "MMSE":
        assert np.all(Z[:, k0].real == 0) and np.all(Z[:, k0].imag == 0)
    else:
        assert np.array_equal(np.sign(Z[:, k0].real), np.sign(a["Z"][:, k0].real))
        assert np.array_equal(np.sign(Z[:, k0].imag), np.sign(a["Z"][:, k0].imag))
        np.testing.assert_allclose(Z[:, k0], a["Z"][:, k0], rtol=1e-3)
    print(f"{st['name']} complex64: {res.bit_errors} / {res.symbol_errors} "
          f"(reference {st['bit_errors']} / {st['symbol_errors']})")
    assert abs(res.bit_errors - st["bit_errors"]) <= max(2, 2e-3 * st["bit_errors"])
    assert abs(res.symbol_errors - st["symbol_errors"]) <= max(2, 2e-3 * st["symbol_errors"])


# ---------------------------------------------------------------- 4. stage fixtures, the operators
def dev(a, plan):
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return (t.to(plan.cdtype) if np.iscomplexobj(a) else t).to("cuda")


def run_demap(plan, z, b):
    n_bytes = (len(z) * b + 7) // 8
    out = torch.full((n_bytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    d = dev(z, plan)
    B.check(B.lib().ofdm_demap(plan.handle, B.stream_ptr(), B.ptr(d), len(z), B.ptr(out)))
    o = out.cpu().numpy()
    assert np.all(o[n_bytes:] == 0xA5)
    return o[:n_bytes].tobytes()


@PRECS
@pytest.mark.parametrize("st", STAGES, **STAGE_IDS)
def test_equalize_on_stage_fixture(gpu, st, prec):
    a = stage_arrays(st["name"])
    N, cp, k0 = st["N"], st["cp"], st["k0"]
    Y = OE.round_input(np.fft.fft(a["y"].reshape(-1, N + cp)[:, cp:], axis=1, norm="ortho"), prec)
    # (H as the fixture holds it: beside the null the taps' DFT cancels, and the plan's own differs from
    # NumPy's by more than the equaliser's 40u; test_plan_response_* hold the plan's H to its zero)
    plan = B.Plan(n_fft=N, cp=cp, precision=prec, equalizer=EQ[st["eq"]], H=a["H"])
    d = dev(Y, plan)
    out = torch.full(Y.shape, float("nan"), dtype=plan.cdtype, device="cuda")
    B.check(B.lib().ofdm_equalize(plan.handle, B.stream_ptr(), B.ptr(d), Y.shape[0], st["snr_db"], B.ptr(out)))
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got.view(got.real.dtype)))
    assert OE.cmp_equalize(got, Y, a["H"], st["eq"], st["snr_db"], prec) <= 1
    if st["eq"] == "MMSE":
        assert np.all(got[:, k0].real == 0) and np.all(got[:, k0].imag == 0)
    else:
        np.testing.assert_allclose(got[:, k0], Y[:, k0] * 1e10, rtol=40 * OE.unit(prec), atol=0)
    if prec == B.OFDM_F64:
        np.testing.assert_allclose(got, a["Z"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("st", STAGES, **STAGE_IDS)
def test_demap_on_stage_fixture(gpu, st):
    """ofdm_demap and ofdm_demap_count on the reference's own Z: its bytes, its counts."""
    a = stage_arrays(st["name"])
    N, M, S = st["N"], st["M"], st["S"]
    b = int(np.log2(M))
    plan = B.Plan(n_fft=N, luts=[O.qam_lut(M)])
    assert run_demap(plan, a["Z"].ravel(), b) == a["rx_bytes"].tobytes()
    assert QAMConstellationMapper(M).decode(a["Z"].ravel()).read() == a["rx_bytes"].tobytes()
    Z = dev(a["Z"], plan)
    tx = torch.from_numpy(a["tx_bytes"].copy()).to(gpu)
    cnt = torch.zeros(2, dtype=torch.int64, device=gpu)
    B.check(B.lib().ofdm_demap_count(plan.handle, B.stream_ptr(), B.ptr(Z), B.ptr(tx), S, B.ptr(cnt)))
    assert tuple(cnt.cpu().tolist()) == (st["bit_errors"], st["symbol_errors"])


def null_bin_points(st):
    """What a null bin holds: the fixture's own column (signed zeros under MMSE, the noise over 1e-10
    under ZF), and every signed zero."""
    a = stage_arrays(st["name"])
    zeros = np.array([complex(0.0, 0.0), complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)])
    return np.concatenate([a["Z"][:, st["k0"]], zeros])


@PRECS
@pytest.mark.parametrize("m", [4, 16, 64, 256, 1024, 4096])
def test_demap_null_bin_points_at_every_order(gpu, m, prec):
    """The null-bin columns of all four fixtures through ofdm_demap at every square order (1024 and
    4096: the per-axis path), in both precisions: zeros and points of 1e8 and more are what they were
    in complex128."""
    lut = O.qam_lut(m)
    b = int(np.log2(m))
    z = np.concatenate([null_bin_points(st) for st in STAGES])
    z = np.concatenate([z, z[: (-len(z)) % 8]])  # whole bytes at every b
    want = O.nn_demap(z, lut)
    assert np.count_nonzero(want == NE.ORIGIN_INDEX[m]) >= 12 + 4 * len(STAGES)
    plan = B.Plan(n_fft=64, precision=prec, luts=[lut])
    got = run_demap(plan, z, b)
    gidx = O.bits_to_indices(O.bytes_to_bits(got), b)[: len(z)]
    assert np.array_equal(gidx, want), (m, np.flatnonzero(gidx != want)[:8], gidx[gidx != want][:8], want[gidx != want][:8])
    # ... and counted, as two OFDM symbols of 64: against all-zero bits the errors are the indices' own bits
    zc, S = np.resize(z, 128), 2
    wc = O.nn_demap(zc, lut)
    tx = torch.zeros((S * 64 * b + 7) // 8 + 8, dtype=torch.uint8, device=gpu)
    cnt = torch.zeros(2, dtype=torch.int64, device=gpu)
    B.check(B.lib().ofdm_demap_count(plan.handle, B.stream_ptr(), B.ptr(dev(zc, plan)), B.ptr(tx), S, B.ptr(cnt)))
    assert tuple(cnt.cpu().tolist()) == (popcount_sum(wc), int(np.count_nonzero(wc)))


@pytest.mark.parametrize("m", sorted(NE.PSK_ORIGIN_INDEX))
def test_psk_origin_decides_index_zero(gpu, m):
    z = np.array([0j, complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)] * 2)
    for prec in (B.OFDM_F64, B.OFDM_F32):
        plan = B.Plan(n_fft=64, precision=prec, luts=[O.psk_lut(m)])
        b = int(np.log2(m))
        got = O.bits_to_indices(O.bytes_to_bits(run_demap(plan, z, b)), b)[: len(z)]
        assert got.tolist() == [NE.PSK_ORIGIN_INDEX[m]] * len(z)


# ---------------------------------------------------------------- 5. records, the generic kernels
INT_ROWS = ("bit_errors", "symbol_errors", "clipped")


def stage_expect(st, a, Z):
    N, S, b = st["N"], st["S"], int(np.log2(st["M"]))
    bk, idx = stage_indices(st, a)
    return PE.expected_rows(Z, idx, bk, S * N * b)


@pytest.mark.parametrize("st", STAGES, **STAGE_IDS)
def test_profile_on_stage_fixture(gpu, st):
    a, eng, res = stage_run(st, profile=True)
    S, N, k0 = st["S"], st["N"], st["k0"]
    prof = res.profile
    exp = stage_expect(st, a, a["Z"])
    nb, ns = null_bin_counts(st, a)
    print(f"{st['name']}: null bin {int(prof.bit_errors[k0])} / {int(prof.symbol_errors[k0])} (reference {nb} / {ns}), "
          f"clipped {int(prof.clipped[k0])}, limbs {prof.error_power_fx[:, k0].tolist()}")
    assert (int(prof.bit_errors[k0]), int(prof.symbol_errors[k0])) == (nb, ns) == (
        int(exp["bit_errors"][k0]), int(exp["symbol_errors"][k0]))
    if st["eq"] == "ZF":
        assert int(prof.clipped[k0]) == S
        assert tuple(int(v) for v in prof.error_power_fx[:, k0]) == NE.fx_limbs(S * NE.CAP)
        assert prof.error_power[k0] == S * NE.CAP
    else:
        assert int(prof.clipped[k0]) == 0
    for k in INT_ROWS:
        assert np.array_equal(getattr(prof, k), exp[k]), (k, np.flatnonzero(getattr(prof, k) != exp[k])[:8])
    bound = PE.power_bound(a["Z"], exp["error_power"], 1e-9)
    assert np.all(np.abs(prof.error_power - exp["error_power"]) <= bound)
    assert int(prof.bit_errors.sum()) == res.bit_errors == st["bit_errors"]
    assert int(prof.symbol_errors.sum()) == res.symbol_errors == st["symbol_errors"]


@pytest.mark.parametrize("st", STAGES, **STAGE_IDS)
def test_profile_null_bin_rows_complex64(gpu, st):
    """Rows 0 and 1 on the null bin are exact in complex64 too: an exact zero (MMSE) or a point the
    noise's sign decides (ZF) leaves the precision nothing to flip."""
    a, eng, res = stage_run(st, B.OFDM_F32, profile=True)
    S, k0 = st["S"], st["k0"]
    nb, ns = null_bin_counts(st, a)
    prof = res.profile
    print(f"{st['name']} complex64: null bin {int(prof.bit_errors[k0])} / {int(prof.symbol_errors[k0])} "
          f"(reference {nb} / {ns})")
    assert (int(prof.bit_errors[k0]), int(prof.symbol_errors[k0])) == (nb, ns)
    assert int(prof.clipped[k0]) == (S if st["eq"] == "ZF" else 0)
    if st["eq"] == "ZF":
        assert tuple(int(v) for v in prof.error_power_fx[:, k0]) == NE.fx_limbs(S * NE.CAP)


@pytest.mark.parametrize("st", STAGES, **STAGE_IDS)
def test_frames_on_stage_fixture(gpu, st):
    a, eng, res = stage_run(st, frame_symbols=3)
    S, N, b = st["S"], st["N"], int(np.log2(st["M"]))
    bk, idx = stage_indices(st, a)
    be, se = FE.per_symbol_from_z(a["Z"], idx, bk, S * N * b)
    fr = res.frames
    assert fr.frame_symbols == 3 and fr.n_symbols == S
    assert np.array_equal(fr.bit_errors, FE.frame_sums(be, 3)), (fr.bit_errors, FE.frame_sums(be, 3))
    assert np.array_equal(fr.symbol_errors, FE.frame_sums(se, 3))
    assert (int(fr.bit_errors.sum()), int(fr.symbol_errors.sum())) == (st["bit_errors"], st["symbol_errors"])


def flat(d):
    return np.concatenate([d.counts.ravel(), [d.outside]]).astype(np.int64)


@PRECS
@pytest.mark.parametrize("st", STAGES, **STAGE_IDS)
def test_density_on_stage_fixture(gpu, st, prec):
    """The whole symbol exactly against the run's own tap; the null bin alone exactly against the
    fixture: outside under ZF, on the grid line at the origin -- bin (16, 16) -- under MMSE."""
    S, N, k0 = st["S"], st["N"], st["k0"]
    a, eng, res = stage_run(st, prec, density=32)
    L = 1.5 * eng.lut_reach
    d = res.density
    c, o = DE.bin_points(res.received.reshape(S, N), 32, L)
    assert d.extent == L and d.n_points == S * N
    assert np.array_equal(d.counts, c) and d.outside == o
    one = eng.run(S, st["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]), density=32,
                  density_subcarriers=(k0, k0 + 1)).density
    c0, o0 = DE.bin_points(a["Z"], 32, L, k_lo=k0, k_hi=k0 + 1)
    assert np.array_equal(one.counts, c0) and one.outside == o0 and one.n_points == S
    if st["eq"] == "ZF":
        assert one.outside == S and d.outside >= S
    else:
        assert one.outside == 0 and int(one.counts[16, 16]) == S


# ---------------------------------------------------------------- 6. throughput forms, Philox streams
SEED = PE.SEED
NULL_H = NE.null_taps("null_dc")
# the bench shapes of PE.THROUGHPUT_CASES, the channel swapped for [1, -1] under MMSE, a handful of
# symbols: more than one workgroup, a partial last one (4 / 2 / 1 symbols per workgroup)
THROUGHPUT = [dict(c, id=c["id"].split("_")[0] + ("_adaptive" if c["M"] == 0 else f"_m{c['M']}") + "_null_dc_mmse",
                   eq="MMSE", S=s)
              for c, s in zip(PE.THROUGHPUT_CASES[1:], (9, 7, 5))]
SWEEP_OFFSETS = (-4.0, 0.0, 3.0)


def gpu_radius(words):
    w = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to("cuda")
    r = torch.empty(w.numel(), dtype=torch.float32, device="cuda")
    B.check(B.lib().ofdm_noise_radius(B.stream_ptr(), B.ptr(w), w.numel(), B.ptr(r)))
    return r.cpu().numpy()


def null_engine(case):
    N = case["N"]
    if case["M"]:
        orders, luts, sc = None, [O.qam_lut(case["M"])], None
        bk = np.full(N, int(np.log2(case["M"])), np.int64)
    else:
        # water-filling refuses the zero gain: CAPACITY_BASED loading at uniform power, which leaves the
        # null bin and its neighbourhood unloaded
        orders, _, _ = O.adaptive_orders(N, NULL_H, case["snr"], 1e-3, False)
        assert orders[0] == 0 and orders.max() <= 256
        luts, sc = AdaptiveConstellationMapper(orders, QAMConstellationMapper, N).lut_tables()
        bk = np.array([int(o).bit_length() - 1 if o > 0 else 0 for o in orders], np.int64)
    return LinkEngine(N, 1, NULL_H, B.EQ_MMSE, luts, sc, B.OFDM_F64), bk, orders


def oracle_counts(case, S, snr, orders, power_sum, sym0=0, total_samples=None):
    """The oracle's run and the bracket a complex128 GPU run's counts must lie in: the decision bracket
    of every subcarrier but the null bin (its points are exact zeros on both sides, which the bracket
    would call undecided), plus the null bin's counts as the reference's first-index rule decides them."""
    N, M = case["N"], case["M"]
    ref = P.run_philox(SEED, S, N, M, NULL_H, 1, "MMSE", snr, precision="f64", radius_fn=gpu_radius,
                       power_sum=power_sum, orders=orders, sym0=sym0, total_samples=total_samples)
    assert np.all(ref.z[:, 0] == 0)
    if orders is not None:  # the null bin is unloaded: nothing is decided there
        return ref, ref.bracket
    lut, b = O.qam_lut(M), int(np.log2(M))
    lo = P.decision_bracket(ref.z[:, 1:], ref.idx[:, 1:], lut, b, ref.delta[:, 1:])
    diff = ref.idx[:, 0] ^ NE.ORIGIN_INDEX[M]
    nb, ns = popcount_sum(diff), int(np.count_nonzero(diff))
    return ref, (lo[0] + nb, lo[1] + nb, lo[2] + ns, lo[3] + ns)


def assert_in(res, ref, br, what):
    print(f"{what}: bits {res.bit_errors} in [{br[0]}, {br[1]}], symbols {res.symbol_errors} in [{br[2]}, {br[3]}] "
          f"(oracle {ref.bit_errors} / {ref.symbol_errors})")
    assert br[0] <= ref.bit_errors <= br[1] and br[2] <= ref.symbol_errors <= br[3]
    assert br[1] - br[0] <= max(2, ref.bit_errors // 1000) and br[3] - br[2] <= max(2, ref.bit_errors // 1000)
    assert br[0] <= res.bit_errors <= br[1], what
    assert br[2] <= res.symbol_errors <= br[3], what


_THROUGHPUT_RUNS = {}


def throughput_runs(case):
    """The case's engine, its plain run, its tapped profile run and the oracle at the case's SNR, once."""
    if case["id"] not in _THROUGHPUT_RUNS:
        eng, bk, orders = null_engine(case)
        S, snr = case["S"], case["snr"]
        plain = eng.run(S, snr, seed=SEED, fused=False)
        tap = eng.run(S, snr, seed=SEED, profile=True, keep_symbols=S)
        ref, br = oracle_counts(case, S, snr, orders, plain.power_sum)
        _THROUGHPUT_RUNS[case["id"]] = (eng, bk, orders, plain, tap, ref, br)
    return _THROUGHPUT_RUNS[case["id"]]


@pytest.mark.parametrize("case", THROUGHPUT, ids=lambda c: c["id"])
def test_throughput_rx_against_the_oracle(gpu, case):
    eng, bk, orders, plain, tap, ref, br = throughput_runs(case)
    S, N, snr = case["S"], case["N"], case["snr"]
    assert ref.bit_errors > 100
    assert_in(plain, ref, br, case["id"] + " ofdm_rx")
    assert_in(eng.run(S, snr, seed=SEED), ref, br, case["id"] + " default route")
    assert_in(tap, ref, br, case["id"] + " generic kernel (tap)")
    Z = tap.received.reshape(S, N)
    assert np.all(Z[:, 0].real == 0) and np.all(Z[:, 0].imag == 0)
    assert np.all(np.abs(Z - ref.z) <= ref.delta + 1e-9 * (1 + np.abs(ref.z)))


@pytest.mark.parametrize("case", THROUGHPUT, ids=lambda c: c["id"])
def test_throughput_profile_rows(gpu, case):
    eng, bk, orders, plain, tap, ref, br = throughput_runs(case)
    S, N, snr = case["S"], case["N"], case["snr"]
    prof = eng.run(S, snr, seed=SEED, profile=True)
    assert_in(prof, ref, br, case["id"] + " ofdm_rx_profile")
    assert (prof.bit_errors, prof.symbol_errors) == (plain.bit_errors, plain.symbol_errors)
    Z = tap.received.reshape(S, N)
    exp = PE.expected_rows(Z, ref.idx, bk, eng.valid_bits(S))
    for p, what in ((tap.profile, "tapped"), (prof.profile, "throughput form")):
        assert int(p.bit_errors.sum()) == plain.bit_errors and int(p.symbol_errors.sum()) == plain.symbol_errors
        print(f"{case['id']} {what}: null bin {int(p.bit_errors[0])} / {int(p.symbol_errors[0])} "
              f"(expected {int(exp['bit_errors'][0])} / {int(exp['symbol_errors'][0])})")
        for k in INT_ROWS:
            assert int(getattr(p, k)[0]) == int(exp[k][0]), (what, k)
            assert np.array_equal(getattr(p, k), exp[k]), (what, k, np.flatnonzero(getattr(p, k) != exp[k])[:8])
        factor = 1.0 if p is tap.profile else 2.0
        assert np.all(np.abs(p.error_power - exp["error_power"]) <= PE.power_bound(Z, exp["error_power"], 1e-9, factor))
    if orders is None:  # the null bin's rows are the origin's point against the transmitted indices
        diff = ref.idx[:, 0] ^ NE.ORIGIN_INDEX[case["M"]]
        assert (int(prof.profile.bit_errors[0]), int(prof.profile.symbol_errors[0])) == (
            popcount_sum(diff), int(np.count_nonzero(diff)))
        want = float(np.sum(np.abs(O.qam_lut(case["M"])[ref.idx[:, 0]]) ** 2))
        assert abs(prof.profile.error_power[0] - want) <= S * 2.0 ** -40 + 1e-12 * want
    else:
        assert not prof.profile.bit_errors[0] and not prof.profile.error_power_fx[:, 0].any()


@pytest.mark.parametrize("case", THROUGHPUT, ids=lambda c: c["id"])
def test_throughput_frames(gpu, case):
    eng, bk, orders, plain, tap, ref, br = throughput_runs(case)
    S, N, snr = case["S"], case["N"], case["snr"]
    res = eng.run(S, snr, seed=SEED, frame_symbols=3)
    assert (res.bit_errors, res.symbol_errors) == (plain.bit_errors, plain.symbol_errors)
    be, se = FE.per_symbol_from_z(tap.received.reshape(S, N), ref.idx, bk, eng.valid_bits(S))
    assert np.array_equal(res.frames.bit_errors, FE.frame_sums(be, 3))
    assert np.array_equal(res.frames.symbol_errors, FE.frame_sums(se, 3))


@pytest.mark.parametrize("case", THROUGHPUT, ids=lambda c: c["id"])
def test_throughput_density(gpu, case):
    eng, bk, orders, plain, tap, ref, br = throughput_runs(case)
    S, N, snr, G = case["S"], case["N"], case["snr"], 32
    L = 1.5 * eng.lut_reach
    active = bk > 0
    res = eng.run(S, snr, seed=SEED, density=G)
    assert (res.bit_errors, res.symbol_errors) == (plain.bit_errors, plain.symbol_errors)
    d = res.density
    assert d.n_points == S * int(np.count_nonzero(active)) == int(d.counts.sum()) + d.outside
    # every subcarrier but the null bin inside the oracle's bracket; the null bin's exact zeros lie on
    # the grid line at the origin and land in bin (G/2, G/2), S of them
    rest = active.copy()
    rest[0] = False
    dec, maybe = DE.bracket(ref.z, ref.delta, G, L, active=rest)
    got = flat(d)
    if active[0]:
        origin, _ = DE.bin_points(np.zeros((S, 1), np.complex128), G, L)
        assert origin[G // 2, G // 2] == S
        got[:-1] -= origin.ravel()
        one = eng.run(S, snr, seed=SEED, density=G, density_subcarriers=(0, 1)).density
        assert np.array_equal(one.counts, origin) and one.outside == 0
    over = got - dec
    assert np.all(over >= 0) and np.all(over <= maybe), np.flatnonzero((over < 0) | (over > maybe))[:8]


@pytest.mark.parametrize("case", [c for c in THROUGHPUT if c["M"]], ids=lambda c: c["id"])
def test_throughput_sweep(gpu, case):
    eng, bk, orders, plain, tap, ref, br = throughput_runs(case)
    S, snr = case["S"], case["snr"]
    snrs = [snr + o for o in SWEEP_OFFSETS]
    sweep = eng.run_sweep(S, snrs, seed=SEED)
    for q, pt in zip(snrs, sweep):
        r, b = (ref, br) if q == snr else oracle_counts(case, S, q, orders, plain.power_sum)
        assert_in(pt, r, b, f"{case['id']} sweep point {q} dB")
        one = eng.run(S, q, seed=SEED, fused=False)
        assert (pt.bit_errors, pt.symbol_errors) == (one.bit_errors, one.symbol_errors)


class Stream:
    """The transmitted stream of a case, kept, and its receivers over any piece of it."""

    def __init__(self, eng, S, snr):
        self.eng, self.S, self.snr = eng, S, snr
        self.samples = S * (eng.n_fft + eng.cp)
        self.y = eng._y(S)
        self.stats = E.new_stats(eng.device())
        eng.tx(eng.stream(), None, SEED, 0, S, self.y, self.stats)

    def rx(self, sym0, n, counters, **kw):
        self.eng.rx(self.eng.stream(), self.y[sym0:], None, None, SEED, self.stats, self.samples, self.snr, True, None,
                    sym0, n, self.eng.valid_bits(self.S), counters, **kw)


@pytest.mark.parametrize("case", THROUGHPUT, ids=lambda c: c["id"])
def test_two_calls_split_at_an_odd_symbol_add_up(gpu, case):
    eng, bk, orders, plain, tap, ref, br = throughput_runs(case)
    S, N, snr = case["S"], case["N"], case["snr"]
    st = Stream(eng, S, snr)
    dev_ = eng.device()
    whole = torch.zeros(2, dtype=torch.int64, device=dev_)
    parts = torch.zeros(2, dtype=torch.int64, device=dev_)
    st.rx(0, S, whole)
    st.rx(0, 3, parts)
    st.rx(3, S - 3, parts)
    pw = torch.zeros((B.PROFILE_ROWS, N), dtype=torch.int64, device=dev_)
    pp = torch.zeros((B.PROFILE_ROWS, N), dtype=torch.int64, device=dev_)
    cw = torch.zeros(2, dtype=torch.int64, device=dev_)
    cp_ = torch.zeros(2, dtype=torch.int64, device=dev_)
    st.rx(0, S, cw, profile=pw)
    st.rx(0, 3, cp_, profile=pp)
    st.rx(3, S - 3, cp_, profile=pp)
    sw = torch.zeros((3, 2), dtype=torch.int64, device=dev_)
    sp = torch.zeros((3, 2), dtype=torch.int64, device=dev_)
    if orders is None:
        snrs = [snr + o for o in SWEEP_OFFSETS]
        eng.rx_sweep(eng.stream(), st.y, SEED, st.stats, st.samples, snrs, 0, S, eng.valid_bits(S), sw)
        eng.rx_sweep(eng.stream(), st.y, SEED, st.stats, st.samples, snrs, 0, 3, eng.valid_bits(S), sp)
        eng.rx_sweep(eng.stream(), st.y[3:], SEED, st.stats, st.samples, snrs, 3, S - 3, eng.valid_bits(S), sp)
    torch.cuda.synchronize()
    assert whole.tolist() == parts.tolist() == cw.tolist() == cp_.tolist() == [plain.bit_errors, plain.symbol_errors]
    a, b = E.combine_profile([pw.cpu().numpy()]), E.combine_profile([pp.cpu().numpy()])
    assert np.array_equal(a, b), np.argwhere(a != b)[:8]
    assert torch.equal(sw, sp) and (orders is not None or sw[1].tolist() == whole.tolist())

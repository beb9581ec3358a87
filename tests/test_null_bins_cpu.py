"""Spectral-null and deep-fade channels without a GPU: the oracle reproduces the reference's runs and
stages over them exactly (tests/golden/make_golden_nulls.py), the first-index tie rule at the origin
is stated as a table and checked against the LUTs, the per-subcarrier, per-frame and density
restatements are run on the fixtures' own symbols, and water-filling refuses a zero gain as the
reference does.  The expectations tests/test_gpu_null_bins.py holds the device to are grounded here."""

import hashlib
import math

import numpy as np
import pytest
from conftest import GOLDEN, stage_arrays

import density_expect as DE
import frames_expect as FE
import null_expect as NE
import ofdm_oracle as O
import profile_expect as PE
from ofdm_based_systems.constellation.adaptive import AdaptiveConstellationMapper
from ofdm_based_systems.constellation.models import QAMConstellationMapper
from ofdm_based_systems.power_allocation.models import WaterfillingPowerAllocation

RUNS = NE.load_runs()
STAGES = NE.load_stages()


def sha(b):
    return hashlib.sha256(b).hexdigest()[:16]


# ---------------------------------------------------------------- the fixtures themselves
def test_fixture_set_is_the_one_described():
    tags = [c["tag"] for c in RUNS]
    assert len(set(tags)) == len(tags)
    for eq in ("mmse", "zf"):
        for ch in ("dc", "half", "quarter"):
            for m in (4, 16, 64, 256):
                assert f"null_n64_m{m}_{ch}_{eq}" in tags
        assert f"null_n64_m1024_dc_{eq}" in tags and f"null_n64_m4096_dc_{eq}" in tags
        assert f"fade_n64_m64_dc_{eq}" in tags
    for t in ("null_n64_psk4_dc_mmse", "null_n64_psk8_dc_mmse", "null_scofdm_n64_m16_half_mmse",
              "null_zp_n64_m16_dc_mmse", "null_n64_adaptive_uniform_dc", "null_n1024_m64_dc_mmse",
              "null_n4096_m256_dc_mmse"):
        assert t in tags
    assert [(s["N"], s["S"], s["M"], s["eq"]) for s in STAGES] == [
        (8, 16, 16, "ZF"), (64, 8, 64, "MMSE"), (64, 8, 64, "ZF"), (1024, 4, 64, "MMSE")]


@pytest.mark.parametrize("c", RUNS, ids=NE.run_id)
def test_recorded_null_bin_is_an_exact_zero(c):
    h, N = NE.taps(c), c["params"]["num_subcarriers"]
    H = np.fft.fft(h, N)
    if c["k0"] is None:  # the deep fade: small, and no exact zero anywhere
        assert c["channel"] == "fade_dc" and np.all(H != 0) and 2e-4 < abs(H[0]) < 3e-4
        return
    assert H[c["k0"]] == 0 and np.count_nonzero(H == 0) == 1
    if "zf_null_bin" in c:
        assert c["zf_null_bin"]["min_abs_component"] > 1e-3 and c["zf_null_bin"]["share_above_2p31"] > 0.5


# ---------------------------------------------------------------- the oracle on the runs
@pytest.mark.parametrize("c", [c for c in RUNS if NE.is_plain_fixed_qam(c)], ids=NE.run_id)
def test_oracle_reproduces_the_fixed_runs(c):
    r = c["result"]
    res = NE.oracle_fixed_run(c)
    assert (res.bit_errors, res.symbol_errors, res.total_bits) == (r["bit_errors"], r["symbol_errors"], r["total_bits"])
    assert math.isclose(res.papr_db, r["papr_db"], rel_tol=1e-9)


def adaptive_case():
    return next(c for c in RUNS if c["tag"] == "null_n64_adaptive_uniform_dc")


def test_oracle_reproduces_the_adaptive_run_and_its_unloaded_bins():
    c = adaptive_case()
    p, r = c["params"], c["result"]
    h, N = NE.taps(c), p["num_subcarriers"]
    orders, power, wl = O.adaptive_orders(N, h, p["snr_db"], p["desired_symbol_error_rate"], False)
    assert orders.tolist() == r["constellation_order_per_subcarrier"] and wl is None and r["water_level"] is None
    np.testing.assert_array_equal(power, np.array(r["allocated_power"]))
    # the null bin and, in this run, its two neighbours carry nothing
    assert sorted(np.flatnonzero(orders == 0).tolist()) == [0, 1, 63]
    bps = sum(int(np.log2(o)) for o in orders if o > 0)
    S = p["num_symbols"]
    cp = O.prefix_length(h, p["prefix_length_ratio"], "CP")
    tx, nz = O.reference_streams(c["seed"], bps * S, S * (N + cp))
    res = O.run_adaptive(tx, orders, N, h, cp, "MMSE", p["snr_db"], nz)
    assert (res.bit_errors, res.symbol_errors, res.total_bits) == (r["bit_errors"], r["symbol_errors"], r["total_bits"])
    # this package's mapper leaves the order-0 bins inactive
    luts, sc = AdaptiveConstellationMapper(orders, QAMConstellationMapper, N).lut_tables()
    assert np.array_equal(sc < 0, orders == 0) and all(len(l) > 0 for l in luts)


# ---------------------------------------------------------------- the oracle on the stages
@pytest.mark.parametrize("st", STAGES, ids=lambda s: s["name"])
def test_oracle_reproduces_the_stages(st):
    a = stage_arrays(st["name"])
    N, M, cp, S, k0 = st["N"], st["M"], st["cp"], st["S"], st["k0"]
    b = int(np.log2(M))
    lut = O.qam_lut(M)
    tx = a["tx_bytes"].tobytes()
    assert sha(tx) == st["tx_sha"] and a["H"][k0] == 0
    X = lut[O.bits_to_indices(O.bytes_to_bits(tx), b)].reshape(-1, N)
    assert np.array_equal(X, a["X"])
    x = O.modulate(X, cp)
    np.testing.assert_allclose(x, a["x"], rtol=0, atol=1e-12)
    y = O.awgn(O.channel_conv(x.ravel(), a["h_raw"]), st["snr_db"], a["noise_re"], a["noise_im"])
    np.testing.assert_allclose(y, a["y"], rtol=0, atol=1e-12)
    # from the reference's own y the oracle's Z is the reference's to the last bit on the null bin
    Z = O.demodulate(a["y"].reshape(-1, N + cp), cp, a["H"], st["eq"], st["snr_db"])
    np.testing.assert_allclose(Z, a["Z"], rtol=1e-9, atol=1e-9)
    if st["eq"] == "MMSE":
        assert np.all(a["Z"][:, k0] == 0) and np.array_equal(Z[:, k0], a["Z"][:, k0])
        for part in (np.real, np.imag):  # the signed zeros
            assert np.array_equal(np.signbit(part(Z[:, k0])), np.signbit(part(a["Z"][:, k0])))
    else:
        assert np.array_equal(Z[:, k0], a["Z"][:, k0]) and np.all(np.abs(a["Z"][:, k0]) > 1e7)
    ridx = O.nn_demap(a["Z"].ravel(), lut)
    rx = O.indices_to_bytes(ridx, b)
    assert rx == a["rx_bytes"].tobytes() and sha(rx) == st["rx_sha"]
    # ... and the whole chain from the bytes and the normals gives the counts
    res = O.run_fixed(tx, S * N * b, N, M, a["h_raw"], cp, st["eq"], st["snr_db"], (a["noise_re"], a["noise_im"]))
    assert (res.bit_errors, res.symbol_errors) == (st["bit_errors"], st["symbol_errors"])
    assert sha(res.rx_bytes) == st["rx_sha"]
    if st["eq"] == "MMSE":  # every symbol of the null bin decides the origin's point
        assert np.all(ridx.reshape(S, N)[:, k0] == NE.ORIGIN_INDEX[M])


# ---------------------------------------------------------------- the tie rule
@pytest.mark.parametrize("m", sorted(NE.ORIGIN_INDEX))
def test_origin_decides_the_first_of_the_four_central_points(m):
    lut = O.qam_lut(m)
    if m <= 256:
        assert np.array_equal(lut, np.load(f"{GOLDEN}/luts.npz")[f"qam{m}"])
    else:
        assert np.array_equal(lut, QAMConstellationMapper(m).constellation)
    d = np.abs(0 - lut)
    tie = np.flatnonzero(d == d.min())
    assert len(tie) == 4 and NE.ORIGIN_INDEX[m] == tie[0] == int(np.argmin(d))
    for z in (complex(0.0, 0.0), complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)):
        assert O.nn_demap(np.array([z]), lut)[0] == NE.ORIGIN_INDEX[m]
    # per axis: I the lower of the two central levels, Q the upper; patterns from the index halves
    side, hb = int(np.sqrt(m)), int(np.log2(m)) // 2
    lev = np.unique(lut.real)
    c = lut[NE.ORIGIN_INDEX[m]]
    ki, kq = int(np.searchsorted(lev, c.real)), int(np.searchsorted(lev, c.imag))
    assert (ki, kq) == NE.ORIGIN_LEVELS[m] == (side // 2 - 1, side // 2)
    assert c.real < 0 < c.imag
    # the other three central points carry other I or Q patterns: the decision changes bits
    ipat, qpat = NE.ORIGIN_INDEX[m] & (side - 1), NE.ORIGIN_INDEX[m] >> hb
    others = [(int(t) & (side - 1), int(t) >> hb) for t in tie[1:]]
    assert all(o != (ipat, qpat) for o in others)
    assert {o[0] for o in others} - {ipat} and {o[1] for o in others} - {qpat}


@pytest.mark.parametrize("m", sorted(NE.PSK_ORIGIN_INDEX))
def test_psk_origin_decides_index_zero(m):
    lut = O.psk_lut(m)
    assert np.array_equal(lut, np.load(f"{GOLDEN}/luts.npz")[f"psk{m}"])
    assert O.nn_demap(np.array([0j, complex(-0.0, 0.0), complex(0.0, -0.0)]), lut).tolist() == [NE.PSK_ORIGIN_INDEX[m]] * 3


# ---------------------------------------------------------------- the record restatements on the fixtures' Z
def stage_indices(st, a):
    N, S, b = st["N"], st["S"], int(np.log2(st["M"]))
    bk = np.full(N, b, np.int64)
    return bk, PE.tx_indices(a["tx_bytes"], bk, S)


@pytest.mark.parametrize("st", STAGES, ids=lambda s: s["name"])
def test_profile_rows_on_the_null_bin(st):
    a = stage_arrays(st["name"])
    N, S, k0, b = st["N"], st["S"], st["k0"], int(np.log2(st["M"]))
    bk, idx = stage_indices(st, a)
    rows = PE.expected_rows(a["Z"], idx, bk, S * N * b)
    assert int(rows["bit_errors"].sum()) == st["bit_errors"] and int(rows["symbol_errors"].sum()) == st["symbol_errors"]
    others = np.arange(N) != k0
    assert not rows["clipped"][others].any()
    if st["eq"] == "ZF":
        assert rows["clipped"][k0] == S and rows["error_power"][k0] == S * NE.CAP
        assert NE.fx_limbs(S * NE.CAP) == (0, S << 28)
    else:
        assert rows["clipped"][k0] == 0
        # |0 - c|^2 of the transmitted points: between the innermost and the outermost point's power
        lut = O.qam_lut(st["M"])
        assert rows["error_power"][k0] == pytest.approx(float(np.sum(np.abs(lut[idx[:, k0]]) ** 2)), rel=1e-12)
        # the origin's point against the transmitted index, bit by bit
        diff = idx[:, k0] ^ NE.ORIGIN_INDEX[st["M"]]
        assert rows["symbol_errors"][k0] == np.count_nonzero(diff)
        assert rows["bit_errors"][k0] == sum(bin(int(d)).count("1") for d in diff)


@pytest.mark.parametrize("st", STAGES, ids=lambda s: s["name"])
def test_frame_rows_of_three_symbols(st):
    a = stage_arrays(st["name"])
    N, S, b = st["N"], st["S"], int(np.log2(st["M"]))
    bk, idx = stage_indices(st, a)
    be, se = FE.per_symbol_from_z(a["Z"], idx, bk, S * N * b)
    be2, se2 = FE.per_symbol_from_bytes(a["tx_bytes"], a["rx_bytes"], bk, S, S * N * b)
    assert np.array_equal(be, be2) and np.array_equal(se, se2)
    fb, fs = FE.frame_sums(be, 3), FE.frame_sums(se, 3)
    assert len(fb) == -(-S // 3) and (int(fb.sum()), int(fs.sum())) == (st["bit_errors"], st["symbol_errors"])


@pytest.mark.parametrize("st", STAGES, ids=lambda s: s["name"])
def test_density_counts_the_null_bin_outside_under_zf(st):
    a = stage_arrays(st["name"])
    N, S, k0 = st["N"], st["S"], st["k0"]
    lut = O.qam_lut(st["M"])
    L = 1.5 * float(max(np.max(np.abs(lut.real)), np.max(np.abs(lut.imag))))  # the engine's default extent
    counts, outside = DE.bin_points(a["Z"], 32, L)
    assert int(counts.sum()) + outside == S * N
    only, out0 = DE.bin_points(a["Z"], 32, L, k_lo=k0, k_hi=k0 + 1)
    if st["eq"] == "ZF":
        assert out0 == S and not only.any() and outside >= S
    else:
        # the origin sits on the grid line between bins 15 and 16: t = 16 exactly, bin (16, 16)
        assert out0 == 0 and only[16, 16] == S and int(only.sum()) == S


# ---------------------------------------------------------------- the receiver's route
def test_dispatch_model_sends_an_mmse_null_plan_to_the_generic_receiver():
    """Only the generic kernel's slicer holds the tie rule: an MMSE plan with a null bin leaves the
    throughput receivers, whatever the shape; its transmitter, and ZF or no equaliser, stay."""
    import dataclasses

    import dispatch_model as DM

    for N, bits in ((1024, 6), (4096, 8), (256, 4)):
        plain = DM.Plan(DM.F64, N, bits, L=2, cp=1, eq="MMSE")
        tx, rx = DM.dispatch(plain)
        assert rx[3:5] == (DM.EQ_CODE["MMSE"], bits)
        txn, rxn = DM.dispatch(dataclasses.replace(plain, null_bin=True))
        assert txn == tx and rxn == ("k_rx", "double", N.bit_length() - 1, -1, 0, True)
        for eq in ("ZF", "NONE"):
            assert DM.dispatch(dataclasses.replace(plain, eq=eq, null_bin=True)) == DM.dispatch(
                dataclasses.replace(plain, eq=eq))


# ---------------------------------------------------------------- water-filling
def test_waterfilling_refuses_a_zero_gain_as_the_reference_does():
    g = np.abs(np.fft.fft(NE.null_taps("null_dc"), 64)) ** 2
    assert g[0] == 0
    with pytest.raises(ValueError) as e:
        WaterfillingPowerAllocation(64.0, g, 1e-2)
    assert str(e.value) == NE.waterfilling_error()
    assert str(e.value).startswith("All channel gains must be positive")

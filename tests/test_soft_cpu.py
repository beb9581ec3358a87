"""The soft-decision record (ofdm_rx_soft, LinkEngine.run(soft=B), engine.SoftDecisions) without a GPU:
the entry point's declaration, export, binding and refusals; the NumPy restatement
(tests/soft_expect.py) on hand-made points; the sign of the max-log difference against the hard decisions
of every stage fixture and of the four throughput cases (the precondition of the GPU comparisons: no
value is exactly zero, the mass on the wrong side of zero is the pinned bit-error count, and few values
lie near a bin line); SoftDecisions' arithmetic; the GMI against the BPSK capacity by quadrature; the
engine's host-made quantities and the settings keys.

On the commit before the record everything here fails: there is no such entry point, engine has no
soft_grid and Simulation no soft_bins."""

import ctypes
import os
import re

import numpy as np
import pytest
from conftest import load_stages, stage_arrays

import density_expect as DE
import ofdm_oracle as O
import profile_expect as PE
import soft_expect as SE
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.configuration.models import SimulationSettings
from ofdm_based_systems.simulation.models import Simulation

RX_ARGS = 17  # ofdm_rx's
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------- the ABI boundary
def test_entry_point_is_declared_exported_and_bound():
    """ofdm_rx_soft is declared in an extension header of ABI 6 (as ofdm_rx_sweep_frames is): ofdm_hip.h and
    SIGNATURES, its mirror, keep the entry points they had, which existing tests enumerate."""
    from test_abi import HEADER, declared_functions

    ext = os.path.join(os.path.dirname(HEADER), "ofdm_hip_soft.h")
    text = open(ext).read()
    assert '#include "ofdm_hip.h"' in text and "ofdm_hip_soft.h" in open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(ofdm_[a-z_0-9]+)\s*\(", code))) == ["ofdm_rx_soft"]
    decl = text[text.index("int ofdm_rx_soft("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    main = open(HEADER).read()
    rx = main[main.index("int ofdm_rx("):]
    rx = re.sub(r"\s+", " ", rx[:rx.index(")")])
    # ofdm_rx's 17 arguments, then the six
    assert decl.startswith(rx.replace("int ofdm_rx(", "int ofdm_rx_soft(") + ", const double* g,")
    assert "const double* g, double inv_w, int32_t bins, int32_t k_lo, int32_t k_hi, uint64_t* hist" in decl
    at = text.index("int ofdm_rx_soft(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "never zeroed" in comment and "FMA" in comment and "bin = B/2 + floor(t)" in comment
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", main).group(1)) == B.ABI_VERSION == 6
    assert int(re.search(r"#define OFDM_MAX_SOFT_BINS (\d+)", text).group(1)) == B.MAX_SOFT_BINS == 256
    assert int(re.search(r"#define OFDM_SOFT_ROWS (\d+)", text).group(1)) == B.SOFT_ROWS == SE.ROWS == 20
    lib = B.load_library()
    assert hasattr(lib, "ofdm_rx_soft") and "ofdm_rx_soft" in B.SOFT_SIGNATURES
    # ofdm_rx's arguments, then g, inv_w, bins, k_lo, k_hi and the record
    assert B.SOFT_SIGNATURES["ofdm_rx_soft"][1] == B.SIGNATURES["ofdm_rx"][1] + [
        ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    assert lib.ofdm_rx_soft.argtypes == B.SOFT_SIGNATURES["ofdm_rx_soft"][1]
    assert len(B.SIGNATURES["ofdm_rx"][1]) == RX_ARGS
    assert set(B.SIGNATURES) == set(declared_functions())


def rx_args(sym0=0, n_sym=0, counters=True):
    cnt = (ctypes.c_uint64 * 2)()
    args = [None, None, None, None, None, 0, None, 0, 0.0, 0, None, sym0, n_sym, 0,
            ctypes.cast(cnt, ctypes.c_void_p) if counters else None, None, 0]
    assert len(args) == RX_ARGS
    return args, cnt


@pytest.mark.parametrize("inv_w,bins,k_lo,k_hi,record,scale,reason", [
    (8.0, 32, 0, 64, False, True, "needs a soft-decision record"),
    (8.0, 32, 0, 64, True, False, "needs the subcarriers' scale table g"),
    (8.0, 0, 0, 64, True, True, "bins 0 is not an even number in [2, 256]"),
    (8.0, -4, 0, 64, True, True, "bins -4 is not an even number in [2, 256]"),
    (8.0, 7, 0, 64, True, True, "bins 7 is not an even number in [2, 256]"),
    (8.0, 258, 0, 64, True, True, "bins 258 is not an even number in [2, 256]"),
    (NAN, 32, 0, 64, True, True, "inv_w is not a finite positive"),
    (INF, 32, 0, 64, True, True, "inv_w is not a finite positive"),
    (0.0, 32, 0, 64, True, True, "inv_w is not a finite positive"),
    (-8.0, 32, 0, 64, True, True, "inv_w is not a finite positive"),
    (8.0, 32, -1, 64, True, True, "range [-1, 64) is not 0 <= k_lo < k_hi <= n_fft"),
    (8.0, 32, 5, 5, True, True, "range [5, 5) is not 0 <= k_lo < k_hi <= n_fft"),
    (8.0, 32, 6, 5, True, True, "range [6, 5) is not 0 <= k_lo < k_hi <= n_fft"),
    (8.0, 32, 0, 64, True, True, "needs a constellation"),      # the arguments are fine: ofdm_rx's own refusal
    (8.0, 2, 0, 1, True, True, "needs a constellation"),
    (8.0, 256, 63, 64, True, True, "needs a constellation"),
])
def test_refusals_name_the_function_without_a_device(inv_w, bins, k_lo, k_hi, record, scale, reason):
    lib = B.load_library()
    args, _ = rx_args(0, 8)
    rec = (ctypes.c_uint64 * (40 * max(bins, 1) + 1))()
    g = (ctypes.c_double * 64)()
    rc = lib.ofdm_rx_soft(*args, ctypes.cast(g, ctypes.c_void_p) if scale else None, inv_w, bins, k_lo, k_hi,
                          ctypes.cast(rec, ctypes.c_void_p) if record else None)
    msg = lib.ofdm_last_error().decode()
    assert rc == -1 and "ofdm_rx_soft" in msg and reason in msg, msg
    assert not any(rec)


def test_what_ofdm_rx_refuses_is_refused():
    lib = B.load_library()
    rec = (ctypes.c_uint64 * 81)()
    g = (ctypes.c_double * 4)()
    for kw in (dict(sym0=-1, n_sym=4), dict(n_sym=-1), dict(counters=False), dict(n_sym=0)):
        args, _ = rx_args(**kw)
        assert lib.ofdm_rx_soft(*args, ctypes.cast(g, ctypes.c_void_p), 1.0, 2, 0, 1, ctypes.cast(rec, ctypes.c_void_p)) == -1
        assert "ofdm_rx_soft" in lib.ofdm_last_error().decode()
        assert lib.ofdm_rx(*args) == -1


def test_kernel_sources_hold_the_section_and_its_exclusions():
    """k_rx_soft is the shared body with OFDM_RX_BODY_SOFT, in translation units of its own, the form is in
    the table, and the soft arguments are no field of RxArgs."""
    from conftest import ROOT

    src = os.path.join(ROOT, "ofdm-based-systems_amd", "csrc")
    body = open(os.path.join(src, "ofdm_rx_body.hpp")).read()
    assert body.count("#ifdef OFDM_RX_BODY_SOFT") >= 5 and "static_assert(!FORM::SOFT" in body
    # the density's pinned line stands as it was
    assert "static_assert(DENS && !REF && !PROF && !SWEEP && !FRAMES" in body
    fused = open(os.path.join(src, "ofdm_fused.hpp")).read()
    at = fused.index("void k_rx_soft(")
    assert "#define OFDM_RX_BODY_SOFT" in fused[at:at + 400] and "RxArgs a, RxSoftTail st" in fused[at:at + 100]
    assert "SOFT = F == RxForm::Soft" in fused and "ONE_WAVE = PROF || SWEEP || DENS || SOFT" in fused
    assert "#pragma clang fp contract(off)" in fused[fused.index("void soft_bin("):at]
    launch = open(os.path.join(src, "ofdm_launch.hpp")).read()
    rxargs = launch[launch.index("struct RxArgs {"):]
    assert "hist" not in rxargs[:rxargs.index("};")] and "struct RxSoftTail {" in launch
    tail = launch[launch.index("struct RxSoftTail {"):]
    for name in ("hist", "g", "inv_w", "bins", "k_lo", "k_hi", "flush"):
        assert re.search(r"\b%s\b" % name, tail[:tail.index("};")]), name
    mk = open(os.path.join(ROOT, "ofdm-based-systems_amd", "Makefile")).read()
    for unit in ("ofdm_kernels_f32_soft", "ofdm_kernels_f64_soft"):
        assert unit + ".o" in mk and os.path.exists(os.path.join(src, unit + ".hip"))


# ---------------------------------------------------------------- the restatement on hand-made points
def one(z, idx, M, B_, L, **kw):
    """The record of a single point (N = 1)."""
    return SE.record(np.array([[z]]), np.array([[idx]]), M, SE.scale(M, 1), B_, L, **kw)


def test_zero_is_a_bin_line_and_the_ends_saturate():
    B_, L = 8, 2.0
    lut = O.qam_lut(4)
    # a point on the Q decision boundary: D of bit 0 is +0.0 or -0.0, both in bin B/2
    for im in (0.0, -0.0):
        counts, inv = one(complex(lut[0].real, im), 0, 4, B_, L)
        assert inv == 0 and counts.sum() == 2 and counts[0, :, B_ // 2].sum() == 1
    # noise free: |u| = 1 exactly in units of the squared minimum distance, on the right side
    for i, c in enumerate(lut):
        counts, inv = one(c, i, 4, B_, L)
        assert inv == 0 and SE.hard_bit_errors(counts) == 0 and counts.sum() == 2
        for r in (0, 1):
            v = (i >> (1 - r)) & 1
            t = 1.0 * SE.inv_width(B_, L)
            want = B_ // 2 + (int(t) if v == 0 else -int(t))   # u = +1 (tx bit 0) or -1 (tx bit 1): 2 bins from zero
            assert counts[r, v, want] == 1, (i, r)
    # far out: the end bins; an infinity saturates too, and only a NaN is invalid
    for z in (complex(100.0, 100.0), complex(-100.0, -100.0)):
        counts, inv = one(z, 0, 4, B_, L)
        assert inv == 0 and counts[:, :, [0, B_ - 1]].sum() == 2 and counts.sum() == 2
        # u = +-inf (the scale overflows the product): compared in double, still the end bins
        counts, inv = SE.record(np.array([[z]]), np.array([[0]]), 4, np.array([1e308]), B_, L)
        assert inv == 0 and counts[:, :, [0, B_ - 1]].sum() == 2 and counts.sum() == 2
    counts, inv = one(complex(NAN, 0.3), 0, 4, B_, L)
    assert inv == 1 and counts.sum() == 1            # the I bit is NaN, the Q bit is counted
    counts, inv = one(complex(INF, 0.3), 0, 4, B_, L)
    assert inv == 1 and counts.sum() == 1            # inf - inf


def test_row_offsets_of_the_four_orders():
    for M, rows in ((4, (0, 2)), (16, (2, 6)), (64, (6, 12)), (256, (12, 20))):
        lut = O.qam_lut(M)
        b = M.bit_length() - 1
        assert SE.row0(b) == rows[0] == E.SoftDecisions.row0(b)
        for i in (0, M // 3, M - 1):
            counts, inv = one(lut[i], i, M, 128, 8.0)
            filled = np.flatnonzero(counts.sum(axis=(1, 2)))
            assert filled.tolist() == list(range(*rows)) and inv == 0 and counts.sum() == b
            # the second index is the transmitted bit, MSB first
            for r in range(b):
                assert counts[rows[0] + r, (i >> (b - 1 - r)) & 1].sum() == 1
            assert SE.hard_bit_errors(counts) == 0


def test_range_mask_and_widening():
    rng = np.random.default_rng(5)
    S, N, M = 3, 8, 16
    idx = rng.integers(0, M, (S, N))
    Z = O.qam_lut(M)[idx] + 0.2 * (rng.standard_normal((S, N)) + 1j * rng.standard_normal((S, N)))
    g = SE.scale(M, N)
    whole, _ = SE.record(Z, idx, M, g, 16, 4.0)
    assert whole.sum() == S * N * 4
    lo, _ = SE.record(Z, idx, M, g, 16, 4.0, 0, 3)
    hi, _ = SE.record(Z, idx, M, g, 16, 4.0, 3, N)
    assert lo.sum() == S * 3 * 4 and np.array_equal(lo + hi, whole)
    col, _ = SE.record(Z, idx, M, g, 16, 4.0, 5, 6)
    assert np.array_equal(col, SE.record(Z[:, 5:6], idx[:, 5:6], M, g[5:6], 16, 4.0)[0])
    # n_valid: the first bits of the stream, MSB first inside a subcarrier
    for nv in (0, 1, 4 * N + 2, S * N * 4 - 3, S * N * 4):
        c, _ = SE.record(Z, idx, M, g, 16, 4.0, n_valid=nv)
        assert c.sum() == nv
    c, _ = SE.record(Z, idx, M, g, 16, 4.0, n_valid=2)
    assert c[2].sum() == 1 and c[3].sum() == 1 and c[4:].sum() == 0
    # an adaptive plan: order-0 subcarriers carry nothing, every order fills its own rows
    orders = np.array([4, 0, 16, 64, 0, 256, 4, 16])
    ix = np.stack([rng.integers(0, max(int(o), 1), S) for o in orders], axis=1)
    c, _ = SE.record(Z, ix, orders, SE.scale(orders, N), 16, 4.0)
    assert c.sum() == S * (2 + 4 + 6 + 8 + 2 + 4)
    assert [int(c[SE.row0(b):SE.row0(b) + b].sum()) for b in (2, 4, 6, 8)] == [S * 4, S * 8, S * 6, S * 8]
    # complex64 is widened, exactly
    z32 = Z.astype(np.complex64)
    assert np.array_equal(SE.record(z32, idx, M, g, 16, 4.0)[0], SE.record(z32.astype(np.complex128), idx, M, g, 16, 4.0)[0])


def test_bracket_holds_a_perturbed_record():
    rng = np.random.default_rng(6)
    S, N, M, B_, L = 5, 16, 64, 128, 8.0
    idx = rng.integers(0, M, (S, N))
    Z = O.qam_lut(M)[idx] + 0.05 * (rng.standard_normal((S, N)) + 1j * rng.standard_normal((S, N)))
    g = SE.scale(M, N)
    delta = np.full((S, N), 1e-4)
    dec, maybe = SE.bracket(Z, delta, idx, M, g, B_, L)
    assert dec.sum() + SE._near_line(*(SE.differences(Z, idx, M, g, B_, L, delta=delta)[2:]), B_).sum() == S * N * 6
    for _ in range(4):
        ph = rng.uniform(0, 2 * np.pi, (S, N))
        got = SE.flat(*SE.record(Z + 1e-4 * np.exp(1j * ph), idx, M, g, B_, L))
        assert np.all(got >= dec) and np.all(got - dec <= maybe)
    assert maybe.sum() > 0


# ---------------------------------------------------------------- the sign of D against hard decisions
def tx_idx(tx_bytes, S, N, b):
    return O.bits_to_indices(O.bytes_to_bits(tx_bytes)[:S * N * b], b).reshape(S, N)


def check_sign(Z, delta, idx, orders, N, n_valid, want_errors, what):
    g = SE.scale(orders, N)
    row, tx, t, bd = SE.differences(Z, idx, orders, g, 128, 8.0, n_valid=n_valid, delta=delta)
    assert not np.any(t == 0.0), what                     # no value is exactly undecided
    counts, inv = SE.record(Z, idx, orders, g, 128, 8.0, n_valid=n_valid)
    assert inv == 0 and counts.sum() == n_valid
    share = float(np.mean(SE._near_line(t, bd, 128)))
    print(f"{what}: wrong-sign mass {SE.hard_bit_errors(counts)} (pinned {want_errors}), share near a line {share:.3e}")
    assert SE.hard_bit_errors(counts) == want_errors, what
    assert share <= 1e-3, what


@pytest.mark.parametrize("st", load_stages(), ids=lambda s: s["name"])
def test_stage_fixtures_sign_is_the_hard_decision(st):
    a = stage_arrays(st["name"])
    S, N, M = st["S"], st["N"], st["M"]
    b = M.bit_length() - 1
    Z = a["Z"].reshape(S, N)
    idx = tx_idx(a["tx_bytes"], S, N, b)
    assert np.array_equal(O.qam_lut(M)[idx], a["X"].reshape(S, N))
    # the project's tolerance on Z
    check_sign(Z, 1e-9 * (1.0 + np.abs(Z)), idx, M, N, S * N * b, st["bit_errors"], st["name"])


@pytest.mark.parametrize("case", PE.THROUGHPUT_CASES, ids=lambda c: c["id"])
def test_throughput_cases_sign_is_the_hard_decision(case):
    N, S = case["N"], case["S"]
    h, cp, orders = PE.case_channel(case)
    Z, delta, idx = DE.philox_points(PE.SEED, S, N, case["M"], h, cp, case["eq"], case["snr"], orders=orders,
                                     radius_fn=PE.np_radius)
    o = SE.per_subcarrier(case["M"] if orders is None else orders, N)
    bps = sum(int(m).bit_length() - 1 for m in o if m > 0)
    n_valid = (S * bps // 8) * 8 if orders is not None else S * bps
    check_sign(Z, delta, idx, o, N, n_valid, case["bit_errors"], case["id"])


# ---------------------------------------------------------------- SoftDecisions and the GMI
def decisions(counts, invalid, L, N=1):
    return E.SoftDecisions(counts=counts, invalid=invalid, bins=counts.shape[-1], extent=L, subcarriers=(0, N),
                           n_bits=int(counts.sum()) + invalid)


def test_soft_decisions_arithmetic():
    counts = np.zeros((20, 2, 4), np.int64)
    counts[2, 0, 3] = 5
    counts[2, 0, 1] = 2      # wrong side
    counts[3, 1, 0] = 4
    counts[3, 1, 2] = 1      # wrong side
    d = decisions(counts, 3, 2.0)
    assert d.hard_bit_errors == 3 == SE.hard_bit_errors(counts) and d.n_bits == 15
    assert d.llr_centres.tolist() == [-1.5, -0.5, 0.5, 1.5]
    assert d.rows(4).shape == (4, 2, 4) and np.array_equal(d.rows(4), counts[2:6]) and d.orders == (4,)
    assert d.rows(2).shape == (2, 2, 4) and d.rows(8).shape == (8, 2, 4) and d.rows(6).shape == (6, 2, 4)
    with pytest.raises(ValueError):
        d.rows(3)
    # a given scale: the formula, row by row
    c = d.llr_centres
    want0 = 1 - (5 * np.log2(1 + np.exp(-0.7 * c[3])) + 2 * np.log2(1 + np.exp(-0.7 * c[1]))) / 7
    want1 = 1 - (4 * np.log2(1 + np.exp(0.7 * c[0])) + 1 * np.log2(1 + np.exp(0.7 * c[2]))) / 5
    per = d.gmi_per_bit(4, scale=0.7)
    assert per.tolist() == pytest.approx([want0, want1, 0.0, 0.0], abs=1e-12)
    assert d.gmi(4, scale=0.7) == pytest.approx(want0 + want1, abs=1e-12)
    # the scale search finds the reference's maximum
    assert d.gmi(4) == pytest.approx(SE.gmi(counts, 4, 2.0), abs=1e-6) and d.gmi(4) >= d.gmi(4, scale=0.7)
    assert d.gmi(2) == 0.0 and d.gmi() == pytest.approx(d.gmi(4), abs=1e-12)


def test_noise_free_points_carry_every_bit():
    for M in (4, 16, 64, 256):
        b = M.bit_length() - 1
        idx = np.arange(M)[None, :].repeat(3, 0)
        counts, inv = SE.record(O.qam_lut(M)[idx], idx, M, SE.scale(M, M), 128, 8.0)
        d = decisions(counts, inv, 8.0, M)
        assert d.hard_bit_errors == 0 and d.gmi(b) > b - 1e-9 and d.gmi() > b - 1e-9
        # |u| is an integer >= 1 to within rounding (t = 8 u): nothing closer to zero than seven bins
        assert counts[:, :, 64 - 7:64 + 7].sum() == 0
    # mixed orders: the total rate per OFDM symbol over the active subcarriers
    orders = np.array([4] * 6 + [0] * 3 + [64] * 2)
    rng = np.random.default_rng(2)
    ix = np.stack([rng.integers(0, max(int(o), 1), 50) for o in orders], axis=1)
    Z = np.zeros(ix.shape, np.complex128)
    for m in (4, 64):
        Z[:, orders == m] = O.qam_lut(m)[ix[:, orders == m]]
    counts, inv = SE.record(Z, ix, orders, SE.scale(orders, len(orders)), 128, 8.0)
    d = decisions(counts, inv, 8.0, len(orders))
    assert d.orders == (2, 6) and d.gmi() == pytest.approx((6 * 2 + 2 * 6) / 8, abs=1e-9)


def bpsk_capacity(snr_lin):
    """C_BPSK in bits at amplitude^2 / noise variance = snr_lin, by quadrature: y = 1 + n, n ~ N(0, 1 / snr)."""
    s2 = 1.0 / snr_lin
    sd = np.sqrt(s2)
    y = np.linspace(1.0 - 12 * sd, 1.0 + 12 * sd, 200001)
    pdf = np.exp(-(y - 1.0) ** 2 / (2 * s2)) / np.sqrt(2 * np.pi * s2)
    f = pdf * np.logaddexp(0.0, -2.0 * y / s2) / np.log(2.0)
    return 1.0 - float(np.sum((f[1:] + f[:-1]) * 0.5 * np.diff(y)))


@pytest.mark.parametrize("snr_db", [0.0, 6.0])
def test_gmi_of_4qam_is_twice_the_bpsk_capacity(snr_db):
    """Max-log is exact for 4-QAM: over a flat channel without equaliser the two bits are two BPSK channels
    at the link's SNR.  The bound: 0.01 bit, 2.5 times the larger of the two differences measured with the
    restatement (0.0038 at 0 dB, 0.0009 at 6 dB: sampling error of 65 536 uses plus the binning)."""
    N, S, M, B_, L = 1024, 64, 4, 128, 8.0
    Z, _, idx = DE.philox_points(PE.SEED, S, N, M, np.array([1.0 + 0j]), 0, "NONE", snr_db, radius_fn=PE.np_radius)
    counts, inv = SE.record(Z, idx, M, SE.scale(M, N), B_, L)
    d = decisions(counts, inv, L, N)
    want = 2.0 * bpsk_capacity(10 ** (snr_db / 10))
    print(f"4-QAM at {snr_db} dB: gmi {d.gmi():.5f}, 2 C_BPSK {want:.5f}, scale {d.gmi_scale(2):.4f}")
    assert inv == 0 and d.n_bits == 2 * S * N
    assert abs(d.gmi() - want) <= 0.01
    assert abs(SE.gmi(counts, 2, L) - want) <= 0.01 and d.gmi() == pytest.approx(SE.gmi(counts, 2, L), abs=1e-5)


# ---------------------------------------------------------------- the engine's host-made quantities
def test_soft_grid_and_scale():
    assert E.soft_grid(128, 8.0) == 8.0 == SE.inv_width(128, 8.0) and E.soft_grid(6, 0.5) == 6.0
    assert E.soft_grid(256) == 16.0
    for bad in (0, 1, 7, 258, 2.5, True, -2):
        with pytest.raises(ValueError, match="soft"):
            E.soft_grid(bad, 8.0)
    for bad in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="soft_extent"):
            E.soft_grid(8, bad)
    N = 16
    h = np.array([1.0, 0.5 - 0.2j, 0.1j])
    for M in (4, 16, 64, 256):
        assert np.array_equal(E.soft_scale([O.qam_lut(M)], None, None, h, N), SE.scale(M, N))
    orders = np.array([4, 0, 16, 64, 0, 256, 4, 16] * 2)
    luts = [O.qam_lut(m) for m in (4, 16, 64, 256)]
    sc = np.array([{0: -1, 4: 0, 16: 1, 64: 2, 256: 3}[int(o)] for o in orders], np.int32)
    assert np.array_equal(E.soft_scale(luts, sc, None, h, N), SE.scale(orders, N))
    w = SE.csi_weights(h, N)
    assert w.max() == 1.0 and np.array_equal(E.soft_scale(luts, sc, "csi", h, N), SE.scale(orders, N, w))
    arr = np.linspace(0.0, 2.0, N)
    assert np.array_equal(E.soft_scale(luts, sc, arr, h, N), SE.scale(orders, N, arr))
    # the unit: a noise-free neighbour is exactly one squared minimum distance away
    lut = O.qam_lut(16)
    step = np.diff(np.unique(lut.real))[0]
    assert SE.scale(16, 1)[0] * step * step == pytest.approx(1.0, rel=1e-15)
    for bad in ("snr", np.ones(N - 1), -np.ones(N), np.full(N, NAN)):
        with pytest.raises(ValueError, match="soft_weights"):
            E.soft_scale(luts, sc, bad, h, N)
    with pytest.raises(ValueError, match="not built"):
        E.soft_scale([O.psk_lut(8)], None, None, h, N)
    with pytest.raises(ValueError, match="not built"):
        E.soft_scale([O.psk_lut(4)], None, None, h, N)
    with pytest.raises(ValueError, match="not built"):
        E.soft_scale([O.qam_lut(1024)], None, None, h, N)


def test_settings_keys():
    base = dict(num_bands=64, signal_noise_ratios=[10.0], channel_model_path="", num_symbols=8)
    s0 = SimulationSettings(**base)
    assert s0.soft_bins is None and s0.soft_extent is None and s0.soft_weights is None
    s = SimulationSettings(**base, soft_bins=64, soft_extent=4.0, soft_weights="csi")
    assert (s.soft_bins, s.soft_extent, s.soft_weights) == (64, 4.0, "csi")
    for bad in (dict(soft_bins=0), dict(soft_bins=7), dict(soft_bins=258), dict(soft_extent=0.0)):
        with pytest.raises(ValueError):
            SimulationSettings(**base, **bad)
    sims = Simulation.create_from_simulation_settings(s)
    assert [(x.soft_bins, x.soft_extent, x.soft_weights) for x in sims] == [(64, 4.0, "csi")]
    assert Simulation.create_from_simulation_settings(s0)[0].soft_bins is None


def test_simulation_refusals_come_before_the_run():
    from ofdm_based_systems.modulation.models import OFDMModulator

    class MyModulator(OFDMModulator):
        pass

    class Composed(Simulation):
        MODULATOR_SCHEME_MAPPERS = {k: MyModulator for k in Simulation.MODULATOR_SCHEME_MAPPERS}

    kw = dict(num_symbols=64 * 4, verbose=False, make_plot=False)
    with pytest.raises(ValueError, match="built-in"):
        Composed(soft_bins=8, **kw).run()
    with pytest.raises(ValueError, match="subcarrier_profile"):
        Simulation(soft_bins=8, subcarrier_profile=True, **kw).run()
    with pytest.raises(ValueError, match="frame_symbols"):
        Simulation(soft_bins=8, frame_symbols=2, **kw).run()
    with pytest.raises(ValueError, match="constellation_density"):
        Simulation(soft_bins=8, constellation_density=8, **kw).run()
    for bad in (0, -2, 2.5, 7, 258):
        with pytest.raises(ValueError, match="soft"):
            Simulation(soft_bins=bad, **kw).run()
    with pytest.raises(ValueError, match="soft_extent"):
        Simulation(soft_bins=8, soft_extent=-1.0, **kw).run()
    with pytest.raises(ValueError, match="without soft_bins"):
        Simulation(soft_extent=4.0, **kw).run()
    sims = [Simulation(num_symbols=64 * 4, snr_db=q, rng_mode="philox", seed=1, received_symbols_keep=0,
                       verbose=False, make_plot=False, soft_bins=8) for q in (10.0, 12.0)]
    with pytest.raises(ValueError, match="soft_bins"):
        Simulation.run_sweep(sims)

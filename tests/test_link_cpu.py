"""The fused link (ofdm_link) without a GPU: the entry point's declaration, export and binding, its
routing predicate restated for the dispatch model, the engine's route over the CPU test doubles, the
kernel's LDS budget, and that the GPU test's 10 dB point counts errors."""

import ctypes
import re

import numpy as np
import pytest

import dispatch_model as D
import philox_streams as P
from ofdm_based_systems import _backend as B
from test_abi import HEADER, declared_functions
from test_engine_schedule_cpu import CASE, S, SEEDS, Logged, make, rx, tx
from test_sweep_cpu import SweepEngine


def test_entry_point_is_declared_exported_and_bound():
    assert "ofdm_link" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_link("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert decl == ("int ofdm_link(ofdm_plan_t plan, void* stream, uint64_t seed, const ofdm_stats* stats, "
                    "int64_t total_samples, double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, "
                    "int64_t n_valid_bits, uint64_t* counters)")
    at = text.index("int ofdm_link(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "OFDM_E_INVALID" in comment and "no fall-back" in comment
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    vp, i32, i64, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    assert B.SIGNATURES["ofdm_link"] == (ctypes.c_int, [vp, vp, u64, vp, i64, f64, i32, i64, i64, i64, vp])
    assert set(B.SIGNATURES) == set(declared_functions())
    lib = B.load_library()
    assert hasattr(lib, "ofdm_link") and lib.ofdm_abi_version() == B.ABI_VERSION


def test_null_plan_is_invalid_without_a_gpu():
    lib = B.load_library()
    assert lib.ofdm_link(None, None, 0, None, 0, 20.0, 1, 0, 4, 0, None) == -1
    assert b"ofdm_link" in lib.ofdm_last_error()


def fused_form(p: D.Plan) -> bool:
    """link_shape (csrc/ofdm_link_inst.hpp) and ofdm_link's checks restated on the dispatch model's
    plan: a complex128 fixed-QAM bench shape (ref_fb > 1) at a symbol per wave with its per-pass
    twiddles in LDS -- N = 1024, 64-QAM -- cyclic-prefix OFDM, a flat channel, no equaliser."""
    zpad = p.prefix == "ZP" and p.cp > 0
    return (p.prec == D.F64 and p.N == 1024 and p.bits == 6 and p.scheme == "QAM" and p.modulator == "OFDM"
            and not zpad and p.L == 1 and p.eq == "NONE")


def test_the_routing_predicate_on_the_dispatch_model():
    b = D.Plan(D.F64, 1024, 6)
    assert fused_form(b)
    # the fused kernel replaces exactly this pair
    assert D.dispatch(b) == (("k_tx", "double", 10, 6, 0, False), ("k_rx", "double", 10, 0, 6, False))
    assert fused_form(D.Plan(D.F64, 1024, 6, cp=16)) and fused_form(D.Plan(D.F64, 1024, 6, prefix="ZP", cp=0))
    for other in (D.Plan(D.F32, 1024, 6), D.Plan(D.F64, 1024, 6, L=8, cp=7, eq="MMSE"), D.Plan(D.F64, 1024, 6, L=2, cp=1),
                  D.Plan(D.F64, 1024, 6, eq="ZF"), D.Plan(D.F64, 1024, 4), D.Plan(D.F64, 1024, 8),
                  D.Plan(D.F64, 512, 6), D.Plan(D.F64, 2048, 6), D.Plan(D.F64, 4096, 8, L=8, cp=7, eq="MMSE"),
                  D.Plan(D.F64, 1024, 6, modulator="SC"), D.Plan(D.F64, 1024, 6, prefix="ZP", cp=16),
                  D.Plan(D.F64, 1024, 5, scheme="PSK"), D.Plan(D.F64, 1024, 0, orders=(64,) * 1024)):
        assert not fused_form(other), other
    # every plan with a fused form dispatches to the flat 64-QAM pair at N = 1024; no other does
    for p in (c.plan for c in D.matrix_cases() + D.geometry_cases() + D.generic_cases()):
        if fused_form(p):
            assert D.dispatch(p) == D.dispatch(b), p


class Linked(Logged):
    """The logging CPU double with a fused form: ``link`` computed as the double's tx into a buffer
    followed by its rx of that buffer (the entry point's contract), and logged."""

    _fused = True

    def link(self, stream, seed, stats, total_samples, snr_db, noise_on, sym0, n_sym, n_valid, counters):
        self.log.append(("link", sym0, n_sym, True, 1))
        self.seeds.append(seed)
        y = self._y(n_sym)
        SweepEngine.tx(self, stream, None, seed, sym0, n_sym, y, stats.clone())
        SweepEngine.rx(self, stream, y, None, None, seed, stats, total_samples, snr_db, noise_on, None, sym0, n_sym,
                       n_valid, counters)


def linked():
    from conftest import channel

    h = channel(CASE["ch"])
    eng = Linked(CASE["N"], CASE["M"], h, len(h) - 1, CASE["eq"])
    for sd in SEEDS:
        eng.seed_streams(sd, S)
    return eng


def ln(sym0, n):
    return ("link", sym0, n, True, 1)


def record(s):
    return (s.bit_errors, s.symbol_errors, s.power_sum, s.x_power_sum, s.x_peak, s.papr_db)


def test_the_fused_route_is_a_power_pass_and_one_link_whatever_the_budget():
    eng = linked()
    want = record(eng.run(S, CASE["snr"], seed=SEEDS[0], fused=False))
    assert eng.log == [tx(0, 10), rx(0, 10)]
    for kw in ({}, {"fused": True}, {"batch": 4}, {"y_budget": 3 * CASE["N"] * 16}):
        eng.log.clear()
        assert record(eng.run(S, CASE["snr"], seed=SEEDS[0], **kw)) == want
        assert eng.log == [tx(0, 10, True), ln(0, 10)], kw


def test_a_tap_a_profile_caller_streams_or_partial_bits_keep_the_two_kernels():
    eng = linked()
    for kw in ({"keep_symbols": 2}, {"profile": True}, {"n_valid_bits": S * eng.bps - 8}):
        eng.log.clear()
        eng.run(S, CASE["snr"], seed=SEEDS[0], noise_on=False, **kw)
        assert eng.log == [tx(0, 10), rx(0, 10)], kw
        with pytest.raises(ValueError):
            eng.run(S, CASE["snr"], seed=SEEDS[0], fused=True, **kw)
    plain = make()  # no fused form
    assert not plain.has_fused
    with pytest.raises(ValueError):
        plain.run(S, CASE["snr"], seed=SEEDS[0], fused=True)
    with pytest.raises(ValueError):
        plain.run_pipelined(S, CASE["snr"], SEEDS, fused=True)
    assert plain.log == []


def test_pipelined_fused_runs_one_power_pass_ahead():
    eng = linked()
    out = [p.result() for p in eng.run_pipelined(S, CASE["snr"], SEEDS, y_budget=0)]
    assert eng.log == [tx(0, 10, True), tx(0, 10, True), ln(0, 10), tx(0, 10, True), ln(0, 10), ln(0, 10)]
    assert eng.seeds == [11, 12, 11, 13, 12, 13]
    eng.log.clear()
    forced = [p.result() for p in eng.run_pipelined(S, CASE["snr"], SEEDS, fused=False)]
    assert eng.log == [tx(0, 10), tx(0, 10), rx(0, 10), tx(0, 10), rx(0, 10), rx(0, 10)]
    assert [record(o) for o in out] == [record(f) for f in forced]


def test_the_link_workgroup_holds_12_symbols_not_16():
    """k_link's LDS (link_carve, csrc/ofdm_link_inst.hpp) restated: both per-pass twiddle tables as the
    plan uploads them (the kernel does not rely on the inverse being the forward's conjugate), the axis
    entries, the block-sum scratch and the rows of reals, beside the static LUT and noise tables."""
    tt = 15 * 16 + 3 * 256                 # tt_size(10): passes of radix 16, 16, 4
    rows = lambda spb: spb * (1024 + 64) * 8  # PADN reals per symbol
    dynamic = lambda spb: 8 * 64 + rows(spb) + 8 * (64 * spb // 64) + 2 * tt * 16
    static = 64 * 16 + 64 * 8 + 64 * 16    # LUT, noise phase table, its widening to double
    assert static == 2560                  # (profiles/link_kernel_audit.txt: group_segment_fixed_size)
    assert dynamic(12) + static == 139872 <= 160 * 1024 < dynamic(16) + static


def test_the_gpu_tests_10_db_point_counts_errors():
    """163 symbols at 10 dB: the oracle alone counts thousands of bit errors, so the GPU test's exact
    equality of the fused and the two-kernel counts is not vacuous."""
    r = P.run_philox(77, 163, 1024, 64, np.array([1.0 + 0j]), 0, "NONE", 10.0)
    assert r.bit_errors > 100 and r.symbol_errors > 100

"""CPU checks of the dispatch model and of the case tables of tests/test_gpu_dispatch_matrix.py.

* coverage: the matrix maps, under the model, onto exactly the reachable k_tx / k_rx instantiations,
  no case of the matrix or the geometry table falls to the generic kernel, and every rotated run-time
  dimension occurs with every log2 N and every FB;
* oracle only: every case, run through philox_streams.run_philox with a float32 NumPy stand-in for
  the hardware noise radius, counts more than 100 bit errors, every complex128 case has a decision
  bracket of width 0, and every complex64 case's rigorous bracket is inside the width the GPU test
  accepts -- conditions on the inputs (SNRs, seeds, channels), so a GPU count outside the bracket
  is the kernel's doing;
* trace: the kernel names a profiler recorded under the GPU file (profiles/dispatch_matrix_kernels.txt)
  are the model's prediction for the case tables -- a change of the launch rules that reroutes a
  shape fails here.
"""

import os
import re

import numpy as np
import pytest

import dispatch_model as D
import philox_streams as P
import test_gpu_philox_parity as PP  # (its tolerances; importing it needs no GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = D.matrix_cases()
GEOMETRY = D.geometry_cases()
GENERIC = D.generic_cases()
FALLBACK = D.fallback_cases()
ORACLE_CASES = MATRIX + GEOMETRY + GENERIC + FALLBACK


def test_reachable_counts():
    # (the launch rules name 396 transmitters; three never fit a CU's LDS: dispatch_model.lds_fallback_tx)
    tx, rx = D.reachable()
    assert (len(tx), len(rx)) == (393, 420)


def test_matrix_covers_every_reachable_instantiation():
    tx, rx = D.predicted_names(MATRIX)
    rtx, rrx = D.reachable()
    assert tx == rtx, (sorted(rtx - tx), sorted(tx - rtx))
    assert rx == rrx, (sorted(rrx - rx), sorted(rx - rrx))
    # the least table that can: per (precision, log2 N, FB) the larger of its transmitters and receivers
    assert len(MATRIX) == 457 and len({c.id for c in MATRIX}) == len(MATRIX)


def test_no_matrix_or_geometry_case_takes_the_generic_kernel():
    for c in MATRIX:
        t, r = D.dispatch(c.plan)
        assert t[3] > 0 and r[4] > 0, c.id
    tx, rx = D.predicted_names(GEOMETRY, (D.F32, D.F64))
    assert all(t[3] == 4 for t in tx) and all(r[4] == 4 for r in rx)
    # the geometry table crosses every FIR hand-over: window <-> run time, guard compiled in or not
    assert {(t[1], t[4], t[5]) for t in tx} == {("float", 4, False), ("float", 8, False), ("float", -1, False),
                                               ("double", 4, False), ("double", 8, False), ("double", -1, False),
                                               ("double", 4, True), ("double", 8, True)}


def test_generic_cases_take_the_generic_kernel():
    tx, rx = D.predicted_names(GENERIC)
    assert all(t[3] == 0 and t[4] == -1 for t in tx) and all(r[3] == -1 and r[4] == 0 for r in rx)
    assert {t[2] for t in tx} == {0, 1, 2, 3, 4, 5, 8}


def test_lds_fallback_cases_pair_the_generic_transmitter_with_the_adaptive_receiver():
    for c in FALLBACK:
        t, r = D.dispatch(c.plan)
        assert t[3:] == (0, -1, False) and r[4:] == (1, True), c.id


def _dims(c):
    """The rotated run-time dimensions a case exercises, as (dimension, value) pairs."""
    p = c.plan
    t, r = D.dispatch(p)
    lt, zpw, mv = t[4], t[5], r[5]
    out = []
    if t[3] != 1:  # (the adaptive kernels take neither SC-OFDM nor zero padding)
        out.append(("tx-sc", p.modulator == "SC"))
        if mv:
            out.append(("mv-runs", (p.modulator, p.prefix)))
    if lt in (4, 8):
        out.append((f"taps-LT{lt}{'Z' if zpw else ''}", p.L))
        out.append((f"cp-LT{lt}", "L-1" if p.cp == p.L - 1 else "TPS" if p.cp == D.tps(p.N) else p.cp))
    if lt == -1 and p.N >= 256:
        out.append(("taps-RT", p.L if p.L > 8 else "cp=TPS+1"))
    return out


def test_every_rotated_dimension_occurs_with_every_logn_and_every_fb():
    want = {("tx-sc", True), ("tx-sc", False),
            ("mv-runs", ("SC", "CP")), ("mv-runs", ("OFDM", "ZP")), ("mv-runs", ("SC", "ZP")),
            ("taps-RT", 9), ("taps-RT", 12), ("taps-RT", 32), ("taps-RT", "cp=TPS+1")}
    want |= {("taps-LT4", L) for L in (2, 3, 4)} | {("taps-LT4Z", L) for L in (1, 2, 3, 4)}
    want |= {(f"taps-LT8{z}", L) for L in (5, 6, 7, 8) for z in ("", "Z")}
    want |= {(f"cp-LT{lt}", v) for lt in (4, 8) for v in ("L-1", 8, 9, "TPS")}
    by_logn, by_fb = {}, {}
    for c in MATRIX:
        t, _ = D.dispatch(c.plan)
        for d in _dims(c):
            by_logn.setdefault(t[2], set()).add(d)
            by_fb.setdefault(t[3], set()).add(d)

    def applies(d, logn=None, fb=None):
        if fb == 1 and (d[0] in ("tx-sc", "mv-runs") or d[0].endswith("Z")):
            return False  # adaptive: OFDM with a cyclic prefix only
        if logn is not None and logn < 8 and (d[0].startswith("taps-") or d[0].startswith("cp-")):
            return False  # no window FIR below N = 256: every multipath channel is one class
        return True

    for logn in D.LOGNS:
        missing = {d for d in want if applies(d, logn=logn)} - by_logn[logn]
        assert not missing, (logn, sorted(missing, key=str))
    for fb in D.FBS:
        missing = {d for d in want if applies(d, fb=fb)} - by_fb[fb]
        assert not missing, (fb, sorted(missing, key=str))


def test_channels_keep_every_subcarrier_above_04():
    for L, N in sorted({(c.plan.L, c.plan.N) for c in ORACLE_CASES}):
        h = D.synthetic_channel(L, N)
        assert len(h) == L and abs(abs(h[0]) - 1) < 1e-15
        if L > 1:
            assert h[0] == 1 and abs(np.sum(np.abs(h[1:])) - 0.6) < 1e-12
        assert np.min(np.abs(np.fft.fft(h, max(N, L)))) >= 0.4 - 1e-12


def test_adaptive_cases_load_square_qam_up_to_256():
    n = 0
    for c in MATRIX:
        if c.plan.bits == 0:
            used = {o for o in c.plan.orders if o > 0}
            assert used and used <= {4, 16, 64, 256}, (c.id, used)
            n += len(used) > 1
    assert n > 0  # some cases mix orders


def np_radius(words: np.ndarray) -> np.ndarray:
    """float32 NumPy stand-in for the hardware radius sqrt(32 - log2(float32(w | 1)))."""
    f = (np.asarray(words, np.uint32) | np.uint32(1)).astype(np.float32)
    return np.sqrt(np.float32(32) - np.log2(f))


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.id for c in ORACLE_CASES])
def test_oracle_alone_counts_errors_with_an_exact_bracket(case):
    p = case.plan
    f64 = p.prec == D.F64
    ref = P.run_philox(77, case.S, p.N, case.M, case.h, p.cp, p.eq, case.snr,
                       precision="f64" if f64 else "f32", radius_fn=np_radius, **D.philox_kwargs(case))
    assert ref.bit_errors > 100, ref.bit_errors
    lo, hi, slo, shi = ref.bracket
    if f64:
        assert (lo, slo) == (hi, shi) == (ref.bit_errors, ref.symbol_errors), ref.bracket
    else:
        # complex64: the rigorous bracket's width is the oracle's too (it moves by a few counts with
        # the hardware radius): inside the bound the GPU test asserts, with a tenth to spare
        wmax = PP.bracket_width_bound(PP.B.OFDM_F32, case.variant(), ref.bit_errors)
        assert wmax is None or max(hi - lo, shi - slo) <= 0.9 * wmax, (ref.bracket, wmax)


# --------------------------------------------------------------------------- the recorded trace

NAMES = os.path.join(ROOT, "profiles", "dispatch_matrix_kernels.txt")


def test_recorded_kernel_names_are_the_models_prediction():
    got_tx, got_rx = set(), set()
    with open(NAMES) as f:
        for line in f:
            m = re.search(r"(k_tx|k_rx)<([^<>]*)>", line)
            if not m or line.startswith("#"):
                continue
            a = [s.strip() for s in m.group(2).split(",")]
            # k_tx: R, LOGN, FB, LT, ZPW, REF, WIDE; k_rx: R, LOGN, EQ, FB, MV, REF, WIDE
            val = [a[0]] + [{"true": True, "false": False}[s] if s in ("true", "false") else int(s) for s in a[1:]]
            assert len(val) == 7 and val[5:] == [False, False], line  # no REF, no WIDE in throughput mode
            (got_tx if m.group(1) == "k_tx" else got_rx).add((m.group(1),) + tuple(val[:5]))
    tx, rx = set(), set()
    for cases, precs in ((MATRIX, None), (GEOMETRY, (D.F32, D.F64)), (GENERIC, None), (FALLBACK, None)):
        t, r = D.predicted_names(cases, precs)
        tx |= t
        rx |= r
    assert got_tx == tx, (sorted(tx - got_tx, key=str), sorted(got_tx - tx, key=str))
    assert got_rx == rx, (sorted(rx - got_rx, key=str), sorted(got_rx - rx, key=str))

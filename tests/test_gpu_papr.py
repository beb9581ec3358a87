"""The per-symbol PAPR histogram on the GPU (ofdm_papr / k_papr, LinkEngine.papr,
Simulation(papr_ccdf=True)) against tests/papr_expect.py, the definition restated with the oracle.

Every case: the per-symbol (peak, sum) trace against the helper value by value (1e-12 relative in
complex128, 1e-4 in complex64), the histogram inside the helper's cumulative bracket (width 0 in
complex128: equality), every symbol counted, and the largest kept peak against LinkEngine.run's x_peak
of the same plan and seed.  Then caller bits, invariance under sym0 splits and batching (exact), the
refusals, the Simulation flag and two gloo ranks."""

import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT
from numpy.random import PCG64, Generator

import ofdm_oracle as O
import papr_expect as PX
import ofdm_based_systems.bits_generation.models as bg
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import LinkEngine
from ofdm_based_systems.simulation.models import DEFAULT_CHANNEL, Simulation

pytestmark = pytest.mark.gpu

H1 = np.array([1.0 + 0j])
PREC = {"f64": B.OFDM_F64, "f32": B.OFDM_F32}
EDGES = PX.ratios(PX.default_edges_db())
_cache = {}


def engine(case, precision="f64"):
    luts, sc = PX.case_plan(case)
    return LinkEngine(case["N"], case["cp"], H1, B.EQ_NONE, luts, sc, PREC[precision],
                      prefix=B.PREFIX_ZERO if case.get("zp") else B.PREFIX_CYCLIC,
                      modulator=B.MOD_SC if case.get("sc") else B.MOD_OFDM)


def symbols(case):
    return PX.case_symbols(case, torch.cuda.get_device_properties(0).multi_processor_count)


def expect(case, S):
    """The helper's (peak, sum, n) of a case, computed once and shared (never written to)."""
    key = (case["id"], S)
    if key not in _cache:
        peak, total, n = PX.case_expect(case, S)
        peak.setflags(write=False)
        total.setflags(write=False)
        _cache[key] = (peak, total, n)
    return _cache[key]


def common_checks(case, precision, what):
    S = symbols(case)
    eng = engine(case, precision)
    peak, total, n = expect(case, S)
    st = eng.papr(S, seed=PX.SEED, keep=S)
    got = st.per_symbol
    assert got.shape == (S, 2) and st.num_ofdm_symbols == S
    tol = PX.TOL[precision]
    err = max(float(np.max(np.abs(got[:, 0] - peak) / peak)), float(np.max(np.abs(got[:, 1] - total) / total)))
    print(f"{what} [{precision}] S = {S}: per-symbol relative error {err:.3e} (tolerance {tol:g})")
    assert err <= tol
    assert st.histogram.sum() == S
    PX.assert_in_bracket(st.histogram, peak, total, n, EDGES, precision, what)
    # the definition on the GPU's own pairs is its histogram, bit for bit (the comparison is in double)
    assert np.array_equal(st.histogram, PX.histogram(got[:, 0], got[:, 1], n, EDGES))
    # the run's peak statistic: k_tx's statements on the same templates
    run = eng.run(S, 20.0, seed=PX.SEED)
    top = float(got[:, 0].max())
    print(f"{what} [{precision}]: max peak {top!r}, run x_peak {run.x_peak!r}, equal {top == run.x_peak}")
    assert abs(top - run.x_peak) <= tol * run.x_peak
    return st


def by_id(cid):
    return next(c for c in PX.CASES + PX.MORE_CASES if c["id"] == cid)


# ---------------------------------------------------------------- 1. the throughput form
def test_throughput_form_n1024_covers_the_grid_loop_and_a_ragged_tail(gpu):
    """S = 2 x compute units x symbols per workgroup + 37: the grid-stride loop, a partial last
    workgroup and inactive symbol slots."""
    common_checks(by_id("n1024_qam64"), "f64", "throughput N = 1024 64-QAM")


def test_throughput_form_n4096_reduces_over_the_symbols_waves(gpu):
    common_checks(by_id("n4096_qam256_cp32"), "f64", "throughput N = 4096 256-QAM cp = 32")


@pytest.mark.parametrize("cid,per_cu", [("n4096_qam256_cp32", 4), ("n2048_adaptive", 16)])
def test_multi_wave_symbols_through_the_grid_stride_loop(gpu, cid, per_cu):
    """More symbols than two rounds of the resident workgroups hold (one 4-symbol workgroup per compute
    unit in the throughput form, at most four 2-symbol ones in the generic form): every workgroup
    reuses its symbols' rows, which carry the waves' partials between the transform's passes."""
    case = by_id(cid)
    S = 2 * torch.cuda.get_device_properties(0).multi_processor_count * per_cu + 37
    peak, total, n = expect(case, S)
    st = engine(case).papr(S, seed=PX.SEED, keep=S)
    assert np.max(np.abs(st.per_symbol[:, 0] - peak) / peak) <= 1e-12
    assert np.max(np.abs(st.per_symbol[:, 1] - total) / total) <= 1e-12
    PX.assert_in_bracket(st.histogram, peak, total, n, EDGES, "f64", f"{cid} S = {S}")


# ---------------------------------------------------------------- 2. the generic form
GENERIC = ["n1", "n2", "n8_qam16", "n16_qam16_cp0", "n16_qam4_cp5", "n64_qam16_cp16", "n64_qam64_cp0",
           "n32_qam64_cp8", "n256_qam16_cp20", "n2048_adaptive", "sc_qam4_n256", "sc_zp_qam16_n256_cp64",
           "sc_psk8_n64", "bpsk_n128"]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("cid", GENERIC)
def test_generic_form(gpu, cid, precision):
    common_checks(by_id(cid), precision, cid)


def test_generic_form_complex64_at_the_bench_shape(gpu):
    common_checks(by_id("n1024_qam64"), "f32", "generic N = 1024 64-QAM")


def test_generic_form_complex64_n4096(gpu):
    common_checks(by_id("n4096_qam256_cp32"), "f32", "generic N = 4096 256-QAM cp = 32")


# ---------------------------------------------------------------- 3. reference mode
@pytest.mark.parametrize("cid", ["n64_qam16_cp16", "n1024_qam64"])
def test_caller_bits(gpu, cid):
    """Seeded PCG64 bytes, as the parity tests draw them: the histogram is the helper's on those bits."""
    case = by_id(cid)
    N, S = case["N"], PX.S_of(case["N"])
    luts, _ = PX.case_plan(case)
    b = int(len(luts[0])).bit_length() - 1
    bits = np.frombuffer(O.generate_bits(S * N * b, Generator(PCG64(17))), np.uint8)
    peak, total, n = PX.per_symbol(N, case["cp"], S, luts, bits=bits)
    eng = engine(case)
    st = eng.papr(S, bits=bits, keep=S)
    assert np.max(np.abs(st.per_symbol[:, 0] - peak) / peak) <= 1e-12
    assert np.max(np.abs(st.per_symbol[:, 1] - total) / total) <= 1e-12
    PX.assert_in_bracket(st.histogram, peak, total, n, EDGES, "f64", cid + " caller bits")
    assert np.array_equal(st.histogram, PX.histogram(peak, total, n, EDGES))
    # Philox streams of the same plan give another histogram: the bits were read
    assert not np.array_equal(st.histogram, eng.papr(S, seed=PX.SEED).histogram)
    assert np.array_equal(eng.papr(S, bits=bits, batch=S // 3).histogram, st.histogram)


# ---------------------------------------------------------------- 4. invariance, exact
def abi_papr(eng, sym0, n_sym, hist, sym_out=None, keep=0, edges=EDGES, seed=PX.SEED):
    eng.papr_hist(eng.stream(), None, seed, sym0, n_sym, edges, hist, sym_out, keep)


@pytest.mark.parametrize("cid,precision", [("n1024_qam64", "f64"), ("n4096_qam256_cp32", "f64"),
                                           ("n64_qam16_cp16", "f32"), ("n2048_adaptive", "f64")])
def test_one_launch_ragged_pieces_and_batches_agree_exactly(gpu, cid, precision):
    case = by_id(cid)
    S = PX.S_of(case["N"]) if cid == "n1024_qam64" else symbols(case)
    eng = engine(case, precision)
    dev = eng.device()
    one = torch.zeros(65, dtype=torch.int64, device=dev)
    trace = torch.zeros((S + 5, 2), dtype=torch.float64, device=dev)
    abi_papr(eng, 0, S, one, trace, S + 5)  # sym_keep larger than n_sym
    assert not trace[S:].any() and bool((trace[:S, 0] > 0).all())
    pieces = torch.zeros(65, dtype=torch.int64, device=dev)
    cuts = [0, 1, S // 2 + 3, S]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        t = torch.zeros((hi - lo, 2), dtype=torch.float64, device=dev)
        abi_papr(eng, lo, hi - lo, pieces, t, hi - lo)
        parts.append(t)
    assert torch.equal(pieces, one) and int(one.sum()) == S
    assert torch.equal(torch.cat(parts), trace[:S])  # the same pairs bit for bit, whatever the grid
    before = one.clone()
    abi_papr(eng, 3, 0, one)  # an empty call
    assert torch.equal(one, before)
    abi_papr(eng, 0, S, one)  # accumulated, not zeroed
    assert torch.equal(one, 2 * before)
    batched = eng.papr(S, seed=PX.SEED, batch=max(1, S // 4 + 1), keep=7)
    assert np.array_equal(batched.histogram, before.cpu().numpy())
    assert np.array_equal(batched.per_symbol, trace[:7].cpu().numpy())


# ---------------------------------------------------------------- 5. refusals
def test_refusals_name_their_reason_and_launch_nothing(gpu):
    eng = engine(by_id("n64_qam16_cp16"))
    for edges_db, why in (([3.0, 2.0], "not above its predecessor"), ([1.0, 1.0], "not above its predecessor"),
                          ([1.0, float("nan")], "not a finite positive"), ([1.0, float("inf")], "not a finite positive"),
                          ([float("-inf"), 1.0], "not a finite positive"),
                          (np.linspace(0.0, 12.0, 129), "1 to 128 edges"), ([], "1 to 128 edges")):
        with pytest.raises(ValueError, match=why):
            eng.papr(16, edges_db=edges_db)
    hist = torch.zeros(3, dtype=torch.int64, device=eng.device())
    with pytest.raises(ValueError, match="not a finite positive"):
        abi_papr(eng, 0, 16, hist, edges=[0.0, 1.0])  # a zero ratio
    with pytest.raises(ValueError, match="ofdm_papr"):
        eng.papr_hist(eng.stream(), None, 0, 0, 16, [1.0, 2.0], None)  # no histogram
    assert not hist.any()
    assert eng.papr(16, edges_db=np.linspace(0.0, 12.0, 128)).histogram.sum() == 16
    wide = LinkEngine(64, 0, H1, B.EQ_NONE, [O.qam_lut(1024)])
    with pytest.raises(ValueError, match="at most 8 bits"):
        wide.papr(16)  # as ofdm_tx answers without caller bits
    with pytest.raises(ValueError, match="above 256 points"):
        wide.papr(16, bits=np.zeros(16 * 64 * 10 // 8, np.uint8))
    mixed = LinkEngine(64, 0, H1, B.EQ_NONE, [O.qam_lut(4), O.qam_lut(1024)], np.arange(64, dtype=np.int32) % 2)
    with pytest.raises(ValueError, match="ofdm_papr"):
        mixed.papr(16)


# ---------------------------------------------------------------- 6. Simulation(papr_ccdf=True)
def seeded(seed, **kw):
    bg.RandomBitsGenerator.__init__.__defaults__ = (Generator(PCG64(seed)),)
    np.random.seed(seed)
    return Simulation(num_symbols=64 * 64, num_subcarriers=64, constellation_order=16, snr_db=12.0, verbose=False,
                      make_plot=False, seed=seed, **kw).run()


@pytest.mark.parametrize("rng_mode", ["reference", "philox"])
def test_simulation_flag(gpu, rng_mode):
    seed, S, N = 21, 64, 64
    plain = seeded(seed, rng_mode=rng_mode)
    got = seeded(seed, rng_mode=rng_mode, papr_ccdf=True)
    assert set(got) - set(plain) == {"papr_ccdf"} and "papr_ccdf" not in plain
    for k in plain:
        if k == "transmission_time_ms":
            continue
        a, b = plain[k], got[k]
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, k
    rec = got["papr_ccdf"]
    assert set(rec) == {"edges_db", "ccdf", "histogram", "num_ofdm_symbols"}
    assert all(isinstance(rec[k], list) for k in ("edges_db", "ccdf", "histogram")) and rec["num_ofdm_symbols"] == S
    h = np.asarray(DEFAULT_CHANNEL, np.complex128)
    eng = LinkEngine(N, len(h) - 1, h, B.EQ_MMSE, [O.qam_lut(16)])
    bits = None
    if rng_mode == "reference":
        bits = np.frombuffer(O.generate_bits(S * N * 4, Generator(PCG64(seed))), np.uint8)
    want = eng.papr(S, seed=seed, bits=bits)
    assert rec["histogram"] == want.histogram.tolist() and sum(rec["histogram"]) == S
    assert rec["ccdf"] == want.ccdf.tolist() and rec["edges_db"] == PX.default_edges_db().tolist()
    few = seeded(seed, rng_mode=rng_mode, papr_ccdf=True, papr_edges_db=[2.0, 6.0])["papr_ccdf"]
    assert few["edges_db"] == [2.0, 6.0] and len(few["histogram"]) == 3 and sum(few["histogram"]) == S


# ---------------------------------------------------------------- 7. two gloo ranks on device 0
def test_two_ranks_hold_the_one_rank_histogram(gpu, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OFDM_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = tmp_path / "papr"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(ROOT, "tests", "papr_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    case = by_id("n1024_qam64")
    S = PX.S_of(case["N"])
    one = engine(case).papr(S, seed=PX.SEED, keep=S)
    for rank in (0, 1):
        got = json.loads((tmp_path / f"papr.{rank}.json").read_text())
        lo, hi = [[0, S // 2], [S // 2, S]][rank]
        assert got["world"] == 2 and got["shard"] == [lo, hi]
        assert got["histogram"] == one.histogram.tolist(), rank
        assert np.array_equal(np.asarray(got["kept"]), one.per_symbol[lo:lo + 4])

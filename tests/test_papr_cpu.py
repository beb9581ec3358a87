"""The per-symbol PAPR histogram (ofdm_papr, LinkEngine.papr, Simulation(papr_ccdf=True)) without a
GPU: the entry point's declaration, export and binding; the helper tests/papr_expect.py meeting the
bracket width caps on every case of the GPU table (the oracle alone: the conditions under which the
GPU test's bracket pins a histogram); PaprStats.ccdf on a hand-made histogram; the engine's batching
and all-reduce over a CPU test double; and the composed path's refusal."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import papr_expect as PX
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import LinkEngine, PaprStats, default_papr_edges_db, shard
from test_abi import HEADER, declared_functions
from test_distributed_cpu import _free_port


def test_entry_point_is_declared_exported_and_bound():
    assert "ofdm_papr" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_papr("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert decl == ("int ofdm_papr(ofdm_plan_t plan, void* stream, const uint8_t* bits, uint64_t seed, "
                    "int64_t sym0, int64_t n_sym, const double* edges, int32_t n_edges, "
                    "uint64_t* hist, double* sym_out, int64_t sym_keep)")
    at = text.index("int ofdm_papr(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "OFDM_E_INVALID" in comment and "HOST array" in comment and "accumulated" in comment
    assert int(re.search(r"#define OFDM_MAX_PAPR_EDGES (\d+)", text).group(1)) == B.MAX_PAPR_EDGES == 128
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    f64p = ctypes.POINTER(ctypes.c_double)
    assert B.SIGNATURES["ofdm_papr"] == (ctypes.c_int, [vp, vp, vp, u64, i64, i64, f64p, i32, vp, vp, i64])
    assert set(B.SIGNATURES) == set(declared_functions())
    lib = B.load_library()
    assert hasattr(lib, "ofdm_papr") and lib.ofdm_abi_version() == B.ABI_VERSION


def test_null_plan_is_invalid_without_a_gpu():
    lib = B.load_library()
    edges = (ctypes.c_double * 2)(1.0, 2.0)
    assert lib.ofdm_papr(None, None, None, 0, 0, 4, edges, 2, None, None, 0) == -1
    assert b"ofdm_papr" in lib.ofdm_last_error()


@pytest.mark.parametrize("case", PX.CASES, ids=lambda c: c["id"])
def test_the_helper_meets_the_width_caps(case):
    """On the default edge grid every complex128 bracket has width 0 and every complex64 one is within
    max(4, 5 % of S): the GPU test's bracket then pins the complex128 histogram exactly."""
    S = PX.case_symbols(case)
    peak, total, n = PX.case_expect(case, S)
    edges = PX.ratios(PX.default_edges_db())
    assert n == case["N"] + case["cp"] and peak.shape == total.shape == (S,)
    for precision in ("f64", "f32"):
        lo, hi = PX.bracket(peak, total, n, edges, PX.DELTA[precision])
        width = int((hi - lo).max())
        print(f"{case['id']} S = {S} {precision}: bracket width {width}")
        assert width <= PX.width_cap(precision, S)
        assert np.all(lo[:-1] >= lo[1:]) and np.all(hi[:-1] >= hi[1:])
    # the definition on the helper's own pairs lies inside its bracket and counts every symbol
    h = PX.histogram(peak, total, n, edges)
    assert h.sum() == S and np.array_equal(PX.cumulative(h), PX.bracket(peak, total, n, edges, 1e-9)[0])
    # (the distribution is not degenerate: OFDM spreads over many bins, single carrier sits low)
    if not case.get("sc") and case["N"] >= 32:
        assert np.count_nonzero(h) >= 8


def test_constant_envelope_symbols_sit_below_the_first_positive_edge():
    """SC 4-QAM / 8-PSK and N = 1: ratio exactly 1 up to rounding -- bin 1 of the offset grid (between
    -0.125 and +0.125 dB), which is why the grid keeps 0 dB out of the edge set."""
    edges = PX.ratios(PX.default_edges_db())
    for cid in ("sc_qam4_n256", "sc_psk8_n64", "n1"):
        case = next(c for c in PX.CASES if c["id"] == cid)
        S = PX.case_symbols(case)
        peak, total, n = PX.case_expect(case, S)
        h = PX.histogram(peak, total, n, edges)
        assert h[1] == S, (cid, np.nonzero(h)[0])


def test_a_symbol_without_power_lands_in_the_last_bin():
    edges = PX.ratios(PX.default_edges_db())
    h = PX.histogram(np.array([0.0, 2.0]), np.array([0.0, 4.0]), 4, edges)
    assert h[len(edges)] == 1 and h.sum() == 2
    lo, hi = PX.bracket(np.array([0.0]), np.array([0.0]), 4, edges, 1e-9)
    assert np.all(lo == 1) and np.all(hi == 1)


def test_ccdf_arithmetic():
    st = PaprStats(edges_db=np.array([0.0, 3.0, 6.0]), histogram=np.array([1, 2, 3, 4], np.int64), num_ofdm_symbols=10,
                   per_symbol=np.array([[4.0, 8.0], [1.0, 4.0], [0.0, 0.0]]), samples_per_symbol=4)
    assert st.ccdf.dtype == np.float64 and np.array_equal(st.ccdf, np.array([0.9, 0.7, 0.4]))
    db = st.papr_db_per_symbol
    assert np.allclose(db[:2], [10 * np.log10(2.0), 0.0]) and np.isinf(db[2])
    assert PaprStats(np.array([0.0]), np.array([0, 0], np.int64), 0).ccdf.tolist() == [0.0]
    assert PaprStats(np.array([0.0]), np.array([0, 5], np.int64), 5).papr_db_per_symbol is None
    e = default_papr_edges_db()
    assert len(e) == 64 and e[0] == -0.125 and e[63] == 15.625 and 0.0 not in e
    assert np.array_equal(e, PX.default_edges_db())


# ------------------------------------------------------------------ the engine over a CPU double
DOUBLE = dict(N=64, cp=16, M=16, S=53, seed=9)


class PaprDouble(LinkEngine):
    """LinkEngine whose ofdm_papr is the helper's definition on the CPU (test double), every call logged
    as (sym0, n_sym, edges, sym_keep)."""

    def __init__(self, N, cp, M):
        self.n_fft, self.cp = N, cp
        self.lut = PX.QAM(M)
        self.bps = N * (int(M).bit_length() - 1)
        self.adaptive = False
        self.log = []

    def device(self):
        return torch.device("cpu")

    def stream(self):
        return None

    def papr_hist(self, stream, bits_d, seed, sym0, n_sym, edges, hist, sym_out=None, sym_keep=0):
        self.log.append((int(sym0), int(n_sym), len(edges), int(sym_keep)))
        if n_sym == 0:
            return
        bits = None if bits_d is None else bits_d.numpy()
        peak, total, n = PX.per_symbol(self.n_fft, self.cp, n_sym, [self.lut], seed=seed, bits=bits, sym0=sym0)
        hist += torch.from_numpy(PX.histogram(peak, total, n, edges))
        k = min(int(sym_keep), n_sym)
        if sym_out is not None and k:
            sym_out[:k] = torch.from_numpy(np.stack([peak, total], axis=1)[:k])


def double():
    return PaprDouble(DOUBLE["N"], DOUBLE["cp"], DOUBLE["M"])


def whole_run(**kw):
    peak, total, n = PX.per_symbol(DOUBLE["N"], DOUBLE["cp"], DOUBLE["S"], [PX.QAM(DOUBLE["M"])], seed=DOUBLE["seed"], **kw)
    return PX.histogram(peak, total, n, PX.ratios(PX.default_edges_db())), np.stack([peak, total], axis=1)


def test_batches_add_integer_histograms_and_the_trace_spans_them():
    S, seed = DOUBLE["S"], DOUBLE["seed"]
    want, pairs = whole_run()
    eng = double()
    one = eng.papr(S, seed=seed)
    assert eng.log == [(0, S, 64, 0)]
    assert one.histogram.dtype == np.int64 and np.array_equal(one.histogram, want) and one.per_symbol is None
    assert one.num_ofdm_symbols == S and np.array_equal(one.edges_db, PX.default_edges_db())
    eng.log.clear()
    got = eng.papr(S, seed=seed, batch=20, keep=25)
    assert eng.log == [(0, 20, 64, 25), (20, 20, 64, 5), (40, 13, 64, 0)]
    assert np.array_equal(got.histogram, want) and np.array_equal(got.per_symbol, pairs[:25])
    assert np.array_equal(got.ccdf, PX.cumulative(want) / S)
    more = eng.papr(S, seed=seed, keep=10 * S, edges_db=[0.5, 3.0, 9.0])
    assert more.per_symbol.shape == (S, 2) and more.histogram.shape == (4,) and more.histogram.sum() == S
    assert np.allclose(more.papr_db_per_symbol, 10 * np.log10(PX.symbol_ratio(pairs[:, 0], pairs[:, 1], 80)))
    eng.log.clear()
    empty = eng.papr(0, seed=seed)
    assert eng.log == [(0, 0, 64, 0)] and not empty.histogram.any() and empty.ccdf.tolist() == [0.0] * 64


def test_caller_bits_go_to_every_batch():
    S = DOUBLE["S"]
    rng = np.random.Generator(np.random.PCG64(4))
    bits = np.frombuffer(rng.bytes(S * DOUBLE["N"] * 4 // 8), np.uint8)
    want, _ = whole_run(bits=bits)
    assert not np.array_equal(want, whole_run()[0])
    got = double().papr(S, bits=bits, batch=17)
    assert np.array_equal(got.histogram, want)
    with pytest.raises(ValueError):
        double().papr(S, bits=bits[:-8])


def _rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = double()
    st = eng.papr(DOUBLE["S"], seed=DOUBLE["seed"], group=dist.group.WORLD, batch=11, keep=3)
    out[rank] = (st.histogram.tolist(), eng.log, st.per_symbol.tolist())
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_all_reduce_the_histograms(world):
    want, pairs = whole_run()
    out = mp.Manager().dict()
    mp.spawn(_rank, args=(world, _free_port(), out), nprocs=world, join=True)
    for r in range(world):
        hist, log, kept = out[r]
        lo, hi = shard(DOUBLE["S"], r, world)
        assert hist == want.tolist(), r
        assert [c[0] for c in log] == list(range(lo, hi, 11)) and sum(c[1] for c in log) == hi - lo
        assert np.array_equal(np.asarray(kept), pairs[lo:lo + 3])  # the shard's first symbols


# ------------------------------------------------------------------ Simulation
def test_simulation_refuses_the_flag_on_the_composed_path(monkeypatch):
    from ofdm_based_systems.configuration.enums import ModulationType
    from ofdm_based_systems.modulation.models import OFDMModulator
    from ofdm_based_systems.simulation.models import Simulation

    class Custom(OFDMModulator):  # a user-supplied strategy: the composed GPU operators
        pass

    monkeypatch.setitem(Simulation.MODULATOR_SCHEME_MAPPERS, ModulationType.OFDM, Custom)
    # (the channel gains come from a plan on the GPU: computed on the host here)
    monkeypatch.setattr(Simulation, "_channel_gains",
                        lambda self, h: np.abs(np.fft.fft(h, self.num_subcarriers)) ** 2)
    sim = Simulation(num_symbols=64 * 8, num_subcarriers=64, constellation_order=16, verbose=False,
                     make_plot=False, papr_ccdf=True)
    assert sim.papr_ccdf and sim.papr_edges_db is None
    with pytest.raises(ValueError, match="papr_ccdf needs the built-in"):
        sim.run()
    assert not Simulation(num_symbols=8, verbose=False).papr_ccdf

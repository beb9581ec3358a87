"""The clipped transmitter (ofdm_tx_clip, LinkEngine(clip_db=...), Simulation(clip_db=...)) without a GPU:
the entry point's declaration, export and binding; the helper tests/clip_expect.py meeting the count
bracket's width caps on every case of the table the GPU tests share; the definition's sanity against
Bussgang's theorem; and the engine's schedule over a fake library -- which transmit counts, the
all-reduce of the record, and the refusals."""

import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import clip_expect as CX
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import LinkEngine, clip_threshold, nominal_sample_power
from test_abi import HEADER, declared_functions
from test_distributed_cpu import _free_port


def test_entry_point_is_declared_exported_and_bound():
    assert "ofdm_tx_clip" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_tx_clip("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert decl == ("int ofdm_tx_clip(ofdm_plan_t plan, void* stream, const uint8_t* bits, uint64_t seed, "
                    "int64_t sym0, int64_t n_sym, void* y, ofdm_stats* stats, "
                    "double clip_a2, uint64_t* clip_counters)")
    at = text.index("int ofdm_tx_clip(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "OFDM_E_INVALID" in comment and "sqrt(A2 / p)" in comment and "accumulated" in comment
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    vp, i64, u64, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    assert B.SIGNATURES["ofdm_tx_clip"] == (ctypes.c_int, [vp, vp, vp, u64, i64, i64, vp, vp, f64, vp])
    assert B.SIGNATURES["ofdm_tx"] == (ctypes.c_int, [vp, vp, vp, u64, i64, i64, vp, vp])  # as it was
    assert set(B.SIGNATURES) == set(declared_functions())
    lib = B.load_library()
    assert hasattr(lib, "ofdm_tx_clip") and lib.ofdm_abi_version() == B.ABI_VERSION


def test_null_plan_and_bad_threshold_are_invalid_without_a_gpu():
    lib = B.load_library()
    assert lib.ofdm_tx_clip(None, None, None, 0, 0, 4, None, None, 1.0, None) == -1
    assert b"ofdm_tx_clip" in lib.ofdm_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ofdm_tx_clip(None, None, None, 0, 0, 4, None, None, bad, None) == -1


# ------------------------------------------------------------------ the helper
@pytest.fixture(scope="module")
def expect():
    cache = {}

    def get(case):
        if case["id"] not in cache:
            cache[case["id"]] = CX.case_expect(case)
        return cache[case["id"]]
    return get


@pytest.mark.parametrize("case", CX.CASES, ids=lambda c: c["id"])
def test_the_helper_meets_the_width_caps(case, expect):
    """complex128: the count bracket has width 0, so the GPU test asserts equality; complex64: at most
    max(4, samples / 1000)."""
    ref = expect(case)
    a2 = CX.case_threshold(case)
    S = CX.case_symbols(case)
    assert ref.samples == S * case["N"] and ref.p.shape == (S, case["N"])
    for precision in ("f64", "f32"):
        lo, hi = ref.count_bracket(precision, a2)
        print(f"{case['id']} {precision}: clipped {ref.clipped} of {ref.samples}, bracket width {hi - lo}")
        assert lo <= ref.clipped <= hi
        assert hi - lo <= CX.count_width_cap(precision, ref.samples), (case["id"], precision, hi - lo)
    # no tie in the table: no sample sits on the threshold
    assert not np.any(ref.p == a2)
    # the limited stream's peak is the threshold wherever anything clips
    if ref.clipped:
        assert ref.x_peak == pytest.approx(a2, rel=1e-12)
    else:
        assert ref.x_peak < a2


def test_the_corner_cases_of_the_table(expect):
    by = {c["id"]: c for c in CX.CASES}
    sc16 = expect(by["sc_qam16_n256_1db"])
    # single-carrier 16-QAM at 1 dB: only the outer corners (power 1.8) clip
    assert sc16.clipped == int(np.count_nonzero(np.isclose(sc16.p, 1.8))) > 0
    assert expect(by["sc_qam4_n64_3db"]).clipped == 0
    n1 = expect(by["n1_qam4_m3db"])
    assert n1.clipped == n1.samples  # every sample clips
    n2 = expect(by["n2_qam4_05db"])
    assert 0 < n2.clipped < n2.samples


@pytest.mark.parametrize("cid,want", [("n1024_qam64_4db", 0.9189), ("n1024_qam64_1db", 0.7160)])
def test_output_power_follows_bussgang(cid, want, expect):
    """E|x'|^2 / P = 1 - exp(-g2), g2 = A2 / P, for a complex Gaussian x: within 1 %."""
    case = next(c for c in CX.CASES if c["id"] == cid)
    ref = expect(case)
    g2 = 10.0 ** (case["clip_db"] / 10.0)
    assert 1.0 - np.exp(-g2) == pytest.approx(want, abs=5e-5)
    pn = CX.nominal_power(case["N"], *CX.case_plan(case))
    got = ref.x_power_sum / ref.samples / pn
    print(f"{cid}: output power / P_nom {got:.4f}, Bussgang {1.0 - np.exp(-g2):.4f}")
    assert got == pytest.approx(1.0 - np.exp(-g2), rel=0.01)


def test_a_high_level_leaves_the_stream_bit_identical():
    case = next(c for c in CX.CASES if c["id"] == "n64_qam16_3db")
    luts, sc = CX.case_plan(case)
    a2 = CX.threshold(40.0, case["N"], luts, sc)
    h = np.array([0.8, 0.5 - 0.3j, 0.1j])
    kw = dict(noise_on=False)
    clipped = CX.run_clipped(CX.SEED, 40, 64, 16, h, 2, "MMSE", 20.0, a2, **kw)
    plain = CX.run_clipped(CX.SEED, 40, 64, 16, h, 2, "MMSE", 20.0, a2, clip=False, **kw)
    assert clipped.clipped == 0 and np.array_equal(clipped.y, plain.y)
    assert (clipped.power_sum, clipped.x_power_sum, clipped.x_peak) == (plain.power_sum, plain.x_power_sum, plain.x_peak)
    # and the restatement without the limiter is the oracle's own run
    import philox_streams as P
    ref = P.run_philox(CX.SEED, 40, 64, 16, h, 2, "MMSE", 20.0, noise_on=False)
    assert np.array_equal(plain.y, ref.y) and (plain.bit_errors, plain.symbol_errors) == (ref.bit_errors, ref.symbol_errors)


def test_a_leading_zero_tap_is_a_delay():
    """h = [0, 0.8, 0.6j]: |h0|^2 = 0.  The restatement's stored samples are the limited stream delayed --
    y[n] = 0.8 s'[n - 1] + 0.6j s'[n - 2] over the serial stream with its prefixes -- and it clips as the
    one-tap restatement of the same plan does."""
    import ofdm_oracle as O
    import philox_streams as P

    case = next(c for c in CX.CASES if c["id"] == "n64_qam16_lead0_3db")
    h = CX.case_taps(case, None)
    assert h[0] == 0 and np.sum(np.abs(h) ** 2) == pytest.approx(1.0)
    S, N, cp, a2 = 40, 64, 2, CX.case_threshold(case)
    ref = CX.case_expect(case, h=h, cp=cp, eq="MMSE", S=S)
    idx = P.tx_indices(P.lane_generators(CX.SEED, np.arange(S), N), S, N, 4)
    s_t, p = CX.limit(np.fft.ifft(CX.QAM(16)[idx], axis=1, norm="ortho"), a2)
    s = O.add_cp(s_t, cp).ravel()
    y = 0.8 * np.concatenate([[0], s[:-1]]) + 0.6j * np.concatenate([[0, 0], s[:-2]])
    assert np.allclose(ref.y, y.reshape(S, N + cp)[:, cp:], rtol=0, atol=1e-14)
    assert ref.clipped == int(np.count_nonzero(p > a2)) == CX.case_expect(case, S=S).clipped > 0


def test_threshold_arithmetic():
    luts, sc = CX.PX.adaptive_2048()
    pn = nominal_sample_power(2048, luts, sc)
    assert pn == CX.nominal_power(2048, luts, sc)
    assert pn == pytest.approx(np.count_nonzero(sc >= 0) / 2048, rel=1e-12)  # unit-power LUTs, inactive ones 0
    assert clip_threshold(3.0, pn) == 10.0 ** 0.3 * pn == CX.threshold(3.0, 2048, luts, sc)
    assert nominal_sample_power(64, [CX.QAM(16)]) == pytest.approx(1.0, rel=1e-12)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e6):
        with pytest.raises(ValueError, match="clip_db"):
            clip_threshold(bad, 1.0)


# ------------------------------------------------------------------ the schedule over a fake library
class FakeLib:
    """Stands in for libofdm_hip: every call logged with its arguments; ofdm_tx_clip adds a fixed count per
    symbol to the record it is given."""
    CLIPPED_PER_SYMBOL = 3

    def __init__(self, N):
        self.N, self.calls = N, []

    def _log(self, name, args):
        self.calls.append((name,) + tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args))
        return 0

    def ofdm_tx(self, *args):
        assert len(args) == 8
        return self._log("ofdm_tx", args)

    def ofdm_tx_clip(self, *args):
        assert len(args) == 10
        plan, stream, bits, seed, sym0, n_sym, y, stats, a2, rec = args
        if rec is not None:
            t = (ctypes.c_int64 * 2).from_address(rec.value)
            t[0] += self.CLIPPED_PER_SYMBOL * n_sym
            t[1] += self.N * n_sym
        return self._log("ofdm_tx_clip", args)

    def ofdm_rx(self, *args):
        return self._log("ofdm_rx", args)

    def ofdm_rx_profile(self, *args):
        return self._log("ofdm_rx_profile", args)

    def ofdm_rx_sweep(self, *args):
        return self._log("ofdm_rx_sweep", args[:6] + (list(args[6][:args[7]]),) + args[7:])

    def ofdm_link(self, *args):
        raise AssertionError("a clipped engine never reaches ofdm_link")

    def ofdm_papr(self, *args):
        raise AssertionError("a clipped engine never reaches ofdm_papr")


class Double(LinkEngine):
    """LinkEngine over FakeLib on CPU tensors: the schedule and the plumbing are the production code."""

    def __init__(self, N=64, cp=4, clip_db=None):
        self.n_fft, self.cp, self.ystride = N, cp, N
        self.bps, self.adaptive, self.cdtype = 4 * N, False, torch.complex128
        self.bits_per_subcarrier = np.full(N, 4, dtype=np.int64)
        self.plan = SimpleNamespace(handle=ctypes.c_void_p(0x1000))
        self._lib = FakeLib(N)
        self._fused = False
        self.nominal_power = nominal_sample_power(N, [CX.QAM(16)])
        if clip_db is not None:
            self.clip_db, self.clip_a2 = float(clip_db), clip_threshold(clip_db, self.nominal_power)

    def device(self):
        return torch.device("cpu")

    def stream(self):
        return None

    def names(self):
        return [c[0] for c in self._lib.calls]


S = 10


def test_without_a_clip_level_the_calls_are_todays():
    eng = Double()
    assert eng.clip_a2 is None and eng.clip_db is None
    st = eng.run(S, 12.0, seed=5, batch=4)
    assert eng.names() == ["ofdm_tx", "ofdm_tx", "ofdm_rx", "ofdm_tx", "ofdm_rx", "ofdm_tx", "ofdm_rx"]
    first = eng._lib.calls[0]
    assert first[0] == "ofdm_tx" and len(first) == 9 and first[3:7] == (None, 5, 0, S) and first[7] is None
    assert (st.clip_db, st.clipped_samples, st.clip_samples) == (None, None, None)
    eng = Double()
    sw = eng.run_sweep(S, [8.0, 12.0], seed=5)
    assert eng.names() == ["ofdm_tx", "ofdm_rx_sweep"] and all(s.clipped_samples is None for s in sw)
    assert "ofdm_tx_clip" not in eng.names()


def test_resident_path_counts_once():
    eng = Double(clip_db=3.0)
    st = eng.run(S, 12.0, seed=5)
    assert eng.names() == ["ofdm_tx_clip", "ofdm_rx"]
    call = eng._lib.calls[0]
    assert call[9] == eng.clip_a2 == 10.0 ** 0.3 * eng.nominal_power and call[10] is not None
    assert (st.clip_db, st.clipped_samples, st.clip_samples) == (3.0, 3 * S, 64 * S)
    assert (st.bit_errors, st.symbol_errors) == (0, 0)  # the record sits behind the counters, not in them


def test_batched_path_counts_in_the_power_pass_only():
    eng = Double(clip_db=3.0)
    st = eng.run(S, 12.0, seed=5, batch=4, profile=True)
    assert eng.names() == ["ofdm_tx_clip", "ofdm_tx_clip", "ofdm_rx_profile", "ofdm_tx_clip", "ofdm_rx_profile",
                           "ofdm_tx_clip", "ofdm_rx_profile"]
    tx = [c for c in eng._lib.calls if c[0] == "ofdm_tx_clip"]
    assert tx[0][5:8] == (0, S, None) and tx[0][10] is not None          # the power pass: no y, the record
    assert [c[5:7] for c in tx[1:]] == [(0, 4), (4, 4), (8, 2)]
    assert all(c[7] is not None and c[10] is None for c in tx[1:])       # the batches: y, no record
    assert all(c[9] == eng.clip_a2 for c in tx)
    assert (st.clipped_samples, st.clip_samples) == (3 * S, 64 * S)
    assert st.profile is not None and not st.profile.bit_errors.any()    # the profile record behind the clip record


def test_sweep_carries_the_record():
    eng = Double(clip_db=1.0)
    out = eng.run_sweep(S, [8.0, 12.0, 10.0], seed=5, batch=6)
    assert eng.names() == ["ofdm_tx_clip", "ofdm_tx_clip", "ofdm_rx_sweep", "ofdm_tx_clip", "ofdm_rx_sweep"]
    assert [c[10] is not None for c in eng._lib.calls if c[0] == "ofdm_tx_clip"] == [True, False, False]
    assert len(out) == 3 and all((s.clip_db, s.clipped_samples, s.clip_samples) == (1.0, 3 * S, 64 * S) for s in out)


def _rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = Double(clip_db=3.0)
    st = eng.run(11, 12.0, seed=5, group=dist.group.WORLD)
    sw = eng.run_sweep(11, [8.0, 9.0], seed=5, group=dist.group.WORLD, batch=2)
    out[rank] = (st.clipped_samples, st.clip_samples, [(s.clipped_samples, s.clip_samples) for s in sw],
                 [c[5:7] for c in eng._lib.calls if c[0] == "ofdm_tx_clip" and c[10] is not None])
    dist.destroy_process_group()


def test_ranks_all_reduce_the_record():
    out = mp.Manager().dict()
    mp.spawn(_rank, args=(2, _free_port(), out), nprocs=2, join=True)
    for r in range(2):
        clipped, seen, sweep, counted = out[r]
        assert (clipped, seen) == (3 * 11, 64 * 11) and sweep == [(3 * 11, 64 * 11)] * 2
        lo, hi = (11 * r) // 2, (11 * (r + 1)) // 2
        assert counted == [(lo, hi - lo), (lo, hi - lo)]  # each rank counts its own shard, once per run


def test_refusals_raise_before_any_call():
    eng = Double(clip_db=3.0)
    with pytest.raises(ValueError, match="no clip level"):
        eng.run(S, 12.0, seed=5, fused=True)
    with pytest.raises(ValueError, match="papr"):
        eng.papr(S, seed=5)
    with pytest.raises(ValueError, match="run_pipelined"):
        eng.run_pipelined(S, 12.0, [1, 2])
    assert eng._lib.calls == []
    with pytest.raises(ValueError, match="above 256 points"):
        LinkEngine(64, 0, np.array([1.0 + 0j]), B.EQ_NONE, [CX.QAM(1024)], clip_db=3.0)


def test_simulation_refusals(monkeypatch):
    from ofdm_based_systems.configuration.enums import ModulationType
    from ofdm_based_systems.modulation.models import OFDMModulator
    from ofdm_based_systems.simulation import models as M
    from ofdm_based_systems.simulation.models import Simulation

    def no_launch(*a, **k):
        raise AssertionError("refused before anything is launched")

    monkeypatch.setattr(Simulation, "_channel_gains", no_launch)
    monkeypatch.setattr(M, "LinkEngine", no_launch)
    kw = dict(num_symbols=64 * 8, num_subcarriers=64, verbose=False, make_plot=False, clip_db=3.0)
    with pytest.raises(ValueError, match="papr_ccdf with clip_db"):
        Simulation(constellation_order=16, papr_ccdf=True, **kw).run()
    with pytest.raises(ValueError, match="orders up to 256"):
        Simulation(constellation_order=1024, **kw).run()

    class Custom(OFDMModulator):  # a user-supplied strategy: the composed GPU operators
        pass

    monkeypatch.setitem(Simulation.MODULATOR_SCHEME_MAPPERS, ModulationType.OFDM, Custom)
    with pytest.raises(ValueError, match="clip_db needs the built-in"):
        Simulation(constellation_order=16, **kw).run()
    assert Simulation(num_symbols=8, verbose=False).clip_db is None


def test_settings_carry_the_level():
    from ofdm_based_systems.configuration.models import SimulationSettings
    from ofdm_based_systems.simulation.models import Simulation

    base = dict(num_bands=64, signal_noise_ratios=[10.0, 12.0], channel_model_path="", num_symbols=512,
                constellation_order=16)
    s = SimulationSettings(**base)
    assert s.clip_db is None and all(x.clip_db is None for x in Simulation.create_from_simulation_settings(s))
    s = SimulationSettings(**base, clip_db=4.5)
    assert [x.clip_db for x in Simulation.create_from_simulation_settings(s)] == [4.5, 4.5]

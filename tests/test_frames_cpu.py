"""The per-frame error record (ofdm_rx_frames, LinkEngine.run(frame_symbols=F), engine.FrameStats)
without a GPU: the entry point's declaration, export, binding and refusals, the expectation helper
against the pinned totals of the stage fixtures, FrameStats against plain NumPy, the engine's schedule
over the oracle's CPU test double (whose rx fills the record from one-symbol oracle calls) resident,
batched and under gloo with frames straddling the shard boundaries, and the Simulation / settings
refusals.

On the commit before the record test_entry_point_is_declared_exported_and_bound fails (no such entry
point), as does everything that passes ``frame_symbols``."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from conftest import channel, stage_arrays

import frames_expect as FE
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.configuration.models import SimulationSettings
from ofdm_based_systems.simulation.models import Simulation
from test_distributed_cpu import CASE, _free_port
from test_sweep_cpu import SweepEngine

SEED = 21
RX_ARGS = 17  # ofdm_rx's


# ---------------------------------------------------------------- the ABI boundary
def test_entry_point_is_declared_exported_and_bound():
    from test_abi import HEADER, declared_functions

    assert "ofdm_rx_frames" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_rx_frames("):]
    decl = decl[:decl.index(";")]
    assert "int64_t frame_len, int64_t n_frames, uint64_t* frames" in decl
    at = text.index("int ofdm_rx_frames(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "floor(s / F)" in comment and "never zeroed" in comment
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    lib = B.load_library()
    assert hasattr(lib, "ofdm_rx_frames") and "ofdm_rx_frames" in B.SIGNATURES
    # ofdm_rx's arguments, then frame_len, n_frames and the record
    assert B.SIGNATURES["ofdm_rx_frames"][1] == B.SIGNATURES["ofdm_rx"][1] + [ctypes.c_int64, ctypes.c_int64,
                                                                            ctypes.c_void_p]
    assert len(B.SIGNATURES["ofdm_rx"][1]) == RX_ARGS
    assert set(B.SIGNATURES) == set(declared_functions())


def rx_args(sym0=0, n_sym=0, counters=True):
    cnt = (ctypes.c_uint64 * 2)()
    args = [None, None, None, None, None, 0, None, 0, 0.0, 0, None, sym0, n_sym, 0,
            ctypes.cast(cnt, ctypes.c_void_p) if counters else None, None, 0]
    assert len(args) == RX_ARGS
    return args, cnt


@pytest.mark.parametrize("sym0,n_sym,frame_len,n_frames,record,reason", [
    (0, 8, 4, 2, False, "needs a frame record"),
    (0, 8, 0, 2, True, "frame_len 0"),
    (0, 8, -3, 2, True, "frame_len -3"),
    (0, 8, 4, 0, True, "n_frames 0"),
    (0, 8, 4, -1, True, "n_frames -1"),
    (0, 9, 4, 2, True, "last symbol 8 lies in frame 2"),      # floor(8 / 4) = 2 >= 2
    (5, 4, 3, 2, True, "last symbol 8 lies in frame 2"),      # sym0 counts: floor(8 / 3) = 2
    (0, (1 << 31) + 1, 1 << 40, 1, True, "at most 2^31 symbols"),
    ((1 << 63) - 2, 4, 3, 10, True, "last symbol 9223372036854775809 lies in frame"),   # no signed overflow
    (0, 8, 4, 2, True, "needs a constellation"),              # the record fits: ofdm_rx's own refusal
    (0, 0, 4, 2, True, "needs a constellation"),
    (3, 6, 3, 3, True, "needs a constellation"),              # floor(8 / 3) = 2 < 3
])
def test_refusals_name_the_function_without_a_device(sym0, n_sym, frame_len, n_frames, record, reason):
    lib = B.load_library()
    args, _ = rx_args(sym0, n_sym)
    rec = (ctypes.c_uint64 * (2 * max(n_frames, 1)))()
    rc = lib.ofdm_rx_frames(*args, frame_len, n_frames, ctypes.cast(rec, ctypes.c_void_p) if record else None)
    msg = lib.ofdm_last_error().decode()
    assert rc == -1 and "ofdm_rx_frames" in msg and reason in msg, msg
    assert not any(rec)


def test_what_ofdm_rx_refuses_is_refused():
    lib = B.load_library()
    rec = (ctypes.c_uint64 * 4)()
    for kw in (dict(sym0=-1, n_sym=4), dict(n_sym=-1), dict(counters=False)):
        args, _ = rx_args(**kw)
        assert lib.ofdm_rx_frames(*args, 4, 2, ctypes.cast(rec, ctypes.c_void_p)) == -1
        assert "ofdm_rx_frames" in lib.ofdm_last_error().decode()
        assert lib.ofdm_rx(*args) == -1


# ---------------------------------------------------------------- the helper against the pinned totals
@pytest.mark.parametrize("st", FE.all_stages(), ids=lambda s: s["name"])
def test_per_symbol_counts_sum_to_the_pinned_totals(st):
    a = stage_arrays(st["name"])
    N, S, b = st["N"], st["S"], int(np.log2(st["M"]))
    bk = np.full(N, b, np.int64)
    be, se = FE.per_symbol_from_bytes(a["tx_bytes"], a["rx_bytes"], bk, S, S * N * b)
    assert be.shape == se.shape == (S,)
    assert (int(be.sum()), int(se.sum())) == (st["bit_errors"], st["symbol_errors"])
    assert np.all(se <= be) and np.all(be <= b * se)
    if st["name"] == "n64_m4_flat_none":
        assert be.tolist() == [7, 2, 8, 4, 5, 4, 0, 8]
    if st["name"] == "n64_m1024_severe_cp_mmse":
        assert be.tolist() == [7, 7, 5, 5, 4, 7, 5, 7, 3, 2, 3, 8, 6, 2, 2, 4]  # (the reference's own bytes)
    # the demapper's route gives the same counts
    idx = FE.PE.tx_indices(a["tx_bytes"], bk, S)
    zbe, zse = FE.per_symbol_from_z(a["Z"], idx, bk, S * N * b)
    assert np.array_equal(zbe, be) and np.array_equal(zse, se)
    for F in (1, 3, S, S + 1):
        assert int(FE.frame_sums(be, F).sum()) == st["bit_errors"] and len(FE.frame_sums(be, F)) == -(-S // F)
    assert np.array_equal(FE.frame_sums(be, 1), be)


def test_helper_masks_a_trailing_partial_byte_and_places_frames_globally():
    bk = np.array([2, 0, 4], np.int64)
    tx = np.zeros(2, np.uint8)
    rx = np.full(2, 0xFF, np.uint8)
    be, se = FE.per_symbol_from_bytes(tx, rx, bk, 2, 8)      # 12 bits, 8 compared
    assert be.tolist() == [6, 2] and se.tolist() == [2, 2]
    # symbols [5, 9) in frames of 3: frames 1 (symbol 5), 2 (6, 7, 8)
    assert FE.frame_sums([1, 2, 3, 4], 3, sym0=5).tolist() == [0, 1, 9]


# ---------------------------------------------------------------- FrameStats
def frame_stats(e, S, F, bits=12, n_valid=None):
    e = np.asarray(e, np.int64)
    return E.FrameStats(frame_symbols=F, n_symbols=S, bits_per_symbol=bits, bit_errors=e,
                        symbol_errors=np.minimum(e, 1), n_valid_bits=n_valid)


@pytest.mark.parametrize("S,F", [(10, 1), (10, 3), (10, 4), (12, 4), (5, 5)])
def test_frame_stats_equal_the_numpy_formulas(S, F):
    rng = np.random.default_rng(S * 31 + F)
    per = rng.integers(0, 4, S) * (rng.random(S) < 0.6)
    e = FE.frame_sums(per, F)
    fs = frame_stats(e, S, F)
    want = FE.stats(e, S, F, 12)
    assert fs.n_full == want["n_full"] == S // F and len(fs.bit_errors) == -(-S // F)
    assert fs.frame_errors == want["frame_errors"] and fs.fer == want["fer"]
    assert np.array_equal(fs.errors_per_frame_hist(), want["hist"])
    assert fs.errors_per_frame_hist().sum() == S // F
    if S // F >= 2:
        n = S // F
        assert fs.ber_stderr == pytest.approx(np.std(e[:n], ddof=1) / math.sqrt(n) / (F * 12), rel=1e-14)
        assert fs.ber_stderr == pytest.approx(want["ber_stderr"], rel=1e-14)
    else:
        assert fs.ber_stderr is None


def test_frame_stats_leave_the_partial_frame_out_of_the_rates():
    fs = frame_stats([0, 2, 0, 7], 10, 3)     # three full frames, the fourth holds symbol 9 alone
    assert (fs.n_full, fs.frame_errors, fs.fer) == (3, 1, 1 / 3)
    assert fs.errors_per_frame_hist().tolist() == [2, 0, 1]
    assert fs.bit_errors.tolist() == [0, 2, 0, 7]


def test_frame_stats_without_a_full_frame():
    fs = frame_stats([3], 4, 5)               # F > S
    assert fs.n_full == 0 and fs.frame_errors == 0 and fs.fer is None and fs.ber_stderr is None
    assert fs.errors_per_frame_hist().tolist() == [] and fs.bit_errors.tolist() == [3]


def test_ber_stderr_needs_every_bit_compared():
    assert frame_stats([1, 0, 2], 3, 1, n_valid=36).ber_stderr is not None
    assert frame_stats([1, 0, 2], 3, 1, n_valid=32).ber_stderr is None


def test_frame_count_and_its_cap():
    assert E.frame_count(10, 3) == 4 and E.frame_count(12, 4) == 3 and E.frame_count(0, 4) == 1
    assert E.frame_count(B.MAX_FRAMES, 1) == B.MAX_FRAMES == 1 << 24
    with pytest.raises(ValueError, match="16777216"):
        E.frame_count(B.MAX_FRAMES + 1, 1)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="frame_symbols"):
            E.frame_count(10, bad)


# ---------------------------------------------------------------- the engine over the oracle double
class FramesEngine(SweepEngine):
    """SweepEngine whose rx takes the frame record: it is filled from one-symbol oracle calls, as
    ofdm_rx_frames defines it.  Every tx / rx call is logged with its keyword names."""

    def __init__(self, *a):
        super().__init__(*a)
        self.log = []

    def tx(self, stream, bits_d, seed, sym0, n_sym, y, stats, **kw):
        self.log.append(("tx", sym0, n_sym, y is not None, tuple(sorted(kw))))
        super().tx(stream, bits_d, seed, sym0, n_sym, y, stats, **kw)

    def rx(self, stream, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits_d, sym0, n_sym, n_valid,
           counters, z_out=None, z_keep=0, **kw):
        self.log.append(("rx", sym0, n_sym, tuple(sorted(kw))))
        if not kw:
            return super().rx(stream, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits_d, sym0, n_sym,
                              n_valid, counters, z_out, z_keep)
        assert set(kw) == {"frames", "frame_symbols"}
        frames, F = kw["frames"], kw["frame_symbols"]
        assert frames.dtype == torch.int64 and frames.shape[1] == 2 and (sym0 + n_sym - 1) // F < frames.shape[0]
        for s in range(sym0, sym0 + n_sym):
            one = torch.zeros(2, dtype=torch.int64)
            super().rx(stream, y[s - sym0:s - sym0 + 1], nr, ni, seed, stats, total_samples, snr_db, noise_on, bits_d,
                       s, 1, n_valid, one)
            frames[s // F] += one
            counters += one


def make(S):
    h = channel(CASE["ch"])
    eng = FramesEngine(CASE["N"], CASE["M"], h, len(h) - 1, CASE["eq"])
    eng.seed_streams(SEED, S)
    return eng


def record(st):
    return (st.bit_errors, st.symbol_errors, st.frames.bit_errors.tolist(), st.frames.symbol_errors.tolist())


def test_engine_record_resident_and_batched():
    S, F = 22, 4      # 22 = 5 full frames + 2 symbols; batches of 3 split every frame
    eng = make(S)
    plain = eng.run(S, CASE["snr"], seed=SEED)
    assert plain.frames is None and plain.bit_errors > 0
    sym = eng.run(S, CASE["snr"], seed=SEED, frame_symbols=1)
    assert (sym.bit_errors, sym.symbol_errors) == (plain.bit_errors, plain.symbol_errors)
    per_be, per_se = sym.frames.bit_errors, sym.frames.symbol_errors
    assert len(per_be) == S and int(per_be.sum()) == plain.bit_errors and int(per_se.sum()) == plain.symbol_errors
    assert (per_be == 0).any() and (per_be > 0).any()
    res = eng.run(S, CASE["snr"], seed=SEED, frame_symbols=F)
    fs = res.frames
    assert (fs.frame_symbols, fs.n_symbols, fs.bits_per_symbol) == (F, S, eng.bps)
    assert np.array_equal(fs.bit_errors, FE.frame_sums(per_be, F)) and len(fs.bit_errors) == 6
    assert np.array_equal(fs.symbol_errors, FE.frame_sums(per_se, F))
    want = FE.stats(fs.bit_errors, S, F, eng.bps)
    assert (fs.n_full, fs.frame_errors, fs.fer) == (5, want["frame_errors"], want["fer"])
    assert fs.ber_stderr == pytest.approx(want["ber_stderr"], rel=1e-14)
    batched = eng.run(S, CASE["snr"], seed=SEED, frame_symbols=F, batch=3)
    assert record(batched) == record(res)
    assert record(eng.run(S, CASE["snr"], seed=SEED, frame_symbols=S + 1)) == (
        plain.bit_errors, plain.symbol_errors, [plain.bit_errors], [plain.symbol_errors])


def test_schedule_without_frames_is_unchanged():
    """Without frame_symbols every tx / rx call carries no new keyword; with it only rx does."""
    S = 7
    eng = make(S)
    eng.run(S, CASE["snr"], seed=SEED)
    eng.run(S, CASE["snr"], seed=SEED, batch=3)
    assert eng.log == [("tx", 0, 7, True, ()), ("rx", 0, 7, ()),
                       ("tx", 0, 7, False, ()), ("tx", 0, 3, True, ()), ("rx", 0, 3, ()), ("tx", 3, 3, True, ()),
                       ("rx", 3, 3, ()), ("tx", 6, 1, True, ()), ("rx", 6, 1, ())]
    eng.log.clear()
    eng.run(S, CASE["snr"], seed=SEED, frame_symbols=2, batch=4)
    kw = ("frame_symbols", "frames")
    assert eng.log == [("tx", 0, 7, False, ()), ("tx", 0, 4, True, ()), ("rx", 0, 4, kw), ("tx", 4, 3, True, ()),
                       ("rx", 4, 3, kw)]


def test_engine_refusals():
    eng = make(8)
    with pytest.raises(ValueError, match="profile"):
        eng.run(8, CASE["snr"], seed=SEED, frame_symbols=2, profile=True)
    with pytest.raises(ValueError, match="run_sweep"):
        eng.run_sweep(8, [10.0, 12.0], seed=SEED, frame_symbols=2)
    with pytest.raises(ValueError, match="run_pipelined"):
        eng.run_pipelined(8, CASE["snr"], [SEED], frame_symbols=2)
    with pytest.raises(ValueError, match="frame_symbols"):
        eng.run(8, CASE["snr"], seed=SEED, frame_symbols=0)
    with pytest.raises(ValueError, match="cap"):
        eng.run(B.MAX_FRAMES + 1, CASE["snr"], seed=SEED, frame_symbols=1)
    # fused=True has no record; None takes the two-kernel path (above: rx was called)
    eng._fused = True
    with pytest.raises(ValueError, match="frame record"):
        eng.run(8, CASE["snr"], seed=SEED, frame_symbols=2, fused=True)
    assert eng._route_fused(None, philox=True, tap=False, profile=True, whole=True) is False
    assert eng.log == []


def _worker(rank, world, port, batch, S, F, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = make(S)
    out[rank] = record(eng.run(S, CASE["snr"], seed=SEED, frame_symbols=F, group=dist.group.WORLD, batch=batch))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,batch", [(2, None), (3, None), (3, 4)])
def test_sharded_record_equals_the_single_process_record(world, batch):
    """25 symbols in frames of 4: the shard boundaries 12 (world 2) and 8 / 16 (world 3) fall on frame
    boundaries or inside frames (25 * 1 // 3 = 8, 25 * 2 // 3 = 16; world 2: 12) -- and with batches of 4
    from 8 and 16 the batches straddle too; F = 5 moves every boundary inside a frame."""
    S = 25
    for F in (4, 5):
        want = record(make(S).run(S, CASE["snr"], seed=SEED, frame_symbols=F))
        assert sum(want[2]) == want[0] > 0
        out = mp.Manager().dict()
        mp.spawn(_worker, args=(world, _free_port(), batch, S, F, out), nprocs=world, join=True)
        for r in range(world):
            assert out[r] == want, (world, F, r)


# ---------------------------------------------------------------- Simulation and the settings
def test_settings_key():
    base = dict(num_bands=64, signal_noise_ratios=[10.0], channel_model_path="", num_symbols=8)
    assert SimulationSettings(**base).frame_symbols is None
    s = SimulationSettings(**base, frame_symbols=8)
    assert s.frame_symbols == 8
    with pytest.raises(ValueError):
        SimulationSettings(**base, frame_symbols=0)
    sims = Simulation.create_from_simulation_settings(s)
    assert [x.frame_symbols for x in sims] == [8]
    assert Simulation.create_from_simulation_settings(SimulationSettings(**base))[0].frame_symbols is None


def test_simulation_run_sweep_refuses_frames():
    sims = [Simulation(num_symbols=64 * 4, snr_db=q, rng_mode="philox", seed=1, received_symbols_keep=0,
                       verbose=False, make_plot=False, frame_symbols=2) for q in (10.0, 12.0)]
    with pytest.raises(ValueError, match="frame_symbols"):
        Simulation.run_sweep(sims)


def test_simulation_refusals_come_before_the_run():
    from ofdm_based_systems.modulation.models import OFDMModulator

    class MyModulator(OFDMModulator):
        pass

    class Composed(Simulation):
        MODULATOR_SCHEME_MAPPERS = {k: MyModulator for k in Simulation.MODULATOR_SCHEME_MAPPERS}

    kw = dict(num_symbols=64 * 4, verbose=False, make_plot=False)
    with pytest.raises(ValueError, match="built-in"):
        Composed(frame_symbols=2, **kw).run()
    with pytest.raises(ValueError, match="subcarrier_profile"):
        Simulation(frame_symbols=2, subcarrier_profile=True, **kw).run()
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="frame_symbols"):
            Simulation(frame_symbols=bad, **kw).run()

"""The frame-error record of a one-pass SNR sweep (ofdm_rx_sweep_frames, LinkEngine.run_frame_sweep,
Simulation.run_frame_sweep) without a GPU: the entry point's declaration, export, binding and refusals;
the engine's schedule over the oracle's CPU test double (tests/test_frames_cpu.FramesEngine, whose
rx fills a frame record from one-symbol oracle calls) -- one transmit per batch, the rx_sweep calls with
their frame keywords, a batch boundary inside a frame, a list longer than one launch split into
launches with the record's slices, the buffer layout, FrameStats per point, gloo worlds of 2 and 3 --
and the refusals, with nothing launched.  Every comparison is of integers and exact.

On the commit before the feature every test here fails: there is no ofdm_rx_sweep_frames and no
run_frame_sweep."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from conftest import channel

from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.simulation.models import AdaptiveModulationMode, Simulation
from test_distributed_cpu import CASE, _free_port
from test_frames_cpu import FramesEngine

SEED = 21
SNRS = [8.0, 14.0, 11.0, 20.0]   # (at 20 dB the double has frames of 4 without errors, and with)
SWEEP_ARGS = 12  # ofdm_rx_sweep's


# ---------------------------------------------------------------- the ABI boundary
EXT_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                          "ofdm_hip_sweep_frames.h")


def test_entry_point_is_declared_exported_and_bound():
    """The entry point is declared in the ABI's extension header and bound from the table that mirrors it;
    ofdm_hip.h and the table that mirrors that header are what they were."""
    from test_abi import HEADER, declared_functions

    text = open(EXT_HEADER).read()
    assert '#include "ofdm_hip.h"' in text and 'extern "C"' in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(ofdm_[a-z_0-9]+)\s*\(", code))) == ["ofdm_rx_sweep_frames"] == sorted(
        B.EXTENSION_SIGNATURES)
    at = text.index("int ofdm_rx_sweep_frames(")
    decl = re.sub(r"\s+", " ", text[at:text.index(";", at)])
    assert "const double* snr_db, int32_t n_snr" in decl
    assert decl.endswith("uint64_t* counters, int64_t frame_len, int64_t n_frames, uint64_t* frames)")
    comment = text[text.rindex("/*", 0, at):at]
    assert "uint64[n_snr][n_frames][2]" in comment and "point-major" in comment and "never zeroed" in comment
    assert "floor(s / F)" in comment and "OFDM_MAX_SYMBOLS" in comment
    main = open(HEADER).read()
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", main).group(1)) == B.ABI_VERSION == 6
    assert "ofdm_hip_sweep_frames.h" in main                      # the main header points to it
    lib = B.load_library()
    assert hasattr(lib, "ofdm_rx_sweep_frames") and lib.ofdm_abi_version() == 6
    # ofdm_rx_sweep's arguments, then frame_len, n_frames and the record; bound with them by load_library
    assert len(B.SIGNATURES["ofdm_rx_sweep"][1]) == SWEEP_ARGS
    assert B.EXTENSION_SIGNATURES["ofdm_rx_sweep_frames"] == (ctypes.c_int, B.SIGNATURES["ofdm_rx_sweep"][1] + [
        ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p])
    assert lib.ofdm_rx_sweep_frames.argtypes == B.EXTENSION_SIGNATURES["ofdm_rx_sweep_frames"][1]
    # the main header's entry points and their table: as they were
    assert set(B.SIGNATURES) == set(declared_functions()) and not set(B.SIGNATURES) & set(B.EXTENSION_SIGNATURES)


def sweep_args(sym0=0, n_sym=0, n_snr=2, counters=True, snrs=None):
    cnt = (ctypes.c_uint64 * (2 * max(n_snr, 1)))()
    pts = (ctypes.c_double * max(n_snr, 1))(*(snrs or [10.0] * max(n_snr, 1)))
    args = [None, None, None, 0, None, 0, pts, n_snr, sym0, n_sym, 0,
            ctypes.cast(cnt, ctypes.c_void_p) if counters else None]
    assert len(args) == SWEEP_ARGS
    return args


@pytest.mark.parametrize("sym0,n_sym,frame_len,n_frames,record,reason", [
    (0, 8, 4, 2, False, "needs a frame record"),
    (0, 8, 0, 2, True, "frame_len 0"),
    (0, 8, -3, 2, True, "frame_len -3"),
    (0, 8, 4, 0, True, "n_frames 0"),
    (0, 9, 4, 2, True, "last symbol 8 lies in frame 2"),      # floor(8 / 4) = 2 >= 2
    (5, 4, 3, 2, True, "last symbol 8 lies in frame 2"),      # sym0 counts: floor(8 / 3) = 2
    (0, (1 << 31) + 1, 1 << 40, 1, True, "at most 2^31 symbols"),
    (0, 8, 4, 2, True, "needs a constellation"),              # the record fits: ofdm_rx_sweep's own refusal
    (0, 0, 4, 2, True, "needs a constellation"),
])
def test_refusals_name_the_function_without_a_device(sym0, n_sym, frame_len, n_frames, record, reason):
    """frames_ok's refusals by the same single check as ofdm_rx_frames', before the plan is looked at."""
    lib = B.load_library()
    rec = (ctypes.c_uint64 * (2 * 2 * max(n_frames, 1)))()
    rc = lib.ofdm_rx_sweep_frames(*sweep_args(sym0, n_sym), frame_len, n_frames,
                                  ctypes.cast(rec, ctypes.c_void_p) if record else None)
    msg = lib.ofdm_last_error().decode()
    assert rc == -1 and "ofdm_rx_sweep_frames" in msg and reason in msg, msg
    assert not any(rec)


def test_what_ofdm_rx_sweep_refuses_is_refused():
    lib = B.load_library()
    rec = (ctypes.c_uint64 * 16)()
    recp = ctypes.cast(rec, ctypes.c_void_p)
    for kw in (dict(sym0=-1, n_sym=4), dict(n_sym=-1), dict(counters=False)):
        args = sweep_args(**kw)
        assert lib.ofdm_rx_sweep_frames(*args, 4, 2, recp) == -1
        assert "ofdm_rx_sweep_frames" in lib.ofdm_last_error().decode()
        assert lib.ofdm_rx_sweep(*args) == -1


# ---------------------------------------------------------------- the engine over the oracle double
class FrameSweepEngine(FramesEngine):
    """FramesEngine whose rx_sweep takes the frame keywords: per point, FramesEngine.rx with the point's
    rows of the record -- ofdm_rx_sweep_frames as it is defined.  Every rx_sweep call is logged with its
    keyword names and the slice of the run's record it was handed."""

    def rx_sweep(self, stream, y, seed, stats, total_samples, snr_dbs, sym0, n_sym, n_valid, counters, **kw):
        assert 1 <= len(snr_dbs) <= B.MAX_SWEEP_POINTS and counters.shape == (len(snr_dbs), 2)
        self.launches.append((sym0, n_sym, len(snr_dbs)))
        self.log.append(("rx_sweep", sym0, n_sym, len(snr_dbs), tuple(sorted(kw))))
        if not kw:
            for k, snr in enumerate(snr_dbs):
                self.rx(stream, y, None, None, seed, stats, total_samples, snr, True, None, sym0, n_sym, n_valid,
                        counters[k])
            return
        assert set(kw) == {"frames", "frame_symbols"}
        frames, F = kw["frames"], kw["frame_symbols"]
        assert frames.dtype == torch.int64 and frames.dim() == 3 and frames.shape[0] == len(snr_dbs)
        assert frames.shape[2] == 2 and frames.is_contiguous() and (sym0 + n_sym - 1) // F < frames.shape[1]
        self.slices.append((frames.data_ptr(), tuple(frames.shape)))
        for k, snr in enumerate(snr_dbs):
            self.rx(stream, y, None, None, seed, stats, total_samples, snr, True, None, sym0, n_sym, n_valid,
                    counters[k], frames=frames[k], frame_symbols=F)

    def __init__(self, *a):
        super().__init__(*a)
        self.slices = []


def make(S):
    h = channel(CASE["ch"])
    eng = FrameSweepEngine(CASE["N"], CASE["M"], h, len(h) - 1, CASE["eq"])
    eng.seed_streams(SEED, S)
    return eng


def record(st):
    fr = st.frames
    return (st.bit_errors, st.symbol_errors, st.power_sum, st.x_power_sum, st.x_peak, st.num_ofdm_symbols, st.samples,
            fr.frame_symbols, fr.n_symbols, fr.bits_per_symbol, fr.n_valid_bits, fr.bit_errors.tolist(),
            fr.symbol_errors.tolist())


def calls(eng, kind):
    return [l for l in eng.log if l[0] == kind]


@pytest.mark.parametrize("batch", [None, 1, 7])
def test_frame_sweep_equals_the_single_point_runs_with_a_record(batch):
    S, F = 22, 4      # 22 = 5 full frames + 2 symbols; batches of 7 end inside frames 1, 3 and 5
    eng = make(S)
    want = [record(eng.run(S, snr, seed=SEED, frame_symbols=F)) for snr in SNRS]
    assert all(w[0] > 0 and sum(w[11]) == w[0] and sum(w[12]) == w[1] for w in want)
    assert len({tuple(w[11]) for w in want}) == len(SNRS)                # the points' records differ
    assert any(0 in w[11] and max(w[11]) > 0 for w in want)             # a frame without and one with errors
    eng.log.clear(), eng.launches.clear()
    got = eng.run_frame_sweep(S, SNRS, F, seed=SEED, batch=batch)
    assert [record(g) for g in got] == want
    assert all(isinstance(g.frames, E.FrameStats) and len(g.frames.bit_errors) == 6 and g.frames.n_full == 5 for g in got)
    # the schedule: one transmit per batch (behind the power pass when batched), then one rx_sweep over
    # all the points with the frame keywords; nothing else is called
    kw = ("frame_symbols", "frames")
    if batch is None:
        assert [l for l in eng.log if l[0] != "rx"] == [("tx", 0, S, True, ()), ("rx_sweep", 0, S, len(SNRS), kw)]
    else:
        want_log = [("tx", 0, S, False, ())]
        for b0 in range(0, S, batch):
            nb = min(batch, S - b0)
            want_log += [("tx", b0, nb, True, ()), ("rx_sweep", b0, nb, len(SNRS), kw)]
        assert [l for l in eng.log if l[0] != "rx"] == want_log
        assert batch == 1 or any(b0 % F for b0 in range(0, S, batch))    # a batch boundary inside a frame
    # the double's rx was reached through rx_sweep only, always with a record
    assert all(l[3] == kw for l in calls(eng, "rx"))


def test_sweep_without_frames_is_called_as_before():
    S = 6
    eng = make(S)
    plain = eng.run_sweep(S, SNRS, seed=SEED)
    assert [l for l in eng.log if l[0] != "rx"] == [("tx", 0, S, True, ()), ("rx_sweep", 0, S, len(SNRS), ())]
    assert all(p.frames is None for p in plain)
    got = eng.run_frame_sweep(S, SNRS, 4, seed=SEED)
    assert [(g.bit_errors, g.symbol_errors) for g in got] == [(p.bit_errors, p.symbol_errors) for p in plain]


def test_a_list_longer_than_the_cap_is_split_with_the_records_slices():
    S, F = 6, 4
    eng = make(S)
    K = B.MAX_SWEEP_POINTS + 3
    snrs = [SNRS[k % len(SNRS)] for k in range(K)]
    short = [record(s) for s in eng.run_frame_sweep(S, SNRS, F, seed=SEED)]
    eng.launches.clear(), eng.slices.clear()
    got = eng.run_frame_sweep(S, snrs, F, seed=SEED)
    assert [l[2] for l in eng.launches] == [B.MAX_SWEEP_POINTS, 3]
    assert [record(g) for g in got] == [short[k % len(SNRS)] for k in range(K)]
    # frames[k0:k1] of one point-major [K][2][2] record: the second launch's rows start 40 points in
    n_frames = 2
    (p0, s0), (p1, s1) = eng.slices
    assert s0 == (B.MAX_SWEEP_POINTS, n_frames, 2) and s1 == (3, n_frames, 2)
    assert p1 - p0 == B.MAX_SWEEP_POINTS * n_frames * 2 * 8


def test_the_record_sits_behind_the_counters_in_one_buffer():
    S, F, K = 10, 4, len(SNRS)
    eng = make(S)
    pend = eng.run_frame_sweep_async(S, SNRS, F, seed=SEED)
    n_frames = 3
    assert pend.counters.shape == (K, 2) and pend.frames.shape == (K, n_frames, 2) and pend.clip is None
    assert pend.frame_info == (F, eng.bps, S * eng.bps)
    base = pend.counters.untyped_storage().data_ptr()
    assert pend.frames.untyped_storage().data_ptr() == base          # one buffer: one all-reduce
    assert pend.counters.storage_offset() == 0 and pend.frames.storage_offset() == 2 * K
    assert pend.counters.untyped_storage().nbytes() == 8 * (2 * K + 2 * K * n_frames)
    assert pend.frames.sum(dim=1).tolist() == pend.counters.tolist()
    res = pend.result()
    assert [r.frames.bit_errors.tolist() for r in res] == pend.frames[:, :, 0].tolist()
    # a clipped engine: the clip record between the counters and the frame record
    eng.clip_a2, eng.clip_db = 1.0, 0.0
    eng.tx = lambda stream, bits_d, seed, sym0, n_sym, y, stats, clip_counters=None: FramesEngine.tx(
        eng, stream, bits_d, seed, sym0, n_sym, y, stats)
    pend = eng.run_frame_sweep_async(S, SNRS, F, seed=SEED)
    assert pend.clip.storage_offset() == 2 * K and pend.clip.shape == (2,)
    assert pend.frames.storage_offset() == 2 * K + 2 and pend.frames.shape == (K, n_frames, 2)
    assert [r.frames.bit_errors.tolist() for r in pend.result()] == [r.frames.bit_errors.tolist() for r in res]


def test_n_valid_bits_reaches_the_receiver_and_the_stats():
    S, F = 8, 3
    eng = make(S)
    short = S * eng.bps - 8
    got = eng.run_frame_sweep(S, SNRS[:2], F, seed=SEED, n_valid_bits=short)
    one = eng.run(S, SNRS[0], seed=SEED, frame_symbols=F, n_valid_bits=short)
    assert got[0].frames.n_valid_bits == one.frames.n_valid_bits == short
    assert got[0].frames.ber_stderr is None and one.frames.ber_stderr is None and got[0].frames.fer == one.frames.fer


def test_engine_refusals_launch_nothing():
    eng = make(8)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="frame_symbols"):
            eng.run_frame_sweep(8, SNRS, bad, seed=SEED)
    with pytest.raises(ValueError, match="cap"):
        eng.run_frame_sweep(B.MAX_FRAMES + 1, SNRS, 1, seed=SEED)             # one point's rows above the cap
    with pytest.raises(ValueError, match="cap"):
        eng.run_frame_sweep(B.MAX_FRAMES // 2, SNRS, 1, seed=SEED)            # 4 x 2^23 rows: the whole record
    with pytest.raises(ValueError, match="run_frame_sweep"):
        eng.run_frame_sweep(8, [], 2, seed=SEED)
    with pytest.raises(ValueError, match="finite"):
        eng.run_frame_sweep(8, [10.0, float("inf")], 2, seed=SEED)
    with pytest.raises(ValueError, match="finite"):
        eng.run_frame_sweep(8, [float("nan")], 2, seed=SEED)
    # caller streams and a tap are no arguments of a sweep
    for kw in ({"bits": np.zeros(8, np.uint8)}, {"normals": (None, None)}, {"keep_symbols": 1}, {"profile": True}):
        with pytest.raises(TypeError):
            eng.run_frame_sweep(8, SNRS, 2, seed=SEED, **kw)
    # run_sweep itself still refuses a frame length, naming both
    with pytest.raises(ValueError, match="run_sweep") as ei:
        eng.run_sweep(8, [10.0, 12.0], seed=SEED, frame_symbols=2)
    assert "frame_symbols" in str(ei.value) and "run_frame_sweep" in str(ei.value)
    assert eng.log == [] and eng.launches == []


def test_rx_sweep_checks_the_records_shape():
    """The production rx_sweep (not the double's) refuses a record that is not [K][n_frames][2] before the
    library is called."""
    eng = make(8)
    cnt = torch.zeros((2, 2), dtype=torch.int64)
    for rec in (torch.zeros((3, 2, 2), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int64),
                torch.zeros((2, 4, 2), dtype=torch.int64)[:, ::2]):
        with pytest.raises(ValueError, match="frame record"):
            E.LinkEngine.rx_sweep(eng, None, None, SEED, None, 0, [10.0, 12.0], 0, 8, 0, cnt, frames=rec, frame_symbols=4)


def _worker(rank, world, port, batch, S, F, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = make(S)
    out[rank] = [record(s) for s in eng.run_frame_sweep(S, SNRS, F, seed=SEED, group=dist.group.WORLD, batch=batch)]
    dist.destroy_process_group()


@pytest.mark.parametrize("world,batch", [(2, None), (3, None), (3, 4)])
def test_sharded_frame_sweep_equals_the_single_process_result(world, batch):
    """25 symbols in frames of 4 and 5: the shard boundaries 12 (world 2) and 8 / 16 (world 3) fall on
    frame boundaries (F = 4) and inside frames (F = 5; 12 at F = 5 and F = 4 with batches of 4 from 8)."""
    S = 25
    for F in (4, 5):
        want = [record(s) for s in make(S).run_frame_sweep(S, SNRS, F, seed=SEED)]
        assert all(sum(w[11]) == w[0] > 0 for w in want)
        out = mp.Manager().dict()
        mp.spawn(_worker, args=(world, _free_port(), batch, S, F, out), nprocs=world, join=True)
        for r in range(world):
            got = out[r]
            # counts, the exact power, the peak and the whole frame record: identical; sum |x|^2 adds in rank order
            assert [g[:3] + g[4:5] + g[5:] for g in got] == [w[:3] + w[4:5] + w[5:] for w in want], (world, F, r)
            assert all(abs(g[3] - w[3]) <= 1e-12 * w[3] for g, w in zip(got, want))


# ---------------------------------------------------------------- Simulation
def _sims(snrs=(10.0, 12.0), **kw):
    base = dict(num_symbols=64 * 4, rng_mode="philox", seed=1, received_symbols_keep=0, verbose=False,
                make_plot=False, frame_symbols=2)
    base.update(kw)
    return [Simulation(snr_db=q, **base) for q in snrs]


def test_simulation_run_sweep_still_refuses_frames():
    with pytest.raises(ValueError, match="frame_symbols") as ei:
        Simulation.run_sweep(_sims())
    assert "run_sweep" in str(ei.value) and "run_frame_sweep" in str(ei.value)


def test_simulation_run_frame_sweep_checks():
    assert Simulation.run_frame_sweep([]) == []
    with pytest.raises(ValueError, match="frame_symbols"):
        Simulation.run_frame_sweep(_sims(frame_symbols=None))
    with pytest.raises(ValueError, match="philox"):
        Simulation.run_frame_sweep(_sims(rng_mode="reference"))
    sims = _sims()
    sims[1].frame_symbols = 4
    with pytest.raises(ValueError, match=r"differ in more than snr_db \(frame_symbols\)"):
        Simulation.run_frame_sweep(sims)
    sims = _sims()
    sims[1].constellation_order = 4
    with pytest.raises(ValueError, match="constellation_order"):
        Simulation.run_frame_sweep(sims)
    with pytest.raises(ValueError, match="received_symbols_keep"):
        Simulation.run_frame_sweep(_sims(received_symbols_keep=8))
    with pytest.raises(ValueError, match="subcarrier_profile"):
        Simulation.run_frame_sweep(_sims(subcarrier_profile=True))
    with pytest.raises(ValueError, match="constellation_density"):
        Simulation.run_frame_sweep(_sims(constellation_density=8))
    with pytest.raises(ValueError, match="FIXED"):
        Simulation.run_frame_sweep(_sims(adaptive_modulation_mode=AdaptiveModulationMode.CAPACITY_BASED))
    for bad in (0, -1, 2.5):    # (_check_frames, before any engine exists)
        with pytest.raises(ValueError, match="frame_symbols"):
            Simulation.run_frame_sweep(_sims(frame_symbols=bad))

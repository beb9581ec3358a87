"""The frame-error record of the one-pass SNR sweep (ofdm_rx_sweep_frames, LinkEngine.run_frame_sweep,
Simulation.run_frame_sweep) on the GPU.  Every comparison is of integers and exact:

  1. against the receiver that exists without the record: ofdm_rx_sweep called once per symbol on the same
     y -- the record at F = 1 is that array, at F = 3 its reshape-sum, and its per-point sums are the
     counters; in both precisions, because it is the same kernel form.  The shapes are test_gpu_sweep's
     (two workgroups and a partial last one; symbols of 4 waves, 1 wave, 16 and 4 lanes, one lane), plus
     the two-wave generic form (N = 2048) and N = 2;
  2. complex128: every point's record equals LinkEngine.run(frame_symbols=F) at that point;
  3. the record does not depend on the order of the list, duplicates, the batching, how a long list is
     split into launches, or how [0, S) is split into calls -- into a record that is not zero;
  4. the inputs discriminate: with the oracle's own counts, a point has frames with and without errors
     and two points differ, so a kernel that wrote one point's counts everywhere, or everything into
     row 0, fails 1.-3.;
  5. the 64-bit halves of the frame index at sym0 = 2^32 - 3;
  6. two gloo ranks whose shard boundary splits a frame;
  7. Simulation.run_frame_sweep, and the ABI's refusals through the binding.

On the commit before the feature every test here fails: there is no ofdm_rx_sweep_frames and no
run_frame_sweep."""

import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
from conftest import ROOT

import frames_expect as FE
import philox_streams as P
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import new_stats
from test_gpu_multirank import _launch
from test_gpu_philox_parity import setup
from test_gpu_sweep import CASES as SWEEP_CASES
from test_gpu_sweep import _simulations

pytestmark = pytest.mark.gpu

SEED = 77
F32, F64 = B.OFDM_F32, B.OFDM_F64
# test_gpu_sweep's case table and SNR lists (every point gives more than 100 bit errors there), and two more:
# the two-wave generic form (adaptive N = 2048 has a throughput receiver, fixed 64-QAM there has none) and
# the smallest transform, one lane for eight symbols
CASES = dict(SWEEP_CASES)
CASES["n2048"] = (2048, 64, "Lin-Phoong_P1", "ZF", 35, [18, 24, 28], {})
CASES["n2"] = (2, 4, "flat_fading", "NONE", 4099, [2, 5, 8], {})
RUNS = [("b", F64), ("c", F64), ("c-zf", F64), ("e", F64), ("g1", F64), ("g1", F32), ("g2", F64), ("g3", F64),
        ("g3", F32), ("g4", F64), ("n2048", F64), ("n2", F64)]
RUNS_F64 = [r for r in RUNS if r[1] == F64]
INVARIANT = [("c", F64), ("c", F32), ("g1", F64)]
# 4.: points chosen with the CPU oracle (philox_streams.run_philox, F = 4): bit errors over the run, and
# frames without / with errors at the last point: b 9550, 167, 34 and 18 / 23; c 2647, 211, 58 and 12 / 29;
# g1 6992, 1849, 770 and 123 / 398
DISCRIMINATE = {"b": [20, 24, 25], "c": [24, 27, 28], "g1": [10, 14, 16]}
F_DISC = 4


def _rid(r):
    return f"{r[0]}-{'f32' if r[1] == F32 else 'f64'}"


@functools.lru_cache(maxsize=None)
def engine(cid, prec):
    N, M, ch, eq, S, snrs, var = CASES[cid]
    return setup(N, M, ch, eq, prec, var)  # (engine, CIR, cp, keyword arguments for run_philox)


class Stream:
    """Symbols [sym0, sym0 + S) of a case transmitted once and held on the device, and the receiver
    calls over them."""

    def __init__(self, cid, prec, sym0=0, S=None, seed=SEED, snrs=None):
        self.eng = engine(cid, prec)[0]
        self.S = CASES[cid][4] if S is None else S
        self.snrs = [float(q) for q in (CASES[cid][5] if snrs is None else snrs)]
        self.sym0, self.seed = sym0, seed
        eng = self.eng
        self.dev, self.st = eng.device(), eng.stream()
        self.samples = self.S * (eng.n_fft + eng.cp)
        self.n_valid = (sym0 + self.S) * eng.bps
        self.y = eng._y(self.S)
        self.stats = new_stats(self.dev)
        eng.tx(self.st, None, seed, sym0, self.S, self.y, self.stats)

    def sweep(self, lo, n, counters, **kw):
        """ofdm_rx_sweep (or, with the frame keywords, ofdm_rx_sweep_frames) over call-relative [lo, lo + n)."""
        self.eng.rx_sweep(self.st, self.y[lo:], self.seed, self.stats, self.samples, self.snrs, self.sym0 + lo, n,
                          self.n_valid, counters, **kw)

    @functools.cached_property
    def per_symbol(self):
        """int64 (K, S, 2): ofdm_rx_sweep -- the receiver without a record -- once per symbol, fresh [K][2]
        counters each.  Computed once and shared (read only)."""
        cnt = torch.zeros((self.S, len(self.snrs), 2), dtype=torch.int64, device=self.dev)
        for s in range(self.S):
            self.sweep(s, 1, cnt[s])
        per = np.ascontiguousarray(cnt.cpu().numpy().transpose(1, 0, 2))
        per.setflags(write=False)
        return per

    def frames(self, F, splits=None, fill=0):
        """(counters (K, 2), record (K, n_frames, 2)) of ofdm_rx_sweep_frames over the stream, one call or
        one per piece of ``splits``, into a record preset to ``fill``."""
        K = len(self.snrs)
        n_frames = (self.sym0 + self.S - 1) // F + 1
        rec = torch.full((K, n_frames, 2), fill, dtype=torch.int64, device=self.dev)
        cnt = torch.zeros((K, 2), dtype=torch.int64, device=self.dev)
        edges = [0] + list(splits or []) + [self.S]
        for lo, hi in zip(edges[:-1], edges[1:]):
            self.sweep(lo, hi - lo, cnt, frames=rec, frame_symbols=F)
        return cnt.cpu().numpy(), rec.cpu().numpy()


@functools.lru_cache(maxsize=None)
def stream(cid, prec):
    return Stream(cid, prec)


def sums(per, F, sym0=0):
    """(K, S, 2) per-symbol counts summed into frames of F global symbols: (K, n_frames, 2)."""
    return np.stack([np.stack([FE.frame_sums(p[:, j], F, sym0) for j in (0, 1)], axis=1) for p in per])


def fields(st):
    fr = st.frames
    return (st.bit_errors, st.symbol_errors, st.power_sum, st.x_power_sum, st.x_peak, fr.frame_symbols, fr.n_symbols,
            fr.bits_per_symbol, fr.n_valid_bits, fr.bit_errors.tolist(), fr.symbol_errors.tolist())


# ---------------------------------------------------------------- 1. against the receiver without the record
@pytest.mark.parametrize("cid,prec", RUNS, ids=[_rid(r) for r in RUNS])
def test_record_equals_the_one_symbol_sweep_calls(gpu, cid, prec):
    ys = stream(cid, prec)
    per, S, K = ys.per_symbol, ys.S, len(ys.snrs)
    whole = torch.zeros((K, 2), dtype=torch.int64, device=ys.dev)
    ys.sweep(0, S, whole)
    whole = whole.cpu().numpy()
    print(_rid((cid, prec)), "bit errors per point:", whole[:, 0].tolist(), "symbols without errors per point:",
          (per[:, :, 0] == 0).sum(axis=1).tolist())
    assert np.array_equal(per.sum(axis=1), whole) and (whole[:, 0] > 0).all()
    assert len({tuple(p[:, 0].tolist()) for p in per}) == K          # no two points alike
    cnt, rec = ys.frames(1)
    assert rec.shape == (K, S, 2)
    if not np.array_equal(rec, per):
        print("F = 1: first difference at (point, symbol, field)", np.argwhere(rec != per)[:4].tolist())
    assert np.array_equal(rec, per)
    assert np.array_equal(cnt, whole) and np.array_equal(rec.sum(axis=1), cnt)
    cnt, rec = ys.frames(3)
    assert rec.shape == (K, -(-S // 3), 2) and np.array_equal(rec, sums(per, 3))
    assert np.array_equal(cnt, whole) and np.array_equal(rec.sum(axis=1), cnt)


# ---------------------------------------------------------------- 2. the engine against the single-point runs
@pytest.mark.parametrize("cid,prec", RUNS_F64, ids=[_rid(r) for r in RUNS_F64])
def test_complex128_points_equal_the_single_point_runs(gpu, cid, prec):
    S, snrs = CASES[cid][4], CASES[cid][5]
    eng = engine(cid, prec)[0]
    for F in (4, 7):
        events = []
        got = eng.run_frame_sweep(S, snrs, F, seed=SEED, events=events)
        assert [e[0] for e in events] == ["ofdm_tx", "ofdm_rx_sweep_frames"] and len(got) == len(snrs)
        for snr, g in zip(snrs, got):
            one = eng.run(S, float(snr), seed=SEED, frame_symbols=F, fused=False)
            assert fields(g) == fields(one), (cid, snr, F)
            assert len(g.frames.bit_errors) == -(-S // F) and int(g.frames.bit_errors.sum()) == g.bit_errors > 0
            assert (g.frames.fer, g.frames.ber_stderr) == (one.frames.fer, one.frames.ber_stderr)
    # the sweep without the record gives the same counters
    plain = eng.run_sweep(S, snrs, seed=SEED)
    assert [(p.bit_errors, p.symbol_errors) for p in plain] == [(g.bit_errors, g.symbol_errors) for g in got]


# ---------------------------------------------------------------- 3. invariance
@pytest.mark.parametrize("cid,prec", INVARIANT, ids=[_rid(r) for r in INVARIANT])
def test_record_does_not_depend_on_order_batching_or_splitting(gpu, cid, prec):
    ys = stream(cid, prec)
    S, snrs, eng, F = ys.S, ys.snrs, ys.eng, 4
    want = sums(ys.per_symbol, F)

    def rec(stats):
        return np.stack([np.stack([s.frames.bit_errors, s.frames.symbol_errors], axis=1) for s in stats])

    base = eng.run_frame_sweep(S, snrs, F, seed=SEED)
    assert np.array_equal(rec(base), want)
    assert np.array_equal(rec(eng.run_frame_sweep(S, snrs[::-1], F, seed=SEED)), want[::-1])
    assert np.array_equal(rec(eng.run_frame_sweep(S, [snrs[1], snrs[0], snrs[1]], F, seed=SEED)), want[[1, 0, 1]])
    one = eng.run_frame_sweep(S, [snrs[2]], F, seed=SEED)
    assert np.array_equal(rec(one), want[2:3])
    if prec == F64:  # K = 1 equals run (complex64: another kernel's float32 rounding)
        assert fields(one[0]) == fields(eng.run(S, snrs[2], seed=SEED, frame_symbols=F, fused=False))
    for batch in (1, S // 3 + 5):  # (the second does not divide S, and is no multiple of 4)
        assert batch == 1 or (S % batch and batch % F)
        got = eng.run_frame_sweep(S, snrs, F, seed=SEED, batch=batch)
        assert [fields(g) for g in got] == [fields(b) for b in base], batch
    # a list longer than one launch takes: split into launches over the same y, each with its rows
    K = B.MAX_SWEEP_POINTS + 3
    order = [k % len(snrs) for k in range(K)]
    long = eng.run_frame_sweep(S, [snrs[k] for k in order], F, seed=SEED)
    assert np.array_equal(rec(long), want[order])
    # direct calls that split [0, S) inside frames, into a record that is not zero
    cnt, whole = ys.frames(F)
    assert np.array_equal(whole, want)
    for splits in ([S // 2 + 1], [1, 6, S - 1]):
        assert all(s % F for s in splits)
        cnt2, rec2 = ys.frames(F, splits=splits, fill=1000)
        assert np.array_equal(cnt2, cnt) and np.array_equal(rec2, whole + 1000), splits


# ---------------------------------------------------------------- 4. the record must discriminate
@pytest.mark.parametrize("cid", sorted(DISCRIMINATE))
def test_the_chosen_points_discriminate(gpu, cid):
    N, M, ch, eq, S, _, var = CASES[cid]
    eng, h, cp, var = engine(cid, F64)
    snrs, F = DISCRIMINATE[cid], F_DISC
    b = int(np.log2(M))
    bk = np.full(N, b, np.int64)
    # the oracle alone: frames without and with errors at a point, and two points that differ
    ref = []
    for snr in snrs:
        r = P.run_philox(SEED, S, N, M, h, cp, eq, float(snr), **var)
        be, _ = FE.per_symbol_from_z(r.z, r.idx, bk, S * N * b)
        ref.append(FE.frame_sums(be, F))
    print(cid, "oracle: frames without / with errors per point:", [(int((f == 0).sum()), int((f > 0).sum())) for f in ref])
    assert any((f == 0).sum() >= 10 and (f > 0).sum() >= 10 for f in ref)
    assert not np.array_equal(ref[0], ref[1]) and ref[0].sum() > 4 * ref[-1].sum() > 0
    # an error outside frame 0 at every point, and a frame that has errors at one point and none at another
    assert all(f[1:].sum() > 0 for f in ref) and ((ref[0] > 0) & (ref[-1] == 0)).any()
    # the device: the same properties, and the record itself against the one-symbol calls
    ys = Stream(cid, F64, snrs=snrs)
    got = eng.run_frame_sweep(S, snrs, F, seed=SEED)
    rec = np.stack([np.stack([g.frames.bit_errors, g.frames.symbol_errors], axis=1) for g in got])
    assert np.array_equal(rec, sums(ys.per_symbol, F))
    dev = [r[:, 0] for r in rec]
    print(cid, "device: frames without / with errors per point:", [(int((f == 0).sum()), int((f > 0).sum())) for f in dev])
    assert any((f == 0).sum() >= 10 and (f > 0).sum() >= 10 for f in dev)
    assert not np.array_equal(dev[0], dev[1]) and ((dev[0] > 0) & (dev[-1] == 0)).any()


# ---------------------------------------------------------------- 5. the 64-bit halves of the frame index
# (six symbols: points low enough that each half of them has errors at every point; g1's own list ends at 14 dB,
# where six symbols of 64 QPSK subcarriers have one error)
ACROSS = {"c": None, "g1": [2, 4, 6]}


@pytest.mark.parametrize("cid", sorted(ACROSS))
def test_frame_index_across_2_32(gpu, cid):
    sym0, S, F = (1 << 32) - 3, 6, 1 << 31
    ys = Stream(cid, F64, sym0=sym0, S=S, seed=0x9E3779B97F4A7C15, snrs=ACROSS[cid])
    per = ys.per_symbol
    assert (per[:, :, 0].sum(axis=1) > 0).all()
    cnt, rec = ys.frames(F)
    # symbols 2^32 - 3 .. 2^32 - 1 lie in frame 1, 2^32 .. 2^32 + 2 in frame 2
    want = np.zeros((len(ys.snrs), 3, 2), np.int64)
    want[:, 1] = per[:, :3].sum(axis=1)
    want[:, 2] = per[:, 3:].sum(axis=1)
    assert rec.shape == want.shape and np.array_equal(rec, want) and np.array_equal(rec, sums(per, F, sym0))
    assert np.array_equal(cnt, per.sum(axis=1)) and (want[:, 1, 0] > 0).all() and (want[:, 2, 0] > 0).all()
    cnt2, rec2 = ys.frames(F, splits=[2, 4])   # (a call that starts at 2^32 + 1: ft.base = 2, ft.first = 2^31 - 1)
    assert np.array_equal(cnt2, cnt) and np.array_equal(rec2, rec)


def test_the_last_supported_symbol(gpu):
    """sym0 = OFDM_MAX_SYMBOLS - 1, one symbol: the record's row 0 of each point is the one-symbol
    ofdm_rx_sweep call's pair, on the throughput form and the generic one."""
    for cid in ("b", "g1"):
        # (0 and 6 dB: the oracle counts 2250 and 1543 bit errors in that symbol of b, 26 and 13 in g1's)
        ys = Stream(cid, F64, sym0=(1 << 46) - 1, S=1, seed=0x9E3779B97F4A7C15, snrs=[0, 6])
        per = ys.per_symbol
        cnt, rec = ys.frames(1 << 62)
        assert rec.shape == (2, 1, 2) and np.array_equal(rec[:, 0], per[:, 0]) and np.array_equal(cnt, per[:, 0])
        assert (per[:, 0, 0] > 0).all() and per[0, 0, 0] != per[1, 0, 0], per.tolist()


# ---------------------------------------------------------------- 6. two gloo ranks on device 0
def test_two_ranks_hold_the_one_rank_record(gpu, tmp_path):
    out = tmp_path / "frame_sweep"
    N, M, ch, eq, S, snrs, _ = CASES["g3"]
    F = 4
    assert (S // 2) % F   # the shard boundary 273 splits frame 68
    r = _launch([os.path.join(ROOT, "tests", "frame_sweep_worker.py"), str(out),
                 json.dumps([N, M, ch, eq, S, snrs, SEED, F])], timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    one = [[s.bit_errors, s.symbol_errors, s.power_sum.hex(), s.x_peak, s.frames.bit_errors.tolist(),
            s.frames.symbol_errors.tolist()] for s in engine("g3", F64)[0].run_frame_sweep(S, snrs, F, seed=SEED)]
    assert all(sum(p[4]) == p[0] > 0 for p in one)
    for rank in (0, 1):
        got = json.loads((tmp_path / f"frame_sweep.{rank}.json").read_text())
        assert got["world"] == 2 and got["shard"] == [[0, S // 2], [S // 2, S]][rank]
        assert got["whole"] == one and got["batched"] == one, rank


# ---------------------------------------------------------------- 7. Simulation, and the ABI's refusals
def test_simulation_run_frame_sweep_gives_run_s_result_dicts(gpu):
    Simulation, sims = _simulations([8.0, 12.0, 16.0], frame_symbols=8)
    got = Simulation.run_frame_sweep(sims)
    want = [s.run() for s in sims]
    assert len(got) == 3
    keys = {"frame_symbols", "num_frames", "frame_errors", "frame_error_rate", "ber_std_error", "bit_errors_per_frame"}
    for g, w in zip(got, want):
        assert set(g) == set(w) and keys <= set(g)
        assert w["bit_errors"] > 100 and sum(w["bit_errors_per_frame"]) == w["bit_errors"]
        assert (w["frame_symbols"], w["num_frames"]) == (8, 25) and len(w["bit_errors_per_frame"]) == 25
        for key in w:
            if key in ("transmission_time_ms", "constellation_plot"):
                continue
            if isinstance(w[key], np.ndarray):
                assert np.array_equal(g[key], w[key]), key
            else:
                assert g[key] == w[key], key
        assert g["received_symbols"].size == 0 and g["constellation_plot"] is None
    assert got[0]["bit_errors_per_frame"] != got[2]["bit_errors_per_frame"]
    with pytest.raises(ValueError, match="frame_symbols"):
        Simulation.run_sweep(sims)
    with pytest.raises(ValueError, match="frame_symbols"):
        Simulation.run_frame_sweep(_simulations([8.0, 12.0])[1])


def test_abi_refusals_launch_nothing(gpu):
    ys = stream("g1", F64)
    eng, S, lib = ys.eng, ys.S, B.lib()
    K, F = len(ys.snrs), 4
    n_frames = -(-S // F)
    cnt = torch.zeros((B.MAX_SWEEP_POINTS + 1, 2), dtype=torch.int64, device=ys.dev)
    rec = torch.zeros((B.MAX_SWEEP_POINTS + 1, n_frames, 2), dtype=torch.int64, device=ys.dev)

    def call(snrs, frame_len, rows, record, n_sym=S):
        pts = (ctypes.c_double * len(snrs))(*snrs)
        return lib.ofdm_rx_sweep_frames(eng.plan.handle, ys.st, B.ptr(ys.y), SEED, B.ptr(ys.stats), ys.samples, pts,
                                        len(snrs), 0, n_sym, ys.n_valid, B.ptr(cnt), frame_len, rows, record)

    for args, reason in (((ys.snrs, F, n_frames, None), "needs a frame record"),
                         ((ys.snrs, 0, n_frames, B.ptr(rec)), "frame_len 0"),
                         ((ys.snrs, F, n_frames - 1, B.ptr(rec)), f"lies in frame {n_frames - 1}"),
                         (([10.0] * (B.MAX_SWEEP_POINTS + 1), F, n_frames, B.ptr(rec)), "SNR points"),
                         (([10.0, float("nan")], F, n_frames, B.ptr(rec)), "not finite")):
        assert call(*args) == -1   # OFDM_E_INVALID
        msg = lib.ofdm_last_error().decode()
        assert "ofdm_rx_sweep_frames" in msg and reason in msg, msg
    torch.cuda.synchronize()
    assert int(cnt.sum()) == 0 and int(rec.sum()) == 0    # refused before any launch
    assert call(ys.snrs, F, n_frames, B.ptr(rec), n_sym=0) == 0   # n_sym = 0: an empty call
    torch.cuda.synchronize()
    assert int(cnt.sum()) == 0 and int(rec.sum()) == 0
    # the engine's rx_sweep raises them as ValueError, and a plan above 256 points is ofdm_rx_sweep's refusal
    with pytest.raises(ValueError, match="frame_len 0"):
        ys.sweep(0, S, cnt[:K], frames=rec[:K], frame_symbols=0)
    # the symbol range (the record itself fits: frames of 2^62 symbols), with a plan: ofdm_rx_sweep's refusal,
    # for a call that ends beyond OFDM_MAX_SYMBOLS and for calls that start there or far beyond
    top = 1 << 46
    for sym0, n in ((top - 2, 3), (top, 1), (1 << 62, 1), ((1 << 63) - 1, 1)):
        with pytest.raises(ValueError, match="OFDM_MAX_SYMBOLS"):
            eng.rx_sweep(ys.st, ys.y, SEED, ys.stats, ys.samples, ys.snrs, sym0, n, ys.n_valid, cnt[:K],
                         frames=rec[:K], frame_symbols=1 << 62)
    torch.cuda.synchronize()
    assert int(cnt.sum()) == 0 and int(rec.sum()) == 0
    wide = setup(64, 1024, "flat_fading", "NONE", F64)[0]
    with pytest.raises(ValueError, match="8 bits"):
        wide.run_frame_sweep(64, [30.0, 35.0], 4, seed=SEED)


def test_a_clipped_engine_sweeps_as_it_runs(gpu):
    """An engine with a clip level: the clip record sits between the counters and the frame record."""
    from conftest import channel

    import ofdm_oracle as O
    from ofdm_based_systems.engine import LinkEngine

    N, M, ch, eq, S, snrs, _ = CASES["g3"]
    h = channel(ch)
    eng = LinkEngine(N, len(h) - 1, h, B.EQ_MMSE, [O.qam_lut(M)], None, F64, clip_db=4.0)
    got = eng.run_frame_sweep(S, snrs, 7, seed=SEED, batch=S // 3 + 5)
    for snr, g in zip(snrs, got):
        one = eng.run(S, float(snr), seed=SEED, frame_symbols=7)
        assert fields(g) == fields(one) and g.clipped_samples == one.clipped_samples > 0
        assert (g.clip_db, g.clip_samples) == (one.clip_db, one.clip_samples)

"""The per-frame error record of the fused receiver (ofdm_rx_frames, LinkEngine.run(frame_symbols=F),
Simulation(frame_symbols=F)) on the GPU.  Every comparison is of integers and exact:

  1. the stage fixtures: the record at F = 1 against the counts derived from the reference's own
     tx_bytes / rx_bytes (tests/frames_expect.py), any batching, and F = 3 as the reshape-sum;
  2. the throughput receivers of the bench shapes against the receiver that exists without the record:
     ofdm_rx called once per symbol on the same y;
  3. the reduction geometry of the generic kernel, N = 2 .. 4096 in both precisions: symbols of 1, 2,
     4, 32 and 64 lanes and of 2 and 4 waves, against the tapped symbols through the oracle's demapper
     (N <= 64) or one-symbol ofdm_rx calls (N >= 512); SC-OFDM with zero padding, 8-PSK, a partial
     n_valid_bits on an adaptive plan (the wide slicer: the 1024-QAM stage fixture of 1.);
  4. accumulation over calls that split a frame, into a record that is not zero;
  5. two gloo ranks whose shard boundary splits a frame;
  6. Simulation(frame_symbols=8) and the refusals.

The complex64 comparisons against tapped symbols decide the float32 symbols the kernel decided, in
double: they can differ only for a symbol within float32 rounding of a decision boundary, which none
of the few thousand symbols of these runs is; the comparison is exact and prints the difference first.

On the commit before the record every test here fails: there is no ``frame_symbols`` argument and no
ofdm_rx_frames."""

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT, channel, load_stages, stage_arrays

import frames_expect as FE
import ofdm_oracle as O
import philox_streams as P
import profile_expect as PE
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.constellation.adaptive import AdaptiveConstellationMapper
from ofdm_based_systems.constellation.models import QAMConstellationMapper
from ofdm_based_systems.engine import LinkEngine
from test_gpu_profile import EQ, golden_case, seeded_simulation, throughput_engine

pytestmark = pytest.mark.gpu

SEED = PE.SEED


def pair(fr):
    return fr.bit_errors.tolist(), fr.symbol_errors.tolist()


def assert_record(res, be, se, F, S, what=""):
    """res.frames is the frame sums of the per-symbol counts (be, se), and sums to the counters."""
    fr = res.frames
    got, want = pair(fr), (FE.frame_sums(be, F).tolist(), FE.frame_sums(se, F).tolist())
    if got != want:
        print(what, "device", got, "expected", want)
    assert got == want, what
    assert (fr.frame_symbols, fr.n_symbols, len(fr.bit_errors)) == (F, S, -(-S // F))
    assert (int(fr.bit_errors.sum()), int(fr.symbol_errors.sum())) == (res.bit_errors, res.symbol_errors), what


# ---------------------------------------------------------------- the receiver, called directly
class Stream:
    """A transmitted throughput-mode stream held on the device: y, its statistics, and what the
    receiver calls of a run over it are given."""

    def __init__(self, eng, S, snr, seed=SEED, n_valid=None):
        self.eng, self.S, self.snr, self.seed = eng, S, snr, seed
        self.dev, self.stream = eng.device(), eng.stream()
        self.samples = S * (eng.n_fft + eng.cp)
        self.n_valid = eng.valid_bits(S) if n_valid is None else n_valid
        self.y = eng._y(S)
        self.stats = E.new_stats(self.dev)
        eng.tx(self.stream, None, seed, 0, S, self.y, self.stats)

    def rx(self, sym0, n, counters, **kw):
        self.eng.rx(self.stream, self.y[sym0:], None, None, self.seed, self.stats, self.samples, self.snr, True, None,
                    sym0, n, self.n_valid, counters, **kw)

    def per_symbol(self, generic=False):
        """int64 (S, 2): ofdm_rx -- the receiver without a record -- once per symbol, fresh counters each.
        generic: with a one-symbol tap, which sends every plan to the generic kernel (in complex64 the
        throughput receivers round differently from it; the record's generic form must equal the
        generic receiver exactly)."""
        cnt = torch.zeros((self.S, 2), dtype=torch.int64, device=self.dev)
        z = torch.empty((1, self.eng.n_fft), dtype=self.eng.cdtype, device=self.dev) if generic else None
        for s in range(self.S):
            self.rx(s, 1, cnt[s], **({"z_out": z, "z_keep": 1} if generic else {}))
        return cnt.cpu().numpy()

    def plain(self):
        cnt = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self.rx(0, self.S, cnt)
        return cnt.cpu().numpy().tolist()

    def frames(self, F, splits=None, fill=0):
        """(counters, record int64 (n_frames, 2)) of ofdm_rx_frames over [0, S), one call or one per
        piece of ``splits``, into a record preset to ``fill``."""
        rec = torch.full((-(-self.S // F), 2), fill, dtype=torch.int64, device=self.dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=self.dev)
        edges = [0] + list(splits or []) + [self.S]
        for lo, hi in zip(edges[:-1], edges[1:]):
            self.rx(lo, hi - lo, cnt, frames=rec, frame_symbols=F)
        return cnt.cpu().numpy().tolist(), rec.cpu().numpy()


def sums(per, F):
    return np.stack([FE.frame_sums(per[:, 0], F), FE.frame_sums(per[:, 1], F)], axis=1)


# ---------------------------------------------------------------- 1. reference-pinned
def stage_run(st, a, F, precision=B.OFDM_F64, **kw):
    eng = LinkEngine(st["N"], st["cp"], a["h_raw"], EQ[st["eq"]], [O.qam_lut(st["M"])], precision=precision)
    return eng.run(st["S"], st["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]),
                   frame_symbols=F, **kw)


@pytest.mark.parametrize("st", FE.all_stages(), ids=lambda s: s["name"])
def test_stage_fixtures_against_the_references_bytes(gpu, st):
    a = stage_arrays(st["name"])
    N, S, b = st["N"], st["S"], int(np.log2(st["M"]))
    be, se = FE.per_symbol_from_bytes(a["tx_bytes"], a["rx_bytes"], np.full(N, b, np.int64), S, S * N * b)
    one = stage_run(st, a, 1)
    print(st["name"], "per symbol:", pair(one.frames))
    assert (one.bit_errors, one.symbol_errors) == (st["bit_errors"], st["symbol_errors"])
    assert_record(one, be, se, 1, S, "F = 1")
    assert one.frames.bits_per_symbol == N * b
    for batch in (1, 3):
        assert_record(stage_run(st, a, 1, batch=batch), be, se, 1, S, f"F = 1, batch {batch}")
    three = stage_run(st, a, 3)
    assert_record(three, be, se, 3, S, "F = 3")
    pad = np.zeros(3 * (-(-S // 3)), np.int64)
    pad[:S] = one.frames.bit_errors
    assert three.frames.bit_errors.tolist() == pad.reshape(-1, 3).sum(axis=1).tolist()
    for batch in (1, 3):
        assert pair(stage_run(st, a, 3, batch=batch).frames) == pair(three.frames)


def test_stage_fixture_complex64_against_its_tapped_symbols(gpu):
    st = next(s for s in load_stages() if s["name"] == "n64_m16_severe_cp_mmse")
    a = stage_arrays(st["name"])
    N, S, b = st["N"], st["S"], 4
    res = stage_run(st, a, 1, precision=B.OFDM_F32, keep_symbols=S)
    bk = np.full(N, b, np.int64)
    Z = res.received.reshape(S, N).astype(np.complex128)
    be, se = FE.per_symbol_from_z(Z, PE.tx_indices(a["tx_bytes"], bk, S), bk, S * N * b)
    print("complex64 per symbol:", pair(res.frames), "from its tapped symbols:", be.tolist(), se.tolist())
    assert_record(res, be, se, 1, S, "complex64")
    assert res.bit_errors > 0


# ---------------------------------------------------------------- 2. against the receiver without a record
@pytest.mark.parametrize("case", PE.THROUGHPUT_CASES, ids=lambda c: c["id"])
def test_throughput_receivers_against_one_symbol_calls(gpu, case):
    eng, bk = throughput_engine(case)
    S, snr = case["S"], case["snr"]
    ys = Stream(eng, S, snr)
    per = ys.per_symbol()
    print(case["id"], "per symbol (ofdm_rx):", per[:, 0].tolist())
    assert per.sum(axis=0).tolist() == [case["bit_errors"], case["symbol_errors"]] == ys.plain()
    if case is PE.THROUGHPUT_CASES[0]:
        # the frame error rate at F = 1 is neither 0 nor 1
        assert 4 * int((per[:, 0] == 0).sum()) >= S and 4 * int((per[:, 0] > 0).sum()) >= S
    cnt, rec = ys.frames(1)
    assert cnt == ys.plain() and np.array_equal(rec, per)
    for F in (4, 7, S, S + 1):
        cnt, rec = ys.frames(F)
        assert cnt == ys.plain() and np.array_equal(rec, sums(per, F)), F
    # the engine: the throughput form, any batching, and the generic form (a received-symbol tap)
    one = eng.run(S, snr, seed=SEED, frame_symbols=1)
    assert_record(one, per[:, 0], per[:, 1], 1, S, "engine")
    assert (one.bit_errors, one.symbol_errors) == (case["bit_errors"], case["symbol_errors"])
    assert pair(eng.run(S, snr, seed=SEED, frame_symbols=1, batch=50).frames) == pair(one.frames)
    assert_record(eng.run(S, snr, seed=SEED, frame_symbols=7, batch=50), per[:, 0], per[:, 1], 7, S, "batch 50, F = 7")
    tap = eng.run(S, snr, seed=SEED, frame_symbols=1, keep_symbols=S)
    assert pair(tap.frames) == pair(one.frames)
    want = FE.stats(per[:, 0], S, 1, eng.bps, whole=eng.valid_bits(S) == S * eng.bps)
    assert (one.frames.n_full, one.frames.frame_errors, one.frames.fer) == (S, want["frame_errors"], want["fer"])
    assert one.frames.ber_stderr == (None if want["ber_stderr"] is None else pytest.approx(want["ber_stderr"], rel=1e-13))


# ---------------------------------------------------------------- 3. the reduction geometry
# N: (symbols per 256-thread workgroup of the generic kernel + 3, capped at 300; SNR at which the oracle
# counts between S / 10 and 4 S bit errors over the S symbols)
GEOMETRY = {2: (259, 8.0), 8: (259, 14.0), 32: (131, 18.0), 64: (67, 18.0), 512: (11, 20.0), 1024: (7, 20.0),
            2048: (5, 20.0), 4096: (4, 22.0)}


def geometry_engine(N, precision, **kw):
    h = channel("flat_fading" if N <= 8 else "severe_multipath")
    return LinkEngine(N, len(h) - 1, h, B.EQ_MMSE, [O.qam_lut(16)], precision=precision, **kw)


def check_against_tapped(eng, S, snr, bk, scheme="QAM", what=""):
    res = eng.run(S, snr, seed=SEED, frame_symbols=1, keep_symbols=S)
    N = eng.n_fft
    Z = res.received.reshape(S, N).astype(np.complex128)
    uniform = len(set(bk.tolist())) == 1
    idx = P.tx_indices(P.lane_generators(SEED, np.arange(S), N), S, N, int(bk[0]) if uniform else bk)
    be, se = FE.per_symbol_from_z(Z, idx, bk, eng.valid_bits(S), scheme)
    print(what, "per symbol:", res.frames.bit_errors.tolist())
    assert_record(res, be, se, 1, S, what)
    return res


def check_against_calls(eng, S, snr, what="", n_valid=None, generic=False):
    ys = Stream(eng, S, snr, n_valid=n_valid)
    per = ys.per_symbol(generic)
    print(what, "per symbol (ofdm_rx):", per[:, 0].tolist())
    for F in (1, 3):
        cnt, rec = ys.frames(F)
        assert cnt == per.sum(axis=0).tolist() and np.array_equal(rec, sums(per, F)), (what, F)
        assert generic or cnt == ys.plain()
    return per


@pytest.mark.parametrize("precision", [B.OFDM_F64, B.OFDM_F32], ids=["complex128", "complex64"])
@pytest.mark.parametrize("N", sorted(GEOMETRY))
def test_reduction_geometry_of_the_generic_kernel(gpu, N, precision):
    S, snr = GEOMETRY[N]
    assert S == min(256 // max(N // 16, 1) + 3, 300)
    eng = geometry_engine(N, precision)
    what = f"N = {N}"
    if N <= 64:
        res = check_against_tapped(eng, S, snr, np.full(N, 4, np.int64), what=what)
        be = res.frames.bit_errors
        assert (be == 0).any() and (be > 0).any()
        # and without the tap, in frames that straddle the workgroups
        assert_record(eng.run(S, snr, seed=SEED, frame_symbols=5), be, res.frames.symbol_errors, 5, S, what)
    else:
        per = check_against_calls(eng, S, snr, what=what, generic=True)
        assert per[:, 0].sum() > 0


def test_single_carrier_with_zero_padding(gpu):
    h = channel("Lin-Phoong_P1")
    eng = LinkEngine(64, len(h) - 1, h, B.EQ_MMSE, [O.qam_lut(16)], prefix=B.PREFIX_ZERO, modulator=B.MOD_SC)
    # (18 dB: the oracle counts 63 bit errors over these 67 symbols)
    per = check_against_calls(eng, 67, 18.0, what="SC-OFDM, zero padding")
    assert (per[:, 0] == 0).any() and (per[:, 0] > 0).any()


def test_8psk(gpu):
    h = channel("severe_multipath")
    eng = LinkEngine(64, len(h) - 1, h, B.EQ_MMSE, [O.psk_lut(8)])
    per = check_against_calls(eng, 67, 16.0, what="8-PSK")
    assert per[:, 0].sum() > 0
    res = check_against_tapped(eng, 67, 16.0, np.full(64, 3, np.int64), scheme="PSK", what="8-PSK, tapped")
    assert res.frames.bit_errors.tolist() == per[:, 0].tolist()


def test_adaptive_plan_with_a_partial_n_valid_bits(gpu):
    N, snr, S = 64, 15.0, 67
    h = channel("Lin-Phoong_P1")
    orders, _, _ = O.adaptive_orders(N, h, snr, 1e-3, True)
    luts, sc = AdaptiveConstellationMapper(orders, QAMConstellationMapper, N).lut_tables()
    eng = LinkEngine(N, len(h) - 1, h, B.EQ_MMSE, luts, sc)
    short = S * eng.bps - 5
    # 6 dB below the loading's SNR: errors in most symbols, the last one's among the masked bits too
    per = check_against_calls(eng, S, snr - 6.0, what="adaptive, 5 bits short", n_valid=short)
    whole = check_against_calls(eng, S, snr - 6.0, what="adaptive", n_valid=S * eng.bps)
    assert per[:, 0].sum() > 0 and per[:-1].tolist() == whole[:-1].tolist() and per[-1, 1] == whole[-1, 1]
    res = eng.run(S, snr - 6.0, seed=SEED, frame_symbols=4, n_valid_bits=short)
    assert_record(res, per[:, 0], per[:, 1], 4, S, "engine, 5 bits short")
    assert res.frames.ber_stderr is None and res.frames.fer is not None


# ---------------------------------------------------------------- 4. accumulation
@pytest.mark.parametrize("case", [PE.THROUGHPUT_CASES[0], None], ids=["throughput", "generic"])
def test_calls_that_split_a_frame_accumulate(gpu, case):
    if case is None:
        eng, S, snr = geometry_engine(64, B.OFDM_F64), 67, 18.0
    else:
        (eng, _), S, snr = throughput_engine(case), case["S"], case["snr"]
    ys = Stream(eng, S, snr)
    F = 4
    cnt, rec = ys.frames(F)
    assert rec[:, 0].sum() == cnt[0] > 0
    for splits in ([S // 2 + 1], [1, 6, S - 1]):     # no split on a multiple of 4
        assert all(s % F for s in splits)
        cnt2, rec2 = ys.frames(F, splits=splits)
        assert cnt2 == cnt and np.array_equal(rec2, rec), splits
    cnt3, rec3 = ys.frames(F, splits=[S // 2 + 1], fill=1000)
    assert cnt3 == cnt and np.array_equal(rec3, rec + 1000)


# ---------------------------------------------------------------- 5. two gloo ranks on device 0
def test_two_ranks_hold_the_one_rank_record(gpu, tmp_path):
    case = PE.THROUGHPUT_CASES[1]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OFDM_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = tmp_path / "frames"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(ROOT, "tests", "frames_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    eng, _ = throughput_engine(case)
    one = eng.run(case["S"], case["snr"], seed=SEED, frame_symbols=4)
    assert 81 % 4 and one.bit_errors == case["bit_errors"]
    for rank in (0, 1):
        got = json.loads((tmp_path / f"frames.{rank}.json").read_text())
        assert got["world"] == 2 and got["shard"] == [[0, 81], [81, 163]][rank]
        assert got["totals"] == [one.bit_errors, one.symbol_errors]
        assert got["record"] == [one.frames.bit_errors.tolist(), one.frames.symbol_errors.tolist()], rank


# ---------------------------------------------------------------- 6. Simulation, and the routes
def test_simulation_frame_keys(gpu):
    case = golden_case("next_zp_n64_m16_p2_mmse", None)
    r = case["result"]
    plain = seeded_simulation(case)
    got = seeded_simulation(case, frame_symbols=8)
    keys = {"frame_symbols", "num_frames", "frame_errors", "frame_error_rate", "ber_std_error", "bit_errors_per_frame"}
    assert set(got) - set(plain) == keys and not keys & set(plain)
    assert (got["bit_errors"], got["symbol_errors"]) == (r["bit_errors"], r["symbol_errors"])
    assert (plain["bit_errors"], plain["symbol_errors"]) == (r["bit_errors"], r["symbol_errors"])
    per = got["bit_errors_per_frame"]
    assert isinstance(per, list) and sum(per) == r["bit_errors"]
    bps = 64 * 4
    S = -(-got["total_bits"] // bps)
    want = FE.stats(per, S, 8, bps)
    assert len(per) == -(-S // 8) and got["frame_symbols"] == 8 and got["num_frames"] == S // 8 == want["n_full"]
    assert got["frame_errors"] == want["frame_errors"] and got["frame_error_rate"] == want["fer"]
    if want["ber_stderr"] is None:
        assert got["ber_std_error"] is None
    else:
        assert got["ber_std_error"] == pytest.approx(want["ber_stderr"], rel=1e-13)


def test_routes_with_a_frame_record(gpu):
    case = PE.THROUGHPUT_CASES[0]     # the plan with a fused form
    eng, _ = throughput_engine(case)
    S, snr = case["S"], case["snr"]
    assert eng.has_fused
    events = []
    res = eng.run(S, snr, seed=SEED, frame_symbols=4, events=events)     # fused=None: the two-kernel path
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_rx_frames"] and res.bit_errors == case["bit_errors"]
    events = []
    assert eng.run(S, snr, seed=SEED, events=events).frames is None
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_link"]
    with pytest.raises(ValueError, match="frame record"):
        eng.run(S, snr, seed=SEED, frame_symbols=4, fused=True)
    with pytest.raises(ValueError, match="run_sweep"):
        eng.run_sweep(S, [snr, snr + 1], seed=SEED, frame_symbols=4)
    with pytest.raises(ValueError, match="run_pipelined"):
        eng.run_pipelined(S, snr, [SEED], frame_symbols=4)
    with pytest.raises(ValueError, match="profile"):
        eng.run(S, snr, seed=SEED, frame_symbols=4, profile=True)
    # a clip level and a tap are allowed
    h, cp, _ = PE.case_channel(case)
    clipped = LinkEngine(case["N"], cp, h, EQ[case["eq"]], [O.qam_lut(case["M"])], None, B.OFDM_F64, clip_db=4.0)
    res = clipped.run(S, snr, seed=SEED, frame_symbols=4, keep_symbols=3)
    assert int(res.frames.bit_errors.sum()) == res.bit_errors > 0 and res.clipped_samples > 0

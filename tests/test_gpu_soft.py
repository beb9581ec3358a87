"""The soft-decision record (ofdm_rx_soft, LinkEngine.run(soft=B), Simulation(soft_bins=B)) on the GPU
against tests/soft_expect.py, the NumPy restatement of the definition.

From the same stored value every double of the definition is the device's bit for bit, so a record is
compared exactly with the restatement of the run's own tap, in both precisions.  The throughput forms,
which have no tap, are compared with the oracle's points (Philox streams, the device's noise radii, the
run's exact power) inside soft_expect.bracket at the per-point bound of philox_streams.z_error_bound:
every cell holds its decided bits and at most the undecided ones that could land in it.

On the commit before the record every test here fails: LinkEngine.run has no ``soft`` argument.
"""

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT, load_stages, stage_arrays

import density_expect as DE
import ofdm_oracle as O
import philox_streams as P
import profile_expect as PE
import soft_expect as SE
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.engine import LinkEngine
from test_gpu_density import radius
from test_gpu_profile import VARIANTS, golden_case, seeded_simulation, throughput_engine

pytestmark = pytest.mark.gpu

EQ = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}
SEED = PE.SEED
GRIDS = ((128, 8.0), (6, 0.5), (256, 8.0))


def flat(d):
    """int64 [40 B + 1]: the record as the device holds it (the last entry: invalid)."""
    return SE.flat(d.counts, d.invalid)


def assert_equal(d, Z, idx, orders, g, what, **kw):
    got, want = flat(d), SE.flat(*SE.record(Z, idx, orders, g, d.bins, d.extent, **kw))
    assert np.array_equal(got, want), (what, d.bins, d.extent, np.flatnonzero(got != want)[:8],
                                       got[got != want][:8], want[got != want][:8])
    assert int(d.counts.sum()) + d.invalid == d.n_bits


def assert_inside(got, dec, maybe, what):
    over = got - dec
    print(f"{what}: {int(maybe.sum())} candidate cells of undecided bits, {int(np.count_nonzero(over))} cells above "
          f"their decided count")
    assert np.all(over >= 0) and np.all(over <= maybe), (what, np.flatnonzero((over < 0) | (over > maybe))[:8])


def tx_idx(tx_bytes, S, N, b):
    return O.bits_to_indices(O.bytes_to_bits(tx_bytes)[:S * N * b], b).reshape(S, N)


# ---------------------------------------------------------------- 1. own tap, the generic form
@pytest.mark.parametrize("precision", [B.OFDM_F64, B.OFDM_F32], ids=["complex128", "complex64"])
@pytest.mark.parametrize("st", load_stages(), ids=lambda s: s["name"])
def test_exact_against_the_runs_own_tap(gpu, st, precision):
    a = stage_arrays(st["name"])
    S, N, M = st["S"], st["N"], st["M"]
    b = M.bit_length() - 1
    eng = LinkEngine(N, st["cp"], a["h_raw"], EQ[st["eq"]], [O.qam_lut(M)], precision=precision)
    kw = dict(bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]), keep_symbols=S)
    plain = eng.run(S, st["snr_db"], **kw)
    assert plain.soft is None
    idx = tx_idx(a["tx_bytes"], S, N, b)
    g = SE.scale(M, N)
    for Bn, L in GRIDS:
        res = eng.run(S, st["snr_db"], soft=Bn, soft_extent=L, **kw)
        d = res.soft
        Z = res.received.reshape(S, N)
        assert Z.dtype == (np.complex128 if precision == B.OFDM_F64 else np.complex64)
        assert d.counts.shape == (20, 2, Bn) and d.counts.dtype == np.int64
        assert (d.bins, d.extent, d.subcarriers) == (Bn, L, (0, N))
        assert_equal(d, Z, idx, M, g, st["name"])
        # the receiver beside the record is ofdm_rx's
        assert (res.bit_errors, res.symbol_errors) == (plain.bit_errors, plain.symbol_errors)
        assert np.array_equal(res.received, plain.received)
        # the sum is the compared bits, the mass on the wrong side the bit errors, only the order's rows fill
        assert d.n_bits == S * N * b and d.invalid == 0
        assert d.hard_bit_errors == res.bit_errors
        assert d.orders == (b,) and int(d.rows(b).sum()) == d.n_bits
        if precision == B.OFDM_F64:
            assert res.bit_errors == st["bit_errors"]


# ---------------------------------------------------------------- 2. throughput forms against the oracle
@pytest.mark.parametrize("case", PE.THROUGHPUT_CASES, ids=lambda c: c["id"])
def test_throughput_forms_against_the_oracle(gpu, case):
    eng, bk = throughput_engine(case)
    N, S, snr, Bn, L = case["N"], case["S"], case["snr"], 128, 8.0
    h, cp, orders = PE.case_channel(case)
    o = SE.per_subcarrier(case["M"] if orders is None else orders, N)
    g = SE.scale(o, N)
    n_valid = eng.valid_bits(S)
    plain = eng.run(S, snr, seed=SEED, fused=False)
    assert (plain.bit_errors, plain.symbol_errors) == (case["bit_errors"], case["symbol_errors"])
    Z, delta, idx = DE.philox_points(SEED, S, N, case["M"], h, cp, case["eq"], snr, orders=orders, radius_fn=radius,
                                     power_sum=plain.power_sum)
    # the condition on the inputs, from the oracle alone: few bits near a bin line
    share = SE.undecided_share(Z, delta, idx, o, g, Bn, L, n_valid=n_valid)
    print(f"{case['id']}: max bound {delta.max():.3e}, undecided share {share:.3e} at B = {Bn}, L = {L}")
    assert share <= 1e-3
    dec, maybe = SE.bracket(Z, delta, idx, o, g, Bn, L, n_valid=n_valid)

    events = []
    res = eng.run(S, snr, seed=SEED, soft=Bn, events=events)
    d = res.soft
    # the form: the record's own entry point, no tap, and the throughput receiver's pinned counts
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_rx_soft"] and res.received is None
    assert (res.bit_errors, res.symbol_errors) == (case["bit_errors"], case["symbol_errors"])
    assert d.extent == L and d.n_bits == n_valid == int(d.counts.sum()) and d.invalid == 0
    assert_inside(flat(d), dec, maybe, case["id"] + " against the oracle")
    assert d.hard_bit_errors == case["bit_errors"]

    # the same run on the generic form (a tap forces it): exact against its own tap, and the throughput
    # record within twice the bound of it
    events = []
    gen = eng.run(S, snr, seed=SEED, soft=Bn, keep_symbols=S, events=events)
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_rx_soft"]
    Zg = gen.received.reshape(S, N)
    assert_equal(gen.soft, Zg, idx, o, g, case["id"] + " generic form", n_valid=n_valid)
    assert_inside(flat(gen.soft), dec, maybe, case["id"] + " generic form against the oracle")
    dec2, maybe2 = SE.bracket(Zg, 2.0 * delta, idx, o, g, Bn, L, n_valid=n_valid)
    assert_inside(flat(d), dec2, maybe2, case["id"] + " against the generic form")
    assert (gen.bit_errors, gen.symbol_errors) == (res.bit_errors, res.symbol_errors)
    assert gen.soft.hard_bit_errors == case["bit_errors"]
    # the rows: the adaptive case loads 4- and 16-QAM only, the 256-QAM case its own eight rows
    filled = np.flatnonzero(d.counts.sum(axis=(1, 2))).tolist()
    if case["id"] == "n2048_adaptive_p1_mmse":
        assert set(np.unique(o)) <= {0, 4, 16} and filled == list(range(0, 6))
    elif case["M"] == 256:
        assert filled == list(range(12, 20))
    else:
        assert filled == list(range(6, 12))
    print(f"{case['id']}: gmi {d.gmi():.4f} bits per subcarrier use")


# ---------------------------------------------------------------- 3. invariance
def test_record_does_not_depend_on_the_batching_or_a_batched_tap(gpu):
    case = PE.THROUGHPUT_CASES[0]
    eng, _ = throughput_engine(case)
    S, N, snr = case["S"], case["N"], case["snr"]
    one = eng.run(S, snr, seed=SEED, soft=128)
    for extra in (dict(batch=1), dict(batch=3), dict(batch=50), dict(y_budget=40 * eng._ybytes())):
        got = eng.run(S, snr, seed=SEED, soft=128, **extra)
        assert (got.bit_errors, got.symbol_errors) == (one.bit_errors, one.symbol_errors)
        assert np.array_equal(flat(got.soft), flat(one.soft)), extra
    # with a tap every batch takes the generic form (z_out with z_keep = 0 on the later ones): the
    # batched record with a short tap is the one-batch tapped record, exactly
    tapped = eng.run(S, snr, seed=SEED, soft=128, keep_symbols=S)
    idx = P.tx_indices(P.lane_generators(SEED, np.arange(S), N), S, N, 6)
    assert_equal(tapped.soft, tapped.received.reshape(S, N), idx, case["M"], SE.scale(case["M"], N), "tapped")
    for extra in (dict(batch=50), dict(batch=3), dict(y_budget=40 * eng._ybytes())):
        got = eng.run(S, snr, seed=SEED, soft=128, keep_symbols=5, **extra)
        assert np.array_equal(flat(got.soft), flat(tapped.soft)), extra
        assert np.array_equal(got.received, tapped.received[:5 * N])


@pytest.mark.parametrize("form", ["throughput", "generic"])
def test_calls_over_halves_accumulate(gpu, form):
    case = PE.THROUGHPUT_CASES[0]
    eng, _ = throughput_engine(case)
    S, N, snr, Bn = case["S"], case["N"], case["snr"], 64
    dev, stream = eng.device(), eng.stream()
    inv_w = E.soft_grid(Bn, 8.0)
    g = eng.upload(E.soft_scale([O.qam_lut(case["M"])], None, None, np.array([1.0 + 0j]), N))
    y, stats = eng._y(S), E.new_stats(dev)
    eng.tx(stream, None, SEED, 0, S, y, stats)
    z = torch.empty((1, N), dtype=eng.cdtype, device=dev) if form == "generic" else None
    words = 40 * Bn + 1

    def record(splits, fill):
        rec = torch.full((words,), fill, dtype=torch.int64, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        edges = [0] + splits + [S]
        for a, b in zip(edges[:-1], edges[1:]):
            eng.rx(stream, y[a:], None, None, SEED, stats, S * (N + eng.cp), snr, True, None, a, b - a,
                   eng.valid_bits(S), cnt, z, 0, soft=rec, soft_params=(g, inv_w, Bn), soft_subcarriers=(0, N))
        return cnt.cpu().numpy().tolist(), rec.cpu().numpy()

    cnt, rec = record([], 0)
    assert rec.sum() == S * N * 6 and cnt == [case["bit_errors"], case["symbol_errors"]]
    for splits in ([S // 2], [1, 70, S - 1]):
        cnt2, rec2 = record(splits, 0)
        assert cnt2 == cnt and np.array_equal(rec2, rec), splits
    cnt3, rec3 = record([S // 2], 1000)
    assert cnt3 == cnt and np.array_equal(rec3, rec + 1000)
    # an empty call is an empty call
    empty = torch.zeros(words, dtype=torch.int64, device=dev)
    eng.rx(stream, y, None, None, SEED, stats, S * (N + eng.cp), snr, True, None, 0, 0, eng.valid_bits(S),
           torch.zeros(2, dtype=torch.int64, device=dev), None, 0, soft=empty, soft_params=(g, inv_w, Bn),
           soft_subcarriers=(0, N))
    assert not empty.cpu().numpy().any()


def test_two_ranks_hold_the_one_rank_record(gpu, tmp_path):
    case = PE.THROUGHPUT_CASES[0]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OFDM_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = tmp_path / "soft"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(ROOT, "tests", "soft_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    eng, _ = throughput_engine(case)
    one = eng.run(case["S"], case["snr"], seed=SEED, soft=64)
    assert one.bit_errors == case["bit_errors"]
    for rank in (0, 1):
        got = json.loads((tmp_path / f"soft.{rank}.json").read_text())
        assert got["world"] == 2 and got["shard"] == [[0, 81], [81, 163]][rank]
        assert got["totals"] == [one.bit_errors, one.symbol_errors]
        assert got["invalid"] == one.soft.invalid and got["n_bits"] == one.soft.n_bits
        assert np.array_equal(np.asarray(got["counts"], np.int64), one.soft.counts), rank


# ---------------------------------------------------------------- 4, 5. the subcarrier range and the weights
def stage_engine(name):
    st = next(s for s in load_stages() if s["name"] == name)
    a = stage_arrays(name)
    eng = LinkEngine(st["N"], st["cp"], a["h_raw"], EQ[st["eq"]], [O.qam_lut(st["M"])])
    kw = dict(bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]))
    idx = tx_idx(a["tx_bytes"], st["S"], st["N"], st["M"].bit_length() - 1)
    return st, a, eng, kw, idx


def test_subcarrier_range(gpu):
    st, a, eng, kw, idx = stage_engine("n64_m16_severe_cp_mmse")
    S, N, M, Bn, L = st["S"], st["N"], st["M"], 32, 4.0
    whole = eng.run(S, st["snr_db"], soft=Bn, soft_extent=L, keep_symbols=S, **kw)
    Z = whole.received.reshape(S, N)
    g = SE.scale(M, N)

    def run(rng):
        res = eng.run(S, st["snr_db"], soft=Bn, soft_extent=L, soft_subcarriers=rng, **kw)
        assert res.soft.subcarriers == rng
        assert (res.bit_errors, res.symbol_errors) == (whole.bit_errors, whole.symbol_errors)
        return res.soft

    assert np.array_equal(flat(run((0, N))), flat(whole.soft))
    one = run((5, 6))
    assert one.n_bits == S * 4
    assert np.array_equal(flat(one), SE.flat(*SE.record(Z, idx, M, g, Bn, L, 5, 6)))
    lo, hi = run((0, 23)), run((23, N))
    assert lo.n_bits == 23 * S * 4 and hi.n_bits == (N - 23) * S * 4
    assert np.array_equal(flat(lo) + flat(hi), flat(whole.soft))
    with pytest.raises(ValueError, match="soft_subcarriers"):
        run((0, N + 1))


def test_weights(gpu):
    st, a, eng, kw, idx = stage_engine("n64_m16_severe_cp_mmse")
    S, N, M = st["S"], st["N"], st["M"]
    plain = eng.run(S, st["snr_db"], soft=128, keep_symbols=S, **kw)
    arr = np.linspace(0.25, 3.0, N)
    for w, table in (("csi", E.soft_scale([O.qam_lut(M)], None, "csi", a["h_raw"], N)),
                     (arr, E.soft_scale([O.qam_lut(M)], None, arr, a["h_raw"], N))):
        res = eng.run(S, st["snr_db"], soft=128, soft_weights=w, keep_symbols=S, **kw)
        assert np.array_equal(res.received, plain.received)
        assert_equal(res.soft, res.received.reshape(S, N), idx, M, table, "weights")
        # positive weights move no value across zero
        assert res.soft.hard_bit_errors == plain.soft.hard_bit_errors == res.bit_errors
        assert not np.array_equal(flat(res.soft), flat(plain.soft))
    assert np.array_equal(E.soft_scale([O.qam_lut(M)], None, "csi", a["h_raw"], N), SE.scale(M, N, SE.csi_weights(a["h_raw"], N)))


# ---------------------------------------------------------------- 6. noise off
def test_noise_off_16qam(gpu):
    N, M, S, Bn, L = 64, 16, 67, 128, 8.0
    lut = O.qam_lut(M)
    eng = LinkEngine(N, 0, np.array([1.0 + 0j]), B.EQ_NONE, [lut])
    res = eng.run(S, 20.0, seed=SEED, noise_on=False, soft=Bn, soft_extent=L)
    assert res.bit_errors == 0 and res.symbol_errors == 0
    d = res.soft
    assert d.invalid == 0 and d.hard_bit_errors == 0 and d.n_bits == S * N * 4
    # every count sits in a bin the restatement names for one of the sixteen points: the received point is
    # the LUT point to within the transforms' rounding, which may move a value across the line it sits on
    idx = np.arange(M)[None, :]
    names = np.zeros(40 * Bn + 1, bool)
    for eps in (0.0, 1e-12, -1e-12):
        for ph in (1.0, 1j, 1 + 1j, 1 - 1j):
            names |= SE.flat(*SE.record(lut[idx] + eps * ph, idx, M, SE.scale(M, M), Bn, L)) > 0
    assert not np.any(flat(d)[~names])
    assert d.gmi() > 4 - 1e-9 and d.gmi(4) > 4 - 1e-9


# ---------------------------------------------------------------- 7. routes and refusals
def test_routes_and_refusals(gpu):
    case = PE.THROUGHPUT_CASES[0]     # the plan with a fused form
    eng, _ = throughput_engine(case)
    S, N, snr = case["S"], case["N"], case["snr"]
    assert eng.has_fused
    events = []
    assert eng.run(S, snr, seed=SEED, events=events).soft is None
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_link"]
    events = []
    assert eng.run(S, snr, seed=SEED, soft=8, events=events).soft is not None   # None: the two-kernel path
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_rx_soft"]
    with pytest.raises(ValueError, match="soft record"):
        eng.run(S, snr, seed=SEED, soft=8, fused=True)
    with pytest.raises(ValueError, match="run_sweep"):
        eng.run_sweep(S, [snr, snr + 1], seed=SEED, soft=8)
    with pytest.raises(ValueError, match="run_frame_sweep"):
        eng.run_frame_sweep(S, [snr, snr + 1], 4, seed=SEED, soft=8)
    with pytest.raises(ValueError, match="run_pipelined"):
        eng.run_pipelined(S, snr, [SEED], soft=8)
    for other in (dict(profile=True), dict(frame_symbols=4), dict(density=8)):
        with pytest.raises(ValueError, match="not built"):
            eng.run(S, snr, seed=SEED, soft=8, **other)
    for bad in (0, 7, 258, 2.5):
        with pytest.raises(ValueError, match="soft"):
            eng.run(S, snr, seed=SEED, soft=bad)
    with pytest.raises(ValueError, match="soft_extent"):
        eng.run(S, snr, seed=SEED, soft=8, soft_extent=0.0)
    with pytest.raises(ValueError, match="soft_weights"):
        eng.run(S, snr, seed=SEED, soft=8, soft_weights=np.ones(3))
    with pytest.raises(ValueError, match="without soft"):
        eng.run(S, snr, seed=SEED, soft_extent=2.0)
    # PSK and wide plans: refused by the engine, and by the library under the function's name
    h, cp, _ = PE.case_channel(case)
    for lut in (O.psk_lut(8), O.qam_lut(1024)):
        other = LinkEngine(64, 0, np.array([1.0 + 0j]), B.EQ_NONE, [lut])
        bits = np.zeros(64 * 10 * 4 // 8 + 8, np.uint8)
        with pytest.raises(ValueError, match="not built"):
            other.run(4, 20.0, bits=bits, soft=8)
        dev = other.device()
        rec = torch.zeros(40 * 8 + 1, dtype=torch.int64, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        with pytest.raises(Exception, match="ofdm_rx_soft.*not built"):
            other.rx(other.stream(), other._y(2), None, None, SEED, E.new_stats(dev), 2 * 64, 20.0, False,
                     other.upload(bits), 0, 2, 2 * other.bps, cnt, None, 0, soft=rec,
                     soft_params=(torch.ones(64, dtype=torch.float64, device=dev), 1.0, 8), soft_subcarriers=(0, 64))
        assert not rec.cpu().numpy().any() and not cnt.cpu().numpy().any()
    # a clip level is allowed: the record behind the counters and the clip record
    clipped = LinkEngine(N, cp, h, EQ[case["eq"]], [O.qam_lut(case["M"])], None, B.OFDM_F64, clip_db=4.0)
    res = clipped.run(S, snr, seed=SEED, soft=16, keep_symbols=S)
    assert res.clip_samples == S * N and res.clipped_samples > 0
    idx = P.tx_indices(P.lane_generators(SEED, np.arange(S), N), S, N, 6)
    assert_equal(res.soft, res.received.reshape(S, N), idx, case["M"], SE.scale(case["M"], N), "clipped")


# ---------------------------------------------------------------- 8. modem variants through Simulation
@pytest.mark.parametrize("tag,snr", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_simulation_variants(gpu, monkeypatch, tag, snr):
    case = golden_case(tag, snr)
    p, r = case["params"], case["result"]
    plain = seeded_simulation(case, received_symbols_keep=1 << 30)
    orders = np.asarray(plain["constellation_order_per_subcarrier"], np.int64)
    Bn, L = 64, 8.0
    if "PSK" in str(p.get("constellation_scheme", "")).upper() or orders.max() > 256:
        # the constellations the record is not built for: refused, naming it
        with pytest.raises(ValueError, match="not built"):
            seeded_simulation(case, soft_bins=Bn)
        return
    # the run's own tx bytes and compared-bit count, as Simulation hands them to the engine
    seen = {}
    run_async = LinkEngine.run_async

    def spy(self, n_sym, snr_db, **kw):
        seen.update(bits=kw.get("bits"), n_valid=kw.get("n_valid_bits"), n_sym=n_sym)
        return run_async(self, n_sym, snr_db, **kw)

    monkeypatch.setattr(LinkEngine, "run_async", spy)
    got = seeded_simulation(case, soft_bins=Bn, soft_extent=L, received_symbols_keep=1 << 30)
    monkeypatch.undo()
    assert set(got) - set(plain) == {"soft_decisions"} and "soft_decisions" not in plain
    assert (got["bit_errors"], got["symbol_errors"]) == (r["bit_errors"], r["symbol_errors"])
    sd = got["soft_decisions"]
    assert set(sd) == {"bins", "extent", "counts", "invalid", "num_bits", "gmi_bits_per_subcarrier", "gmi_scale"}
    assert isinstance(sd["counts"], list) and (sd["bins"], sd["extent"]) == (Bn, L)
    N = p["num_subcarriers"]
    bk = np.array([int(o).bit_length() - 1 if o > 0 else 0 for o in orders], np.int64)
    bps = int(bk.sum())
    S = seen["n_sym"]
    Z = got["received_symbols"].reshape(S, N)
    assert np.array_equal(got["received_symbols"], plain["received_symbols"])
    bits = O.bytes_to_bits(np.asarray(seen["bits"], np.uint8))[:S * bps].reshape(S, bps)
    off = np.concatenate([[0], np.cumsum(bk)[:-1]])
    idx = np.zeros((S, N), np.int64)
    for k in np.flatnonzero(bk):
        idx[:, k] = bits[:, off[k]:off[k] + bk[k]] @ (1 << np.arange(bk[k] - 1, -1, -1))
    n_valid = min(int(seen["n_valid"]), S * bps)
    counts, invalid = SE.record(Z, idx, orders, SE.scale(orders, N), Bn, L, n_valid=n_valid)
    assert np.array_equal(np.asarray(sd["counts"], np.int64), counts) and sd["invalid"] == invalid
    assert sd["num_bits"] == n_valid == int(counts.sum()) + invalid
    assert SE.hard_bit_errors(counts) == r["bit_errors"]
    d = E.SoftDecisions(counts=counts, invalid=invalid, bins=Bn, extent=L, subcarriers=(0, N), n_bits=n_valid)
    assert sd["gmi_bits_per_subcarrier"] == pytest.approx(d.gmi(), abs=1e-12)
    assert set(sd["gmi_scale"]) == {str(b) for b in d.orders}

"""The constellation-density record (ofdm_rx_density, LinkEngine.run(density=G),
Simulation(constellation_density=G)) on the GPU against tests/density_expect.py, the NumPy restatement
of the index.

From the same stored value the index is the device's bit for bit, so a record is compared exactly with
the binning of the run's own tap, in both precisions; and exactly with the binning of a stage fixture's
Z, which tests/test_density_cpu.py entitles (no fixture point lies within the tolerance on Z of a grid
line).  The throughput forms, which have no tap, are compared with the oracle's points (Philox streams,
the device's noise radii, the run's exact power) inside density_expect.bracket at the per-point bound of
philox_streams.z_error_bound: every bin holds its decided points and at most the undecided ones that
could land in it.

On the commit before the record every test here fails: LinkEngine.run has no ``density`` argument.
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
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.engine import LinkEngine
from test_gpu_profile import VARIANTS, golden_case, seeded_simulation, throughput_engine

pytestmark = pytest.mark.gpu

EQ = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}
SEED = PE.SEED


def flat(d):
    """int64 [G * G + 1]: the record as the device holds it (the last entry: outside)."""
    return np.concatenate([d.counts.ravel(), [d.outside]]).astype(np.int64)


def expect_flat(Z, G, L, *a, **kw):
    c, o = DE.bin_points(Z, G, L, *a, **kw)
    return np.concatenate([c.ravel(), [o]]).astype(np.int64)


def assert_equal(d, Z, G, L, what, **kw):
    got, want = flat(d), expect_flat(Z, G, L, **kw)
    assert np.array_equal(got, want), (what, G, L, np.flatnonzero(got != want)[:8])
    assert int(d.counts.sum()) + d.outside == d.n_points


def assert_inside(got, dec, maybe, what):
    over = got - dec
    print(f"{what}: {int(maybe.sum())} candidate cells of undecided points, {int(np.count_nonzero(over))} bins above "
          f"their decided count")
    assert np.all(over >= 0) and np.all(over <= maybe), (what, np.flatnonzero((over < 0) | (over > maybe))[:8])


# ---------------------------------------------------------------- 1, 2. reference streams, the generic form
_STAGE_RUNS = {}


def stage_runs(st, precision):
    """The stage's runs, once per (fixture, precision): (arrays, {(G, L): LinkStats})."""
    key = (st["name"], precision)
    if key not in _STAGE_RUNS:
        a = stage_arrays(st["name"])
        eng = LinkEngine(st["N"], st["cp"], a["h_raw"], EQ[st["eq"]], [O.qam_lut(st["M"])], precision=precision)
        S = st["S"]
        runs = {}
        for G, L in ((31, 2.0), (128, 2.0), (31, 1.0)):
            runs[(G, L)] = eng.run(S, st["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]),
                                   keep_symbols=S, density=G, density_extent=L)
        runs["plain"] = eng.run(S, st["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]),
                                keep_symbols=S)
        _STAGE_RUNS[key] = (a, runs)
    return _STAGE_RUNS[key]


@pytest.mark.parametrize("precision", [B.OFDM_F64, B.OFDM_F32], ids=["complex128", "complex64"])
@pytest.mark.parametrize("st", load_stages(), ids=lambda s: s["name"])
def test_exact_against_the_runs_own_tap(gpu, st, precision):
    a, runs = stage_runs(st, precision)
    S, N = st["S"], st["N"]
    plain = runs["plain"]
    assert plain.density is None
    for (G, L) in ((31, 2.0), (128, 2.0), (31, 1.0)):
        res = runs[(G, L)]
        d = res.density
        Z = res.received.reshape(S, N)
        assert Z.dtype == (np.complex128 if precision == B.OFDM_F64 else np.complex64)
        assert d.counts.shape == (G, G) and d.extent == L and d.subcarriers == (0, N)
        assert_equal(d, Z, G, L, st["name"])
        assert d.n_points == S * N
        # the receiver beside the record is ofdm_rx's
        assert (res.bit_errors, res.symbol_errors) == (plain.bit_errors, plain.symbol_errors)
        assert np.array_equal(res.received, plain.received)
        if precision == B.OFDM_F64:  # as test_stage_fixtures_generic_kernel
            assert (res.bit_errors, res.symbol_errors) == (st["bit_errors"], st["symbol_errors"])
    # L = 1.0 exercises `outside` wherever the fixture reaches it (every fixture but the N = 8 one, whose
    # largest coordinate is 0.99); no fixture reaches 2.0
    reach = max(np.abs(a["Z"].real).max(), np.abs(a["Z"].imag).max())
    assert (runs[(31, 1.0)].density.outside > 0) == (reach >= 1.0 + 1e-6) and abs(reach - 1.0) > 1e-6
    assert (reach >= 1.0) == (st["N"] > 8) and runs[(31, 2.0)].density.outside == 0


@pytest.mark.parametrize("st", load_stages(), ids=lambda s: s["name"])
def test_exact_against_the_fixture(gpu, st):
    a, runs = stage_runs(st, B.OFDM_F64)
    for G in (31, 128):
        res = runs[(G, 2.0)]
        np.testing.assert_allclose(res.received, a["Z"].ravel(), rtol=1e-9, atol=1e-9)
        assert_equal(res.density, a["Z"].reshape(st["S"], st["N"]), G, 2.0, st["name"] + " against the fixture")


# ---------------------------------------------------------------- 3. throughput streams, bench shapes
def radius(words):
    """The receivers' noise radius of each lane word on this GPU (ofdm_noise_radius)."""
    w = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to("cuda")
    r = torch.empty(w.numel(), dtype=torch.float32, device="cuda")
    B.check(B.lib().ofdm_noise_radius(B.stream_ptr(), B.ptr(w), w.numel(), B.ptr(r)))
    return r.cpu().numpy()


@pytest.mark.parametrize("case", PE.THROUGHPUT_CASES, ids=lambda c: c["id"])
def test_throughput_forms_against_the_oracle(gpu, case):
    eng, bk = throughput_engine(case)
    N, S, snr, G = case["N"], case["S"], case["snr"], 128
    active = bk > 0
    L = 1.5 * eng.lut_reach   # the default extent
    h, cp, orders = PE.case_channel(case)
    plain = eng.run(S, snr, seed=SEED, fused=False)
    assert (plain.bit_errors, plain.symbol_errors) == (case["bit_errors"], case["symbol_errors"])
    Z, delta, _ = DE.philox_points(SEED, S, N, case["M"], h, cp, case["eq"], snr, orders=orders, radius_fn=radius,
                                   power_sum=plain.power_sum)
    # the condition on the inputs, from the oracle alone: few points near a grid line
    share = float(np.mean(DE.undecided(Z[:, active], delta[:, active], G, L)))
    print(f"{case['id']}: max bound {delta.max():.3e}, undecided share {share:.3e} at G = {G}, L = {L:.4f}")
    assert share <= 1e-3
    dec, maybe = DE.bracket(Z, delta, G, L, active=active)

    events = []
    res = eng.run(S, snr, seed=SEED, density=G, events=events)
    d = res.density
    # the form: the record's own entry point, no tap, and the throughput receiver's pinned counts
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_rx_density"] and res.received is None
    assert (res.bit_errors, res.symbol_errors) == (case["bit_errors"], case["symbol_errors"])
    assert d.extent == L and d.n_points == S * int(np.count_nonzero(active)) == int(d.counts.sum()) + d.outside
    assert_inside(flat(d), dec, maybe, case["id"] + " against the oracle")

    # the same run on the generic form (a tap forces it): exact against its own tap, and the throughput
    # record within twice the bound of it
    events = []
    gen = eng.run(S, snr, seed=SEED, density=G, keep_symbols=S, events=events)
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_rx_density"]
    Zg = gen.received.reshape(S, N)
    assert_equal(gen.density, Zg, G, L, case["id"] + " generic form", active=active)
    assert_inside(flat(gen.density), dec, maybe, case["id"] + " generic form against the oracle")
    dec2, maybe2 = DE.bracket(Zg, 2.0 * delta, G, L, active=active)
    assert_inside(flat(d), dec2, maybe2, case["id"] + " against the generic form")
    assert (gen.bit_errors, gen.symbol_errors) == (res.bit_errors, res.symbol_errors)


def test_routes_with_a_density_record(gpu):
    case = PE.THROUGHPUT_CASES[0]     # the plan with a fused form
    eng, _ = throughput_engine(case)
    S, snr = case["S"], case["snr"]
    assert eng.has_fused
    events = []
    assert eng.run(S, snr, seed=SEED, events=events).density is None
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_link"]
    with pytest.raises(ValueError, match="density record"):
        eng.run(S, snr, seed=SEED, density=8, fused=True)
    with pytest.raises(ValueError, match="run_sweep"):
        eng.run_sweep(S, [snr, snr + 1], seed=SEED, density=8)
    with pytest.raises(ValueError, match="run_pipelined"):
        eng.run_pipelined(S, snr, [SEED], density=8)
    with pytest.raises(ValueError, match="profile"):
        eng.run(S, snr, seed=SEED, density=8, profile=True)
    with pytest.raises(ValueError, match="frame_symbols"):
        eng.run(S, snr, seed=SEED, density=8, frame_symbols=4)
    # a clip level is allowed: the record behind the counters and the clip record
    h, cp, _ = PE.case_channel(case)
    clipped = LinkEngine(case["N"], cp, h, EQ[case["eq"]], [O.qam_lut(case["M"])], None, B.OFDM_F64, clip_db=4.0)
    res = clipped.run(S, snr, seed=SEED, density=16, keep_symbols=S)
    assert res.clip_samples == S * case["N"] and res.clipped_samples > 0
    assert_equal(res.density, res.received.reshape(S, case["N"]), 16, res.density.extent, "clipped")


# ---------------------------------------------------------------- 4. invariance
def test_generic_record_does_not_depend_on_the_batching(gpu):
    st = next(s for s in load_stages() if s["name"] == "n64_m16_severe_cp_mmse")
    a, runs = stage_runs(st, B.OFDM_F64)
    eng = LinkEngine(st["N"], st["cp"], a["h_raw"], EQ[st["eq"]], [O.qam_lut(st["M"])])
    want = flat(runs[(31, 2.0)].density)
    kw = dict(bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]), density=31, density_extent=2.0)
    for extra in (dict(batch=1), dict(batch=3), dict(y_budget=3 * eng._ybytes()), dict(batch=3, keep_symbols=2)):
        got = eng.run(st["S"], st["snr_db"], **kw, **extra)
        assert np.array_equal(flat(got.density), want), extra


def test_throughput_record_does_not_depend_on_the_batching_or_a_batched_tap(gpu):
    case = PE.THROUGHPUT_CASES[0]
    eng, _ = throughput_engine(case)
    S, snr = case["S"], case["snr"]
    one = eng.run(S, snr, seed=SEED, density=128)
    for extra in (dict(batch=1), dict(batch=3), dict(batch=50), dict(y_budget=40 * eng._ybytes())):
        got = eng.run(S, snr, seed=SEED, density=128, **extra)
        assert (got.bit_errors, got.symbol_errors) == (one.bit_errors, one.symbol_errors)
        assert np.array_equal(flat(got.density), flat(one.density)), extra
    # with a tap every batch takes the generic form (z_out with z_keep = 0 on the later ones): the
    # batched record is the one-batch tapped record, exactly
    tapped = eng.run(S, snr, seed=SEED, density=128, keep_symbols=S)
    assert_equal(tapped.density, tapped.received.reshape(S, case["N"]), 128, tapped.density.extent, "tapped")
    for extra in (dict(batch=50), dict(batch=3), dict(y_budget=40 * eng._ybytes())):
        got = eng.run(S, snr, seed=SEED, density=128, keep_symbols=5, **extra)
        assert np.array_equal(flat(got.density), flat(tapped.density)), extra
        assert np.array_equal(got.received, tapped.received[:5 * case["N"]])


def test_two_ranks_hold_the_one_rank_record(gpu, tmp_path):
    case = PE.THROUGHPUT_CASES[0]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OFDM_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = tmp_path / "density"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(ROOT, "tests", "density_worker.py"), str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    eng, _ = throughput_engine(case)
    one = eng.run(case["S"], case["snr"], seed=SEED, density=64)
    assert one.bit_errors == case["bit_errors"]
    for rank in (0, 1):
        got = json.loads((tmp_path / f"density.{rank}.json").read_text())
        assert got["world"] == 2 and got["shard"] == [[0, 81], [81, 163]][rank]
        assert got["totals"] == [one.bit_errors, one.symbol_errors]
        assert got["outside"] == one.density.outside and got["n_points"] == one.density.n_points
        assert np.array_equal(np.asarray(got["counts"], np.int64), one.density.counts), rank


# ---------------------------------------------------------------- 5. modem variants through Simulation
@pytest.mark.parametrize("tag,snr", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_simulation_variants(gpu, tag, snr):
    case = golden_case(tag, snr)
    p, r = case["params"], case["result"]
    plain = seeded_simulation(case)
    G, L = 64, 2.0
    got = seeded_simulation(case, constellation_density=G, constellation_density_extent=L,
                            received_symbols_keep=1 << 30)
    assert set(got) - set(plain) == {"constellation_density"} and "constellation_density" not in plain
    assert (got["bit_errors"], got["symbol_errors"]) == (r["bit_errors"], r["symbol_errors"])
    cd = got["constellation_density"]
    assert set(cd) == {"bins", "extent", "counts", "outside", "num_points"} and isinstance(cd["counts"], list)
    N = p["num_subcarriers"]
    orders = np.asarray(got["constellation_order_per_subcarrier"], np.int64)
    active = orders > 0
    bits = sum(int(o).bit_length() - 1 for o in orders if o > 0)
    S = got["total_bits"] // bits
    Z = got["received_symbols"].reshape(S, N)
    counts, outside = DE.bin_points(Z, G, L, active=active)
    assert (cd["bins"], cd["extent"]) == (G, L)
    assert np.array_equal(np.asarray(cd["counts"], np.int64), counts) and cd["outside"] == outside
    assert cd["num_points"] == S * int(np.count_nonzero(active)) == int(counts.sum()) + outside
    if tag == "cfg_d_n64_adaptive":
        assert not active.all()   # order-0 subcarriers carry no point


# ---------------------------------------------------------------- 6. the subcarrier range
def test_subcarrier_range(gpu):
    st = next(s for s in load_stages() if s["name"] == "n64_m16_severe_cp_mmse")
    a, runs = stage_runs(st, B.OFDM_F64)
    S, N, G, L = st["S"], st["N"], 31, 2.0
    eng = LinkEngine(N, st["cp"], a["h_raw"], EQ[st["eq"]], [O.qam_lut(st["M"])])
    whole = runs[(G, L)]
    Z = whole.received.reshape(S, N)

    def run(rng):
        res = eng.run(S, st["snr_db"], bits=a["tx_bytes"], normals=(a["noise_re"], a["noise_im"]), density=G,
                      density_extent=L, density_subcarriers=rng)
        assert res.density.subcarriers == rng
        assert (res.bit_errors, res.symbol_errors) == (whole.bit_errors, whole.symbol_errors)
        return res.density

    assert np.array_equal(flat(run((0, N))), flat(whole.density))
    one = run((5, 6))
    assert one.n_points == S and np.array_equal(flat(one), expect_flat(Z[:, 5:6], G, L))
    assert np.array_equal(flat(one), expect_flat(Z, G, L, 5, 6))
    lo, hi = run((0, 23)), run((23, N))
    assert lo.n_points == 23 * S and hi.n_points == (N - 23) * S
    assert np.array_equal(flat(lo) + flat(hi), flat(whole.density))
    with pytest.raises(ValueError, match="density_subcarriers"):
        run((0, N + 1))


# ---------------------------------------------------------------- 7. accumulate, never zero (the ABI)
@pytest.mark.parametrize("form", ["throughput", "generic"])
def test_calls_over_halves_accumulate(gpu, form):
    case = PE.THROUGHPUT_CASES[0]
    eng, _ = throughput_engine(case)
    S, N, snr, G = case["S"], case["N"], case["snr"], 64
    dev, stream = eng.device(), eng.stream()
    lo, inv_w = E.density_grid(G, 2.0)
    y, stats = eng._y(S), E.new_stats(dev)
    eng.tx(stream, None, SEED, 0, S, y, stats)
    z = torch.empty((1, N), dtype=eng.cdtype, device=dev) if form == "generic" else None

    def record(splits, fill):
        rec = torch.full((G * G + 1,), fill, dtype=torch.int64, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        edges = [0] + splits + [S]
        for a, b in zip(edges[:-1], edges[1:]):
            eng.rx(stream, y[a:], None, None, SEED, stats, S * (N + eng.cp), snr, True, None, a, b - a,
                   eng.valid_bits(S), cnt, z, 0, density=rec, density_params=(lo, inv_w, G),
                   density_subcarriers=(0, N))
        return cnt.cpu().numpy().tolist(), rec.cpu().numpy()

    cnt, rec = record([], 0)
    assert rec.sum() == S * N and cnt == [case["bit_errors"], case["symbol_errors"]]
    for splits in ([S // 2], [1, 70, S - 1]):
        cnt2, rec2 = record(splits, 0)
        assert cnt2 == cnt and np.array_equal(rec2, rec), splits
    cnt3, rec3 = record([S // 2], 1000)
    assert cnt3 == cnt and np.array_equal(rec3, rec + 1000)
    # an empty call is an empty call
    empty = torch.zeros(G * G + 1, dtype=torch.int64, device=dev)
    eng.rx(stream, y, None, None, SEED, stats, S * (N + eng.cp), snr, True, None, 0, 0, eng.valid_bits(S),
           torch.zeros(2, dtype=torch.int64, device=dev), None, 0, density=empty, density_params=(lo, inv_w, G),
           density_subcarriers=(0, N))
    assert not empty.cpu().numpy().any()


def test_a_bad_grid_is_refused_through_the_engine(gpu):
    case = PE.THROUGHPUT_CASES[0]
    eng, _ = throughput_engine(case)
    dev = eng.device()
    rec = torch.zeros(5, dtype=torch.int64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    y, stats = eng._y(2), E.new_stats(dev)
    for params, rng, reason in (((-2.0, 1.0, 129), (0, 4), "bins 129"), ((-2.0, 0.0, 2), (0, 4), "inv_w"),
                                ((-2.0, 1.0, 2), (0, case["N"] + 1), "n_fft = 1024")):
        with pytest.raises(Exception, match=reason):
            eng.rx(eng.stream(), y, None, None, SEED, stats, 2 * case["N"], 20.0, True, None, 0, 2, 2 * eng.bps, cnt,
                   None, 0, density=rec, density_params=params, density_subcarriers=rng)
    assert not rec.cpu().numpy().any() and not cnt.cpu().numpy().any()


# ---------------------------------------------------------------- 8. noise off
def test_noise_off_16qam_falls_on_sixteen_bins(gpu):
    N, M, S, G, L = 64, 16, 67, 31, 2.0
    lut = O.qam_lut(M)
    eng = LinkEngine(N, 0, np.array([1.0 + 0j]), B.EQ_NONE, [lut])
    res = eng.run(S, 20.0, seed=SEED, noise_on=False, density=G, density_extent=L)
    assert res.bit_errors == 0 and res.symbol_errors == 0
    d = res.density
    idx = P.tx_indices(P.lane_generators(SEED, np.arange(S), N), S, N, 4)
    want = np.zeros((G, G), np.int64)
    for i, c in enumerate(lut):
        cell, out = DE.bin_points(np.array([[c]]), G, L)
        assert out == 0
        want += cell * int(np.count_nonzero(idx == i))
    assert np.count_nonzero(want) == 16 and want.sum() == S * N
    assert np.count_nonzero(d.counts) == 16 and d.outside == 0
    assert np.array_equal(d.counts, want)

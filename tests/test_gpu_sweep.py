"""The one-pass SNR sweep receiver (ofdm_rx_sweep, LinkEngine.run_sweep, Simulation.run_sweep) on the
GPU: point k of a sweep is the run ``LinkEngine.run(n_sym, snr_k, seed=seed)`` -- the same bits, noise
words, sigma and per-sample arithmetic -- from one transmit.

Per point the counts are held to the oracle's decision brackets exactly as
test_gpu_philox_parity.check_error_counts holds a single run (its helpers are imported), in complex128
they equal the single-point run, and they do not depend on the order of the list, duplicates, the
batching, how a long list is split into launches or the rank count.  The shapes are the dispatch
matrix's (S = 32 * 4096 / N + 35: two workgroups and a partial last one): the complex128 bench shapes
take the throughput form of k_rx_sweep, everything else the generic one (zero padding's tail noise
samples, SC-OFDM, PSK, N < 64, complex64)."""

import functools
import json
import os

import numpy as np
import pytest
from conftest import CHANNELS, ROOT

import philox_streams as P
from ofdm_based_systems import _backend as B
from test_gpu_multirank import _launch
from test_gpu_philox_parity import bracket_width_bound, gpu_radius, setup, stat_width_bound, tx_deviation

pytestmark = pytest.mark.gpu

SEED = 77
F32, F64 = B.OFDM_F32, B.OFDM_F64
# id: N, M, channel, equaliser, OFDM symbols, SNR points (dB), variant
CASES = {
    "b": (1024, 64, "flat_fading", "NONE", 163, [14, 18, 20, 22, 23], {}),
    "c": (1024, 64, "severe_multipath", "MMSE", 163, [16, 20, 24, 26, 27], {}),
    "c-zf": (1024, 64, "Lin-Phoong_P1", "ZF", 163, [18, 24, 28, 30], {}),
    "e": (4096, 256, "Lin-Phoong_P1", "MMSE", 67, [25, 31, 35, 37], {}),
    "g1": (64, 4, "rayleigh_fading", "ZF", 2083, [6, 10, 14], {}),
    "g2": (128, 4, "Lin-Phoong_P2", "MMSE", 1059, [4, 8, 10], {"scheme": "PSK", "modulator": "SC", "prefix": "ZP"}),
    "g3": (256, 16, "severe_multipath", "MMSE", 547, [10, 16, 20], {}),
    "g4": (16, 16, "flat_fading", "NONE", 8227, [8, 14, 17], {}),
}
RUNS = [("b", F64), ("c", F64), ("c", F32), ("c-zf", F64), ("e", F64), ("g1", F64), ("g1", F32), ("g2", F64),
        ("g3", F64), ("g3", F32), ("g4", F64)]
RUNS_F64 = [r for r in RUNS if r[1] == F64]
INVARIANT = [("c", F64), ("c", F32), ("g1", F64)]


def _rid(r):
    return f"{r[0]}-{'f32' if r[1] == F32 else 'f64'}"


@functools.lru_cache(maxsize=None)
def engine(cid, prec):
    N, M, ch, eq, S, snrs, var = CASES[cid]
    return setup(N, M, ch, eq, prec, var)  # (engine, CIR, cp, keyword arguments for run_philox)


@functools.lru_cache(maxsize=None)
def swept(cid, prec):
    """The case's sweep, run once and shared (read only) by the tests."""
    S, snrs = CASES[cid][4], CASES[cid][5]
    return engine(cid, prec)[0].run_sweep(S, snrs, seed=SEED)


def counts(stats):
    return [(s.bit_errors, s.symbol_errors) for s in stats]


def record(s):
    return (s.bit_errors, s.symbol_errors, s.power_sum, s.x_power_sum, s.x_peak)


@pytest.mark.parametrize("cid,prec", RUNS, ids=[_rid(r) for r in RUNS])
def test_every_point_is_inside_the_oracle_brackets(gpu, cid, prec):
    N, M, ch, eq, S, snrs, _ = CASES[cid]
    eng, h, cp, var = engine(cid, prec)
    res = swept(cid, prec)
    assert len(res) == len(snrs)
    f32 = prec == F32
    dev = tx_deviation(eng, SEED, S) if f32 else None
    for snr, r in zip(snrs, res):
        ref = P.run_philox(SEED, S, N, M, h, cp, eq, float(snr), precision="f32" if f32 else "f64",
                           radius_fn=gpu_radius, power_sum=r.power_sum, stat_sigma=dev, **var)
        assert ref.bit_errors > 100, "SNR too high for a meaningful count"
        be_lo, be_hi, se_lo, se_hi = ref.bracket
        print(f"bracket {cid} {snr} dB: bits {r.bit_errors} in [{be_lo}, {be_hi}], symbols {r.symbol_errors} in "
              f"[{se_lo}, {se_hi}] (oracle {ref.bit_errors} / {ref.symbol_errors})")
        if f32:
            sb_lo, sb_hi, ss_lo, ss_hi = ref.stat_bracket
            print(f"stat bracket {cid} {snr} dB: bits in [{sb_lo}, {sb_hi}], symbols in [{ss_lo}, {ss_hi}]")
            assert sb_lo <= r.bit_errors <= sb_hi and ss_lo <= r.symbol_errors <= ss_hi, (snr, r, ref.stat_bracket)
            wst = stat_width_bound(ref.bit_errors)
            assert sb_hi - sb_lo <= wst and ss_hi - ss_lo <= wst, (snr, ref.stat_bracket, wst)
        assert be_lo <= ref.bit_errors <= be_hi and se_lo <= ref.symbol_errors <= se_hi
        assert be_lo <= r.bit_errors <= be_hi, (snr, r.bit_errors, ref.bracket)
        assert se_lo <= r.symbol_errors <= se_hi, (snr, r.symbol_errors, ref.bracket)
        wmax = bracket_width_bound(prec, var, ref.bit_errors)
        if wmax is not None:
            assert be_hi - be_lo <= wmax and se_hi - se_lo <= wmax, (snr, ref.bracket, wmax)
        assert r.power_sum == pytest.approx(ref.power_sum, rel=1e-5 if f32 else 1e-12)
        assert r.num_ofdm_symbols == S and r.samples == S * (N + cp)


@pytest.mark.parametrize("cid,prec", RUNS_F64, ids=[_rid(r) for r in RUNS_F64])
def test_complex128_points_equal_the_single_point_runs(gpu, cid, prec):
    S, snrs = CASES[cid][4], CASES[cid][5]
    eng = engine(cid, prec)[0]
    for snr, r in zip(snrs, swept(cid, prec)):
        assert record(r) == record(eng.run(S, float(snr), seed=SEED)), (cid, snr)


@pytest.mark.parametrize("cid,prec", INVARIANT, ids=[_rid(r) for r in INVARIANT])
def test_counts_do_not_depend_on_order_batching_or_splitting(gpu, cid, prec):
    S, snrs = CASES[cid][4], CASES[cid][5]
    eng = engine(cid, prec)[0]
    base = counts(swept(cid, prec))
    assert counts(eng.run_sweep(S, snrs[::-1], seed=SEED)) == base[::-1]
    dup = eng.run_sweep(S, [snrs[1], snrs[0], snrs[1]], seed=SEED)
    assert counts(dup) == [base[1], base[0], base[1]]
    one = eng.run_sweep(S, [snrs[2]], seed=SEED)
    assert counts(one) == [base[2]]
    if prec == F64:  # K = 1 equals run (complex64: another kernel's float32 rounding, held by the brackets)
        assert [record(s) for s in one] == [record(eng.run(S, float(snrs[2]), seed=SEED))]
    for batch in (1, S // 3 + 5):  # (the second does not divide S)
        assert S % batch != 0 or batch == 1
        got = eng.run_sweep(S, snrs, seed=SEED, batch=batch)
        assert [record(s) for s in got] == [record(s) for s in swept(cid, prec)], batch
    # a list longer than one launch takes: split into launches over the same y
    K = B.MAX_SWEEP_POINTS + 3
    long = eng.run_sweep(S, [snrs[k % len(snrs)] for k in range(K)], seed=SEED)
    assert counts(long) == [base[k % len(snrs)] for k in range(K)]


def test_refusals(gpu):
    import torch

    from ofdm_based_systems.engine import new_stats

    S = CASES["g1"][4]
    eng = engine("g1", F64)[0]
    y = torch.empty((S, eng.ystride), dtype=eng.cdtype, device="cuda")
    stats = new_stats("cuda")
    eng.tx(eng.stream(), None, SEED, 0, S, y, stats)
    cnt = torch.zeros((B.MAX_SWEEP_POINTS + 1, 2), dtype=torch.int64, device="cuda")
    args = (S * (64 + eng.cp),)
    with pytest.raises(ValueError, match="SNR points"):
        eng.rx_sweep(eng.stream(), y, SEED, stats, args[0], [], 0, S, S * eng.bps, cnt)
    with pytest.raises(ValueError, match="SNR points"):
        eng.rx_sweep(eng.stream(), y, SEED, stats, args[0], [10.0] * (B.MAX_SWEEP_POINTS + 1), 0, S, S * eng.bps, cnt)
    with pytest.raises(ValueError, match="not finite"):
        eng.rx_sweep(eng.stream(), y, SEED, stats, args[0], [10.0, float("nan")], 0, S, S * eng.bps, cnt)
    torch.cuda.synchronize()
    assert int(cnt.sum()) == 0  # refused before any launch
    eng.rx_sweep(eng.stream(), y, SEED, stats, args[0], [10.0], 0, 0, 0, cnt)  # n_sym = 0: an empty call
    torch.cuda.synchronize()
    assert int(cnt.sum()) == 0
    with pytest.raises(ValueError):
        eng.run_sweep(S, [], seed=SEED)
    with pytest.raises(ValueError):
        eng.run_sweep(S, [10.0, float("nan")], seed=SEED)
    # a 1024-QAM plan: the throughput stream carries at most 8 bits per subcarrier
    wide = setup(64, 1024, "flat_fading", "NONE", F64)[0]
    with pytest.raises(ValueError, match="8 bits"):
        wide.run_sweep(64, [30.0, 35.0], seed=SEED)
    yw = torch.empty((64, wide.ystride), dtype=wide.cdtype, device="cuda")
    with pytest.raises(ValueError, match="8 bits"):
        wide.rx_sweep(wide.stream(), yw, SEED, stats, 64 * 64, [30.0], 0, 64, 64 * wide.bps, cnt)


def _simulations(snrs, **over):
    from ofdm_based_systems.configuration.models import SimulationSettings
    from ofdm_based_systems.simulation.models import Simulation

    kw = dict(num_bands=64, signal_noise_ratios=snrs, channel_model_path=os.path.join(CHANNELS, "severe_multipath.npy"),
              channel_type="CUSTOM", num_symbols=64 * 200, constellation_order=16, constellation_type="QAM",
              equalization_method="MMSE", prefix_length_ratio=1.0, rng_mode="philox", seed=SEED)
    kw.update(over)
    sims = Simulation.create_from_simulation_settings(SimulationSettings(**kw))
    for s in sims:
        s.received_symbols_keep, s.make_plot, s.verbose = 0, False, False
    return Simulation, sims


def test_simulation_run_sweep_gives_run_s_result_dicts(gpu):
    Simulation, sims = _simulations([8.0, 12.0, 16.0])
    got = Simulation.run_sweep(sims)
    want = [s.run() for s in sims]
    assert len(got) == 3
    for g, w in zip(got, want):
        assert set(g) == set(w)
        assert w["bit_errors"] > 100
        for key in w:
            if key in ("transmission_time_ms", "constellation_plot"):
                continue
            if isinstance(w[key], np.ndarray):
                assert np.array_equal(g[key], w[key]), key
            else:
                assert g[key] == w[key], key
        assert g["received_symbols"].size == 0 and g["constellation_plot"] is None


def test_simulation_run_sweep_refusals(gpu):
    Simulation, sims = _simulations([8.0, 12.0], rng_mode="reference")
    with pytest.raises(ValueError, match="philox"):
        Simulation.run_sweep(sims)
    Simulation, sims = _simulations([8.0, 12.0])
    sims[1].constellation_order = 4
    with pytest.raises(ValueError, match="constellation_order"):
        Simulation.run_sweep(sims)
    Simulation, sims = _simulations([8.0, 12.0])
    for s in sims:
        s.received_symbols_keep = 8
    with pytest.raises(ValueError, match="received_symbols_keep"):
        Simulation.run_sweep(sims)
    Simulation, sims = _simulations([8.0, 12.0], adaptive_modulation_mode="CAPACITY_BASED")
    with pytest.raises(ValueError, match="FIXED"):
        Simulation.run_sweep(sims)


def test_two_ranks_give_the_one_rank_counts(gpu, tmp_path):
    """Two gloo ranks on device 0 (the scheme of test_gpu_multirank): case g3 with group=."""
    out = tmp_path / "sweep_ranks.json"
    N, M, ch, eq, S, snrs, _ = CASES["g3"]
    r = _launch([os.path.join(ROOT, "tests", "sweep_worker.py"), str(out), json.dumps([N, M, ch, eq, S, snrs, SEED])],
                timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(out.read_text())
    assert got["world"] == 2
    one = [[s.bit_errors, s.symbol_errors, s.power_sum.hex(), s.x_peak] for s in swept("g3", F64)]
    assert got["whole"] == one and got["batched"] == one

"""The fused link kernel (ofdm_link, k_link: transmit and receive in one kernel, y never leaving the
registers) on the GPU, on the config-(b) plan in complex128: N = 1024, 64-QAM, flat channel, no
equaliser.  A fused run must give exactly what the two-kernel path (``fused=False``: k_tx into a buffer,
then k_rx of that buffer) gives with the same seed -- the counts and every statistic, bit for bit: the
kernel recomputes the transmitter's samples with the transmitter's code and receives them with the
receiver's.  The ``fused=False`` legs keep k_rx<double, 10, 0, 6> exercised now that the default route of
this shape is the fused one."""

import functools

import pytest
import torch

from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import new_stats
from test_gpu_philox_parity import setup

pytestmark = pytest.mark.gpu

SEED = 77
FIELDS = ("bit_errors", "symbol_errors", "power_sum", "x_power_sum", "x_peak", "papr_db")
# 163 = 32 * 4096 / N + 35 (the dispatch matrix's shape): several workgroups of 12 symbols, a partial
# last one; 2 * 4096 + 35: more workgroups than two rounds of the resident ones, so workgroups loop
COUNTS = [1, 15, 16, 17, 163, 2 * 4096 + 35]


def record(s):
    return tuple(getattr(s, f) for f in FIELDS)


@functools.lru_cache(maxsize=None)
def engine():
    return setup(1024, 64, "flat_fading", "NONE", B.OFDM_F64)[0]


@functools.lru_cache(maxsize=None)
def forced(n_sym, snr, noise_on=True, seed=SEED):
    """The two-kernel run, computed once and shared (read only)."""
    return engine().run(n_sym, snr, seed=seed, noise_on=noise_on, fused=False)


def test_the_bench_plan_has_a_fused_form_and_takes_it_by_default(gpu):
    eng = engine()
    assert eng.has_fused
    ev = []
    eng.run(17, 20.0, seed=SEED, events=ev)
    assert [e[0] for e in ev] == ["ofdm_tx", "ofdm_link"] and [e[1] for e in ev] == [17, 17]
    ev = []
    eng.run(17, 20.0, seed=SEED, events=ev, fused=False)
    assert [e[0] for e in ev] == ["ofdm_tx", "ofdm_rx"]
    # a run of any size is one power pass and one link launch, whatever the budget and the batch say
    ev = []
    got = eng.run(163, 10.0, seed=SEED, events=ev, y_budget=4 * 1024 * 16, batch=5)
    assert [(e[0], e[1]) for e in ev] == [("ofdm_tx", 163), ("ofdm_link", 163)]
    assert record(got) == record(forced(163, 10.0))
    # a tap, a profile or caller streams keep the two-kernel path
    ev = []
    eng.run(17, 20.0, seed=SEED, events=ev, keep_symbols=2)
    assert [e[0] for e in ev] == ["ofdm_tx", "ofdm_rx"]


@pytest.mark.parametrize("n_sym", COUNTS)
def test_symbol_counts(gpu, n_sym):
    want = forced(n_sym, 10.0)
    got = engine().run(n_sym, 10.0, seed=SEED, fused=True)
    print(f"n_sym {n_sym}: fused {record(got)}, two kernels {record(want)}")
    assert want.bit_errors > 100 * min(n_sym, 2)  # (10 dB: ~1000 bit errors per symbol)
    assert record(got) == record(want)


@pytest.mark.parametrize("snr,noise_on", [(10.0, True), (24.0, True), (24.0, False)])
def test_snrs(gpu, snr, noise_on):
    want = forced(163, snr, noise_on)
    got = engine().run(163, snr, seed=SEED, noise_on=noise_on, fused=True)
    print(f"{snr} dB, noise {noise_on}: fused {record(got)}, two kernels {record(want)}")
    if not noise_on:
        assert (want.bit_errors, want.symbol_errors) == (0, 0)
    elif snr == 10.0:
        assert want.bit_errors > 1000
    assert record(got) == record(want)


def test_shard_offset(gpu):
    """A global run of 326 symbols as two ofdm_link calls, sym0 = 0 and 163, after one power pass."""
    eng = engine()
    dev, st = eng.device(), eng.stream()
    stats = new_stats(dev)
    eng.tx(st, None, SEED, 0, 326, None, stats)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    for sym0 in (0, 163):
        eng.link(st, SEED, stats, 326 * 1024, 10.0, True, sym0, 163, 326 * 1024 * 6, counters)
    one = torch.zeros(2, dtype=torch.int64, device=dev)
    eng.link(st, SEED, stats, 326 * 1024, 10.0, True, 0, 326, 326 * 1024 * 6, one)
    want = forced(326, 10.0)
    assert counters.tolist() == one.tolist() == [want.bit_errors, want.symbol_errors]
    assert float(stats[0]) == want.power_sum


@pytest.mark.parametrize("lanes", [1, 2])
def test_run_pipelined(gpu, lanes):
    eng = engine()
    seeds = [3, 4, 5]
    ev = []
    got = [p.result() for p in eng.run_pipelined(163, 14.0, seeds, lanes=lanes, events=ev)]
    assert sorted(e[0] for e in ev) == ["ofdm_link"] * 3 + ["ofdm_tx"] * 3
    want = [p.result() for p in eng.run_pipelined(163, 14.0, seeds, lanes=lanes, fused=False)]
    assert [record(g) for g in got] == [record(w) for w in want]
    assert [record(w) for w in want] == [record(forced(163, 14.0, True, s)) for s in seeds]
    assert all(w.bit_errors > 100 for w in want)


def _link_rc(eng, n_valid=None, n_sym=4):
    dev = eng.device()
    stats = new_stats(dev)
    stats[0] = 1.0
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    n_valid = n_sym * eng.bps if n_valid is None else n_valid
    rc = B.lib().ofdm_link(eng.plan.handle, eng.stream(), SEED, B.ptr(stats), n_sym * (eng.n_fft + eng.cp), 20.0, 1,
                           0, n_sym, n_valid, B.ptr(counters))
    torch.cuda.synchronize()
    return rc, B.lib().ofdm_last_error().decode(), counters.tolist()


def test_refusals(gpu):
    """No fused form: OFDM_E_INVALID naming the reason, nothing launched, never another path."""
    f32 = setup(1024, 64, "flat_fading", "NONE", B.OFDM_F32)[0]
    multipath = setup(1024, 64, "severe_multipath", "NONE", B.OFDM_F64)[0]
    for eng, word in ((f32, "complex64"), (multipath, "taps")):
        assert not eng.has_fused
        rc, msg, counters = _link_rc(eng)
        assert rc == -1 and "ofdm_link" in msg and word in msg and counters == [0, 0], (rc, msg)
        with pytest.raises(ValueError):
            eng.run(4, 20.0, seed=SEED, fused=True)
        with pytest.raises(ValueError):
            eng.run_pipelined(4, 20.0, [1, 2], fused=True)
        ev = []
        eng.run(4, 20.0, seed=SEED, events=ev)  # (and the default stays on the two kernels)
        assert [e[0] for e in ev] == ["ofdm_tx", "ofdm_rx"]
    eng = engine()
    rc, msg, counters = _link_rc(eng, n_valid=4 * eng.bps - 1)
    assert rc == -1 and "n_valid_bits" in msg and counters == [0, 0], (rc, msg)
    with pytest.raises(ValueError):
        eng.run(4, 20.0, seed=SEED, n_valid_bits=4 * eng.bps - 8, fused=True)
    ev = []
    eng.run(4, 20.0, seed=SEED, n_valid_bits=4 * eng.bps - 8, events=ev)
    assert [e[0] for e in ev] == ["ofdm_tx", "ofdm_rx"]
    assert _link_rc(eng)[0] == 0

"""The order and arguments of LinkEngine's kernel calls, without a GPU: run, run_sweep and
run_pipelined over the oracle's CPU test doubles (test_distributed_cpu.OracleEngine,
test_sweep_cpu.SweepEngine), with every tx / rx / rx_sweep call logged as
(name, sym0, n_sym, y is None, SNR points) and compared with the schedule written out here."""

import numpy as np
from conftest import channel

from ofdm_based_systems import _backend as B
from test_distributed_cpu import CASE
from test_sweep_cpu import SweepEngine

S = 10
SEEDS = [11, 12, 13]


class Logged(SweepEngine):
    """SweepEngine that logs its calls; rx also notes z_keep and whether ``profile=`` was passed (the
    oracle's rx takes no profile: the record stays zero)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.bits_per_subcarrier = np.full(self.n_fft, self.b, dtype=np.int64)
        self.log, self.seeds, self.z_keeps, self.profiled, self.sweep_y = [], [], [], [], []
        self._inner = False

    def tx(self, stream, bits_d, seed, sym0, n_sym, y, stats):
        self.log.append(("tx", sym0, n_sym, y is None, 0))
        self.seeds.append(seed)
        super().tx(stream, bits_d, seed, sym0, n_sym, y, stats)

    def rx(self, stream, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits_d, sym0, n_sym,
           n_valid, counters, z_out=None, z_keep=0, **kw):
        if not self._inner:  # (SweepEngine.rx_sweep calls rx once per point)
            assert set(kw) <= {"profile"} and (z_out is None) == (z_keep == 0)
            self.log.append(("rx", sym0, n_sym, y is None, 1))
            self.seeds.append(seed)
            self.z_keeps.append(z_keep)
            self.profiled.append("profile" in kw and kw["profile"] is not None)
        super().rx(stream, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits_d, sym0, n_sym,
                   n_valid, counters, z_out, z_keep)

    def rx_sweep(self, stream, y, seed, stats, total_samples, snr_dbs, sym0, n_sym, n_valid, counters):
        self.log.append(("rx_sweep", sym0, n_sym, y is None, len(snr_dbs)))
        self.sweep_y.append(y.data_ptr())
        self._inner = True
        try:
            super().rx_sweep(stream, y, seed, stats, total_samples, snr_dbs, sym0, n_sym, n_valid, counters)
        finally:
            self._inner = False


def make():
    h = channel(CASE["ch"])
    eng = Logged(CASE["N"], CASE["M"], h, len(h) - 1, CASE["eq"])
    for sd in SEEDS:
        eng.seed_streams(sd, S)
    return eng


def tx(sym0, n, power_pass=False):
    return ("tx", sym0, n, power_pass, 0)


def rx(sym0, n):
    return ("rx", sym0, n, False, 1)


def sw(sym0, n, k):
    return ("rx_sweep", sym0, n, False, k)


BATCHED = [tx(0, 10, True), tx(0, 4), rx(0, 4), tx(4, 4), rx(4, 4), tx(8, 2), rx(8, 2)]


def test_run_resident():
    eng = make()
    st = eng.run(S, CASE["snr"], seed=SEEDS[0])
    assert eng.log == [tx(0, 10), rx(0, 10)]
    assert eng.z_keeps == [0] and eng.profiled == [False]
    assert st.num_ofdm_symbols == S and st.bit_errors > 0 and st.profile is None


def test_run_batched():
    eng = make()
    whole = eng.run(S, CASE["snr"], seed=SEEDS[0])
    eng.log.clear()
    st = eng.run(S, CASE["snr"], seed=SEEDS[0], batch=4)
    assert eng.log == BATCHED
    assert (st.bit_errors, st.symbol_errors, st.power_sum) == (whole.bit_errors, whole.symbol_errors,
                                                               whole.power_sum)


def test_kept_symbols_come_from_the_first_batch_only():
    eng = make()
    st = eng.run(S, CASE["snr"], seed=SEEDS[0], keep_symbols=3, batch=4, noise_on=False)
    assert eng.log == BATCHED
    assert eng.z_keeps == [3, 0, 0]
    assert st.received.shape == (3 * CASE["N"],)


def test_profile_is_passed_only_when_asked_for():
    eng = make()
    st = eng.run(S, CASE["snr"], seed=SEEDS[0], profile=True, batch=4)
    assert eng.log == BATCHED and eng.profiled == [True, True, True]
    assert st.profile is not None and st.profile.n_symbols == S
    assert st.profile.bit_errors.shape == (CASE["N"],)
    eng.profiled.clear()
    assert eng.run(S, CASE["snr"], seed=SEEDS[0], batch=4).profile is None
    assert eng.profiled == [False, False, False]
    eng.profiled.clear()
    eng.run(S, CASE["snr"], seed=SEEDS[0], profile=True)
    eng.run(S, CASE["snr"], seed=SEEDS[0])
    assert eng.profiled == [True, False]


def test_sweep_resident_and_batched_split_a_long_list_over_the_same_y():
    eng = make()
    cap, K = B.MAX_SWEEP_POINTS, B.MAX_SWEEP_POINTS + 3
    snrs = [8.0 + 0.25 * k for k in range(K)]
    whole = eng.run_sweep(S, snrs, seed=SEEDS[0])
    assert eng.log == [tx(0, 10), sw(0, 10, cap), sw(0, 10, 3)]
    assert eng.sweep_y[0] == eng.sweep_y[1]
    eng.log.clear()
    eng.sweep_y.clear()
    got = eng.run_sweep(S, snrs, seed=SEEDS[0], batch=4)
    assert eng.log == [tx(0, 10, True), tx(0, 4), sw(0, 4, cap), sw(0, 4, 3), tx(4, 4), sw(4, 4, cap),
                       sw(4, 4, 3), tx(8, 2), sw(8, 2, cap), sw(8, 2, 3)]
    assert len(set(eng.sweep_y)) == 1  # one y buffer, refilled per batch
    assert len(got) == K and [(g.bit_errors, g.symbol_errors) for g in got] == [
        (w.bit_errors, w.symbol_errors) for w in whole]
    assert eng.z_keeps == [] and eng.profiled == []  # (no rx call of the schedule's own)


def test_pipelined_transmits_one_run_ahead():
    eng = make()
    out = [p.result() for p in eng.run_pipelined(S, CASE["snr"], SEEDS)]
    assert eng.log == [tx(0, 10), tx(0, 10), rx(0, 10), tx(0, 10), rx(0, 10), rx(0, 10)]
    assert eng.seeds == [11, 12, 11, 13, 12, 13]  # tx0, tx1, rx0, tx2, rx1, rx2
    assert eng.z_keeps == [0, 0, 0] and eng.profiled == [False, False, False]
    serial = [eng.run(S, CASE["snr"], seed=sd) for sd in SEEDS]
    assert [(o.bit_errors, o.symbol_errors, o.power_sum) for o in out] == [
        (s.bit_errors, s.symbol_errors, s.power_sum) for s in serial]


def test_pipelined_falls_back_to_batched_runs_under_a_small_budget():
    eng = make()
    # 8 symbols of y: below two 10-symbol shards, so each seed goes through run_async in 8-symbol batches
    pend = eng.run_pipelined(S, CASE["snr"], SEEDS, y_budget=8 * CASE["N"] * 16)
    assert eng.log == [tx(0, 10, True), tx(0, 8), rx(0, 8), tx(8, 2), rx(8, 2)] * 3
    assert eng.seeds == [11] * 5 + [12] * 5 + [13] * 5
    assert all(p.result().num_ofdm_symbols == S for p in pend)

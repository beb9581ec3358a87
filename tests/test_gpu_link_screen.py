"""The fused link's float32 screen (ofdm_link's automatic mode, ofdm_link_screen) on the GPU, on the
config-(b) plan: N = 1024, 64-QAM, flat channel, no equaliser, complex128.  A screened wave decides its
symbol in float32 when it can prove every decision is the complex128 one and redoes it in complex128
otherwise, so a run must give exactly what the two-kernel path (``fused=False``) gives -- the counts and
every statistic, bit for bit -- in automatic and in forced mode, whatever share is redone.  The screen
counts show the equality is not vacuous, and the margin test that the bound delta is one."""

import math

import numpy as np
import pytest
import torch

import link_screen_expect as X
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import new_stats
from test_gpu_link import SEED, engine, forced, record
from test_gpu_philox_parity import setup

pytestmark = pytest.mark.gpu

# 1: one wave; 12 / 13: a whole workgroup and one symbol more; 163: several workgroups and a partial
# last one; 2 * 4096 + 35: more workgroups than two rounds of the resident ones, so workgroups loop
COUNTS = [1, 12, 13, 163, 2 * 4096 + 35]
SNRS = [(10.0, True), (20.0, True), (24.0, True), (30.0, True), (24.0, False)]
MODES = {"auto": B.LINK_SCREEN_AUTO, "forced": B.LINK_SCREEN_FORCED, "off": B.LINK_SCREEN_OFF}
# forced at this SNR redoes about half of the symbols (81 of 163 with SEED)
MID_SNR = 21.0


class screened:
    """The shared engine in a screen mode, counting; put back as it was on exit."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        eng = engine()
        eng.screen_mode = MODES[self.mode]
        eng.screen_counts = torch.zeros(2, dtype=torch.int64, device=eng.device())
        return eng

    def __exit__(self, *exc):
        eng = engine()
        eng.screen_mode = None
        eng.screen_counts = None


def counts(mode, n_sym, snr, noise_on=True):
    with screened(mode) as eng:
        got = eng.run(n_sym, snr, seed=SEED, noise_on=noise_on, fused=True)
        return record(got), eng.screen_counts.tolist()


@pytest.mark.parametrize("snr,noise_on", SNRS)
@pytest.mark.parametrize("n_sym", COUNTS)
def test_exactly_the_two_kernel_run(gpu, n_sym, snr, noise_on):
    want = record(forced(n_sym, snr, noise_on))
    for mode in ("auto", "forced"):
        got, sc = counts(mode, n_sym, snr, noise_on)
        print(f"n_sym {n_sym}, {snr} dB, noise {noise_on}, {mode}: {got[:2]}, screened / redone {sc}")
        assert got == want, mode
    if noise_on and snr == 10.0:
        assert want[0] > 100 * min(n_sym, 2)


def test_screen_counts(gpu):
    n = 163
    # noise off: every point sits on its level, half a level from every boundary
    for mode in ("auto", "forced"):
        assert counts(mode, n, 24.0, False)[1] == [n, 0]
    # 10 dB: almost every symbol has a point near a boundary
    _, (scr, redo) = counts("forced", n, 10.0)
    print(f"forced, 10 dB: screened {scr}, redone {redo}")
    assert scr == n and redo >= n - 8
    # a mid SNR: both the float32 count and the redo serve a share of the symbols
    _, (scr, redo) = counts("forced", n, MID_SNR)
    print(f"forced, {MID_SNR} dB: screened {scr}, redone {redo}")
    assert scr == n and redo >= 0.1 * n and scr - redo >= 0.1 * n
    # the bench's point
    _, (scr, redo) = counts("auto", n, 24.0)
    print(f"auto, 24 dB: screened {scr}, redone {redo}")
    assert scr > 0.9 * n and redo < 0.1 * n
    # screen off: the mode, and the automatic rule at 10 dB
    assert counts("off", n, 24.0)[1] == [0, 0]
    assert counts("auto", n, 10.0)[1] == [0, 0]
    assert X.undecided(10.0) > X.MAX_UNDECIDED > X.undecided(24.0)


def test_a_bad_mode_is_refused(gpu):
    eng = engine()
    c = torch.zeros(2, dtype=torch.int64, device=eng.device())
    rc = B.lib().ofdm_link_screen(eng.plan.handle, eng.stream(), SEED, None, 0, 20.0, 0, 0, 0, 0, B.ptr(c), 3, None)
    assert rc == -1 and "ofdm_link_screen" in B.lib().ofdm_last_error().decode()


def test_shard_offset_forced(gpu):
    """A global run of 326 symbols as two forced-mode calls, sym0 = 0 and 163, after one power pass."""
    with screened("forced") as eng:
        dev, st = eng.device(), eng.stream()
        stats = new_stats(dev)
        eng.tx(st, None, SEED, 0, 326, None, stats)
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        for sym0 in (0, 163):
            eng.link(st, SEED, stats, 326 * 1024, MID_SNR, True, sym0, 163, 326 * 1024 * 6, counters)
        parts = eng.screen_counts.tolist()
        eng.screen_counts.zero_()
        one = torch.zeros(2, dtype=torch.int64, device=dev)
        eng.link(st, SEED, stats, 326 * 1024, MID_SNR, True, 0, 326, 326 * 1024 * 6, one)
        whole = eng.screen_counts.tolist()
    want = forced(326, MID_SNR)
    assert counters.tolist() == one.tolist() == [want.bit_errors, want.symbol_errors]
    # (a symbol's screen depends on the symbol alone)
    assert parts == whole and whole[0] == 326 and 0.1 * 326 <= whole[1] <= 0.9 * 326


@pytest.mark.parametrize("lanes", [1, 2])
def test_run_pipelined_forced(gpu, lanes):
    seeds = [3, 4, 5]
    with screened("forced") as eng:
        ev = []
        got = [p.result() for p in eng.run_pipelined(163, MID_SNR, seeds, lanes=lanes, events=ev)]
        sc = eng.screen_counts.tolist()
    assert sorted(e[0] for e in ev) == ["ofdm_link"] * 3 + ["ofdm_tx"] * 3
    assert [record(g) for g in got] == [record(forced(163, MID_SNR, True, s)) for s in seeds]
    assert sc[0] == 3 * 163 and 0.1 * sc[0] <= sc[1] <= 0.9 * sc[0]
    assert all(g.bit_errors > 100 for g in got)


def margin(snr, keep=64):
    """The same seed through a complex64 and a complex128 engine on the two kernels: over the kept
    symbols, the largest max_k |z32 - z64| / delta_sym, the largest |z32 - z64| and the range of delta_sym."""
    z = {}
    for prec in (B.OFDM_F32, B.OFDM_F64):
        eng = engine() if prec == B.OFDM_F64 else setup(1024, 64, "flat_fading", "NONE", prec)[0]
        got = eng.run(keep, snr, seed=SEED, keep_symbols=keep, fused=False)
        z[prec] = np.asarray(got.received).astype(np.complex128).reshape(keep, 1024)
    amax = math.sqrt(98 / 42)  # |h| = 1 times the 64-QAM corner at unit mean power
    err = np.abs(z[B.OFDM_F32] - z[B.OFDM_F64]).max(axis=1)
    delta = np.array([X.delta_sym(float(np.linalg.norm(row)), 1024, amax) for row in z[B.OFDM_F32]])
    return {"snr_db": snr, "symbols": keep, "max_ratio": float((err / delta).max()), "max_abs_err": float(err.max()),
            "min_delta_sym": float(delta.min()), "max_delta_sym": float(delta.max())}


@pytest.mark.parametrize("snr", [24.0, 10.0])
def test_margin_of_delta(gpu, snr):
    m = margin(snr)
    print(m)
    assert m["max_ratio"] <= 0.25

"""The fused link's noise screen (ofdm_link's automatic mode, ofdm_link_nscreen) on the GPU, on the
config-(b) plan: N = 1024, 64-QAM, flat channel, no equaliser, complex128.  A screened wave transforms
the symbol's noise alone in float32, adds the LUT point, and keeps its float32 decisions when it can
prove every one is the complex128 one; otherwise it redoes the symbol in complex128.  So a run must give
exactly what the two-kernel path (``fused=False``) gives -- the counts and every statistic, bit for bit --
by the default route and by the new entry point in automatic and forced mode, whatever share is redone.
The screen counts show the equality is not vacuous, and the margin test that the bound delta is one."""

import math

import numpy as np
import pytest
import torch

import link_nscreen_expect as NX
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import new_stats
from test_gpu_link import SEED, engine, forced, record
from test_gpu_philox_parity import setup

pytestmark = pytest.mark.gpu

# 1: one wave; 12 / 13: a whole workgroup and one symbol more; 163: several workgroups and a partial
# last one; 2 * 4096 + 35: more workgroups than two rounds of the resident ones, so workgroups loop
COUNTS = [1, 12, 13, 163, 2 * 4096 + 35]
SNRS = [(6.0, True), (10.0, True), (14.0, True), (18.0, True), (21.0, True), (24.0, True), (30.0, True), (24.0, False)]
MODES = {"auto": B.LINK_SCREEN_AUTO, "forced": B.LINK_SCREEN_FORCED, "off": B.LINK_SCREEN_OFF}
LOW_SNR = 10.0  # forced: the model redoes 0.41 of the symbols


class nscreened:
    """The shared engine on ofdm_link_nscreen in a mode, counting; put back as it was on exit."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        eng = engine()
        eng.nscreen_mode = MODES[self.mode]
        eng.nscreen_counts = torch.zeros(2, dtype=torch.int64, device=eng.device())
        return eng

    def __exit__(self, *exc):
        eng = engine()
        eng.nscreen_mode = None
        eng.nscreen_counts = None


def counts(mode, n_sym, snr, noise_on=True):
    with nscreened(mode) as eng:
        got = eng.run(n_sym, snr, seed=SEED, noise_on=noise_on, fused=True)
        return record(got), eng.nscreen_counts.tolist()


@pytest.mark.parametrize("snr,noise_on", SNRS)
@pytest.mark.parametrize("n_sym", COUNTS)
def test_exactly_the_two_kernel_run(gpu, n_sym, snr, noise_on):
    want = record(forced(n_sym, snr, noise_on))
    got = record(engine().run(n_sym, snr, seed=SEED, noise_on=noise_on, fused=True))
    print(f"n_sym {n_sym}, {snr} dB, noise {noise_on}, ofdm_link: {got[:2]}")
    assert got == want, "ofdm_link"
    for mode in ("auto", "forced"):
        got, sc = counts(mode, n_sym, snr, noise_on)
        print(f"n_sym {n_sym}, {snr} dB, noise {noise_on}, {mode}: {got[:2]}, screened / redone {sc}")
        assert got == want, mode
    if noise_on and snr in (6.0, 10.0):
        assert want[0] > 100 * n_sym


def test_screen_counts(gpu):
    n = 163
    # noise off: every point sits on its level, half a level from every boundary
    for mode in ("auto", "forced"):
        assert counts(mode, n, 24.0, False)[1] == [n, 0]
    # 10 dB: both the float32 count and the redo serve a share of the symbols (model: 0.41 redone)
    _, (scr, redo) = counts("forced", n, LOW_SNR)
    print(f"forced, {LOW_SNR} dB: screened {scr}, redone {redo}")
    assert scr == n and 0.2 * n <= redo <= 0.65 * n
    assert redo >= 0.1 * n and scr - redo >= 0.1 * n
    # the bench's point: a few symbols in a thousand (model: 0.33 %, about 27 of 8227)
    big = 2 * 4096 + 35
    _, (scr, redo) = counts("forced", big, 24.0)
    print(f"forced, 24 dB: screened {scr}, redone {redo}")
    assert scr == big and 0 < redo < 0.02 * big
    assert counts("off", n, 24.0)[1] == [0, 0]


def test_a_bad_mode_is_refused(gpu):
    eng = engine()
    c = torch.zeros(2, dtype=torch.int64, device=eng.device())
    for mode in (3, 7):
        rc = B.lib().ofdm_link_nscreen(eng.plan.handle, eng.stream(), SEED, None, 0, 20.0, 0, 0, 0, 0, B.ptr(c), mode, None)
        assert rc == -1 and "ofdm_link_nscreen" in B.lib().ofdm_last_error().decode()


def test_shard_offset_forced(gpu):
    """A global run of 326 symbols as two forced-mode calls, sym0 = 0 and 163, after one power pass."""
    with nscreened("forced") as eng:
        dev, st = eng.device(), eng.stream()
        stats = new_stats(dev)
        eng.tx(st, None, SEED, 0, 326, None, stats)
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        for sym0 in (0, 163):
            eng.link(st, SEED, stats, 326 * 1024, LOW_SNR, True, sym0, 163, 326 * 1024 * 6, counters)
        parts = eng.nscreen_counts.tolist()
        eng.nscreen_counts.zero_()
        one = torch.zeros(2, dtype=torch.int64, device=dev)
        eng.link(st, SEED, stats, 326 * 1024, LOW_SNR, True, 0, 326, 326 * 1024 * 6, one)
        whole = eng.nscreen_counts.tolist()
    want = forced(326, LOW_SNR)
    assert counters.tolist() == one.tolist() == [want.bit_errors, want.symbol_errors]
    # (a symbol's screen depends on the symbol alone)
    assert parts == whole and whole[0] == 326 and 0.1 * 326 <= whole[1] <= 0.9 * 326


@pytest.mark.parametrize("lanes", [1, 2])
def test_run_pipelined_forced(gpu, lanes):
    seeds = [3, 4, 5]
    with nscreened("forced") as eng:
        ev = []
        got = [p.result() for p in eng.run_pipelined(163, LOW_SNR, seeds, lanes=lanes, events=ev)]
        sc = eng.nscreen_counts.tolist()
    assert sorted(e[0] for e in ev) == ["ofdm_link"] * 3 + ["ofdm_tx"] * 3
    assert [record(g) for g in got] == [record(forced(163, LOW_SNR, True, s)) for s in seeds]
    assert sc[0] == 3 * 163 and 0.1 * sc[0] <= sc[1] <= 0.9 * sc[0]
    assert all(g.bit_errors > 100 for g in got)


def margin(snr, keep=64):
    """The same seed through a complex64 and a complex128 engine on the two kernels: over the kept
    symbols, the largest max_k |z32 - z64| / delta_sym, the largest |z32 - z64| and the range of delta_sym
    (||z32||_2 standing for ||ghat||_2: link_nscreen_expect.delta_sym)."""
    z = {}
    for prec in (B.OFDM_F32, B.OFDM_F64):
        eng = engine() if prec == B.OFDM_F64 else setup(1024, 64, "flat_fading", "NONE", prec)[0]
        got = eng.run(keep, snr, seed=SEED, keep_symbols=keep, fused=False)
        z[prec] = np.asarray(got.received).astype(np.complex128).reshape(keep, 1024)
    amax = math.sqrt(98 / 42)  # |h| = 1 times the 64-QAM corner at unit mean power
    err = np.abs(z[B.OFDM_F32] - z[B.OFDM_F64]).max(axis=1)
    delta = np.array([NX.delta_sym(float(np.linalg.norm(row)), amax) for row in z[B.OFDM_F32]])
    return {"snr_db": snr, "symbols": keep, "max_ratio": float((err / delta).max()), "max_abs_err": float(err.max()),
            "min_delta_sym": float(delta.min()), "max_delta_sym": float(delta.max())}


def test_margin_of_delta(gpu):
    """-20 dB: the received spectrum is almost only transformed noise, what the noise screen's float32
    arithmetic handles (the float32 kernels here also carry the signal through two transforms, so the
    distance measured is no smaller than the screen's)."""
    m = margin(-20.0)
    print(m)
    assert m["max_ratio"] <= 0.25

"""The fused link's sparse slicer (ofdm_link's automatic mode, ofdm_link_sparse) on the GPU, on the
config-(b) plan: N = 1024, 64-QAM, flat channel, no equaliser, complex128.  The kernel is the noise screen
up to the symbol's bound; it then slices only the quads in which some component of the transformed noise
exceeds a threshold T, chosen so that a skipped quad provably holds the transmitted levels inside the
screen's margin.  So a run must give exactly what the two-kernel path (``fused=False``) gives -- the counts
and every statistic, bit for bit -- by the default route and by the new entry point in automatic and forced
mode, and the screen's own counts must be the noise screen's.  The quad counts show that quads are in fact
skipped, in the share the model predicts."""

import pytest
import torch

import link_sparse_expect as SX
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import new_stats
from test_gpu_link import SEED, engine, forced, record
from test_gpu_link_nscreen import counts as nscreen_counts

pytestmark = pytest.mark.gpu

# 1: one wave; 12 / 13: a whole workgroup and one symbol more; 163: several workgroups and a partial
# last one; 2 * 4096 + 35: more workgroups than two rounds of the resident ones, so workgroups loop
COUNTS = [1, 12, 13, 163, 2 * 4096 + 35]
# 6 dB: the screen is off in automatic mode; 14: on, every quad sliced; 21: the last rung without the test;
# 24: the bench's point, the test on; 30: hardly a quad sliced; noise off: none
SNRS = [(6.0, True), (14.0, True), (21.0, True), (24.0, True), (30.0, True), (24.0, False)]
MODES = {"auto": B.LINK_SCREEN_AUTO, "forced": B.LINK_SCREEN_FORCED, "off": B.LINK_SCREEN_OFF}
BIG = 2 * 4096 + 35


class sparse:
    """The shared engine on ofdm_link_sparse in a mode, counting; put back as it was on exit."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        eng = engine()
        eng.sparse_mode = MODES[self.mode]
        eng.sparse_counts = torch.zeros(4, dtype=torch.int64, device=eng.device())
        return eng

    def __exit__(self, *exc):
        eng = engine()
        eng.sparse_mode = None
        eng.sparse_counts = None


def counts(mode, n_sym, snr, noise_on=True):
    with sparse(mode) as eng:
        got = eng.run(n_sym, snr, seed=SEED, noise_on=noise_on, fused=True)
        return record(got), eng.sparse_counts.tolist()


@pytest.mark.parametrize("snr,noise_on", SNRS)
@pytest.mark.parametrize("n_sym", COUNTS)
def test_exactly_the_two_kernel_run(gpu, n_sym, snr, noise_on):
    want = record(forced(n_sym, snr, noise_on))
    got = record(engine().run(n_sym, snr, seed=SEED, noise_on=noise_on, fused=True))
    print(f"n_sym {n_sym}, {snr} dB, noise {noise_on}, ofdm_link: {got[:2]}")
    assert got == want, "ofdm_link"
    for mode in ("auto", "forced"):
        got, sc = counts(mode, n_sym, snr, noise_on)
        print(f"n_sym {n_sym}, {snr} dB, noise {noise_on}, {mode}: {got[:2]}, "
              f"screened / redone / quads tested / sliced {sc}")
        assert got == want, mode
        if mode == "forced":
            # the symbols screened and redone are the noise screen's, on the same inputs
            assert sc[:2] == nscreen_counts("forced", n_sym, snr, noise_on)[1]
            assert sc[2] == 4 * n_sym and 0 <= sc[3] <= sc[2]
    if noise_on and snr == 6.0:
        assert want[0] > 100 * n_sym


def test_quad_counts(gpu):
    n = 163
    # noise off: the transform is never run, every component is 0: four quads a symbol tested, none sliced
    for mode in ("auto", "forced"):
        assert counts(mode, n, 24.0, False)[1] == [n, 0, 4 * n, 0]
    # 6 dB: hardly a quad without a component over T
    _, (scr, redo, tested, sliced) = counts("forced", n, 6.0)
    print(f"forced, 6 dB: screened {scr}, redone {redo}, tested {tested}, sliced {sliced}")
    assert scr == n and tested == 4 * n and sliced >= 0.99 * tested
    # the bench's point: the model gives 0.243 of the quads, the binomial deviation over 32 908 is 0.0024
    assert 0.23 < SX.sliced_share(24.0) < 0.26
    _, (scr, redo, tested, sliced) = counts("forced", BIG, 24.0)
    print(f"forced, 24 dB: screened {scr}, redone {redo}, tested {tested}, sliced {sliced}: {sliced / tested:.4f} "
          f"(model {SX.sliced_share(24.0):.4f})")
    assert scr == BIG and tested == 4 * BIG
    assert 0.20 <= sliced / tested <= 0.29
    # automatic: the test on at 24 dB (the same counts), off at 21 dB (nothing tested), as the rule says
    assert SX.sparse_rule(24.0) and not SX.sparse_rule(21.0)
    assert counts("auto", BIG, 24.0)[1] == [scr, redo, tested, sliced]
    assert counts("auto", n, 21.0)[1][2:] == [0, 0]
    # off: the noise screen itself, and nothing counted
    assert counts("off", n, 24.0) == (record(forced(n, 24.0)), [0, 0, 0, 0])


def test_a_bad_mode_is_refused(gpu):
    eng = engine()
    c = torch.zeros(2, dtype=torch.int64, device=eng.device())
    for mode in (3, 7):
        rc = B.lib().ofdm_link_sparse(eng.plan.handle, eng.stream(), SEED, None, 0, 20.0, 0, 0, 0, 0, B.ptr(c), mode, None)
        assert rc == -1 and "ofdm_link_sparse" in B.lib().ofdm_last_error().decode()


def test_shard_offset_forced(gpu):
    """A global run of 326 symbols as two forced-mode calls, sym0 = 0 and 163, after one power pass."""
    snr = 24.0
    with sparse("forced") as eng:
        dev, st = eng.device(), eng.stream()
        stats = new_stats(dev)
        eng.tx(st, None, SEED, 0, 326, None, stats)
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        for sym0 in (0, 163):
            eng.link(st, SEED, stats, 326 * 1024, snr, True, sym0, 163, 326 * 1024 * 6, counters)
        parts = eng.sparse_counts.tolist()
        eng.sparse_counts.zero_()
        one = torch.zeros(2, dtype=torch.int64, device=dev)
        eng.link(st, SEED, stats, 326 * 1024, snr, True, 0, 326, 326 * 1024 * 6, one)
        whole = eng.sparse_counts.tolist()
    want = forced(326, snr)
    assert counters.tolist() == one.tolist() == [want.bit_errors, want.symbol_errors]
    # (a symbol's screen and its quads depend on the symbol alone)
    print(f"two calls {parts}, one call {whole}")
    assert parts == whole and whole[0] == 326 and whole[2] == 4 * 326 and 0 < whole[3] < whole[2]

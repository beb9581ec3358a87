"""The sparse link kernel's trimmed screen on the GPU (config-(b) plan: N = 1024, 64-QAM, flat, complex128):
the wave sum of the norm taken in registers (DPP and lane swaps, a pairing of its own) and the quad test's
largest modulus taken with max3 on |.| operands.  Neither may move a count: every run equals the two-kernel
path (``fused=False``) in all six statistics, bit for bit, and the symbols screened and redone equal the
noise screen's, which shares the norm's text.  The symbol counts sit around the workgroup's 12 symbols and
the multiples of 16 and 64 a wider workgroup or a per-symbol record would have as edges."""

import pytest
import torch

from ofdm_based_systems.engine import new_stats
from test_gpu_link import SEED, engine, forced, record
from test_gpu_link_nscreen import counts as nscreen_counts
from test_gpu_link_sparse import BIG, counts, sparse

pytestmark = pytest.mark.gpu

COUNTS = [1, 15, 16, 17, 63, 64, 65, 163, BIG]


@pytest.mark.parametrize("n_sym", COUNTS)
def test_forced_at_6_db(gpu, n_sym):
    """About half of the symbols undecided and redone in complex128 (0.53 measured), hardly a quad skipped."""
    want = record(forced(n_sym, 6.0))
    got, sc = counts("forced", n_sym, 6.0)
    print(f"n_sym {n_sym}, forced, 6 dB: {got[:2]}, screened / redone / tested / sliced {sc}")
    assert got == want
    assert sc[:2] == nscreen_counts("forced", n_sym, 6.0)[1]
    assert sc[0] == n_sym and sc[2] == 4 * n_sym
    if n_sym == BIG:
        assert sc[1] >= 0.4 * n_sym
    assert want[0] > 100 * n_sym


@pytest.mark.parametrize("n_sym", COUNTS)
def test_automatic_at_24_db(gpu, n_sym):
    """The bench's point by the default route and by the entry point that counts."""
    want = record(forced(n_sym, 24.0))
    assert record(engine().run(n_sym, 24.0, seed=SEED, fused=True)) == want
    got, sc = counts("auto", n_sym, 24.0)
    print(f"n_sym {n_sym}, automatic, 24 dB: {got[:2]}, screened / redone / tested / sliced {sc}")
    assert got == want
    assert sc[:2] == nscreen_counts("auto", n_sym, 24.0)[1]
    assert sc[0] == n_sym and sc[2] == 4 * n_sym and sc[3] <= sc[2]
    if n_sym == BIG:
        assert sc[1] >= 1 and want[0] > 0


@pytest.mark.parametrize("n_sym", COUNTS)
def test_forced_with_noise_off(gpu, n_sym):
    """No transform, a norm of 0, every component 0: nothing sliced, nothing redone, no error."""
    want = record(forced(n_sym, 24.0, False))
    got, sc = counts("forced", n_sym, 24.0, False)
    assert got == want and got[:2] == (0, 0)
    assert sc == [n_sym, 0, 4 * n_sym, 0]


def test_shards(gpu):
    """326 symbols as two calls, sym0 = 0 and 163, after one power pass, against one call."""
    snr = 24.0
    eng = engine()
    dev, st = eng.device(), eng.stream()
    stats = new_stats(dev)
    eng.tx(st, None, SEED, 0, 326, None, stats)
    two = torch.zeros(2, dtype=torch.int64, device=dev)
    for sym0 in (0, 163):
        eng.link(st, SEED, stats, 326 * 1024, snr, True, sym0, 163, 326 * 1024 * 6, two)
    one = torch.zeros(2, dtype=torch.int64, device=dev)
    eng.link(st, SEED, stats, 326 * 1024, snr, True, 0, 326, 326 * 1024 * 6, one)
    want = forced(326, snr)
    assert two.tolist() == one.tolist() == [want.bit_errors, want.symbol_errors]


def test_a_run_leaves_nothing_behind(gpu):
    """A long forced run at 6 dB, then a short one at 24 dB on the same engine and stream."""
    with sparse("forced") as eng:
        assert record(eng.run(BIG, 6.0, seed=SEED, fused=True)) == record(forced(BIG, 6.0))
    got = record(engine().run(17, 24.0, seed=SEED, fused=True))
    assert got == record(forced(17, 24.0))


def test_lanes(gpu):
    eng = engine()
    seeds = [3, 4, 5]
    got = [record(p.result()) for p in eng.run_pipelined(163, 14.0, seeds, lanes=2)]
    serial = [record(eng.run(163, 14.0, seed=s, fused=True)) for s in seeds]
    assert got == serial == [record(forced(163, 14.0, True, s)) for s in seeds]

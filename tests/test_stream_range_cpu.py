"""The oracle's symbol offset (philox_streams.run_philox(sym0=..., total_samples=...)) without a GPU.

tests/test_gpu_stream_range.py holds the kernels to the oracle at symbol indices beyond 2^31, 2^32 and
2^40 and at seeds above 2^32; that is worth as much as the oracle's own offset is right.  Checked here:

* tiling: symbols [a, a + S) asked for with sym0 = a are rows [a, a + S) of the run [0, a + S) -- the
  indices and the stored channel samples (the predecessor's tail through a multipath channel among
  them) noise-free, and with noise the counts of [0, a) and [a, a + S), given the long run's power and
  sample count, add up to the long run's;
* the adaptive plans' "trailing partial byte" is that of the stream [0, sym0 + S);
* distinct streams: symbol 2^32 + j is not symbol j, and a seed is not its low word -- the Philox
  known-answer vectors (tests/test_oracle_philox.py) pin the block function on all six input words, this
  pins that lane_generators feeds the upper halves into it;
* the default (sym0 = 0) is what it was;
* a seed of -1 and of 2^64 - 1 reach an entry point of the C ABI as the same uint64.
"""

import ctypes

import numpy as np
import pytest
from conftest import channel

import clip_expect as CX
import density_expect as DE
import philox_streams as P
from ofdm_based_systems import _backend as B

SEED = 0x9E3779B97F4A7C15
N, M, S = 64, 16, 4
CHANNELS = {"one_tap": lambda: np.array([1.0 + 0j]), "multipath": lambda: channel("severe_multipath")}


def case(ch, prefix):
    h = CHANNELS[ch]()
    cp = max(len(h) - 1, 4)  # (a guard on the one-tap channel too: the prefix geometry is under test)
    return h, cp, dict(prefix=prefix, eq="NONE" if len(h) == 1 else "MMSE")


@pytest.mark.parametrize("prefix", ["CP", "ZP"])
@pytest.mark.parametrize("ch", sorted(CHANNELS))
@pytest.mark.parametrize("a", [1, 5])
def test_an_offset_run_is_the_rows_of_the_long_run(a, ch, prefix):
    h, cp, kw = case(ch, prefix)
    snr = 12.0
    long_ = P.run_philox(SEED, a + S, N, M, h, cp, kw["eq"], snr, noise_on=False, prefix=prefix)
    part = P.run_philox(SEED, S, N, M, h, cp, kw["eq"], snr, noise_on=False, prefix=prefix, sym0=a)
    assert part.idx.shape == (S, N) and np.array_equal(part.idx, long_.idx[a:])
    # the same taps times the same samples, summed in the same order: the rows are equal, not close
    assert part.y.shape == long_.y[a:].shape and np.array_equal(part.y, long_.y[a:])
    head = P.run_philox(SEED, a, N, M, h, cp, kw["eq"], snr, noise_on=False, prefix=prefix)
    assert part.power_sum + head.power_sum == pytest.approx(long_.power_sum, rel=1e-14)
    assert part.x_power_sum + head.x_power_sum == pytest.approx(long_.x_power_sum, rel=1e-14)
    assert max(part.x_peak, head.x_peak) == long_.x_peak
    # with noise: the pieces of the stream, given the stream's power and length, add up to it
    total = (a + S) * (N + cp)
    noisy = P.run_philox(SEED, a + S, N, M, h, cp, kw["eq"], snr, prefix=prefix, precision="f64")
    assert noisy.bit_errors > 20, "SNR too high for a meaningful count"
    pieces = [P.run_philox(SEED, n, N, M, h, cp, kw["eq"], snr, prefix=prefix, precision="f64", sym0=s0,
                           power_sum=noisy.power_sum, total_samples=total) for s0, n in ((0, a), (a, S))]
    assert sum(p.bit_errors for p in pieces) == noisy.bit_errors
    assert sum(p.symbol_errors for p in pieces) == noisy.symbol_errors
    assert np.array_equal(pieces[1].z, noisy.z[a:]) and np.array_equal(pieces[1].delta, noisy.delta[a:])
    assert tuple(sum(p.bracket[i] for p in pieces) for i in range(4)) == noisy.bracket
    # without total_samples a piece takes its own length: another sigma, other points
    own = P.run_philox(SEED, S, N, M, h, cp, kw["eq"], snr, prefix=prefix, sym0=a, power_sum=noisy.power_sum)
    assert not np.array_equal(own.z, pieces[1].z)


def test_the_first_symbol_of_an_offset_run_carries_its_predecessors_tail():
    h = channel("severe_multipath")
    cp = len(h) - 1
    a = 3
    long_ = P.run_philox(SEED, a + 1, N, M, h, 0, "MMSE", 20.0, noise_on=False)   # no prefix: the tail is kept
    part = P.run_philox(SEED, 1, N, M, h, 0, "MMSE", 20.0, noise_on=False, sym0=a)
    assert np.array_equal(part.y, long_.y[a:])
    # the same symbol's indices at the head of a stream: the same bits, another first row
    gen = P.lane_generators(SEED, np.array([a]), N)
    assert np.array_equal(P.tx_indices(gen, 1, N, 4), part.idx)
    x = np.fft.ifft(P.O.qam_lut(M)[part.idx], axis=1, norm="ortho")
    head_only = P.O.channel_conv(x.ravel(), h)
    assert np.max(np.abs(head_only[:cp] - part.y[0, :cp])) > 1e-3
    assert np.array_equal(head_only[cp:], part.y[0, cp:])


def test_clipped_and_density_restatements_take_the_same_offset():
    h = channel("severe_multipath")
    cp, a = len(h) - 1, 5
    a2 = CX.threshold(2.0, N, [P.O.qam_lut(M)])
    long_ = CX.run_clipped(SEED, a + S, N, M, h, cp, "MMSE", 14.0, a2, noise_on=False)
    part = CX.run_clipped(SEED, S, N, M, h, cp, "MMSE", 14.0, a2, noise_on=False, sym0=a)
    assert long_.clipped > 0 and np.array_equal(part.y, long_.y[a:]) and np.array_equal(part.p, long_.p[a:])
    assert part.clipped == int(np.count_nonzero(long_.p[a:] > a2)) and part.samples == S * N
    z, delta, idx = DE.philox_points(SEED, S, N, M, h, cp, "MMSE", 14.0, sym0=a)
    ref = P.run_philox(SEED, S, N, M, h, cp, "MMSE", 14.0, precision="f64", sym0=a)
    assert np.array_equal(z, ref.z) and np.array_equal(delta, ref.delta) and np.array_equal(idx, ref.idx)
    # sym0 = 0: philox_points' own statement and run_philox's points are the same numbers
    z0, d0, i0 = DE.philox_points(SEED, S, N, M, h, cp, "MMSE", 14.0)
    ref0 = P.run_philox(SEED, S, N, M, h, cp, "MMSE", 14.0, precision="f64")
    assert np.array_equal(z0, ref0.z) and np.array_equal(d0, ref0.delta) and np.array_equal(i0, ref0.idx)


@pytest.mark.parametrize("a", [1, 5, (1 << 32) - 3, (1 << 40) + 5])
def test_the_adaptive_partial_byte_is_that_of_the_whole_stream(a):
    """adaptive_counts at an offset: positions (sym0 + s) tot + off_k + j against the whole bytes of
    [0, sym0 + S) -- restated here bit by bit with Python integers."""
    rng = np.random.default_rng(3)
    bk = np.array([2, 0, 3, 4, 1, 0, 6, 1], np.int64)     # 17 bits per symbol: byte boundaries wander
    tot, Sx = int(bk.sum()), 5
    diff = rng.integers(0, 64, size=(Sx, len(bk))) & ((1 << bk) - 1)[None, :]
    valid = ((a + Sx) * tot // 8) * 8
    want = 0
    for s in range(Sx):
        pos = (a + s) * tot
        for k, b in enumerate(bk):
            for j in range(int(b)):
                if (int(diff[s, k]) >> (int(b) - 1 - j)) & 1 and pos < valid:
                    want += 1
                pos += 1
    be, se = P.adaptive_counts(diff.astype(np.int64), bk, Sx, a)
    assert (be, se) == (want, int(np.count_nonzero(diff[:, bk > 0])))
    all_bits = sum(int(v).bit_count() for v in diff.ravel())
    assert all_bits - be <= ((a + Sx) * tot) % 8


def test_adaptive_run_at_an_offset_against_the_long_run():
    h = channel("Lin-Phoong_P1")
    cp, a, snr = len(h) - 1, 5, 12.0
    orders, _, _ = P.O.adaptive_orders(N, h, 18.0, 1e-3, True)
    total = (a + S) * (N + cp)
    long_ = P.run_philox(SEED, a + S, N, 0, h, cp, "MMSE", snr, orders=orders)
    part = P.run_philox(SEED, S, N, 0, h, cp, "MMSE", snr, orders=orders, sym0=a, power_sum=long_.power_sum,
                        total_samples=total)
    assert np.array_equal(part.idx, long_.idx[a:]) and np.array_equal(part.z, long_.z[a:])
    # the head's count with every bit of it valid (its own partial byte is inside the long stream)
    bk = np.array([int(np.log2(o)) if o > 0 else 0 for o in orders], np.int64)
    ridx = np.zeros((a, N), np.int64)
    for o in np.unique(orders[orders > 0]):
        cols = np.flatnonzero(orders == o)
        ridx[:, cols] = P.O.nn_demap(long_.z[:a, cols].ravel(), P.O.qam_lut(int(o))).reshape(a, len(cols))
    head_bits = sum(int(v).bit_count() for v in (ridx ^ long_.idx[:a]).ravel())
    assert long_.bit_errors > 10 and part.bit_errors + head_bits == long_.bit_errors


def test_symbols_and_seeds_that_differ_above_bit_31_are_other_streams():
    for j in (0, 1, (1 << 32) - 3):
        lo = P.run_philox(SEED, 3, N, M, np.array([1.0 + 0j]), 0, "NONE", 20.0, noise_on=False, sym0=j)
        hi = P.run_philox(SEED, 3, N, M, np.array([1.0 + 0j]), 0, "NONE", 20.0, noise_on=False, sym0=(1 << 32) + j)
        # 192 4-bit indices: equal by chance with probability 2^-768; at least a third differ
        assert np.count_nonzero(lo.idx != hi.idx) > lo.idx.size // 3
    for seed in (SEED, 7 + (1 << 32)):
        full = P.run_philox(seed, 3, N, M, np.array([1.0 + 0j]), 0, "NONE", 20.0, sym0=2)
        low = P.run_philox(seed & 0xFFFFFFFF, 3, N, M, np.array([1.0 + 0j]), 0, "NONE", 20.0, sym0=2)
        assert np.count_nonzero(full.idx != low.idx) > full.idx.size // 3
        assert not np.array_equal(full.z, low.z)
    # the words themselves: the counter's third word and the key's second reach the block function
    g = P.lane_generators(SEED, np.array([(1 << 40) + 5]), N)
    p = P.philox4x32_10(np.arange(4), np.full(4, 5), np.full(4, 1 << 8), np.full(4, P.K_LANE), SEED & 0xFFFFFFFF, SEED >> 32)
    assert np.array_equal(g.payload[:, 0], p[2]) and np.array_equal(g.payload[:, 1], p[3])


def test_the_default_is_symbol_zero_of_a_stream_of_its_own_length():
    h = channel("severe_multipath")
    cp = len(h) - 1
    for kw in (dict(), dict(prefix="ZP"), dict(modulator="SC")):
        a = P.run_philox(SEED, S, N, M, h, cp, "MMSE", 14.0, precision="f64", **kw)
        b = P.run_philox(SEED, S, N, M, h, cp, "MMSE", 14.0, precision="f64", sym0=0, total_samples=S * (N + cp), **kw)
        assert (a.bit_errors, a.symbol_errors, a.power_sum, a.x_power_sum, a.x_peak, a.bracket) == \
               (b.bit_errors, b.symbol_errors, b.power_sum, b.x_power_sum, b.x_peak, b.bracket)
        assert np.array_equal(a.idx, b.idx) and np.array_equal(a.y, b.y) and np.array_equal(a.z, b.z)
        # and the restatement before the offset existed, written out: generators of arange(S), no predecessor
        gen = P.lane_generators(SEED, np.arange(S), N)
        assert np.array_equal(P.tx_indices(gen, S, N, 4), a.idx)


def test_a_negative_seed_and_its_twos_complement_are_one_seed_at_the_abi():
    """engine.LinkEngine hands int(seed) to ctypes, whose c_uint64 wraps: -1 and 2^64 - 1 arrive as the
    same word.  The double is a C callback with ofdm_link's bound signature (tests/test_link_cpu.py
    asserts that signature against the header), which records the seed it receives."""
    res, args = B.SIGNATURES["ofdm_link"]
    assert args[2] is ctypes.c_uint64
    seen = []

    def double(plan, stream, seed, *rest):
        seen.append(seed)
        return 0

    fn = ctypes.CFUNCTYPE(res, *args)(double)
    for seed in (-1, (1 << 64) - 1, SEED, SEED - (1 << 64)):
        assert fn(None, None, int(seed), None, 0, 20.0, 1, 0, 0, 0, None) == 0
    assert seen == [(1 << 64) - 1] * 2 + [SEED] * 2
    a = P.lane_generators(-1, np.arange(2), N).payload
    assert np.array_equal(a, P.lane_generators((1 << 64) - 1, np.arange(2), N).payload)

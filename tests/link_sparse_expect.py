"""The fused link's sparse slicer (csrc/ofdm_link_inst.hpp) restated: the threshold T
under which a quad of the transformed noise is skipped, the roundings eps that T keeps clear of, the
automatic mode's rule, and a numpy model on the noise screen's own model (link_nscreen_expect.model).

Units as tests/link_nscreen_expect.py where a function says so; the model works on the kernel's
unnormalised spectrum."""

import math

import numpy as np

import link_nscreen_expect as NX

U = NX.U
MAX_PER_QUAD = 2.0  # kSparseMaxPerQuad
LANES, QUAD_COMPONENTS = 64, 8


def eps_terms(side=8):
    """What eps must cover, in units of u of a level: the final add fl(N l32 + ghat) (a coordinate of at most
    side / 2 levels from the offset), the slicer's first FMA (a coordinate of at most side - 1/2), the
    margin's FMA (at most 1/2), thr = fl(1/2 - delta) (1/4), and T = fl(fl(thr - e0) fl(1 / lvl)) (1/4 for
    the difference, two relative u on less than half a level, 1).  The slicer's two constants need no term:
    rho is taken from the table under the float32 constants themselves."""
    return {"final add": side / 2, "first FMA": side - 0.5, "margin FMA": 0.5, "thr": 0.25, "T": 1.25}


def eps(side=8):
    """sparse_eps: (1.5 side + 6) u."""
    return (1.5 * side + 6.0) * U


def slicer_constants(n_fft=1024, side=8, step=2 / math.sqrt(42)):
    """The float32 multiplier and offset of ScreenSlicer::load on the unnormalised spectrum, times
    side - 1: levels per unit of z, and the offset in levels."""
    mul = np.float32((1 / step) * (1 / math.sqrt(n_fft)) / (side - 1))
    add = np.float32((side - 1) / 2 / (side - 1))
    return float(mul) * (side - 1), float(add) * (side - 1)


def rho(n_fft=1024, side=8, step=2 / math.sqrt(42)):
    """The largest distance of a table point N l32 from its own level under those constants."""
    lvl, off = slicer_constants(n_fft, side, step)
    lev = (np.arange(side) - (side - 1) / 2) * step
    p = (np.float32(n_fft) * (lev / math.sqrt(n_fft)).astype(np.float32)).astype(np.float64)
    return float(np.abs(p * lvl + off - np.arange(side)).max())


def e0(side=8):
    return float(np.float32(1.001 * (eps(side) + rho(side=side))))


def threshold(delta, side=8, n_fft=1024):
    """T of a symbol whose bound is delta levels, in units of the unnormalised spectrum; negative (every
    quad sliced) when delta leaves nothing under 1/2 or is not finite."""
    thr = 0.5 - delta if delta < 0.5 else -1.0
    return (thr - e0(side)) / slicer_constants(n_fft, side)[0]


def mu(snr_db, n_fft=1024, side=8, step=2 / math.sqrt(42), amax=math.sqrt(98 / 42), power=1.0):
    """sparse_mu: the expected number of components over T per quad index and wave, 8 * 64 * 2 Q(T / sigma_c)
    in levels, T at the expected norm of the transformed noise (the delta of link_nscreen_expect.undecided)."""
    sigma = math.sqrt(power / 10 ** (snr_db / 10) / 2)
    sc = sigma / step
    delta = NX.delta_sym(math.sqrt(2 * n_fft) * sigma, amax) / step + NX.SLICER_U * U
    t = 0.5 - delta - 1.001 * (eps(side) + rho(n_fft, side, step))
    return LANES * QUAD_COMPONENTS * math.erfc(t / (sc * math.sqrt(2))) if t > 0 else float(LANES * QUAD_COMPONENTS)


def sliced_share(snr_db):
    """The share of quads with a component over T: 1 - exp(-mu)."""
    return 1 - math.exp(-mu(snr_db))


def sparse_rule(snr_db, noise_on=True):
    """Automatic mode tests the quads when the noise is off or mu is below kSparseMaxPerQuad."""
    return not noise_on or mu(snr_db) < MAX_PER_QUAD


def model(snr_db, symbols, seed=1, n_fft=1024):
    """link_nscreen_expect.draw's symbols, noise and bound (the noise screen's model runs on the same), with the
    quads of the sparse slicer: components k = 256 q .. 256 q + 255 stand for quad q (the property is one
    of each component, so the grouping only sets how many quads are skipped).  Returns the number of quads,
    of skipped quads, and of skipped quads that hold an element whose float64 decision differs from the
    transmitted level, whose float32 decision does, or whose float32 margin exceeds thr."""
    ii, qq, z64, ghat, zhat, delta = NX.draw(snr_db, symbols, seed, n_fft)
    lvl, off = slicer_constants(n_fft)
    thr = np.where(delta < 0.5, 0.5 - delta, -1.0)
    t = np.array([threshold(d) for d in delta])

    def levels(z):
        y = np.clip(np.stack([z.real, z.imag]) * lvl + off, 0, 7)
        return y, np.round(y)

    sent = np.stack([ii, qq])
    y32, l32 = levels(zhat.astype(np.complex128))
    _, l64 = levels(z64)
    bad = (l64 != sent) | (l32 != sent) | (np.abs(y32 - l32) > thr[None, :, None])  # (2, S, N)
    bad = bad.any(axis=0).reshape(symbols, 4, n_fft // 4).any(axis=2)
    g = np.maximum(np.abs(ghat.real), np.abs(ghat.imag)).reshape(symbols, 4, n_fft // 4).max(axis=2)
    skipped = g <= t[:, None]
    return 4 * symbols, int(skipped.sum()), int((skipped & bad).sum())

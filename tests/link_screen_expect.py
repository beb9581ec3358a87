"""The fused link's float32 screen (csrc/ofdm_link_inst.hpp) restated: the bound
delta on |z32 - z64| of a symbol, the automatic mode's rule and the workgroup's LDS."""

import math

K = 70.0            # kScreenK
U = 2.0 ** -24      # kScreenU: the float32 unit roundoff
SLICER_U = 40.0     # kScreenSlicerU: the level coordinate's own roundings, in u
MAX_UNDECIDED = 0.35  # kScreenMaxUndecided


def higham_eta(mu=U):
    """Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2: eta = mu + gamma_4 (sqrt 2 + mu)."""
    g4 = 4 * U / (1 - 4 * U)
    return mu + g4 * (math.sqrt(2) + mu)


def k_derived(log2n=10):
    """One transform's t eta / (1 - t eta) in units of u, plus one u for the LUT's rounding (first
    transform) or the noise FMA's (second): what K must cover."""
    t_eta = log2n * higham_eta()
    return t_eta / (1 - t_eta) / U + 1


def delta_sym(z32_norm, n_fft, amax):
    """The bound on |z32_k - z64_k| for every k of a symbol, in the units of the received points z
    (the ortho-normalised spectrum: the kernel's unnormalised one over sqrt N): K u (||z32||_2 +
    sqrt N amax), amax the largest modulus of the channel tap times the constellation.  (The kernel's
    sqrt N ||x||_2 <= N^1.5 a with a = amax / sqrt N, all over sqrt N.)"""
    return K * U * (z32_norm + math.sqrt(n_fft) * amax)


def undecided(snr_db, n_fft=1024, side=8, step=2 / math.sqrt(42), amax=math.sqrt(98 / 42), power=1.0):
    """Expected undecided axes per symbol (screen_const): the automatic mode screens below MAX_UNDECIDED."""
    sigma = math.sqrt(power / 10 ** (snr_db / 10) / 2)       # per component, of a normalised point
    sc = sigma / step                                         # in levels
    delta = delta_sym(math.sqrt(n_fft * (power + 2 * sigma * sigma)), n_fft, amax) / step + SLICER_U * U
    phi = math.exp(-0.125 / (sc * sc)) / math.sqrt(2 * math.pi) / sc
    return 2 * n_fft * (side - 1) * (2 / side) * 2 * delta * phi


def lds_bytes(spb=12, screen=True):
    """link_carve + the static tables of k_link<double, 10, 6, SCREEN>."""
    tt = 15 * 16 + 3 * 256                           # tt_size(10)
    dynamic = 8 * 64 + spb * (1024 + 64) * 8 + 8 * (64 * spb // 64) + 2 * tt * 16
    if screen:
        dynamic += 2 * tt * 8 + 64 * 8               # float32 twiddles [forward | inverse], float32 LUT
    return dynamic + 64 * 16 + 64 * 8 + 64 * 16      # LUT, noise phase table, its widening to double

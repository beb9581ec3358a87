"""The fused link's noise screen (csrc/ofdm_link_inst.hpp) restated: the bound
delta on |zhat - z64| of a symbol, the automatic mode's rule, the workgroup's LDS, and a numpy model of
the screen itself.

The screen never runs the transmitter's IFFT.  With a flat channel folded into the LUT the spectrum the
slicer sees is, in exact arithmetic, z_k = N l_k + G_k (l the folded LUT entry of subcarrier k, G the
unnormalised FFT of the symbol's noise), so the screen transforms the noise alone in float32 and adds
the float32 LUT point times N.  Below everything is in the units of the received points (the
ortho-normalised spectrum: the kernel's unnormalised one over sqrt N), as tests/link_screen_expect.py."""

import math

import numpy as np

import link_screen_expect as X

K_N = 72.0            # kNScreenK
C_LUT = 3.0           # kNScreenC
U = X.U               # kScreenU: the float32 unit roundoff
SLICER_U = X.SLICER_U  # kScreenSlicerU, unchanged
MAX_UNDECIDED = 0.5   # kNScreenMaxUndecided


def k_derived(log2n=10):
    """What K_N must cover, in units of u ||ghat||_2: one transform's t eta / (1 - t eta) (Higham 24.2,
    66.6), one u for the noise product's rounding (nhat = fl(r e): ||nhat - n||_2 <= u ||n||_2, carried
    through the transform by linearity), and one u for the |ghat_k| <= ||ghat||_2 of the final add."""
    t_eta = log2n * X.higham_eta()
    return t_eta / (1 - t_eta) / U + 1 + 1


def c_derived(n_fft=1024):
    """What C_LUT must cover, in units of u N a: the LUT's rounding (1), the final add's u N a (1), and
    the complex128 kernel's own two transforms, 70 2^-53 (2 N^1.5 a + ||G||_2), whose first term is
    140 sqrt N 2^-29 of u N a (the second, against K_N u ||ghat||_2, is 2^-29 of it)."""
    return 2 + 140 * math.sqrt(n_fft) * 2.0 ** -29


def delta_sym(ghat_norm, amax):
    """The bound on |zhat_k - z64_k| for every k of a symbol: K_N u ||ghat||_2 + C_LUT u amax, amax the
    largest modulus of the channel tap times the constellation (the kernel's N a over sqrt N).  Where
    only the whole float32 spectrum z32 is at hand (the margin test), ||z32||_2 stands for ||ghat||_2:
    at -20 dB the signal's norm is about 10 % of the noise's and adds in quadrature, sqrt(1 + snr) - 1 =
    0.5 % on the norm, so the bound tested is the kernel's to within that."""
    return K_N * U * ghat_norm + C_LUT * U * amax


def undecided(snr_db, n_fft=1024, side=8, step=2 / math.sqrt(42), amax=math.sqrt(98 / 42), power=1.0):
    """Expected undecided axes per symbol (nscreen_const): ||ghat||_2 ~ sqrt(2 N) sigma in these units."""
    sigma = math.sqrt(power / 10 ** (snr_db / 10) / 2)
    sc = sigma / step
    delta = delta_sym(math.sqrt(2 * n_fft) * sigma, amax) / step + SLICER_U * U
    phi = math.exp(-0.125 / (sc * sc)) / math.sqrt(2 * math.pi) / sc
    return 2 * n_fft * (side - 1) * (2 / side) * 2 * delta * phi


def lds_bytes(spb=12):
    """link_carve + the static tables of the noise-screen k_link: the forward float32 twiddles only and
    the float32 LUT times N beside what the unscreened kernel holds."""
    tt = 15 * 16 + 3 * 256
    return X.lds_bytes(spb, screen=False) + tt * 8 + 64 * 8


# ---------------------------------------------------------------- a numpy model of the screen
def fft32(x):
    """Radix-2 decimation-in-time FFT in float32 arithmetic with once-rounded twiddles; x: (S, N)."""
    s, n = x.shape
    b = n.bit_length() - 1
    idx = np.arange(n)
    rev = np.zeros(n, dtype=np.int64)
    for i in range(b):
        rev |= ((idx >> i) & 1) << (b - 1 - i)
    a = x[:, rev].astype(np.complex64)
    m = 1
    while m < n:
        w = np.exp(-2j * np.pi * np.arange(m) / (2 * m)).astype(np.complex64)
        a = a.reshape(s, n // (2 * m), 2, m)
        t = (a[:, :, 1, :] * w).astype(np.complex64)
        u = a[:, :, 0, :]
        a = np.stack([(u + t).astype(np.complex64), (u - t).astype(np.complex64)], axis=2).reshape(s, n)
        m *= 2
    return a


def draw(snr_db, symbols, seed=1, n_fft=1024):
    """64-QAM at unit power over a flat unit channel; the noise as Mwc64x forms it (a float32 radius times
    a float32 entry of 64 phases: exact in double on the complex128 side, rounded once on the screen's).
    Returns the drawn level indices (ii, qq), the complex128 spectrum z64, the screen's transformed noise
    ghat and spectrum zhat, and its bound delta per symbol in levels (model and link_sparse_expect.model
    share the draw: the same generator calls in the same order)."""
    rng = np.random.default_rng(seed)
    lev = np.arange(-7, 8, 2) / math.sqrt(42)
    step, amax = 2 / math.sqrt(42), math.sqrt(98 / 42)
    ii, qq = rng.integers(0, 8, (symbols, n_fft)), rng.integers(0, 8, (symbols, n_fft))
    lut = (lev[ii] + 1j * lev[qq]) / math.sqrt(n_fft)            # folded LUT entries, per subcarrier
    x = np.fft.ifft(lut, axis=1) * n_fft                          # the transmitter's unnormalised IFFT
    sigma = np.float32(math.sqrt(1 / 10 ** (snr_db / 10) / 2))
    r = np.sqrt(-2 * np.log(1 - rng.random((symbols, n_fft)))).astype(np.float32)
    th = (2 * rng.integers(0, 64, (symbols, n_fft)) + 1) / 64 * np.pi
    er, ei = sigma * np.cos(th).astype(np.float32), sigma * np.sin(th).astype(np.float32)
    z64 = np.fft.fft(x + (r.astype(np.float64) * er + 1j * (r.astype(np.float64) * ei)), axis=1)
    # the screen: once-rounded products, one float32 transform, the point added
    ghat = fft32(((r * er) + 1j * (r * ei)).astype(np.complex64))
    zhat = (ghat + (lut * n_fft).astype(np.complex64)).astype(np.complex64)
    gn = np.linalg.norm(ghat.astype(np.complex128), axis=1)
    lvl = 1 / (step * math.sqrt(n_fft))                           # levels per unit of unnormalised z
    delta = (delta_sym(gn / math.sqrt(n_fft), amax) * math.sqrt(n_fft)) * lvl + SLICER_U * U
    return ii, qq, z64, ghat, zhat, delta


def model(snr_db, symbols, seed=1, n_fft=1024):
    """The screen on draw()'s symbols, with its margin.  Returns (kept, wrong_kept): the mask of symbols the
    screen keeps, and how many kept symbols hold an element whose float32 level differs from the float64
    one."""
    _, _, z64, _, zhat, delta = draw(snr_db, symbols, seed, n_fft)
    lvl = 1 / (2 / math.sqrt(42) * math.sqrt(n_fft))

    def levels(z):
        y = np.clip(np.stack([z.real, z.imag]) * lvl + 3.5, 0, 7)
        return y, np.round(y)

    y32, l32 = levels(zhat.astype(np.complex128))
    _, l64 = levels(z64)
    undec = (0.5 - np.abs(y32 - l32)) <= delta[None, :, None]
    kept = ~undec.any(axis=(0, 2))
    wrong = (l32 != l64).any(axis=(0, 2))
    return kept, int((kept & wrong).sum())

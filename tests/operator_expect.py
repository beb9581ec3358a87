"""The operator entry points' yardstick (ofdm_fft, ofdm_modulate, ofdm_demodulate, ofdm_equalize, ofdm_map,
ofdm_demap, ofdm_demap_count, ofdm_channel, ofdm_power, ofdm_awgn; include/ofdm_hip.h "operators"): one
float64 reference per operator on oracle/ofdm_oracle.py, one derived bound on |kernel - reference| per
operator, the comparators that apply them, the input generators of the deciders, and the shapes the
tests run -- shared by tests/test_operator_expect_cpu.py (the yardstick checked without a GPU) and
tests/test_gpu_operator_abi.py (the kernels).

A complex64 plan's reference takes the input ALREADY ROUNDED to float32 (round_input) and computes in
float64: what is compared is the kernel's arithmetic, not the rounding of its input.  u is the unit
roundoff of the plan precision.  Every bound is a hard assertion derived in its docstring; none is fitted.
A comparator returns the largest error / bound ratio (inf where an exact property is violated): <= 1 passes.
"""

import math

import numpy as np

import ofdm_oracle as O

F32, F64 = 0, 1                      # enum ofdm_precision
U32, U64 = 2.0 ** -24, 2.0 ** -53
K_BLOCK = 256                        # kBlock: threads of a workgroup
MAX_GRID = 4096                      # kMaxGrid: clamp_grid caps every launch there
# The complex64 rows kernels' worst row-wise relative error may be this many times that of numpy's own
# complex64 transform of the same rows: eta grows by 1.45 from mu = u to mu = 4u, and a radix-16 pass
# rounds more per butterfly than a radix-4 one (measured: profiles/operator_abi_margins.json)
NUMPY_RATIO = 8.0
F64_ABS = 1e-12                      # the suite's complex128 tolerance at unit-scale inputs


def unit(prec):
    return U32 if prec == F32 else U64


def cdtype(prec):
    return np.complex64 if prec == F32 else np.complex128


def round_input(a, prec):
    """The array as a plan of this precision reads it, widened back to complex128 (or float64)."""
    a = np.asarray(a)
    if prec == F64:
        return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)
    if np.iscomplexobj(a):
        return a.astype(np.complex64).astype(np.complex128)
    return a.astype(np.float32).astype(np.float64)


def spb(n):
    """Geo<LOGN>::SPB restated: rows one workgroup iteration of k_rows holds.  E = min(N, 16) elements
    per thread, TPS = N / E threads per row, SPB = 256 / TPS: 256 at N <= 16, then 4096 / N."""
    return K_BLOCK if n <= 16 else 4096 // n


# --------------------------------------------------------------------------- references (float64)


def ref_fft(x, inverse):
    return np.fft.ifft(x, axis=1, norm="ortho") if inverse else np.fft.fft(x, axis=1, norm="ortho")


def ref_modulate(X, cp, zp=False):
    """OFDMModulator.modulate: [prefix | ifft(X, ortho)], or with zero padding [ifft(X, ortho) | 0 ... 0]."""
    if not zp:
        return O.modulate(X, cp)
    return np.concatenate([np.fft.ifft(X, axis=1, norm="ortho"), np.zeros((X.shape[0], cp))], axis=1)


def fold(yt, n, cp, zp, fold_len=None):
    """The receiver's rows of N before the transform: the prefix stripped, or the zero guard overlap-added
    onto the head (as test_zero_padding_and_sc_ofdm_vs_oracle writes it).  fold_len: a mutation's length."""
    if not zp:
        return yt[:, cp:]
    f = yt[:, :n].copy()
    m = cp if fold_len is None else fold_len
    f[:, :m] += yt[:, n:n + m]
    return f


def ref_demod_rows(yt, n, cp, zp=False):
    """ofdm_demodulate before its equaliser: fft(ortho) of the folded rows."""
    return np.fft.fft(fold(yt, n, cp, zp), axis=1, norm="ortho")


def eq_weights(Y, H, eq, snr_db):
    """The reference's weight w with Z = w Y, per element: 1 (NONE), 1 / where(H == 0, 1e-10, H) (ZF),
    conj H / (|H|^2 + nv) with nv of each row (MMSE; O.equalize's arithmetic)."""
    if eq == "NONE":
        return np.ones(Y.shape, np.complex128)
    if eq == "ZF":
        return np.broadcast_to(1.0 / np.where(H == 0, 1e-10, H)[None, :], Y.shape).astype(np.complex128)
    g = np.mean(np.abs(H) ** 2)
    sp = np.mean(np.abs(Y) ** 2, axis=1, keepdims=True)
    nv = (sp / 10 ** (snr_db / 10)) / g if g != 0 else np.full_like(sp, np.inf)
    return np.conj(H)[None, :] / (np.abs(H)[None, :] ** 2 + nv)


def ref_equalize(Y, H, eq, snr_db):
    return O.equalize(Y, H, eq, snr_db)


def ref_demodulate(yt, n, cp, zp, H, eq, snr_db):
    return O.equalize(ref_demod_rows(yt, n, cp, zp), H, eq, snr_db)


def ref_conv(s, h_raw):
    return O.channel_conv(s, np.asarray(h_raw, np.complex128))


def sigma_of(power_sum, length, snr_db):
    """AWGNoiseModel's sigma from a power record: sqrt((power_sum / len) / 10^(snr/10) / 2)."""
    return math.sqrt((power_sum / length) / 10 ** (snr_db / 10) / 2)


def ref_awgn(y, power_sum, length, snr_db, nr, ni):
    """O.awgn with the power taken from the record the kernel reads (the same power_sum and len)."""
    return y + sigma_of(power_sum, length, snr_db) * (nr + 1j * ni)


def fixed_indices(data, n_out, b):
    """ofdm_map's fixed-mode indices: element e uses bits [e b, e b + b), bits past the input are zero."""
    bits = O.bytes_to_bits(data).astype(np.int64)
    bits = np.concatenate([bits, np.zeros(max(0, n_out * b - len(bits)), np.int64)])[: n_out * b]
    return bits.reshape(n_out, b) @ (1 << np.arange(b - 1, -1, -1))


def map_points(lut, idx, prec):
    """The map's output: the LUT rounded ONCE to the plan precision, gathered."""
    return lut.astype(cdtype(prec))[idx]


def adaptive_layout(orders):
    """bits and bit offset of every subcarrier, and the OFDM symbol's bits."""
    bps = np.array([int(np.log2(o)) if o > 0 else 0 for o in orders], np.int64)
    offs = np.concatenate([[0], np.cumsum(bps)[:-1]])
    return bps, offs, int(bps.sum())


def adaptive_indices(data, orders, n_sym, offs=None):
    """(S, N) LUT indices of AdaptiveConstellationMapper.encode; offs: a mutation's offsets."""
    bps, o, tot = adaptive_layout(orders)
    offs = o if offs is None else offs
    bits = O.bytes_to_bits(data)[: n_sym * tot].reshape(n_sym, tot).astype(np.int64)
    idx = np.zeros((n_sym, len(orders)), np.int64)
    for k in np.flatnonzero(bps):
        idx[:, k] = bits[:, offs[k]:offs[k] + bps[k]] @ (1 << np.arange(bps[k] - 1, -1, -1))
    return idx


def adaptive_bytes(idx, orders, offs=None):
    """AdaptiveConstellationMapper.decode's bytes from (S, N) decided indices: subcarrier-major bits,
    whole bytes only."""
    bps, o, tot = adaptive_layout(orders)
    offs = o if offs is None else offs
    rb = np.zeros((idx.shape[0], tot), np.uint8)
    for k in np.flatnonzero(bps):
        rb[:, offs[k]:offs[k] + bps[k]] = (idx[:, k][:, None] >> np.arange(bps[k] - 1, -1, -1)) & 1
    allb = rb.ravel()
    return np.packbits(allb[: len(allb) // 8 * 8]).tobytes()


def count_errors(idx_rx, idx_tx, b):
    """ofdm_demap_count's fixed-mode increments: (bit errors over every bit, symbol errors)."""
    d = np.asarray(idx_rx, np.int64) ^ np.asarray(idx_tx, np.int64)
    bits = sum(((d >> j) & 1) for j in range(b))
    return int(bits.sum()), int(np.count_nonzero(d))


# --------------------------------------------------------------------------- bounds


def higham_eta(u, mu):
    """Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2: eta = mu + gamma_4 (sqrt 2 + mu),
    gamma_4 = 4u / (1 - 4u); in float32 this is link_screen_expect.higham_eta(mu)."""
    g4 = 4 * u / (1 - 4 * u)
    return mu + g4 * (math.sqrt(2) + mu)


def rows_rel(n, prec):
    """The rows kernels' relative bound per row: ||y^ - y||_2 <= (t eta + 2u) ||y||_2, t = max(log2 N, 1).
    Theorem 24.2 bounds a radix-2 transform of t stages whose twiddles carry a relative error mu by
    t eta / (1 - t eta) ~ t eta; a radix-16 pass is four such stages evaluated together, so t = log2 N
    holds for the kernel's passes (t = 1 at N = 1, where nothing is transformed).  The kernels form a
    twiddle as the product of two table entries each rounded once from double (lo[m & 63] * hi[m >> 6],
    ofdm_device.hpp twiddle()): (1 + u)^2 for the entries, sqrt 2 gamma_2 ~ 2u for the complex product,
    hence mu = 4u.  The extra 2u: the ortho scale 1 / sqrt N rounded to the plan precision and multiplied
    in (2 roundings; the transforms are linear, so it scales the row), which also covers the single
    addition of the zero-padding overlap-add (u |sum| per folded sample, before the same scale)."""
    u = unit(prec)
    t = max(int(round(math.log2(n))), 1)
    return t * higham_eta(u, 4 * u) + 2 * u


def rows_bound(y_ref, n, prec):
    """B_row, (rows, 1): the bound on the 2-norm of a row's error, and therefore on every element's."""
    return rows_rel(n, prec) * np.linalg.norm(y_ref, axis=1, keepdims=True)


EQ_U = 40.0


def equalizer_bound(Z_ref, w, b_row, prec):
    """|Z^_k - Z_k| <= |w_k| B_row + 40u |Z_k|: the row's transform error through the weight, plus the
    equaliser's own roundings relative to the result (b_row = 0 for ofdm_equalize, which reads Y itself).
    The count behind 40u, for one row's nv = mean |Y|^2 / snr / gain_mean and w = conj H / (|H|^2 + nv):
      |Y_k|^2 = re^2 + im^2            2u   (two products, one addition of positive terms)
      the sum over the row            24u   (<= 16 terms serially per thread: 15 additions at most; then a
                                             tree of log2 256 = 8 levels over the row's threads; every
                                             term positive, so the errors add relatively: 15u + 8u, +1u
                                             for the finalising addition of the wave partials)
      / N                              0    (a power of two)
      / snr_lin, / gain_mean           4u   (each rounded to the plan precision, each one division)
      |H|^2 table entry, + nv          2u   (the entry rounded once; one addition, both terms positive,
                                             so d = |H|^2 + nv carries at most the larger part's error + u)
      conj H entry, / d                2u   (the entry rounded once; one division per component)
      w Y                              3u   (sqrt 2 gamma_2 of the complex product)
    together 37u, under 40u.  ZF reads a table entry rounded once (1 / H formed in double) and multiplies:
    4u.  Two things this count leaves out, as the bound is the one the operators are held to: gain_mean
    is summed in double by k_eq_tables in another order than numpy's mean (a few 2^-53, nothing in
    complex64), and in ofdm_demodulate nv is formed from the transformed row Y^, whose error enters nv
    with relative weight <= 2 B_row |Y_k| / ||Y||_2 on top of |w_k| B_row."""
    u = unit(prec)
    return np.abs(w) * b_row + EQ_U * u * np.abs(Z_ref)


def conv_bound(s, h_raw, prec):
    """|y^_n - y_n| <= (L + 5) u (|h| * |s|)_n.  y_n = sum_l h_l s_(n-l) accumulated serially from l = 0:
    each complex product errs by sqrt 2 gamma_2 < 3u of |h_l| |s_(n-l)|, each term then passes through at
    most L - 1 complex additions (u each, relative to the partial sums, which |h| * |s| bounds), and the
    normalised taps are rounded once to the plan precision (u): (3 + L - 1 + 1) u = (L + 3) u to first
    order, L + 5 with the second-order terms and the taps' normalisation in double."""
    h = O.normalize_h(np.asarray(h_raw, np.complex128))
    L = len(h)
    return (L + 5) * unit(prec) * np.convolve(np.abs(s), np.abs(h), mode="full")[: len(s)]


def power_rel(prec):
    """Relative bound on a power sum: 3 u_R + 64 2^-53.  |v|^2 is formed in the plan precision (two
    products, one addition: < 3 u_R, every term positive, so it carries to the sum); the sum itself is
    double: at most 2 serial terms per thread at the lengths the tests run (grid = min(ceil(len / 256),
    4096)), an 8-level tree over the workgroup, the 16-term serial finalize over 256 threads' strided
    partials and its own tree -- under 64 roundings of 2^-53 on positive terms, the += included."""
    return 3 * unit(prec) + 64 * U64


def awgn_bound(y, sigma, nr, ni, prec):
    """Per component, |y^ - (y + sigma n)| <= 5u (|y| + sigma |n|): sigma rounded to the plan precision (u),
    the normal rounded to it (u), their product (u), the addition (u of the result, itself within
    |y| + sigma |n|): 4u to first order, 5u with the second-order terms and sigma's own double arithmetic."""
    u = unit(prec)
    return 5 * u * (np.abs(y.real) + sigma * np.abs(nr)), 5 * u * (np.abs(y.imag) + sigma * np.abs(ni))


# --------------------------------------------------------------------------- comparators


def worst(err, bound):
    """max err / bound; where the bound is 0 the error must be 0 (else inf).  Non-finite values fail."""
    err = np.asarray(err, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    if err.size == 0:
        return 0.0
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound))):
        return math.inf
    zero = bound == 0
    if np.any(err[zero] != 0):
        return math.inf
    if np.all(zero):
        return 0.0
    return float(np.max(err[~zero] / bound[~zero]))


def rows_ratio(got, ref, n, prec):
    """The rows bound applied to the 2-norm of each row's error (which implies it per element)."""
    err = np.linalg.norm(np.asarray(got, np.complex128) - ref, axis=1, keepdims=True)
    return worst(err, rows_bound(ref, n, prec))


def rows_rel_error(got, ref):
    """Worst row-wise relative 2-norm error (the figure compared with numpy's complex64 transform)."""
    nrm = np.linalg.norm(ref, axis=1)
    err = np.linalg.norm(np.asarray(got, np.complex128) - ref, axis=1)
    ok = nrm > 0
    return float(np.max(err[ok] / nrm[ok])) if np.any(ok) else 0.0


def cmp_fft(got, x, inverse, prec):
    return rows_ratio(got, ref_fft(x, inverse), x.shape[1], prec)


def cmp_modulate(got, X, cp, zp, prec):
    """Body within the rows bound; prefix samples equal to the body samples they copy EXACTLY, guard
    samples exactly 0 (inf otherwise)."""
    n = X.shape[1]
    got = np.asarray(got)
    if zp:
        body, guard = got[:, :n], got[:, n:]
        if np.any(guard != 0):
            return math.inf
    else:
        body, pre = got[:, cp:], got[:, :cp]
        if not np.array_equal(pre, body[:, n - cp:]):
            return math.inf
    return rows_ratio(body, ref_modulate(X, 0), n, prec)


def cmp_demodulate(got, yt, n, cp, zp, H, eq, snr_db, prec):
    Y = ref_demod_rows(yt, n, cp, zp)
    if eq == "NONE":
        return rows_ratio(got, Y, n, prec)
    w = eq_weights(Y, H, eq, snr_db)
    Z = w * Y
    return worst(np.abs(np.asarray(got, np.complex128) - Z), equalizer_bound(Z, w, rows_bound(Y, n, prec), prec))


def cmp_equalize(got, Y, H, eq, snr_db, prec):
    """ofdm_equalize: NONE is a copy (exact); ZF / MMSE within 40u |Z| (B_row = 0)."""
    if eq == "NONE":
        return 0.0 if np.array_equal(np.asarray(got, np.complex128), Y) else math.inf
    w = eq_weights(Y, H, eq, snr_db)
    Z = np.where(w == 0, 0, w * Y)  # nv = inf: the weight is 0 and so is every output
    return worst(np.abs(np.asarray(got, np.complex128) - Z), equalizer_bound(Z, w, 0.0, prec))


def cmp_conv(got, s, h_raw, prec):
    return worst(np.abs(np.asarray(got, np.complex128) - ref_conv(s, h_raw)), conv_bound(s, h_raw, prec))


def cmp_power(got, v, prec, start=0.0):
    """*power_sum after one call that found `start` (>= 0) there: start + sum |v|^2 (the "+="), within the
    relative bound of the result."""
    ref = start + float(np.sum(np.abs(v) ** 2))
    return worst(abs(got - ref), power_rel(prec) * ref)


def cmp_awgn(got, y, power_sum, snr_db, nr, ni, prec):
    sg = sigma_of(power_sum, len(y), snr_db)
    ref = ref_awgn(y, power_sum, len(y), snr_db, nr, ni)
    br, bi = awgn_bound(y, sg, nr, ni, prec)
    got = np.asarray(got, np.complex128)
    return max(worst(np.abs(got.real - ref.real), br), worst(np.abs(got.imag - ref.imag), bi))


# --------------------------------------------------------------------------- inputs of the deciders
# Every point provably off a decision boundary: no case is ever excluded (the share is 0 by construction).

DISPLACE = 0.45  # of half a level step (QAM, per axis) or of half the angular spacing (PSK)


def qam_points(lut, idx, rng):
    """LUT[idx] displaced by at most 0.45 of half a level step per axis; outer rows and columns also
    pushed outwards by up to 5 half-steps (as test_qam1024_decode_matches_argmin)."""
    lev = np.unique(lut.real)
    half = (lev[1] - lev[0]) / 2
    p = lut[idx]
    z = p + DISPLACE * half * (rng.uniform(-1, 1, len(idx)) + 1j * rng.uniform(-1, 1, len(idx)))
    edge = np.abs(p.real) == np.abs(lut.real).max()
    z[edge] += rng.uniform(0, 5, int(edge.sum())) * half * np.sign(p[edge].real)
    edge = np.abs(p.imag) == np.abs(lut.imag).max()
    z[edge] += 1j * rng.uniform(0, 5, int(edge.sum())) * half * np.sign(p[edge].imag)
    return z


def psk_points(lut, idx, rng):
    """LUT[idx] rotated by at most 0.45 of half the angular spacing, scaled radially in [0.7, 1.3]
    (2-PSK: the half spacing is pi / 2, the boundary the imaginary axis)."""
    m = len(lut)
    return lut[idx] * rng.uniform(0.7, 1.3, len(idx)) * np.exp(1j * DISPLACE * (np.pi / m) * rng.uniform(-1, 1, len(idx)))


def decider_points(kind, lut, idx, rng):
    return qam_points(lut, idx, rng) if kind == "qam" else psk_points(lut, idx, rng)


def make_lut(kind, order):
    return O.qam_lut(order) if kind == "qam" else O.psk_lut(order)


def wrong_decisions(lut, n, rng, kind="qam"):
    """The "wrong decision" inputs: points built around entry j while the transmitted bits say entry i,
    j != i for every element.  Returns (idx_tx, idx_rx, z): the counts are count_errors(idx_rx, idx_tx)."""
    m = len(lut)
    i = rng.integers(0, m, n)
    j = (i + rng.integers(1, m, n)) % m
    return i, j, decider_points(kind, lut, j, rng)


def case_indices(m, n, rng):
    """n random LUT indices, the first one 1: its single set bit lands in a different place under any
    other bit order, whatever n and b."""
    idx = rng.integers(0, m, n)
    idx[0] = 1
    return idx


def adaptive_case(seed=3, n=64):
    """Orders drawn from {0, 4, 16, 64, 256} with subcarrier 0 active (as test_adaptive_mapper_vs_oracle)."""
    rng = np.random.default_rng(seed)
    orders = rng.choice([0, 4, 16, 64, 256], size=n)
    orders[0] = 16
    return orders


ADAPTIVE_SYMS = [1, 3, 8]


def pack_indices(idx, b):
    """MSB-first bytes of fixed-mode indices (tail zero-padded): the tx bits of these symbols."""
    return O.indices_to_bytes(np.asarray(idx, np.int64), b)


# --------------------------------------------------------------------------- shapes the tests run

LOGNS = list(range(13))
FIXED_ORDERS = [("psk", 2), ("psk", 8), ("psk", 1024), ("qam", 4), ("qam", 16), ("qam", 64), ("qam", 256),
                ("qam", 1024), ("qam", 4096)]
MAP_COUNTS = [1, 255, 256, 257]
SECOND_TRIP_FLAT = (1 << 20) + 257    # elements: more than kMaxGrid workgroups of 256
SECOND_TRIP_DEMAP64 = -(-SECOND_TRIP_FLAT * 8 // 6)  # 64-QAM symbols whose demap writes 2^20 + 257 bytes
CONV_TAPS = [1, 2, 4, 32]
EQ_NAMES = ["NONE", "ZF", "MMSE"]
DEMOD_SNR_DB = 15.0
EQUALIZE_N = [1, 2, 64, 256, 4096]
CPU_CUT = 4096                        # the CPU emulations cut the large-count shapes to this many elements


def row_counts(n):
    s = spb(n)
    return [1, s + 1, 2 * s - 1]


def prefixes(n):
    """(cp, zero_padding): cyclic cp in {0, 1, N} (cp = 1 dropped where N = 1 makes it N), ZP cp = min(N, 3)."""
    out = [(0, False)] + ([(1, False)] if n > 1 else []) + [(n, False), (min(n, 3), True)]
    return out


def conv_lengths(L):
    return sorted({x for x in (1, L - 1, L, 255, 256, 257, 1000) if x >= 1})


def decaying_taps(L=32):
    """The 32-tap decaying draw of test_lds_limit_shapes_run (cut to L taps)."""
    rng = np.random.default_rng(8)
    h = (rng.normal(size=32) + 1j * rng.normal(size=32)) * np.exp(-np.arange(32) / 6.0)
    return h[:L]


def rows_input(rows, width, seed, scaled=False):
    """Unit-variance complex rows; scaled: row r times 1 + r / 4, so no row's nv is its neighbour's."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(rows, width)) + 1j * rng.normal(size=(rows, width))) / math.sqrt(2)
    if scaled:
        x = x * (1 + np.arange(rows)[:, None] / 4.0)
    return x

"""The soft-decision record (ofdm_rx_soft, include/ofdm_hip.h) restated in NumPy: what
tests/test_soft_cpu.py and tests/test_gpu_soft.py compare the device record against.

For an element on subcarrier k with b bits (hb = b / 2, side = 2^hb) and point v, widened to double:
bit i (MSB first) belongs to the Q axis for i < hb (a = idx >> hb, level LUT[a << hb].im, c = v.im,
j = i) and to the I axis otherwise (a = idx & (side - 1), level LUT[a].re, c = v.re, j = i - hb).  A
brute-force scan: d_a = (c - lev_a)**2 for every a -- one rounded subtraction and one rounded
multiplication, which is what NumPy does with two array operations -- m_0 / m_1 the minimum over the a
whose bit j (MSB first within hb) is 0 / 1, D = m_1 - m_0, u = D * g[k], t = u * inv_w, each one rounded
array operation.  t NaN: `invalid`; otherwise bin B/2 + floor(t) clamped to [0, B - 1].  The record is
counts[row][tx bit][bin] with row = hb (hb - 1) + i.  From the same stored value every double is the
device's bit for bit, so a record is compared with the restatement of the run's own tap exactly.

Against points only known to within delta, D moves by at most 4 delta (max level - min level) -- D is
piecewise linear in c with slope 2 (l_0 - l_1) -- so a bit whose t lies within that bound times g inv_w
of a bin line may fall on either side: `bracket` counts, per cell, the decided bits and the undecided
ones that could land there.
"""

import numpy as np

import ofdm_oracle as O

ROWS = 20


def row0(b):
    return (b // 2) * (b // 2 - 1)


def inv_width(B, L):
    """inv_w as the engine hands it to the library (engine.soft_grid)."""
    return int(B) / (2.0 * float(L))


def per_subcarrier(orders, N):
    """int64 [N]: the order of every subcarrier (0: inactive) from a scalar M or an array."""
    o = np.asarray(orders, np.int64)
    return np.full(N, int(o), np.int64) if o.ndim == 0 else o


def scale(orders, N, weights=None):
    """float64 [N]: g[k] = w_k / step_k^2, step_k = (max I level - min I level) / (side - 1) of the
    reference's square-QAM LUT of the subcarrier's order (engine.soft_scale); inactive: 0."""
    o = per_subcarrier(orders, N)
    g = np.zeros(N, np.float64)
    for m in np.unique(o[o > 0]):
        re = O.qam_lut(int(m)).real
        step = (float(re.max()) - float(re.min())) / (int(np.sqrt(m)) - 1)
        g[o == m] = 1.0 / (step * step)
    w = np.ones(N, np.float64) if weights is None else np.asarray(weights, np.float64)
    return w * g


def csi_weights(h_raw, N):
    p = np.abs(np.fft.fft(np.asarray(h_raw, np.complex128), N)) ** 2
    return p / p.max()


def _bits(Z, idx, orders, g, B, L, k_lo, k_hi, n_valid, sym0, span_scale=None):
    """Every compared bit in range, flattened: (row, tx bit, t) and, with span_scale (the per-element delta),
    the bound on t."""
    Z = np.asarray(Z)
    if Z.ndim == 1:
        Z = Z[None, :]
    S, N = Z.shape
    idx = np.asarray(idx, np.int64).reshape(S, N)
    o = per_subcarrier(orders, N)
    g = np.asarray(g, np.float64)
    inv_w = inv_width(B, L)
    bk = np.array([int(m).bit_length() - 1 if m > 0 else 0 for m in o], np.int64)
    bitoff = np.concatenate([[0], np.cumsum(bk)[:-1]])
    bps = int(bk.sum())
    k_hi = N if k_hi is None else k_hi
    inrange = np.zeros(N, bool)
    inrange[k_lo:k_hi] = True
    sg = sym0 + np.arange(S, dtype=np.int64)
    rows, txs, ts, bounds = [], [], [], []
    for m in np.unique(o[o > 0]):
        m = int(m)
        b = m.bit_length() - 1
        hb, side = b // 2, 1 << (b // 2)
        lut = O.qam_lut(m)
        cols = np.flatnonzero((o == m) & inrange)
        if cols.size == 0:
            continue
        z = Z[:, cols]
        ix = idx[:, cols]
        for i in range(b):
            if i < hb:
                a_tx, lev, c, j = ix >> hb, lut[np.arange(side) << hb].imag, z.imag.astype(np.float64), i
            else:
                a_tx, lev, c, j = ix & (side - 1), lut[:side].real, z.real.astype(np.float64), i - hb
            lev = lev.astype(np.float64)
            abit = (np.arange(side) >> (hb - 1 - j)) & 1
            with np.errstate(invalid="ignore", over="ignore"):
                d = (c[..., None] - lev) ** 2
                m0 = d[..., abit == 0].min(axis=-1)
                m1 = d[..., abit == 1].min(axis=-1)
                D = m1 - m0
                u = D * g[cols]
                t = u * inv_w
            tx = (a_tx >> (hb - 1 - j)) & 1
            valid = np.ones(z.shape, bool)
            if n_valid is not None:
                valid = sg[:, None] * bps + bitoff[cols][None, :] + i < n_valid
            rows.append(np.full(int(valid.sum()), row0(b) + i, np.int64))
            txs.append(tx[valid])
            ts.append(t[valid])
            if span_scale is not None:
                span = float(lev.max() - lev.min())
                dl = np.broadcast_to(np.asarray(span_scale, np.float64), Z.shape)[:, cols]
                bounds.append((4.0 * dl * span * g[cols] * inv_w)[valid])
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
    return cat(rows, np.int64), cat(txs, np.int64), cat(ts, np.float64), (cat(bounds, np.float64) if span_scale is not None else None)


def _bin(t, B):
    h = B // 2
    return (np.clip(np.floor(t), -h, h - 1) + h).astype(np.int64)


def record(Z, idx, orders, g, B, L, k_lo=0, k_hi=None, n_valid=None, sym0=0):
    """(counts int64 [20][2][B], invalid) of the (S, N) points Z with transmitted indices idx: the compared
    bits (global bit position below n_valid; None: all) of the subcarriers k_lo <= k < k_hi."""
    row, tx, t, _ = _bits(Z, idx, orders, g, B, L, k_lo, k_hi, n_valid, sym0)
    nan = np.isnan(t)
    cell = (row[~nan] * 2 + tx[~nan]) * B + _bin(t[~nan], B)
    counts = np.bincount(cell, minlength=ROWS * 2 * B).astype(np.int64).reshape(ROWS, 2, B)
    return counts, int(np.count_nonzero(nan))


def flat(counts, invalid):
    return np.concatenate([np.asarray(counts, np.int64).ravel(), [invalid]]).astype(np.int64)


def differences(Z, idx, orders, g, B, L, **kw):
    """(row, tx bit, t, bound) of every compared bit: what the tests of the sign look at."""
    return _bits(Z, idx, orders, g, B, L, kw.get("k_lo", 0), kw.get("k_hi"), kw.get("n_valid"), kw.get("sym0", 0),
                 span_scale=kw.get("delta", 0.0))


def _near_line(t, d, B):
    """t within d of a bin line: the integers -B/2 + 1 .. B/2 - 1 (beyond them the end bins saturate)."""
    h = B // 2
    with np.errstate(invalid="ignore"):
        line = np.clip(np.rint(t), -h + 1, h - 1)
        return np.isfinite(t) & (np.abs(t - line) <= d)


def undecided_share(Z, delta, idx, orders, g, B, L, **kw):
    row, tx, t, bd = differences(Z, idx, orders, g, B, L, delta=delta, **kw)
    return float(np.mean(_near_line(t, bd, B))) if t.size else 0.0


def bracket(Z, delta, idx, orders, g, B, L, k_lo=0, k_hi=None, n_valid=None, sym0=0):
    """(decided, maybe), int64 [40 B + 1] each (the last entry: invalid): per cell the count of the decided
    bits, and the number of undecided bits that could land there.  A record consistent with Z to within
    delta satisfies decided <= record <= decided + maybe."""
    row, tx, t, bd = _bits(Z, idx, orders, g, B, L, k_lo, k_hi, n_valid, sym0, span_scale=delta)
    assert np.all(bd[np.isfinite(bd)] < 0.5), "the bound is wider than half a bin"
    und = _near_line(t, bd, B)
    nan = np.isnan(t)
    dec = ~und & ~nan
    cells = ROWS * 2 * B
    decided = np.bincount((row[dec] * 2 + tx[dec]) * B + _bin(t[dec], B), minlength=cells + 1).astype(np.int64)
    decided[cells] = int(np.count_nonzero(nan))
    maybe = np.zeros(cells + 1, np.int64)
    lo, hi = _bin(t[und] - bd[und], B), _bin(t[und] + bd[und], B)
    base = (row[und] * 2 + tx[und]) * B
    np.add.at(maybe, base + lo, 1)
    np.add.at(maybe, (base + hi)[hi != lo], 1)
    return decided, maybe


def hard_bit_errors(counts):
    B = counts.shape[-1]
    return int(counts[:, 0, :B // 2].sum() + counts[:, 1, B // 2:].sum())


def gmi(counts, b, L, scales=None):
    """The reference GMI of the rows of b bits, in bits per subcarrier use: the largest over a dense grid of s
    of sum_rows [1 - sum_{v, j} counts log2(1 + exp(-(1 - 2 v) s centre_j)) / n_row]."""
    counts = np.asarray(counts, np.float64)
    B = counts.shape[-1]
    centres = (np.arange(B) - B / 2 + 0.5) * (2.0 * L / B)
    rows = counts[row0(b):row0(b) + b]
    n = rows.sum(axis=(1, 2))
    best = -np.inf
    for s in (np.logspace(-2, 3, 2001) if scales is None else scales):
        pen = np.stack([np.logaddexp(0.0, -s * centres), np.logaddexp(0.0, s * centres)]) / np.log(2.0)
        info = np.where(n > 0, 1.0 - (rows * pen[None]).sum(axis=(1, 2)) / np.maximum(n, 1.0), 0.0)
        best = max(best, float(info.sum()))
    return best

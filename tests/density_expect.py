"""The constellation-density record (ofdm_rx_density, include/ofdm_hip.h) restated in NumPy: what
tests/test_density_cpu.py and tests/test_gpu_density.py compare the device record against.

The index of a point c + i d in a grid of G bins per axis over [-L, L): per axis
t = (c - lo) * inv_w in float64 with lo = -L and inv_w = G / (2 L) -- one rounded subtraction and one
rounded multiplication, which is what NumPy does with two array operations -- inside iff 0 <= t < G on
both axes (NaN and infinities fail), bin (int(t_im), int(t_re)); everything else is `outside`.  From the
same stored value the index is the device's bit for bit, so a record is compared with the binning of
the run's own tap exactly.

Against points that are only known to within delta (the oracle's, or another kernel form's) a point
whose t lies within delta * inv_w of a grid line may fall on either side: `undecided` finds them and
`bracket` counts, per bin, the decided points and the undecided ones that could land there.
"""

import numpy as np

import ofdm_oracle as O
import philox_streams as P


def grid(G, L):
    """(lo, inv_w) as the engine hands them to the library (engine.density_grid)."""
    return -float(L), int(G) / (2.0 * float(L))


def _select(Z, k_lo, k_hi, active):
    Z = np.asarray(Z)
    if Z.ndim == 1:
        Z = Z[None, :]
    N = Z.shape[1]
    cols = np.zeros(N, bool)
    cols[k_lo:N if k_hi is None else k_hi] = True
    if active is not None:
        cols &= np.asarray(active, bool)
    return Z[:, cols], cols


def _coords(z, G, L):
    lo, inv_w = grid(G, L)
    with np.errstate(invalid="ignore", over="ignore"):
        tr = (z.real.astype(np.float64) - lo) * inv_w
        ti = (z.imag.astype(np.float64) - lo) * inv_w
    return tr, ti


def bin_points(Z, G, L, k_lo=0, k_hi=None, active=None):
    """(counts int64 [G][G] with row = imaginary bin, outside) of the (S, N) points Z: the columns
    k_lo <= k < k_hi that ``active`` (bool [N], None = all) keeps."""
    z, _ = _select(Z, k_lo, k_hi, active)
    tr, ti = _coords(z.ravel(), G, L)
    with np.errstate(invalid="ignore"):
        inside = (tr >= 0) & (tr < G) & (ti >= 0) & (ti < G)
    cell = ti[inside].astype(np.int64) * G + tr[inside].astype(np.int64)
    counts = np.bincount(cell, minlength=G * G).astype(np.int64).reshape(G, G)
    return counts, int(inside.size - np.count_nonzero(inside))


def _near_line(t, d, G):
    """t within d of an integer grid line 0 .. G (a non-finite t is decided: outside)."""
    with np.errstate(invalid="ignore"):
        line = np.clip(np.rint(t), 0, G)
        return np.isfinite(t) & (np.abs(t - line) <= d)


def undecided(Z, delta, G, L):
    """bool, Z's shape: the points whose t on either axis lies within delta * inv_w of an integer in
    [0, G] (0 and G, the square's border, among them); delta broadcasts against Z."""
    Z = np.asarray(Z)
    _, inv_w = grid(G, L)
    d = np.broadcast_to(np.asarray(delta, np.float64), Z.shape) * inv_w
    tr, ti = _coords(Z, G, L)
    return _near_line(tr, d, G) | _near_line(ti, d, G)


def bracket(Z, delta, G, L, k_lo=0, k_hi=None, active=None):
    """(decided, maybe), int64 [G * G + 1] each (the last entry: outside): per bin the count of the
    decided points, and the number of undecided points that could land there (every cell within
    delta * inv_w of the point on each axis).  A record consistent with Z to within delta satisfies
    decided <= record <= decided + maybe."""
    Z = np.asarray(Z)
    if Z.ndim == 1:
        Z = Z[None, :]
    dl = np.broadcast_to(np.asarray(delta, np.float64), Z.shape)
    z, cols = _select(Z, k_lo, k_hi, active)
    z, dl = z.ravel(), dl[:, cols].ravel()
    _, inv_w = grid(G, L)
    assert np.all(dl * inv_w < 0.5), "the bound is wider than half a bin"
    und = undecided(z, dl, G, L)
    c, out = bin_points(z[~und][None, :], G, L)
    decided = np.concatenate([c.ravel(), [out]]).astype(np.int64)
    maybe = np.zeros(G * G + 1, np.int64)
    tr, ti = _coords(z[und], G, L)
    d = dl[und] * inv_w
    for a, b, w in zip(tr, ti, d):
        cells = set()
        for x in {int(np.floor(a - w)), int(np.floor(a + w))}:
            for y in {int(np.floor(b - w)), int(np.floor(b + w))}:
                cells.add(y * G + x if 0 <= x < G and 0 <= y < G else G * G)
        for cell in cells:
            maybe[cell] += 1
    return decided, maybe


def philox_points(seed, S, N, M, h_raw, cp, eq, snr_db, orders=None, radius_fn=None, power_sum=None, sym0=0):
    """(Z, delta, idx) of a complex128 cyclic-prefix OFDM throughput-mode run: the equalised points of
    philox_streams.run_philox (the same calls in the same order, written out for sym0 = 0),
    the per-point bound z_error_bound puts on a GPU run's deviation from them, and the transmitted
    indices.  radius_fn / power_sum: the device's noise radii and the run's exact power (run_philox).
    sym0 > 0: global symbols [sym0, sym0 + S), run_philox's own z, delta and idx at that sym0 (at sym0 = 0
    they equal the ones written out here: tests/test_stream_range_cpu.py)."""
    if sym0:
        r = P.run_philox(seed, S, N, M, h_raw, cp, eq, snr_db, orders=orders, precision="f64", radius_fn=radius_fn,
                         power_sum=power_sum, sym0=sym0)
        return r.z, r.delta, r.idx
    gen = P.lane_generators(seed, np.arange(S), N)
    if orders is not None:
        orders = np.asarray(orders, np.int64)
        bk = np.array([int(np.log2(o)) if o > 0 else 0 for o in orders], np.int64)
        idx = P.tx_indices(gen, S, N, bk)
        X = np.zeros((S, N), np.complex128)
        for o in np.unique(orders[orders > 0]):
            cols = orders == o
            X[:, cols] = O.qam_lut(int(o))[idx[:, cols]]
    else:
        idx = P.tx_indices(gen, S, N, int(np.log2(M)))
        X = O.qam_lut(M)[idx]
    x = O.add_cp(np.fft.ifft(X, axis=1, norm="ortho"), cp)
    y = O.channel_conv(x.ravel(), np.asarray(h_raw, np.complex128)).reshape(S, N + cp)
    py = float(np.sum(np.abs(y) ** 2))
    p = (py if power_sum is None else float(power_sum)) / (S * (N + cp))
    sigma = float(np.sqrt((p / 10 ** (snr_db / 10)) / 2.0))
    nz, nb = P.lane_noise(gen, S, N, sigma, with_bound=True, radius_fn=radius_fn, product_rel=2.0 ** -53)
    rxs = y[:, cp:] + nz
    H = np.fft.fft(np.asarray(h_raw, np.complex128), N)
    Y = np.fft.fft(rxs, axis=1, norm="ortho")
    Z = O.equalize(Y, H, eq, snr_db)
    delta = P.z_error_bound("f64", Y, H, eq, snr_db, nb.sum(axis=1), "OFDM", N, np.sqrt((nb ** 2).sum(axis=1)))
    return Z, delta, idx

"""Fused GPU link engine: the hot path of ``Simulation.run`` (simulation/models.py:454-606).

One :class:`LinkEngine` = one modem configuration (N, prefix, channel, LUTs,
equaliser) held in a libofdm_hip plan.  :meth:`LinkEngine.run` pushes S OFDM
symbols through

    ofdm_tx  : bits -> map -> IFFT(ortho) + CP -> FIR (across symbol boundaries)
               -> kept channel samples y (HBM) + sum|y|^2 / PAPR statistics
    [all-reduce of the statistics across ranks]
    ofdm_rx  : y + AWGN (sigma from the global mean power) -> FFT(ortho) -> ZF/MMSE
               -> slicer -> XOR/popcount against the tx bits -> u64 counters
    [all-reduce of the counters across ranks]

Bit / noise sources:
  * reference mode -- the caller passes the reference's packed PCG64 bytes and its
    legacy-RNG normals (the whole serial stream): integer counts are bit-exact with
    the reference;
  * philox mode    -- bits and noise are generated inside the kernels from a
    counter-based Philox4x32-10 keyed by (seed, global symbol), so nothing but y
    touches HBM and results do not depend on the number of GPUs.

Multi-GPU: symbols [r*S/R, (r+1)*S/R) go to rank r; the only exchanges are one
all-gather of the 40-byte ofdm_stats record per rank (the AWGN power is a whole-stream
mean, noise/models.py:14, kept as an exact fixed-point sum so that sigma does not depend
on the rank count) and one all-reduce of the two u64 counters -- with ``profile=True`` of the
counters and the per-subcarrier record behind them (integers: the sum is exact).

Fused route (``fused=``, :meth:`LinkEngine.run_async`): where the plan has a fused form -- complex128,
N = 1024, fixed 64-QAM, cyclic-prefix OFDM, flat channel, no equaliser -- a Philox run is

    ofdm_tx(y = None) : the power pass -- the statistics alone, nothing stored
    [all-gather of the statistics]
    ofdm_link         : every symbol transmitted and received in registers -> u64 counters

with no y in HBM at all and the same results bit for bit.

SNR sweeps: :meth:`LinkEngine.run_sweep` transmits once and receives at every SNR of a list in one
pass (ofdm_rx_sweep); point k is ``run(n_sym, snr_k, seed=seed)``.  :meth:`LinkEngine.run_frame_sweep`
does the same with the per-frame error record of every point (ofdm_rx_sweep_frames): point k is
``run(n_sym, snr_k, seed=seed, frame_symbols=F)`` -- an FER-versus-SNR curve from one transmit.

Clipping: ``LinkEngine(..., clip_db=...)`` limits the envelope of the modulated samples at that level
above the nominal sample power (ofdm_tx_clip: a soft limiter directly after the IFFT, before the guard
and the channel); every run of the engine then transmits the limited stream, its statistics describe it,
and LinkStats carries the count of limited samples (integers, all-reduced behind the error counters).

Constellation density: ``run(..., density=G)`` also bins every equalised point of the run into a G x G
grid over a square of the I/Q plane (ofdm_rx_density: 32-bit bins in LDS per workgroup, integer atomics
into a uint64 record behind the counters); :class:`ConstellationDensity` carries it.

Soft decisions: ``run(..., soft=B)`` also bins, for every compared bit, the max-log distance difference
in units of the subcarrier's squared minimum distance into a histogram conditioned on the transmitted bit
(ofdm_rx_soft: integers, behind the counters like the density); :class:`SoftDecisions` carries it and
computes the LLR histograms and the bit-wise mutual information (GMI) from it on the host.

PAPR distribution: :meth:`LinkEngine.papr` bins the per-symbol PAPR of the stream ``run`` transmits
(ofdm_papr: the transmitter's map and IFFT, no channel, no receiver) into an integer histogram on the
device; :class:`PaprStats` carries it and its CCDF.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from ofdm_based_systems import _backend as B

DEFAULT_Y_BUDGET = 64 << 30  # bytes of kept channel samples held at once per GPU


@dataclass
class SubcarrierProfile:
    """Per-subcarrier results of a whole run (``ofdm_rx_profile``, include/ofdm_hip.h), accumulated
    on the device in integers: identical for any batching and rank count."""
    bit_errors: np.ndarray           # int64 [N]; sums to LinkStats.bit_errors
    symbol_errors: np.ndarray        # int64 [N]; sums to LinkStats.symbol_errors
    clipped: np.ndarray              # int64 [N]: samples whose |z - c|^2 reached 2^20 or was not finite
    error_power: np.ndarray          # float64 [N]: sum over the symbols of min(|z - c|^2, 2^20)
    error_power_fx: np.ndarray       # int64 [2][N]: error_power's exact 32-bit limbs, units of 2^-40
    n_symbols: int                   # OFDM symbols of the run
    bits_per_subcarrier: np.ndarray  # int64 [N]; 0 = inactive (every row zero there)

    @property
    def ber(self) -> np.ndarray:
        """Bit error rate per subcarrier (NaN where inactive).  The denominator is every bit the
        subcarrier carried; an adaptive run's trailing partial byte is not compared (valid_bits)."""
        den = (self.n_symbols * self.bits_per_subcarrier).astype(np.float64)
        return np.divide(self.bit_errors, den, out=np.full(len(den), np.nan), where=den > 0)

    @property
    def ser(self) -> np.ndarray:
        """Symbol error rate per subcarrier (NaN where inactive)."""
        den = np.where(self.bits_per_subcarrier > 0, float(self.n_symbols), 0.0)
        return np.divide(self.symbol_errors, den, out=np.full(len(den), np.nan), where=den > 0)

    @property
    def mer_db(self) -> np.ndarray:
        """Modulation error ratio -10 log10(error_power / n_symbols) in dB: the LUTs have unit
        power, so this is the post-equaliser SNR of the subcarrier (NaN where inactive)."""
        out = np.full(len(self.error_power), np.nan)
        act = (self.bits_per_subcarrier > 0) & (self.n_symbols > 0)
        with np.errstate(divide="ignore"):
            out[act] = -10.0 * np.log10(self.error_power[act] / max(self.n_symbols, 1))
        return out


@dataclass
class FrameStats:
    """Per-frame error counts of a whole run (``ofdm_rx_frames``, include/ofdm_hip.h): a frame is
    ``frame_symbols`` consecutive global OFDM symbols, frame f holding symbols [f F, (f + 1) F).
    Accumulated on the device in integers: identical for any batching and rank count.  The arrays
    cover every frame the run touches; the derived quantities the ``n_full`` full frames only -- a
    trailing partial frame stays in the arrays and out of the rates."""
    frame_symbols: int          # F
    n_symbols: int              # OFDM symbols of the run
    bits_per_symbol: int        # bits one OFDM symbol carries
    bit_errors: np.ndarray      # int64 [ceil(n_symbols / F)]; sums to LinkStats.bit_errors
    symbol_errors: np.ndarray   # int64 [ceil(n_symbols / F)]; sums to LinkStats.symbol_errors
    # bits of the run that were compared (LinkEngine.valid_bits, or the caller's n_valid_bits); None:
    # all of them
    n_valid_bits: Optional[int] = None

    @property
    def n_full(self) -> int:
        """Full frames of the run: n_symbols // F."""
        return self.n_symbols // self.frame_symbols

    @property
    def frame_errors(self) -> int:
        """Full frames with at least one bit error."""
        return int(np.count_nonzero(self.bit_errors[:self.n_full] > 0))

    @property
    def fer(self) -> Optional[float]:
        """Frame error rate over the full frames; None without one."""
        return self.frame_errors / self.n_full if self.n_full else None

    def errors_per_frame_hist(self) -> np.ndarray:
        """hist[e] = full frames with exactly e bit errors (``np.bincount``)."""
        return np.bincount(self.bit_errors[:self.n_full])

    @property
    def ber_stderr(self) -> Optional[float]:
        """Standard error of the run's BER from the spread of the error count across the n full
        frames, sqrt(sum (e_f - mean)^2 / (n (n - 1))) / (F bits per symbol): valid when bit errors
        cluster inside a frame.  None with fewer than two full frames, or when ``n_valid_bits`` leaves
        a bit of the run uncompared (the frames then do not compare the same number of bits)."""
        n = self.n_full
        if n < 2 or self.frame_symbols * self.bits_per_symbol == 0:
            return None
        if self.n_valid_bits is not None and self.n_valid_bits < self.n_symbols * self.bits_per_symbol:
            return None
        e = self.bit_errors[:n].astype(np.float64)
        var = float(np.sum((e - e.mean()) ** 2)) / (n * (n - 1))
        return math.sqrt(var) / (self.frame_symbols * self.bits_per_symbol)


def frame_count(n_sym: int, frame_symbols) -> int:
    """Frames a run of n_sym OFDM symbols touches, ceil(n_sym / F) (at least one record row); ValueError
    for an F below 1 or a record above B.MAX_FRAMES frames."""
    if isinstance(frame_symbols, bool) or int(frame_symbols) != frame_symbols or int(frame_symbols) < 1:
        raise ValueError(f"frame_symbols = {frame_symbols!r} is not a positive number of OFDM symbols")
    n = max(1, -(-int(n_sym) // int(frame_symbols)))
    if n > B.MAX_FRAMES:
        raise ValueError(f"frame_symbols = {frame_symbols} gives {n} frames over {n_sym} OFDM symbols, above the "
                         f"cap of {B.MAX_FRAMES} (2^24 frames, a 256 MiB record); use longer frames or shorter runs")
    return n


@dataclass
class ConstellationDensity:
    """Where the received points of a whole run fall in the I/Q plane (``ofdm_rx_density``,
    include/ofdm_hip.h): every equalised point of the subcarriers in ``subcarriers`` binned into a G x G
    grid over the square [-extent, extent)^2.  Accumulated on the device in integers: identical for any
    batching and rank count."""
    counts: np.ndarray     # int64 [G][G]: row = imaginary bin, column = real bin
    outside: int           # points outside the square (NaN and infinities among them)
    extent: float          # L
    n_points: int          # counts.sum() + outside
    subcarriers: tuple     # (k_lo, k_hi): the subcarriers binned, [k_lo, k_hi)

    @property
    def bins(self) -> int:
        return int(self.counts.shape[0])

    @property
    def edges(self) -> np.ndarray:
        """float64 [G + 1]: the bin edges of either axis, -L + 2 L j / G (for plotting; the device's
        index is floor((c + L) * (G / (2 L))), see :func:`density_grid`)."""
        G = self.bins
        return -self.extent + (2.0 * self.extent / G) * np.arange(G + 1, dtype=np.float64)

    def to_image(self, scale: int = 4):
        """A PIL heat map ("L") of log(1 + counts), the imaginary axis pointing up, every bin
        ``scale`` x ``scale`` pixels."""
        from PIL import Image

        lg = np.log1p(self.counts.astype(np.float64))
        top = float(lg.max())
        px = np.zeros(lg.shape, np.uint8) if top == 0.0 else np.round(255.0 * lg / top).astype(np.uint8)
        img = Image.fromarray(px[::-1].copy())  # (uint8, two axes: mode "L")
        return img.resize((self.bins * int(scale),) * 2, Image.NEAREST) if scale != 1 else img


def density_grid(bins, extent) -> tuple:
    """(lo, inv_w) of ofdm_rx_density's grid from G bins per axis over [-L, L): lo = -L and
    inv_w = G / (2 L), formed here in double (the library never sees L).  ValueError for a G outside
    [1, B.MAX_DENSITY_BINS] or an L that is not finite and positive."""
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= B.MAX_DENSITY_BINS:
        raise ValueError(f"density = {bins!r} is not a number of bins per axis in [1, {B.MAX_DENSITY_BINS}] "
                         "(more than 128 bins per axis are not built)")
    L = float(extent)
    if not (math.isfinite(L) and L > 0.0):
        raise ValueError(f"density_extent = {extent!r} is not a finite positive extent")
    return -L, int(bins) / (2.0 * L)


def soft_grid(bins, extent=8.0) -> float:
    """inv_w = B / (2 L) of ofdm_rx_soft's histograms: B bins over [-L, L) in units of the subcarrier's
    squared minimum distance, formed here in double (the library never sees L).  B is even, so zero is a
    bin line.  ValueError for a B that is not an even number in [2, B.MAX_SOFT_BINS] or an L that is not
    finite and positive."""
    if isinstance(bins, bool) or int(bins) != bins or not 2 <= int(bins) <= B.MAX_SOFT_BINS or int(bins) % 2:
        raise ValueError(f"soft = {bins!r} is not an even number of bins in [2, {B.MAX_SOFT_BINS}] "
                         "(more than 256 bins are not built)")
    L = float(extent)
    if not (math.isfinite(L) and L > 0.0):
        raise ValueError(f"soft_extent = {extent!r} is not a finite positive extent")
    return int(bins) / (2.0 * L)


def soft_orders(luts: Sequence[np.ndarray]) -> None:
    """ValueError unless every LUT is a separable square QAM of order 4, 16, 64 or 256 -- LUT[i] =
    I[i & (side - 1)] + j Q[i >> hb] -- the constellations the soft record is built for."""
    for l in luts:
        l = np.asarray(l, np.complex128)
        m = len(l)
        if m > 256:
            raise ValueError(f"soft: a constellation above 256 points ({m}) has no soft record (not built)")
        hb = (m.bit_length() - 1) // 2
        sq = m in (4, 16, 64, 256) and np.array_equal(l.reshape(1 << hb, 1 << hb).real, np.tile(l[:1 << hb].real, (1 << hb, 1))) \
            and np.array_equal(l.reshape(1 << hb, 1 << hb).imag, np.tile(l[::1 << hb].imag[:, None], (1, 1 << hb))) \
            and len(np.unique(l[:1 << hb].real)) == 1 << hb and len(np.unique(l[::1 << hb].imag)) == 1 << hb
        if not sq:
            raise ValueError(f"soft: a non-separable (PSK) or non-square constellation of {m} points has no soft "
                             "record (not built: square QAM of order 4, 16, 64 or 256 only)")


def soft_scale(luts: Sequence[np.ndarray], sc_lut, weights, h_raw, n_fft: int) -> np.ndarray:
    """float64 [N]: ofdm_rx_soft's scale table g[k] = w_k / step_k^2.  step_k = (max I level - min I
    level) / (side - 1) of subcarrier k's LUT, in double; an inactive subcarrier has g = 0.  ``weights``:
    None: w = 1; "csi": w_k = |H_k|^2 / max |H|^2 with H = fft(h_raw, N), the equaliser's H; an array of N
    finite non-negative floats: taken as given.  ValueError for anything else."""
    soft_orders(luts)
    N = int(n_fft)
    inv2 = []
    for l in luts:
        re = np.asarray(l, np.complex128).real
        side = 1 << ((len(l).bit_length() - 1) // 2)
        step = (float(re.max()) - float(re.min())) / (side - 1)
        inv2.append(1.0 / (step * step))
    inv2 = np.array(inv2, np.float64)
    if sc_lut is None:
        base = np.full(N, inv2[0], np.float64)
    else:
        sc = np.asarray(sc_lut, np.int64)
        base = np.where(sc >= 0, inv2[np.maximum(sc, 0)], 0.0)
    if weights is None:
        w = np.ones(N, np.float64)
    elif isinstance(weights, str):
        if weights != "csi":
            raise ValueError(f"soft_weights = {weights!r} is not None, \"csi\" or an array of {N} weights")
        p = np.abs(np.fft.fft(np.asarray(h_raw, np.complex128), N)) ** 2
        top = float(p.max())
        if not (math.isfinite(top) and top > 0.0):
            raise ValueError("soft_weights = \"csi\": the channel response has no finite positive maximum")
        w = p / top
    else:
        w = np.asarray(weights, np.float64)
        if w.shape != (N,) or not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError(f"soft_weights is not None, \"csi\" or an array of {N} finite non-negative floats")
    return np.ascontiguousarray(w * base, dtype=np.float64)


@dataclass
class SoftDecisions:
    """The soft decisions of a whole run (``ofdm_rx_soft``, include/ofdm_hip.h): for every compared bit the
    max-log distance difference D = min over the points with bit 1 - min over the points with bit 0 of the
    squared distance, per axis, times the subcarrier's weight over its squared level spacing, binned into B
    bins over [-extent, extent) (the end bins saturate) and conditioned on the transmitted bit.  A positive
    value favours bit 0.  Accumulated on the device in integers: identical for any batching and rank count.
    Row (b/2)(b/2 - 1) + i holds bit i (MSB first) of the subcarriers with b bits."""
    counts: np.ndarray     # int64 [20][2][B]: row, transmitted bit, bin
    invalid: int           # bits whose value was NaN (a ZF point on a null bin)
    bins: int              # B
    extent: float          # L
    subcarriers: tuple     # (k_lo, k_hi): the subcarriers counted, [k_lo, k_hi)
    n_bits: int            # counts.sum() + invalid: the compared bits in range

    ORDERS = (2, 4, 6, 8)  # bits per subcarrier of the orders the record has rows for

    @staticmethod
    def row0(b: int) -> int:
        if b not in SoftDecisions.ORDERS:
            raise ValueError(f"b = {b!r} is not 2, 4, 6 or 8 bits per subcarrier")
        return (b // 2) * (b // 2 - 1)

    def rows(self, b: int) -> np.ndarray:
        """int64 [b][2][B]: the rows of the subcarriers with b bits, bit 0 (the MSB) first."""
        return self.counts[self.row0(b):self.row0(b) + b]

    @property
    def orders(self) -> tuple:
        """The b whose rows hold anything."""
        return tuple(b for b in self.ORDERS if self.rows(b).any())

    @property
    def hard_bit_errors(self) -> int:
        """The mass on the wrong side of zero: tx bit 0 in bins < B/2 plus tx bit 1 in bins >= B/2 -- the
        hard decisions' bit errors, as long as no value is exactly undecided."""
        h = self.bins // 2
        return int(self.counts[:, 0, :h].sum() + self.counts[:, 1, h:].sum())

    @property
    def llr_centres(self) -> np.ndarray:
        """float64 [B]: the bin centres (j - B/2 + 0.5) 2 L / B, in the record's unit."""
        return (np.arange(self.bins, dtype=np.float64) - self.bins / 2 + 0.5) * (2.0 * self.extent / self.bins)

    def _row_info(self, rows: np.ndarray, s: float) -> np.ndarray:
        """float64 [rows]: 1 - sum counts log2(1 + exp(-(1 - 2 v) s centre)) / n_row (0 for an empty row)."""
        x = s * self.llr_centres
        pen = np.stack([np.logaddexp(0.0, -x), np.logaddexp(0.0, x)]) / math.log(2.0)  # [tx bit][bin]
        n = rows.sum(axis=(1, 2)).astype(np.float64)
        loss = (rows * pen[None]).sum(axis=(1, 2))
        return np.where(n > 0, 1.0 - loss / np.maximum(n, 1.0), 0.0)

    def gmi_scale(self, b: int) -> float:
        """The s >= 0 in [1e-2, 1e3] that maximises the order's GMI: a golden-section search on log s (the
        sum is concave in s, so it has one maximum)."""
        rows = self.rows(b)
        f = lambda t: float(self._row_info(rows, math.exp(t)).sum())
        lo, hi = math.log(1e-2), math.log(1e3)
        q = (math.sqrt(5.0) - 1.0) / 2.0
        x1, x2 = hi - q * (hi - lo), lo + q * (hi - lo)
        f1, f2 = f(x1), f(x2)
        for _ in range(80):
            if f1 < f2:
                lo, x1, f1 = x1, x2, f2
                x2 = lo + q * (hi - lo)
                f2 = f(x2)
            else:
                hi, x2, f2 = x2, x1, f1
                x1 = hi - q * (hi - lo)
                f1 = f(x1)
        cands = [math.log(1e-2), 0.5 * (lo + hi), math.log(1e3)]
        return math.exp(max(cands, key=f))

    def gmi_per_bit(self, b: int, scale: Optional[float] = None) -> np.ndarray:
        """float64 [b]: the mutual information of each bit of the subcarriers with b bits, in bits (the
        mismatched-decoding GMI of the binned values read as LLRs s * value; ``scale`` None: the s that
        maximises their sum)."""
        s = self.gmi_scale(b) if scale is None else float(scale)
        return self._row_info(self.rows(b), s)

    def gmi(self, b: Optional[int] = None, scale: Optional[float] = None) -> float:
        """The bit-wise mutual information (BICM rate) in bits per subcarrier use of the subcarriers with b
        bits: sum over their rows of 1 - sum counts log2(1 + exp(-(1 - 2 v) s centre)) / n_row, with
        ``scale`` None at the s >= 0 that maximises it -- it needs no noise variance.  b None: over every
        order of the run, the total rate per OFDM symbol divided by the active subcarriers, one s per order
        (a run of one order: that order's)."""
        if b is not None:
            return float(self.gmi_per_bit(b, scale).sum())
        # subcarrier uses of an order: the bits of its first row
        use = {o: int(self.rows(o)[0].sum()) for o in self.ORDERS}
        total = sum(use.values())
        if total == 0:
            return 0.0
        return float(sum(use[o] * self.gmi(o, scale) for o in self.ORDERS if use[o]) / total)


@dataclass
class LinkStats:
    bit_errors: int
    symbol_errors: int
    num_ofdm_symbols: int
    power_sum: float      # sum |y|^2 over the whole serial stream (all ranks)
    x_power_sum: float    # sum |x|^2 over the modulated stream incl. prefix
    x_peak: float         # max |x|^2
    samples: int          # S * (N + cp)
    papr_db: float
    received: Optional[np.ndarray] = None
    timings: dict = field(default_factory=dict)
    profile: Optional[SubcarrierProfile] = None  # run(..., profile=True)
    # an engine with a clip level (LinkEngine(clip_db=...)); None without one
    clip_db: Optional[float] = None
    clipped_samples: Optional[int] = None  # samples whose |x|^2 exceeded the threshold
    clip_samples: Optional[int] = None     # samples examined: N per OFDM symbol
    frames: Optional[FrameStats] = None    # run(..., frame_symbols=F)
    density: Optional[ConstellationDensity] = None  # run(..., density=G)
    soft: Optional[SoftDecisions] = None   # run(..., soft=B)


def default_papr_edges_db() -> np.ndarray:
    """The default edge grid of :meth:`LinkEngine.papr`: -0.125 + 0.25 j dB, j < 64.  It keeps 0 dB out
    of the edge set: constant-envelope waveforms sit at exactly 0 dB, and an edge there would be
    decided by rounding."""
    return -0.125 + 0.25 * np.arange(64, dtype=np.float64)


@dataclass
class PaprStats:
    """The distribution of the per-symbol PAPR of a run (``ofdm_papr``, include/ofdm_hip.h), binned on
    the device in integers: identical for any batching and rank count.  Bin j counts the symbols whose
    ratio peak * n / sum lies in [edge j-1, edge j); bin 0 lies below the first edge, bin K at or
    above the last (a symbol without power among them)."""
    edges_db: np.ndarray                     # float64 [K], strictly increasing
    histogram: np.ndarray                    # int64 [K + 1]; sums to num_ofdm_symbols
    num_ofdm_symbols: int
    per_symbol: Optional[np.ndarray] = None  # float64 (keep, 2): (max |x|^2, sum |x|^2) of the kept symbols
    samples_per_symbol: int = 0              # n = N + cp (the prefix or the zero guard counts)

    @property
    def ccdf(self) -> np.ndarray:
        """float64 [K]: ccdf[i] = sum_{j > i} histogram[j] / S = P(ratio >= edge i)."""
        h = np.asarray(self.histogram, dtype=np.int64)
        above = np.cumsum(h[::-1])[::-1][1:]
        return above.astype(np.float64) / max(int(self.num_ofdm_symbols), 1)

    @property
    def papr_db_per_symbol(self) -> Optional[np.ndarray]:
        """10 log10(peak n / sum) of the kept symbols (inf for a symbol without power), or None."""
        if self.per_symbol is None:
            return None
        ps = np.asarray(self.per_symbol, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(ps[:, 1] > 0, ps[:, 0] * self.samples_per_symbol / ps[:, 1], np.inf)
            return 10.0 * np.log10(ratio)


def new_stats(dev) -> torch.Tensor:
    """A zeroed ofdm_stats record (include/ofdm_hip.h): power_sum, x_power_sum, x_peak as
    float64 and the two int64 fixed-point limbs of sum |y|^2, 5 x 8 bytes."""
    return torch.zeros(B.STATS_WORDS, dtype=torch.float64, device=dev)


def combine_stats(stats: torch.Tensor, parts) -> None:
    """Reduce every rank's ofdm_stats record into ``stats`` (the same on every rank): the
    fixed-point power limbs add as integers -- exact, so power_sum and sigma equal the
    single-GPU values bit for bit -- then power_sum is recomputed from them as the kernels do;
    sum |x|^2 adds in rank order, max |x|^2 is the maximum."""
    g = torch.stack(list(parts))                      # (world, 5) float64
    limbs = g.view(torch.int64)[:, 3:5].sum(0)        # exact
    l0 = limbs[0] & 0xFFFFFFFF
    l1 = limbs[1] + (limbs[0] >> 32)
    si = stats.view(torch.int64)
    si[3] = l0
    si[4] = l1
    stats[0] = l1.to(torch.float64) * B.FX_HI + l0.to(torch.float64) * B.FX_LO
    stats[1] = g[:, 1].sum()
    stats[2] = g[:, 2].max()


def combine_profile(parts) -> np.ndarray:
    """Add profile records (int64 [5][N] each: a rank's, or a batch's) and normalise the
    error-power limbs as combine_stats does: rows 2 / 3 are 32-bit limbs in units of 2^-40
    (ofdm_stats.power_fx's format) that every workgroup adds to without carrying, so row 3 takes
    row 2's carry and row 2 keeps its low 32 bits.  Integer arithmetic: exact in any order."""
    rec = np.sum([np.asarray(p, dtype=np.int64) for p in parts], axis=0, dtype=np.int64)
    rec[3] += rec[2] >> 32
    rec[2] &= 0xFFFFFFFF
    return rec


def profile_power(rec: np.ndarray) -> np.ndarray:
    """The error-vector power of a normalised record (combine_profile), as fx_value on the device."""
    return rec[3].astype(np.float64) * B.FX_HI + rec[2].astype(np.float64) * B.FX_LO


def nominal_sample_power(n_fft: int, luts: Sequence[np.ndarray], sc_lut=None) -> float:
    """P_nom = (1/N) sum_k mean_i |LUT_l(k)[i]|^2 in double, k ascending, inactive subcarriers
    contributing 0: the nominal mean power of a time sample (include/ofdm_hip.h, ofdm_tx_clip)."""
    mean = [float(np.mean(np.abs(np.asarray(l, np.complex128)) ** 2)) for l in luts]
    total = 0.0
    for k in range(n_fft):
        l = 0 if sc_lut is None else int(sc_lut[k])
        total += mean[l] if l >= 0 else 0.0
    return total / n_fft


def clip_threshold(clip_db: float, nominal_power: float) -> float:
    """A2 = 10^(clip_db / 10) P_nom, the threshold on |x|^2 (finite and positive, or ValueError)."""
    try:
        a2 = 10.0 ** (float(clip_db) / 10.0) * nominal_power
    except OverflowError:
        a2 = math.inf
    if not (math.isfinite(a2) and a2 > 0.0):
        raise ValueError(f"clip_db = {clip_db!r} gives no finite positive threshold (nominal power {nominal_power})")
    return a2


def shard(n: int, rank: int, world: int) -> tuple:
    """Contiguous [lo, hi) share of n items for one rank."""
    lo = (n * rank) // world
    hi = (n * (rank + 1)) // world
    return lo, hi


def _world_rank(group) -> tuple:
    """(world size, rank) of a process group; (1, 0) without one."""
    if group is None:
        return 1, 0
    import torch.distributed as dist

    return dist.get_world_size(group), dist.get_rank(group)


@dataclass
class _Share:
    """This rank's share [lo, hi) of a run of global OFDM symbols [0, n_sym), and what every kernel
    call of the run is given."""
    dev: torch.device
    stream: object
    world: int
    lo: int
    hi: int
    samples: int  # of the whole run: n_sym * (N + cp)
    n_valid: int  # bits compared, of the whole run

    @property
    def mine(self) -> int:
        return self.hi - self.lo


@dataclass(frozen=True)
class _Record:
    """One record kind of the receiver, described once: the int64 words it takes in a run's buffer (_acc), what
    it hands :meth:`LinkEngine.rx`, the receiver's event name with it, and how ``result()`` reads it."""
    shape: tuple     # of the record; .words: their product
    event: str
    field: str       # of LinkStats
    rx_kw: object    # the device record -> rx()'s keyword arguments
    decode: object   # (the record on the host, int64; n_sym) -> the field's value
    info: tuple = ()
    words = property(lambda self: math.prod(self.shape))


def _profile_record(n_fft: int, bits_per_subcarrier) -> _Record:
    """ofdm_rx_profile's record, int64 [5][N] (the events keep ofdm_rx's name)."""
    def decode(rec, n_sym):
        rec = combine_profile([rec])
        return SubcarrierProfile(bit_errors=rec[0], symbol_errors=rec[1], clipped=rec[4],
                                 error_power=profile_power(rec), error_power_fx=rec[2:4].copy(),
                                 n_symbols=n_sym, bits_per_subcarrier=bits_per_subcarrier)

    return _Record((B.PROFILE_ROWS, n_fft), "ofdm_rx", "profile", lambda rec: {"profile": rec}, decode)


def _frames_record(n_frames: int, frame_symbols: int, bps: int, n_valid: int, points: tuple = ()) -> _Record:
    """ofdm_rx_frames' record, int64 [n_frames][2]; with ``points`` = (K,) ofdm_rx_sweep_frames' [K][n_frames][2],
    which PendingSweep decodes point by point.  info: (F, bits per OFDM symbol, bits compared)."""
    F = int(frame_symbols)

    def decode(rec, n_sym):
        rec = rec[:-(-n_sym // F)]  # (an empty run: no frame)
        return FrameStats(frame_symbols=F, n_symbols=n_sym, bits_per_symbol=bps, bit_errors=rec[:, 0].copy(),
                          symbol_errors=rec[:, 1].copy(), n_valid_bits=n_valid)

    return _Record(points + (n_frames, 2), "ofdm_rx_sweep_frames" if points else "ofdm_rx_frames", "frames",
                   lambda rec: {"frames": rec, "frame_symbols": F}, decode, (F, bps, n_valid))


def _density_record(grid: tuple, subcarriers: tuple) -> _Record:
    """ofdm_rx_density's record, int64 [G * G + 1]; grid: (lo, inv_w, G) of :func:`density_grid`."""
    G, L = grid[2], -grid[0]

    def decode(rec, n_sym):
        return ConstellationDensity(counts=rec[:G * G].reshape(G, G).copy(), outside=int(rec[G * G]), extent=L,
                                    n_points=int(rec.sum()), subcarriers=subcarriers)

    return _Record((G * G + 1,), "ofdm_rx_density", "density",
                   lambda rec: {"density": rec, "density_params": grid, "density_subcarriers": subcarriers}, decode)


def _soft_record(g, inv_w: float, bins: int, extent: float, subcarriers: tuple) -> _Record:
    """ofdm_rx_soft's record, int64 [20 * 2 * B + 1]; g: the device scale table of :func:`soft_scale`."""
    Bn = int(bins)
    cells = B.SOFT_ROWS * 2 * Bn

    def decode(rec, n_sym):
        return SoftDecisions(counts=rec[:cells].reshape(B.SOFT_ROWS, 2, Bn).copy(), invalid=int(rec[cells]), bins=Bn,
                             extent=extent, subcarriers=subcarriers, n_bits=int(rec.sum()))

    return _Record((cells + 1,), "ofdm_rx_soft", "soft",
                   lambda rec: {"soft": rec, "soft_params": (g, inv_w, Bn), "soft_subcarriers": subcarriers}, decode)


class LinkEngine:
    plan = None    # the libofdm_hip plan (set by __init__)
    _fused = None  # has_fused, asked of the library once per engine
    # the fused link's float32 screens (link()): everything None = ofdm_link (the noise screen with the
    # sparse slicer, automatic).  screen_mode, a B.LINK_SCREEN_* mode = ofdm_link_screen (the two-transform
    # screen), counting into screen_counts (device int64 [2], or None); nscreen_mode / nscreen_counts = the
    # same for ofdm_link_nscreen (the noise screen); sparse_mode / sparse_counts (device int64 [4]: symbols
    # screened, redone, quads tested, sliced) for ofdm_link_sparse.  One pair at a time; the counts of a
    # run do not depend on any.
    screen_mode = None
    screen_counts = None
    nscreen_mode = None
    nscreen_counts = None
    sparse_mode = None
    sparse_counts = None
    # (mode attribute, counts attribute, library function), in link()'s order
    _LINK_SCREENS = (("screen_mode", "screen_counts", "ofdm_link_screen"),
                     ("nscreen_mode", "nscreen_counts", "ofdm_link_nscreen"),
                     ("sparse_mode", "sparse_counts", "ofdm_link_sparse"))
    # the soft limiter (ofdm_tx_clip): the level in dB above nominal_power, and the threshold on |x|^2
    # handed to the library; None = no limiter, ofdm_tx as before
    clip_db = None
    clip_a2 = None
    _nominal = None  # (nominal_sample_power's arguments until first asked for, then its value)

    @property
    def nominal_power(self) -> Optional[float]:
        """The nominal mean power of a time sample (:func:`nominal_sample_power`); computed when first
        asked for -- at construction only on an engine with a clip level."""
        if isinstance(self._nominal, tuple):
            self._nominal = nominal_sample_power(*self._nominal)
        return self._nominal

    @nominal_power.setter
    def nominal_power(self, value) -> None:
        self._nominal = value

    def __init__(self, n_fft: int, cp: int, h_raw: np.ndarray, equalizer: int, luts: Sequence[np.ndarray],
                 sc_lut: Optional[np.ndarray] = None, precision: int = B.OFDM_F64,
                 prefix: int = B.PREFIX_CYCLIC, modulator: int = B.MOD_OFDM, clip_db: Optional[float] = None):
        """prefix: cyclic prefix (or none, cp = 0) or zero padding; modulator: OFDM or
        single-carrier OFDM; non-square constellations (PSK) are decided by
        brute-force nearest point.

        clip_db: limit the envelope of the modulated samples (after the IFFT, before the guard and
        the channel) at ``clip_db`` dB above the nominal mean power of a time sample
        (:func:`nominal_sample_power`); None: a linear transmitter."""
        self._nominal = (n_fft, list(luts), sc_lut)
        # what a soft record's scale table is made of (soft_scale)
        self._soft_src = (list(luts), sc_lut, np.asarray(h_raw, np.complex128))
        # max over the LUT pool of max(|re|, |im|): the default extent of a density record is 1.5 of it
        self.lut_reach = max(float(max(np.max(np.abs(np.real(l))), np.max(np.abs(np.imag(l))))) for l in luts)
        if clip_db is not None:
            self.clip_db, self.clip_a2 = float(clip_db), clip_threshold(clip_db, self.nominal_power)
            if max(len(l) for l in luts) > 256:
                raise ValueError("clip_db: a constellation above 256 points has no clipped transmitter "
                                 "(ofdm_tx_clip takes orders up to 256)")
        self.plan = B.Plan(n_fft=n_fft, cp=cp, precision=precision, equalizer=equalizer, luts=list(luts),
                           sc_lut=sc_lut, h_raw=np.asarray(h_raw, np.complex128), prefix=prefix,
                           modulator=modulator)
        self.n_fft = n_fft
        self.cp = cp
        # stored channel samples per OFDM symbol: the post-prefix N, or all N + cp with
        # zero padding (the receiver overlap-adds the guard)
        self.ystride = n_fft + cp if prefix == B.PREFIX_ZERO else n_fft
        self.bps = self.plan.bits_per_ofdm_symbol
        self.adaptive = self.plan.adaptive
        self.cdtype = self.plan.cdtype
        # bits per subcarrier (0 = inactive), for the per-subcarrier profile's rates
        orders = np.array([int(len(l)).bit_length() - 1 for l in luts], dtype=np.int64)
        if sc_lut is None:
            self.bits_per_subcarrier = np.full(n_fft, orders[0], dtype=np.int64)
        else:
            sc = np.asarray(sc_lut, dtype=np.int64)
            self.bits_per_subcarrier = np.where(sc >= 0, orders[np.maximum(sc, 0)], 0).astype(np.int64)
        self._lib = B.lib()

    # ------------------------------------------------------------------ helpers
    def device(self) -> torch.device:
        return B.device()

    def stream(self):
        return B.stream_ptr()

    def upload(self, a: np.ndarray) -> torch.Tensor:
        a = np.ascontiguousarray(a)
        if not a.flags.writeable:  # e.g. np.frombuffer(bytes): torch wants a writable array
            a = a.copy()
        return torch.from_numpy(a).to(self.device())

    def valid_bits(self, n_sym: int) -> int:
        """Bits the reference compares: all of them in FIXED mode, whole bytes in adaptive mode
        (AdaptiveConstellationMapper.decode drops a partial byte, constellation/adaptive.py:259-263)."""
        total = n_sym * self.bps
        return (total // 8) * 8 if self.adaptive else total

    @staticmethod
    def _timed(events, name, n_sym, fn):
        if events is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        events.append((name, n_sym, e0, e1))

    def tx(self, stream, bits_d, seed, sym0, n_sym, y, stats, clip_counters=None):
        """ofdm_tx, or on an engine with a clip level ofdm_tx_clip at its threshold, counting into
        ``clip_counters`` (device int64 [2], accumulated; None: nothing is counted)."""
        args = (self.plan.handle, stream, B.ptr(bits_d), int(seed), int(sym0), int(n_sym), B.ptr(y), B.ptr(stats))
        if self.clip_a2 is None:
            B.check(self._lib.ofdm_tx(*args))
        else:
            B.check(self._lib.ofdm_tx_clip(*args, float(self.clip_a2), B.ptr(clip_counters)))

    def rx(self, stream, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits_d, sym0, n_sym,
           n_valid, counters, z_out=None, z_keep=0, profile=None, frames=None, frame_symbols=None,
           density=None, density_params=None, density_subcarriers=None,
           soft=None, soft_params=None, soft_subcarriers=None):
        """ofdm_rx, or with a profile record (device int64 [5][N]) ofdm_rx_profile, or with a frame
        record (``frames``: device int64 [n_frames][2] of the whole run, ``frame_symbols`` OFDM symbols
        per frame) ofdm_rx_frames, or with a density record (``density``: device int64 [G * G + 1],
        ``density_params``: (lo, inv_w, G), ``density_subcarriers``: (k_lo, k_hi)) ofdm_rx_density, or with a
        soft record (``soft``: device int64 [40 B + 1], ``soft_params``: (g: device float64 [N], inv_w, B),
        ``soft_subcarriers``: (k_lo, k_hi)) ofdm_rx_soft."""
        args = (self.plan.handle, stream, B.ptr(y), B.ptr(nr), B.ptr(ni), int(seed), B.ptr(stats),
                int(total_samples), float(snr_db), int(noise_on), B.ptr(bits_d), int(sym0), int(n_sym),
                int(n_valid), B.ptr(counters), B.ptr(z_out), int(z_keep))
        if soft is not None:
            if profile is not None or frames is not None or density is not None:
                raise ValueError("rx: a soft record together with another record has no kernel")
            g, inv_w, bins = soft_params
            B.check(self._lib.ofdm_rx_soft(*args, B.ptr(g), float(inv_w), int(bins), int(soft_subcarriers[0]),
                                           int(soft_subcarriers[1]), B.ptr(soft)))
        elif density is not None:
            if profile is not None or frames is not None:
                raise ValueError("rx: a density record together with a profile or a frame record has no kernel")
            lo, inv_w, G = density_params
            B.check(self._lib.ofdm_rx_density(*args, float(lo), float(inv_w), int(G), int(density_subcarriers[0]),
                                              int(density_subcarriers[1]), B.ptr(density)))
        elif frames is not None:
            if profile is not None:
                raise ValueError("rx: a profile and a frame record together have no kernel (PROF x FRAMES is not built)")
            B.check(self._lib.ofdm_rx_frames(*args, int(frame_symbols), int(frames.shape[0]), B.ptr(frames)))
        elif profile is None:
            B.check(self._lib.ofdm_rx(*args))
        else:
            B.check(self._lib.ofdm_rx_profile(*args, B.ptr(profile)))

    def rx_sweep(self, stream, y, seed, stats, total_samples, snr_dbs, sym0, n_sym, n_valid, counters,
                 frames=None, frame_symbols=None):
        """ofdm_rx_sweep: the receiver at every SNR of ``snr_dbs`` (at most B.MAX_SWEEP_POINTS, a host
        list copied at the call) over the same y; counters: device int64 [len(snr_dbs)][2], accumulated.
        With a frame record (``frames``: device int64 [len(snr_dbs)][n_frames][2], the points' rows of
        the whole run, contiguous; ``frame_symbols`` OFDM symbols per frame) ofdm_rx_sweep_frames."""
        if frames is not None and (frames.dim() != 3 or frames.shape[0] != len(snr_dbs) or frames.shape[2] != 2
                                   or not frames.is_contiguous()):
            raise ValueError("rx_sweep: the frame record is not a contiguous int64 [len(snr_dbs)][n_frames][2]")
        snrs = (ctypes.c_double * len(snr_dbs))(*[float(q) for q in snr_dbs])
        args = (self.plan.handle, stream, B.ptr(y), int(seed), B.ptr(stats), int(total_samples), snrs, len(snr_dbs),
                int(sym0), int(n_sym), int(n_valid), B.ptr(counters))
        if frames is None:
            B.check(self._lib.ofdm_rx_sweep(*args))
        else:
            B.check(self._lib.ofdm_rx_sweep_frames(*args, int(frame_symbols), int(frames.shape[1]), B.ptr(frames)))

    def link(self, stream, seed, stats, total_samples, snr_db, noise_on, sym0, n_sym, n_valid, counters):
        """ofdm_link: transmit and receive symbols [sym0, sym0 + n_sym) in one kernel, y never leaving
        the registers; ``stats`` holds the whole stream's record (a power pass, :meth:`tx` with y = None).
        With :attr:`screen_mode` set (B.LINK_SCREEN_*), ofdm_link_screen in that mode, adding to
        :attr:`screen_counts` (device int64 [2]: symbols screened, symbols redone) when that is set;
        with :attr:`nscreen_mode` set, ofdm_link_nscreen and :attr:`nscreen_counts` likewise; with
        :attr:`sparse_mode` set, ofdm_link_sparse and :attr:`sparse_counts` (device int64 [4]).  Setting
        anything of more than one pair is an error."""
        pairs = [(getattr(self, mode), getattr(self, counts), fn) for mode, counts, fn in self._LINK_SCREENS]
        if sum(mode is not None or counts is not None for mode, counts, _ in pairs) > 1:
            raise ValueError("screen_mode / screen_counts (ofdm_link_screen), nscreen_mode / nscreen_counts "
                             "(ofdm_link_nscreen) and sparse_mode / sparse_counts (ofdm_link_sparse) are set "
                             "together: one screen at a time")
        args = (self.plan.handle, stream, int(seed), B.ptr(stats), int(total_samples), float(snr_db), int(noise_on),
                int(sym0), int(n_sym), int(n_valid), B.ptr(counters))
        for mode, counts, fn in pairs:
            if mode is not None:
                B.check(getattr(self._lib, fn)(*args, int(mode), B.ptr(counts)))
                return
        B.check(self._lib.ofdm_link(*args))

    def papr_hist(self, stream, bits_d, seed, sym0, n_sym, edges, hist, sym_out=None, sym_keep=0):
        """ofdm_papr: bin the per-symbol PAPR of symbols [sym0, sym0 + n_sym) at ``edges`` (linear ratios,
        strictly increasing, at most B.MAX_PAPR_EDGES: a host list copied at the call) into ``hist``
        (device int64 [len(edges) + 1], accumulated); sym_out: device float64 (sym_keep, 2) or None."""
        e = (ctypes.c_double * len(edges))(*[float(q) for q in edges])
        B.check(self._lib.ofdm_papr(self.plan.handle, stream, B.ptr(bits_d), int(seed), int(sym0), int(n_sym),
                                    e, len(edges), B.ptr(hist), B.ptr(sym_out), int(sym_keep)))

    def papr(self, n_sym: int, *, seed: int = 0, bits: Optional[np.ndarray] = None, edges_db=None,
             keep: int = 0, group=None, batch: Optional[int] = None, events: Optional[list] = None) -> PaprStats:
        """The distribution of the per-symbol PAPR over global OFDM symbols [0, n_sym) of the stream
        :meth:`run` transmits with the same ``seed`` (or ``bits``: the packed tx bytes of the whole
        run, reference mode): the modulated samples before the channel, prefix or zero guard
        included (include/ofdm_hip.h: the definition).  No receiver, no channel, nothing in HBM but the
        histogram.

        edges_db : strictly increasing edges in dB (default: :func:`default_papr_edges_db`), converted
                   to ratios on the host as 10 ** (edges_db / 10); at most B.MAX_PAPR_EDGES
        keep     : keep (max |x|^2, sum |x|^2) of the first ``keep`` symbols of this rank's shard
                   (PaprStats.per_symbol)
        batch    : symbols per launch (default: one launch over the shard)
        group    : the rank's shard of [0, n_sym) is processed here, and the int64 histograms are
                   all-reduced over the group, as the counters are: every rank holds the whole run's
        events   : if a list, ("ofdm_papr", n_symbols, start, end) HIP events are appended per launch
        """
        if self.clip_a2 is not None:
            raise ValueError("papr() on an engine with clip_db: ofdm_papr bins the unclipped stream, and the "
                             "histogram of a clipped one is not built")
        edb = default_papr_edges_db() if edges_db is None else np.asarray(edges_db, dtype=np.float64).reshape(-1)
        edges = 10.0 ** (edb / 10.0)
        r = self._share(n_sym, group)
        bits_d = self._upload_bits(bits, n_sym, r)
        hist = torch.zeros(len(edges) + 1, dtype=torch.int64, device=r.dev)
        kept = max(0, min(int(keep), r.mine))
        sym_out = torch.zeros((kept, 2), dtype=torch.float64, device=r.dev) if kept else None
        per_batch = max(1, int(batch)) if batch else max(r.mine, 1)
        for b0 in range(r.lo, r.hi, per_batch):
            nb = min(per_batch, r.hi - b0)
            off = b0 - r.lo  # the trace: the shard's first symbols, so its first batches
            so = sym_out[off:] if kept > off else None
            self._timed(events, "ofdm_papr", nb, lambda: self.papr_hist(
                r.stream, bits_d, seed, b0, nb, edges, hist, so, kept - off if so is not None else 0))
        if r.mine == 0:  # (an empty shard still answers for the arguments)
            self.papr_hist(r.stream, bits_d, seed, r.lo, 0, edges, hist, None, 0)
        done, work = self._finish(hist, group, r.dev)
        _Pending(n_sym, 0, None, hist, done, work)._wait()
        return PaprStats(edges_db=edb.copy(), histogram=hist.cpu().numpy().astype(np.int64),
                         num_ofdm_symbols=int(n_sym),
                         per_symbol=None if sym_out is None else sym_out.cpu().numpy(),
                         samples_per_symbol=self.n_fft + self.cp)

    @property
    def has_fused(self) -> bool:
        """Whether the plan has a fused form (ofdm_link; include/ofdm_hip.h: complex128, N = 1024, fixed
        64-QAM, cyclic-prefix OFDM, flat channel, no equaliser).  The library decides: an empty
        ofdm_link call answers for the plan before anything is launched."""
        if self._fused is None and self.plan is None:
            self._fused = False  # (no library plan, no library kernel)
        if self._fused is None:
            probe = torch.zeros(2, dtype=torch.int64, device=self.device())
            rc = self._lib.ofdm_link(self.plan.handle, self.stream(), 0, None, 0, 0.0, 0, 0, 0, 0, B.ptr(probe))
            self._fused = rc == 0
        return self._fused

    def _route_fused(self, fused: Optional[bool], *, philox: bool, tap: bool, profile: bool, whole: bool) -> bool:
        """The route of a run: ``fused`` None takes the fused one when the plan has a fused form, the
        streams are Philox, there is no received-symbol tap, no profile (a frame or density record counts
        as one: k_link has none of them) and every bit is compared; False forces the two-kernel path; True raises
        where no fused form exists."""
        clip = self.clip_a2 is not None  # (asked first: a clipped engine never probes the library)
        can = not clip and self.has_fused and philox and not tap and not profile and whole
        if fused and not can:
            raise ValueError("no fused form for this run: ofdm_link takes a complex128 N = 1024 fixed 64-QAM "
                             "cyclic-prefix OFDM plan over a flat channel without equaliser, Philox streams, "
                             "no received-symbol tap, no profile, frame record, density record or soft record and every bit compared, and no clip level "
                             "(clip_db: the limiter is not built into k_link)")
        return can if fused is None else bool(fused)

    def reserve(self, n_sym: int, runs_in_flight: int = 2, group=None, lanes: int = 1) -> None:
        """Allocate, and hand back to torch's caching allocator, the channel-sample buffers of
        ``runs_in_flight`` concurrent runs of n_sym global symbols (run_pipelined keeps two
        alive), so that later runs reuse them instead of paying for a multi-GB hipMalloc; with
        lanes > 1, spread over run_pipelined's lane streams (the allocator pools buffers per
        stream): run k lives on lane k mod lanes, so a lane holds ceil(runs_in_flight / lanes) of
        them at once -- one each with two lanes."""
        if lanes > 1 and self.device().type == "cuda":
            per_lane = -(-runs_in_flight // lanes)
            for st in self.lane_streams(lanes):
                with torch.cuda.stream(st):
                    self.reserve(n_sym, per_lane, group)
            return
        world, rank = _world_rank(group)
        lo, hi = shard(n_sym, rank, world)
        bufs = [self._y(hi - lo) for _ in range(runs_in_flight)]
        del bufs

    # ------------------------------------------------------------------ the schedule's parts
    def _share(self, n_sym: int, group, n_valid_bits: Optional[int] = None) -> _Share:
        world, rank = _world_rank(group)
        lo, hi = shard(n_sym, rank, world)
        n_valid = self.valid_bits(n_sym) if n_valid_bits is None else int(n_valid_bits)
        return _Share(self.device(), self.stream(), world, lo, hi, n_sym * (self.n_fft + self.cp), n_valid)

    def _upload_bits(self, bits, n_sym: int, r: _Share):
        """The caller's packed tx bytes on the device, up to this rank's last symbol (None: Philox bits)."""
        if bits is None:
            return None
        need = math.ceil(n_sym * self.bps / 8)
        if len(bits) < need:
            raise ValueError(f"need {need} tx bytes for {n_sym} OFDM symbols, got {len(bits)}")
        return self.upload(np.asarray(bits, dtype=np.uint8)[: math.ceil(r.hi * self.bps / 8) + 1])

    def _acc(self, n_counters: int, rec: Optional[_Record], dev) -> tuple:
        """A run's one int64 buffer, which one all-reduce carries: the counters, and behind them the clip
        record (an engine with a clip level: [2]) and the record ``rec`` describes (profile, frames or density;
        every rank adds its own symbols' counts into the whole run's).  (buffer, counters, clip, record)."""
        nclip = 0 if self.clip_a2 is None else 2
        acc = torch.zeros(n_counters + nclip + (rec.words if rec else 0), dtype=torch.int64, device=dev)
        return (acc, acc[:n_counters], acc[n_counters:n_counters + nclip] if nclip else None,
                acc[n_counters + nclip:].view(rec.shape) if rec else None)

    def _y(self, n_sym: int) -> torch.Tensor:
        """The kept channel samples of n_sym OFDM symbols."""
        return torch.empty((max(n_sym, 1), self.ystride), dtype=self.cdtype, device=self.device())

    def _ybytes(self) -> int:
        """Bytes of y per OFDM symbol."""
        return self.ystride * (8 if self.cdtype == torch.complex64 else 16)

    @staticmethod
    def _finish(acc: torch.Tensor, group, dev) -> tuple:
        """The end of a run: the asynchronous all-reduce of its counters ``acc`` -- off the critical
        path: the next run's TX does not wait for it, result() does before reading the counters -- and
        the ``done`` event on the launch stream (result() may be called under another stream)."""
        work = None
        if group is not None:
            import torch.distributed as dist

            work = dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group, async_op=True)
        done = None
        if dev.type == "cuda":
            done = torch.cuda.Event()
            done.record()
        return done, work

    def _schedule(self, r: _Share, seed, bits_d, stats, receive, acc, *, group, y_budget, batch, events,
                  link=None, clip=None) -> tuple:
        """The schedule of run_async and run_sweep_async for this rank's share: the fused route when
        ``link`` is given (run_async decided it, _route_fused) -- the power pass ``tx(y=None)`` over the
        shard, the statistics all-gather, then ``link()``: one ofdm_link over the whole shard, with no y
        buffer and no batching whatever ``y_budget`` and ``batch`` say -- and otherwise the whole shard
        resident -- one TX, one receive -- or, when its y exceeds ``y_budget`` (or ``batch`` says so),
        a power pass first (the AWGN power is a whole-stream mean) and then TX + receive per batch;
        between TX and the first receive the one statistics all-gather, at the end the counters'
        all-reduce (_finish, whose (done, work) are returned).  ``receive(y, sym0, n, resident)``
        enqueues the receiver(s) of symbols [sym0, sym0 + n) held in y; TX is timed into ``events``
        on the resident path only.  ``clip`` (an engine with a clip level: the record, device int64
        [2] inside ``acc``) goes to the one transmit that covers every symbol once -- the resident
        one, or the power pass -- and the batch transmits count nothing."""
        stream = r.stream
        # (tx without a clip level is called as before)
        count = {} if self.clip_a2 is None else {"clip_counters": clip}
        quiet = {} if self.clip_a2 is None else {"clip_counters": None}

        def reduce_stats():
            # one collective on the TX -> RX critical path: every rank gathers all ranks'
            # ofdm_stats records and reduces them (combine_stats), so all ranks hold the
            # statistics -- and sigma -- of a single-GPU run, bit for bit
            # (run with any process group, one rank included: a 1-rank RCCL group exercises the
            # same collectives, tests/test_gpu_multirank.py)
            if group is not None:
                import torch.distributed as dist

                parts = [torch.empty_like(stats) for _ in range(r.world)]
                dist.all_gather(parts, stats, group=group)
                combine_stats(stats, parts)

        if link is not None:
            self._timed(events, "ofdm_tx", r.mine, lambda: self.tx(stream, bits_d, seed, r.lo, r.mine, None, stats))
            reduce_stats()
            link()
            return self._finish(acc, group, r.dev)
        per_batch = batch or max(1, min(r.mine, y_budget // self._ybytes()))
        if per_batch >= r.mine:
            y = self._y(r.mine)
            self._timed(events, "ofdm_tx", r.mine,
                        lambda: self.tx(stream, bits_d, seed, r.lo, r.mine, y, stats, **count))
            reduce_stats()
            receive(y, r.lo, r.mine, True)
        else:
            self.tx(stream, bits_d, seed, r.lo, r.mine, None, stats, **count)
            reduce_stats()
            scratch = new_stats(r.dev)
            y = self._y(per_batch)
            for b0 in range(r.lo, r.hi, per_batch):
                nb = min(per_batch, r.hi - b0)
                self.tx(stream, bits_d, seed, b0, nb, y, scratch, **quiet)
                receive(y, b0, nb, False)
        return self._finish(acc, group, r.dev)

    # ------------------------------------------------------------------ run
    def run(self, n_sym: int, snr_db: float, **kw) -> LinkStats:
        """Simulate global OFDM symbols [0, n_sym) and return the counts (see :meth:`run_async`)."""
        return self.run_async(n_sym, snr_db, **kw).result()

    def run_async(self, n_sym: int, snr_db: float, *, bits: Optional[np.ndarray] = None,
                  normals: Optional[tuple] = None, seed: int = 0, noise_on: bool = True, keep_symbols: int = 0,
                  group=None, y_budget: int = DEFAULT_Y_BUDGET, batch: Optional[int] = None,
                  n_valid_bits: Optional[int] = None, events: Optional[list] = None,
                  profile: bool = False, fused: Optional[bool] = None,
                  frame_symbols: Optional[int] = None, density: Optional[int] = None,
                  density_extent: Optional[float] = None,
                  density_subcarriers: Optional[tuple] = None, soft: Optional[int] = None,
                  soft_extent: Optional[float] = None, soft_weights=None,
                  soft_subcarriers: Optional[tuple] = None) -> "PendingLink":
        """Enqueue global OFDM symbols [0, n_sym) (this rank's shard when ``group`` is set) on
        the current stream without waiting for them; :meth:`PendingLink.result` reads the
        counts back.  Back-to-back calls therefore keep the GPU busy while the host prepares
        the next batch.

        bits    : packed tx bytes of the whole run (reference mode) or None (Philox)
        normals : (nr, ni) float64 arrays of length n_sym*(N+cp) (reference mode), or None
                  for Philox noise
        events  : if a list, (kernel, n_symbols, start, end) HIP events are appended around
                  every ofdm_tx / ofdm_rx launch (recorded on the launch stream); with frame_symbols the
                  receiver's are named "ofdm_rx_frames", with density "ofdm_rx_density"
        profile : accumulate the per-subcarrier record of the whole run (LinkStats.profile): bit and
                  symbol errors, error-vector power and clipped samples per subcarrier, summed on the
                  device in integers by every batch and, with a group, over the ranks -- exact, so
                  the same for any batching and rank count.  ofdm_rx_profile: the complex128 bench
                  shapes with Philox streams and keep_symbols = 0 run their throughput receiver with
                  the profile compiled in, every other run the generic receiver; run_pipelined takes
                  no profile.
        frame_symbols : F: accumulate the per-frame error record of the whole run (LinkStats.frames):
                  the bit and symbol errors of every frame of F consecutive global OFDM symbols, int64
                  [ceil(n_sym / F)][2] behind the counters, from which come the frame error rate, the
                  BER's standard error and the errors-per-frame histogram (:class:`FrameStats`).  Each
                  batch and each rank adds its own symbols' counts -- integers, so a frame split over
                  two batches or two ranks just sums and the record is the same for any batching and
                  rank count.  ofdm_rx_frames: the complex128 bench shapes with Philox streams and
                  keep_symbols = 0 run their throughput receiver with the record compiled in, every
                  other run the generic receiver.  At most B.MAX_FRAMES frames; not together with
                  ``profile``; the fused route has no record (None takes the two-kernel path).
        density : G: accumulate the constellation density of the whole run (LinkStats.density,
                  :class:`ConstellationDensity`): every equalised point -- the value the tap stores --
                  binned into a G x G grid (G <= B.MAX_DENSITY_BINS) over the square [-L, L)^2, int64
                  [G * G + 1] behind the counters (the last word counts the points outside).
                  ``density_extent``: L (default 1.5 times the largest |re| or |im| of the plan's LUT
                  pool); ``density_subcarriers``: (k_lo, k_hi), only subcarriers k_lo <= k < k_hi are
                  binned (default the whole symbol).  ofdm_rx_density: the complex128 bench shapes with
                  Philox streams and keep_symbols = 0 run their throughput receiver with the record
                  compiled in, every other run the generic receiver -- a run with a tap on all its
                  batches (the later ones are handed the tap buffer with z_keep = 0), so the record of
                  any run is the same for every batching and rank count, exactly.  Not together with
                  ``profile`` or ``frame_symbols``; the fused route has no record (None takes the
                  two-kernel path).
        soft    : B: accumulate the soft decisions of the whole run (LinkStats.soft, :class:`SoftDecisions`):
                  for every compared bit the max-log distance difference, in units of the subcarrier's
                  squared minimum distance, binned into B bins (even, <= B.MAX_SOFT_BINS) over [-L, L) and
                  conditioned on the transmitted bit, int64 [20][2][B] + 1 behind the counters (the last
                  word counts NaN values).  ``soft_extent``: L (default 8); ``soft_weights``: None, "csi"
                  (|H_k|^2 / max |H|^2) or N non-negative floats (:func:`soft_scale`);
                  ``soft_subcarriers``: (k_lo, k_hi).  Square QAM of order 4 to 256 only, fixed or
                  adaptive.  ofdm_rx_soft, routed as the density (a run with a tap: the generic receiver on
                  all its batches).  Not together with ``profile``, ``frame_symbols`` or ``density``; the
                  fused route has no record (None takes the two-kernel path).
        fused   : the route.  None: the fused one -- a power pass, then one ofdm_link launch that
                  transmits and receives every symbol of the shard in registers: no y buffer, no
                  batching -- when the plan has a fused form (has_fused), the streams are Philox
                  and there is no tap, no profile and no partial n_valid_bits; the same counts and
                  statistics, bit for bit.  False: the two-kernel path.  True: ValueError where no
                  fused form exists.  Events: ("ofdm_tx", ...) for the power pass, ("ofdm_link", ...).
        """
        n_frames = 0
        if frame_symbols is not None:
            if profile:
                raise ValueError("profile=True together with frame_symbols: the receiver with both records "
                                 "(PROF x FRAMES) is not built; run twice")
            n_frames = frame_count(n_sym, frame_symbols)
        dgrid = None
        if density is not None:
            if profile:
                raise ValueError("profile=True together with density: the receiver with both records "
                                 "(PROF x DENS) is not built; run twice")
            if frame_symbols is not None:
                raise ValueError("frame_symbols together with density: the receiver with both records "
                                 "(FRAMES x DENS) is not built; run twice")
            L = 1.5 * self.lut_reach if density_extent is None else float(density_extent)
            dgrid = density_grid(density, L) + (int(density),)
            drange = (0, self.n_fft) if density_subcarriers is None else tuple(int(k) for k in density_subcarriers)
            if len(drange) != 2 or not 0 <= drange[0] < drange[1] <= self.n_fft:
                raise ValueError(f"density_subcarriers = {density_subcarriers!r} is not a range "
                                 f"0 <= k_lo < k_hi <= {self.n_fft}")
        elif density_extent is not None or density_subcarriers is not None:
            raise ValueError("density_extent / density_subcarriers without density")
        sgrid = None
        if soft is not None:
            for other, name in ((profile, "profile=True"), (frame_symbols is not None, "frame_symbols"),
                                (density is not None, "density")):
                if other:
                    raise ValueError(f"{name} together with soft: the receiver with both records is not built; "
                                     "run twice")
            sL = 8.0 if soft_extent is None else float(soft_extent)
            sgrid = (soft_grid(soft, sL), int(soft), sL)
            srange = (0, self.n_fft) if soft_subcarriers is None else tuple(int(k) for k in soft_subcarriers)
            if len(srange) != 2 or not 0 <= srange[0] < srange[1] <= self.n_fft:
                raise ValueError(f"soft_subcarriers = {soft_subcarriers!r} is not a range "
                                 f"0 <= k_lo < k_hi <= {self.n_fft}")
            luts, sc_lut, h_raw = self._soft_src
            g_host = soft_scale(luts, sc_lut, soft_weights, h_raw, self.n_fft)  # (PSK, wide plans: ValueError)
        elif soft_extent is not None or soft_weights is not None or soft_subcarriers is not None:
            raise ValueError("soft_extent / soft_weights / soft_subcarriers without soft")
        r = self._share(n_sym, group, n_valid_bits)
        dev, N = r.dev, self.n_fft
        # the run's record, at most one (the pairs were refused above)
        rec = (_profile_record(N, self.bits_per_subcarrier) if profile else
               _frames_record(n_frames, frame_symbols, self.bps, r.n_valid) if n_frames else
               _density_record(dgrid, drange) if dgrid else
               _soft_record(self.upload(g_host), sgrid[0], sgrid[1], sgrid[2], srange) if sgrid else None)
        use_link = self._route_fused(fused, philox=bits is None and normals is None, tap=keep_symbols > 0,
                                     profile=rec is not None, whole=r.n_valid >= n_sym * self.bps)

        bits_d = self._upload_bits(bits, n_sym, r)
        nr_d = ni_d = None
        if normals is not None and noise_on:
            nr_d = self.upload(np.asarray(normals[0], np.float64))
            ni_d = self.upload(np.asarray(normals[1], np.float64))

        stats = new_stats(dev)
        acc, counters, clip, record = self._acc(2, rec, dev)
        pkw = rec.rx_kw(record) if rec else {}  # (rx without a record is called as before)
        keep = min(keep_symbols, r.mine)
        z_out = torch.empty((keep, N), dtype=self.cdtype, device=dev) if keep else None
        rx_name = rec.event if rec else "ofdm_rx"

        def receive(y, sym0, n, resident):
            zk = keep if sym0 == r.lo else 0  # the tap: the shard's first symbols, so its first batch
            # (a density record: the later batches of a run with a tap keep the tap buffer, z_keep = 0, so
            # that every batch takes the generic receiver -- one form per run, ofdm_rx_density)
            zo = z_out if zk or dgrid or sgrid else None
            self._timed(events if resident else None, rx_name, n, lambda: self.rx(
                r.stream, y, nr_d, ni_d, seed, stats, r.samples, snr_db, noise_on, bits_d, sym0, n, r.n_valid,
                counters, zo, zk, **pkw))

        def link():
            self._timed(events, "ofdm_link", r.mine, lambda: self.link(
                r.stream, seed, stats, r.samples, snr_db, noise_on, r.lo, r.mine, r.n_valid, counters))

        done, work = self._schedule(r, seed, bits_d, stats, receive, acc, group=group, y_budget=y_budget,
                                    batch=batch, events=events, link=link if use_link else None, clip=clip)
        return PendingLink(n_sym, r.samples, stats, counters, done, work, clip, self.clip_db, record, rec, z_out)

    # ------------------------------------------------------------------ one-pass SNR sweep
    def run_sweep(self, n_sym: int, snr_dbs, **kw) -> list:
        """A BER curve from one transmit: the counts of :meth:`run` at every SNR of ``snr_dbs`` (see
        :meth:`run_sweep_async`), one LinkStats per point in the order given."""
        return self.run_sweep_async(n_sym, snr_dbs, **kw).result()

    def run_sweep_async(self, n_sym: int, snr_dbs, *, seed: int = 0, group=None,
                        y_budget: int = DEFAULT_Y_BUDGET, batch: Optional[int] = None,
                        n_valid_bits: Optional[int] = None, events: Optional[list] = None,
                        frame_symbols: Optional[int] = None, density: Optional[int] = None,
                        soft: Optional[int] = None) -> "PendingSweep":
        """Throughput-mode (Philox) runs of global OFDM symbols [0, n_sym) at every SNR of
        ``snr_dbs`` with one seed, from one transmit: point k is ``run(n_sym, snr_dbs[k], seed=seed)``
        -- the same bits, noise words, sigma and per-sample arithmetic, so in complex128 the same
        counts -- but the stream is transmitted, written and read once per batch, and the receiver
        (``ofdm_rx_sweep``) draws each symbol's noise words once for all points.  The points share
        their noise realisation (common random numbers: a smooth, monotone curve).

        The schedule is :meth:`run_async`'s (_schedule), with the [K][2] counters all-reduced.  A list
        longer than B.MAX_SWEEP_POINTS is split into several receiver launches over the same y.  The
        counts do not depend on the batching, the rank count, the order of the list or how it is split.

        Not taken: caller bits or normals, orders above 256, a profile, a frame record
        (``frame_symbols``: ValueError -- :meth:`run_frame_sweep_async` is the sweep with one), a density
        record (``density``: ValueError), a received-symbol tap, and a plan per point (adaptive loading
        re-derived per SNR)."""
        if soft is not None:
            raise ValueError("run_sweep with soft: the sweep receiver keeps no soft record "
                             "(the soft decisions inside k_rx_sweep are not built); use run per point")
        if density is not None:
            raise ValueError("run_sweep with density: the sweep receiver keeps no density record "
                             "(the density inside k_rx_sweep is not built); use run per point")
        if frame_symbols is not None:
            raise ValueError("run_sweep with frame_symbols: run_sweep keeps no frame record; the sweep with "
                             "the record of every point is run_frame_sweep / run_frame_sweep_async")
        return self._sweep_async("run_sweep", n_sym, snr_dbs, None, seed=seed, group=group, y_budget=y_budget,
                                 batch=batch, n_valid_bits=n_valid_bits, events=events)

    def run_frame_sweep(self, n_sym: int, snr_dbs, frame_symbols: int, **kw) -> list:
        """An FER curve from one transmit: :meth:`run` with ``frame_symbols`` at every SNR of ``snr_dbs``
        (see :meth:`run_frame_sweep_async`), one LinkStats per point in the order given."""
        return self.run_frame_sweep_async(n_sym, snr_dbs, frame_symbols, **kw).result()

    def run_frame_sweep_async(self, n_sym: int, snr_dbs, frame_symbols: int, *, seed: int = 0, group=None,
                              y_budget: int = DEFAULT_Y_BUDGET, batch: Optional[int] = None,
                              n_valid_bits: Optional[int] = None, events: Optional[list] = None,
                              soft: Optional[int] = None) -> "PendingSweep":
        """:meth:`run_sweep_async` with the per-frame error record of every point: point k is
        ``run(n_sym, snr_dbs[k], seed=seed, frame_symbols=F)`` -- its counters as :meth:`run_sweep`
        gives them, and ``.frames`` the :class:`FrameStats` that run builds, with the same
        ``n_valid_bits`` handling -- from one transmit (``ofdm_rx_sweep_frames``).

        The record is int64 [K][ceil(n_sym / F)][2], point-major, behind the [K][2] counters (and the
        clip record) in the one buffer the asynchronous all-reduce carries; every batch and every rank
        adds its own symbols' counts -- integers, so the record does not depend on the batching, the
        rank count, the order of the list, how a list longer than B.MAX_SWEEP_POINTS is split into
        launches (each takes the contiguous rows of its points), or whether a frame straddles any of
        those.  Events are named "ofdm_rx_sweep_frames".

        ValueError before any launch: a bad F or too many frames (:func:`frame_count`), more than
        B.MAX_FRAMES rows over all points (the 256 MiB cap on the whole record), an empty list, a
        non-finite point; otherwise what :meth:`run_sweep_async` does not take is not taken here."""
        if soft is not None:
            raise ValueError("run_frame_sweep with soft: the sweep receiver keeps no soft record "
                             "(the soft decisions inside k_rx_sweep_frames are not built); use run per point")
        return self._sweep_async("run_frame_sweep", n_sym, snr_dbs, frame_symbols, seed=seed, group=group,
                                 y_budget=y_budget, batch=batch, n_valid_bits=n_valid_bits, events=events)

    def _sweep_async(self, who: str, n_sym: int, snr_dbs, frame_symbols, *, seed, group, y_budget, batch,
                     n_valid_bits, events) -> "PendingSweep":
        """run_sweep_async (``frame_symbols`` None) and run_frame_sweep_async: one schedule."""
        n_frames = 0 if frame_symbols is None else frame_count(n_sym, frame_symbols)
        snrs = [float(q) for q in snr_dbs]
        if not snrs:
            raise ValueError(f"{who} needs at least one SNR point")
        if not all(math.isfinite(q) for q in snrs):
            raise ValueError(f"{who} needs finite SNR points")
        K = len(snrs)
        if K * n_frames > B.MAX_FRAMES:
            raise ValueError(f"{who}: frame_symbols = {frame_symbols} gives {n_frames} frames at each of {K} SNR "
                             f"points, {K * n_frames} rows, above the cap of {B.MAX_FRAMES} (2^24 rows, a 256 MiB "
                             "record); use longer frames, shorter runs or fewer points per sweep")
        r = self._share(n_sym, group, n_valid_bits)
        stats = new_stats(r.dev)
        rec = _frames_record(n_frames, frame_symbols, self.bps, r.n_valid, (K,)) if n_frames else None
        acc, counters, clip, frec = self._acc(2 * K, rec, r.dev)  # (the [K][2] counters, the [K][n_frames][2] record)
        counters = counters.view(K, 2)
        rx_name = rec.event if rec else "ofdm_rx_sweep"

        def receive(y, sym0, n, resident):  # (timed per launch on either path)
            for k0 in range(0, K, B.MAX_SWEEP_POINTS):
                k1 = k0 + B.MAX_SWEEP_POINTS
                fkw = rec.rx_kw(frec[k0:k1]) if rec else {}  # (rx_sweep without a frame record is called as before)
                self._timed(events, rx_name, n, lambda: self.rx_sweep(
                    r.stream, y, seed, stats, r.samples, snrs[k0:k1], sym0, n, r.n_valid, counters[k0:k1], **fkw))

        done, work = self._schedule(r, seed, None, stats, receive, acc, group=group, y_budget=y_budget,
                                    batch=batch, events=events, clip=clip)
        return PendingSweep(n_sym, r.samples, stats, counters, done, work, clip, self.clip_db, frec, rec)

    def lane_streams(self, lanes: int) -> list:
        """The current stream and lanes - 1 more, kept per engine (their allocator pools persist:
        reserve() fills them before a timed region)."""
        if lanes <= 1 or self.device().type != "cuda":
            return [None]
        cur = torch.cuda.current_stream()
        extra = getattr(self, "_lanes", [])
        while len(extra) < lanes - 1:
            extra.append(torch.cuda.Stream())
        self._lanes = extra
        return [cur] + extra[:lanes - 1]

    def run_pipelined(self, n_sym: int, snr_db, seeds, *, group=None,
                      events: Optional[list] = None, y_budget: int = DEFAULT_Y_BUDGET, lanes: int = 1,
                      fused: Optional[bool] = None, frame_symbols: Optional[int] = None,
                      density: Optional[int] = None, soft: Optional[int] = None) -> list:
        """Independent throughput-mode runs (one per seed) of global OFDM symbols [0, n_sym),
        software-pipelined across runs: run k+1's TX is enqueued before run k's RX, so with
        several ranks the statistics exchange of run k (the one collective on a run's
        TX -> RX path) is in flight while the GPU transmits run k+1.  Every run is complete
        and its counts are those of :meth:`run_async` with the same seed; returns the
        PendingLink of each run.  Two runs' channel samples are live at once; when they do not
        fit ``y_budget`` the runs go through :meth:`run_async` one after another (batched).

        snr_db: one SNR for every run, or one per seed -- an SNR sweep (the reference's one
        Simulation per SNR point, simulation/models.py:190-211, run in order by main.py:234-239),
        its points pipelined the same way (the SNR enters only the receiver).

        lanes: HIP streams the runs alternate over (run k on lane k mod lanes, each run's TX,
        exchanges and RX in order on its lane): with 2, one run's receiver overlaps the next run's
        transmitter -- the launch tails and the one-workgroup statistics kernel between them of
        short runs (a sweep's points) fill with the other lane's work.  One y buffer per lane.

        fused: as :meth:`run_async`.  On the fused route a run is a power pass and one ofdm_link
        launch, pipelined and laned in the same way (run k+1's power pass before run k's link), with
        no y buffer: ``y_budget`` does not matter."""
        if self.clip_a2 is not None:
            raise ValueError("run_pipelined on an engine with clip_db: the pipelined schedule carries no clip "
                             "record; use run_async or run_sweep")
        if frame_symbols is not None:
            raise ValueError("run_pipelined with frame_symbols: the pipelined schedule carries no frame record; "
                             "use run_async")
        if soft is not None:
            raise ValueError("run_pipelined with soft: the pipelined schedule carries no soft record; "
                             "use run_async")
        if density is not None:
            raise ValueError("run_pipelined with density: the pipelined schedule carries no density record; "
                             "use run_async")
        seeds = list(seeds)
        snrs = list(snr_db) if isinstance(snr_db, (list, tuple, np.ndarray)) else [snr_db] * len(seeds)
        if len(snrs) != len(seeds):
            raise ValueError("one SNR per seed")
        r = self._share(n_sym, group)
        dev, lo, mine = r.dev, r.lo, r.mine
        use_link = self._route_fused(fused, philox=True, tap=False, profile=False, whole=True)
        if not use_link and 2 * max(mine, 1) * self._ybytes() > y_budget:
            return [self.run_async(n_sym, q, seed=s, group=group, events=events, y_budget=y_budget, fused=False)
                    for s, q in zip(seeds, snrs)]

        lane_list = self.lane_streams(lanes) if lanes > 1 and dev.type == "cuda" else None

        def on(k):
            """Context of run k's lane (the current stream when not alternating)."""
            import contextlib

            return torch.cuda.stream(lane_list[k % len(lane_list)]) if lane_list else contextlib.nullcontext()

        def tx(k):
            seed = seeds[k]
            with on(k):
                st = self.stream()
                stats = new_stats(dev)
                y = None if use_link else self._y(mine)  # (fused: the power pass)
                self._timed(events, "ofdm_tx", mine, lambda: self.tx(st, None, seed, lo, mine, y, stats))
                work = None
                if group is not None:
                    import torch.distributed as dist

                    parts = [torch.empty_like(stats) for _ in range(r.world)]
                    work = (dist.all_gather(parts, stats, group=group, async_op=True), parts)
            return seed, y, stats, work

        def rx(state, snr, k):
            with on(k):
                return rx_on(state, snr, self.stream())

        def rx_on(state, snr, stream):
            seed, y, stats, work = state
            if work is not None:  # reduce the gathered statistics (as _schedule)
                work[0].wait()
                combine_stats(stats, work[1])
            counters = torch.zeros(2, dtype=torch.int64, device=dev)
            if use_link:
                self._timed(events, "ofdm_link", mine, lambda: self.link(
                    stream, seed, stats, r.samples, snr, True, lo, mine, r.n_valid, counters))
            else:
                self._timed(events, "ofdm_rx", mine, lambda: self.rx(
                    stream, y, None, None, seed, stats, r.samples, snr, True, None, lo, mine, r.n_valid, counters))
            done, red = self._finish(counters, group, dev)
            return PendingLink(n_sym, r.samples, stats, counters, done, red)

        out = []
        cur = tx(0) if seeds else None
        for k in range(len(seeds)):
            nxt = tx(k + 1) if k + 1 < len(seeds) else None
            out.append(rx(cur, snrs[k], k))
            cur = nxt
        return out


class _Pending:
    """Device-side results of a run: its statistics record and counters (of papr(): its histogram), the ``done``
    event of its launch stream and ``work``, its asynchronous counter all-reduce (multi-rank) or None; its clip
    record (a clip level: device int64 [2]); its record and the record's description (_Record); run_async's tap."""

    def __init__(self, n_sym, samples, stats, counters, done=None, work=None, clip=None, clip_db=None,
                 record=None, kind=None, z_out=None):
        self.n_sym, self.samples, self.stats, self.counters = n_sym, samples, stats, counters
        self.done, self.work, self.clip, self.clip_db = done, work, clip, clip_db
        self.record, self.kind, self.z_out = record, kind, z_out

    def _wait(self) -> None:
        if self.done is not None:
            self.done.synchronize()
        if self.work is not None:
            self.work.wait()  # the reduced counters (host-blocking for gloo, stream-ordered for RCCL)
            self.work = None
            if self.counters.is_cuda:
                torch.cuda.current_stream().synchronize()

    def _statistics(self) -> dict:
        """LinkStats' fields from the run's statistics record (the same for every SNR point of a sweep),
        and with a clip level the clip record's."""
        st = self.stats.cpu().numpy()
        avg = st[1] / self.samples if self.samples else 0.0
        papr = float(10 * np.log10(st[2] / avg)) if avg > 0 else float("inf")
        out = dict(num_ofdm_symbols=self.n_sym, power_sum=float(st[0]), x_power_sum=float(st[1]),
                   x_peak=float(st[2]), samples=self.samples, papr_db=papr)
        if self.clip is not None:
            rec = self.clip.cpu().numpy()
            out.update(clip_db=self.clip_db, clipped_samples=int(rec[0]), clip_samples=int(rec[1]))
        return out


class PendingLink(_Pending):
    """Device-side results of one :meth:`LinkEngine.run_async` call."""

    def result(self) -> LinkStats:
        self._wait()
        shared = self._statistics()
        cnt = self.counters.cpu().numpy()
        if self.kind is not None:
            shared[self.kind.field] = self.kind.decode(self.record.cpu().numpy().astype(np.int64), self.n_sym)
        return LinkStats(bit_errors=int(cnt[0]), symbol_errors=int(cnt[1]), **shared,
                         received=None if self.z_out is None else self.z_out.cpu().numpy().reshape(-1))


class PendingSweep(_Pending):
    """Device-side results of one :meth:`LinkEngine.run_sweep_async` call: the [K][2] counters and
    the run's one statistics record; of :meth:`LinkEngine.run_frame_sweep_async` also the
    [K][n_frames][2] frame record."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        # the points' frame records (device int64 [K][n_frames][2]) and (F, bits per OFDM symbol, bits compared)
        self.frames, self.frame_info = self.record, self.kind.info if self.kind else None

    def result(self) -> list:
        """One LinkStats per SNR point, in the order given: the point's counts and the run's shared
        power / PAPR fields."""
        self._wait()
        shared = self._statistics()
        cnt = self.counters.cpu().numpy()
        if self.frames is None:
            return [LinkStats(bit_errors=int(c[0]), symbol_errors=int(c[1]), **shared) for c in cnt]
        rec = self.frames.cpu().numpy().astype(np.int64)
        return [LinkStats(bit_errors=int(c[0]), symbol_errors=int(c[1]), frames=self.kind.decode(p, self.n_sym), **shared)
                for c, p in zip(cnt, rec)]

"""What ofdm_papr must compute (include/ofdm_hip.h: the definition), restated with the oracle's public
functions -- not a test module.

Per global OFDM symbol s the modulated samples x_s[0 .. n), n = N + cp: the constellation map of the
symbol's indices (Philox lane blocks: philox_streams.lane_generators / tx_indices; caller bits: the
oracle's MSB-first map), np.fft.ifft(norm="ortho") for OFDM and nothing for single carrier, the cyclic
prefix (ofdm_oracle.add_cp) or the zero guard.  peak_s = max |x|^2, sum_s = sum |x|^2 in double.

The GPU takes both in its arithmetic precision and in another summation order, so a histogram is not
compared bin by bin but through the **cumulative bracket**: for each edge e and a relative margin d,
``#{r_s >= e (1 + d)} <= sum_{j > i} hist[j] <= #{r_s >= e (1 - d)}`` with r_s = peak n / sum.
  d = 1e-9 in complex128 (three orders over the project's 1e-12 TX sample tolerance),
  d = 1e-3 in complex64 (ten times the 1e-4 rms TX tolerance, which enters peak power about twice).
A complex128 bracket must have width 0 at every edge (the assertion is then equality of the histogram);
a complex64 one at most max(4, 5 % of S), the cap the project uses for complex64 counts.
"""

import numpy as np

import ofdm_oracle as O
import philox_streams as P

DELTA = {"f64": 1e-9, "f32": 1e-3}
TOL = {"f64": 1e-12, "f32": 1e-4}  # per-symbol (peak, sum), relative


def default_edges_db():
    """-0.125 + 0.25 j dB, j < 64: 0 dB is no edge (constant-envelope symbols sit exactly there)."""
    return -0.125 + 0.25 * np.arange(64, dtype=np.float64)


def ratios(edges_db):
    return 10.0 ** (np.asarray(edges_db, np.float64) / 10.0)


def bits_per_subcarrier(luts, sc_lut, N):
    b = np.array([int(len(l)).bit_length() - 1 for l in luts], np.int64)
    if sc_lut is None:
        return np.full(N, b[0], np.int64)
    sc = np.asarray(sc_lut, np.int64)
    return np.where(sc >= 0, b[np.maximum(sc, 0)], 0)


def indices(N, S, luts, sc_lut=None, *, seed=0, bits=None, sym0=0):
    """Constellation indices (S, N) of global symbols [sym0, sym0 + S): the Philox lane blocks, or the
    caller's packed bytes of the whole run (fixed orders: symbol s starts at bit s N b)."""
    bk = bits_per_subcarrier(luts, sc_lut, N)
    if bits is None:
        gen = P.lane_generators(seed, np.arange(sym0, sym0 + S), N)
        return P.tx_indices(gen, S, N, bk if sc_lut is not None else int(bk[0]))
    assert sc_lut is None, "caller bits: fixed orders here"
    b = int(bk[0])
    stream = O.bytes_to_bits(np.asarray(bits, np.uint8))[sym0 * N * b:(sym0 + S) * N * b]
    return O.bits_to_indices(stream, b).reshape(S, N)


def per_symbol(N, cp, S, luts, sc_lut=None, *, seed=0, bits=None, sym0=0, single_carrier=False, zero_pad=False):
    """(peak (S,), sum (S,), n) of the modulated symbols, in double."""
    idx = indices(N, S, luts, sc_lut, seed=seed, bits=bits, sym0=sym0)
    if sc_lut is None:
        X = np.asarray(luts[0], np.complex128)[idx]
    else:
        sc = np.asarray(sc_lut, np.int64)
        X = np.zeros((S, N), np.complex128)
        for l, lut in enumerate(luts):
            k = np.nonzero(sc == l)[0]
            X[:, k] = np.asarray(lut, np.complex128)[idx[:, k]]
    x = X if single_carrier else np.fft.ifft(X, axis=1, norm="ortho")
    if zero_pad:
        x = np.concatenate([x, np.zeros((S, cp), np.complex128)], axis=1)
    else:
        x = O.add_cp(x, cp)
    p = x.real ** 2 + x.imag ** 2
    return p.max(axis=1), p.sum(axis=1), N + cp


def symbol_ratio(peak, total, n):
    """r_s = peak n / sum (inf for a symbol without power: it lies at or above every edge)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total > 0, peak * n / total, np.inf)


def histogram(peak, total, n, edges):
    """The definition itself on given pairs: bin j = #{i : peak n >= edges[i] sum}, in double."""
    lhs = np.asarray(peak, np.float64) * float(n)
    j = (lhs[:, None] >= np.asarray(edges, np.float64)[None, :] * np.asarray(total, np.float64)[:, None]).sum(axis=1)
    return np.bincount(j, minlength=len(edges) + 1).astype(np.int64)


def bracket(peak, total, n, edges, delta):
    """(lo [K], hi [K]): #{r_s >= e (1 + delta)} and #{r_s >= e (1 - delta)} per edge e."""
    r = symbol_ratio(peak, total, n)
    e = np.asarray(edges, np.float64)
    lo = (r[:, None] >= e[None, :] * (1.0 + delta)).sum(axis=0)
    hi = (r[:, None] >= e[None, :] * (1.0 - delta)).sum(axis=0)
    return lo.astype(np.int64), hi.astype(np.int64)


def cumulative(hist):
    """sum_{j > i} hist[j] for i < K."""
    h = np.asarray(hist, np.int64)
    return np.cumsum(h[::-1])[::-1][1:]


def width_cap(precision, S):
    return 0 if precision == "f64" else max(4, int(0.05 * S))


def assert_in_bracket(hist, peak, total, n, edges, precision, what=""):
    """The histogram's cumulative counts inside the bracket, the bracket no wider than its cap."""
    S = len(peak)
    lo, hi = bracket(peak, total, n, edges, DELTA[precision])
    width = int((hi - lo).max())
    print(f"{what} [{precision}] S = {S}: bracket width {width} (cap {width_cap(precision, S)})")
    assert width <= width_cap(precision, S), (what, precision, width)
    cum = cumulative(hist)
    assert int(np.sum(hist)) == S, (what, int(np.sum(hist)), S)
    assert np.all(lo <= cum) and np.all(cum <= hi), (what, precision, np.nonzero((cum < lo) | (cum > hi))[0][:8])


# The width-cap table (CPU) and the GPU cases share these plans.  seed: the Philox seed of the case.
QAM, PSK = O.qam_lut, O.psk_lut


def S_of(N):
    return 32 * 4096 // N + 35  # as the dispatch matrix


def adaptive_2048():
    """N = 2048 adaptive loading over 4 / 16 / 64 / 256-QAM with some order-0 subcarriers."""
    N = 2048
    k = np.arange(N)
    sc = (k // 96) % 5 - 1  # -1 (unused), 0 .. 3, in runs of 96 subcarriers
    return [QAM(4), QAM(16), QAM(64), QAM(256)], sc.astype(np.int32)


CASES = [
    # id, N, cp, luts, kwargs of the engine / the helper, S (None: from the device)
    dict(id="n1024_qam64", N=1024, cp=0, luts=lambda: [QAM(64)], S=None),
    dict(id="n4096_qam256_cp32", N=4096, cp=32, luts=lambda: [QAM(256)], S=67),
    dict(id="n64_qam16_cp16", N=64, cp=16, luts=lambda: [QAM(16)]),
    dict(id="n32_qam64_cp8", N=32, cp=8, luts=lambda: [QAM(64)]),
    dict(id="sc_qam4_n256", N=256, cp=0, luts=lambda: [QAM(4)], sc=True),
    dict(id="sc_zp_qam16_n256_cp64", N=256, cp=64, luts=lambda: [QAM(16)], sc=True, zp=True),
    dict(id="sc_psk8_n64", N=64, cp=0, luts=lambda: [PSK(8)], sc=True),
    dict(id="n2", N=2, cp=0, luts=lambda: [QAM(4)]),
    dict(id="n1", N=1, cp=0, luts=lambda: [QAM(4)]),
]
# further generic-form cases of the GPU tests (several symbols per wave with cp = 0 and cp > TPS,
# N = 8, N = 256, the adaptive N = 2048 shape, BPSK)
MORE_CASES = [
    dict(id="n8_qam16", N=8, cp=2, luts=lambda: [QAM(16)]),
    dict(id="n16_qam16_cp0", N=16, cp=0, luts=lambda: [QAM(16)]),
    dict(id="n16_qam4_cp5", N=16, cp=5, luts=lambda: [QAM(4)]),   # TPS = 1: cp > TPS
    dict(id="n64_qam64_cp0", N=64, cp=0, luts=lambda: [QAM(64)]),
    dict(id="n256_qam16_cp20", N=256, cp=20, luts=lambda: [QAM(16)]),  # TPS = 16: cp > TPS
    dict(id="n2048_adaptive", N=2048, cp=16, luts=None, adaptive=True),
    dict(id="bpsk_n128", N=128, cp=8, luts=lambda: [PSK(2)]),
]
SEED = 2024
THROUGHPUT_SPB = 16  # symbols per workgroup of the throughput form at N = 1024 (1024 threads)


def case_plan(case):
    """(luts, sc_lut) of a case."""
    if case.get("adaptive"):
        return adaptive_2048()
    return case["luts"](), None


def case_symbols(case, compute_units=256):
    """S of a case: the table's, else 32 * 4096 / N + 35; the N = 1024 throughput case two rounds of the
    device's compute units plus a ragged tail (256 compute units: S = 8229)."""
    if case["id"] == "n1024_qam64":
        return 2 * compute_units * THROUGHPUT_SPB + 37
    return case.get("S") or S_of(case["N"])


def case_expect(case, S, **kw):
    luts, sc = case_plan(case)
    return per_symbol(case["N"], case["cp"], S, luts, sc, seed=kw.pop("seed", SEED),
                      single_carrier=case.get("sc", False), zero_pad=case.get("zp", False), **kw)

"""What a clipped throughput-mode run must compute (include/ofdm_hip.h, ofdm_tx_clip: the definition),
restated with the oracle's public functions -- not a test module.

``run_clipped`` is the body of philox_streams.run_philox with the limiter applied to the modulated
samples s_t right after the IFFT (single carrier: to the mapped points), before the guard and the channel:

    p = re^2 + im^2;   x' = x if p <= A2 else x * sqrt(A2 / p)

Everything downstream -- prefix or zero guard, channel, power, noise sigma, receiver, decision brackets --
is computed from x'.  It also returns the clipped-sample count #{p > A2} and its bracket
``#{p > A2 (1 + d)} .. #{p > A2 (1 - d)}``: the GPU forms p in its own arithmetic, so a sample within
rounding of the threshold may fall on either side (the stored sample is the same to the tolerance either
way: the limiter is continuous).  d = papr_expect.DELTA: 1e-9 in complex128, 1e-3 in complex64, with the
same reasoning (orders over the 1e-12 / 1e-4 sample tolerances, which enter |x|^2 about twice).

Width caps: a complex128 count bracket must have width 0 (the assertion is then equality); a complex64 one
at most max(4, samples / 1000) -- for near-Gaussian samples |x|^2 / P is exponential, so the expected share
inside the margin is 2 d t e^-t <= 2 d / e = 0.74e-3 of the samples (t = A2 / P).

The threshold: A2 = 10^(clip_db / 10) P_nom, P_nom = (1/N) sum_k mean_i |LUT_l(k)[i]|^2 in double, inactive
subcarriers contributing 0, k ascending (``nominal_power`` / ``threshold``).

CASES is the one table the CPU width-cap test and the GPU tests share.
"""

from dataclasses import dataclass
from typing import Optional

import numpy as np

import ofdm_oracle as O
import papr_expect as PX
import philox_streams as P

DELTA = PX.DELTA
SEED = 2024


def nominal_power(N, luts, sc_lut=None) -> float:
    mean = [float(np.mean(np.abs(np.asarray(l, np.complex128)) ** 2)) for l in luts]
    total = 0.0
    for k in range(N):
        l = 0 if sc_lut is None else int(sc_lut[k])
        if l >= 0:
            total += mean[l]
    return total / N


def threshold(clip_db, N, luts, sc_lut=None) -> float:
    return 10.0 ** (clip_db / 10.0) * nominal_power(N, luts, sc_lut)


def limit(s_t: np.ndarray, a2: float):
    """(x', p): the limiter of the definition on an array of samples, in double."""
    p = s_t.real ** 2 + s_t.imag ** 2
    over = p > a2
    scale = np.ones_like(p)
    scale[over] = np.sqrt(a2 / p[over])
    return s_t * scale, p


def count_bracket(p: np.ndarray, a2: float, delta: float):
    return int(np.count_nonzero(p > a2 * (1.0 + delta))), int(np.count_nonzero(p > a2 * (1.0 - delta)))


def count_width_cap(precision: str, samples: int) -> int:
    return 0 if precision == "f64" else max(4, samples // 1000)


@dataclass
class ClippedLink:
    bit_errors: int
    symbol_errors: int
    power_sum: float
    x_power_sum: float
    x_peak: float
    idx: np.ndarray
    y: np.ndarray                  # stored channel samples before noise: (S, N) kept, or (S, N + cp) with ZP
    clipped: int                   # #{p > A2}
    samples: int                   # S * N
    p: np.ndarray                  # (S, N) |x|^2 before the limiter
    evm: float                     # mean |Z - X|^2 over the active subcarriers
    bracket: Optional[tuple] = None
    stat_bracket: Optional[tuple] = None

    def count_bracket(self, precision: str, a2: float):
        return count_bracket(self.p, a2, DELTA[precision])


def run_clipped(seed, S, N, M, h_raw, cp, eq, snr_db, a2, noise_on=True, modulator="OFDM", prefix="CP",
                scheme="QAM", orders=None, luts=None, sc_lut=None, precision=None, radius_fn=None, power_sum=None,
                stat_sigma=None, stat_k=P.STAT_K, clip=True, sym0=0) -> ClippedLink:
    """philox_streams.run_philox with the limiter at threshold ``a2`` on |x|^2 (clip=False: without it, the
    same body).  Adaptive loading: either ``orders`` (per-subcarrier QAM / PSK orders, as run_philox) or the
    plan's own ``luts`` / ``sc_lut`` (papr_expect.adaptive_2048).  sym0: global symbols [sym0, sym0 + S), as
    run_philox takes it: on a multipath channel the (limited) symbol sym0 - 1 is generated too and its row
    dropped after the channel; every field covers [sym0, sym0 + S) only."""
    E, tps = P.geometry(N)
    sym0 = int(sym0)
    gen = P.lane_generators(seed, sym0 + np.arange(S, dtype=np.int64), N)
    pre = 1 if (sym0 > 0 and len(np.atleast_1d(h_raw)) > 1) else 0
    genp = P.lane_generators(seed, np.array([sym0 - 1], np.int64), N) if pre else None
    want_bound = precision is not None and noise_on
    prel = 2.0 ** -53 if precision == "f64" else 2.0 ** -24
    if orders is None and sc_lut is not None:
        sizes = np.array([len(l) for l in luts], np.int64)
        sc = np.asarray(sc_lut, np.int64)
        orders = np.where(sc >= 0, sizes[np.maximum(sc, 0)], 0)
    if orders is not None:
        orders = np.asarray(orders, np.int64)
        bk = np.array([int(np.log2(o)) if o > 0 else 0 for o in orders], np.int64)
        idx = P.tx_indices(gen, S, N, bk)
        make = O.psk_lut if scheme == "PSK" else O.qam_lut
        tabs = {int(o): make(int(o)) for o in np.unique(orders) if o > 0}
        ia = np.concatenate([P.tx_indices(genp, 1, N, bk), idx]) if pre else idx
        X = np.zeros((S + pre, N), np.complex128)
        for o, lt in tabs.items():
            cols = orders == o
            X[:, cols] = lt[ia[:, cols]]
    else:
        b = int(np.log2(M))
        lut = O.qam_lut(M) if scheme == "QAM" else O.psk_lut(M)
        idx = P.tx_indices(gen, S, N, b)
        X = lut[np.concatenate([P.tx_indices(genp, 1, N, b), idx]) if pre else idx]
    s_t = np.fft.ifft(X, axis=1, norm="ortho") if modulator == "OFDM" else X
    p_raw = s_t.real ** 2 + s_t.imag ** 2
    if clip:
        s_t, p_raw = limit(s_t, a2)
    p_raw, X = p_raw[pre:], X[pre:]
    if prefix == "ZP":
        x = np.concatenate([s_t, np.zeros((S + pre, cp), np.complex128)], axis=1)
    else:
        x = O.add_cp(s_t, cp)
    px = float(np.sum(np.abs(x[pre:]) ** 2))
    mx = float(np.max(np.abs(x[pre:]) ** 2))
    y = O.channel_conv(x.ravel(), np.asarray(h_raw, np.complex128)).reshape(S + pre, N + cp)[pre:]
    py = float(np.sum(np.abs(y) ** 2))
    if prefix == "ZP":
        yk, tail = y[:, :N].copy(), y[:, N:].copy()
    else:
        yk, tail = y[:, cp:].copy(), None
    rxs = yk.copy()
    nbs = np.zeros((S, N))
    if noise_on:
        pw = (py if power_sum is None else float(power_sum)) / (S * (N + cp))
        sigma = float(np.sqrt((pw / 10 ** (snr_db / 10)) / 2.0))
        if want_bound:
            nz, nb = P.lane_noise(gen, S, N, sigma, with_bound=True, radius_fn=radius_fn, product_rel=prel)
            nbs += nb
        else:
            nz = P.lane_noise(gen, S, N, sigma, radius_fn=radius_fn)
        rxs = rxs + nz
    if prefix == "ZP" and cp > 0:
        if noise_on:
            t = np.tile(np.arange(tps), S)
            for i in range(E):
                k = t + i * tps
                w, ph = gen.noise_draw()
                n, nb = P.noise_from_words(w, ph, sigma, with_bound=True, radius_fn=radius_fn, product_rel=prel)
                use = k < cp
                srow = np.repeat(np.arange(S), tps)[use]
                tail[srow, k[use]] += n[use]
                np.add.at(nbs, (srow, k[use]), nb[use])
        rxs[:, :cp] += tail
    nerr = nbs.sum(axis=1)
    nerr2 = (nbs ** 2).sum(axis=1)
    H = np.fft.fft(np.asarray(h_raw, np.complex128), N)
    Y = np.fft.fft(rxs, axis=1, norm="ortho")
    Z = O.equalize(Y, H, eq, snr_db)
    if modulator == "SC":
        Z = np.fft.ifft(Z, axis=1, norm="ortho")
    bracket = stat_bracket = None
    if precision is not None:
        delta = P.z_error_bound(precision, Y, H, eq, snr_db, nerr, modulator, N, np.sqrt(nerr2))
        dstat = None
        if stat_sigma is not None:
            sig = stat_sigma(y if prefix == "ZP" else yk) if callable(stat_sigma) else float(stat_sigma)
            dstat = P.z_stat_bound(precision, Y, H, eq, snr_db, sig, np.sqrt(np.mean(np.abs(yk) ** 2)),
                                   modulator, N, stat_k)
        if orders is not None:
            bracket = P.adaptive_bracket(Z, idx, orders, bk, delta, scheme, sym0)
            if dstat is not None:
                stat_bracket = P.adaptive_bracket(Z, idx, orders, bk, dstat, scheme, sym0)
        else:
            bracket = P.decision_bracket(Z, idx, lut, b, delta, scheme)
            if dstat is not None:
                stat_bracket = P.decision_bracket(Z, idx, lut, b, dstat, scheme)
    stored = y if prefix == "ZP" else yk
    if orders is not None:
        ridx = np.zeros((S, N), np.int64)
        for o, lt in tabs.items():
            cols = np.flatnonzero(orders == o)
            ridx[:, cols] = O.nn_demap(Z[:, cols].ravel(), lt).reshape(S, len(cols))
        be, se = P.adaptive_counts((ridx ^ idx).astype(np.int64), bk, S, sym0)
        act = orders > 0
        evm = float(np.mean(np.abs(Z[:, act] - X[:, act]) ** 2)) if act.any() else 0.0
    else:
        ridx = O.nn_demap(Z.ravel(), lut).reshape(S, N)
        diff = (ridx ^ idx).astype(np.uint64)
        be = int(sum(int(np.count_nonzero((diff >> np.uint64(j)) & np.uint64(1))) for j in range(b)))
        se = int(np.count_nonzero(ridx != idx))
        evm = float(np.mean(np.abs(Z - X) ** 2))
    return ClippedLink(be, se, py, px, mx, idx, stored, int(np.count_nonzero(p_raw > a2)) if clip else 0, S * N,
                       p_raw, evm, bracket, stat_bracket)


# ------------------------------------------------------------------ the table
QAM, PSK = O.qam_lut, O.psk_lut

# id, N, M, scheme, modulator, prefix, clip_db, S (None: papr_expect.S_of(N)); adaptive: the N = 2048 plan.
# ch (or h: the taps themselves) / cp / eq: the channel fixture, prefix length (None: the channel's order) and equaliser of the GPU
# stored-sample test; the CPU width caps do not depend on them.
# SC clip levels stay off the constellation's own power levels (a threshold equal to a level is a tie):
# 16-QAM points have |x|^2 in {0.2, 1.0, 1.8}, 1 dB = 1.2589; 4-QAM points 1.0, 3 dB = 1.9953.
CASES = [
    dict(id="n64_qam16_3db", N=64, M=16, clip_db=3.0, ch="severe_multipath", cp=7, eq="MMSE"),
    dict(id="n1024_qam64_4db", N=1024, M=64, clip_db=4.0, S=67, ch="flat_fading", eq="NONE", fast=True),
    dict(id="n1024_qam64_1db", N=1024, M=64, clip_db=1.0, S=67, ch="severe_multipath", eq="MMSE", fast=True),
    dict(id="n8_qam16_2db_zp", N=8, M=16, clip_db=2.0, ch="two_ray", cp=2, eq="ZF", prefix="ZP"),
    dict(id="n256_qam16_5db", N=256, M=16, clip_db=5.0, ch="Lin-Phoong_P1", eq="ZF"),
    dict(id="n4096_qam256_3db", N=4096, M=256, clip_db=3.0, S=67, ch="Lin-Phoong_P1", eq="MMSE"),
    dict(id="n2048_adaptive_3db", N=2048, M=0, clip_db=3.0, S=99, adaptive=True, ch="Lin-Phoong_P1", eq="MMSE"),
    dict(id="sc_qam16_n256_1db", N=256, M=16, clip_db=1.0, modulator="SC", ch="Lin-Phoong_P1", eq="ZF"),
    dict(id="sc_qam4_n64_3db", N=64, M=4, clip_db=3.0, modulator="SC", ch="two_ray", eq="ZF"),
    dict(id="n1_qam4_m3db", N=1, M=4, clip_db=-3.0, ch="flat_fading", eq="NONE"),
    dict(id="n2_qam4_05db", N=2, M=4, clip_db=0.5, ch="flat_fading", eq="NONE"),
    dict(id="n16_qam16_cp5_3db", N=16, M=16, clip_db=3.0, ch="severe_multipath", cp=5, eq="MMSE"),
    dict(id="psk8_n64_2db", N=64, M=8, clip_db=2.0, scheme="PSK", ch="two_ray", eq="ZF"),
    # a channel whose first tap is exactly 0 (a leading delay): |h0|^2 = 0, which only the flat throughput
    # form's threshold A2 |h0|^2 would ever see -- and that form takes one-tap channels only
    dict(id="n64_qam16_lead0_3db", N=64, M=16, clip_db=3.0, h=[0.0, 0.8, 0.6j], eq="MMSE"),
    dict(id="n1024_qam64_lead0_4db", N=1024, M=64, clip_db=4.0, S=67, h=[0.0, 0.8, 0.6j], eq="MMSE", fast=True),
    # 4 taps on the complex128 window-FIR shape: the clipped form is the 8-tap kernel, the taps zero past L
    dict(id="n1024_qam64_p1_4db", N=1024, M=64, clip_db=4.0, S=67, ch="Lin-Phoong_P1", eq="MMSE", fast=True),
]


def case_taps(case, fixture):
    """The case's impulse response: its own ``h``, or the channel fixture ``ch`` through ``fixture(name)``."""
    return np.asarray(case["h"], np.complex128) if "h" in case else fixture(case["ch"])


def case_symbols(case) -> int:
    return case.get("S") or PX.S_of(case["N"])


def case_plan(case):
    """(luts, sc_lut) of a case."""
    if case.get("adaptive"):
        return PX.adaptive_2048()
    return [PSK(case["M"]) if case.get("scheme") == "PSK" else QAM(case["M"])], None


def case_threshold(case) -> float:
    luts, sc = case_plan(case)
    return threshold(case["clip_db"], case["N"], luts, sc)


def case_kwargs(case) -> dict:
    """run_clipped's keywords of a case."""
    kw = {k: case[k] for k in ("modulator", "prefix", "scheme") if k in case}
    if case.get("adaptive"):
        luts, sc = case_plan(case)
        kw.update(luts=luts, sc_lut=sc)
    return kw


def case_expect(case, h=None, cp=0, eq="NONE", S=None, seed=SEED, **kw):
    """The noiseless restatement of a case (CPU width caps: a one-tap channel, no prefix)."""
    h = np.array([1.0 + 0j]) if h is None else h
    return run_clipped(seed, S or case_symbols(case), case["N"], case["M"], h, cp, eq, 30.0, case_threshold(case),
                       noise_on=False, **case_kwargs(case), **kw)

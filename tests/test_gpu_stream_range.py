"""The 64-bit halves of the throughput-mode streams on the GPU: symbol indices beyond 2^31, 2^32 and
2^40, seeds with their upper word set, and the supported symbol range (OFDM_MAX_SYMBOLS).

Stream version 3 gives a lane the Philox counter (t, s mod 2^32, s >> 32, kLane) and the key
(seed mod 2^32, seed >> 32).  Every other GPU test runs symbols below a few thousand with seeds below
2^32: the counter's third word and the key's second are zero there, and a kernel that dropped either, or
that formed the global symbol index in 32 bits at one of the four places that form it (k_tx, the
receivers' body, k_link, k_papr), would pass them all -- symbol 2^32 + j would silently repeat symbol j.
Here every entry point that takes ``sym0`` is called directly at

  2^31 - 3   across the int32 sign,
  2^32 - 3   across the counter's word boundary inside one call (and inside one window-FIR group),
  2^32       whose regenerated predecessor is the last index with an all-ones low word,
  2^40 + 5   a high word above 1,

with the seed 0x9E3779B97F4A7C15, and compared with the oracle at that ``sym0``
(philox_streams.run_philox(sym0=...), tests/test_stream_range_cpu.py).  The tolerances are the project's
own (tests/test_gpu_philox_parity.py): transmitted samples within 1e-12 (complex128) / 1e-4 (complex64) of
the oracle's rms, complex128 decision brackets of width 0 and counts equal to the oracle's, complex64
counts inside the rigorous and the statistical bracket, the power within 1e-12 / 1e-5.  Every call's
``stats`` is the record of ``tx`` over the same [sym0, sym0 + S) with total_samples = S (N + cp), and the
oracle is handed that power.
"""

import numpy as np
import pytest
import torch
from conftest import channel

import clip_expect as CX
import density_expect as DE
import frames_expect as FE
import ofdm_oracle as O
import papr_expect as PX
import philox_streams as P
import profile_expect as PE
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.engine import LinkEngine, new_stats
from test_gpu_link_nscreen import LOW_SNR
from test_gpu_link_screen import MID_SNR
from test_gpu_philox_parity import gpu_radius, setup, stat_width_bound

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
OFFSETS = [(1 << 31) - 3, (1 << 32) - 3, 1 << 32, (1 << 40) + 5]
FAR = [(1 << 32) - 3, (1 << 40) + 5]
F32, F64 = B.OFDM_F32, B.OFDM_F64
MAX_SYMBOLS = 1 << 46  # OFDM_MAX_SYMBOLS (include/ofdm_hip.h; asserted against the header below)

# id: N, M, channel, equaliser, OFDM symbols, SNR dB, precision, variant -- the smallest shapes that reach
# each site: the flat throughput k_tx / k_rx pair (config b's shape, which k_link fuses), the window FIR
# with its regenerated predecessor, the generic kernel (N < 64; SC + ZP with the tail's noise samples),
# symbols of more than one wave, and the adaptive throughput kernels (FB = 1).  SNRs as in
# tests/test_gpu_philox_parity.py's cases of the same shapes, or lower: tens of errors in 9 .. 40 symbols.
SHAPES = {
    "flat_f64": (1024, 64, "flat_fading", "NONE", 13, 20.0, F64, {}),
    "flat_f32": (1024, 64, "flat_fading", "NONE", 13, 20.0, F32, {}),
    "fir_f64": (1024, 64, "severe_multipath", "MMSE", 40, 24.0, F64, {}),
    "fir_f32": (1024, 64, "severe_multipath", "MMSE", 40, 24.0, F32, {}),
    "n32_f64": (32, 16, "flat_fading", "NONE", 40, 10.0, F64, {}),
    "n32_f32": (32, 16, "flat_fading", "NONE", 40, 10.0, F32, {}),
    "sc_zp_psk": (256, 16, "Lin-Phoong_P1", "MMSE", 16, 16.0, F64, {"scheme": "PSK", "modulator": "SC", "prefix": "ZP"}),
    "n4096": (4096, 256, "Lin-Phoong_P1", "MMSE", 9, 28.0, F64, {}),
    "adaptive": (2048, 0, "Lin-Phoong_P1", "MMSE", 9, 14.0, F64, {"adaptive": True}),
}
# (the adaptive plan is loaded for 20 dB, as the parity test's, and run 6 dB below it)
ADAPTIVE_LOADING_SNR = 20.0

# the shapes of the caller-bits tests beyond the ones above: the generic kernel's staged words (stage_words)
REF_SHAPES = {
    "n256_f64": (256, 16, "severe_multipath", "MMSE", 16, 16.0, F64, {}),
    "n256_f32": (256, 16, "severe_multipath", "MMSE", 16, 16.0, F32, {}),
}

_ENGINES = {}


def engine(sid):
    """(engine, CIR, cp, run_philox keywords) of a shape, built once."""
    if sid not in _ENGINES:
        N, M, ch, eq, _, snr, prec, var = {**SHAPES, **REF_SHAPES}[sid]
        _ENGINES[sid] = setup(N, M, ch, eq, prec, var, ADAPTIVE_LOADING_SNR if var.get("adaptive") else snr)
    return _ENGINES[sid]


class Run:
    """tx then rx of global symbols [sym0, sym0 + S) of a shape, called directly, and the oracle at that
    sym0 on the transmitter's own power: what every test here starts from."""

    def __init__(self, sid, sym0, seed=SEED, snr=None, S=None, n_valid=None, **rx_kw):
        N, M, ch, eq, S0, snr0, prec, _ = SHAPES[sid]
        self.eng, self.h, self.cp, self.var = engine(sid)
        eng = self.eng
        self.sid, self.sym0, self.seed, self.N, self.M, self.eq, self.prec = sid, sym0, seed, N, M, eq, prec
        self.S, self.snr = S or S0, snr0 if snr is None else snr
        self.total = self.S * (N + self.cp)
        self.n_valid = eng.valid_bits(sym0 + self.S) if n_valid is None else n_valid
        self.dev, self.stream = eng.device(), eng.stream()
        self.y = torch.empty((self.S, eng.ystride), dtype=eng.cdtype, device=self.dev)
        self.stats = new_stats(self.dev)
        eng.tx(self.stream, None, seed, sym0, self.S, self.y, self.stats)
        self.counts = self.rx(**rx_kw)
        self.got_y = self.y.cpu().numpy()
        self.st = self.stats.cpu().numpy()
        self._ref = None

    def rx(self, snr=None, **kw):
        """[bit errors, symbol errors] of ofdm_rx (or, with a record in kw, its form with that record)."""
        cnt = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self.eng.rx(self.stream, self.y, None, None, self.seed, self.stats, self.total, self.snr if snr is None else snr,
                    True, None, self.sym0, self.S, self.n_valid, cnt, **kw)
        torch.cuda.synchronize()
        return cnt.cpu().numpy().tolist()

    def oracle(self, snr=None):
        f32 = self.prec == F32
        got = self.got_y.astype(np.complex128)
        return P.run_philox(self.seed, self.S, self.N, self.M, self.h, self.cp, self.eq, self.snr if snr is None else snr,
                            precision="f32" if f32 else "f64", radius_fn=gpu_radius, power_sum=float(self.st[0]),
                            stat_sigma=(lambda yref: float(np.sqrt(np.mean(np.abs(got - yref) ** 2)))) if f32 else None,
                            sym0=self.sym0, total_samples=self.total, **self.var)

    @property
    def ref(self):
        if self._ref is None:
            self._ref = self.oracle()
        return self._ref

    def check_tx(self):
        ref, f32 = self.ref, self.prec == F32
        rms = np.sqrt(np.mean(np.abs(ref.y) ** 2))
        assert self.got_y.shape == ref.y.shape
        err = float(np.max(np.abs(self.got_y - ref.y))) / rms
        print(f"{self.sid} at {self.sym0}: tx max |dy| / rms {err:.3e}")
        assert err <= (1e-4 if f32 else 1e-12)
        rt = 1e-5 if f32 else 1e-12
        assert self.st[0] == pytest.approx(ref.power_sum, rel=rt)
        assert self.st[1] == pytest.approx(ref.x_power_sum, rel=rt)
        assert self.st[2] == pytest.approx(ref.x_peak, rel=rt)

    def check_counts(self, counts=None, ref=None, least=10):
        ref = self.ref if ref is None else ref
        be, se = self.counts if counts is None else counts
        lo, hi, slo, shi = ref.bracket
        print(f"{self.sid} at {self.sym0}: bits {be} in [{lo}, {hi}], symbols {se} in [{slo}, {shi}] "
              f"(oracle {ref.bit_errors} / {ref.symbol_errors})")
        assert ref.bit_errors >= least, "SNR too high for a meaningful count"
        if self.prec == F64:
            assert (lo, slo) == (hi, shi) == (ref.bit_errors, ref.symbol_errors), ref.bracket
            assert (be, se) == (ref.bit_errors, ref.symbol_errors)
        else:
            blo, bhi, sslo, sshi = ref.stat_bracket
            print(f"{self.sid} at {self.sym0}: statistical bracket bits [{blo}, {bhi}], symbols [{sslo}, {sshi}]")
            assert lo <= be <= hi and slo <= se <= shi, ((be, se), ref.bracket)
            assert blo <= be <= bhi and sslo <= se <= sshi, ((be, se), ref.stat_bracket)
            w = stat_width_bound(ref.bit_errors)
            assert bhi - blo <= w and sshi - sslo <= w, (ref.stat_bracket, w)


def test_the_limit_is_the_headers():
    import re
    from test_abi import HEADER

    text = open(HEADER).read()
    m = re.search(r"#define OFDM_MAX_SYMBOLS \(\(int64_t\)1 << (\d+)\)", text)
    assert m and 1 << int(m.group(1)) == MAX_SYMBOLS
    # the derivation the header states: 4096 subcarriers of 12 bits stay below 2^16 bits per symbol
    assert 4096 * 12 < 1 << 16 and MAX_SYMBOLS * (1 << 16) <= 1 << 62


# ---------------------------------------------------------------- tx and rx at every offset and shape
@pytest.mark.parametrize("sid", sorted(SHAPES))
@pytest.mark.parametrize("sym0", OFFSETS, ids=lambda v: hex(v))
def test_tx_and_rx_against_the_oracle(gpu, sym0, sid):
    r = Run(sid, sym0)
    r.check_tx()
    r.check_counts()
    if sid == "adaptive":
        # the trailing partial byte is that of [0, sym0 + S): masked on the device as in the oracle
        assert r.n_valid == 8 * ((sym0 + r.S) * r.eng.bps // 8)


def test_a_seed_above_2_32_is_not_its_low_word(gpu):
    r = Run("flat_f64", (1 << 32) - 3, seed=7 + (1 << 32))
    r.check_tx()
    r.check_counts()
    low = Run("flat_f64", (1 << 32) - 3, seed=7)
    low.check_tx()
    assert np.count_nonzero(low.ref.idx != r.ref.idx) > r.ref.idx.size // 3
    assert np.max(np.abs(low.got_y - r.got_y)) > 0.1 * np.sqrt(np.mean(np.abs(r.got_y) ** 2))
    assert low.counts != r.counts


@pytest.mark.parametrize("sym0", OFFSETS, ids=lambda v: hex(v))
def test_n_valid_bits_cut_inside_the_second_to_last_symbol(gpu, sym0):
    """The generic kernel masks at global bit positions (sym0 + s) bps + offset < n_valid_bits."""
    sid = "n32_f64"
    eng = engine(sid)[0]
    S = SHAPES[sid][4]
    bps = eng.bps
    cut = (sym0 + S - 2) * bps + bps // 2 + 3
    r = Run(sid, sym0, n_valid=cut)
    whole = Run(sid, sym0)
    ref = r.ref
    assert ref.bracket[0] == ref.bracket[1] and ref.bracket[2] == ref.bracket[3]
    bk = eng.bits_per_subcarrier
    be, se = FE.per_symbol_from_z(ref.z, ref.idx, bk, cut, "QAM", sym0)
    allb, _ = FE.per_symbol_from_z(ref.z, ref.idx, bk, (sym0 + S) * bps, "QAM", sym0)
    print(f"cut at bit {cut}: per symbol {be.tolist()}, uncut {allb.tolist()}")
    assert int(allb.sum()) == ref.bit_errors == whole.counts[0]
    assert be[-1] == 0 and be[:-2].tolist() == allb[:-2].tolist() and be[-2] <= allb[-2]
    assert int(allb[-2:].sum()) > int(be[-2:].sum()), "the cut masks no error: choose another SNR"
    assert r.counts == [int(be.sum()), int(se.sum())]


# ---------------------------------------------------------------- the fused link, all four forms
# (SNR, the forms run at it): each forced screen at the SNR at which its own test shows a known share of the
# symbols redone in complex128 -- the two-transform screen about half at 21 dB
# (tests/test_gpu_link_screen.py), the noise screen, whose symbols the sparse form's are, 0.41 at 10 dB
# (tests/test_gpu_link_nscreen.py) -- and ofdm_link itself at both
LINK_FORMS = [(MID_SNR, [(None, 0), ("screen", 2)]), (LOW_SNR, [(None, 0), ("nscreen", 2), ("sparse", 4)])]


@pytest.mark.parametrize("sym0", FAR, ids=lambda v: hex(v))
def test_link_in_all_four_forms(gpu, sym0):
    """ofdm_link, and ofdm_link_screen / _nscreen / _sparse forced with their redo paths reached: exactly
    tx + rx of the same symbols, and the oracle's counts."""
    S = 25  # two workgroups of 12 symbols and one more
    for snr, forms in LINK_FORMS:
        r = Run("flat_f64", sym0, snr=snr, S=S)
        r.check_counts()
        eng = r.eng
        assert eng.has_fused
        for form, n_counts in forms:
            cnt = torch.zeros(2, dtype=torch.int64, device=r.dev)
            sc = torch.zeros(n_counts, dtype=torch.int64, device=r.dev) if form else None
            try:
                if form:
                    setattr(eng, form + "_mode", B.LINK_SCREEN_FORCED)
                    setattr(eng, form + "_counts", sc)
                eng.link(r.stream, SEED, r.stats, r.total, snr, True, sym0, S, r.n_valid, cnt)
                torch.cuda.synchronize()
            finally:
                if form:
                    setattr(eng, form + "_mode", None)
                    setattr(eng, form + "_counts", None)
            got = cnt.cpu().numpy().tolist()
            print(f"link {form} at {sym0}, {snr} dB: {got}, screen counts {None if sc is None else sc.tolist()}")
            assert got == r.counts == [r.ref.bit_errors, r.ref.symbol_errors], form
            if form:
                screened, redone = sc.tolist()[:2]
                assert screened == S and 0 < redone < S, (form, sc.tolist())


# ---------------------------------------------------------------- the sweep receiver
@pytest.mark.parametrize("sid", ["flat_f64", "fir_f64"])
@pytest.mark.parametrize("sym0", FAR, ids=lambda v: hex(v))
def test_rx_sweep_is_rx_at_every_point(gpu, sym0, sid):
    r = Run(sid, sym0)
    snrs = [r.snr - 3.0, r.snr, r.snr + 2.0]
    cnt = torch.zeros((3, 2), dtype=torch.int64, device=r.dev)
    r.eng.rx_sweep(r.stream, r.y, SEED, r.stats, r.total, snrs, sym0, r.S, r.n_valid, cnt)
    torch.cuda.synchronize()
    got = cnt.cpu().numpy().tolist()
    want = [r.rx(snr=q) for q in snrs]
    print(f"sweep {sid} at {sym0}: {got}")
    assert got == want and want[1] == r.counts and want[0][0] > want[2][0] > 0
    r.check_counts()


# ---------------------------------------------------------------- PAPR
H1 = np.array([1.0 + 0j])
EDGES = PX.ratios(PX.default_edges_db())
PAPR = {"n1024_f64": (1024, 0, 64, "f64", 40), "n64_f64": (64, 16, 16, "f64", 40), "n64_f32": (64, 16, 16, "f32", 40)}


@pytest.mark.parametrize("pid", sorted(PAPR))
@pytest.mark.parametrize("sym0", FAR, ids=lambda v: hex(v))
def test_papr_pairs_and_histogram(gpu, sym0, pid):
    N, cp, M, precision, S = PAPR[pid]
    luts = [O.qam_lut(M)]
    eng = LinkEngine(N, cp, H1, B.EQ_NONE, luts, None, F64 if precision == "f64" else F32)
    hist = torch.zeros(len(EDGES) + 1, dtype=torch.int64, device=eng.device())
    out = torch.zeros((S, 2), dtype=torch.float64, device=eng.device())
    eng.papr_hist(eng.stream(), None, SEED, sym0, S, EDGES, hist, out, S)
    torch.cuda.synchronize()
    got, h = out.cpu().numpy(), hist.cpu().numpy()
    peak, total, n = PX.per_symbol(N, cp, S, luts, seed=SEED, sym0=sym0)
    err = max(float(np.max(np.abs(got[:, 0] - peak) / peak)), float(np.max(np.abs(got[:, 1] - total) / total)))
    print(f"papr {pid} at {sym0}: per-symbol relative error {err:.3e}")
    assert n == N + cp and err <= PX.TOL[precision]
    PX.assert_in_bracket(h, peak, total, n, EDGES, precision, pid)
    if sym0 >= 1 << 32:  # (and these are not the pairs of the symbols whose index is the low word)
        low, _, _ = PX.per_symbol(N, cp, S, luts, seed=SEED, sym0=sym0 & 0xFFFFFFFF)
        assert np.count_nonzero(np.abs(low - peak) > 1e-3 * peak) > S // 2


# ---------------------------------------------------------------- the receiver's records
FRAME_CASES = {"A": ((1 << 32) - 3, 8, 1 << 31, 3), "B": ((1 << 40) + 5, 8, 1 << 40, 2)}


@pytest.mark.parametrize("sid", ["flat_f64", "n32_f64"])
@pytest.mark.parametrize("cid", sorted(FRAME_CASES))
def test_frame_record_splits_the_index_at_64_bits(gpu, cid, sid):
    """A: frame 0 stays zero, frame 1 takes the first 3 symbols (up to 2^32 - 1), frame 2 the other 5.
    B: frame 1 takes all 8.  From the oracle's equalised points through frames_expect."""
    sym0, S, F, n_frames = FRAME_CASES[cid]
    r = Run(sid, sym0, S=S)
    rec = torch.zeros((n_frames, 2), dtype=torch.int64, device=r.dev)
    counts = r.rx(frames=rec, frame_symbols=F)
    got = rec.cpu().numpy()
    ref = r.ref
    assert ref.bracket[0] == ref.bracket[1] and ref.bracket[2] == ref.bracket[3]
    be, se = FE.per_symbol_from_z(ref.z, ref.idx, r.eng.bits_per_subcarrier, r.n_valid, "QAM", sym0)
    want = np.stack([FE.frame_sums(be, F, sym0), FE.frame_sums(se, F, sym0)], axis=1)
    print(f"frames {cid} {sid}: device {got.tolist()}, expected {want.tolist()}")
    assert want.shape == (n_frames, 2) and np.array_equal(got, want)
    assert counts == r.counts == [int(be.sum()), int(se.sum())] and be.sum() > 0
    if cid == "A":
        assert not got[0].any() and got[1].tolist() == [int(be[:3].sum()), int(se[:3].sum())] and be[:3].sum() > 0
    else:
        assert not got[0].any()


def test_profile_record(gpu):
    sym0 = (1 << 32) - 3
    r = Run("flat_f64", sym0)
    prof = torch.zeros((B.PROFILE_ROWS, r.N), dtype=torch.int64, device=r.dev)
    counts = r.rx(profile=prof)
    rows = PE.record_rows(E.combine_profile([prof.cpu().numpy()]))
    ref = r.ref
    bk = r.eng.bits_per_subcarrier
    exp = PE.expected_rows(ref.z, ref.idx, bk, r.S * r.eng.bps)
    for k in ("bit_errors", "symbol_errors", "clipped"):
        assert np.array_equal(rows[k], exp[k]), (k, np.flatnonzero(rows[k] != exp[k])[:8])
    err = np.abs(rows["error_power"] - exp["error_power"])
    bound = PE.power_bound(ref.z, exp["error_power"], 1e-9)
    print(f"profile at {sym0}: error power max |diff| {err.max():.3e} (bound at least {bound.min():.3e})")
    assert np.all(err <= bound)
    assert counts == r.counts == [int(exp["bit_errors"].sum()), int(exp["symbol_errors"].sum())]
    r.check_counts()


def test_density_record(gpu):
    sym0 = (1 << 32) - 3
    r = Run("flat_f64", sym0)
    G, L = 64, 1.5 * r.eng.lut_reach
    rec = torch.zeros(G * G + 1, dtype=torch.int64, device=r.dev)
    counts = r.rx(density=rec, density_params=E.density_grid(G, L) + (G,), density_subcarriers=(0, r.N))
    got = rec.cpu().numpy()
    Z, delta, _ = DE.philox_points(SEED, r.S, r.N, r.M, r.h, r.cp, r.eq, r.snr, radius_fn=gpu_radius,
                                   power_sum=float(r.st[0]), sym0=sym0)
    assert float(np.mean(DE.undecided(Z, delta, G, L))) <= 1e-3
    dec, maybe = DE.bracket(Z, delta, G, L)
    over = got - dec
    print(f"density at {sym0}: {int(maybe.sum())} candidate cells of undecided points")
    assert int(got.sum()) == r.S * r.N and np.all(over >= 0) and np.all(over <= maybe)
    assert counts == r.counts
    r.check_counts()


# ---------------------------------------------------------------- the clipped transmitter
CLIPPED = {"flat_throughput": (1024, 64, "flat_fading", None, "NONE", 4.0, 13),
           "generic": (64, 16, "severe_multipath", 7, "MMSE", 3.0, 40)}


@pytest.mark.parametrize("cid", sorted(CLIPPED))
def test_clipped_transmitter(gpu, cid):
    sym0 = (1 << 32) - 3
    N, M, ch, cp, eq, clip_db, S = CLIPPED[cid]
    h = channel(ch)
    cp = len(h) - 1 if cp is None else cp
    luts = [O.qam_lut(M)]
    eng = LinkEngine(N, cp, h, {"NONE": B.EQ_NONE, "MMSE": B.EQ_MMSE}[eq], luts, None, F64, clip_db=clip_db)
    a2 = CX.threshold(clip_db, N, luts)
    assert eng.clip_a2 == pytest.approx(a2, rel=1e-15)
    y = torch.empty((S, eng.ystride), dtype=eng.cdtype, device=eng.device())
    stats, rec = new_stats(eng.device()), torch.zeros(2, dtype=torch.int64, device=eng.device())
    eng.tx(eng.stream(), None, SEED, sym0, S, y, stats, clip_counters=rec)
    torch.cuda.synchronize()
    ref = CX.run_clipped(SEED, S, N, M, h, cp, eq, 30.0, eng.clip_a2, noise_on=False, sym0=sym0)
    got, st = y.cpu().numpy(), stats.cpu().numpy()
    err = float(np.max(np.abs(got - ref.y))) / np.sqrt(np.mean(np.abs(ref.y) ** 2))
    lo, hi = ref.count_bracket("f64", eng.clip_a2)
    print(f"clip {cid} at {sym0}: tx max |dy| / rms {err:.3e}, clipped {rec.tolist()} in [{lo}, {hi}]")
    assert err <= 1e-12
    assert st[0] == pytest.approx(ref.power_sum, rel=1e-12) and st[2] == pytest.approx(ref.x_peak, rel=1e-12)
    clipped, samples = rec.tolist()
    assert samples == S * N and lo <= clipped <= hi and hi - lo <= CX.count_width_cap("f64", S * N) and clipped > 0


# ---------------------------------------------------------------- the whole engine path, a 64-bit seed
@pytest.mark.parametrize("sid", ["flat_f64", "fir_f64"])
def test_engine_run_with_a_64_bit_seed(gpu, sid):
    N, M, ch, eq, S, snr, prec, _ = SHAPES[sid]
    eng, h, cp, var = engine(sid)
    res = eng.run(S, snr, seed=SEED)
    ref = P.run_philox(SEED, S, N, M, h, cp, eq, snr, precision="f64", radius_fn=gpu_radius, power_sum=res.power_sum, **var)
    low = P.run_philox(SEED & 0xFFFFFFFF, S, N, M, h, cp, eq, snr, power_sum=res.power_sum, **var)
    print(f"run {sid}: {res.bit_errors} / {res.symbol_errors}, oracle {ref.bit_errors} / {ref.symbol_errors}, "
          f"the low word's stream {low.bit_errors} / {low.symbol_errors}")
    assert ref.bracket == (ref.bit_errors, ref.bit_errors, ref.symbol_errors, ref.symbol_errors)
    assert (res.bit_errors, res.symbol_errors) == (ref.bit_errors, ref.symbol_errors) and ref.bit_errors >= 10
    assert res.power_sum == pytest.approx(ref.power_sum, rel=1e-12) and res.x_peak == pytest.approx(ref.x_peak, rel=1e-12)
    assert res.x_peak != pytest.approx(low.x_peak, rel=1e-9)


# ---------------------------------------------------------------- the supported symbol range
def _entry_points():
    """name -> a call of that entry point over [sym0, sym0 + 1) on the flat complex128 shape (the one
    plan every entry point takes), returning what it counted."""
    eng = engine("flat_f64")[0]
    dev, st = eng.device(), eng.stream()
    N, snr = 1024, 20.0
    h = channel("flat_fading")
    clip = LinkEngine(N, len(h) - 1, h, B.EQ_NONE, [O.qam_lut(64)], None, F64, clip_db=4.0)
    y = torch.zeros((1, N), dtype=eng.cdtype, device=dev)
    stats = new_stats(dev)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.int64, device=dev)

    def rx(sym0, **kw):
        c = z(2)
        eng.rx(st, y, None, None, SEED, stats, N, snr, True, None, sym0, 1, (sym0 + 1) * eng.bps, c, **kw)
        return c

    def link(form, n):
        def call(sym0):
            c = z(2)
            try:
                if form:
                    setattr(eng, form + "_mode", B.LINK_SCREEN_FORCED)
                    setattr(eng, form + "_counts", z(n))
                eng.link(st, SEED, stats, N, snr, True, sym0, 1, (sym0 + 1) * eng.bps, c)
            finally:
                if form:
                    setattr(eng, form + "_mode", None)
                    setattr(eng, form + "_counts", None)
            return c
        return call

    def sweep(sym0):
        c = z(2, 2)
        eng.rx_sweep(st, y, SEED, stats, N, [snr, snr + 1.0], sym0, 1, (sym0 + 1) * eng.bps, c)
        return c[0]

    def papr(sym0):
        hist, pair = z(len(EDGES) + 1), torch.zeros((1, 2), dtype=torch.float64, device=dev)
        eng.papr_hist(st, None, SEED, sym0, 1, EDGES, hist, pair, 1)
        return torch.cat([pair[0], hist.to(torch.float64)])  # (peak, sum, the histogram)

    def tx(e, **kw):
        def call(sym0):
            stats.zero_()
            e.tx(st, None, SEED, sym0, 1, y, stats, **kw)
            return stats
        return call

    G = 16
    return {
        "ofdm_tx": tx(eng), "ofdm_tx_clip": tx(clip, clip_counters=z(2)), "ofdm_rx": rx,
        "ofdm_rx_profile": lambda s: rx(s, profile=z(B.PROFILE_ROWS, N)),
        "ofdm_rx_frames": lambda s: rx(s, frames=z(2, 2), frame_symbols=1 << 62),
        "ofdm_rx_density": lambda s: rx(s, density=z(G * G + 1), density_params=E.density_grid(G, 2.0) + (G,),
                                        density_subcarriers=(0, N)),
        "ofdm_rx_sweep": sweep, "ofdm_link": link(None, 0), "ofdm_link_screen": link("screen", 2),
        "ofdm_link_nscreen": link("nscreen", 2), "ofdm_link_sparse": link("sparse", 4), "ofdm_papr": papr,
    }


ENTRY_POINTS = ["ofdm_tx", "ofdm_tx_clip", "ofdm_rx", "ofdm_rx_profile", "ofdm_rx_frames", "ofdm_rx_density",
                "ofdm_rx_sweep", "ofdm_link", "ofdm_link_screen", "ofdm_link_nscreen", "ofdm_link_sparse", "ofdm_papr"]


def test_every_entry_point_with_a_symbol_offset_is_listed():
    takes = [n for n, (_, args) in B.SIGNATURES.items() if n.startswith(("ofdm_tx", "ofdm_rx", "ofdm_link", "ofdm_papr"))]
    assert sorted(takes) == sorted(ENTRY_POINTS)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_symbols_beyond_the_supported_range_are_refused(gpu, name):
    calls = _entry_points()
    # the transmit first: the receivers of the last supported symbol read its record and its samples
    calls["ofdm_tx"](MAX_SYMBOLS - 1)
    call = calls[name]
    for sym0 in (MAX_SYMBOLS, 1 << 62, (1 << 63) - 1):
        with pytest.raises(ValueError, match="OFDM_MAX_SYMBOLS"):
            call(sym0)
    calls["ofdm_tx"](MAX_SYMBOLS - 1)
    out = call(MAX_SYMBOLS - 1)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    print(f"{name} at OFDM_MAX_SYMBOLS - 1: {got.tolist()[:4]}")
    luts, h = [O.qam_lut(64)], channel("flat_fading")
    if name == "ofdm_papr":
        peak, total, _ = PX.per_symbol(1024, 0, 1, luts, seed=SEED, sym0=MAX_SYMBOLS - 1)
        assert got[0] == pytest.approx(peak[0], rel=1e-12) and got[1] == pytest.approx(total[0], rel=1e-12)
        assert int(got[2:].sum()) == 1
    elif name == "ofdm_tx":
        ref = P.run_philox(SEED, 1, 1024, 64, h, 0, "NONE", 20.0, noise_on=False, sym0=MAX_SYMBOLS - 1)
        assert got[0] == pytest.approx(ref.power_sum, rel=1e-12) and got[2] == pytest.approx(ref.x_peak, rel=1e-12)
    elif name == "ofdm_tx_clip":
        ref = CX.run_clipped(SEED, 1, 1024, 64, h, 0, "NONE", 20.0, CX.threshold(4.0, 1024, luts), noise_on=False,
                             sym0=MAX_SYMBOLS - 1)
        assert ref.clipped > 0
        assert got[0] == pytest.approx(ref.power_sum, rel=1e-12) and got[2] == pytest.approx(ref.x_peak, rel=1e-12)
    else:
        r = Run("flat_f64", MAX_SYMBOLS - 1, S=1)
        assert got.tolist() == r.counts == [r.ref.bit_errors, r.ref.symbol_errors] and r.ref.bit_errors > 0


def test_the_refusal_is_formed_without_overflow(gpu):
    """n_sym near 2^63 with a small sym0, and both large: refused, not wrapped into range."""
    eng = engine("flat_f64")[0]
    stats = new_stats(eng.device())
    for sym0, n in ((0, MAX_SYMBOLS + 1), (1, (1 << 63) - 1), ((1 << 63) - 1, (1 << 63) - 1), (MAX_SYMBOLS - 1, 2)):
        with pytest.raises(ValueError, match="OFDM_MAX_SYMBOLS"):
            eng.tx(eng.stream(), None, SEED, sym0, n, None, stats)
    assert not stats.cpu().numpy().any()


# ---------------------------------------------------------------- caller bits beyond bit 2^31 and 2^32
# Reference mode: the kernels read the caller's packed bits at s bps + offset, formed in int64_t by
# stage_words (the generic kernel), ref_lane (the throughput kernels' REF instantiations) and
# ref_lane_adaptive.  One buffer of 2^29 + 64 Ki zero bytes holds bit 2^32 and 16 symbols of any plan here
# beyond it; random bytes are written only over the window a call reads (its predecessor's among them).
BIG_BYTES = (1 << 29) + (64 << 10)
REF_S = 16
REF_CASES = ["fir_f64", "adaptive", "n256_f64", "n256_f32"]


@pytest.fixture(scope="module")
def big_buffer(gpu):
    buf = torch.zeros(BIG_BYTES, dtype=torch.uint8, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


class Shifted:
    """A device array of the symbols [sym0, sym0 + S) of a whole-stream array, standing for the whole
    stream: the address the entry points are handed is that of the stream's element 0, and the kernels
    index it at sg (N + cp) + m for the call's own symbols sg only -- inside ``t``."""

    def __init__(self, t, first_element):
        self.t, self.first = t, first_element

    def data_ptr(self):
        return self.t.data_ptr() - self.first * self.t.element_size()


def window_sym0(bps, threshold):
    """A multiple of 8 (so the window starts on a byte for any bps) with sym0 bps < threshold <=
    (sym0 + 16) bps: the largest multiple of 8 at most q - 8, q = ceil(threshold / bps)."""
    q = -(-threshold // bps)
    sym0 = (q - 8) // 8 * 8
    assert sym0 % 8 == 0 and sym0 * bps < threshold <= (sym0 + REF_S) * bps
    return sym0


def indices_of(window, skip, bk, rows):
    """(rows, N) constellation indices of the OFDM symbols packed MSB first in the bytes ``window`` from
    bit ``skip``: subcarrier k takes its bk[k] bits in subcarrier order (constellation/adaptive.py:178-199;
    fixed orders: bk constant)."""
    tot = int(bk.sum())
    bits = O.bytes_to_bits(window.tobytes())[skip:skip + rows * tot].astype(np.int64).reshape(rows, tot)
    off = np.concatenate([[0], np.cumsum(bk)[:-1]])
    idx = np.zeros((rows, len(bk)), np.int64)
    for k in np.flatnonzero(bk > 0):
        idx[:, k] = bits[:, off[k]:off[k] + bk[k]] @ (1 << np.arange(bk[k] - 1, -1, -1))
    return idx


@pytest.mark.parametrize("sid", REF_CASES)
@pytest.mark.parametrize("log2", [31, 32])
def test_caller_bits_beyond_2_31_and_2_32(gpu, big_buffer, log2, sid):
    N, M, ch, eq, _, snr, prec, _ = {**SHAPES, **REF_SHAPES}[sid]
    eng, h, cp, var = engine(sid)
    S, bps, bk = REF_S, eng.bps, eng.bits_per_subcarrier
    dev, st = eng.device(), eng.stream()
    sym0 = window_sym0(bps, 1 << log2)
    lead = -(-bps // 8)                       # the predecessor's bytes (its first one may be shared)
    b0, b1 = sym0 * bps // 8 - lead, -(-(sym0 + S) * bps // 8)
    assert 0 < b0 and b1 <= BIG_BYTES and b0 * 8 < 1 << log2 <= b1 * 8
    rng = np.random.default_rng(log2 * 1000 + N)
    window = rng.integers(0, 256, size=b1 - b0, dtype=np.uint8)
    big_buffer[b0:b1] = torch.from_numpy(window).to(dev)
    small = torch.zeros(8 * bps // 8 + (b1 - b0) - lead + 8, dtype=torch.uint8, device=dev)
    small[8 * bps // 8 - lead:8 * bps // 8 - lead + (b1 - b0)] = torch.from_numpy(window).to(dev)
    nr, ni = (torch.from_numpy(rng.standard_normal(S * (N + cp))).to(dev) for _ in range(2))
    total = S * (N + cp)

    def call(bits_d, s0):
        y = torch.empty((S, eng.ystride), dtype=eng.cdtype, device=dev)
        stats, cnt = new_stats(dev), torch.zeros(2, dtype=torch.int64, device=dev)
        eng.tx(st, bits_d, 0, s0, S, y, stats)
        eng.rx(st, y, Shifted(nr, s0 * (N + cp)), Shifted(ni, s0 * (N + cp)), 0, stats, total, snr, True, bits_d, s0, S,
               eng.valid_bits(s0 + S), cnt)
        torch.cuda.synchronize()
        return y.cpu().numpy(), stats.cpu().numpy(), cnt.cpu().numpy().tolist()

    try:
        y_big, st_big, c_big = call(big_buffer, sym0)
    finally:
        big_buffer[b0:b1] = 0
    y_small, st_small, c_small = call(small, 8)
    print(f"{sid}, bit 2^{log2} inside symbols [{sym0}, {sym0 + S}): counts {c_big} (at symbol 8: {c_small})")
    assert np.array_equal(y_big, y_small) and np.array_equal(st_big, st_small) and c_big == c_small

    # the oracle's arithmetic on the same bytes: the predecessor's symbol, then the 16
    skip = 8 * lead - bps                     # the window's first byte holds the predecessor's first bit
    assert 0 <= skip < 8 and (b0 * 8 + skip) == (sym0 - 1) * bps
    idx_all = indices_of(window, skip, bk, S + 1)
    orders = var.get("orders")
    luts = PE.luts_for(orders) if orders is not None else {M: O.qam_lut(M)}
    order_of = np.asarray(orders if orders is not None else np.full(N, M), np.int64)
    X = np.zeros((S + 1, N), np.complex128)
    for o, lt in luts.items():
        X[:, order_of == o] = lt[idx_all[:, order_of == o]]
    y = O.channel_conv(O.modulate(X, cp).ravel(), h).reshape(S + 1, N + cp)[1:]
    f32 = prec == F32
    rms = np.sqrt(np.mean(np.abs(y) ** 2))
    err = float(np.max(np.abs(y_big - y[:, cp:]))) / rms
    print(f"{sid}: tx max |dy| / rms {err:.3e}")
    assert err <= (1e-4 if f32 else 1e-12)
    power = float(np.sum(np.abs(y) ** 2))
    assert st_big[0] == pytest.approx(power, rel=1e-5 if f32 else 1e-12)
    sigma = np.sqrt(st_big[0] / total / 10 ** (snr / 10) / 2.0)  # as the receivers: from the run's exact power
    rxs = (y + sigma * (nr.cpu().numpy() + 1j * ni.cpu().numpy()).reshape(S, N + cp))[:, cp:]
    H = np.fft.fft(np.asarray(h, np.complex128), N)
    Y = np.fft.fft(rxs, axis=1, norm="ortho")
    Z = O.equalize(Y, H, eq, snr)
    idx = idx_all[1:]
    delta = P.z_error_bound("f32" if f32 else "f64", Y, H, eq, snr, np.zeros(S), "OFDM", N)
    if orders is not None:
        lo, hi, slo, shi = P.adaptive_bracket(Z, idx, order_of, bk, delta, "QAM", sym0)
    else:
        lo, hi, slo, shi = P.decision_bracket(Z, idx, luts[M], int(np.log2(M)), delta, "QAM")
    print(f"{sid}: bits {c_big[0]} in [{lo}, {hi}], symbols {c_big[1]} in [{slo}, {shi}]")
    assert lo >= 10, "SNR too high for a meaningful count"
    assert lo <= c_big[0] <= hi and slo <= c_big[1] <= shi
    if not f32:
        assert (lo, slo) == (hi, shi)

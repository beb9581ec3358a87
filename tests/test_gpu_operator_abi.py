"""The operator entry points through B.lib() and B.Plan(precision=...) directly, in complex128 AND
complex64, against the float64 references and derived bounds of tests/operator_expect.py: the rows
kernels (ofdm_fft, ofdm_modulate, ofdm_demodulate) at every N = 2^0 .. 2^12, every prefix geometry and
row counts around one workgroup iteration; a second trip of every grid-stride loop (more than kMaxGrid =
4096 workgroups of work); ofdm_equalize, ofdm_map / ofdm_demap (fixed orders up to 4096 and adaptive),
ofdm_demap_count with known error counts, ofdm_channel / ofdm_power / ofdm_awgn across workgroup
boundaries with "+=" pinned; bit-identical repeats on one and on two streams; refusals and empty calls.

Integer outputs are exact.  Floating-point outputs are held to the rigorous bounds (hard assertions); the
complex64 rows kernels are also held to 8 times the error of numpy's own complex64 transform, and
complex128 to the suite's 1e-12 at unit scale.  Every comparison prints its largest error / bound ratio;
with OFDM_OPERATOR_MARGINS_OUT set the module writes the table (profiles/operator_abi_margins.json).

Largest device footprints: rows tests a few MB; the N = 4 second trip 100 MB in + 67 MB out (complex128
demodulate); the in-place complex64 FFT at N = 4096 134 MB; flat second trips 17 MB per buffer."""

import json
import math
import os

import numpy as np
import pytest
import torch
from conftest import DEFAULT_4TAP, channel

import ofdm_oracle as O
import operator_expect as E
from ofdm_based_systems import _backend as B

pytestmark = pytest.mark.gpu
PRECS = pytest.mark.parametrize("prec", [B.OFDM_F64, B.OFDM_F32], ids=["f64", "f32"])
EQ_ID = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}
PNAME = {B.OFDM_F64: "complex128", B.OFDM_F32: "complex64"}
MARGINS = []

assert (B.OFDM_F32, B.OFDM_F64) == (E.F32, E.F64)


@pytest.fixture(scope="module", autouse=True)
def margins_table():
    yield
    out = os.environ.get("OFDM_OPERATOR_MARGINS_OUT")
    if out and MARGINS:
        with open(out, "w") as f:
            json.dump({"what": "largest error / rigorous bound per operator entry point, precision and N; rows "
                               "kernels in complex64 also against numpy's complex64 transform (worst row-wise "
                               "relative 2-norm error of each, and their ratio, asserted <= 8)",
                       "rows": MARGINS}, f, indent=1)


def report(entry, prec, n, ratio, **extra):
    """One line per entry point, precision and N; asserts the rigorous bound."""
    row = {"entry": entry, "precision": PNAME[prec], "n": n, "share_of_bound": ratio, **extra}
    MARGINS.append(row)
    print(f"{entry} {PNAME[prec]} N={n}: error / bound {ratio:.4f}" +
          "".join(f", {k} {v:.3e}" if isinstance(v, float) else f", {k} {v}" for k, v in extra.items()))
    assert ratio <= 1.0, row


def dev(a, prec=None):
    """Host array -> device tensor (complex arrays in the plan's precision)."""
    a = np.ascontiguousarray(a)
    if prec is not None and np.iscomplexobj(a):
        a = a.astype(E.cdtype(prec))
    return torch.from_numpy(a.copy()).to("cuda")


def host(t):
    return t.cpu().numpy()


def taps(L):
    return {1: np.array([0.8 - 0.6j]), 2: DEFAULT_4TAP[:2], 4: DEFAULT_4TAP, 32: E.decaying_taps()}[L]


def channel_for(logn):
    """The three test channels in turn over N: the default 4 taps, severe_multipath, the 32-tap draw."""
    return [DEFAULT_4TAP, channel("severe_multipath"), E.decaying_taps()][logn % 3]


def plan_H(plan):
    H = torch.empty(plan.n_fft, dtype=torch.complex128, device="cuda")
    B.check(B.lib().ofdm_plan_response(plan.handle, B.stream_ptr(), B.ptr(H), None))
    return host(H)


def run_fft(plan, x, inverse, prec):
    d = dev(x, prec)
    B.check(B.lib().ofdm_fft(plan.handle, B.stream_ptr(), B.ptr(d), x.shape[0], inverse))
    return host(d)


def run_modulate(plan, X, prec):
    d = dev(X, prec)
    out = torch.full((X.shape[0], plan.n_fft + plan.cp), float("nan"), dtype=plan.cdtype, device="cuda")
    B.check(B.lib().ofdm_modulate(plan.handle, B.stream_ptr(), B.ptr(d), X.shape[0], B.ptr(out)))
    return host(out)


def run_demodulate(plan, yt, snr_db, prec):
    d = dev(yt, prec)
    out = torch.full((yt.shape[0], plan.n_fft), float("nan"), dtype=plan.cdtype, device="cuda")
    B.check(B.lib().ofdm_demodulate(plan.handle, B.stream_ptr(), B.ptr(d), yt.shape[0], snr_db, B.ptr(out)))
    return host(out)


def numpy32(x, inverse):
    x = np.asarray(x, np.complex64)
    return np.fft.ifft(x, axis=1, norm="ortho") if inverse else np.fft.fft(x, axis=1, norm="ortho")


class Yard:
    """The second yardstick of one (entry, precision, N): the kernel's worst row-wise relative 2-norm error
    against numpy's complex64 transform of the same rows (complex64), or 1e-12 absolute at unit scale
    (complex128)."""

    def __init__(self):
        self.kernel = self.numpy = self.abs64 = 0.0

    def add(self, got, ref, np32=None, unit_scale=None):
        self.kernel = max(self.kernel, E.rows_rel_error(got, ref))
        if np32 is not None:
            self.numpy = max(self.numpy, E.rows_rel_error(np32, ref))
        if unit_scale is not None:
            self.abs64 = max(self.abs64, float(np.max(np.abs(got - ref) / unit_scale)))

    def check(self, entry, prec, n, ratio):
        if prec == B.OFDM_F32:
            r = self.kernel / self.numpy if self.numpy > 0 else (0.0 if self.kernel == 0 else math.inf)
            report(entry, prec, n, ratio, kernel_rel_error=self.kernel, numpy_rel_error=self.numpy,
                   kernel_over_numpy=r)
            assert self.kernel <= E.NUMPY_RATIO * self.numpy, (entry, n, self.kernel, self.numpy)
        else:
            report(entry, prec, n, ratio, kernel_rel_error=self.kernel, abs_error_unit_scale=self.abs64)
            assert self.abs64 <= E.F64_ABS, (entry, n, self.abs64)


# --------------------------------------------------------------------------- rows kernels, every N


@PRECS
@pytest.mark.parametrize("logn", E.LOGNS)
def test_fft_rows(gpu, logn, prec):
    n = 1 << logn
    plan = B.Plan(n_fft=n, precision=prec)
    worst, yard = 0.0, Yard()
    for rows in E.row_counts(n):
        x = E.round_input(E.rows_input(rows, n, 100 + logn), prec)
        for inv in (0, 1):
            got = run_fft(plan, x, inv, prec)
            worst = max(worst, E.cmp_fft(got, x, inv, prec))
            yard.add(got, E.ref_fft(x, inv), numpy32(x, inv) if prec == B.OFDM_F32 else None, 1.0)
    yard.check("ofdm_fft", prec, n, worst)


@PRECS
@pytest.mark.parametrize("logn", E.LOGNS)
def test_modulate_rows(gpu, logn, prec):
    """Cyclic prefix cp in {0, 1, N} and zero padding cp = min(N, 3): the body within the rows bound, the
    prefix bit-identical to the body samples it copies, the guard exactly zero."""
    n = 1 << logn
    worst, yard = 0.0, Yard()
    for cp, zp in E.prefixes(n):
        plan = B.Plan(n_fft=n, cp=cp, precision=prec, prefix=B.PREFIX_ZERO if zp else B.PREFIX_CYCLIC)
        for rows in E.row_counts(n):
            X = E.round_input(E.rows_input(rows, n, 200 + logn), prec)
            got = run_modulate(plan, X, prec)
            r = E.cmp_modulate(got, X, cp, zp, prec)
            assert r <= 1, (n, cp, zp, rows, r)
            worst = max(worst, r)
            body = got[:, :n] if zp else got[:, cp:]
            yard.add(body, E.ref_fft(X, 1), numpy32(X, 1) if prec == B.OFDM_F32 else None, 1.0)
    yard.check("ofdm_modulate", prec, n, worst)


@PRECS
@pytest.mark.parametrize("logn", E.LOGNS)
def test_demodulate_rows(gpu, logn, prec):
    """The same prefixes, each with NONE, ZF and MMSE at 15 dB; row r carries 1 + r / 4 of the amplitude, so
    a row's nv cannot be its neighbour's.  H is the plan's own (fft of the taps, cropped to N), read back
    and checked against numpy."""
    n = 1 << logn
    snr = E.DEMOD_SNR_DB
    h = channel_for(logn)
    worst = {eq: 0.0 for eq in E.EQ_NAMES}
    yard = Yard()
    for cp, zp in E.prefixes(n):
        for eq in E.EQ_NAMES:
            plan = B.Plan(n_fft=n, cp=cp, precision=prec, equalizer=EQ_ID[eq], h_raw=h,
                          prefix=B.PREFIX_ZERO if zp else B.PREFIX_CYCLIC)
            H = plan_H(plan)
            np.testing.assert_allclose(H, np.fft.fft(h, n), rtol=0, atol=1e-13 * np.sum(np.abs(h)))
            for rows in E.row_counts(n):
                yt = E.round_input(E.rows_input(rows, n + cp, 300 + logn, scaled=True), prec)
                got = run_demodulate(plan, yt, snr, prec)
                r = E.cmp_demodulate(got, yt, n, cp, zp, H, eq, snr, prec)
                assert r <= 1, (n, cp, zp, eq, rows, r)
                worst[eq] = max(worst[eq], r)
                if eq == "NONE":
                    np32 = numpy32(E.fold(yt.astype(np.complex64), n, cp, zp), 0) if prec == B.OFDM_F32 else None
                    yard.add(got, E.ref_demod_rows(yt, n, cp, zp), np32, 1 + np.arange(rows)[:, None] / 4.0)
    yard.check("ofdm_demodulate[NONE]", prec, n, worst["NONE"])
    report("ofdm_demodulate[ZF]", prec, n, worst["ZF"])
    report("ofdm_demodulate[MMSE]", prec, n, worst["MMSE"])


# --------------------------------------------------------------------------- second trip of k_rows' loop


@PRECS
@pytest.mark.parametrize("mode", ["fft", "modulate", "demodulate"])
def test_rows_second_trip_n4(gpu, mode, prec):
    """N = 4 (256 rows per workgroup iteration), 4096 * 256 + 257 rows: workgroups 0 and 1 take a second
    trip (groups 4096 and the one-row group 4097) over the LDS their first trip left behind."""
    n, cp, snr = 4, 2, E.DEMOD_SNR_DB
    rows = E.MAX_GRID * E.spb(n) + 257
    trip = E.MAX_GRID * E.spb(n)
    if mode == "fft":
        plan = B.Plan(n_fft=n, precision=prec)
        x = E.round_input(E.rows_input(rows, n, 41), prec)
        got, ref = run_fft(plan, x, 0, prec), E.ref_fft(x, 0)
        ratio = E.rows_ratio(got, ref, n, prec)
        parts = [E.rows_ratio(got[a:b], ref[a:b], n, prec) for a, b in ((trip, trip + 256), (trip + 256, rows))]
    elif mode == "modulate":
        plan = B.Plan(n_fft=n, cp=cp, precision=prec)
        X = E.round_input(E.rows_input(rows, n, 42), prec)
        got = run_modulate(plan, X, prec)
        ratio = E.cmp_modulate(got, X, cp, False, prec)
        parts = [E.cmp_modulate(got[a:b], X[a:b], cp, False, prec) for a, b in ((trip, trip + 256), (trip + 256, rows))]
    else:
        h = DEFAULT_4TAP
        plan = B.Plan(n_fft=n, cp=cp, precision=prec, equalizer=B.EQ_MMSE, h_raw=h)
        H = plan_H(plan)
        rng = np.random.default_rng(43)  # row powers over two decades, independent of the row's place
        yt = E.round_input(E.rows_input(rows, n + cp, 43) * 10 ** rng.uniform(-1, 1, (rows, 1)), prec)
        got = run_demodulate(plan, yt, snr, prec)
        ratio = E.cmp_demodulate(got, yt, n, cp, False, H, "MMSE", snr, prec)
        parts = [E.cmp_demodulate(got[a:b], yt[a:b], n, cp, False, H, "MMSE", snr, prec)
                 for a, b in ((trip, trip + 256), (trip + 256, rows))]
    assert all(p <= 1 for p in parts), parts
    report(f"second trip ofdm_{mode}", prec, n, ratio, rows=rows)


def test_fft_second_trip_n4096_in_place(gpu):
    """complex64, N = 4096 (one row per workgroup iteration), 4096 + 3 rows in place: rows 4096 .. 4098 are
    second trips."""
    n, prec = 4096, B.OFDM_F32
    rows = E.MAX_GRID + 3
    plan = B.Plan(n_fft=n, precision=prec)
    x = E.round_input(E.rows_input(rows, n, 44), prec)
    got, ref = run_fft(plan, x, 0, prec), E.ref_fft(x, 0)
    assert E.rows_ratio(got[E.MAX_GRID:], ref[E.MAX_GRID:], n, prec) <= 1
    assert E.rows_ratio(got[:3], ref[:3], n, prec) <= 1
    report("second trip ofdm_fft", prec, n, E.rows_ratio(got, ref, n, prec), rows=rows)


# --------------------------------------------------------------------------- ofdm_equalize


def run_equalize(plan, Y, snr_db, prec):
    d = dev(Y, prec)
    out = torch.full(Y.shape, float("nan"), dtype=plan.cdtype, device="cuda")
    B.check(B.lib().ofdm_equalize(plan.handle, B.stream_ptr(), B.ptr(d), Y.shape[0], snr_db, B.ptr(out)))
    return host(out)


@PRECS
@pytest.mark.parametrize("n", E.EQUALIZE_N)
def test_equalize(gpu, n, prec):
    """Rows of N = 1 (255 idle threads) to 4096 (16 loop trips per thread); 1 and 3 rows, and at N = 2
    4096 + 5 rows for the second trip; a null bin under ZF, an all-zero response under MMSE."""
    snr = E.DEMOD_SNR_DB
    H = np.fft.fft(DEFAULT_4TAP[:n], n)
    worst = {eq: 0.0 for eq in E.EQ_NAMES}
    for rows in [1, 3] + ([E.MAX_GRID + 5] if n == 2 else []):
        Y = E.round_input(E.rows_input(rows, n, 400 + n, scaled=rows <= 3), prec)
        if rows > 3:
            Y = E.round_input(Y * 10 ** np.random.default_rng(5).uniform(-1, 1, (rows, 1)), prec)
        for eq in E.EQ_NAMES:
            plan = B.Plan(n_fft=n, precision=prec, equalizer=EQ_ID[eq], H=H)
            got = run_equalize(plan, Y, snr, prec)
            r = E.cmp_equalize(got, Y, H, eq, snr, prec)
            assert r <= 1, (n, rows, eq, r)
            if rows > 3:
                assert E.cmp_equalize(got[E.MAX_GRID:], Y[E.MAX_GRID:], H, eq, snr, prec) <= 1
            worst[eq] = max(worst[eq], r)
    Y = E.round_input(E.rows_input(3, n, 450 + n, scaled=True), prec)
    Hn = H.copy()
    Hn[n // 2] = 0
    got = run_equalize(B.Plan(n_fft=n, precision=prec, equalizer=B.EQ_ZF, H=Hn), Y, snr, prec)
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got[:, n // 2], Y[:, n // 2] * 1e10, rtol=40 * E.unit(prec), atol=0)
    worst["ZF"] = max(worst["ZF"], E.cmp_equalize(got, Y, Hn, "ZF", snr, prec))
    plan0 = B.Plan(n_fft=n, precision=prec, equalizer=B.EQ_MMSE, H=np.zeros(n, complex))
    assert plan0.channel_gain_mean == 0.0
    assert np.all(run_equalize(plan0, Y, snr, prec) == 0)
    for eq in E.EQ_NAMES:
        report(f"ofdm_equalize[{eq}]", prec, n, worst[eq])


# --------------------------------------------------------------------------- ofdm_map / ofdm_demap

CANARY = 0xA5


def run_map(plan, data, n_out):
    by = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to("cuda")
    out = torch.full((n_out,), float("nan"), dtype=plan.cdtype, device="cuda")
    B.check(B.lib().ofdm_map(plan.handle, B.stream_ptr(), B.ptr(by), len(data), n_out, B.ptr(out)))
    return host(out)


def run_demap(plan, z, n_bytes, prec):
    """The demapped bytes; the buffer is 16 canary bytes longer, which must stay as they were."""
    d = dev(z, prec)
    out = torch.full((n_bytes + 16,), CANARY, dtype=torch.uint8, device="cuda")
    B.check(B.lib().ofdm_demap(plan.handle, B.stream_ptr(), B.ptr(d), len(z), B.ptr(out)))
    o = host(out)
    assert np.all(o[n_bytes:] == CANARY)
    return o[:n_bytes].tobytes()


@PRECS
@pytest.mark.parametrize("kind,m", E.FIXED_ORDERS, ids=[f"{k}{m}" for k, m in E.FIXED_ORDERS])
def test_map_demap_fixed(gpu, kind, m, prec):
    """n_out in {1, 255, 256, 257}, the input one byte short of n_out b bits (the zero padding of the bit
    window); orders above 256 take the wide slicer, in complex64 in float32.  Bit-exact."""
    lut = E.make_lut(kind, m)
    b = int(np.log2(m))
    plan = B.Plan(n_fft=64, precision=prec, luts=[lut])
    for n in E.MAP_COUNTS:
        rng = np.random.default_rng(1000 * m + n)
        idx = E.case_indices(m, n, rng)
        full = E.pack_indices(idx, b)
        short = full[:-1]
        got = run_map(plan, short, n)
        want = E.map_points(lut, E.fixed_indices(short, n, b), prec)
        assert got.dtype == want.dtype and np.array_equal(got, want), (kind, m, n)
        assert np.array_equal(run_map(plan, full, n), E.map_points(lut, idx, prec))
        z = E.round_input(E.decider_points(kind, lut, idx, rng), prec)
        assert run_demap(plan, z, (n * b + 7) // 8, prec) == full, (kind, m, n)


@PRECS
@pytest.mark.parametrize("n", [E.SECOND_TRIP_FLAT, E.SECOND_TRIP_DEMAP64])
def test_map_demap_second_trip(gpu, n, prec):
    """64-QAM at 2^20 + 257 symbols: more than 4096 workgroups of elements, the map's second trip.  The
    demap runs a thread per output BYTE, 786 625 of them there; its second trip needs 2^20 + 257 bytes,
    which 1 398 444 symbols give."""
    lut, b = O.qam_lut(64), 6
    rng = np.random.default_rng(64)
    idx = E.case_indices(64, n, rng)
    data = E.pack_indices(idx, b)
    assert (n + 255) // 256 > E.MAX_GRID
    assert ((len(data) + 255) // 256 > E.MAX_GRID) == (n == E.SECOND_TRIP_DEMAP64)
    plan = B.Plan(n_fft=64, precision=prec, luts=[lut])
    assert np.array_equal(run_map(plan, data, n), E.map_points(lut, idx, prec))
    z = E.round_input(E.qam_points(lut, idx, rng), prec)
    assert run_demap(plan, z, len(data), prec) == data


@PRECS
@pytest.mark.parametrize("S", E.ADAPTIVE_SYMS)
def test_map_demap_adaptive(gpu, S, prec):
    """N = 64, orders from {0, 4, 16, 64, 256}: inactive subcarriers exactly 0, whole bytes only."""
    orders = E.adaptive_case()
    n = len(orders)
    bps, offs, tot = E.adaptive_layout(orders)
    used = sorted({int(o) for o in orders if o})
    luts = [O.qam_lut(o) for o in used]
    sc = np.array([used.index(int(o)) if o else -1 for o in orders], np.int32)
    plan = B.Plan(n_fft=n, precision=prec, luts=luts, sc_lut=sc)
    assert plan.adaptive and plan.bits_per_ofdm_symbol == tot
    rng = np.random.default_rng(S)
    data = rng.integers(0, 256, size=(S * tot + 7) // 8, dtype=np.uint8).tobytes()
    idx = E.adaptive_indices(data, orders, S)
    want = np.zeros((S, n), E.cdtype(prec))
    z = np.zeros((S, n), np.complex128)
    for k in np.flatnonzero(bps):
        lut = O.qam_lut(int(orders[k]))
        want[:, k] = E.map_points(lut, idx[:, k], prec)
        z[:, k] = E.qam_points(lut, idx[:, k], rng)
    got = run_map(plan, data, S * n).reshape(S, n)
    assert np.array_equal(got, want)
    assert np.all(got[:, bps == 0] == 0)
    z[:, bps == 0] = 7.0 + 7.0j  # whatever an inactive subcarrier receives is ignored
    out = run_demap(plan, E.round_input(z.ravel(), prec), S * tot // 8, prec)
    assert out == E.adaptive_bytes(idx, orders) == data[: S * tot // 8]


# --------------------------------------------------------------------------- ofdm_demap_count


def run_count(plan, Z, tx, n_sym, prec, start=(0, 0)):
    d = dev(Z, prec)
    t = torch.from_numpy(np.frombuffer(tx, np.uint8).copy()).to("cuda")
    cnt = torch.tensor(list(start), dtype=torch.int64, device="cuda")
    B.check(B.lib().ofdm_demap_count(plan.handle, B.stream_ptr(), B.ptr(d), B.ptr(t), n_sym, B.ptr(cnt)))
    return tuple(cnt.cpu().tolist())


@PRECS
@pytest.mark.parametrize("m", [64, 1024])
def test_demap_count_wrong_decisions(gpu, m, prec):
    """Every point built around entry j while the transmitted bits say entry i != j: every symbol is an
    error and the bit errors are the popcounts of i ^ j, known exactly; the counters accumulate."""
    lut, b, N, S = O.qam_lut(m), int(np.log2(m)), 64, 9
    i, j, z = E.wrong_decisions(lut, S * N, np.random.default_rng(m))
    be, se = E.count_errors(j, i, b)
    assert se == S * N and be > se
    plan = B.Plan(n_fft=N, precision=prec, luts=[lut])
    got = run_count(plan, E.round_input(z, prec), E.pack_indices(i, b), S, prec, start=(5, 7))
    assert got == (5 + be, 7 + se)


@PRECS
def test_demap_count_second_trip(gpu, prec):
    """64-QAM, N = 64, 16 384 + 5 OFDM symbols: more than 4096 workgroups of elements; half the symbols
    decide wrongly, the counts exact."""
    lut, b, N, S = O.qam_lut(64), 6, 64, 16384 + 5
    rng = np.random.default_rng(65)
    n = S * N
    assert (n + 255) // 256 > E.MAX_GRID
    i, j, _ = E.wrong_decisions(lut, n, rng)
    j = np.where(rng.random(n) < 0.5, i, j)
    z = E.qam_points(lut, j, rng)
    be, se = E.count_errors(j, i, b)
    assert 0 < se < n
    plan = B.Plan(n_fft=N, precision=prec, luts=[lut])
    assert run_count(plan, E.round_input(z, prec), E.pack_indices(i, b), S, prec) == (be, se)


# --------------------------------------------------------------------------- ofdm_channel / _power / _awgn


def f64_record(v=0.0):
    return torch.tensor([v], dtype=torch.float64, device="cuda")


def channel_power_awgn(plan, L, n, prec, seed):
    """One length through ofdm_channel (without and with a record that starts at 3.5), ofdm_power of the
    result, ofdm_awgn at 10 and 60 dB with that power.  Returns the four worst ratios."""
    lib, st = B.lib(), B.stream_ptr()
    h = taps(L)
    s = E.round_input(E.rows_input(1, n, seed)[0], prec)
    sd = dev(s, prec)
    y0 = torch.full((n,), float("nan"), dtype=plan.cdtype, device="cuda")
    y1 = torch.full((n,), float("nan"), dtype=plan.cdtype, device="cuda")
    B.check(lib.ofdm_channel(plan.handle, st, B.ptr(sd), n, B.ptr(y0), None))
    rec = f64_record(3.5)
    B.check(lib.ofdm_channel(plan.handle, st, B.ptr(sd), n, B.ptr(y1), B.ptr(rec)))
    y = host(y0)
    assert np.array_equal(y, host(y1))
    r_conv = E.cmp_conv(y, s, h, prec)
    yw = y.astype(np.complex128)
    r_pow = E.cmp_power(float(rec.cpu()[0]), yw, prec, start=3.5)  # 3.5 + the sum: "+="
    pw = f64_record(0.0)
    B.check(lib.ofdm_power(plan.handle, st, B.ptr(y0), n, B.ptr(pw)))
    ps = float(pw.cpu()[0])
    r_pow = max(r_pow, E.cmp_power(ps, yw, prec))
    rng = np.random.default_rng(seed + 1)
    nr, ni = rng.normal(size=n), rng.normal(size=n)
    nrd, nid = dev(nr), dev(ni)
    r_awgn = 0.0
    for snr in (10.0, 60.0):
        yn = y0.clone()
        B.check(lib.ofdm_awgn(plan.handle, st, B.ptr(yn), n, B.ptr(nrd), B.ptr(nid), B.ptr(pw), snr))
        r_awgn = max(r_awgn, E.cmp_awgn(host(yn), yw, ps, snr, nr, ni, prec))
    return r_conv, r_pow, r_awgn


@PRECS
@pytest.mark.parametrize("L", E.CONV_TAPS)
def test_channel_power_awgn(gpu, L, prec):
    """len in {1, L - 1, L, 255, 256, 257, 1000}: every workgroup boundary n = 256 j between a sample and
    its taps, the 1000-sample case across three."""
    plan = B.Plan(n_fft=64, precision=prec, h_raw=taps(L))
    worst = np.zeros(3)
    for n in E.conv_lengths(L):
        r = channel_power_awgn(plan, L, n, prec, 500 + 7 * L + n)
        assert max(r) <= 1, (L, n, r)
        worst = np.maximum(worst, r)
    for name, r in zip(("ofdm_channel", "ofdm_power", "ofdm_awgn"), worst):
        report(f"{name}[L={L}]", prec, 0, float(r))


@PRECS
@pytest.mark.parametrize("L", E.CONV_TAPS)
def test_channel_power_awgn_second_trip(gpu, L, prec):
    """2^20 + 257 samples: 4098 workgroups of work on a grid of 4096."""
    plan = B.Plan(n_fft=64, precision=prec, h_raw=taps(L))
    r = channel_power_awgn(plan, L, E.SECOND_TRIP_FLAT, prec, 900 + L)
    for name, x in zip(("ofdm_channel", "ofdm_power", "ofdm_awgn"), r):
        report(f"second trip {name}[L={L}]", prec, 0, float(x), samples=E.SECOND_TRIP_FLAT)


# --------------------------------------------------------------------------- determinism and streams


@PRECS
def test_power_records_repeat_bit_for_bit_on_one_and_two_streams(gpu, prec):
    """ofdm_power, and ofdm_channel with a power record, twice on one stream and once on each of two side
    streams of the same plan, 2^20 + 257 samples each, launched back to back so the side streams overlap:
    the reductions keep one workspace per stream, and all four records are bit-identical."""
    lib = B.lib()
    n, L = E.SECOND_TRIP_FLAT, 4
    plan = B.Plan(n_fft=64, precision=prec, h_raw=taps(L))
    s = dev(E.rows_input(1, n, 77)[0], prec)
    ys = [torch.empty(n, dtype=plan.cdtype, device="cuda") for _ in range(4)]
    pw = [f64_record() for _ in range(4)]
    ch = [f64_record() for _ in range(4)]
    for i in (0, 1):
        B.check(lib.ofdm_channel(plan.handle, B.stream_ptr(), B.ptr(s), n, B.ptr(ys[i]), B.ptr(ch[i])))
        B.check(lib.ofdm_power(plan.handle, B.stream_ptr(), B.ptr(s), n, B.ptr(pw[i])))
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    for st in side:
        st.wait_stream(torch.cuda.current_stream())
    for i, st in zip((2, 3), side):  # back to back: nothing waits between the two streams' launches
        with torch.cuda.stream(st):
            B.check(lib.ofdm_channel(plan.handle, B.stream_ptr(), B.ptr(s), n, B.ptr(ys[i]), B.ptr(ch[i])))
            B.check(lib.ofdm_power(plan.handle, B.stream_ptr(), B.ptr(s), n, B.ptr(pw[i])))
    torch.cuda.synchronize()
    pws = [host(p).tobytes() for p in pw]
    chs = [host(c).tobytes() for c in ch]
    assert len(set(pws)) == 1 and len(set(chs)) == 1, (pws, chs)
    assert float(host(pw[0])[0]) > 0 and float(host(ch[0])[0]) > 0
    y0 = host(ys[0])
    for y in ys[1:]:
        assert np.array_equal(y0, host(y))
    sw = host(s).astype(np.complex128)
    assert E.cmp_power(float(host(pw[0])[0]), sw, prec) <= 1
    assert E.cmp_power(float(host(ch[0])[0]), y0.astype(np.complex128), prec) <= 1


# --------------------------------------------------------------------------- refusals and empty calls


def last_error():
    return B.lib().ofdm_last_error().decode()


def test_refusals_and_empty_calls(gpu):
    lib, st = B.lib(), B.stream_ptr()
    n = 64
    h = DEFAULT_4TAP
    p64 = B.Plan(n_fft=n, precision=B.OFDM_F64, equalizer=B.EQ_MMSE, h_raw=h)
    p32 = B.Plan(n_fft=n, precision=B.OFDM_F32, equalizer=B.EQ_MMSE, h_raw=h)
    # gains come from complex128 plans only; H alone from either, and identically
    H32 = torch.zeros(n, dtype=torch.complex128, device="cuda")
    g = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert lib.ofdm_plan_response(p32.handle, st, B.ptr(H32), B.ptr(g)) == -1
    assert last_error() == "gains are exported by float64 plans only"
    H32.zero_()
    assert lib.ofdm_plan_response(p32.handle, st, B.ptr(H32), None) == 0
    H64 = torch.zeros(n, dtype=torch.complex128, device="cuda")
    assert lib.ofdm_plan_response(p64.handle, st, B.ptr(H64), B.ptr(g)) == 0
    assert np.array_equal(host(H32), host(H64)) and np.any(host(H64) != 0)
    np.testing.assert_allclose(host(g), np.abs(np.fft.fft(h, n)) ** 2, rtol=1e-13, atol=1e-15)
    for prec in (B.OFDM_F64, B.OFDM_F32):
        dt = torch.complex64 if prec == B.OFDM_F32 else torch.complex128

        def canary(k):
            return torch.full((k,), 3.0 - 4.0j, dtype=dt, device="cuda")

        # an equaliser without a channel response
        nochan = B.Plan(n_fft=n, precision=prec, equalizer=B.EQ_ZF)
        a, z = canary(n), canary(n)
        assert lib.ofdm_equalize(nochan.handle, st, B.ptr(a), 1, 10.0, B.ptr(z)) == -1
        assert "no channel response" in last_error()
        assert lib.ofdm_demodulate(nochan.handle, st, B.ptr(a), 1, 10.0, B.ptr(z)) == -1
        assert "no channel response" in last_error()
        # adaptive map / demap take whole OFDM symbols
        sc = np.full(n, -1, np.int32)
        sc[:8] = 0
        ad = B.Plan(n_fft=n, precision=prec, luts=[O.qam_lut(16)], sc_lut=sc)
        by = torch.zeros(64, dtype=torch.uint8, device="cuda")
        assert lib.ofdm_map(ad.handle, st, B.ptr(by), 64, n + 1, B.ptr(canary(2 * n))) == -1
        assert "whole OFDM symbols" in last_error()
        assert lib.ofdm_demap(ad.handle, st, B.ptr(canary(2 * n)), n - 1, B.ptr(by)) == -1
        assert "whole OFDM symbols" in last_error()
        # negative counts are refused, zero counts are empty calls that touch nothing
        plan = B.Plan(n_fft=n, cp=4, precision=prec, equalizer=B.EQ_MMSE, h_raw=h, luts=[O.qam_lut(16)])
        src, out = canary(4 * (n + 4)), canary(4 * (n + 4))
        rec = f64_record(3.5)
        cnt = torch.tensor([11, 13], dtype=torch.int64, device="cuda")
        outb = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda")
        nr = torch.zeros(8, dtype=torch.float64, device="cuda")
        calls = {
            "ofdm_fft": lambda k: lib.ofdm_fft(plan.handle, st, B.ptr(out), k, 0),
            "ofdm_modulate": lambda k: lib.ofdm_modulate(plan.handle, st, B.ptr(src), k, B.ptr(out)),
            "ofdm_demodulate": lambda k: lib.ofdm_demodulate(plan.handle, st, B.ptr(src), k, 10.0, B.ptr(out)),
            "ofdm_equalize": lambda k: lib.ofdm_equalize(plan.handle, st, B.ptr(src), k, 10.0, B.ptr(out)),
            "ofdm_map": lambda k: lib.ofdm_map(plan.handle, st, B.ptr(by), 64 if k >= 0 else k, k, B.ptr(out)),
            "ofdm_demap": lambda k: lib.ofdm_demap(plan.handle, st, B.ptr(src), k, B.ptr(outb)),
            "ofdm_demap_count": lambda k: lib.ofdm_demap_count(plan.handle, st, B.ptr(src), B.ptr(by), k, B.ptr(cnt)),
            "ofdm_channel": lambda k: lib.ofdm_channel(plan.handle, st, B.ptr(src), k, B.ptr(out), B.ptr(rec)),
            "ofdm_power": lambda k: lib.ofdm_power(plan.handle, st, B.ptr(src), k, B.ptr(rec)),
            "ofdm_awgn": lambda k: lib.ofdm_awgn(plan.handle, st, B.ptr(out), k, B.ptr(nr), B.ptr(nr), B.ptr(rec), 10.0),
        }
        for name, call in calls.items():
            assert call(-1) == -1, name
            assert last_error(), name
            assert call(0) == 0, name
        torch.cuda.synchronize()
        assert torch.all(out == 3.0 - 4.0j) and torch.all(outb == CANARY)
        assert cnt.cpu().tolist() == [11, 13] and float(rec.cpu()[0]) == 3.5

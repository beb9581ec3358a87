"""The operator yardstick (tests/operator_expect.py) checked without a GPU: its references reproduce the
reference's stage fixtures; a float32 emulation of every operator in the kernels' operation order stays
inside its bound at every shape tests/test_gpu_operator_abi.py runs (the large counts cut to 4096
elements); and ten wrong variants -- a dropped tap, a restarted convolution, a shifted prefix copy, a short
ZP fold, a neighbour's or a mis-averaged MMSE noise variance, sigma from len - 1, a half-precision
twiddle table, LSB-first packing, a shifted adaptive bit offset -- are each REJECTED by the comparators
at every shape where they apply: the bounds, rigorous and therefore loose, still tell wrong from
imprecise."""

import math

import numpy as np
import pytest
from conftest import DEFAULT_4TAP, channel, load_stages, stage_arrays

import link_screen_expect as LS
import ofdm_oracle as O
import operator_expect as E

f32 = np.float32
CHANNELS = {"default4": DEFAULT_4TAP, "severe": channel("severe_multipath"), "decay32": E.decaying_taps()}


def taps(L):
    """The test channels by length: one tap, two and four of the default channel, the 32-tap draw."""
    return {1: np.array([0.8 - 0.6j]), 2: DEFAULT_4TAP[:2], 4: DEFAULT_4TAP, 32: E.decaying_taps()}[L]


# --------------------------------------------------------------------------- float32 emulations


def cmul32(ar, ai, br, bi):
    """cmul in float32: (ar br - ai bi, ar bi + ai br), every operation rounded."""
    return (ar * br - ai * bi).astype(f32), (ar * bi + ai * br).astype(f32)


def conv32(s, h_raw, restart=None):
    """k_conv<float>: the normalised taps rounded once, v += cmul(h[l], s[n - l]) from l = 0.
    restart: a mutation -- s[n - l] read as 0 across every multiple of `restart`."""
    h = O.normalize_h(np.asarray(h_raw, np.complex128)).astype(np.complex64)
    s = np.asarray(s, np.complex64)
    n = np.arange(len(s))
    vr, vi = np.zeros(len(s), f32), np.zeros(len(s), f32)
    for l in range(len(h)):
        ok = n - l >= 0
        if restart:
            ok &= (n - l) // restart == n // restart
        sl = np.where(ok, s[np.maximum(n - l, 0)], 0).astype(np.complex64)
        tr, ti = cmul32(f32(h[l].real), f32(h[l].imag), sl.real, sl.imag)
        vr, vi = (vr + tr).astype(f32), (vi + ti).astype(f32)
    return vr.astype(np.float64) + 1j * vi.astype(np.float64)


def conv64(s, h_raw, restart=None, drop=None):
    """The convolution in double, serially, with the mutations: restart as conv32, drop = a tap set to 0
    AFTER the normalisation (the kernel's table with one entry missing)."""
    h = O.normalize_h(np.asarray(h_raw, np.complex128)).copy()
    if drop is not None:
        h[drop] = 0
    n = np.arange(len(s))
    v = np.zeros(len(s), np.complex128)
    for l in range(len(h)):
        ok = n - l >= 0
        if restart:
            ok &= (n - l) // restart == n // restart
        v += h[l] * np.where(ok, s[np.maximum(n - l, 0)], 0)
    return v


def awgn32(y, sigma, nr, ni):
    """k_awgn<float>: sg = (float)sigma; v.re += sg * (float)nr; v.im += sg * (float)ni."""
    y = np.asarray(y, np.complex64)
    sg = f32(sigma)
    re = (y.real + (sg * nr.astype(f32)).astype(f32)).astype(f32)
    im = (y.imag + (sg * ni.astype(f32)).astype(f32)).astype(f32)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def tree32(p):
    """Pairwise float32 sum over the last axis (a power of two): the shuffle tree of the reductions."""
    while p.shape[-1] > 1:
        p = (p[..., 0::2] + p[..., 1::2]).astype(f32)
    return p[..., 0]


def equalize32(Y, H, eq, snr_db, mean_over=None, nv_roll=0):
    """k_equalize<float> / the equaliser of k_rows<float, LOGN, 2>: the tables rounded once from double,
    |Y|^2 summed serially per thread (elements t, t + T, ...) and then over the threads in a tree, nv and
    the weight in float32.  mean_over / nv_roll: mutations (the mean's divisor; nv of row r + nv_roll)."""
    Y = np.asarray(Y, np.complex64)
    rows, n = Y.shape
    if eq == "NONE":
        return Y.astype(np.complex128)
    yr, yi = Y.real, Y.imag
    if eq == "ZF":
        w = (1.0 / np.where(H == 0, 1e-10, H)).astype(np.complex64)
        zr, zi = cmul32(yr, yi, w.real[None, :], w.imag[None, :])
        return zr.astype(np.float64) + 1j * zi.astype(np.float64)
    g = np.mean(np.abs(H) ** 2)
    p2 = ((yr * yr).astype(f32) + (yi * yi).astype(f32)).astype(f32)
    T = min(n, 256)
    part = np.zeros((rows, T), f32)
    for i in range(n // T):                      # serial per thread
        part = (part + p2[:, i * T:(i + 1) * T]).astype(f32)
    p = tree32(part)
    if g == 0:
        nv = np.full(rows, np.inf, f32)
    else:
        nv = (((p / f32(mean_over or n)).astype(f32) / f32(10 ** (snr_db / 10))).astype(f32) / f32(g)).astype(f32)
    nv = np.roll(nv, nv_roll)
    d = ((np.abs(H) ** 2).astype(f32)[None, :] + nv[:, None]).astype(f32)
    hc = np.conj(H).astype(np.complex64)
    with np.errstate(invalid="ignore"):
        wr, wi = (hc.real[None, :] / d).astype(f32), (hc.imag[None, :] / d).astype(f32)
    zr, zi = cmul32(yr, yi, wr, wi)
    return zr.astype(np.float64) + 1j * zi.astype(np.float64)


def numpy_rows32(x, inverse):
    """numpy's complex64 transform (pocketfft in float32): an independent float32 implementation."""
    x = np.asarray(x, np.complex64)
    out = np.fft.ifft(x, axis=1, norm="ortho") if inverse else np.fft.fft(x, axis=1, norm="ortho")
    assert out.dtype == np.complex64
    return out


def table_fft32(x, inverse, half_table=False):
    """A radix-2 float32 transform with the kernels' twiddle scheme: W^m = lo[m & 63] * hi[m >> 6], both
    tables rounded once from double, the ortho scale rounded and multiplied in at the load.
    half_table: the mutation -- the lo table rounded to half precision."""
    x = np.asarray(x, np.complex64)
    rows, n = x.shape
    t = int(round(math.log2(n)))
    j = np.arange(64)
    lo = np.exp(-2j * np.pi * (j % n) / n).astype(np.complex64)
    hi = np.exp(-2j * np.pi * ((64 * j) % n) / n).astype(np.complex64)
    if half_table:
        lo = (lo.real.astype(np.float16).astype(f32) + 1j * lo.imag.astype(np.float16).astype(f32)).astype(np.complex64)
    rev = np.array([int(format(i, f"0{t}b")[::-1], 2) if t else 0 for i in range(n)])
    v = (x[:, rev] * f32(1.0 / math.sqrt(n))).astype(np.complex64)
    for s in range(1, t + 1):
        half, stride = 1 << (s - 1), n >> s
        m = np.arange(half) * stride
        w = (lo[m & 63] * hi[m >> 6]).astype(np.complex64)
        if inverse:
            w = np.conj(w)
        v = v.reshape(rows, n >> s, 2, half)
        a, b = v[:, :, 0, :], (v[:, :, 1, :] * w).astype(np.complex64)
        v = np.stack([a + b, a - b], axis=2).astype(np.complex64).reshape(rows, n)
    return v


# --------------------------------------------------------------------------- the yardstick's own pieces


def test_eta_is_the_screen_yardsticks_in_float32():
    assert E.higham_eta(E.U32, 4 * E.U32) == LS.higham_eta(mu=4 * LS.U)
    # two-level twiddles cost 1.45 of once-rounded ones; the rigorous bound at N = 1024 is ~1e-5 of the norm
    assert 1.4 < E.higham_eta(E.U32, 4 * E.U32) / E.higham_eta(E.U32, E.U32) < 1.5
    assert 90 * E.U32 < E.rows_rel(1024, E.F32) < 100 * E.U32
    assert E.rows_rel(1, E.F32) == E.rows_rel(2, E.F32)          # t = max(log2 N, 1)
    assert [E.spb(1 << l) for l in range(13)] == [256] * 5 + [128, 64, 32, 16, 8, 4, 2, 1]


def test_worst_treats_zero_bounds_as_exact():
    assert E.worst(np.array([0.0, 1.0]), np.array([0.0, 2.0])) == 0.5
    assert E.worst(np.array([1e-300, 1.0]), np.array([0.0, 2.0])) == math.inf
    assert E.worst(np.array([np.nan]), np.array([1.0])) == math.inf
    assert E.worst(np.zeros(3), np.zeros(3)) == 0.0


@pytest.mark.parametrize("st", load_stages(), ids=lambda s: s["name"])
def test_references_reproduce_the_stage_fixtures(st):
    """x, y_clean, y, Z, rx_bytes of the reference's own stages, to test_oracle_golden.py's tolerances."""
    a = stage_arrays(st["name"])
    N, M, cp, snr = st["N"], st["M"], st["cp"], st["snr_db"]
    b = int(np.log2(M))
    lut = O.qam_lut(M)
    idx = E.fixed_indices(a["tx_bytes"].tobytes(), a["X"].size, b)
    assert np.array_equal(E.map_points(lut, idx, E.F64).reshape(-1, N), a["X"])
    np.testing.assert_allclose(E.ref_modulate(a["X"], cp), a["x"], rtol=0, atol=1e-12)
    y_clean = E.ref_conv(a["x"].ravel(), a["h_raw"])
    np.testing.assert_allclose(y_clean, a["y_clean"], rtol=0, atol=1e-12)
    ps = float(np.sum(np.abs(y_clean) ** 2))
    y = E.ref_awgn(y_clean, ps, len(y_clean), snr, a["noise_re"], a["noise_im"])
    np.testing.assert_allclose(y, a["y"], rtol=0, atol=1e-12)
    Z = E.ref_demodulate(a["y"].reshape(-1, N + cp), N, cp, False, a["H"], st["eq"], snr)
    np.testing.assert_allclose(Z, a["Z"], rtol=1e-9, atol=1e-9)
    Y = E.ref_demod_rows(a["y"].reshape(-1, N + cp), N, cp)
    np.testing.assert_allclose(E.eq_weights(Y, a["H"], st["eq"], snr) * Y, a["Z"], rtol=1e-9, atol=1e-9)
    assert O.indices_to_bytes(O.nn_demap(a["Z"].ravel(), lut), b) == a["rx_bytes"].tobytes()
    # the fixtures pass their own comparators in complex128
    assert E.cmp_modulate(a["x"], a["X"], cp, False, E.F64) <= 1
    assert E.cmp_conv(a["y_clean"], a["x"].ravel(), a["h_raw"], E.F64) <= 1
    assert E.cmp_awgn(a["y"], a["y_clean"], ps, snr, a["noise_re"], a["noise_im"], E.F64) <= 1


# --------------------------------------------------------------------------- rows: emulations and mutations


def demod_H(n, name):
    return np.fft.fft(CHANNELS[name], n) if n >= len(CHANNELS[name]) else np.fft.fft(CHANNELS[name][:n], n)


@pytest.mark.parametrize("logn", E.LOGNS)
def test_float32_transforms_stay_inside_the_rows_bound(logn):
    """numpy's complex64 transform and the table emulation, both directions, every row count; the report
    pins numpy's share of the rigorous bound (0.02 at N = 1024)."""
    n = 1 << logn
    worst_np = 0.0
    for rows in E.row_counts(n):
        x = E.round_input(E.rows_input(rows, n, 100 + logn), E.F32)
        for inv in (0, 1):
            r_np = E.cmp_fft(numpy_rows32(x, inv), x, inv, E.F32)
            r_tab = E.cmp_fft(table_fft32(x, inv), x, inv, E.F32)
            assert r_np <= 1 and r_tab <= 1, (n, rows, inv, r_np, r_tab)
            worst_np = max(worst_np, r_np)
            if n >= 8:  # mutation 8 (N <= 4: every twiddle is 1 or -i, exact in half precision)
                assert E.cmp_fft(table_fft32(x, inv, half_table=True), x, inv, E.F32) > 1, (n, rows, inv)
    print(f"numpy complex64 fft N={n}: {worst_np:.3f} of the rows bound")
    if n == 1024:
        assert worst_np < 0.05


@pytest.mark.parametrize("logn", E.LOGNS)
def test_float32_modulate_and_its_prefix_mutation(logn):
    n = 1 << logn
    for cp, zp in E.prefixes(n):
        for rows in E.row_counts(n):
            X = E.round_input(E.rows_input(rows, n, 200 + logn), E.F32)
            body = numpy_rows32(X, 1)
            got = np.concatenate([body, np.zeros((rows, cp), np.complex64)], 1) if zp else O.add_cp(body, cp)
            assert E.cmp_modulate(got, X, cp, zp, E.F32) <= 1, (n, cp, zp, rows)
            if not zp and cp >= 1 and n >= 2:
                # mutation 3: the prefix copied from N - cp + m - 1 (in complex128: only the index is wrong)
                ref = E.ref_modulate(X, cp)
                bad = ref.copy()
                bad[:, :cp] = ref[:, cp:][:, (n - cp + np.arange(cp) - 1) % n]
                assert E.cmp_modulate(ref, X, cp, zp, E.F64) <= 1
                assert E.cmp_modulate(bad, X, cp, zp, E.F64) > 1, (n, cp, rows)
            if zp:
                bad = got.copy()
                bad[0, n] = 1e-30  # a guard sample that is not exactly zero
                assert E.cmp_modulate(bad, X, cp, zp, E.F32) == math.inf


@pytest.mark.parametrize("logn", E.LOGNS)
def test_float32_demodulate_and_its_mutations(logn):
    n = 1 << logn
    snr = E.DEMOD_SNR_DB
    H = demod_H(n, "severe")
    for cp, zp in E.prefixes(n):
        for rows in E.row_counts(n):
            yt = E.round_input(E.rows_input(rows, n + cp, 300 + logn, scaled=True), E.F32)
            Y32 = numpy_rows32(E.fold(yt.astype(np.complex64), n, cp, zp), 0)
            for eq in E.EQ_NAMES:
                got = equalize32(Y32, H, eq, snr)
                assert E.cmp_demodulate(got, yt, n, cp, zp, H, eq, snr, E.F32) <= 1, (n, cp, zp, rows, eq)
            # mutations, in complex128 so that only the mutation differs
            Y = E.ref_demod_rows(yt, n, cp, zp)
            assert E.cmp_demodulate(O.equalize(Y, H, "MMSE", snr), yt, n, cp, zp, H, "MMSE", snr, E.F64) <= 1
            if zp:  # 4: the fold applied to cp - 1 samples
                bad = np.fft.fft(E.fold(yt, n, cp, zp, fold_len=cp - 1), axis=1, norm="ortho")
                assert E.cmp_demodulate(bad, yt, n, cp, zp, H, "NONE", snr, E.F64) > 1, (n, cp, rows)
            w = E.eq_weights(Y, H, "MMSE", snr)
            if rows >= 2:  # 5: nv of the neighbouring row
                sp =np.mean(np.abs(Y) ** 2, axis=1, keepdims=True)
                nv = np.roll((sp / 10 ** (snr / 10)) / np.mean(np.abs(H) ** 2), 1, axis=0)
                bad = Y * (np.conj(H)[None, :] / (np.abs(H)[None, :] ** 2 + nv))
                assert E.cmp_demodulate(bad, yt, n, cp, zp, H, "MMSE", snr, E.F64) > 1, (n, cp, rows)
            if cp >= 1:  # 6: the mean over N + cp instead of N
                sp = np.sum(np.abs(Y) ** 2, axis=1, keepdims=True) / (n + cp)
                nv = (sp / 10 ** (snr / 10)) / np.mean(np.abs(H) ** 2)
                bad = Y * (np.conj(H)[None, :] / (np.abs(H)[None, :] ** 2 + nv))
                assert E.cmp_demodulate(bad, yt, n, cp, zp, H, "MMSE", snr, E.F64) > 1, (n, cp, rows)


def equalize_cases():
    for n in E.EQUALIZE_N:
        for rows in (1, 3):
            yield n, rows
    yield 2, min(E.MAX_GRID + 5, E.CPU_CUT // 2)  # the second trip, cut


@pytest.mark.parametrize("n,rows", list(equalize_cases()))
def test_float32_equalize_and_its_mutations(n, rows):
    snr = E.DEMOD_SNR_DB
    Y = E.round_input(E.rows_input(rows, n, 400 + n, scaled=True), E.F32)
    H = demod_H(n, "default4")
    for eq in E.EQ_NAMES:
        assert E.cmp_equalize(equalize32(Y, H, eq, snr), Y, H, eq, snr, E.F32) <= 1, (n, rows, eq)
    if rows >= 2:
        assert E.cmp_equalize(equalize32(Y, H, "MMSE", snr, nv_roll=1), Y, H, "MMSE", snr, E.F32) > 1
    assert E.cmp_equalize(equalize32(Y, H, "MMSE", snr, mean_over=n + 1), Y, H, "MMSE", snr, E.F32) > 1
    # a null bin under ZF: the 1e-10 substitution, finite in float32; an all-zero H under MMSE: all 0
    Hn = H.copy()
    Hn[n // 2] = 0
    got = equalize32(Y, Hn, "ZF", snr)
    assert np.all(np.isfinite(got)) and E.cmp_equalize(got, Y, Hn, "ZF", snr, E.F32) <= 1
    got = equalize32(Y, np.zeros(n, complex), "MMSE", snr)
    assert np.all(got == 0) and E.cmp_equalize(got, Y, np.zeros(n, complex), "MMSE", snr, E.F32) == 0.0


# --------------------------------------------------------------------------- convolution, power, noise


def conv_cases():
    for L in E.CONV_TAPS:
        for n in E.conv_lengths(L) + [E.CPU_CUT]:  # the second-trip length, cut
            yield L, n


@pytest.mark.parametrize("L,n", list(conv_cases()))
def test_float32_convolution_and_its_mutations(L, n):
    h = taps(L)
    s = E.round_input(E.rows_input(1, n, 500 + L)[0], E.F32)
    r = E.cmp_conv(conv32(s, h), s, h, E.F32)
    assert r <= 1, (L, n, r)
    assert E.cmp_conv(conv64(s, h), s, h, E.F64) <= 1
    small = int(np.argmin(np.abs(h)))
    if L >= 2 and n > small:  # 1: the smallest tap dropped (it reaches sample n >= its index)
        assert E.cmp_conv(conv64(s, h, drop=small), s, h, E.F32) > 1, (L, n)
    if L >= 2 and n > 256:    # 2: restarted at every 256-sample boundary
        assert E.cmp_conv(conv32(s, h, restart=256), s, h, E.F32) > 1, (L, n)
        assert E.cmp_conv(conv64(s, h, restart=256), s, h, E.F64) > 1, (L, n)


def test_smallest_tap_of_the_decaying_channel_is_seen_everywhere():
    """The smallest tap of the 32-tap draw (|h_27| = 0.0008 after normalisation) replaced by zero puts
    nearly every sample of a float32 comparison over the bound, and the emulation itself sits well inside."""
    h = E.decaying_taps()
    hn = O.normalize_h(h)
    small = int(np.argmin(np.abs(hn)))
    assert small == 27 and 7e-4 < abs(hn[small]) < 9e-4
    s = E.round_input(E.rows_input(1, 4096, 77)[0], E.F32)
    err = np.abs(conv64(s, h, drop=small) - E.ref_conv(s, h))
    assert np.mean(err[small:] > E.conv_bound(s, h, E.F32)[small:]) > 0.98
    assert E.cmp_conv(conv32(s, h), s, h, E.F32) < 0.5


@pytest.mark.parametrize("L,n", list(conv_cases()))
@pytest.mark.parametrize("snr", [10.0, 60.0])
def test_float32_noise_and_sigma_from_len_minus_one(L, n, snr):
    rng = np.random.default_rng(600 + n)
    y = E.round_input(E.ref_conv(E.rows_input(1, n, 600 + L)[0], taps(L)), E.F32)
    nr, ni = rng.normal(size=n), rng.normal(size=n)
    ps = float(np.sum(np.abs(y) ** 2))
    assert E.cmp_power(float(np.sum((y.real.astype(f32) ** 2 + y.imag.astype(f32) ** 2).astype(np.float64))),
                       y, E.F32) <= 1
    assert E.cmp_power(3.5 + ps, y, E.F64, start=3.5) <= 1 and E.cmp_power(ps, y, E.F64, start=3.5) > 1
    if ps == 0:
        return
    sg = E.sigma_of(ps, n, snr)
    assert E.cmp_awgn(awgn32(y, sg, nr, ni), y, ps, snr, nr, ni, E.F32) <= 1
    assert E.cmp_awgn(E.ref_awgn(y, ps, n, snr, nr, ni), y, ps, snr, nr, ni, E.F64) <= 1
    if n >= 2:  # 7: sigma from len - 1.  In complex128 always seen; in complex64 wherever the change of
        # sigma, sigma / (2 len), exceeds the rounding the bound allows: 5u (|y| + sigma |n|) ~ 5u |y| at
        # 60 dB, i.e. up to len ~ sigma / (10 u rms) -- the 10 dB cases, and the short ones at 60 dB
        bad = y + E.sigma_of(ps, n - 1, snr) * (nr + 1j * ni)
        assert E.cmp_awgn(bad, y, ps, snr, nr, ni, E.F64) > 1, (L, n, snr)
        if snr == 10.0 or n <= 257:
            assert E.cmp_awgn(bad, y, ps, snr, nr, ni, E.F32) > 1, (L, n, snr)


# --------------------------------------------------------------------------- the deciders' inputs


@pytest.mark.parametrize("kind,m", E.FIXED_ORDERS)
def test_decider_inputs_are_off_every_boundary(kind, m):
    """Every generated point decides to the entry it was built around, in double and after rounding to
    float32, with room to spare: no case is excluded.  Mutation 9: LSB-first packing is seen at every
    count."""
    lut = E.make_lut(kind, m)
    b = int(np.log2(m))
    rng = np.random.default_rng(m)
    idx = np.concatenate([np.arange(m), E.case_indices(m, 2 * m + 257, rng)])
    z = E.decider_points(kind, lut, idx, rng)
    for prec in (E.F64, E.F32):
        zz = E.round_input(z, prec)
        d = np.abs(zz[:, None] - lut[None, :]) if m <= 256 else None
        if d is not None:
            best = np.argmin(d, axis=1)
            assert np.array_equal(best, idx)
            srt = np.sort(d, axis=1)
            assert np.all(srt[:, 1] - srt[:, 0] > 1e-3 * srt[:, 1])  # far from any tie
        else:
            assert np.array_equal(O.nn_demap(zz, lut), idx)
    i, j, zw = E.wrong_decisions(lut, 4 * m + 5, rng, kind)
    assert np.all(i != j) and np.array_equal(O.nn_demap(zw, lut), j)
    be, se = E.count_errors(j, i, b)
    assert se == len(i) and be >= se
    for n in E.MAP_COUNTS:
        ix = E.case_indices(m, n, np.random.default_rng(n))
        bits = ((ix[:, None] >> np.arange(b - 1, -1, -1)) & 1).astype(np.uint8).ravel()
        assert np.packbits(bits).tobytes() == E.pack_indices(ix, b)
        assert np.packbits(bits, bitorder="little").tobytes() != E.pack_indices(ix, b), (m, n)
        # the map reads its input one byte short of n b bits: the missing bits are zeros
        data = E.pack_indices(ix, b)
        short = data[:-1]
        got = E.fixed_indices(short, n, b)
        keep = (len(short) * 8) // b
        assert np.array_equal(got[:keep], ix[:keep]) and len(got) == n


@pytest.mark.parametrize("S", E.ADAPTIVE_SYMS)
def test_adaptive_layout_and_shifted_offset(S):
    """Mutation 10: the bit offset of one subcarrier shifted by one changes the mapped indices and the
    demapped bytes at every S."""
    orders = E.adaptive_case()
    bps, offs, tot = E.adaptive_layout(orders)
    rng = np.random.default_rng(S)
    data = rng.integers(0, 256, size=(S * tot + 7) // 8, dtype=np.uint8).tobytes()
    idx = E.adaptive_indices(data, orders, S)
    assert np.all(idx[:, bps == 0] == 0)
    assert E.adaptive_bytes(idx, orders) == data[: S * tot // 8]
    k = int(np.flatnonzero(bps == bps.max())[1])
    bad = offs.copy()
    bad[k] -= 1
    assert not np.array_equal(E.adaptive_indices(data, orders, S, offs=bad), idx)
    assert E.adaptive_bytes(idx, orders, offs=bad) != E.adaptive_bytes(idx, orders)

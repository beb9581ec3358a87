"""Expected per-subcarrier profile rows (ofdm_rx_profile, include/ofdm_hip.h) from a run's equalised
symbols, restated with the oracle's demapper: what tests/test_profile_cpu.py and
tests/test_gpu_profile.py compare the device record against.

The rows of subcarrier k over the S symbols of Z:
  bit errors     popcount(rx index ^ tx index) over the bits whose position in the run's bit stream
                 (symbol s at s * sum(b), subcarrier k at its offset, MSB first) is < n_valid_bits
  symbol errors  rx index != tx index (every symbol: the partial-byte rule masks bits only)
  error power    sum of min(|Z - c|^2, 2^20), c the transmitted LUT point
  clipped        samples whose |Z - c|^2 reached 2^20 or is not finite
"""

import numpy as np

import ofdm_oracle as O

CAP = 2.0 ** 20


def luts_for(orders, scheme="QAM"):
    make = O.psk_lut if scheme == "PSK" else O.qam_lut
    return {int(o): make(int(o)) for o in np.unique(orders) if o > 0}


def tx_indices(tx_bytes, bk, S):
    """(S, N) transmitted constellation indices from the run's packed bytes: OFDM symbol s takes
    sum(bk) bits, subcarrier k its bk[k] bits in subcarrier order, MSB first (zeros past the end)."""
    bk = np.asarray(bk, np.int64)
    tot = int(bk.sum())
    bits = O.bytes_to_bits(np.asarray(tx_bytes, np.uint8).tobytes()).astype(np.int64)
    need = S * tot
    if len(bits) < need:
        bits = np.concatenate([bits, np.zeros(need - len(bits), np.int64)])
    rows = bits[:need].reshape(S, tot)
    off = np.concatenate([[0], np.cumsum(bk)[:-1]])
    idx = np.zeros((S, len(bk)), np.int64)
    for b in np.unique(bk[bk > 0]):
        for k in np.flatnonzero(bk == b):
            idx[:, k] = O.bits_to_indices(rows[:, off[k]:off[k] + b].ravel(), int(b))
    return idx


def expected_rows(Z, idx, bk, n_valid_bits, scheme="QAM"):
    """dict(bit_errors, symbol_errors, clipped: int64 [N]; error_power: float64 [N]) of the (S, N)
    equalised symbols Z against the transmitted indices idx, bk bits per subcarrier (0 = inactive)."""
    Z = np.asarray(Z, np.complex128)
    S, N = Z.shape
    bk = np.asarray(bk, np.int64)
    tot = int(bk.sum())
    off = np.concatenate([[0], np.cumsum(bk)[:-1]])
    luts = luts_for(np.where(bk > 0, 1 << bk, 0), scheme)
    be = np.zeros(N, np.int64)
    se = np.zeros(N, np.int64)
    cl = np.zeros(N, np.int64)
    ep = np.zeros(N, np.float64)
    sym = np.arange(S, dtype=np.int64)
    for order, lut in luts.items():
        b = order.bit_length() - 1
        cols = np.flatnonzero(bk == b)
        z = Z[:, cols]
        ridx = O.nn_demap(z.ravel(), lut).reshape(S, len(cols))
        tidx = idx[:, cols]
        diff = ridx ^ tidx
        se[cols] = np.count_nonzero(diff, axis=0)
        for j in range(b):  # bit j, MSB first
            pos = sym[:, None] * tot + (off[cols] + j)[None, :]
            bit = (diff >> (b - 1 - j)) & 1
            be[cols] += np.count_nonzero((bit == 1) & (pos < n_valid_bits), axis=0)
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.abs(z - lut[tidx]) ** 2
        clip = ~(p < CAP)
        cl[cols] = np.count_nonzero(clip, axis=0)
        ep[cols] = np.where(clip, CAP, p).sum(axis=0)
    return {"bit_errors": be, "symbol_errors": se, "clipped": cl, "error_power": ep}


def power_bound(Z, error_power, delta, factor=1.0):
    """Bound on |device error power - expected| per subcarrier when every device symbol is within
    delta_k = delta (1 + max_s |Z_sk|) of Z (the project's tolerance on Z: rtol = atol = delta):
    |dEP_k| <= 2 delta_k sqrt(S EP_k) + S delta_k^2 (Cauchy-Schwarz) + S 2^-41 (each sample is
    rounded once to 2^-40).  factor 2 for a comparison of two device runs."""
    Z = np.asarray(Z, np.complex128)
    S = Z.shape[0]
    with np.errstate(invalid="ignore"):
        zmax = np.nanmax(np.where(np.isfinite(np.abs(Z)), np.abs(Z), 0.0), axis=0)
    dk = delta * (1.0 + zmax)
    return factor * (2.0 * dk * np.sqrt(S * np.asarray(error_power)) + S * dk ** 2 + S * 2.0 ** -41)


def record_rows(rec):
    """The same dict from a normalised int64 [5][N] record (engine.combine_profile)."""
    rec = np.asarray(rec, np.int64)
    return {"bit_errors": rec[0], "symbol_errors": rec[1], "clipped": rec[4],
            "error_power": rec[3].astype(np.float64) * 2.0 ** -8 + rec[2].astype(np.float64) * 2.0 ** -40}


# ---------------------------------------------------------------- throughput cases (bench shapes)
# Philox streams, complex128, seed 77, S = 32 * 4096 / N + 35 symbols (the dispatch matrix's rule:
# two workgroups of the throughput receivers, a partial last one, a ragged symbol group).  The
# counts are the oracle's (philox_streams.run_philox) with decision brackets of width 0
# (tests/test_profile_cpu.py), so a GPU run has to reproduce them exactly.
SEED = 77
THROUGHPUT_CASES = [
    dict(id="n1024_m64_flat_none", N=1024, M=64, channel="flat_fading", eq="NONE", snr=24.0, S=163,
         bit_errors=167, symbol_errors=151),
    dict(id="n1024_m64_severe_mmse", N=1024, M=64, channel="severe_multipath", eq="MMSE", snr=24.0, S=163,
         bit_errors=2647, symbol_errors=2294),
    dict(id="n2048_adaptive_p1_mmse", N=2048, M=0, channel="Lin-Phoong_P1", eq="MMSE", snr=15.0, S=99,
         bit_errors=207, symbol_errors=207),
    dict(id="n4096_m256_p1_mmse", N=4096, M=256, channel="Lin-Phoong_P1", eq="MMSE", snr=30.0, S=67,
         bit_errors=21903, symbol_errors=16237),
]


def matrix_symbols(N):
    return 32 * 4096 // N + 35


def case_channel(case):
    """(h, cp, orders): the case's CIR, its prefix (ratio 1) and, for M = 0, the CAPACITY_BASED
    water-filling orders at desired SER 1e-3 (else None)."""
    from conftest import channel

    h = channel(case["channel"])
    cp = len(h) - 1
    orders = None
    if case["M"] == 0:
        orders, _, _ = O.adaptive_orders(case["N"], h, case["snr"], 1e-3, True)
    return h, cp, orders


def np_radius(words):
    """float32 NumPy stand-in for the hardware noise radius sqrt(32 - log2(float32(w | 1)))
    (as tests/test_dispatch_model.py)."""
    f = (np.asarray(words, np.uint32) | np.uint32(1)).astype(np.float32)
    return np.sqrt(np.float32(32) - np.log2(f))

"""Expected per-frame error records (ofdm_rx_frames, include/ofdm_hip.h) restated on the CPU: what
tests/test_frames_cpu.py and tests/test_gpu_frames.py compare the device record and
engine.FrameStats against.

Per OFDM symbol s of a run (bk[k] bits on subcarrier k, sum(bk) bits per symbol, subcarrier-major,
MSB first):
  bit errors     differing bits of the symbol whose position in the run's bit stream is < n_valid
  symbol errors  subcarriers whose transmitted and received indices differ in any bit
A frame is F consecutive symbols: frame f sums symbols [f F, (f + 1) F); the last one may be partial.
"""

import json
import math
import os

import numpy as np
from conftest import GOLDEN, load_stages

import ofdm_oracle as O
import profile_expect as PE


def all_stages():
    """Every stage fixture: stages.json and the wide-order one."""
    with open(os.path.join(GOLDEN, "stages_wide.json")) as f:
        return load_stages() + json.load(f)


def _bit_rows(raw, S, tot):
    bits = O.bytes_to_bits(np.asarray(raw, np.uint8).tobytes()).astype(np.int64)
    if len(bits) < S * tot:
        bits = np.concatenate([bits, np.zeros(S * tot - len(bits), np.int64)])
    return bits[:S * tot].reshape(S, tot)


def per_symbol_from_bytes(tx_bytes, rx_bytes, bk, S, n_valid):
    """(bit errors, symbol errors), int64 [S] each, from the run's transmitted and received packed
    bytes (zeros past the end of either)."""
    bk = np.asarray(bk, np.int64)
    tot = int(bk.sum())
    diff = _bit_rows(tx_bytes, S, tot) ^ _bit_rows(rx_bytes, S, tot)
    pos = np.arange(S, dtype=np.int64)[:, None] * tot + np.arange(tot, dtype=np.int64)[None, :]
    be = np.count_nonzero((diff == 1) & (pos < n_valid), axis=1).astype(np.int64)
    edges = np.concatenate([[0], np.cumsum(bk)])
    se = np.zeros(S, np.int64)
    for k in np.flatnonzero(bk > 0):
        se += diff[:, edges[k]:edges[k + 1]].any(axis=1)
    return be, se


def per_symbol_from_z(Z, idx, bk, n_valid, scheme="QAM", sym0=0):
    """The same from the (S, N) equalised symbols Z and the transmitted indices idx through the
    oracle's demapper, one symbol at a time (profile_expect.expected_rows over a one-symbol run whose
    bit positions start at symbol sym0 + s)."""
    Z = np.asarray(Z, np.complex128)
    S = Z.shape[0]
    bk = np.asarray(bk, np.int64)
    tot = int(bk.sum())
    be = np.zeros(S, np.int64)
    se = np.zeros(S, np.int64)
    for s in range(S):
        # (expected_rows places its first symbol at bit 0: shift the valid count instead)
        rows = PE.expected_rows(Z[s:s + 1], idx[s:s + 1], bk, n_valid - (sym0 + s) * tot, scheme)
        be[s] = int(rows["bit_errors"].sum())
        se[s] = int(rows["symbol_errors"].sum())
    return be, se


def frame_sums(per_symbol, F, sym0=0):
    """int64 [ceil((sym0 + S) / F)]: the per-symbol counts of global symbols [sym0, sym0 + S) summed
    into frames of F global symbols."""
    v = np.asarray(per_symbol, np.int64)
    n = -(-(sym0 + len(v)) // F)
    out = np.zeros(n, np.int64)
    np.add.at(out, (sym0 + np.arange(len(v))) // F, v)
    return out


def stats(bit_errors, n_symbols, F, bits_per_symbol, whole=True):
    """FrameStats' derived quantities in plain NumPy: dict(n_full, frame_errors, fer, hist, ber_stderr)
    over the n_symbols // F full frames (whole: every bit of the run was compared)."""
    e = np.asarray(bit_errors, np.int64)[:n_symbols // F]
    n = len(e)
    out = {"n_full": n, "frame_errors": int((e > 0).sum()), "fer": None, "hist": np.bincount(e), "ber_stderr": None}
    if n:
        out["fer"] = out["frame_errors"] / n
    if n >= 2 and whole:
        out["ber_stderr"] = float(np.std(e, ddof=1)) / math.sqrt(n) / (F * bits_per_symbol)
    return out

"""The fused launchers' dispatch rules restated in Python, and the case tables built on them.

TEST INFRASTRUCTURE ONLY: pure Python + NumPy, no GPU, no package import.

``dispatch`` restates, for throughput mode (Philox bits and noise, no received-symbol tap), what
``csrc/ofdm_kernels_inst.hpp`` picks: ``tx_one`` / ``tx_fast`` / ``rx_one`` / ``rx_eq`` with
``fixed_fast``, ``adaptive_fast``, ``philox_streams`` and ``kFastMinLogN``, and the plan flags they read as
``csrc/ofdm_abi.hip`` sets them (``separable``, ``upat``, ``psk_m``, ``zpad = zero padding and
cp > 0``, ``zero_tie = MMSE and an exact zero in H``).  It returns the pair

    ("k_tx", R, LOGN, FB, LT, ZPW), ("k_rx", R, LOGN, EQ, FB, MV)

with R "float" | "double" and EQ -1 (run time: the generic kernel) | 0 NONE | 1 ZF | 2 MMSE --
the leading template arguments of the kernel a profiler trace names.  The LDS fallback of
``tx_launch`` / ``rx_launch`` (``kLdsPerCu``) is not restated in general -- no case below comes
near it -- with the one exception the trace showed: it holds for every cp (``lds_fallback_tx``).
tests/test_dispatch_model.py holds the names a GPU trace recorded against this model.

``reachable`` enumerates every instantiation the rules can pick for log2 N 6..12;
``matrix_cases`` is one oracle-checked case per instantiation (tests/test_gpu_dispatch_matrix.py),
``geometry_cases`` the prefix / tap geometry of the window FIR and the zero-padding receiver,
``generic_cases`` the generic kernel's throughput row.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

F32, F64 = "f32", "f64"
R_NAME = {F32: "float", F64: "double"}
EQ_CODE = {"NONE": 0, "ZF": 1, "MMSE": 2}
EQS = ("NONE", "ZF", "MMSE")
FAST_MIN_LOGN = 6            # kFastMinLogN
FB_CASES = (2, 3, 4, 5, 6, 8)  # OFDM_FB_CASES
FBS = (1,) + FB_CASES        # with the adaptive throughput kernels (FB = 1)
LOGNS = tuple(range(6, 13))
MAX_TAPS = 32


def tps(N: int) -> int:
    """Lanes per symbol: E = min(16, N) elements per lane."""
    return N // min(16, N)


def symbols(N: int) -> int:
    """Symbols of every case: with 32-symbol groups on a small multipath launch and 256 threads
    that is at least two workgroups, a partial last workgroup and a ragged last group, for every
    transmitter and receiver (67 symbols at N = 4096, 2083 at N = 64)."""
    return 32 * 4096 // N + 35


@dataclass(frozen=True)
class Plan:
    """A throughput-mode plan.  bits: bits per subcarrier of a fixed constellation, 0 = adaptive
    loading (orders: the per-subcarrier orders, 0 = unused)."""
    prec: str
    N: int
    bits: int
    scheme: str = "QAM"       # "QAM" | "PSK"
    L: int = 1
    cp: int = 0
    prefix: str = "CP"        # "CP" | "ZP"
    modulator: str = "OFDM"   # "OFDM" | "SC"
    eq: str = "NONE"
    orders: Optional[tuple] = None
    # the channel response is exactly zero on some subcarrier (RxArgs::zero_tie with MMSE): the
    # receiver decides that subcarrier's exact zeros by the first-index rule, in the generic kernel
    null_bin: bool = False


def _separable(bits: int, scheme: str) -> bool:
    # build_axis: the reference's square-QAM LUTs; PSK levels never form a side x side grid
    return scheme == "QAM" and bits % 2 == 0


def _fb(p: Plan) -> int:
    """The FB both launchers specialise on; 0 = the generic kernel."""
    logn = p.N.bit_length() - 1
    if logn < FAST_MIN_LOGN:
        return 0
    zpad = p.prefix == "ZP" and p.cp > 0
    if p.bits == 0:
        used = sorted({int(o) for o in p.orders if o > 0})
        sep = all(_separable(o.bit_length() - 1, p.scheme) for o in used)
        # universal_patterns: at most 4 LUTs of side <= 16, the reference's level patterns
        upat = sep and 1 <= len(used) <= 4 and all(o <= 256 for o in used)
        return 1 if upat and p.modulator == "OFDM" and not zpad else 0  # adaptive_fast
    nn = not _separable(p.bits, p.scheme)
    psk_m = (1 << p.bits) if p.scheme == "PSK" and (1 << p.bits) <= 32 else 0  # psk_order
    fixed_fast = (not nn or psk_m > 0) and (p.bits % 2 == 0 or psk_m > 0)
    return p.bits if fixed_fast and p.bits in FB_CASES else 0


def lds_fallback_tx(prec: str, logn: int, fb: int, lt: int) -> bool:
    """The one LDS fallback that does not depend on the plan's cp or taps: the complex128 adaptive
    flat transmitter at N >= 1024.  At its 1024 threads (OFDM_F64_TX_BLOCK) the rows of reals, the
    per-pass twiddles and the per-subcarrier table take 156672 .. 164832 bytes of dynamic LDS and
    the adaptive LUT pool 8216 bytes of static LDS -- 164888 bytes at the least (N = 2048), above
    kLdsPerCu = 163840 -- so tx_launch always hands these plans to the generic kernel and
    k_tx<double, 10 | 11 | 12, 1, 0> never runs (N = 512: 159128 bytes, it fits)."""
    return prec == F64 and fb == 1 and lt == 0 and logn >= 10


def dispatch(p: Plan):
    if p.N < 1 or p.N & (p.N - 1) or p.N > 4096 or not 1 <= p.L <= MAX_TAPS or not 0 <= p.cp <= p.N:
        raise ValueError(f"not a plan: {p}")
    logn = p.N.bit_length() - 1
    R = R_NAME[p.prec]
    zpad = p.prefix == "ZP" and p.cp > 0
    fb = _fb(p)
    if fb == 0:
        return ("k_tx", R, logn, 0, -1, False), ("k_rx", R, logn, -1, 0, True)
    # tx_fast
    lt, zpw = -1, False
    if p.L == 1 and not zpad:
        lt = 0
    elif logn >= 8 and p.cp <= tps(p.N) and (not zpad or p.prec == F64) and p.L <= 8:
        lt, zpw = (4 if p.L <= 4 else 8), zpad
    tx = ("k_tx", R, logn, 0, -1, False) if lds_fallback_tx(p.prec, logn, fb, lt) else ("k_tx", R, logn, fb, lt, zpw)
    # rx_one / rx_eq: complex64 compiles the modem variants into every receiver, complex128 keeps
    # them in kernels of their own; the adaptive receiver is rx_eq's default (MV)
    mv = True if (p.prec == F32 or fb == 1) else (p.modulator == "SC" or zpad)
    if p.null_bin and p.eq == "MMSE":  # philox_streams: zero_tie keeps the receiver off the throughput forms
        return tx, ("k_rx", R, logn, -1, 0, True)
    return tx, ("k_rx", R, logn, EQ_CODE[p.eq], fb, mv)


def reachable(logns=LOGNS, fbs=FBS):
    """Every (k_tx, ...) and (k_rx, ...) instantiation the rules can pick for these sizes."""
    tx, rx = set(), set()
    for prec in (F32, F64):
        R = R_NAME[prec]
        for logn in logns:
            for fb in fbs:
                lts = [(0, False), (-1, False)]
                if logn >= 8:
                    lts += [(4, False), (8, False)]
                    if prec == F64 and fb != 1:  # (adaptive_fast: no zero padding)
                        lts += [(4, True), (8, True)]
                tx |= {("k_tx", R, logn, fb, lt, z) for lt, z in lts if not lds_fallback_tx(prec, logn, fb, lt)}
                mvs = [True] if prec == F32 or fb == 1 else [False, True]
                rx |= {("k_rx", R, logn, e, fb, mv) for e in (0, 1, 2) for mv in mvs}
    return tx, rx


# --------------------------------------------------------------------------- channels, SNRs

def synthetic_channel(L: int, N: int) -> np.ndarray:
    """Deterministic L-tap channel of a case.  L = 1: one complex tap of magnitude 1.  Otherwise the
    first tap is 1 and taps 1 .. L-1 are complex Gaussian draws (generator seeded by (L, N)) weighted
    by exp(-l / 4) and scaled so their magnitudes sum to 0.6: |H| >= 0.4 on every subcarrier, so no
    equaliser gain inflates the decision bracket."""
    rng = np.random.default_rng([L, N])
    g = rng.standard_normal(max(L, 2) - 1) + 1j * rng.standard_normal(max(L, 2) - 1)
    if L == 1:
        return np.array([g[0] / abs(g[0])], np.complex128)
    t = g * np.exp(-np.arange(1, L) / 4.0)
    t *= 0.6 / np.sum(np.abs(t))
    return np.concatenate([[1.0 + 0j], t]).astype(np.complex128)


# Es/N0 in dB at which the oracle counts errors at a BER around 1e-2 over these channels
# (equalised; |H| down to 0.4 costs the weakest subcarriers 8 dB).  The densest constellations sit at
# the upper end of that: the complex64 rigorous bracket (philox_streams.z_error_bound: every point
# gets the whole transform's 2-norm bound) does not depend on the error count, so its width stays
# under the parity file's 10 % of the count only while the count is large enough -- at 27 dB
# (256-QAM, N = 4096, MMSE) and 43 dB (256-PSK) it came to 9 % and 10.4 %.
# tests/test_dispatch_model.py checks every complex64 case's width on the CPU.
SNR_DB = {("QAM", 2): 8.0, ("QAM", 4): 15.0, ("QAM", 6): 21.0, ("QAM", 8): 25.0,
          ("PSK", 1): 5.0, ("PSK", 2): 8.0, ("PSK", 3): 13.0, ("PSK", 4): 19.0, ("PSK", 5): 25.0,
          ("PSK", 6): 31.0, ("PSK", 8): 40.0}
# adaptive loading (SNR dB, SER target): a mix of 4-, 16- and 64-QAM over a multipath channel; a flat
# one loads every subcarrier alike, with the order's whole rounding margin to spare at 18 dB
ADAPTIVE_POINT = {False: (18.0, 0.04), True: (20.0, 0.02)}  # by "the channel is flat"


@dataclass(frozen=True)
class Case:
    plan: Plan
    snr: float
    tag: str = ""
    ser: float = 0.0          # adaptive loading: the SER target

    @property
    def S(self) -> int:
        return symbols(self.plan.N)

    @property
    def h(self) -> np.ndarray:
        return synthetic_channel(self.plan.L, self.plan.N)

    @property
    def M(self) -> int:
        return 1 << self.plan.bits if self.plan.bits else 0

    @property
    def id(self) -> str:
        p = self.plan
        c = "adaptive" if p.bits == 0 else f"{p.scheme}{1 << p.bits}"
        v = ("-SC" if p.modulator == "SC" else "") + ("-ZP" if p.prefix == "ZP" else "")
        prec = "" if self.tag == "geo-" else f"-{p.prec}"  # (geometry cases run both precisions)
        return f"{self.tag}N{p.N}-{c}-L{p.L}-cp{p.cp}-{p.eq}{prec}{v}"

    def variant(self) -> dict:
        """The keyword arguments of philox_streams.run_philox (and of the parity file's setup)."""
        p = self.plan
        v = {"cp": p.cp}
        if p.modulator == "SC":
            v["modulator"] = "SC"
        if p.prefix == "ZP":
            v["prefix"] = "ZP"
        if p.scheme == "PSK":
            v["scheme"] = "PSK"
        if p.bits == 0:
            v["adaptive"] = True
            v["ser"] = self.ser
        return v


def philox_kwargs(c: Case) -> dict:
    """The variant as philox_streams.run_philox takes it when called directly (no engine setup)."""
    p = c.plan
    kw = {"modulator": p.modulator, "prefix": p.prefix, "scheme": p.scheme}
    if p.bits == 0:
        kw["orders"] = np.asarray(p.orders, np.int64)
    return kw


def with_orders(p: Plan, snr: float, ser: float) -> Plan:
    """The plan with its adaptive orders filled in (ofdm_oracle.adaptive_orders, as the GPU tests'
    setup computes them)."""
    import ofdm_oracle as O

    if p.bits != 0:
        return p
    orders, _, _ = O.adaptive_orders(p.N, synthetic_channel(p.L, p.N), snr, ser, True, p.scheme)
    return Plan(p.prec, p.N, 0, p.scheme, p.L, p.cp, p.prefix, p.modulator, p.eq, tuple(int(o) for o in orders))


# --------------------------------------------------------------------------- part 2: the matrix

# the constellations that reach each FB; where two do (4 / 16 points) the cases alternate
CONSTELLATIONS = {1: [("QAM", 0)], 2: [("QAM", 2), ("PSK", 2)], 3: [("PSK", 3)], 4: [("QAM", 4), ("PSK", 4)],
                  5: [("PSK", 5)], 6: [("QAM", 6)], 8: [("QAM", 8)]}
LT_TAPS = {4: (2, 3, 4), 8: (5, 6, 7, 8)}
RT_TAPS = (9, 12, 32, 0)       # LT = -1 at N >= 256: a long channel, or (0) cp = TPS + 1 with L <= 8
SMALL_TAPS = (2, 3, 5, 8, 9, 12, 32)  # N < 256: every multipath channel takes the run-time FIR
MV_VARIANTS = (("SC", "CP"), ("OFDM", "ZP"), ("SC", "ZP"))


def _cp_choices(L: int, N: int):
    return (L - 1, 8, 9, tps(N))


def matrix_cases():
    """One case per reachable instantiation: per (precision, log2 N, FB) the transmitters (LT, ZPW)
    are paired with the receivers (EQ, MV) they can share a plan with.  r, a counter over the
    group's position, rotates the run-time dimensions: the equaliser paired with each FIR, the
    tap count within the LT class, cp within what the class allows, SC-OFDM, and which of SC / ZP /
    SC + ZP an MV receiver runs."""
    out = []
    for pi, prec in enumerate((F32, F64)):
        for li, logn in enumerate(LOGNS):
            N = 1 << logn
            T = tps(N)
            for fi, fb in enumerate(FBS):
                win = logn >= 8
                split = prec == F64 and fb != 1   # complex128: MV receivers are kernels of their own
                # (TX, MV receiver?) slots; a slot is (lt, zpw)
                plain = [(0, False), (4, False), (8, False)] if win else [(0, False), (-1, False), (-1, False)]
                slots = [(s, False) for s in plain]
                if split:
                    slots += [(s, True) for s in ([(4, True), (8, True), (-1, False)] if win else plain)]
                elif lds_fallback_tx(prec, logn, fb, 0):  # three receivers, three transmitters left
                    slots = [((lt, False), False) for lt in (4, 8, -1)]
                elif win:
                    slots.append(((-1, False), False))
                for si, ((lt, zpw), mv) in enumerate(slots):
                    r = li + fi + pi + si
                    eq = EQS[(si + li + fi) % 3]
                    scheme, bits = CONSTELLATIONS[fb][r % len(CONSTELLATIONS[fb])]
                    mod, prefix = "OFDM", "CP"
                    if fb != 1:
                        if mv:       # complex128 MV receiver: it must run SC, ZP or both
                            if zpw:
                                mod, prefix = MV_VARIANTS[1 + r % 2]
                            elif lt == -1:
                                mod, prefix = MV_VARIANTS[r % 3]
                            else:    # flat / window FIR without the guard: SC-OFDM
                                mod, prefix = MV_VARIANTS[0]
                        elif prec == F32:  # every complex64 receiver is MV: none, SC, ZP, SC + ZP
                            if lt == -1:
                                mod, prefix = ((("OFDM", "CP"),) + MV_VARIANTS)[r % 4]
                            else:    # (complex64 zero padding takes the run-time FIR)
                                mod = "SC" if r % 2 else "OFDM"
                    # taps and cp of the slot's FIR class
                    if lt == 0:
                        L, cp = 1, (0, 8, T, T + 1)[r % 4]
                    elif lt in (4, 8):
                        taps = LT_TAPS[lt] + ((1,) if zpw and lt == 4 else ())
                        L = taps[r % len(taps)]
                        cp = _cp_choices(L, N)[r % 4]
                        if prefix == "ZP":
                            cp = max(cp, 1)
                    elif win:
                        L = RT_TAPS[r % 4]
                        if L == 0:
                            L, cp = (2, 4, 7, 8)[(r // 4) % 4], T + 1
                        else:
                            cp = _cp_choices(L, N)[r % 4]
                    else:
                        L = SMALL_TAPS[r % len(SMALL_TAPS)]
                        cp = min(_cp_choices(L, N)[r % 4], N)
                    snr, ser = ADAPTIVE_POINT[L == 1] if bits == 0 else (SNR_DB[(scheme, bits)], 0.0)
                    p = with_orders(Plan(prec, N, bits, scheme, L, cp, prefix, mod, eq), snr, ser)
                    out.append(Case(p, snr, ser=ser))
    return out


# --------------------------------------------------------------------------- part 3: geometry

def geometry_cases():
    """Prefix and tap geometry of the window FIR (the A8 row alignment, the cp <= TPS hand-over to
    the run-time FIR) and of the zero-padding receiver (overlap-add, the tail noise samples each
    lane owns): 16-QAM, MMSE; the precision is looped inside the test (plan.prec is a placeholder)."""
    out = []

    def add(N, L, cps):
        for prefix in ("CP", "ZP"):
            for cp in sorted({c for c in cps if c >= (1 if prefix == "ZP" else 0)}):
                out.append(Case(Plan(F64, N, 4, "QAM", L, cp, prefix, "OFDM", "MMSE"), SNR_DB[("QAM", 4)], "geo-"))

    for N in (256, 1024):
        T = tps(N)
        for L in (2, 3, 4, 5, 6, 8, 9):
            add(N, L, [0, 1, L - 2, L - 1, 7, 8, 9, 15, 16, 17, T - 1, T, T + 1, 2 * (L - 1)])
    for N in (2048, 4096):
        T = tps(N)
        for L in (3, 8):
            add(N, L, [L - 1, T, T + 1])
    return out


# --------------------------------------------------------------------------- part 4: generic row

def generic_cases():
    """The generic kernel (FB = 0) in throughput mode: N < 64, and the constellations no throughput
    kernel takes -- BPSK (no FB = 1 slicer) and 64 / 256-PSK (nearest-point search)."""
    out = []
    for prec in (F32, F64):
        for N in (1, 2, 4, 8, 16, 32):
            out.append(Case(Plan(prec, N, 4, "QAM", 1, 0, "CP", "OFDM", "ZF"), SNR_DB[("QAM", 4)], "gen-"))
            if N >= 2:
                out.append(Case(Plan(prec, N, 4, "QAM", 3, 2, "CP", "OFDM", "ZF"), SNR_DB[("QAM", 4)], "gen-"))
        for bits in (1, 6, 8):
            out.append(Case(Plan(prec, 256, bits, "PSK", 3, 2, "CP", "OFDM", "MMSE"), SNR_DB[("PSK", bits)], "gen-"))
    return out


def fallback_cases():
    """lds_fallback_tx as it runs: the generic transmitter feeding the adaptive throughput receiver."""
    snr, ser = ADAPTIVE_POINT[True]
    return [Case(with_orders(Plan(F64, N, 0, "QAM", 1, cp, "CP", "OFDM", eq), snr, ser), snr, "lds-", ser)
            for N, cp, eq in ((1024, 8, "ZF"), (2048, 0, "MMSE"), (4096, 257, "NONE"))]


def predicted_names(cases, precs=None):
    """The instantiations a run of these cases launches, as sets of tuples (TX, RX)."""
    tx, rx = set(), set()
    for c in cases:
        for prec in (precs or (c.plan.prec,)):
            p = c.plan
            t, r = dispatch(Plan(prec, p.N, p.bits, p.scheme, p.L, p.cp, p.prefix, p.modulator, p.eq, p.orders))
            tx.add(t)
            rx.add(r)
    return tx, rx


def kernel_name(inst) -> str:
    """'k_tx<double, 10, 6, 4, false>' -- the leading template arguments as a trace prints them."""
    return f"{inst[0]}<" + ", ".join(str(v).lower() if isinstance(v, bool) else str(v) for v in inst[1:]) + ">"

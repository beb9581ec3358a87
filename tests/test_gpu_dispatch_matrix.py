"""Every throughput-kernel instantiation, and the prefix / tap geometry, against the oracle.

The fused transmitter and receiver are templates on precision, log2 N, bits per subcarrier, FIR
kind, zero-padding guard, equaliser and modem variant: 393 k_tx and 420 k_rx instantiations are
reachable in throughput mode for N = 64 .. 4096 (tests/dispatch_model.py restates the launch rules
and enumerates them).  tests/test_gpu_philox_parity.py pins hand-picked configurations; here the
case table is generated from the model so that

* MATRIX runs each reachable instantiation at least once (457 cases: per precision, log2 N and FB
  the larger of its transmitters and receivers), rotating the run-time dimensions -- SC-OFDM, which
  of SC / ZP / SC + ZP an MV receiver runs, the tap count within the FIR class, cp within what the
  class allows -- over every log2 N and FB;
* GEOMETRY walks cp and the tap count across the window FIR's row alignment ((cp + 7) & ~7;
  complex64 (cp + 15) & ~15), its cp <= TPS hand-over to the run-time FIR, taps that pad the
  4- / 8-tap window, and the zero-padding receiver's overlap-add and per-lane tail noise, in both
  precisions;
* GENERIC runs the generic kernel's throughput row: N = 1 .. 32, BPSK, 64- and 256-PSK; three more
  cases run the one cp-independent LDS fallback (dispatch_model.lds_fallback_tx).

Channels are synthetic (dispatch_model.synthetic_channel), S = 32 * 4096 / N + 35 symbols gives
every kernel at least two workgroups, a partial last one and a ragged last symbol group.  The
checks and tolerances are the parity file's (check_tx_samples, check_error_counts); complex128
brackets are additionally held to width <= 2 (tests/test_dispatch_model.py shows, without a GPU,
that the oracle's own bracket of every complex128 case has width 0 and more than 100 errors).
profiles/dispatch_matrix_kernels.txt holds the kernel names a profiler recorded under this file.
"""

import numpy as np
import pytest
import torch

import dispatch_model as D
import test_gpu_philox_parity as PP
from ofdm_based_systems import _backend as B

pytestmark = pytest.mark.gpu

PREC = {D.F32: B.OFDM_F32, D.F64: B.OFDM_F64}
MATRIX = D.matrix_cases()
GEOMETRY = D.geometry_cases()
GENERIC = D.generic_cases()
BOTH = MATRIX + GENERIC + D.fallback_cases()


def _args(c, prec=None):
    p = c.plan
    return p.N, c.M, c.h, p.eq, c.S, c.snr, PREC[prec or p.prec], c.variant()


def _counts(c, prec=None):
    prec = prec or c.plan.prec
    res, ref = PP.check_error_counts(c.id if prec == c.plan.prec else f"{c.id}[{prec}]", *_args(c, prec))
    if prec == D.F64:  # the oracle holds the receivers' noise bit for bit: exact counts
        lo, hi, slo, shi = ref.bracket
        assert hi - lo <= 2 and shi - slo <= 2, ref.bracket


@pytest.mark.parametrize("case", BOTH, ids=[c.id for c in BOTH])
def test_tx_samples(gpu, case):
    PP.check_tx_samples(*_args(case))


@pytest.mark.parametrize("case", BOTH, ids=[c.id for c in BOTH])
def test_counts(gpu, case):
    _counts(case)


@pytest.mark.parametrize("N,L", [(1, 2), (2, 3), (4, 9), (16, 32), (64, 32)])
def test_plan_response_is_the_cropped_fft(gpu, N, L):
    """H of a plan is np.fft.fft(h, N), which crops a channel longer than N (the generic row's
    N = 2 / 3-tap case showed it aliased: taps l >= N were folded onto l mod N)."""
    h = D.synthetic_channel(L, N)
    plan = B.Plan(n_fft=N, h_raw=h)
    H = torch.empty(N, dtype=torch.complex128, device=B.device())
    B.check(B.lib().ofdm_plan_response(plan.handle, B.stream_ptr(), B.ptr(H), None))
    ref = np.fft.fft(h, N)
    # a direct L-term sum in double: a few roundings of 2^-53 per term
    assert np.max(np.abs(H.cpu().numpy() - ref)) <= 4 * L * 2.0 ** -53 * np.sum(np.abs(h))


@pytest.mark.parametrize("case", GEOMETRY, ids=[c.id for c in GEOMETRY])
def test_prefix_and_tap_geometry(gpu, case):
    """Both precisions against one oracle run of the transmitter; with zero padding also the counts
    (the receiver's overlap-add and the tail noise samples each lane owns depend on cp)."""
    ref = None
    for prec in (D.F64, D.F32):
        ref = PP.check_tx_samples(*_args(case, prec), ref=ref)
    if case.plan.prefix == "ZP":
        for prec in (D.F64, D.F32):
            _counts(case, prec)

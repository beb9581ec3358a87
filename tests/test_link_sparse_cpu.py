"""The fused link's sparse slicer without a GPU: the new entry point's declaration, export and binding,
the engine's routing of each attribute pair, eps and T restated against the kernel's source, the rule, and
a numpy model showing that no skipped quad holds anything the slicer would have had to see."""

import math
import os
import re
import types

import pytest

import link_nscreen_expect as NX
import link_sparse_expect as SX
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import LinkEngine
from test_abi import HEADER, declared_functions
from test_engine_schedule_cpu import make
from test_link_nscreen_cpu import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "ofdm-based-systems_amd", "csrc", "ofdm_link_inst.hpp")


def test_entry_point_is_declared_exported_and_bound():
    assert "ofdm_link_sparse" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_link_sparse("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert decl == ("int ofdm_link_sparse(ofdm_plan_t plan, void* stream, uint64_t seed, const ofdm_stats* stats, "
                    "int64_t total_samples, double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, "
                    "int64_t n_valid_bits, uint64_t* counters, int32_t mode, uint64_t* sparse_counts)")
    # ofdm_link's arguments, a mode and a pointer, as the two screens' entry points; the version stands
    assert B.SIGNATURES["ofdm_link_sparse"] == B.SIGNATURES["ofdm_link_nscreen"]
    assert B.SIGNATURES["ofdm_link_sparse"][1][:11] == B.SIGNATURES["ofdm_link"][1]
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    assert set(B.SIGNATURES) == set(declared_functions())
    assert hasattr(B.load_library(), "ofdm_link_sparse")


def test_null_plan_and_bad_mode_are_invalid_without_a_gpu():
    lib = B.load_library()
    assert lib.ofdm_link_sparse(None, None, 0, None, 0, 20.0, 1, 0, 4, 0, None, B.LINK_SCREEN_FORCED, None) == -1
    assert b"ofdm_link" in lib.ofdm_last_error()
    for mode in (3, 7, -1):
        assert lib.ofdm_link_sparse(None, None, 0, None, 0, 20.0, 1, 0, 4, 0, None, mode, None) == -1
        assert b"ofdm_link_sparse: mode %d" % mode in lib.ofdm_last_error()


def test_the_engine_routes_each_attribute_pair_to_its_entry_point():
    eng = make()  # the logging CPU double; LinkEngine.link itself is what is called below
    eng._lib, eng.plan = Recorder(), types.SimpleNamespace(handle=None)
    call = lambda: LinkEngine.link(eng, None, 1, None, 4096, 20.0, True, 0, 4, 4 * 6144, None)
    pairs = ("screen_mode", "screen_counts", "nscreen_mode", "nscreen_counts", "sparse_mode", "sparse_counts")
    assert all(getattr(eng, p) is None for p in pairs)
    call()
    eng.sparse_mode = B.LINK_SCREEN_FORCED
    call()
    eng.sparse_mode, eng.nscreen_mode = None, B.LINK_SCREEN_OFF
    call()
    assert eng._lib.calls == [("ofdm_link", 11, ()), ("ofdm_link_sparse", 13, (B.LINK_SCREEN_FORCED, None)),
                              ("ofdm_link_nscreen", 13, (B.LINK_SCREEN_OFF, None))]
    # more than one pair at once: an error, whichever halves are set, and nothing is called
    for one in pairs[:4]:
        for other in pairs[4:]:
            for p in pairs:
                setattr(eng, p, None)
            setattr(eng, one, 0)
            setattr(eng, other, 0)
            with pytest.raises(ValueError, match="ofdm_link_sparse"):
                call()
    assert len(eng._lib.calls) == 3


def test_eps_and_the_threshold_are_the_kernels_and_cover_their_derivation():
    src = open(KERNEL).read()
    body = re.search(r"constexpr double sparse_eps\(int side\) \{ return ([^;]+); \}", src).group(1)
    assert body == "(1.5 * side + 6.0) * kScreenU"
    assert float(re.search(r"constexpr double kSparseMaxPerQuad = ([^;]+);", src).group(1)) == SX.MAX_PER_QUAD
    assert "e0 = (float)(1.001 * (sparse_eps(SIDE) + rho));" in src and "const float T = (thr - e0) * inv_lvl;" in src
    for side in (2, 4, 8, 16):
        need = sum(SX.eps_terms(side).values())
        assert need == 1.5 * side + 1.5
        assert SX.eps(side) / SX.U - need == 4.5  # (second-order terms, the double evaluation of rho)
    # 64-QAM, N = 1024: the table points sit on their levels to a few u (the offset 1/2 is exact, the
    # multiplier and each point are rounded once: at most 2 u of 3.5 levels), far inside eps
    assert 0 <= SX.rho() <= 8 * SX.U < SX.eps()
    assert 0 < SX.e0() < 30 * SX.U
    # T sits just under half a level: at 24 dB delta is about 2.8e-5 of a level
    lvl = SX.slicer_constants()[0]
    assert abs(lvl - math.sqrt(42) / 2 / 32) < 1e-7
    sigma = math.sqrt(1 / 10 ** 2.4 / 2)
    delta = NX.delta_sym(math.sqrt(2 * 1024) * sigma, math.sqrt(98 / 42)) / (2 / math.sqrt(42)) + NX.SLICER_U * SX.U
    t = SX.threshold(delta) * lvl
    assert 0.4999 < t < 0.5 - delta - SX.eps()
    # nothing under 1/2, or a bound that is not finite: no quad is skipped (|component| >= 0 > T)
    assert SX.threshold(0.5) < 0 and SX.threshold(0.7) < 0 and SX.threshold(float("inf")) < 0
    assert not (0.0 <= SX.threshold(float("nan")))


def test_mu_and_the_rule():
    # the issue's figures at 24 dB: 0.278 components per quad index and wave, 0.24 of the quads sliced
    assert 0.27 < SX.mu(24.0) < 0.29
    assert 0.24 < SX.sliced_share(24.0) < 0.25
    assert SX.mu(30.0) < 1e-6 < SX.mu(26.0) < SX.mu(24.0) < SX.mu(23.0) < SX.mu(22.0) < SX.mu(21.0) < SX.mu(6.0) <= 512
    assert SX.sliced_share(21.0) > 0.999
    # the rule: on with the noise off and at the bench's point, off where every quad holds a candidate
    assert SX.sparse_rule(24.0, noise_on=False) and SX.sparse_rule(6.0, noise_on=False)
    assert SX.sparse_rule(30.0) and SX.sparse_rule(24.0) and not SX.sparse_rule(21.0) and not SX.sparse_rule(6.0)
    # the measured crossing of forced against the noise screen (profiles/link_sparse_ab.txt)
    assert SX.mu(23.0) < SX.MAX_PER_QUAD < SX.mu(22.0)


# 30 dB: every quad skipped; 24: three in four; 21: hardly one; 10: none -- and none of them wrongly
@pytest.mark.parametrize("snr_db,symbols,lo,hi", [(30.0, 100, 0.999, 1.0), (24.0, 400, 0.70, 0.82),
                                                  (21.0, 200, 0.0, 0.01), (10.0, 100, 0.0, 0.0)])
def test_the_numpy_model_skips_no_quad_the_slicer_had_to_see(snr_db, symbols, lo, hi):
    quads, skipped, bad = SX.model(snr_db, symbols)
    print(f"{snr_db} dB: {quads} quads, skipped {skipped} ({skipped / quads:.4f}; the rule's share "
          f"{1 - SX.sliced_share(snr_db):.4f}), skipped with a wrong level or a margin failure {bad}")
    assert bad == 0
    assert lo <= skipped / quads <= hi
    if snr_db == 24.0:  # the model's own figure for the GPU test's range: 0.243 sliced, deviation 0.011 over 1600
        assert abs((1 - skipped / quads) - SX.sliced_share(24.0)) < 0.04

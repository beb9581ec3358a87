"""The fused link's float32 screen without a GPU: the new entry point's declaration, export and binding,
the screened kernel's LDS budget, and the bound delta restated and held against the recorded margin."""

import ctypes
import json
import math
import os
import re

import link_screen_expect as X
from ofdm_based_systems import _backend as B
from test_abi import HEADER, declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "ofdm-based-systems_amd", "csrc", "ofdm_link_inst.hpp")


def test_entry_point_is_declared_exported_and_bound():
    assert "ofdm_link_screen" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_link_screen("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert decl == ("int ofdm_link_screen(ofdm_plan_t plan, void* stream, uint64_t seed, const ofdm_stats* stats, "
                    "int64_t total_samples, double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, "
                    "int64_t n_valid_bits, uint64_t* counters, int32_t mode, uint64_t* screen_counts)")
    # ofdm_link's arguments, then the mode and the counts; an added entry point: the version stands
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    res, args = B.SIGNATURES["ofdm_link"]
    assert B.SIGNATURES["ofdm_link_screen"] == (res, args + [i32, vp])
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    for name, value in (("AUTO", B.LINK_SCREEN_AUTO), ("OFF", B.LINK_SCREEN_OFF), ("FORCED", B.LINK_SCREEN_FORCED)):
        assert int(re.search(rf"#define OFDM_LINK_SCREEN_{name} (\d+)", text).group(1)) == value
    assert sorted((B.LINK_SCREEN_AUTO, B.LINK_SCREEN_OFF, B.LINK_SCREEN_FORCED)) == [0, 1, 2]
    lib = B.load_library()
    assert hasattr(lib, "ofdm_link_screen")


def test_null_plan_and_bad_mode_are_invalid_without_a_gpu():
    lib = B.load_library()
    assert lib.ofdm_link_screen(None, None, 0, None, 0, 20.0, 1, 0, 4, 0, None, B.LINK_SCREEN_FORCED, None) == -1
    assert b"ofdm_link" in lib.ofdm_last_error()
    assert lib.ofdm_link_screen(None, None, 0, None, 0, 20.0, 1, 0, 4, 0, None, 7, None) == -1
    assert b"mode 7" in lib.ofdm_last_error()


def test_the_screened_workgroup_still_holds_12_symbols():
    """link_carve with SCREEN: the float32 twiddles [forward | inverse] (16 128 B) and the float32 LUT
    (512 B) beside what the unscreened kernel holds; one workgroup of 768 threads per CU either way."""
    assert X.lds_bytes(12, screen=False) == 139872
    assert X.lds_bytes(12, screen=True) == 139872 + 16128 + 512 == 156512 <= 160 * 1024
    assert X.lds_bytes(13, screen=True) > 160 * 1024
    # a row of PADN complex64 is the row of PADN reals the complex128 exchange uses
    assert (1024 + 64) * 8 == (1024 + 64) * 2 * 4


def test_the_bound_is_the_kernels_and_covers_its_derivation():
    src = open(KERNEL).read()
    const = lambda name: re.search(rf"constexpr double {name} = ([^;]+);", src).group(1)
    assert float(const("kScreenK")) == X.K
    assert const("kScreenU") == "0x1p-24" and X.U == 2.0 ** -24
    assert float(const("kScreenSlicerU")) == X.SLICER_U
    assert float(const("kScreenMaxUndecided")) == X.MAX_UNDECIDED
    # Higham 24.2 for ten radix-2 levels with once-rounded twiddles, plus the LUT's / the noise FMA's u
    assert 6.65 < X.higham_eta() / X.U < 6.66
    assert 67.5 < X.k_derived() < 67.7 < X.K
    # the slicer's roundings: (0.6 + 0.5 + 1) u of the clamped coordinate times side - 1 <= 15, and the margin's
    assert 2.1 * 15 + 0.5 < X.SLICER_U
    # delta_sym: K u (||z32||_2 + sqrt N amax), e.g. a unit-power symbol of 64-QAM at N = 1024
    amax = math.sqrt(98 / 42)
    d = X.delta_sym(32.0, 1024, amax)
    assert d == 70 * 2.0 ** -24 * (32.0 + 32.0 * amax)
    # in levels (step 2 / sqrt 42) about 1e-3: a few symbols in a hundred undecided at 24 dB
    assert 0.9e-3 < d / (2 / math.sqrt(42)) < 1.2e-3
    assert 0.04 < X.undecided(24.0) < 0.07
    # the automatic rule: on from about 22 dB up
    assert X.undecided(21.0) > X.undecided(22.0) > X.MAX_UNDECIDED > X.undecided(23.0) > X.undecided(30.0)


def test_the_recorded_margin_is_inside_a_quarter_of_the_bound():
    rec = json.load(open(os.path.join(ROOT, "profiles", "link_screen_margin.json")))
    assert rec["K"] == X.K
    assert {p["snr_db"] for p in rec["points"]} == {24.0, 10.0}
    for p in rec["points"]:
        assert 0 < p["max_abs_err"] <= p["max_ratio"] * p["max_delta_sym"]
        assert p["max_ratio"] <= 0.25
        # the recorded bounds are delta_sym's of 64-QAM symbols at N = 1024: norms within a few sigma of sqrt(N (1 + 1/snr))
        amax = math.sqrt(98 / 42)
        lo = X.delta_sym(0.8 * 32.0, 1024, amax)
        hi = X.delta_sym(1.2 * 32.0 * math.sqrt(1 + 10 ** (-p["snr_db"] / 10)), 1024, amax)
        assert lo < p["min_delta_sym"] <= p["max_delta_sym"] < hi

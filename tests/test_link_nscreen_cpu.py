"""The fused link's noise screen without a GPU: the new entry point's declaration, export and binding,
the engine's routing of each attribute pair, the noise-screen kernel's LDS budget, the bound restated
and held against the recorded margin, and a numpy model of the screen."""

import ctypes
import json
import math
import os
import re
import types

import pytest

import link_nscreen_expect as NX
import link_screen_expect as X
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import LinkEngine
from test_abi import HEADER, declared_functions
from test_engine_schedule_cpu import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "ofdm-based-systems_amd", "csrc", "ofdm_link_inst.hpp")


def test_entry_point_is_declared_exported_and_bound():
    assert "ofdm_link_nscreen" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_link_nscreen("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert decl == ("int ofdm_link_nscreen(ofdm_plan_t plan, void* stream, uint64_t seed, const ofdm_stats* stats, "
                    "int64_t total_samples, double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, "
                    "int64_t n_valid_bits, uint64_t* counters, int32_t mode, uint64_t* screen_counts)")
    # exactly ofdm_link_screen's signature; an added entry point: the version stands
    assert B.SIGNATURES["ofdm_link_nscreen"] == B.SIGNATURES["ofdm_link_screen"]
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    assert set(B.SIGNATURES) == set(declared_functions())
    assert hasattr(B.load_library(), "ofdm_link_nscreen")


def test_null_plan_and_bad_mode_are_invalid_without_a_gpu():
    lib = B.load_library()
    assert lib.ofdm_link_nscreen(None, None, 0, None, 0, 20.0, 1, 0, 4, 0, None, B.LINK_SCREEN_FORCED, None) == -1
    assert b"ofdm_link" in lib.ofdm_last_error()
    for mode in (3, 7, -1):
        assert lib.ofdm_link_nscreen(None, None, 0, None, 0, 20.0, 1, 0, 4, 0, None, mode, None) == -1
        assert b"ofdm_link_nscreen: mode %d" % mode in lib.ofdm_last_error()


class Recorder:
    """Stands for the library under LinkEngine.link: notes the entry point and its trailing arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name, len(a), a[11:])) or 0


def test_the_engine_routes_each_attribute_pair_to_its_entry_point():
    eng = make()  # the logging CPU double; LinkEngine.link itself is what is called below
    eng._lib, eng.plan = Recorder(), types.SimpleNamespace(handle=None)
    call = lambda: LinkEngine.link(eng, None, 1, None, 4096, 20.0, True, 0, 4, 4 * 6144, None)
    assert (eng.screen_mode, eng.screen_counts, eng.nscreen_mode, eng.nscreen_counts) == (None,) * 4
    call()
    eng.screen_mode = B.LINK_SCREEN_FORCED
    call()
    eng.screen_mode, eng.nscreen_mode = None, B.LINK_SCREEN_OFF
    call()
    assert eng._lib.calls == [("ofdm_link", 11, ()), ("ofdm_link_screen", 13, (B.LINK_SCREEN_FORCED, None)),
                              ("ofdm_link_nscreen", 13, (B.LINK_SCREEN_OFF, None))]
    # both pairs at once: an error, whichever halves are set, and nothing is called
    for two, noise in (("screen_mode", "nscreen_mode"), ("screen_counts", "nscreen_mode"),
                       ("screen_mode", "nscreen_counts"), ("screen_counts", "nscreen_counts")):
        eng.screen_mode = eng.screen_counts = eng.nscreen_mode = eng.nscreen_counts = None
        setattr(eng, two, 0)
        setattr(eng, noise, 0)
        with pytest.raises(ValueError, match="ofdm_link_nscreen"):
            call()
    assert len(eng._lib.calls) == 3


def test_the_noise_screen_workgroup_holds_12_symbols():
    """link_carve for the noise screen: the forward float32 twiddles (8 064 B) and the float32 LUT times N
    (512 B) beside what the unscreened kernel holds; one workgroup of 768 threads per CU."""
    assert NX.lds_bytes(12) == 139872 + 8064 + 512 == 148448 <= 160 * 1024
    assert NX.lds_bytes(13) < 160 * 1024 < NX.lds_bytes(14)  # (12: whole waves of a 768-thread workgroup)
    assert NX.lds_bytes(12) < X.lds_bytes(12, screen=True)


def test_the_bound_is_the_kernels_and_covers_its_derivation():
    src = open(KERNEL).read()
    const = lambda name: re.search(rf"constexpr double {name} = ([^;]+);", src).group(1)
    assert float(const("kNScreenK")) == NX.K_N
    assert float(const("kNScreenC")) == NX.C_LUT
    assert float(const("kNScreenMaxUndecided")) == NX.MAX_UNDECIDED
    # the two-transform screen's constants stand
    assert (float(const("kScreenK")), const("kScreenU"), float(const("kScreenSlicerU")),
            float(const("kScreenMaxUndecided"))) == (X.K, "0x1p-24", X.SLICER_U, X.MAX_UNDECIDED)
    # K_N: one transform (Higham 24.2), the noise product's u, the final add's |ghat_k| u
    assert 68.5 < NX.k_derived() < 68.7 and NX.k_derived() == X.k_derived() + 1
    assert 67.6 + 1 + 1 < NX.K_N  # (a whole u above what the derivation needs, and then some)
    assert NX.K_N - NX.k_derived() > 2  # (second-order terms, the float32 norm and bound: a few u)
    # C: the LUT's rounding, the final add's u N a, the float64 side (1e-3 u N a at most)
    assert 2 < NX.c_derived() < 2 + 1e-3 < NX.C_LUT
    # at unit power, 64-QAM, N = 1024: delta over the two-transform screen's, as sqrt(1 / (2 snr))
    amax = math.sqrt(98 / 42)
    for snr_db, lo, hi in ((24.0, 0.02, 0.035), (10.0, 0.1, 0.15)):
        sigma = math.sqrt(1 / 10 ** (snr_db / 10) / 2)
        new = NX.delta_sym(math.sqrt(2 * 1024) * sigma, amax)
        old = X.delta_sym(math.sqrt(1024 * (1 + 2 * sigma * sigma)), 1024, amax)
        assert lo < new / old < hi
    # the automatic rule: on at the bench's point and far below the two-transform screen's 22 dB
    assert NX.undecided(30.0) < NX.undecided(24.0) < 0.01 < NX.undecided(10.0) < NX.MAX_UNDECIDED
    # the measured crossing of forced against off lies between 8 and 6 dB (profiles/link_nscreen_ab.txt)
    assert NX.undecided(8.0) < NX.MAX_UNDECIDED < NX.undecided(6.0)
    assert NX.undecided(24.0) < X.undecided(24.0) / 10


def test_the_recorded_margin_is_inside_a_quarter_of_the_bound():
    rec = json.load(open(os.path.join(ROOT, "profiles", "link_nscreen_margin.json")))
    assert rec["K_N"] == NX.K_N and rec["C"] == NX.C_LUT
    assert [p["snr_db"] for p in rec["points"]] == [-20.0]
    for p in rec["points"]:
        assert 0 < p["max_abs_err"] <= p["max_ratio"] * p["max_delta_sym"]
        assert p["max_ratio"] <= 0.25
        # delta_sym's of symbols that are almost only noise: norms within a few sigma of sqrt(N (1 + 1/snr))
        n = 32.0 * math.sqrt(1 + 10 ** (-p["snr_db"] / 10))
        amax = math.sqrt(98 / 42)
        assert NX.delta_sym(0.8 * n, amax) < p["min_delta_sym"] <= p["max_delta_sym"] < NX.delta_sym(1.2 * n, amax)


# 24 dB: the model redoes about 0.3 % of the symbols, so "more than none" needs over a thousand of them
# (1500: five expected); 10 dB: about 40 %
@pytest.mark.parametrize("snr_db,symbols,lo,hi", [(24.0, 1500, 0.0, 0.02), (10.0, 300, 0.2, 0.65)])
def test_the_numpy_screen_keeps_no_symbol_whose_float64_decision_differs(snr_db, symbols, lo, hi):
    kept, wrong_kept = NX.model(snr_db, symbols)
    redone = 1 - kept.mean()
    print(f"{snr_db} dB: {symbols} symbols, redone {redone:.4f}, kept with a wrong level {wrong_kept}")
    assert wrong_kept == 0
    assert lo < redone < hi

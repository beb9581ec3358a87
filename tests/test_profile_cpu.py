"""The per-subcarrier profile (ofdm_rx_profile, LinkEngine.run(profile=True)) without a GPU: the
expectation helper against the pinned totals of the stage fixtures, the limb-combining function,
the ABI boundary of the new entry point, and the inputs of the throughput cases that
tests/test_gpu_profile.py runs (decision brackets of width 0 and the listed counts, so a GPU count
that differs is the kernel's doing)."""

import ctypes
import random
import re

import numpy as np
import pytest
from conftest import load_stages, stage_arrays

import philox_streams as P
import profile_expect as PE
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E


@pytest.mark.parametrize("st", load_stages(), ids=lambda s: s["name"])
def test_expected_rows_sum_to_the_pinned_totals(st):
    a = stage_arrays(st["name"])
    N, S = st["N"], st["S"]
    b = int(np.log2(st["M"]))
    bk = np.full(N, b, np.int64)
    idx = PE.tx_indices(a["tx_bytes"], bk, S)
    rows = PE.expected_rows(a["Z"], idx, bk, S * N * b)
    assert int(rows["bit_errors"].sum()) == st["bit_errors"]
    assert int(rows["symbol_errors"].sum()) == st["symbol_errors"]
    assert not rows["clipped"].any()
    assert np.all(rows["error_power"] > 0) and np.all(np.isfinite(rows["error_power"]))
    # an error is at least one bit, at most b
    assert np.all(rows["symbol_errors"] <= rows["bit_errors"]) and np.all(rows["bit_errors"] <= b * rows["symbol_errors"])


def test_expected_rows_mask_a_trailing_partial_byte_and_inactive_subcarriers():
    """Adaptive layout: 3 subcarriers of 2 / 0 / 4 bits, 2 symbols = 12 bits, 8 compared."""
    bk = np.array([2, 0, 4], np.int64)
    idx = np.array([[0, 0, 0], [0, 0, 0]], np.int64)
    import ofdm_oracle as O

    q4, q16 = O.qam_lut(4), O.qam_lut(16)
    # every subcarrier received as the point whose index has all bits set
    Z = np.array([[q4[3], 5.0, q16[15]], [q4[3], 5.0, q16[15]]])
    rows = PE.expected_rows(Z, idx, bk, 8)
    # symbol 0: bits 0-1 (k = 0) and 2-5 (k = 2); symbol 1: bits 6-7 (k = 0), 8-11 (k = 2) not compared
    assert rows["bit_errors"].tolist() == [4, 0, 4]
    assert rows["symbol_errors"].tolist() == [2, 0, 2]
    assert rows["error_power"][1] == 0 and rows["clipped"].tolist() == [0, 0, 0]


def test_expected_rows_clip():
    import ofdm_oracle as O

    bk = np.array([2, 2], np.int64)
    idx = np.zeros((3, 2), np.int64)
    c = O.qam_lut(4)[0]
    Z = np.array([[c, c + 2048.0], [c, complex(np.nan, 0.0)], [c + 0.5, complex(np.inf, 0.0)]])
    rows = PE.expected_rows(Z, idx, bk, 12)
    assert rows["clipped"].tolist() == [0, 3]
    assert rows["error_power"].tolist() == [0.25, 3 * 2.0 ** 20]


def test_combine_profile_is_the_exact_integer_sum():
    rng = random.Random(5)
    N, ranks = 37, 6
    parts = []
    for _ in range(ranks):
        rec = np.zeros((B.PROFILE_ROWS, N), np.int64)
        for k in range(N):
            rec[0, k] = rng.randrange(1 << 40)
            rec[1, k] = rng.randrange(1 << 40)
            rec[2, k] = rng.randrange(1 << 52)   # unnormalised low limbs, as the workgroups leave them
            rec[3, k] = rng.randrange(1 << 50)
            rec[4, k] = rng.randrange(1 << 30)
        parts.append(rec)
    got = E.combine_profile(parts)
    power = E.profile_power(got)
    for k in range(N):
        for r in (0, 1, 4):
            assert int(got[r, k]) == sum(int(p[r, k]) for p in parts)
        total = sum(int(p[2, k]) + (int(p[3, k]) << 32) for p in parts)   # units of 2^-40
        assert 0 <= int(got[2, k]) < 1 << 32
        assert int(got[2, k]) + (int(got[3, k]) << 32) == total
        assert power[k] == float(int(got[3, k])) * 2.0 ** -8 + float(int(got[2, k])) * 2.0 ** -40
    # any grouping of the records gives the same record
    again = E.combine_profile([E.combine_profile(parts[:2]), E.combine_profile(parts[2:])])
    assert np.array_equal(again, got)
    assert np.array_equal(PE.record_rows(got)["error_power"], power)


def test_profile_dataclass_rates():
    prof = E.SubcarrierProfile(bit_errors=np.array([4, 0, 0]), symbol_errors=np.array([2, 0, 0]),
                               clipped=np.zeros(3, np.int64), error_power=np.array([1.0, 0.0, 0.1]),
                               error_power_fx=np.zeros((2, 3), np.int64),
                               n_symbols=10, bits_per_subcarrier=np.array([2, 0, 4]))
    assert prof.ber[0] == 4 / 20 and np.isnan(prof.ber[1]) and prof.ber[2] == 0
    assert prof.ser[0] == 0.2 and np.isnan(prof.ser[1])
    assert prof.mer_db[0] == pytest.approx(10.0) and np.isnan(prof.mer_db[1]) and prof.mer_db[2] == pytest.approx(20.0)


def test_entry_point_is_declared_exported_and_bound():
    from test_abi import HEADER, declared_functions

    assert "ofdm_rx_profile" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_rx_profile("):]
    decl = decl[:decl.index(";")]
    assert "int64_t* profile" in decl
    # declared with the reference interface it stands in for
    at = text.index("int ofdm_rx_profile(")
    assert "simulation/models.py:596-618" in text[text.rindex("/*", 0, at):at]
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    lib = B.load_library()
    assert hasattr(lib, "ofdm_rx_profile") and "ofdm_rx_profile" in B.SIGNATURES
    # ofdm_rx's arguments and the record
    assert B.SIGNATURES["ofdm_rx_profile"][1] == B.SIGNATURES["ofdm_rx"][1] + [ctypes.c_void_p]
    assert set(B.SIGNATURES) == set(declared_functions())


def test_null_plan_is_invalid_without_a_gpu():
    lib = B.load_library()
    rec = (ctypes.c_int64 * 5)()
    cnt = (ctypes.c_uint64 * 2)()
    args = [None, None, None, None, None, 0, None, 0, 0.0, 0, None, 0, 0, 0, ctypes.cast(cnt, ctypes.c_void_p), None, 0]
    assert lib.ofdm_rx_profile(*args, ctypes.cast(rec, ctypes.c_void_p)) == -1
    assert "ofdm_rx_profile" in lib.ofdm_last_error().decode()
    with pytest.raises(ValueError):
        B.check(-1)
    assert lib.ofdm_rx_profile(*args, None) == -1
    assert "profile record" in lib.ofdm_last_error().decode()


@pytest.mark.parametrize("case", PE.THROUGHPUT_CASES, ids=lambda c: c["id"])
def test_throughput_cases_have_exact_brackets(case):
    S = PE.matrix_symbols(case["N"])
    assert S == case["S"]
    h, cp, orders = PE.case_channel(case)
    if orders is not None:
        assert [int(np.count_nonzero(orders == o)) for o in (0, 4, 16)] == [268, 1057, 723]
        assert set(np.unique(orders)) == {0, 4, 16}
    ref = P.run_philox(PE.SEED, S, case["N"], case["M"], h, cp, case["eq"], case["snr"], orders=orders,
                       precision="f64", radius_fn=PE.np_radius)
    lo, hi, slo, shi = ref.bracket
    assert (lo, hi, slo, shi) == (case["bit_errors"], case["bit_errors"], case["symbol_errors"], case["symbol_errors"])
    assert (ref.bit_errors, ref.symbol_errors) == (case["bit_errors"], case["symbol_errors"])

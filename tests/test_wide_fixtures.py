"""Host-side ground for constellations above 256 points (no GPU): the package's 1024/4096-QAM and
1024-PSK LUTs are the oracle's, the 1024-QAM stage fixture is built from them, the LUTs separate
into per-axis levels exactly (what the wide map and slicer tables rely on), and the wide reference
runs each pin something."""

import json
import os

import numpy as np
import pytest
from conftest import GOLDEN, stage_arrays

import ofdm_oracle as O
from ofdm_based_systems.constellation.models import PSKConstellationMapper, QAMConstellationMapper


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@pytest.mark.parametrize("m", [1024, 4096])
def test_wide_qam_lut_is_the_oracles_and_separable(m):
    lut = QAMConstellationMapper(m).constellation
    assert np.array_equal(lut, O.qam_lut(m))
    side, hb = int(np.sqrt(m)), int(np.log2(m)) // 2
    lev = np.unique(lut.real)
    assert len(lev) == side and np.array_equal(lev, np.unique(lut.imag))
    np.testing.assert_allclose(np.diff(lev), (lev[-1] - lev[0]) / (side - 1), rtol=1e-9)
    i = np.arange(m)
    ki, kq = np.searchsorted(lev, lut.real), np.searchsorted(lev, lut.imag)
    # one level per low / high half of the index, both ways: LUT[i] = lev[inv_i[lo]] + j lev[inv_q[hi]]
    inv_i, inv_q = np.full(side, -1), np.full(side, -1)
    inv_i[i & (side - 1)] = ki
    inv_q[i >> hb] = kq
    assert sorted(inv_i) == list(range(side)) and sorted(inv_q) == list(range(side))
    assert np.array_equal(lev[inv_i[i & (side - 1)]] + 1j * lev[inv_q[i >> hb]], lut)


def test_wide_psk_lut_is_the_oracles():
    assert np.array_equal(PSKConstellationMapper(1024).constellation, O.psk_lut(1024))


def test_stage_fixture_is_1024_qam_of_its_bytes():
    st = load("stages_wide.json")[0]
    a = stage_arrays(st["name"])
    assert (st["M"], st["N"]) == (1024, 64) and st["bit_errors"] >= 10
    idx = O.bits_to_indices(O.bytes_to_bits(a["tx_bytes"].tobytes()), 10)
    assert idx.max() > 255  # index bits above a byte are in play
    assert np.array_equal(O.qam_lut(1024)[idx].reshape(-1, 64), a["X"])
    assert O.indices_to_bytes(O.nn_demap(a["Z"].ravel(), O.qam_lut(1024)), 10) == a["rx_bytes"].tobytes()


def test_wide_runs_pin_something():
    runs = load("runs_wide.json")
    for c in runs:
        r = c["result"]
        assert 10 <= r["bit_errors"] < 0.1 * r["total_bits"], c["tag"]
    top = {c["tag"] + str(c["params"]["snr_db"]): max(c["result"]["constellation_order_per_subcarrier"]) for c in runs}
    assert top["wide_n64_adaptive_p135.0"] == 1024 and top["wide_n64_adaptive_p140.0"] == 4096
    assert top["wide_n2048_adaptive_p135.0"] == 1024 and top["wide_n4096_m4096_p1_mmse44.0"] == 4096

"""The constellation-density record (ofdm_rx_density, LinkEngine.run(density=G),
engine.ConstellationDensity) without a GPU: the entry point's declaration, export, binding and refusals,
the NumPy restatement (tests/density_expect.py) on small hand-made inputs, ConstellationDensity against
plain NumPy, the engine's schedule, buffer layout and refusals over the oracle's CPU test double (whose
rx bins the points it equalises), resident, batched, with a tap and under gloo, the Simulation /
settings keys and refusals -- and the precondition of the GPU comparisons against the stage fixtures:
none of their points is within the tolerance of a grid line, and none lies outside the square.

On the commit before the record test_entry_point_is_declared_exported_and_bound fails (no such entry
point), as does everything that passes ``density``."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from conftest import channel, load_stages, stage_arrays

import density_expect as DE
import ofdm_oracle as O
from ofdm_based_systems import _backend as B
from ofdm_based_systems import engine as E
from ofdm_based_systems.configuration.models import SimulationSettings
from ofdm_based_systems.simulation.models import Simulation
from test_distributed_cpu import CASE, _free_port
from test_sweep_cpu import SweepEngine

SEED = 21
RX_ARGS = 17  # ofdm_rx's


# ---------------------------------------------------------------- the ABI boundary
def test_entry_point_is_declared_exported_and_bound():
    from test_abi import HEADER, declared_functions

    assert "ofdm_rx_density" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_rx_density("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert "double lo, double inv_w, int32_t bins, int32_t k_lo, int32_t k_hi, uint64_t* hist" in decl
    at = text.index("int ofdm_rx_density(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "(c - lo) * inv_w" in comment and "never zeroed" in comment and "never" in comment and "FMA" in comment
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION == 6
    assert int(re.search(r"#define OFDM_MAX_DENSITY_BINS (\d+)", text).group(1)) == B.MAX_DENSITY_BINS == 128
    lib = B.load_library()
    assert hasattr(lib, "ofdm_rx_density") and "ofdm_rx_density" in B.SIGNATURES
    # ofdm_rx's arguments, then lo, inv_w, bins, k_lo, k_hi and the record
    assert B.SIGNATURES["ofdm_rx_density"][1] == B.SIGNATURES["ofdm_rx"][1] + [
        ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    assert len(B.SIGNATURES["ofdm_rx"][1]) == RX_ARGS
    assert set(B.SIGNATURES) == set(declared_functions())


def rx_args(sym0=0, n_sym=0, counters=True):
    cnt = (ctypes.c_uint64 * 2)()
    args = [None, None, None, None, None, 0, None, 0, 0.0, 0, None, sym0, n_sym, 0,
            ctypes.cast(cnt, ctypes.c_void_p) if counters else None, None, 0]
    assert len(args) == RX_ARGS
    return args, cnt


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("lo,inv_w,bins,k_lo,k_hi,record,reason", [
    (-2.0, 8.0, 32, 0, 64, False, "needs a density record"),
    (-2.0, 8.0, 0, 0, 64, True, "bins 0 is not in [1, 128]"),
    (-2.0, 8.0, -4, 0, 64, True, "bins -4 is not in [1, 128]"),
    (-2.0, 8.0, 129, 0, 64, True, "bins 129 is not in [1, 128]"),
    (NAN, 8.0, 32, 0, 64, True, "lo is not finite"),
    (-INF, 8.0, 32, 0, 64, True, "lo is not finite"),
    (-2.0, NAN, 32, 0, 64, True, "inv_w is not a finite positive"),
    (-2.0, INF, 32, 0, 64, True, "inv_w is not a finite positive"),
    (-2.0, 0.0, 32, 0, 64, True, "inv_w is not a finite positive"),
    (-2.0, -8.0, 32, 0, 64, True, "inv_w is not a finite positive"),
    (-2.0, 8.0, 32, -1, 64, True, "range [-1, 64) is not 0 <= k_lo < k_hi <= n_fft"),
    (-2.0, 8.0, 32, 5, 5, True, "range [5, 5) is not 0 <= k_lo < k_hi <= n_fft"),
    (-2.0, 8.0, 32, 6, 5, True, "range [6, 5) is not 0 <= k_lo < k_hi <= n_fft"),
    (-2.0, 8.0, 32, 0, 64, True, "needs a constellation"),      # the grid is fine: ofdm_rx's own refusal
    (-2.0, 8.0, 1, 0, 1, True, "needs a constellation"),
    (-2.0, 8.0, 128, 63, 64, True, "needs a constellation"),
])
def test_refusals_name_the_function_without_a_device(lo, inv_w, bins, k_lo, k_hi, record, reason):
    lib = B.load_library()
    args, _ = rx_args(0, 8)
    rec = (ctypes.c_uint64 * (max(bins, 1) ** 2 + 1))()
    rc = lib.ofdm_rx_density(*args, lo, inv_w, bins, k_lo, k_hi, ctypes.cast(rec, ctypes.c_void_p) if record else None)
    msg = lib.ofdm_last_error().decode()
    assert rc == -1 and "ofdm_rx_density" in msg and reason in msg, msg
    assert not any(rec)


def test_what_ofdm_rx_refuses_is_refused():
    lib = B.load_library()
    rec = (ctypes.c_uint64 * 17)()
    for kw in (dict(sym0=-1, n_sym=4), dict(n_sym=-1), dict(counters=False), dict(n_sym=0)):
        args, _ = rx_args(**kw)
        assert lib.ofdm_rx_density(*args, -2.0, 1.0, 4, 0, 1, ctypes.cast(rec, ctypes.c_void_p)) == -1
        assert "ofdm_rx_density" in lib.ofdm_last_error().decode()
        assert lib.ofdm_rx(*args) == -1


def test_kernel_sources_hold_the_section_and_its_exclusions():
    """k_rx_dens is the shared body with OFDM_RX_BODY_DENS, in translation units of its own, and the
    density's arguments are no field of RxArgs."""
    from conftest import ROOT

    src = os.path.join(ROOT, "ofdm-based-systems_amd", "csrc")
    body = open(os.path.join(src, "ofdm_rx_body.hpp")).read()
    assert "#ifdef OFDM_RX_BODY_DENS" in body
    assert "static_assert(DENS && !REF && !PROF && !SWEEP && !FRAMES" in body and "static_assert(!DENS" in body
    fused = open(os.path.join(src, "ofdm_fused.hpp")).read()
    at = fused.index("void k_rx_dens(")
    assert "#define OFDM_RX_BODY_DENS" in fused[at:at + 400] and "RxArgs a, RxDensTail dt" in fused[at:at + 100]
    launch = open(os.path.join(src, "ofdm_launch.hpp")).read()
    rxargs = launch[launch.index("struct RxArgs {"):]
    assert "hist" not in rxargs[:rxargs.index("};")] and "struct RxDensTail {" in launch
    mk = open(os.path.join(ROOT, "ofdm-based-systems_amd", "Makefile")).read()
    for unit in ("ofdm_kernels_f32_dens", "ofdm_kernels_f64_dens"):
        assert unit + ".o" in mk and os.path.exists(os.path.join(src, unit + ".hip"))


# ---------------------------------------------------------------- the restatement on hand-made points
def test_bin_points_index_edges_and_outside():
    G, L = 4, 2.0   # bins of width 1: [-2, -1), [-1, 0), [0, 1), [1, 2)
    Z = np.array([[-2.0 - 2.0j, -1.0 + 0.0j, 1.999 + 1.0j, 2.0 + 0.0j, 0.5 - 2.0000001j,
                   complex(np.nan, 0.0), complex(0.0, np.inf), -0.0 + 0.0j]])
    counts, outside = DE.bin_points(Z, G, L)
    want = np.zeros((4, 4), np.int64)
    want[0, 0] = 1      # the lower corner is inside
    want[2, 1] = 1      # (-1, 0): re bin 1, im bin 2 -- row = imaginary bin
    want[3, 3] = 1
    want[2, 2] = 1      # -0.0 + 0.0j
    assert np.array_equal(counts, want) and outside == 4   # re = 2.0, im just below -2, NaN, inf
    assert counts.sum() + outside == Z.size
    # the range and the active mask select columns
    c, o = DE.bin_points(Z, G, L, 1, 3)
    assert c.sum() == 2 and o == 0 and c[2, 1] == 1 and c[3, 3] == 1
    act = np.ones(8, bool)
    act[[3, 5]] = False
    c, o = DE.bin_points(Z, G, L, active=act)
    assert c.sum() == 4 and o == 2
    # complex64 is widened, exactly
    z32 = np.array([[0.1 + 0.7j, -1.3 - 0.2j]], np.complex64)
    assert np.array_equal(DE.bin_points(z32, 31, 2.0)[0], DE.bin_points(z32.astype(np.complex128), 31, 2.0)[0])
    # the index is (c - lo) * inv_w in two rounded operations: G = 31 has an inexact inv_w
    lo, inv_w = DE.grid(31, 2.0)
    assert (lo, inv_w) == (-2.0, 31 / 4.0) == E.density_grid(31, 2.0)
    c = 0.7096774193548387
    assert np.array_equal(DE.bin_points(np.array([[complex(c, c)]]), 31, 2.0)[0].nonzero(),
                          (np.array([int((c - lo) * inv_w)]),) * 2)


def test_undecided_and_bracket():
    G, L = 4, 2.0
    Z = np.array([[0.5 + 0.5j, 1.0 + 1e-7 + 0.5j, 0.5 - 1.0j + 1e-7j, 2.0 - 1e-7 + 0.5j, 3.5 + 0.5j, -2.0 + 1e-7 + 0.5j]])
    und = DE.undecided(Z, 1e-6, G, L)
    assert und.tolist() == [[False, True, True, True, False, True]]
    assert not DE.undecided(Z, 1e-9, G, L).any()
    dec, maybe = DE.bracket(Z, 1e-6, G, L)
    assert dec.sum() == 2 and dec[2 * 4 + 2] == 1 and dec[16] == 1        # 0.5 + 0.5j, and 3.5 is outside
    want = np.zeros(17, np.int64)
    want[[2 * 4 + 2, 2 * 4 + 3]] += 1      # re near 1: bins 2 | 3
    want[[0 * 4 + 2, 1 * 4 + 2]] += 1      # im near -1: rows 0 | 1
    want[[2 * 4 + 3, 16]] += 1             # re near 2: bin 3 | outside
    want[[2 * 4 + 0, 16]] += 1             # re near -2: outside | bin 0
    assert np.array_equal(maybe, want)
    got = np.concatenate([DE.bin_points(Z, G, L)[0].ravel(), [DE.bin_points(Z, G, L)[1]]])
    assert np.all(got >= dec) and np.all(got - dec <= maybe) and got.sum() == Z.size


# ---------------------------------------------------------------- the precondition of the GPU comparisons
@pytest.mark.parametrize("st", load_stages(), ids=lambda s: s["name"])
def test_stage_fixtures_are_decided_and_inside(st):
    """tests/test_gpu_density.py demands equality with the binning of the fixture's Z: that needs every
    point further than the project's tolerance on Z (rtol = atol = 1e-9) from every grid line."""
    Z = stage_arrays(st["name"])["Z"].reshape(st["S"], st["N"])
    assert np.max(np.abs(Z.real)) < 2.0 and np.max(np.abs(Z.imag)) < 2.0
    for G in (31, 128):
        assert not DE.undecided(Z, 1e-9 * (1.0 + np.abs(Z)), G, 2.0).any(), G
        counts, outside = DE.bin_points(Z, G, 2.0)
        assert outside == 0 and counts.sum() == Z.size


# ---------------------------------------------------------------- ConstellationDensity
def test_constellation_density_arithmetic_edges_and_image():
    counts = np.zeros((4, 4), np.int64)
    counts[0, 3] = 9
    counts[2, 1] = 1
    d = E.ConstellationDensity(counts=counts, outside=2, extent=2.0, n_points=12, subcarriers=(0, 64))
    assert d.bins == 4 and d.counts.sum() + d.outside == d.n_points
    assert d.edges.tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0]
    e = E.ConstellationDensity(counts=np.zeros((31, 31), np.int64), outside=0, extent=1.5, n_points=0, subcarriers=(0, 8))
    assert len(e.edges) == 32 and e.edges[0] == -1.5 and e.edges[-1] == pytest.approx(1.5, abs=1e-15)
    assert np.all(np.diff(e.edges) > 0)
    img = d.to_image(scale=1)
    assert img.size == (4, 4) and img.mode == "L"
    px = np.asarray(img)
    # the imaginary axis points up: row 0 of the counts is the image's last row
    assert px[3, 3] == 255 and px[1, 1] == round(255 * np.log1p(1) / np.log1p(9)) and int(px.sum()) == 255 + int(px[1, 1])
    assert d.to_image().size == (16, 16) and np.asarray(e.to_image(scale=1)).sum() == 0


def test_density_grid_refuses_bad_grids():
    assert E.density_grid(128, 2.0) == (-2.0, 32.0)
    for bad in (0, -1, 129, 2.5, True):
        with pytest.raises(ValueError, match="density"):
            E.density_grid(bad, 2.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="density_extent"):
            E.density_grid(8, bad)


# ---------------------------------------------------------------- the engine over the oracle double
class DensityEngine(SweepEngine):
    """SweepEngine whose rx takes the density record: it bins the points it equalises (the oracle's
    arithmetic, as OracleEngine.rx) with density_expect.bin_points and stores the tap.  Every rx call is
    logged with its keyword names, its z_out and z_keep."""
    lut_reach = float(np.max(np.abs(O.qam_lut(CASE["M"]).real)))

    def __init__(self, *a):
        super().__init__(*a)
        self.log = []
        self.records = []

    def rx(self, stream, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits_d, sym0, n_sym, n_valid,
           counters, z_out=None, z_keep=0, **kw):
        self.log.append((sym0, n_sym, tuple(sorted(kw)), z_out is not None, z_keep))
        super().rx(stream, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits_d, sym0, n_sym, n_valid,
                   counters)
        if not kw and z_out is None:
            return
        N, cp = self.n_fft, self.cp
        _, nr, ni = self.streams[seed]
        sigma = np.sqrt(float(stats[0]) / total_samples / 10 ** (snr_db / 10) / 2)
        g = (np.arange(sym0, sym0 + n_sym)[:, None] * (N + cp) + cp + np.arange(N)[None, :])
        v = y[:n_sym].numpy() + sigma * (nr.numpy()[g] + 1j * ni.numpy()[g])
        Z = O.equalize(np.fft.fft(v, axis=1, norm="ortho"), self.H, self.eq, snr_db)
        if z_out is not None and z_keep:
            z_out[:z_keep] = torch.from_numpy(Z[:z_keep])
        if kw:
            assert set(kw) == {"density", "density_params", "density_subcarriers"}
            rec, (lo, inv_w, G), (k_lo, k_hi) = kw["density"], kw["density_params"], kw["density_subcarriers"]
            assert rec.dtype == torch.int64 and rec.shape == (G * G + 1,)
            # the record sits right behind the two counters in the run's one buffer
            assert rec.data_ptr() == counters.data_ptr() + 16
            L = -lo
            assert (lo, inv_w) == DE.grid(G, L)
            self.records.append(rec)
            c, o = DE.bin_points(Z, G, L, k_lo, k_hi)
            rec[:G * G] += torch.from_numpy(c.ravel())
            rec[G * G] += o


def make(S):
    h = channel(CASE["ch"])
    eng = DensityEngine(CASE["N"], CASE["M"], h, len(h) - 1, CASE["eq"])
    eng.seed_streams(SEED, S)
    return eng


def record(st):
    d = st.density
    return (st.bit_errors, st.symbol_errors, d.counts.tolist(), d.outside, d.n_points, d.extent, d.subcarriers)


def test_engine_record_resident_batched_and_tapped():
    S, N = 11, CASE["N"]
    eng = make(S)
    plain = eng.run(S, CASE["snr"], seed=SEED)
    assert plain.density is None and eng.log == [(0, S, (), False, 0)]
    res = eng.run(S, CASE["snr"], seed=SEED, density=16, density_extent=2.0, keep_symbols=S)
    d = res.density
    assert (res.bit_errors, res.symbol_errors) == (plain.bit_errors, plain.symbol_errors)
    assert d.counts.shape == (16, 16) and d.counts.dtype == np.int64 and d.extent == 2.0 and d.subcarriers == (0, N)
    assert d.n_points == S * N == int(d.counts.sum()) + d.outside
    c, o = DE.bin_points(res.received.reshape(S, N), 16, 2.0)
    assert np.array_equal(d.counts, c) and d.outside == o
    for kw in (dict(batch=3), dict(batch=1), dict(y_budget=4 * eng._ybytes())):
        assert record(eng.run(S, CASE["snr"], seed=SEED, density=16, density_extent=2.0, **kw)) == record(res), kw
    # the default extent: 1.5 times the LUT pool's largest coordinate; the range reaches the receiver
    dflt = eng.run(S, CASE["snr"], seed=SEED, density=8, density_subcarriers=(5, 9)).density
    assert dflt.extent == 1.5 * eng.lut_reach and dflt.subcarriers == (5, 9) and dflt.n_points == 4 * S
    assert np.array_equal(dflt.counts, DE.bin_points(res.received.reshape(S, N), 8, dflt.extent, 5, 9)[0])
    # every record seen by rx was the tail of the run's one accumulator
    assert all(r.shape == (r.numel(),) for r in eng.records)


def test_schedule_without_density_is_unchanged_and_a_tap_keeps_one_form():
    """Without density no rx call carries a new keyword, and only the first batch has the tap.  With
    density and a tap every batch is handed the tap buffer, the later ones with z_keep = 0."""
    S = 7
    eng = make(S)
    eng.run(S, CASE["snr"], seed=SEED, batch=3, keep_symbols=2)
    assert eng.log == [(0, 3, (), True, 2), (3, 3, (), False, 0), (6, 1, (), False, 0)]
    eng.log.clear()
    kw = ("density", "density_params", "density_subcarriers")
    eng.run(S, CASE["snr"], seed=SEED, batch=3, keep_symbols=2, density=4)
    assert eng.log == [(0, 3, kw, True, 2), (3, 3, kw, True, 0), (6, 1, kw, True, 0)]
    eng.log.clear()
    eng.run(S, CASE["snr"], seed=SEED, batch=4, density=4)
    assert eng.log == [(0, 4, kw, False, 0), (4, 3, kw, False, 0)]


def test_engine_refusals():
    eng = make(8)
    with pytest.raises(ValueError, match="profile"):
        eng.run(8, CASE["snr"], seed=SEED, density=8, profile=True)
    with pytest.raises(ValueError, match="frame_symbols"):
        eng.run(8, CASE["snr"], seed=SEED, density=8, frame_symbols=2)
    with pytest.raises(ValueError, match="run_sweep"):
        eng.run_sweep(8, [10.0, 12.0], seed=SEED, density=8)
    with pytest.raises(ValueError, match="run_pipelined"):
        eng.run_pipelined(8, CASE["snr"], [SEED], density=8)
    for bad in (0, 129, 2.5):
        with pytest.raises(ValueError, match="density"):
            eng.run(8, CASE["snr"], seed=SEED, density=bad)
    with pytest.raises(ValueError, match="density_extent"):
        eng.run(8, CASE["snr"], seed=SEED, density=8, density_extent=0.0)
    for bad in ((5, 5), (-1, 4), (0, CASE["N"] + 1), (3,)):
        with pytest.raises(ValueError, match="density_subcarriers"):
            eng.run(8, CASE["snr"], seed=SEED, density=8, density_subcarriers=bad)
    with pytest.raises(ValueError, match="without density"):
        eng.run(8, CASE["snr"], seed=SEED, density_extent=2.0)
    # fused=True has no record; None takes the two-kernel path
    eng._fused = True
    with pytest.raises(ValueError, match="density record"):
        eng.run(8, CASE["snr"], seed=SEED, density=8, fused=True)
    assert eng.log == []
    eng.run(8, CASE["snr"], seed=SEED, density=8)
    assert len(eng.log) == 1   # (rx was called: the two-kernel path)


def _worker(rank, world, port, batch, S, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = make(S)
    out[rank] = record(eng.run(S, CASE["snr"], seed=SEED, density=16, density_extent=1.25, group=dist.group.WORLD,
                               batch=batch))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,batch", [(2, None), (3, 4)])
def test_sharded_record_equals_the_single_process_record(world, batch):
    """The record rides the counters' all-reduce: every rank adds its own symbols and holds the whole."""
    S = 13
    want = record(make(S).run(S, CASE["snr"], seed=SEED, density=16, density_extent=1.25))
    assert want[3] > 0 and want[4] == S * CASE["N"]   # L = 1.25 leaves points outside
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), batch, S, out), nprocs=world, join=True)
    for r in range(world):
        assert out[r] == want, (world, r)


# ---------------------------------------------------------------- Simulation and the settings
def test_settings_keys():
    base = dict(num_bands=64, signal_noise_ratios=[10.0], channel_model_path="", num_symbols=8)
    s0 = SimulationSettings(**base)
    assert s0.constellation_density is None and s0.constellation_density_extent is None
    s = SimulationSettings(**base, constellation_density=64, constellation_density_extent=2.0)
    assert (s.constellation_density, s.constellation_density_extent) == (64, 2.0)
    for bad in (dict(constellation_density=0), dict(constellation_density=129), dict(constellation_density_extent=0.0)):
        with pytest.raises(ValueError):
            SimulationSettings(**base, **bad)
    sims = Simulation.create_from_simulation_settings(s)
    assert [(x.constellation_density, x.constellation_density_extent) for x in sims] == [(64, 2.0)]
    assert Simulation.create_from_simulation_settings(s0)[0].constellation_density is None


def test_simulation_run_sweep_refuses_density():
    sims = [Simulation(num_symbols=64 * 4, snr_db=q, rng_mode="philox", seed=1, received_symbols_keep=0,
                       verbose=False, make_plot=False, constellation_density=8) for q in (10.0, 12.0)]
    with pytest.raises(ValueError, match="constellation_density"):
        Simulation.run_sweep(sims)


def test_simulation_refusals_come_before_the_run():
    from ofdm_based_systems.modulation.models import OFDMModulator

    class MyModulator(OFDMModulator):
        pass

    class Composed(Simulation):
        MODULATOR_SCHEME_MAPPERS = {k: MyModulator for k in Simulation.MODULATOR_SCHEME_MAPPERS}

    kw = dict(num_symbols=64 * 4, verbose=False, make_plot=False)
    with pytest.raises(ValueError, match="built-in"):
        Composed(constellation_density=8, **kw).run()
    with pytest.raises(ValueError, match="subcarrier_profile"):
        Simulation(constellation_density=8, subcarrier_profile=True, **kw).run()
    with pytest.raises(ValueError, match="frame_symbols"):
        Simulation(constellation_density=8, frame_symbols=2, **kw).run()
    for bad in (0, -1, 2.5, 129):
        with pytest.raises(ValueError, match="density"):
            Simulation(constellation_density=bad, **kw).run()
    with pytest.raises(ValueError, match="density_extent"):
        Simulation(constellation_density=8, constellation_density_extent=-1.0, **kw).run()

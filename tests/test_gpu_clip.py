"""The clipped transmitter on the GPU (ofdm_tx_clip, LinkEngine(clip_db=...), Simulation(clip_db=...))
against tests/clip_expect.py, the restatement of a clipped throughput-mode run.

* stored samples, statistics and the clip record of every code path: the generic form (N = 1 .. 4096, zero
  padding, cp > lanes per symbol, SC-OFDM, PSK, adaptive loading) in both precisions, and the two
  complex128 throughput forms (flat, window FIR) over several chunks and a ragged tail -- and the
  generic form on the same shapes through caller bits equal to the Philox bits;
* error counts inside the restatement's decision brackets (test_gpu_philox_parity.check_error_counts'
  procedure and caps), and exactly equal with the noise off;
* invariance under batching, rank count and the sweep; the profile, a +40 dB level and Simulation;
* the refusals.

Tolerances: the stored samples' are test_gpu_philox_parity.test_tx_samples_match_oracle's (1e-12 / 1e-4 of
the rms sample, statistics at relative 1e-12 / 1e-5); the clip count lies inside the helper's bracket, whose
width the CPU test caps (complex128: 0, i.e. equality)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import ROOT, channel

import clip_expect as CX
from ofdm_based_systems import _backend as B
from ofdm_based_systems.engine import LinkEngine, new_stats
from test_gpu_multirank import _env, _port
from test_gpu_philox_parity import EQ, bracket_width_bound, gpu_radius, stat_width_bound

pytestmark = pytest.mark.gpu

PRECS = [B.OFDM_F64, B.OFDM_F32]
PNAME = {B.OFDM_F64: "f64", B.OFDM_F32: "f32"}
BY_ID = {c["id"]: c for c in CX.CASES}
# symbols per workgroup of the two complex128 throughput transmitters at N = 1024 (64 lanes per symbol):
# the flat one runs 1024 threads, the window-FIR one 256
FAST_SPB = {"n1024_qam64_4db": 16, "n1024_qam64_1db": 4, "n1024_qam64_lead0_4db": 4, "n1024_qam64_p1_4db": 4}


def make_engine(case, prec, clip_db="case", eq=None):
    h = CX.case_taps(case, channel)
    cp = case.get("cp", len(h) - 1)
    luts, sc = CX.case_plan(case)
    eng = LinkEngine(case["N"], cp, h, EQ[eq or case["eq"]], luts, sc, prec,
                     prefix=B.PREFIX_ZERO if case.get("prefix") == "ZP" else B.PREFIX_CYCLIC,
                     modulator=B.MOD_SC if case.get("modulator") == "SC" else B.MOD_OFDM,
                     clip_db=case["clip_db"] if clip_db == "case" else clip_db)
    return eng, h, cp


def symbols(case, prec):
    """S of a case; the complex128 throughput forms: two rounds of the device's compute units times the
    kernel's symbols per workgroup, plus 37 -- a ragged tail and several chunks."""
    if prec == B.OFDM_F64 and case["id"] in FAST_SPB:
        return 2 * torch.cuda.get_device_properties(0).multi_processor_count * FAST_SPB[case["id"]] + 37
    return CX.case_symbols(case)


def transmit(eng, S, seed, bits=None):
    y = torch.empty((S, eng.ystride), dtype=eng.cdtype, device="cuda")
    stats = new_stats("cuda")
    rec = torch.zeros(2, dtype=torch.int64, device="cuda")
    bits_d = None if bits is None else eng.upload(bits)
    eng.tx(eng.stream(), bits_d, seed, 0, S, y, stats, clip_counters=rec)
    torch.cuda.synchronize()
    return y.cpu().numpy(), stats.cpu().numpy(), rec.cpu().numpy()


def packed_bits(idx, b):
    """The Philox indices as the caller's byte stream (MSB first, symbol s at bit s N b)."""
    bits = (idx[:, :, None] >> np.arange(b - 1, -1, -1)[None, None, :]) & 1
    return np.packbits(bits.astype(np.uint8).ravel())


def check_stored(case, prec, got, ref, a2, what=""):
    y, st, rec = got
    name = PNAME[prec]
    rms = np.sqrt(np.mean(np.abs(ref.y) ** 2))
    tol, rt = (1e-12, 1e-12) if prec == B.OFDM_F64 else (1e-4, 1e-5)
    dev = float(np.max(np.abs(y - ref.y)) / rms)
    lo, hi = ref.count_bracket(name, a2)
    print(f"{case['id']} {name}{what}: max deviation {dev:.3e} rms (tol {tol}), clipped {rec[0]} in [{lo}, {hi}] "
          f"of {rec[1]}, power {st[0]:.12e} / {ref.power_sum:.12e}, peak {st[2]:.12e} / {ref.x_peak:.12e}")
    assert y.shape == ref.y.shape
    assert dev <= tol
    assert st[0] == pytest.approx(ref.power_sum, rel=rt)
    assert st[1] == pytest.approx(ref.x_power_sum, rel=rt)
    assert st[2] == pytest.approx(ref.x_peak, rel=rt)
    assert lo <= rec[0] <= hi
    assert rec[1] == ref.samples


_refs = {}


def restated(case, S, h, cp):
    """The noiseless restatement of a case at S symbols, computed once and shared."""
    key = (case["id"], S)
    if key not in _refs:
        _refs[key] = CX.case_expect(case, h=h, cp=cp, eq=case["eq"], S=S)
    return _refs[key]


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("case", CX.CASES, ids=lambda c: c["id"])
def test_stored_samples_match_the_restatement(gpu, case, prec):
    eng, h, cp = make_engine(case, prec)
    S = symbols(case, prec)
    a2 = CX.case_threshold(case)
    assert eng.clip_a2 == a2 and eng.nominal_power == CX.nominal_power(case["N"], *CX.case_plan(case))
    ref = restated(case, S, h, cp)
    got = transmit(eng, S, CX.SEED)
    check_stored(case, prec, got, ref, a2)
    if prec == B.OFDM_F64:
        assert got[2][0] == ref.clipped
    if case.get("fast") and prec == B.OFDM_F64:
        # the generic form on the same shape: caller bits equal to the Philox bits
        gen = transmit(eng, S, CX.SEED, bits=packed_bits(ref.idx, 6))
        check_stored(case, prec, gen, ref, a2, " (generic form, caller bits)")
        assert gen[2][0] == got[2][0]
        rms = np.sqrt(np.mean(np.abs(ref.y) ** 2))
        assert np.max(np.abs(gen[0] - got[0])) <= 1e-12 * rms
        # ... and it is another kernel: the generic form's transform rounds differently (other twiddle
        # tables), so equal bits here would mean the Philox run was not routed to the throughput form
        # (test_a_40_db_level_is_the_unclipped_run pins the other half: the throughput form's bits)
        assert not np.array_equal(gen[0], got[0])


# ------------------------------------------------------------------ error counts
def tx_deviation(eng, seed, S):
    """test_gpu_philox_parity.tx_deviation on the clipped transmitter."""
    got = transmit(eng, S, seed)[0].astype(np.complex128)
    return lambda yref: float(np.sqrt(np.mean(np.abs(got - yref) ** 2)))


# case, equaliser, SNR dB, OFDM symbols.  Restated on the CPU (seed 77, without the GPU's radii: an upper
# bound on the widths) -- bit errors / bracket width in complex128 / in complex64:
#   N = 64 16-QAM severe MMSE, 3 dB, 18 dB SNR:  355 (66 without the limiter) / 0 / 0
#   N = 1024 64-QAM flat, 4 dB, 24 dB:           10683 / 2 / 72
#   N = 1024 64-QAM severe MMSE, 4 dB, 27 dB:    9125 / 9 / 167
#   SC 16-QAM N = 256 P1 ZF, 1 dB, 20 dB:        814 / 1 / 6
#   N = 8 4-QAM two_ray ZF ZP, 2 dB, 12 dB:      width 0 / 0
#   N = 64 16-QAM h = [0, 0.8, 0.6j] MMSE, 3 dB, 18 dB (a whole run on a leading-delay channel): 979 / 0 / 1
COUNT_CASES = [
    (BY_ID["n64_qam16_3db"], "MMSE", 18.0, 99),
    (BY_ID["n1024_qam64_4db"], "NONE", 24.0, 67),
    (dict(BY_ID["n1024_qam64_1db"], id="n1024_qam64_severe_4db", clip_db=4.0), "MMSE", 27.0, 67),
    (BY_ID["sc_qam16_n256_1db"], "ZF", 20.0, 135),
    (dict(id="n8_qam4_2db_zp", N=8, M=4, clip_db=2.0, ch="two_ray", cp=2, eq="ZF", prefix="ZP"), "ZF", 12.0, 547),
    (BY_ID["n64_qam16_lead0_3db"], "MMSE", 18.0, 99),
]


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("case,eq,snr,S", COUNT_CASES, ids=[c[0]["id"] for c in COUNT_CASES])
def test_error_counts_match_the_restatement(gpu, case, eq, snr, S, prec):
    eng, h, cp = make_engine(case, prec, eq=eq)
    seed = 77
    f32 = prec == B.OFDM_F32
    res = eng.run(S, snr, seed=seed)
    ref = CX.run_clipped(seed, S, case["N"], case["M"], h, cp, eq, snr, CX.case_threshold(case),
                         precision=PNAME[prec], radius_fn=gpu_radius, power_sum=res.power_sum,
                         stat_sigma=tx_deviation(eng, seed, S) if f32 else None, **CX.case_kwargs(case))
    be_lo, be_hi, se_lo, se_hi = ref.bracket
    print(f"bracket {case['id']} {PNAME[prec]}: bits {res.bit_errors} in [{be_lo}, {be_hi}] (width {be_hi - be_lo}), "
          f"symbols {res.symbol_errors} in [{se_lo}, {se_hi}] (width {se_hi - se_lo}); restated "
          f"{ref.bit_errors} / {ref.symbol_errors}; clipped {res.clipped_samples} of {res.clip_samples}")
    assert ref.bit_errors > 0
    if f32:
        sb_lo, sb_hi, ss_lo, ss_hi = ref.stat_bracket
        print(f"stat bracket: bits [{sb_lo}, {sb_hi}], symbols [{ss_lo}, {ss_hi}]")
        assert sb_lo <= res.bit_errors <= sb_hi and ss_lo <= res.symbol_errors <= ss_hi, (res, ref.stat_bracket)
        wst = stat_width_bound(ref.bit_errors)
        assert sb_hi - sb_lo <= wst and ss_hi - ss_lo <= wst, (ref.stat_bracket, wst)
    assert be_lo <= ref.bit_errors <= be_hi and se_lo <= ref.symbol_errors <= se_hi
    assert be_lo <= res.bit_errors <= be_hi, (res.bit_errors, ref.bracket)
    assert se_lo <= res.symbol_errors <= se_hi, (res.symbol_errors, ref.bracket)
    wmax = bracket_width_bound(prec, CX.case_kwargs(case), ref.bit_errors)
    if wmax is not None:
        assert be_hi - be_lo <= wmax and se_hi - se_lo <= wmax, (ref.bracket, wmax)
    assert res.power_sum == pytest.approx(ref.power_sum, rel=1e-5 if f32 else 1e-12)
    lo, hi = ref.count_bracket(PNAME[prec], CX.case_threshold(case))
    assert lo <= res.clipped_samples <= hi and res.clip_samples == S * case["N"] and res.clip_db == case["clip_db"]


NOISELESS = dict(id="n64_qam16_2db_flat", N=64, M=16, clip_db=2.0, ch="flat_fading", eq="NONE")


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
def test_without_noise_the_limiter_alone_makes_the_errors(gpu, prec):
    """Noise off: every error comes from the limiter, and the restatement's bracket has width 0 in both
    precisions -- the counts are equal."""
    eng, h, cp = make_engine(NOISELESS, prec)
    S = 99
    res = eng.run(S, 30.0, seed=CX.SEED, noise_on=False)
    ref = CX.run_clipped(CX.SEED, S, 64, 16, h, cp, "NONE", 30.0, CX.case_threshold(NOISELESS), noise_on=False,
                         precision=PNAME[prec])
    print(f"noise off {PNAME[prec]}: {res.bit_errors} / {res.symbol_errors}, restated {ref.bit_errors} / "
          f"{ref.symbol_errors}, bracket {ref.bracket}")
    assert ref.bracket == (ref.bit_errors, ref.bit_errors, ref.symbol_errors, ref.symbol_errors)
    assert (ref.bit_errors, ref.symbol_errors) == (224, 222)
    assert (res.bit_errors, res.symbol_errors) == (ref.bit_errors, ref.symbol_errors)
    plain = make_engine(NOISELESS, prec, clip_db=None)[0].run(S, 30.0, seed=CX.SEED, noise_on=False)
    assert (plain.bit_errors, plain.symbol_errors, plain.clipped_samples) == (0, 0, None)


# ------------------------------------------------------------------ invariance
def record(st):
    return [st.bit_errors, st.symbol_errors, st.clipped_samples, st.clip_samples, st.power_sum.hex(),
            st.x_power_sum.hex(), st.x_peak.hex()]


INV = dict(cid="n1024_qam64_1db", S=300, snr=27.0, seed=31)


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
def test_batching_and_the_sweep_change_nothing(gpu, prec):
    eng = make_engine(BY_ID[INV["cid"]], prec)[0]
    S, seed = INV["S"], INV["seed"]
    whole = eng.run(S, INV["snr"], seed=seed)
    assert whole.bit_errors > 0 and whole.clipped_samples > 0 and whole.clip_samples == S * 1024
    batched = eng.run(S, INV["snr"], seed=seed, batch=S // 3 + 1)  # three batches
    assert record(batched) == record(whole)
    snrs = [24.0, INV["snr"], 30.0]
    singles = [record(eng.run(S, q, seed=seed)) for q in snrs]
    assert [record(s) for s in eng.run_sweep(S, snrs, seed=seed)] == singles
    assert [record(s) for s in eng.run_sweep(S, snrs, seed=seed, batch=S // 3 + 1)] == singles
    assert len({r[0] for r in singles}) == 3


def test_two_ranks_match_one_rank(gpu, tmp_path):
    """Two gloo ranks on device 0, in a fresh child process each (tests/clip_rank_worker.py)."""
    out = tmp_path / "ranks.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}",
           os.path.join(ROOT, "tests", "clip_rank_worker.py"), str(out)]
    r = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(out.read_text())
    assert got["world"] == 2
    eng = make_engine(BY_ID[INV["cid"]], B.OFDM_F64)[0]
    one = eng.run(INV["S"], INV["snr"], seed=INV["seed"])
    want = record(one)
    for name in ("whole", "batched"):
        rec = got[name]
        # counts, the clip record and the exact power: identical; sum |x|^2 adds in rank order (rel 1e-12)
        assert rec[:5] == want[:5] and rec[6] == want[6], (name, rec, want)
        assert float.fromhex(rec[5]) == pytest.approx(one.x_power_sum, rel=1e-12)


# ------------------------------------------------------------------ interplay
@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
def test_profile_sees_the_clipping_noise(gpu, prec):
    case = BY_ID["n1024_qam64_4db"]
    eng, h, cp = make_engine(case, prec)
    S = CX.case_symbols(case)
    st = eng.run(S, 30.0, seed=CX.SEED, noise_on=False, profile=True)
    ref = restated(case, S, h, cp)
    evm = float(st.profile.error_power.sum()) / (S * 1024)
    print(f"profile {PNAME[prec]}: error-vector power per symbol {evm:.6e}, restated {ref.evm:.6e}; "
          f"symbol errors {st.symbol_errors}")
    assert int(st.profile.symbol_errors.sum()) == st.symbol_errors
    assert int(st.profile.bit_errors.sum()) == st.bit_errors
    assert evm == pytest.approx(ref.evm, rel=0.05)
    assert st.clipped_samples > 0


# A level nothing reaches must leave the stream as it is, bit for bit -- where the unclipped run takes the same
# kernel form.  That is so on the two complex128 throughput shapes (the CLIP instantiation of the same
# throughput kernel), on plans whose unclipped run takes the generic kernel too (N < 64 here), and with
# caller bits on any plan off the bench shapes (generic on both sides).  Elsewhere -- complex64 at N >= 64, or
# complex128 at N = 64 with Philox bits -- the unclipped run takes a throughput kernel whose twiddles come from
# other tables than the generic form's, and the two agree to the transmitter's tolerance, not bit for bit
# (measured: N = 64 16-QAM severe_multipath complex128, 8816 of 9600 samples differ, by at most 9.5e-16 rms;
# N = 1024 complex64, 1.3e-6 rms): those pairs are covered by test_stored_samples_match_the_restatement.
SAME_FORM = [("n1024_qam64_4db", B.OFDM_F64), ("n1024_qam64_1db", B.OFDM_F64), ("n1024_qam64_p1_4db", B.OFDM_F64),
             ("n16_qam16_cp5_3db", B.OFDM_F64), ("n16_qam16_cp5_3db", B.OFDM_F32),
             ("n8_qam16_2db_zp", B.OFDM_F64), ("n8_qam16_2db_zp", B.OFDM_F32)]


def plain_transmit(eng, S, seed, bits=None):
    y = torch.empty((S, eng.ystride), dtype=eng.cdtype, device="cuda")
    eng.tx(eng.stream(), None if bits is None else eng.upload(bits), seed, 0, S, y, new_stats("cuda"))
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("cid,prec", SAME_FORM, ids=[f"{c}-{PNAME[p]}" for c, p in SAME_FORM])
def test_a_40_db_level_is_the_unclipped_run(gpu, cid, prec):
    case = BY_ID[cid]
    high, h, cp = make_engine(case, prec, clip_db=40.0)
    plain = make_engine(case, prec, clip_db=None)[0]
    S, snr = 150, 12.0
    a, b = high.run(S, snr, seed=9), plain.run(S, snr, seed=9)
    print(f"+40 dB {cid} {PNAME[prec]}: {a.bit_errors} / {a.symbol_errors} against {b.bit_errors} / {b.symbol_errors}, "
          f"power {a.power_sum.hex()} / {b.power_sum.hex()}, sum |x|^2 {a.x_power_sum.hex()} / {b.x_power_sum.hex()}")
    assert (a.bit_errors, a.symbol_errors) == (b.bit_errors, b.symbol_errors) and b.bit_errors > 0
    rt = 1e-12 if prec == B.OFDM_F64 else 1e-5
    assert a.power_sum == pytest.approx(b.power_sum, rel=rt) and a.x_power_sum == pytest.approx(b.x_power_sum, rel=rt)
    assert a.x_peak == pytest.approx(b.x_peak, rel=rt)
    assert (a.clipped_samples, a.clip_samples) == (0, S * case["N"]) and b.clipped_samples is None
    ya, _, rec = transmit(high, S, 9)
    assert rec.tolist() == [0, S * case["N"]]
    assert np.array_equal(ya, plain_transmit(plain, S, 9))


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
def test_a_40_db_level_with_caller_bits_is_the_unclipped_stream(gpu, prec):
    """Caller bits take the generic kernel with and without a level (N = 64, off the bench shapes)."""
    case = BY_ID["n64_qam16_3db"]
    high = make_engine(case, prec, clip_db=40.0)[0]
    plain = make_engine(case, prec, clip_db=None)[0]
    S = 150
    bits = np.frombuffer(np.random.Generator(np.random.PCG64(4)).bytes(S * 64 * 4 // 8), np.uint8)
    ya, _, rec = transmit(high, S, 0, bits=bits)
    assert rec.tolist() == [0, S * 64]
    assert np.array_equal(ya, plain_transmit(plain, S, 0, bits=bits))


def test_simulation_returns_the_new_keys(gpu):
    from ofdm_based_systems.simulation.models import Simulation

    kw = dict(num_symbols=64 * 64, num_subcarriers=64, constellation_order=16, snr_db=18.0, verbose=False,
              make_plot=False, rng_mode="philox", seed=3)
    plain = Simulation(**kw).run()
    clipped = Simulation(clip_db=3.0, **kw).run()
    assert set(clipped) - set(plain) == {"clip_db", "clipped_samples", "clipped_fraction"}
    assert set(plain) - set(clipped) == set()
    assert clipped["clip_db"] == 3.0 and clipped["clipped_samples"] > 0
    assert clipped["clipped_fraction"] == clipped["clipped_samples"] / (64 * 64)
    assert 0.02 < clipped["clipped_fraction"] < 0.4   # about exp(-2) of near-Gaussian samples
    assert clipped["bit_errors"] > plain["bit_errors"] and clipped["papr_db"] < plain["papr_db"]
    # today's key set without a level
    assert set(plain) == {
        "num_bits", "num_symbols", "num_subcarriers", "constellation_order", "constellation_scheme",
        "modulator_type", "prefix_scheme", "prefix_acronym", "equalizator_type", "snr_db", "noise_scheme",
        "power_allocation_type", "power_allocation_acronym", "adaptive_modulation_mode",
        "constellation_order_per_subcarrier", "water_level", "title", "subtitle", "allocated_power", "papr_db",
        "bit_errors", "symbol_errors", "total_bits", "bit_error_rate", "symbol_error_rate", "received_symbols",
        "constellation_plot", "transmission_time_ms", "bitrate_mbps"}


# ------------------------------------------------------------------ refusals
def test_refusals_on_the_device(gpu):
    h = np.array([1.0 + 0j])
    with pytest.raises(ValueError, match="above 256 points"):
        LinkEngine(64, 0, h, B.EQ_NONE, [CX.QAM(1024)], clip_db=3.0)
    # the library's own answer for a wide plan, whatever the engine does
    wide = LinkEngine(64, 0, h, B.EQ_NONE, [CX.QAM(1024)])
    rec = torch.zeros(2, dtype=torch.int64, device="cuda")
    y = torch.zeros((4, 64), dtype=torch.complex128, device="cuda")
    bits = torch.zeros(4 * 64 * 10 // 8 + 1, dtype=torch.uint8, device="cuda")
    stats = new_stats("cuda")
    rc = B.lib().ofdm_tx_clip(wide.plan.handle, wide.stream(), B.ptr(bits), 0, 0, 4, B.ptr(y), B.ptr(stats), 1.0, B.ptr(rec))
    assert rc == -1 and b"above 256 points" in B.lib().ofdm_last_error()
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        plain = LinkEngine(64, 0, h, B.EQ_NONE, [CX.QAM(16)])
        assert B.lib().ofdm_tx_clip(plain.plan.handle, plain.stream(), None, 0, 0, 4, B.ptr(y), B.ptr(stats), bad,
                                    B.ptr(rec)) == -1
        assert b"clip_a2" in B.lib().ofdm_last_error()
    # an empty call is fine
    assert B.lib().ofdm_tx_clip(plain.plan.handle, plain.stream(), None, 0, 0, 0, None, B.ptr(stats), 1.0, None) == 0
    torch.cuda.synchronize()
    assert not rec.cpu().numpy().any() and not y.cpu().numpy().any() and not stats.cpu().numpy().any()
    # the fused shape with a level: the two-kernel path, and no fused route
    eng = LinkEngine(1024, 0, h, B.EQ_NONE, [CX.QAM(64)], clip_db=4.0)
    with pytest.raises(ValueError, match="no clip level"):
        eng.run(64, 24.0, seed=1, fused=True)
    with pytest.raises(ValueError, match="papr"):
        eng.papr(64, seed=1)
    with pytest.raises(ValueError, match="run_pipelined"):
        eng.run_pipelined(64, 24.0, [1, 2])
    events = []
    st = eng.run(64, 24.0, seed=1, events=events)
    assert [e[0] for e in events] == ["ofdm_tx", "ofdm_rx"] and st.clipped_samples > 0

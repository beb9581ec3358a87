"""LinkEngine.run_sweep without a GPU: the schedule -- one transmit per batch, the statistics
all-gather, the [K][2] counter all-reduce, the split of a long list into launches -- is the
production code; the two kernels are the oracle's CPU test double (test_distributed_cpu.OracleEngine),
whose rx_sweep calls its rx once per point.  A sweep must equal the single-point runs, resident and
batched, alone and under gloo with uneven shards.  Also the entry point's declaration, export and
binding."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp
from conftest import channel

from ofdm_based_systems import _backend as B
from test_distributed_cpu import CASE, OracleEngine, _free_port

SNRS = [8.0, 14.0, 11.0, 17.0]
SEED = 21


class SweepEngine(OracleEngine):
    """OracleEngine with the sweep receiver: rx per point over the same y (the launches are recorded)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.launches = []

    def rx_sweep(self, stream, y, seed, stats, total_samples, snr_dbs, sym0, n_sym, n_valid, counters):
        assert 1 <= len(snr_dbs) <= B.MAX_SWEEP_POINTS and counters.shape == (len(snr_dbs), 2)
        self.launches.append((sym0, n_sym, len(snr_dbs)))
        for k, snr in enumerate(snr_dbs):
            self.rx(stream, y, None, None, seed, stats, total_samples, snr, True, None, sym0, n_sym, n_valid,
                    counters[k])


def make(S):
    h = channel(CASE["ch"])
    eng = SweepEngine(CASE["N"], CASE["M"], h, len(h) - 1, CASE["eq"])
    eng.seed_streams(SEED, S)
    return eng


def record(s):
    return (s.bit_errors, s.symbol_errors, s.power_sum, s.x_power_sum, s.x_peak, s.papr_db, s.num_ofdm_symbols,
            s.samples)


@pytest.mark.parametrize("batch", [None, 1, 7])
def test_sweep_equals_the_single_point_runs(batch):
    S = 24
    eng = make(S)
    want = [record(eng.run(S, snr, seed=SEED)) for snr in SNRS]
    assert all(w[0] > 0 for w in want) and len({w[0] for w in want}) == len(SNRS)
    eng.launches.clear()
    got = eng.run_sweep(S, SNRS, seed=SEED, batch=batch)
    assert [record(g) for g in got] == want
    # one receiver launch per batch (7 does not divide 24), each over all the points
    nb = 1 if batch is None else -(-S // batch)
    assert [l[2] for l in eng.launches] == [len(SNRS)] * nb and sum(l[1] for l in eng.launches) == S


def test_a_list_longer_than_the_cap_is_split():
    S = 6
    eng = make(S)
    K = B.MAX_SWEEP_POINTS + 3
    snrs = [SNRS[k % len(SNRS)] for k in range(K)]
    short = [record(s) for s in eng.run_sweep(S, SNRS, seed=SEED)]
    eng.launches.clear()
    got = eng.run_sweep(S, snrs, seed=SEED)
    assert [l[2] for l in eng.launches] == [B.MAX_SWEEP_POINTS, 3]
    assert [record(g) for g in got] == [short[k % len(SNRS)] for k in range(K)]


def test_empty_and_non_finite_lists_are_refused():
    eng = make(4)
    with pytest.raises(ValueError):
        eng.run_sweep(4, [], seed=SEED)
    with pytest.raises(ValueError):
        eng.run_sweep(4, [10.0, float("inf")], seed=SEED)
    assert eng.launches == []


def _worker(rank, world, port, batch, S, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = make(S)
    out[rank] = [record(s) for s in eng.run_sweep(S, SNRS, seed=SEED, group=dist.group.WORLD, batch=batch)]
    dist.destroy_process_group()


@pytest.mark.parametrize("world,batch,S", [(2, None, 25), (2, 5, 25), (3, None, 25), (3, 4, 25)])
def test_sharded_sweep_equals_the_single_process_runs(world, batch, S):
    """25 symbols over 2 / 3 ranks: shards of unequal length."""
    eng = make(S)
    want = [record(eng.run(S, snr, seed=SEED)) for snr in SNRS]
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), batch, S, out), nprocs=world, join=True)
    for r in range(world):
        got = out[r]
        # counts, the exact power and the peak: identical; sum |x|^2 adds in rank order
        assert [g[:3] + g[4:5] + g[6:] for g in got] == [w[:3] + w[4:5] + w[6:] for w in want], r
        assert all(abs(g[3] - w[3]) <= 1e-12 * w[3] and abs(g[5] - w[5]) < 1e-9 for g, w in zip(got, want))


def test_entry_point_is_declared_exported_and_bound():
    from test_abi import HEADER, declared_functions

    assert "ofdm_rx_sweep" in declared_functions()
    text = open(HEADER).read()
    decl = text[text.index("int ofdm_rx_sweep("):]
    decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert "const double* snr_db, int32_t n_snr" in decl and "uint64_t* counters" in decl
    at = text.index("int ofdm_rx_sweep(")
    assert "HOST array" in text[text.rindex("/*", 0, at):at]  # the ABI's one host-side array, documented
    assert int(re.search(r"#define OFDM_ABI_VERSION (\d+)", text).group(1)) == B.ABI_VERSION
    assert int(re.search(r"#define OFDM_MAX_SWEEP_POINTS (\d+)", text).group(1)) == B.MAX_SWEEP_POINTS >= 40
    lib = B.load_library()
    assert hasattr(lib, "ofdm_rx_sweep") and "ofdm_rx_sweep" in B.SIGNATURES
    assert lib.ofdm_abi_version() == B.ABI_VERSION
    assert len(B.SIGNATURES["ofdm_rx_sweep"][1]) == 12
    assert set(B.SIGNATURES) == set(declared_functions())


def test_null_plan_is_invalid_without_a_gpu():
    lib = B.load_library()
    snrs = (ctypes.c_double * 2)(10.0, 12.0)
    assert lib.ofdm_rx_sweep(None, None, None, 0, None, 0, snrs, 2, 0, 0, 0, None) == -1
    assert b"ofdm_rx_sweep" in lib.ofdm_last_error()

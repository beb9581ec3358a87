"""Rank program of tests/test_gpu_soft.py::test_two_ranks_hold_the_one_rank_record (not a test
module): two gloo ranks bind device 0 (as tests/multirank_worker.py), run the first throughput case of
tests/profile_expect.py (N = 1024, 64-QAM, flat) through LinkEngine.run(group=..., soft=64) -- every
rank bins the bits of its own shard and the counters' all-reduce carries the record -- and every rank writes the
record it holds as JSON to argv[1].<rank>.json."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ofdm-based-systems_amd"), os.path.join(ROOT, "oracle"),
                os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import ofdm_oracle as O  # noqa: E402
import profile_expect as PE  # noqa: E402
from ofdm_based_systems import _backend as B  # noqa: E402
from ofdm_based_systems.engine import LinkEngine, shard  # noqa: E402


def main():
    out = sys.argv[1]
    torch.cuda.set_device(int(os.environ.get("OFDM_BENCH_DEVICE", "0")))
    dist.init_process_group("gloo")
    g = dist.group.WORLD
    rank, world = dist.get_rank(), dist.get_world_size()
    case = PE.THROUGHPUT_CASES[0]
    h, cp, _ = PE.case_channel(case)
    eq = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}[case["eq"]]
    eng = LinkEngine(case["N"], cp, h, eq, [O.qam_lut(case["M"])], None, B.OFDM_F64)
    res = eng.run(case["S"], case["snr"], seed=PE.SEED, group=g, soft=64)
    d = res.soft
    with open(f"{out}.{rank}.json", "w") as f:
        json.dump({"world": world, "shard": list(shard(case["S"], rank, world)),
                   "totals": [res.bit_errors, res.symbol_errors], "counts": d.counts.tolist(),
                   "invalid": d.invalid, "n_bits": d.n_bits}, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

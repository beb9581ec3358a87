"""Rank program of tests/test_gpu_frames.py::test_two_ranks_hold_the_one_rank_record (not a test
module): two gloo ranks bind device 0 (as tests/multirank_worker.py), run the second throughput case
of tests/profile_expect.py through LinkEngine.run(group=..., frame_symbols=4) -- the shard boundary 81
splits frame 20 -- and every rank writes the record it holds, [bit errors, symbol errors] x frames, as
JSON to argv[1].<rank>.json."""

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
    case = PE.THROUGHPUT_CASES[1]
    h, cp, _ = PE.case_channel(case)
    eq = {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}[case["eq"]]
    eng = LinkEngine(case["N"], cp, h, eq, [O.qam_lut(case["M"])], None, B.OFDM_F64)
    res = eng.run(case["S"], case["snr"], seed=PE.SEED, group=g, frame_symbols=4)
    with open(f"{out}.{rank}.json", "w") as f:
        json.dump({"world": world, "shard": list(shard(case["S"], rank, world)),
                   "totals": [res.bit_errors, res.symbol_errors],
                   "record": [res.frames.bit_errors.tolist(), res.frames.symbol_errors.tolist()]}, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

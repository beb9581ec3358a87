"""Rank program of tests/test_gpu_papr.py::test_two_ranks_hold_the_one_rank_histogram (not a test
module): two gloo ranks bind device 0 (as tests/multirank_worker.py), run the N = 1024 64-QAM case of
tests/papr_expect.py through LinkEngine.papr(group=...), and every rank writes the histogram it holds
and the first kept pairs of its shard as JSON to argv[1].<rank>.json."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ofdm-based-systems_amd"), os.path.join(ROOT, "oracle"),
                os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import papr_expect as PX  # noqa: E402
from ofdm_based_systems import _backend as B  # noqa: E402
from ofdm_based_systems.engine import LinkEngine, shard  # noqa: E402


def main():
    out = sys.argv[1]
    torch.cuda.set_device(int(os.environ.get("OFDM_BENCH_DEVICE", "0")))
    dist.init_process_group("gloo")
    g = dist.group.WORLD
    rank, world = dist.get_rank(), dist.get_world_size()
    case = next(c for c in PX.CASES if c["id"] == "n1024_qam64")
    S = PX.S_of(case["N"])
    eng = LinkEngine(case["N"], case["cp"], np.array([1.0 + 0j]), B.EQ_NONE, case["luts"](), None, B.OFDM_F64)
    st = eng.papr(S, seed=PX.SEED, group=g, keep=4, batch=50)
    with open(f"{out}.{rank}.json", "w") as f:
        json.dump({"world": world, "shard": list(shard(S, rank, world)), "histogram": st.histogram.tolist(),
                   "kept": st.per_symbol.tolist()}, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

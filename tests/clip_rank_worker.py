"""Rank program of tests/test_gpu_clip.py::test_two_ranks_match_one_rank (not a test module): every rank
binds device 0 over gloo (as tests/multirank_worker.py), runs the clipped complex128 window-FIR shape
through LinkEngine's sharded schedules, resident and batched, and rank 0 writes the results as JSON."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ofdm-based-systems_amd")]

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import test_gpu_clip as T  # noqa: E402
from ofdm_based_systems import _backend as B  # noqa: E402


def main():
    out_path = sys.argv[1]
    torch.cuda.set_device(int(os.environ.get("OFDM_BENCH_DEVICE", "0")))
    dist.init_process_group("gloo")
    g = dist.group.WORLD
    eng = T.make_engine(T.BY_ID[T.INV["cid"]], B.OFDM_F64)[0]
    S, snr, seed = T.INV["S"], T.INV["snr"], T.INV["seed"]
    whole = eng.run(S, snr, seed=seed, group=g)
    batched = eng.run(S, snr, seed=seed, group=g, batch=S // 6 + 1)  # three batches per rank
    if dist.get_rank() == 0:
        with open(out_path, "w") as f:
            json.dump({"world": dist.get_world_size(), "whole": T.record(whole), "batched": T.record(batched)}, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

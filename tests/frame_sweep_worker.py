"""Rank program of tests/test_gpu_frame_sweep.py::test_two_ranks_hold_the_one_rank_record (not a test
module): every rank binds device 0 over gloo (as tests/multirank_worker.py), runs one case's SNR sweep
with the frame record through LinkEngine.run_frame_sweep with the group -- whole shard resident, and
batched -- and every rank writes every point's record as JSON to argv[1].<rank>.json.
argv: output path, JSON [N, M, channel, equaliser, symbols, [SNR points], seed, frame length]."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ofdm-based-systems_amd"), os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import ofdm_oracle as O  # noqa: E402
from ofdm_based_systems import _backend as B  # noqa: E402
from ofdm_based_systems.engine import LinkEngine, shard  # noqa: E402


def record(s):
    return [s.bit_errors, s.symbol_errors, s.power_sum.hex(), s.x_peak, s.frames.bit_errors.tolist(),
            s.frames.symbol_errors.tolist()]


def main():
    out = sys.argv[1]
    N, M, ch, eq, S, snrs, seed, F = json.loads(sys.argv[2])
    torch.cuda.set_device(int(os.environ.get("OFDM_BENCH_DEVICE", "0")))
    dist.init_process_group("gloo")
    g = dist.group.WORLD
    rank, world = dist.get_rank(), dist.get_world_size()
    h = np.load(os.path.join(ROOT, "config", "channel_models", ch + ".npy"))
    eng = LinkEngine(N, len(h) - 1, h, {"NONE": B.EQ_NONE, "ZF": B.EQ_ZF, "MMSE": B.EQ_MMSE}[eq], [O.qam_lut(M)])
    whole = eng.run_frame_sweep(S, snrs, F, seed=seed, group=g)
    batched = eng.run_frame_sweep(S, snrs, F, seed=seed, group=g, batch=S // (2 * world) + 7)
    with open(f"{out}.{rank}.json", "w") as f:
        json.dump({"world": world, "shard": list(shard(S, rank, world)), "whole": [record(s) for s in whole],
                   "batched": [record(s) for s in batched]}, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

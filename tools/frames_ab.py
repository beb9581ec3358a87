#!/usr/bin/env python3
"""Cost of the per-frame error record (ofdm_rx_frames, LinkEngine.run(frame_symbols=1)) against the plain
receiver of the same plan, on one GPU in complex128: bench configs (b) -- the two-kernel path, fused=False,
at its 24 dB and at 10 dB, where nearly every symbol issues its atomics -- (c) and (e) at the bench's
symbols per step.  In one process, after a warm-up, steps alternate

    A  run(n, snr, fused=False)                     ofdm_tx + ofdm_rx
    B  run(n, snr, fused=False, frame_symbols=1)    ofdm_tx + ofdm_rx_frames, a frame per symbol

and the receiver's HIP-event time and the step's wall time (launch to result()) are reported as medians
with their spread; the A column's own spread is the run-to-run noise the difference is read against.

The expectation it is compared with is static: the VALU instructions of the symbol loop of k_rx_frames
against those of its k_rx counterpart (tools/isa_mix.py on a device-only compile of the two kernels of
each config; needs hipcc, no GPU):

    python tools/frames_ab.py --static profiles/frames_static.json          # no GPU
    python tools/frames_ab.py [--steps 20] [--warmup 3] --out measured.json  # on the GPU
    python tools/frames_ab.py --report profiles/frames_static.json measured.json > profiles/frames_ab.txt
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ofdm-based-systems_amd")]

import numpy as np  # noqa: E402

# (config, SNR in dB or None = the config's own, symbols per step: bench.py's 1e6 // (N / 1024))
CASES = (("b", None, 1_000_000), ("b", 10.0, 1_000_000), ("c", None, 1_000_000), ("e", None, 250_000))


# config: the template arguments <R, log2 N, EQ, FB, MV> of its throughput receiver
STATIC = {"b": "double, 10, 0, 6, false", "c": "double, 10, 2, 6, false", "e": "double, 12, 2, 8, false"}


def static_counts(hipcc="/opt/rocm/bin/hipcc"):
    """Per config, from a device-only compile of the pair: (instructions, VALU, weighted VALU issue) of the
    whole kernel and of its largest loop (tools/isa_mix.py) for k_rx and k_rx_frames.  The new sequence's
    VALU are the difference of the two kernels' totals -- everything k_rx_frames adds sits inside the symbol
    loop, the branch a symbol with errors takes included -- and the receiver loop they are set against is
    k_rx's largest loop (the symbol loop; where the layout folds the short reduction loops behind it into
    the same back edge it is a few per cent larger, which makes the estimate smaller by as much)."""
    src = '#include "ofdm_record_inst.hpp"\nnamespace ofdm {\n' + "".join(
        f"template __global__ void k_rx<{a}, false, false>(RxArgs);\n"
        f"template __global__ void k_rx_frames<{a}, false>(RxArgs, RxFramesTail);\n" for a in STATIC.values()) + "}\n"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        hip, asm = os.path.join(d, "pair.hip"), os.path.join(d, "pair.s")
        open(hip, "w").write(src)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-DOFDM_TX_WAVES=3",
                        "-DOFDM_RX_WAVES=1", "-Wno-unused-function", f"-I{ROOT}/include",
                        f"-I{ROOT}/ofdm-based-systems_amd/csrc", "--cuda-device-only", "-S", hip, "-o", asm], check=True,
                       stderr=subprocess.DEVNULL)
        names = re.findall(r"^(_ZN4ofdm\d+k_rx\w*):", open(asm).read(), re.M)
        dem = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")
        for name, d_ in zip(names, dem):
            txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_mix.py"), asm, name], check=True,
                                 capture_output=True, text=True).stdout
            pat = r": (\d+) instr, (\d+) VALU, weighted VALU issue (\d+)"
            loops = [tuple(int(x) for x in m) for m in re.findall(r"== loop \[\d+, \d+\]" + pat, txt)]
            whole = tuple(int(x) for x in re.search(r"== kernel" + pat, txt).groups())
            kern = "k_rx_frames" if "k_rx_frames" in d_ else "k_rx"
            cfg = next(c for c, a in STATIC.items() if f"<{a}," in d_)
            keys = ("instr", "valu", "valu_issue")
            out.setdefault(cfg, {})[kern] = {"kernel": dict(zip(keys, whole)), "loop": dict(zip(keys, max(loops)))}
    for c in out.values():
        c["added_valu"] = c["k_rx_frames"]["kernel"]["valu"] - c["k_rx"]["kernel"]["valu"]
        c["added_instr"] = c["k_rx_frames"]["kernel"]["instr"] - c["k_rx"]["kernel"]["instr"]
        c["valu_cost"] = c["added_valu"] / c["k_rx"]["loop"]["valu"]
    return out


def report(static, measured):
    """profiles/frames_ab.txt: the static expectation, the measured A/B, and each measured receiver cost
    against its static estimate and the spread of the unchanged column."""
    print("# tools/frames_ab.py: the per-frame record (ofdm_rx_frames, a frame per symbol) against ofdm_rx, complex128")
    print("# static (tools/isa_mix.py): the VALU k_rx_frames adds to k_rx (kernel totals; all of it inside the symbol loop,")
    print("# the branch a symbol with errors takes included) against the VALU of k_rx's symbol loop, per lane and symbol")
    for c, v in sorted(static.items()):
        a, b = v["k_rx"], v["k_rx_frames"]
        print(f"static config {c}: kernel instructions {a['kernel']['instr']} -> {b['kernel']['instr']} (+{v['added_instr']}), "
              f"VALU {a['kernel']['valu']} -> {b['kernel']['valu']} (+{v['added_valu']}); k_rx symbol loop "
              f"{a['loop']['instr']} instructions, {a['loop']['valu']} VALU: estimate {100 * v['valu_cost']:+.2f} %")
    print(f"# measured on {measured['device']}: {measured['cases'][0]['steps']} alternating steps each after the warm-up; "
          "medians, iqr in brackets, ms")
    for m in measured["cases"]:
        est = static[m["config"]]["valu_cost"]
        over = m["rx_cost"] - est
        noise = m["rx_spread_of_unchanged"]
        verdict = ("within the static estimate plus the unchanged column's spread" if over <= noise else
                   f"{100 * (over - noise):.2f} points above the static estimate plus the unchanged column's spread")
        print(f"config {m['config']} at {m['snr_db']} dB, {m['n_sym']} symbols, {100 * m['symbols_with_errors']:.1f} % of them "
              f"with errors: ofdm_rx {m['ofdm_rx_ms']['median']:.3f} [{m['ofdm_rx_ms']['iqr']:.3f}] -> ofdm_rx_frames "
              f"{m['ofdm_rx_frames_ms']['median']:.3f} [{m['ofdm_rx_frames_ms']['iqr']:.3f}] = {100 * m['rx_cost']:+.2f} % "
              f"(static {100 * est:+.2f} %, spread of ofdm_rx {100 * noise:.2f} %: {verdict}); step "
              f"{m['step_ms']['median']:.3f} [{m['step_ms']['iqr']:.3f}] -> {m['step_frames_ms']['median']:.3f} "
              f"[{m['step_frames_ms']['iqr']:.3f}] = {100 * m['step_cost']:+.2f} %")


def step(eng, n, snr, seed, frames):
    """(receiver event ms, step wall ms, bit errors, symbols with errors or None) of one run."""
    import torch

    ev = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = eng.run(n, snr, seed=seed, fused=False, events=ev, **({"frame_symbols": 1} if frames else {}))
    wall = (time.perf_counter() - t0) * 1e3
    name = "ofdm_rx_frames" if frames else "ofdm_rx"
    rx = sum(e0.elapsed_time(e1) for k, _, e0, e1 in ev if k == name)
    hit = int(np.count_nonzero(res.frames.bit_errors)) if frames else None
    if frames:
        assert int(res.frames.bit_errors.sum()) == res.bit_errors
    return rx, wall, res.bit_errors, hit


def summary(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


def case(name, snr, n, steps, warmup):
    import bench

    cfg = bench.CONFIGS[name]
    eng = bench.make_engine(cfg, "f64")
    snr = cfg[5] if snr is None else snr
    eng.reserve(n, 1)
    for k in range(warmup):
        step(eng, n, snr, 100 + k, False)
        step(eng, n, snr, 100 + k, True)
    rows = {False: [], True: []}
    for k in range(steps):
        for frames in ((False, True) if k % 2 == 0 else (True, False)):   # alternate which goes first
            rows[frames].append(step(eng, n, snr, 1000 + k, frames))
    assert [r[2] for r in rows[False]] == [r[2] for r in rows[True]]      # the same counts, seed by seed
    a_rx, b_rx = summary([r[0] for r in rows[False]]), summary([r[0] for r in rows[True]])
    a_st, b_st = summary([r[1] for r in rows[False]]), summary([r[1] for r in rows[True]])
    return {"config": name, "snr_db": snr, "n_fft": eng.n_fft, "n_sym": n, "steps": steps,
            "symbols_with_errors": float(np.mean([r[3] for r in rows[True]])) / n,
            "ofdm_rx_ms": a_rx, "ofdm_rx_frames_ms": b_rx, "step_ms": a_st, "step_frames_ms": b_st,
            "rx_cost": b_rx["median"] / a_rx["median"] - 1.0, "step_cost": b_st["median"] / a_st["median"] - 1.0,
            "rx_spread_of_unchanged": a_rx["iqr"] / a_rx["median"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--static", metavar="JSON", default=None, help="write the static instruction counts (no GPU) and stop")
    ap.add_argument("--report", nargs=2, metavar=("STATIC_JSON", "MEASURED_JSON"), default=None,
                    help="print the text report of the two files and stop")
    args = ap.parse_args()
    if args.static:
        with open(args.static, "w") as f:
            json.dump(static_counts(), f, indent=1)
            f.write("\n")
        return
    if args.report:
        report(json.load(open(args.report[0])), json.load(open(args.report[1])))
        return
    import torch

    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "precision": "complex128", "cases": []}
    for name, snr, n in CASES:
        c = case(name, snr, n, args.steps, args.warmup)
        res["cases"].append(c)
        print(f"config {c['config']} at {c['snr_db']} dB, {c['n_sym']} symbols ({100 * c['symbols_with_errors']:.1f} % "
              f"with errors): ofdm_rx {c['ofdm_rx_ms']['median']:.3f} ms (iqr {c['ofdm_rx_ms']['iqr']:.3f}), "
              f"ofdm_rx_frames {c['ofdm_rx_frames_ms']['median']:.3f} ms (iqr {c['ofdm_rx_frames_ms']['iqr']:.3f}): "
              f"{100 * c['rx_cost']:+.2f} %; step {c['step_ms']['median']:.3f} -> {c['step_frames_ms']['median']:.3f} ms: "
              f"{100 * c['step_cost']:+.2f} %", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

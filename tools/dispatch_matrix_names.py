#!/usr/bin/env python3
"""Write profiles/dispatch_matrix_kernels.txt and profiles/dispatch_matrix_gpu_tests.txt from one
traced run of tests/test_gpu_dispatch_matrix.py:

    rocprofv3 --kernel-trace --stats -d OUT -o matrix --output-format csv -- \\
        python -m pytest tests/test_gpu_dispatch_matrix.py -m gpu -v -s -p no:cacheprovider > OUT/pytest.txt 2>&1
    python tools/dispatch_matrix_names.py OUT/matrix_kernel_stats.csv OUT/pytest.txt

(a kernel trace only -- no counters).  tests/test_dispatch_model.py holds the names file against the
dispatch model, so re-record it when the launch rules or the case tables change on purpose.
"""

import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(stats_csv, pytest_txt):
    names = set()
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            m = re.search(r"(k_tx|k_rx)<[^<>]*>", row["Name"])
            if m:
                names.add(m.group(0))
    with open(os.path.join(ROOT, "profiles", "dispatch_matrix_kernels.txt"), "w") as f:
        f.write("# distinct fused-kernel names of a rocprofv3 --kernel-trace --stats run of "
                "tests/test_gpu_dispatch_matrix.py on an MI355X\n"
                "# k_tx: R, LOGN, FB, LT, ZPW, REF, WIDE   k_rx: R, LOGN, EQ, FB, MV, REF, WIDE\n")
        f.write("\n".join(sorted(names)) + "\n")
    out = []
    with open(pytest_txt) as f:
        for line in f:
            # the profiler's own log lines, and pytest's description of the machine
            line = re.sub(r" ?[WEI]\d{8} \d\d:\d\d:\d\d\.\d+ \d+ \S+\] .*$", "", line.rstrip("\n"))
            if not re.match(r"(platform |rootdir:|plugins:|hypothesis profile|cachedir:)", line):
                out.append(line)
    with open(os.path.join(ROOT, "profiles", "dispatch_matrix_gpu_tests.txt"), "w") as f:
        f.write("# pytest tests/test_gpu_dispatch_matrix.py -m gpu -v -s on an MI355X, under rocprofv3 "
                "--kernel-trace --stats\n" + "\n".join(out).strip() + "\n")
    print(f"{len(names)} kernel names, {sum('bracket' in s for s in out)} bracket lines")


if __name__ == "__main__":
    main(*sys.argv[1:3])

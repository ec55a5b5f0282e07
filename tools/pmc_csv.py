#!/usr/bin/env python3
"""Per-kernel averages of every counter in rocprofv3 --pmc --output-format csv results (one row per dispatch and counter).
usage: pmc_csv.py <kernel-regex> file_counter_collection.csv [...]      (kernels are grouped by what the regex matches of their name)"""
import csv
import re
import sys
from collections import defaultdict


def main(pattern, paths):
    acc = defaultdict(list)
    for p in paths:
        with open(p) as f:
            for row in csv.DictReader(f):
                m = re.search(pattern, row["Kernel_Name"])
                if m:
                    acc[(m.group(0), row["Counter_Name"])].append(float(row["Counter_Value"]))
    for (k, c), v in sorted(acc.items()):
        print("%-45s %-22s n=%3d avg=%16.1f min=%16.1f max=%16.1f" % (k, c, len(v), sum(v) / len(v), min(v), max(v)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])

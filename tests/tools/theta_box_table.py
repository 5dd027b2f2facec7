#!/usr/bin/env python3
"""The tables of profiles/theta_box.md from the output of ``pytest -s -m gpu tests/test_theta_box_gpu.py``: the lines
``theta_box <model> <path> <quantity>: err .. E64 .. ratio ..`` that ``theta_box_model.report`` prints.

    python tests/tools/theta_box_table.py LOG > tables.md
"""
import collections
import re
import sys

LINE = re.compile(r"theta_box (\S+) (\S+) (\S+): err (\S+) E64 (\S+) ratio (\S+)")
COLUMNS = ("lml", "grad", "var", "V")


def parse(path):
    cells = collections.OrderedDict()
    for line in open(path):
        m = LINE.search(line)
        if m and m[3] in COLUMNS:
            cells.setdefault((m[1], m[2]), {})[m[3]] = (float(m[4]), float(m[5]), float(m[6]))
    return cells


def main(path):
    cells = parse(path)
    worst = collections.defaultdict(dict)
    for (model, p), row in cells.items():
        for q, (err, e64, ratio) in row.items():
            if ratio > worst[p].get(q, (0.0, ""))[0]:
                worst[p][q] = (ratio, model)
    print("### Worst ratio per path\n")
    print("| path | " + " | ".join(COLUMNS) + " |")
    print("|---|" + "---|" * len(COLUMNS))
    for p in sorted(worst):
        print(f"| {p} | " + " | ".join(f"{worst[p][q][0]:.2f} ({worst[p][q][1]})" if q in worst[p] else "" for q in COLUMNS) + " |")
    print("\n### Every model and path: device error / E64 (ratio)\n")
    print("| model | path | " + " | ".join(COLUMNS) + " |")
    print("|---|---|" + "---|" * len(COLUMNS))
    for (model, p), row in cells.items():
        if p == "batch_latency":            # the bits of `lml`, asserted
            continue
        print(f"| {model} | {p} | " + " | ".join(f"{row[q][0]:.1e} / {row[q][1]:.1e} ({row[q][2]:.2f})" if q in row else ""
                                                 for q in COLUMNS) + " |")


if __name__ == "__main__":
    main(sys.argv[1])

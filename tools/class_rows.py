#!/usr/bin/env python3
"""Pseudo-row counts of the tables that keep a class record (csrc/gk_classrows.h), from the lines that
``GK_TRACE=class_bound`` leaves on stderr:

    GK_TRACE=class_bound python bench.py --gpus 1 --steps 1 --warmup 0 2> trace.txt; python tools/class_rows.py trace.txt

Per distinct table: rows, columns, classes, pseudo-rows (one per set bit of a class's weight), the padded pseudo-rows the
bound runs over, their share of the rows, the bound classes x ceil(log2(max weight + 1)) and the route that was taken."""
import re
import sys

PAT = re.compile(r"\[class_bound\] rows (\d+) cols (\d+) classes (\d+) pseudo_rows (\d+) padded (\d+) weight_bits (\d+) route (\w+)")


def main(path):
    seen = {}
    for line in open(path, errors="replace"):
        m = PAT.search(line)
        if m:
            key = tuple(int(x) for x in m.groups()[:6]) + (m.group(7),)
            seen[key] = seen.get(key, 0) + 1
    print(f"{'rows':>9} {'cols':>5} {'classes':>8} {'pseudo':>8} {'padded':>8} {'padded/rows':>11} {'bound':>9} {'pseudo/bound':>12} route  (times seen)")
    tot = [0, 0, 0, 0]
    for (rows, cols, classes, pseudo, padded, bits, route), n in sorted(seen.items(), key=lambda kv: -kv[0][0]):
        bound = min(rows, classes * bits)
        print(f"{rows:9d} {cols:5d} {classes:8d} {pseudo:8d} {padded:8d} {padded / rows:11.3f} {bound:9d} {pseudo / max(bound, 1):12.3f} {route}  ({n})")
        for k, v in enumerate((rows, classes, pseudo, padded)):
            tot[k] += v
    if seen:
        print(f"all distinct tables: rows {tot[0]}, classes {tot[1]}, pseudo-rows {tot[2]}, padded {tot[3]} = {tot[3] / tot[0]:.3f} of the rows")


if __name__ == "__main__":
    main(sys.argv[1])

"""Time the read bootstrap of the copy-number stage next to the depth of the sample on one synthetic sample (needs the GPU).

    python tools/time_cn_bootstrap.py --pairs 10000000 --boot 100

The sample is ``bench.build_inputs(seed, pairs)`` (configs[2]: 10 M pairs, configs[1]: 1 M), in HBM as its compact words
(what the command line holds when ``--cn-bootstrap`` runs).  After ``--warmup`` untimed rounds, ``--repeats`` timed rounds of
``cn_bootstrap.bootstrapGeneDepths`` with ``--boot`` replicates -- the point estimate and every replicate: the draws
(``gk_boot_row_counts``), ``gk_depth_weighted`` and the host side -- host clock around a call that ends in a stream wait,
medians reported.  The per-kernel times are the library's own event spans (``gk_prof``), per round: the draw
(``callboot_draw``), the marking (``depthw_mark``), the scan's kernels, ``depthw_finish`` and ``depthw_select``.  The
yardstick is ``gk_depth_compact`` on the same sample, card and process (HIP events around the whole call): it marks every
mate of the sample once, a round of the bootstrap marks it about 0.63 x ``--boot`` + 1 times (the share of pairs a replicate
draws at least once).  One JSON line per statistic on stdout."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--boot", type=int, default=100)
    ap.add_argument("--select", default="p75", help="comma-separated: p75, mean, median")
    ap.add_argument("--exon", action="store_true", help="statistics over the exons only (--cn-exon)")
    ap.add_argument("--seed", type=int, default=1031, help="seed of the synthetic sample")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import numpy as np

    import bench
    from kir_graph_amd import _lib
    from kir_graph_amd.cn_bootstrap import bootstrapGeneDepths
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.packed import CompactMates

    sidx, gidx, sample, rec, table = bench.build_inputs(args.seed, args.pairs)
    dev = _lib.Device(0)
    tab = Tabulation(DeviceIndex(dev, gidx), CompactMates(rec, threads=4), dev=dev)
    data = SampleData(tab, gidx, tab.novelVariants(table.strings))
    gene_len = {g: len(sidx.backbone[g]) for g in sidx.genes}

    # the yardstick: the depth of the whole sample from the same compact words
    lens = np.array([gene_len[g] for g in gidx.genes], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    depth = np.zeros(int(off[-1]), dtype=np.uint32)
    depth_ms = []
    for k in range(args.warmup + args.repeats):
        dev.sync()
        dev.timerStart()
        _lib.check(_lib.lib().gk_depth_compact(dev.ctx, tab.handle, tab.mates.words.ptr, 0, off.ctypes.data, len(lens),
                                               depth.ctypes.data))
        ms = dev.timerStopMs()
        if k >= args.warmup:
            depth_ms.append(round(ms, 4))
    depth_bases = int(depth.astype(np.int64).sum())

    for mode in args.select.split(","):
        made = {}

        def round_():
            made["boot"] = bootstrapGeneDepths(data, gene_len, args.boot, select_mode=mode,
                                               regions=sidx.exons if args.exon else None)
        for _ in range(args.warmup):
            round_()
        dev.sync()
        dev.profEnable(True)
        dev.profCollect()
        wall = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            round_()
            dev.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
        prof = dev.profCollect()
        dev.profEnable(False)
        spans = {k: round(ms / args.repeats, 4) for k, (n, ms) in sorted(prof.items())}
        launches = {k: n // args.repeats for k, (n, ms) in sorted(prof.items())}
        boot = made["boot"]
        scan = sum(v for k, v in spans.items() if k in ("scan_tiles", "add_tile_offsets"))
        print(json.dumps({
            "tool": "time_cn_bootstrap", "pairs": args.pairs, "valid_pairs": int(tab.n_valid), "records": "compact",
            "replicates": args.boot, "select_mode": mode, "exon": bool(args.exon), "genes": len(lens), "positions": int(off[-1]),
            "warmup": args.warmup, "repeats": args.repeats,
            "bootstrap_ms": round(statistics.median(wall), 3), "bootstrap_ms_all": [round(w, 3) for w in wall],
            "draw_ms": spans.get("callboot_draw", 0.0), "mark_ms": spans.get("depthw_mark", 0.0), "scan_ms": round(scan, 4),
            "finish_ms": spans.get("depthw_finish", 0.0), "select_ms": spans.get("depthw_select", 0.0),
            "spans_ms": spans, "launches": launches,
            "gk_depth_compact_ms": statistics.median(depth_ms), "gk_depth_compact_ms_all": depth_ms,
            "gk_depth_compact_bases": depth_bases,
            "mark_over_depth_per_replicate": round(spans.get("depthw_mark", 0.0) / (args.boot + 1) / statistics.median(depth_ms), 3),
            "point": [float(x) for x in boot.point],
            "replicate_sd_over_point": [round(float(s / p), 5) if p else None
                                        for s, p in zip(boot.replicates.std(axis=0, ddof=1) if args.boot > 1 else boot.point * 0,
                                                        boot.point)],
        }), flush=True)


if __name__ == "__main__":
    main()

"""Time the EM read bootstrap next to the point EM on one synthetic sample (needs the GPU).

    python tools/time_em_bootstrap.py --pairs 10000000 --boot 100

The sample is ``bench.build_inputs(seed, pairs)`` (configs[2]: 10 M pairs, configs[1]: 1 M).  After ``--warmup`` untimed
rounds, ``--repeats`` timed rounds of (a) ``TypingWithReport.typing`` -- the point EM of every gene, ``gk_sample_em`` --
and (b) one ``gk_em_bootstrap`` call for the same genes; host clock around calls that end in a stream wait, medians
reported.  The per-kernel times are the library's own event spans (``gk_prof``), per call.  The yardstick of the batched
solver is ``boot`` x the point EM's ``em_kernel_genes`` time: what ``boot`` separate EM launches would take.  One JSON
line on stdout."""
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
    ap.add_argument("--seed", type=int, default=1031, help="seed of the synthetic sample")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    import bench
    from kir_graph_amd import _lib
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.kir_typing import TypingWithReport, _GeneView
    from kir_graph_amd.typing_em import bootstrapEM, candidateSetsDistinct

    sidx, gidx, sample, rec, table = bench.build_inputs(args.seed, args.pairs)
    dev = _lib.Device(0)
    tab0 = Tabulation(DeviceIndex(dev, gidx), rec)
    data = SampleData(tab0, gidx, tab0.novelVariants(table.strings))
    typer = TypingWithReport(data)
    tab = typer._context()[0]            # the lane's context: every call below runs on its stream
    todo = [(g, int(cn)) for g, cn in sample.gene_cn.items() if cn]
    jobs = []
    for gene, _ in todo:
        v = _GeneView(data, gene, multiple=False, tab=tab)
        if v.g is None or not v.alleles or not v.n_rows:
            continue
        sets, count = candidateSetsDistinct(tab, v.rows, v.n_rows, v.vbeg, v.vbeg + v.n_span, v.mask, gidx.tables[v.g].words)
        jobs.append((sets, count, len(v.alleles), v.g))
    reads = sum(int(j[1].sum()) for j in jobs)

    def timed(call):
        for _ in range(args.warmup):
            call()
        tab.dev.sync()
        tab.dev.profEnable(True)
        tab.dev.profCollect()
        wall = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            call()
            tab.dev.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
        prof = {k: ms / args.repeats for k, (n, ms) in tab.dev.profCollect().items()}
        tab.dev.profEnable(False)
        return statistics.median(wall), [round(w, 3) for w in wall], prof

    point_ms, point_all, point_prof = timed(lambda: typer.typing(sample.gene_cn))
    boot_ms, boot_all, boot_prof = timed(lambda: bootstrapEM(tab, jobs, args.boot, 2022))
    both = TypingWithReport(data, bootstrap=args.boot)
    both_ms, both_all, _ = timed(lambda: both.typing(sample.gene_cn))
    em_ms = point_prof.get("em_kernel_genes", float("nan"))
    draw_ms, batch_ms = boot_prof.get("boot_resample", float("nan")), boot_prof.get("boot_em_batch", float("nan"))
    print(json.dumps({
        "tool": "time_em_bootstrap", "pairs": args.pairs, "boot": args.boot, "genes": len(jobs), "reads": reads,
        "distinct_sets": sum(len(j[1]) for j in jobs), "max_sets_per_gene": max((len(j[1]) for j in jobs), default=0),
        "alleles": sum(j[2] for j in jobs), "warmup": args.warmup, "repeats": args.repeats,
        "point_typing_ms": round(point_ms, 3), "point_typing_ms_all": point_all,
        "point_kernels_ms": {k: round(v, 4) for k, v in sorted(point_prof.items())},
        "bootstrap_call_ms": round(boot_ms, 3), "bootstrap_call_ms_all": boot_all,
        "bootstrap_kernels_ms": {k: round(v, 4) for k, v in sorted(boot_prof.items())},
        "typing_with_bootstrap_ms": round(both_ms, 3), "typing_with_bootstrap_ms_all": both_all,
        "yardstick_boot_x_em_kernel_genes_ms": round(args.boot * em_ms, 3),
        "boot_em_batch_over_yardstick": round(batch_ms / (args.boot * em_ms), 4),
        "draws_per_s": round(args.boot * reads / (draw_ms * 1e-3), 1),
        "resample_share_of_bootstrap_kernels": round(draw_ms / (draw_ms + batch_ms), 4),
    }))


if __name__ == "__main__":
    main()

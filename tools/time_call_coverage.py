"""Time the per-allele coverage of the likelihood strategies next to the typing itself on one synthetic sample (needs the GPU).

    python tools/time_call_coverage.py --pairs 10000000

The sample is ``bench.build_inputs(seed, pairs)`` (configs[2]: 10 M pairs, configs[1]: 1 M), in HBM as its compact words
(what the command line keeps with ``--call-coverage``).  Per strategy (``full``, ``exonfirst``), after ``--warmup`` untimed
rounds, ``--repeats`` timed rounds of (a) ``TypingWithPosNegAllele.typing`` without the flag, (b) ``call_coverage.coverCall``
for every typed gene of that result -- the whole report of the sample: ``gk_call_coverage`` and the host side per gene --
and (c) the typing with ``call_coverage=True``; host clock around calls that end in a stream wait, medians reported.  The
per-kernel times are the library's own event spans (``gk_prof``), per round: the marking kernel (``callcov_mark_lds`` where
a gene's track fits the LDS, else ``callcov_mark``), the scan's kernels and ``callcov_finish``; (b) is then timed again with
``GK_CALLCOV=direct``, which makes ``callcov_mark`` mark every gene.  The yardstick of the marking is ``gk_depth_compact``
on the same sample, card and process (HIP events around the whole call: it marks every mate of the sample once, the report
marks the rows of every gene's model once per track they count in).  One JSON line per strategy on stdout."""
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
    ap.add_argument("--strategies", default="full,exonfirst")
    ap.add_argument("--seed", type=int, default=1031, help="seed of the synthetic sample")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import numpy as np

    import bench
    from kir_graph_amd import _lib
    from kir_graph_amd.call_report import modelOf
    from kir_graph_amd.call_coverage import coverCall
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.kir_typing import TypingWithPosNegAllele
    from kir_graph_amd.packed import CompactMates

    sidx, gidx, sample, rec, table = bench.build_inputs(args.seed, args.pairs)
    dev = _lib.Device(0)
    tab0 = Tabulation(DeviceIndex(dev, gidx), CompactMates(rec, threads=4), dev=dev)
    data = SampleData(tab0, gidx, tab0.novelVariants(table.strings))
    gene_len = {g: len(sidx.backbone[g]) for g in sidx.genes}

    # the yardstick: the depth of the whole sample from the same compact words
    lens = np.array([gene_len[g] for g in gidx.genes], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    depth = np.zeros(int(off[-1]), dtype=np.uint32)
    depth_ms = []
    for k in range(args.warmup + args.repeats):
        dev.sync()
        dev.timerStart()
        _lib.check(_lib.lib().gk_depth_compact(dev.ctx, tab0.handle, tab0.mates.words.ptr, 0, off.ctypes.data, len(lens),
                                               depth.ctypes.data))
        ms = dev.timerStopMs()
        if k >= args.warmup:
            depth_ms.append(round(ms, 4))
    depth_bases = int(depth.astype(np.int64).sum())

    for strategy in args.strategies.split(","):
        kw = {"exon_first": True, "exon_candidate_threshold": 1.0} if strategy == "exonfirst" else {}
        typer = TypingWithPosNegAllele(data, top_n=600, variant_correction=True, **kw)
        lane = typer._context()[0].dev       # the lane's context: every call below runs on its stream

        def timed(call):
            for _ in range(args.warmup):
                call()
            lane.sync()
            lane.profEnable(True)
            lane.profCollect()
            wall = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                call()
                lane.sync()
                wall.append((time.perf_counter() - t0) * 1e3)
            prof = {k: ms / args.repeats for k, (n, ms) in lane.profCollect().items()}
            lane.profEnable(False)
            return statistics.median(wall), [round(w, 3) for w in wall], prof

        point_ms, point_all, _ = timed(lambda: typer.typing(sample.gene_cn))
        genes = [(gene, steps[-1]) for gene, steps in typer._result.items() if steps and not steps[-1].isFail()]
        made: dict = {}

        def report():
            for gene, res in genes:
                g = gidx.gene_id[gene]
                made[gene] = coverCall(res, gene_len[gene], gidx.exons.get(gene, []), gidx.tables[g])
        cov_ms, cov_all, cov_prof = timed(report)
        os.environ["GK_CALLCOV"] = "direct"            # the direct form of the marking, forced (read at every call)
        try:
            direct_ms, direct_all, direct_prof = timed(report)
        finally:
            del os.environ["GK_CALLCOV"]
        both = TypingWithPosNegAllele(data, top_n=600, variant_correction=True, call_coverage=True, call_coverage_len=gene_len,
                                      **kw)
        both_ms, both_all, _ = timed(lambda: both.typing(sample.gene_cn))

        rows, tracks, marked = [], 0, 0
        for gene, res in genes:
            model, c = modelOf(res), made.get(gene)
            if model is None or c is None:
                continue
            rows.append(int(model.n_rows))
            tracks += len(c.depth)
            marked += int(c.bases[0].sum())          # bases over every track = what the marks add up to
        mark = sum(v for k, v in cov_prof.items() if k.startswith("callcov_mark"))
        rest = {k: round(v, 4) for k, v in sorted(cov_prof.items()) if not k.startswith("callcov_mark")}
        print(json.dumps({
            "tool": "time_call_coverage", "strategy": strategy, "pairs": args.pairs, "records": "compact",
            "genes": len(genes), "reports": sum(c is not None for c in made.values()), "rows": sum(rows),
            "max_rows_per_gene": max(rows, default=0), "tracks": tracks, "bases_marked": marked,
            "warmup": args.warmup, "repeats": args.repeats,
            "point_typing_ms": round(point_ms, 3), "point_typing_ms_all": point_all,
            "coverage_ms": round(cov_ms, 3), "coverage_ms_all": cov_all,
            "mark_spans_ms": {k: round(v, 4) for k, v in sorted(cov_prof.items()) if k.startswith("callcov_mark")},
            "mark_ms": round(mark, 4), "scan_and_finish_spans_ms": rest,
            "coverage_direct_ms": round(direct_ms, 3), "coverage_direct_ms_all": direct_all,
            "mark_direct_spans_ms": {k: round(v, 4) for k, v in sorted(direct_prof.items()) if k.startswith("callcov_mark")},
            "typing_with_coverage_ms": round(both_ms, 3), "typing_with_coverage_ms_all": both_all,
            "gk_depth_compact_ms": statistics.median(depth_ms), "gk_depth_compact_ms_all": depth_ms,
            "gk_depth_compact_valid_pairs": int(tab0.n_valid), "gk_depth_compact_bases": depth_bases,
            "mark_over_depth": round(mark / statistics.median(depth_ms), 3),
        }), flush=True)


if __name__ == "__main__":
    main()

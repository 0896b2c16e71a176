"""Time the copy-dosage report: its kernel next to the fit report's on one synthetic table, and the whole report next to the
typing itself on one synthetic sample (needs the GPU).

    python tools/time_call_dosage.py table --rows 1000000,10000000 --called 2,4 --columns 600
    python tools/time_call_dosage.py sample --pairs 10000000

``table``: per number of rows a ``uint8`` table ``[columns][ldm]`` is put in HBM once -- ``--values gene``: 0 with probability
17 / 20, else 1 .. 3, the few-pattern shape of a gene's reads; ``--values drawn``: the table of tools/time_call_alternatives.py
(0 .. 3, 17 and 255), hundreds of patterns at K = 4 -- drawn for 37 columns and repeated.  Per number of called columns K,
after ``--warmup`` untimed rounds, ``--repeats`` rounds of ``gk_call_patterns`` (``calldosage_patterns``) and of the yardstick,
``gk_call_fit`` without ``d_min`` (``callfit_profile``), which reads the same K columns of the same table.  Kernel times are
the library's own event spans (``gk_prof``), per round; ``*_call_ms`` is the host clock around the library call, which waits
for its result; ``solver_ms`` is ``solveDosage`` on the patterns found.  Both kernels read ``K R`` bytes.

``sample``: the sample is ``bench.build_inputs(seed, pairs)`` (configs[2]: 10 M pairs).  Per strategy, (a) the typing without
the flag, (b) ``call_dosage.dosageOfCall`` for every typed gene of that result -- the whole report of the sample -- and
(c) the typing with ``call_dosage=True``; the patterns seen per gene.  One JSON line per (rows, K) or strategy on stdout."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL, YARDSTICK = "calldosage_patterns", "callfit_profile"


def timed(dev, call, warmup: int, repeats: int):
    for _ in range(warmup):
        call()
    dev.sync()
    dev.profEnable(True)
    dev.profCollect()
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        dev.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
    prof = {name: ms / repeats for name, (n, ms) in dev.profCollect().items() if n}
    dev.profEnable(False)
    return statistics.median(wall), [round(w, 3) for w in wall], prof


def tableMode(args) -> None:
    import numpy as np

    from kir_graph_amd import _lib
    from kir_graph_amd.call_dosage import patternsOfColumns, solveDosage
    from kir_graph_amd.call_fit import profileColumns

    dev = _lib.Device(0)
    a = args.columns
    levels = np.array([0] * 17 + [1, 2, 3] if args.values == "gene" else [0, 0, 0, 0, 0, 1, 1, 2, 3, 17, 255], dtype=np.uint8)
    for n_rows in (int(x) for x in args.rows.split(",")):
        rng = np.random.default_rng(args.seed)
        ldm = (n_rows + 63) // 64 * 64
        base = np.zeros((37, ldm), dtype=np.uint8)
        base[:, :n_rows] = rng.choice(levels, (37, n_rows))
        miss8 = dev.put(base[np.arange(a) % 37])
        del base
        for k in (int(x) for x in args.called.split(",")):
            cols = (np.arange(k, dtype=np.int32) * 7 + 1) % a           # distinct columns of the drawn 37
            got = {}

            def patterns():
                got["patterns"] = patternsOfColumns(dev, miss8, ldm, n_rows, a, cols)

            def fit():
                got["fit"] = profileColumns(dev, miss8, ldm, n_rows, a, cols, want_min=False)

            pat_ms, _, pat_prof = timed(dev, patterns, args.warmup, args.repeats)
            fit_ms, _, fit_prof = timed(dev, fit, args.warmup, args.repeats)
            pats, counts, oor = got["patterns"]
            hist = got["fit"][0]
            assert int(counts.sum()) + oor == n_rows and oor == int(hist[17])      # the two agree where they overlap
            t0 = time.perf_counter()
            sol = solveDosage(pats, counts, [1] * k) if len(counts) else None
            solver_ms = (time.perf_counter() - t0) * 1e3
            span, yard = pat_prof.get(KERNEL, float("nan")), fit_prof.get(YARDSTICK, float("nan"))
            print(json.dumps({
                "tool": "time_call_dosage", "mode": "table", "values": args.values, "rows": n_rows, "columns": a, "called": k,
                "warmup": args.warmup, "repeats": args.repeats, "patterns": len(counts), "out_of_range": oor,
                "kernels_ms": {KERNEL: round(span, 4), YARDSTICK: round(yard, 4)},
                "kernel_bytes": k * n_rows,
                "kernel_gb_per_s": {KERNEL: round(k * n_rows / span / 1e6, 1), YARDSTICK: round(k * n_rows / yard / 1e6, 1)},
                "patterns_over_profile": round(span / yard, 3),
                "patterns_call_ms": round(pat_ms, 3), "fit_call_ms": round(fit_ms, 3),
                "solver_ms": round(solver_ms, 3), "solver_passes": sol.iterations if sol else None,
            }), flush=True)
        miss8.free()
    dev.close()


def sampleMode(args) -> None:
    import bench
    from kir_graph_amd import _lib
    from kir_graph_amd.call_dosage import dosageOfCall
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.kir_typing import TypingWithPosNegAllele

    sidx, gidx, sample, rec, table = bench.build_inputs(args.seed, args.pairs)
    dev = _lib.Device(0)
    tab0 = Tabulation(DeviceIndex(dev, gidx), rec)
    data = SampleData(tab0, gidx, tab0.novelVariants(table.strings))
    for strategy in args.strategies.split(","):
        kw = {"exon_first": True, "exon_candidate_threshold": 1.0} if strategy == "exonfirst" else {}
        typer = TypingWithPosNegAllele(data, top_n=600, variant_correction=True, **kw)
        lane = typer._context()[0].dev       # the lane's context: every call below runs on its stream
        point_ms, point_all, _ = timed(lane, lambda: typer.typing(sample.gene_cn), args.warmup, args.repeats)
        genes = [(gene, steps[-1]) for gene, steps in typer._result.items() if steps and not steps[-1].isFail()]
        made: dict = {}

        def report():
            for gene, res in genes:
                made[gene] = dosageOfCall(res, names=gidx.tables[gidx.gene_id[gene]].alleles)
        rep_ms, rep_all, rep_prof = timed(lane, report, args.warmup, args.repeats)
        both = TypingWithPosNegAllele(data, top_n=600, variant_correction=True, call_dosage=True, **kw)
        both_ms, both_all, _ = timed(lane, lambda: both.typing(sample.gene_cn), args.warmup, args.repeats)
        done = {g: d for g, d in made.items() if d is not None}
        print(json.dumps({
            "tool": "time_call_dosage", "mode": "sample", "strategy": strategy, "pairs": args.pairs, "genes": len(genes),
            "reports": len(done), "rows": sum(d.reads for d in done.values()),
            "max_rows_per_gene": max((d.reads for d in done.values()), default=0),
            "warmup": args.warmup, "repeats": args.repeats,
            "point_typing_ms": round(point_ms, 3), "point_typing_ms_all": point_all,
            "dosage_ms": round(rep_ms, 3), "dosage_ms_all": rep_all,
            "dosage_kernel_ms": round(rep_prof.get(KERNEL, float("nan")), 4),
            "typing_with_dosage_ms": round(both_ms, 3), "typing_with_dosage_ms_all": both_all,
            "patterns": {g: len(d.counts) for g, d in done.items()},
            "called_alleles": {g: len(d.alleles) for g, d in done.items()},
            "passes": {g: d.iterations for g, d in done.items()},
            "dosage": {g: [round(a.dosage, 4) if a.dosage is not None else None for a in d.alleles] for g, d in done.items()},
        }), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("table", "sample"))
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--called", default="2,4")
    ap.add_argument("--columns", type=int, default=600)
    ap.add_argument("--values", choices=("gene", "drawn"), default="gene")
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--strategies", default="full,exonfirst")
    ap.add_argument("--seed", type=int, default=1031)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    (tableMode if args.mode == "table" else sampleMode)(args)


if __name__ == "__main__":
    main()

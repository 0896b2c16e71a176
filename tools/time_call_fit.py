"""Time the fit report of the likelihood strategies next to the typing itself on one synthetic sample (needs the GPU).

    python tools/time_call_fit.py --pairs 10000000 --extra 3

The sample is ``bench.build_inputs(seed, pairs)`` (configs[2]: 10 M pairs, configs[1]: 1 M).  Per strategy (``full``,
``exonfirst``), after ``--warmup`` untimed rounds, ``--repeats`` timed rounds of (a) ``TypingWithPosNegAllele.typing`` without
the flag, (b) ``call_fit.fitCall`` for every typed gene of that result -- the whole report of the sample: ``gk_call_fit``,
``gk_call_fit_extra`` and the host side per gene -- and (c) the typing with ``call_fit=True``; host clock around calls that
end in a stream wait, medians reported.  The per-kernel times are the library's own event spans (``gk_prof``), per round.
Bytes per second of a kernel: the bytes its shapes say it moves over the genes of the sample -- ``callfit_profile``
``(K + 1) R`` (K called columns read, ``d_min`` written), ``callfit_extra`` ``(A + ceil(A / 16)) R`` (every column of the table
read once, ``d_min`` once per workgroup column tile) -- over its span.  One JSON line per strategy on stdout."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("callfit_profile", "callfit_extra")
EXTRA_TILE = 16      # kExtraCols of csrc/gk_callfit.hip


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--extra", type=int, default=3)
    ap.add_argument("--strategies", default="full,exonfirst")
    ap.add_argument("--seed", type=int, default=1031, help="seed of the synthetic sample")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import numpy as np

    import bench
    from kir_graph_amd import _lib
    from kir_graph_amd.call_report import modelOf
    from kir_graph_amd.call_fit import fitCall
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
                made[gene] = fitCall(res, args.extra, names=gidx.tables[gidx.gene_id[gene]].alleles)
        fit_ms, fit_all, fit_prof = timed(report)
        both = TypingWithPosNegAllele(data, top_n=600, variant_correction=True, call_fit=True, call_fit_extra=args.extra, **kw)
        both_ms, both_all, _ = timed(lambda: both.typing(sample.gene_cn))

        # the bytes the two kernels move over the sample's genes, from the shapes
        rows, profile_bytes, extra_bytes, table_cols = [], 0, 0, 0
        for gene, res in genes:
            model = modelOf(res)
            if model is None or made.get(gene) is None:
                continue
            r = int(model.n_rows)
            k = len(np.unique(np.asarray(res.allele_id)[res.bestRank()]))
            a = model.n_allele if model.tableColumns is None else len(model.tableColumns)
            rows.append(r)
            table_cols += a
            profile_bytes += (k + (1 if args.extra > 0 else 0)) * r
            extra_bytes += (a + -(-a // EXTRA_TILE)) * r if args.extra > 0 else 0
        spans = {k: fit_prof.get(k, float("nan")) for k in KERNELS}
        print(json.dumps({
            "tool": "time_call_fit", "strategy": strategy, "pairs": args.pairs, "extra": args.extra,
            "genes": len(genes), "reports": sum(f is not None for f in made.values()), "rows": sum(rows),
            "max_rows_per_gene": max(rows, default=0), "table_columns": table_cols,
            "warmup": args.warmup, "repeats": args.repeats,
            "point_typing_ms": round(point_ms, 3), "point_typing_ms_all": point_all,
            "fit_ms": round(fit_ms, 3), "fit_ms_all": fit_all,
            "fit_kernels_ms": {k: round(v, 4) for k, v in spans.items()},
            "fit_kernel_bytes": {"callfit_profile": profile_bytes, "callfit_extra": extra_bytes},
            "fit_kernel_gb_per_s": {"callfit_profile": round(profile_bytes / spans["callfit_profile"] / 1e6, 1),
                                    "callfit_extra": round(extra_bytes / spans["callfit_extra"] / 1e6, 1)},
            "other_spans_ms": {k: round(v, 4) for k, v in sorted(fit_prof.items()) if k not in KERNELS},
            "typing_with_fit_ms": round(both_ms, 3), "typing_with_fit_ms_all": both_all,
            "mismatches": {g: f.mismatches for g, f in made.items() if f is not None},
            "largest_gain": {g: (f.extra[0][1] if f.extra else 0) for g, f in made.items() if f is not None},
        }), flush=True)


if __name__ == "__main__":
    main()

"""Time the call bootstrap of the likelihood strategies next to the typing itself on one synthetic sample (needs the GPU).

    python tools/time_call_bootstrap.py --pairs 10000000 --boot 100 --top 32

The sample is ``bench.build_inputs(seed, pairs)`` (configs[2]: 10 M pairs, configs[1]: 1 M).  Per strategy (``full``,
``exonfirst``), after ``--warmup`` untimed rounds, ``--repeats`` timed rounds of (a) ``TypingWithPosNegAllele.typing`` without
the flag, (b) ``call_bootstrap.bootstrapCall`` for every typed gene of that result -- the whole bootstrap of the sample:
``gk_setmax``, ``gk_boot_row_counts``, ``gk_weighted_sums`` and the host summary per gene -- and (c) the typing with
``call_bootstrap=boot``; host clock around calls that end in a stream wait, medians reported.  The per-kernel times are the
library's own event spans (``gk_prof``), per round.  One JSON line per strategy on stdout."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("setmax_kernel", "callboot_draw", "callboot_sums", "callboot_fold")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--boot", type=int, default=100)
    ap.add_argument("--top", type=int, default=32)
    ap.add_argument("--strategies", default="full,exonfirst")
    ap.add_argument("--seed", type=int, default=1031, help="seed of the synthetic sample")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import bench
    from kir_graph_amd import _lib
    from kir_graph_amd.call_bootstrap import bootstrapCall, homoFactor
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

        def bootstrap():
            for gene, res in genes:
                made[gene] = bootstrapCall(res, homoFactor(res), args.boot, 2022, gidx.gene_id[gene], args.top)
        boot_ms, boot_all, boot_prof = timed(bootstrap)
        both = TypingWithPosNegAllele(data, top_n=600, variant_correction=True, call_bootstrap=args.boot,
                                      call_bootstrap_top=args.top, **kw)
        both_ms, both_all, _ = timed(lambda: both.typing(sample.gene_cn))
        rows = [int(modelRows(res)) for _, res in genes]
        print(json.dumps({
            "tool": "time_call_bootstrap", "strategy": strategy, "pairs": args.pairs, "boot": args.boot, "top": args.top,
            "genes": len(genes), "rows": sum(rows), "max_rows_per_gene": max(rows, default=0),
            "candidate_sets": sum(len(b.rows) for b in made.values() if b is not None),
            "warmup": args.warmup, "repeats": args.repeats,
            "point_typing_ms": round(point_ms, 3), "point_typing_ms_all": point_all,
            "bootstrap_ms": round(boot_ms, 3), "bootstrap_ms_all": boot_all,
            "bootstrap_kernels_ms": {k: round(boot_prof.get(k, float("nan")), 4) for k in KERNELS},
            "other_spans_ms": {k: round(v, 4) for k, v in sorted(boot_prof.items()) if k not in KERNELS},
            "typing_with_bootstrap_ms": round(both_ms, 3), "typing_with_bootstrap_ms_all": both_all,
            "min_call_support": min((b.call_support for b in made.values() if b is not None), default=None),
        }), flush=True)


def modelRows(result) -> int:
    from kir_graph_amd.call_report import modelOf
    model = modelOf(result)
    return model.n_rows if model is not None else 0


if __name__ == "__main__":
    main()

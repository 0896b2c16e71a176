"""Time the two kernels of the call alternatives next to the two of the fit report on one synthetic table (needs the GPU).

    python tools/time_call_alternatives.py --rows 1000000,10000000 --called 2,4 --columns 600

Per number of rows a ``uint8`` table ``[columns][ldm]`` is put in HBM once (values 0 .. 3 with a few large ones and some 255,
drawn for 37 columns and repeated: the kernels' work does not depend on the values).  Per number of called columns K,
after ``--warmup`` untimed rounds, ``--repeats`` rounds of ``gk_call_swap`` (``callswap_rows`` + ``callswap_sums``) and of the
yardstick on the same table and columns, ``gk_call_fit`` + ``gk_call_fit_extra`` (``callfit_profile`` + ``callfit_extra``),
which read the same bytes once.  Kernel times are the library's own event spans (``gk_prof``), per round; ``*_call_ms`` is
the host clock around the library calls, which wait for their result.  Bytes by the shapes, R rows, A columns, T = the tile
of ``callswap_sums`` (32 / KT, at most 16): ``callswap_rows`` ``(K + 3) R``, ``callswap_sums`` ``(A + 3 ceil(A / T)) R``,
``callfit_profile`` ``(K + 1) R``, ``callfit_extra`` ``(A + ceil(A / 16)) R``.  One JSON line per (rows, K) on stdout."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWAP = ("callswap_rows", "callswap_sums")
FIT = ("callfit_profile", "callfit_extra")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--called", default="2,4")
    ap.add_argument("--columns", type=int, default=600)
    ap.add_argument("--seed", type=int, default=1031)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import numpy as np

    from kir_graph_amd import _lib
    from kir_graph_amd.call_alternatives import swapSums
    from kir_graph_amd.call_fit import extraSums, profileColumns

    dev = _lib.Device(0)
    a = args.columns
    for n_rows in (int(x) for x in args.rows.split(",")):
        rng = np.random.default_rng(args.seed)
        ldm = (n_rows + 63) // 64 * 64
        base = np.zeros((37, ldm), dtype=np.uint8)
        base[:, :n_rows] = rng.choice(np.array([0, 0, 0, 0, 0, 1, 1, 2, 3, 17, 255], dtype=np.uint8), (37, n_rows))
        miss8 = dev.put(base[np.arange(a) % 37])
        del base
        for k in (int(x) for x in args.called.split(",")):
            cols = (np.arange(k, dtype=np.int32) * 7 + 1) % a           # distinct columns of the drawn 37
            kt = next(t for t in (1, 2, 4, 8, 16) if k <= t)
            tile = min(16, 32 // kt)

            def timed(call):
                for _ in range(args.warmup):
                    call()
                dev.sync()
                dev.profEnable(True)
                dev.profCollect()
                wall = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    call()
                    wall.append((time.perf_counter() - t0) * 1e3)
                prof = {name: ms / args.repeats for name, (n, ms) in dev.profCollect().items() if n}
                dev.profEnable(False)
                return statistics.median(wall), prof

            got = {}

            def swap():
                got["swap"] = swapSums(dev, miss8, ldm, n_rows, a, cols)

            def fit():
                hist, per_col, m, d_min = profileColumns(dev, miss8, ldm, n_rows, a, cols, want_min=True)
                try:
                    got["fit"] = (m, extraSums(dev, miss8, ldm, n_rows, a, d_min))
                finally:
                    d_min.free()

            swap_ms, swap_prof = timed(swap)
            fit_ms, fit_prof = timed(fit)
            loss, rows_for, gain, against, m, beyond = got["swap"]
            assert m == got["fit"][0] and np.array_equal(gain, m - got["fit"][1])      # the two agree where they overlap
            spans = {name: swap_prof.get(name, float("nan")) for name in SWAP}
            spans.update({name: fit_prof.get(name, float("nan")) for name in FIT})
            nbytes = {"callswap_rows": (k + 3) * n_rows, "callswap_sums": (a + 3 * -(-a // tile)) * n_rows,
                      "callfit_profile": (k + 1) * n_rows, "callfit_extra": (a + -(-a // 16)) * n_rows}
            swap_total, fit_total = sum(spans[n] for n in SWAP), sum(spans[n] for n in FIT)
            print(json.dumps({
                "tool": "time_call_alternatives", "rows": n_rows, "columns": a, "called": k, "tile": tile,
                "warmup": args.warmup, "repeats": args.repeats,
                "kernels_ms": {n: round(v, 4) for n, v in spans.items()},
                "kernel_bytes": nbytes,
                "kernel_gb_per_s": {n: round(nbytes[n] / spans[n] / 1e6, 1) for n in spans},
                "swap_kernels_ms": round(swap_total, 4), "fit_kernels_ms": round(fit_total, 4),
                "swap_over_fit": round(swap_total / fit_total, 3),
                "sums_over_extra": round(spans["callswap_sums"] / spans["callfit_extra"], 3),
                "sums_over_k_plus_1_extras": round(spans["callswap_sums"] / ((k + 1) * spans["callfit_extra"]), 3),
                "swap_call_ms": round(swap_ms, 3), "fit_calls_ms": round(fit_ms, 3),
                "mismatches": m, "out_of_range": beyond,
            }), flush=True)
        miss8.free()
    dev.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev tool: how many rows of a gene's compatibility table are distinct.
  python tools/dup_rows.py [pairs, default 10000000] [--lists]

Default: the classes the library itself forms (``gk_row_classes``, csrc/gk_rowclass.hip) -- rows of equal KEPT (id, sign)
sequence after the error correction -- per gene, for the full and for the exon preparation of a ``bench.py`` sample, with
the time the class stage takes next to it.
--lists: the older estimate on the host, pairs of a gene that share their four id lists as tabulated (no correction)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                            # noqa: E402
from kir_graph_amd import _lib                          # noqa: E402
from kir_graph_amd._lib import DeviceSlice, check, lib  # noqa: E402
from kir_graph_amd.engine import DeviceIndex, Tabulation   # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
pairs = int(args[0]) if args else 10_000_000
dev = _lib.Device(0)
sidx, gidx, by_gene = bench.build_index()
t = time.time()
sample, rec, table = bench.build_sample(sidx, gidx, by_gene, 1031, pairs)
print(f"sample of {pairs} pairs in {time.time() - t:.1f}s", flush=True)
dindex = DeviceIndex(dev, gidx)
mates = dev.put(rec)
tab = Tabulation(dindex, mates, dev=dev)
n = tab.n_valid


def kept_classes():
    for exon in (False, True):
        prep = tab.prepared(dev, exon=exon)
        tot_r = tot_c = 0
        tot_t = 0.0
        print(f"{'exon' if exon else 'full'} preparation: rows with a kept id {int(prep.off[-1])} of {n} pairs", flush=True)
        for g in range(len(gidx.genes)):
            a, b = int(prep.off[g]), int(prep.off[g + 1])
            if b == a:
                continue
            rows = DeviceSlice(prep.rows, a, b - a, dev)
            n_cls = C.c_int64()
            best = None
            for _ in range(3):      # the call waits for the stream: its wall time is the class stage + one fetch
                dev.sync()
                t0 = time.perf_counter()
                check(lib().gk_row_classes(dev.ctx, tab.handle, rows.ptr, b - a, prep.vflag.ptr, 0, C.byref(n_cls)))
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            print(f"  gene {g:2d} {gidx.genes[g]:10s} rows {b - a:8d} classes {n_cls.value:8d} ({n_cls.value / (b - a):.3f}); "
                  f"class stage {1e3 * best:.3f} ms", flush=True)
            tot_r += b - a
            tot_c += n_cls.value
            tot_t += best
        print(f"  all genes: rows {tot_r}, classes {tot_c} ({tot_c / max(tot_r, 1):.3f}); class stages {1e3 * tot_t:.2f} ms", flush=True)


def equal_lists():
    off = tab.offsets().astype(np.int64)
    ids = tab.ids().astype(np.uint64)
    gene = tab.pairGene()
    nh = tab.pairNH()
    print(f"valid {n}, ids {len(ids)} ({len(ids) / n:.1f} per pair)", flush=True)
    # an order-independent hash per list (lists are sorted), the four lists mixed with different multipliers
    h = (ids + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    csum = np.concatenate([[np.uint64(0)], np.cumsum(h, dtype=np.uint64)])
    per_list = csum[off[1:]] - csum[off[:-1]]               # [4 * n]
    per_list = per_list.reshape(n, 4)
    lens = np.diff(off).reshape(n, 4).astype(np.uint64)
    key = np.zeros(n, dtype=np.uint64)
    for q, m in enumerate((0x94D049BB133111EB, 0xD6E8FEB86659FD93, 0xA0761D6478BD642F, 0xE7037ED1A0B428DB)):
        key += (per_list[:, q] + lens[:, q] * np.uint64(0x632BE59BD9B4E019)) * np.uint64(m)
    tot_r = tot_d = 0
    for g in range(len(gidx.genes)):
        sel = (gene == g) & (nh == 1)
        k = key[sel]
        if not len(k):
            continue
        u, c = np.unique(k, return_counts=True)
        top = np.sort(c)[::-1]
        print(f"gene {g:2d} {gidx.genes[g]:10s} rows {len(k):8d} distinct {len(u):8d} ({len(u) / len(k):.3f}); "
              f"largest classes {top[:4].tolist()}; rows in classes >= 2: {int(c[c >= 2].sum()) / len(k):.3f}", flush=True)
        tot_r += len(k)
        tot_d += len(u)
    print(f"all genes: rows {tot_r}, distinct {tot_d} ({tot_d / tot_r:.3f})")


if "--lists" in sys.argv:
    equal_lists()
else:
    kept_classes()

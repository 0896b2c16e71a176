"""``gk_sample_prepare_exon_from``: the exon model's preparation with its first tally read out of the full model's counts
(``cnt[v] = full[v]`` where the incoming drop flag is clear, 0 where it is set) must write what ``gk_sample_prepare_exon``
writes after walking every list itself -- drop flags, tallies, rows, gene offsets, surviving lists -- and both must equal
the two correction passes done on the CPU (``compat_reference.tally`` / ``correctionFlags``)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from compat_reference import correctionFlags, tally  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def synthetic(device):
    """bench.build_inputs(7, 3000): (index, device index, records), made once."""
    sys.path.insert(0, ROOT)
    import bench
    from kir_graph_amd.engine import DeviceIndex
    sidx, gidx, sample, rec, table = bench.build_inputs(7, 3000)
    rec.setflags(write=False)
    dindex = DeviceIndex(device, gidx)
    yield gidx, dindex, rec
    dindex.close()


def exonFlags(gidx, tab) -> np.ndarray:
    flags = np.full(max(tab.n_var_total, 1), 3, dtype=np.uint8)           # novel variants are never in an exon
    flags[:gidx.n_variant][gidx.in_exon.astype(bool)] = 0
    return flags


def prepareFull(dev, tab, multiple: bool):
    """gk_sample_prepare: (tallies of the uncorrected lists, on the device)."""
    from kir_graph_amd._lib import check, lib
    nv = max(tab.n_var_total, 1)
    vflag, cnt, rows = dev.alloc(nv, np.uint8), dev.alloc(2 * nv, np.uint32), dev.alloc(max(tab.n_valid, 1), np.int32)
    off = np.zeros(len(tab.dindex.host.genes) + 1, dtype=np.int64)
    check(lib().gk_sample_prepare(dev.ctx, tab.handle, int(multiple), vflag.ptr, cnt.ptr, rows.ptr, off.ctypes.data))
    vflag.free()
    rows.free()
    return cnt


def prepareExon(dev, tab, multiple: bool, flags: np.ndarray, cnt_full=None) -> dict:
    """Every output of the exon preparation: the old entry, or -- with the full model's tallies -- the new one."""
    from kir_graph_amd._lib import check, lib
    nv = max(tab.n_var_total, 1)
    vflag, cnt, rows = dev.put(flags), dev.alloc(2 * nv, np.uint32), dev.alloc(max(tab.n_valid, 1), np.int32)
    rows.zero()
    off = np.zeros(len(tab.dindex.host.genes) + 1, dtype=np.int64)
    o, p, q = (np.zeros(nv, dtype=t) for t in (np.int32, np.uint32, np.uint32))
    n = C.c_int64()
    args = (dev.ctx, tab.handle, int(multiple), vflag.ptr, cnt.ptr, rows.ptr, off.ctypes.data, nv, o.ctypes.data,
            p.ctypes.data, q.ctypes.data, C.byref(n))
    if cnt_full is None:
        check(lib().gk_sample_prepare_exon(*args))
    else:
        check(lib().gk_sample_prepare_exon_from(*args, cnt_full.ptr))
    out = {"vflag": vflag.download(), "cnt": cnt.download(), "rows": rows.download()[:int(off[-1])], "off": off,
           "ord": o[:n.value], "pos": p[:n.value], "neg": q[:n.value]}
    for b in (vflag, cnt, rows):
        b.free()
    return out


def cpuExon(tab, multiple: bool, flags: np.ndarray) -> dict:
    """The two correction passes of the exon model on the host."""
    off, ids, gene, nh = tab.offsets(), tab.ids(), tab.pairGene(), tab.pairNH()
    nv = max(tab.n_var_total, 1)
    rows = np.flatnonzero((nh == 1) | bool(multiple))
    flags = flags.copy()
    for _ in range(2):
        pos, neg = tally(off, ids, rows, flags, nv)
        flags |= correctionFlags(pos, neg)
    alive = []
    for r in rows:
        p, q = ids[off[4 * r]:off[4 * r + 2]], ids[off[4 * r + 2]:off[4 * r + 4]]
        alive.append(bool(((flags[p] & 1) == 0).any() or ((flags[q] & 2) == 0).any()))
    kept = rows[np.array(alive, dtype=bool)] if len(rows) else rows
    order = np.argsort(gene[kept], kind="stable")
    n_gene = len(tab.dindex.host.genes)
    survive = np.flatnonzero((((flags & 1) == 0) & (pos > 0)) | (((flags & 2) == 0) & (neg > 0)))
    return {"vflag": flags, "cnt": np.concatenate([pos, neg]), "rows": kept[order].astype(np.int32),
            "off": np.searchsorted(gene[kept][order], np.arange(n_gene + 1)).astype(np.int64), "ord": survive.astype(np.int32),
            "pos": np.where(flags[survive] & 1, 0, pos[survive]).astype(np.uint32),
            "neg": np.where(flags[survive] & 2, 0, neg[survive]).astype(np.uint32)}


def assertSame(a: dict, b: dict, what=""):
    for k in ("vflag", "cnt", "rows", "off", "ord", "pos", "neg"):
        assert np.array_equal(a[k], b[k]), (what, k)


def tabulated(device, dindex, rec):
    from kir_graph_amd.engine import Tabulation
    return Tabulation(dindex, np.ascontiguousarray(rec), dev=device)


CASES = ("sample", "no exon id", "no valid pair", "a gene without rows")


@pytest.mark.parametrize("multiple", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_shared_tallies_give_the_outputs_of_the_walk(device, synthetic, case, multiple):
    gidx, dindex, src = synthetic
    rec = src
    if case == "no valid pair":
        rec = src[:800].copy()
        rec["flag"] &= ~np.uint16(2)
    elif case == "a gene without rows":
        gene = int(np.bincount(src["ref"]).argmax())
        rec = src[np.repeat(src["ref"][::2] != gene, 2)]
    tab = tabulated(device, dindex, rec)
    flags = exonFlags(gidx, tab)
    if case == "no exon id":
        flags[:] = 3
    elif case == "sample":
        assert tab.n_novel > 0 and (flags[gidx.n_variant:] == 3).all()      # novel variants: flags 3 on entry
    assert (tab.n_valid == 0) == (case == "no valid pair")
    full = prepareFull(device, tab, multiple)
    walked = prepareExon(device, tab, multiple, flags)
    shared = prepareExon(device, tab, multiple, flags, cnt_full=full)
    assertSame(walked, shared, "walked against shared")
    assertSame(cpuExon(tab, multiple, flags), shared, "host against shared")
    if case in ("sample", "a gene without rows"):
        assert len(shared["rows"]) > 0 and len(shared["ord"]) > 0 and shared["cnt"].sum() > 0
        assert (shared["vflag"][flags == 0] != 0).any()                       # the correction dropped ids inside the exons
    else:
        assert len(shared["rows"]) == 0 and shared["cnt"].sum() == 0
    if case == "a gene without rows":
        assert shared["off"][gene] == shared["off"][gene + 1]
    if case == "sample" and not multiple:
        assert len(shared["rows"]) < len(prepareExon(device, tab, True, flags, cnt_full=prepareFull(device, tab, True))["rows"])
    full.free()
    tab.mates.free()
    tab.close()


def test_prepared_takes_the_full_tallies_when_they_are_there(device, synthetic):
    """``Tabulation.prepared(exon=True)`` before any full preparation walks the lists itself (two tallies); after the full
    preparation of the same ``multiple`` it reads that one's counts (one tally) -- with the same result."""
    gidx, dindex, rec = synthetic
    device.profEnable(True)
    device.profCollect()
    got = []
    for full_first in (False, True):
        tab = tabulated(device, dindex, rec)
        device.profCollect()
        if full_first:
            tab.prepared(device, False)
            tab.prepared(device, True)                  # another `multiple`: not the tallies of the exon model's rows
        prep = tab.prepared(device, False, exon=True)
        prof = device.profCollect()
        walks, masks = prof.get("count_ids_genes", (0, 0))[0], prof.get("mask_tallies", (0, 0))[0]
        assert (walks, masks) == ((3, 1) if full_first else (2, 0))
        n = int(prep.off[-1])
        got.append({"vflag": prep.vflag.download(), "cnt": prep.cnt.download(), "rows": prep.rows.download()[:n],
                    "off": prep.off, "ord": prep.surviving.ordinals, "pos": prep.surviving.pos, "neg": prep.surviving.neg})
        tab.mates.free()
        tab.close()
    device.profEnable(False)
    assertSame(got[0], got[1])

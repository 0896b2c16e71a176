"""Who gives a pool block back (csrc/gk_blocks.h), checked on the real entry points by failure injection: the test-only
``gk_test_pool_fail`` makes the n-th allocation from the pool fail as if the device were out of memory.  Every entry point
that takes device scratch is run clean (twice: M = the allocations of the second run, the outputs), then once per
n = 1 .. M with allocation n failing: the call returns an error with a message, the context has as many blocks out as
before the call, and the same call with nothing armed gives the clean run's bytes.  The failure is an error return of a
host allocator: nothing faults and no kernel sees it.

``TAKES`` declares M per entry point, because the cases are made when the tests are collected; the clean run checks it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kir_graph_amd import _lib, packed, synth
from kir_graph_amd._lib import check, lib
from kir_graph_amd.engine import DeviceIndex, LogTable, Tabulation
from kir_graph_amd.hisat2 import pairLines
from kir_graph_amd.index import GkIndex

sys.path.insert(0, os.path.dirname(__file__))
import emsets_reference as er      # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20261020
BEYOND = 1 << 40      # an n-th allocation no run reaches: arms the counting only


def hook(ctx, nth):
    """Arm (0: disarm); (blocks of the context that are out, allocations counted since the call before)."""
    live, count = C.c_int64(), C.c_int64()
    check(lib().gk_test_pool_fail(ctx, nth, C.byref(live), C.byref(count)))
    return live.value, count.value


def toy(n_rows, n_allele, n_var, seed):
    """Hand-built lists: per row four disjoint ascending lists of 0 .. 2 of ``n_var`` variants, and the alleles' bit rows."""
    rng = np.random.default_rng(seed)
    lists = []
    for _ in range(n_rows):
        perm = rng.permutation(n_var)
        lens = rng.integers(0, 3, size=4)
        cuts = np.concatenate([[0], np.cumsum(lens)])
        lists.append([sorted(perm[cuts[k]:cuts[k + 1]].tolist()) for k in range(4)])
    off, ids = er.packLists(lists)
    bits = rng.random((n_var, n_allele)) < 0.5
    return off, ids, bits


class FromCsr:
    """A tabulation made by ``gk_tab_from_csr`` with its rows, drop flags and bit rows on the device."""

    def __init__(self, dev, n_rows, n_allele, n_var, seed):
        self.dev, self.n_rows, self.n_allele, self.n_var = dev, n_rows, n_allele, n_var
        self.off, self.ids, self.bits = toy(n_rows, n_allele, n_var, seed)
        self.gene, self.nh = np.zeros(n_rows, np.uint8), np.ones(n_rows, np.uint8)
        self.tab = self.make()
        self.rows = dev.put(np.arange(n_rows, dtype=np.int32))
        self.vflag = dev.alloc(n_var, np.uint8).zero()
        self.ldm = (n_rows + 63) // 64 * 64

    def create(self, out):
        return lib().gk_tab_from_csr(self.dev.ctx, self.n_var, self.n_rows, self.off.ctypes.data, self.ids.ctypes.data,
                                     self.gene.ctypes.data, self.nh.ctypes.data, C.byref(out))

    def make(self):
        h = C.c_void_p()
        check(self.create(h))
        return h

    def args(self, n_allele):
        """The leading arguments of the compatibility calls for the gene's first ``n_allele`` alleles."""
        mask = self.dev.put(er.pack(self.bits[:, :n_allele], 1))
        self.keep = getattr(self, "keep", []) + [mask]
        return (self.dev.ctx, self.tab, self.rows.ptr, self.n_rows, self.vflag.ptr, 0, self.n_var, mask.ptr, 1, n_allele, 1)


def tab_arrays(dev, h):
    """Everything a tabulation holds on the device, then the tabulation is destroyed."""
    info = _lib.TabInfo()
    check(lib().gk_tab_get_info(h, C.byref(info)))
    nv, ni = int(info.n_valid), int(info.n_ids)
    out = [np.array([info.n_pairs, nv, ni, info.n_novel, info.err_flags], dtype=np.int64),
           dev.view(info.d_off, 4 * nv + 1, np.uint32), dev.view(info.d_ids, ni, np.uint32),
           dev.view(info.d_pair_gene, nv, np.uint8), dev.view(info.d_pair_nh, nv, np.uint8)]
    if info.d_pair_src:
        out.append(dev.view(info.d_pair_src, nv, np.int32))
    if info.d_novel_key:
        out.append(dev.view(info.d_novel_key, int(info.n_novel), np.uint64))
    lib().gk_tab_destroy(h)
    return out


class World:
    """The inputs of every entry point, made once with nothing armed."""

    def __init__(self, dev):
        self.dev, ctx = dev, dev.ctx
        L = lib()
        sidx = synth.makeIndex(seed=7, n_genes=2, len_range=(4200, 4600), var_range=(10, 10), allele_range=(5, 5))
        self.gidx = gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
        sample = synth.makeSample(sidx, seed=11, n_pairs=64, gene_cn={g: 2 for g in sidx.genes})
        lines = synth.toSamLines(sample)
        self.n_pairs = 64
        rec, _ = packed.packPairs(pairLines(lines), gidx, spill=[])
        pure = [p for p in range(64) if all(l.split("\t")[5][:-1].isdigit() for l in lines[2 * p:2 * p + 2])]
        spill: list = []
        rec_w, _ = packed.packPairs(pairLines(synth.withManyMismatches(lines, sidx, pure[:2], np.random.default_rng(3))), gidx,
                                    spill=spill)
        self.wide, self.which = packed.spillArrays(spill)
        assert len(self.which) == 2 and len(rec) == len(rec_w) == 128
        self.key = np.ascontiguousarray(gidx.key, dtype=np.uint64)
        self.vbeg = np.ascontiguousarray(gidx.gene_vbeg, dtype=np.int32)
        self.dindex = DeviceIndex(dev, gidx)
        self.tab = Tabulation(self.dindex, rec)
        self.mates_w = dev.put(rec_w)
        self.gene_off = np.concatenate([[0], np.cumsum([len(sidx.backbone[g]) for g in sidx.genes])]).astype(np.int64)
        # the rows of gene 0 (this builds the row partition, so that later calls find it), their tallies
        tab = self.tab
        self.nv = nv = max(tab.n_var_total, 1)
        self.rows, self.n = tab.selectGene(0)
        assert self.n > 8
        self.vflag = dev.alloc(nv, np.uint8).zero()
        self.cnt = dev.alloc(2 * nv, np.uint32).zero()
        tab.countVariants(self.rows, self.n, self.vflag, self.cnt)
        self.exon_flags = np.full(nv, 3, dtype=np.uint8)
        self.exon_flags[:gidx.n_variant][gidx.in_exon.astype(bool)] = 0
        # hand-built lists: 48 rows x 8 alleles (the tables of 5 take its first five), 32 rows x 4 alleles, 8 rows
        self.logs = LogTable(dev)
        self.c48 = FromCsr(dev, 48, 8, 12, SEED)
        self.c32 = FromCsr(dev, 32, 4, 12, SEED + 1)
        self.c8 = FromCsr(dev, 8, 4, 12, SEED + 2)
        self.mask4 = dev.put(er.pack(self.c32.bits, 1))
        self.sets32 = dev.alloc((32, 1), np.uint32)
        check(L.gk_em_sets(ctx, self.c32.tab, self.c32.rows.ptr, 32, 0, 12, self.mask4.ptr, 1, self.sets32.ptr))
        self.uniq = np.array([[1], [2], [3], [12]], dtype=np.uint32)
        self.mult = np.array([5, 3, 2, 7], dtype=np.uint32)
        # replicate weights, a mismatch table, the minima of a fit and the groups of a novel assignment
        rng = np.random.default_rng(SEED)
        self.ldw = (tab.n_valid + 63) // 64 * 64
        self.W = dev.alloc((3, self.ldw), np.uint32).zero()
        check(L.gk_boot_row_counts(ctx, tab.n_valid, 3, 0, SEED, 1, self.W.ptr, self.ldw))
        self.W100 = dev.alloc((4, 128), np.uint32).zero()
        check(L.gk_boot_row_counts(ctx, 100, 4, 0, SEED, 1, self.W100.ptr, 128))
        self.V = dev.put(rng.random((3, 128)))
        self.ldm = (self.n + 63) // 64 * 64
        self.miss8 = dev.put(rng.integers(0, 4, size=(3, self.ldm), dtype=np.uint8))
        self.fit_cols = np.array([0, 2], dtype=np.int32)
        self.d_min = dev.alloc(self.ldm, np.uint8).zero()
        check(self.call_fit(np.zeros(18, np.uint64), np.zeros(6, np.uint64), np.zeros(1, np.uint64)))
        self.probs = dev.put(rng.choice([0.5, 0.25], size=(2, self.n)))
        self.entries = np.array([1, 2], dtype=np.uint32)
        self.code = dev.alloc(self.n, np.uint16).zero()
        check(self.novel_assign(np.zeros(self.n, np.uint16), np.zeros(4, np.uint32), np.zeros(4, np.int32)))
        t = gidx.tables[0]
        self.span = (int(t.vbeg), int(t.vend))
        self.carry = dev.put(rng.integers(0, 4, size=max(t.vend - t.vbeg, 1)).astype(np.uint32))
        dev.sync()

    def call_fit(self, hist, col, m):
        return lib().gk_call_fit(self.dev.ctx, self.miss8.ptr, self.ldm, self.n, 3, self.fit_cols.ctypes.data, 2,
                                 hist.ctypes.data, col.ctypes.data, m.ctypes.data, self.d_min.ptr)

    def novel_assign(self, code, count, first):
        return lib().gk_novel_assign(self.dev.ctx, self.probs.ptr, self.n, 2, self.entries.ctypes.data, 2, self.code.ptr,
                                     code.ctypes.data, count.ctypes.data, first.ctypes.data)


# ---------------------------------------------------------------------------------------------------------- entry points
# A scenario is a function of the world that returns `call`: `call()` runs the entry point once and returns (return code,
# finish), where `finish()` -- run with nothing armed, after a success -- gives the outputs as arrays and releases what
# the call created.  Buffers that a scenario needs are made before `call` is returned, so that the armed window holds the
# entry point alone.  Optional attributes of `call`: `before()` makes, with nothing armed, what every call needs afresh and
# `discard()` releases it after a call that failed; `settle()` runs once after the first clean run.
def s_index_create(w):
    def call():
        h = C.c_void_p()
        rc = lib().gk_index_create(w.dev.ctx, w.key.ctypes.data, len(w.key), w.vbeg.ctypes.data, len(w.gidx.genes), C.byref(h))
        assert (rc == 0) == bool(h.value)

        def finish():      # what the index holds shows in a tabulation made with it
            t = C.c_void_p()
            check(lib().gk_tabulate(w.dev.ctx, h, w.tab.mates.ptr, w.n_pairs, C.byref(t)))
            out = tab_arrays(w.dev, t)
            lib().gk_index_destroy(h)
            return out
        return rc, finish
    return call


def s_tabulate(wide):
    def make(w):
        def call():
            h = C.c_void_p()
            if wide:
                rc = lib().gk_tabulate_spilled(w.dev.ctx, w.dindex.handle, w.mates_w.ptr, w.n_pairs, 0, 0, w.wide.ctypes.data,
                                               w.which.ctypes.data, len(w.which), C.byref(h))
            else:
                rc = lib().gk_tabulate_spilled(w.dev.ctx, w.dindex.handle, w.tab.mates.ptr, w.n_pairs, 0, 0, None, None, 0,
                                               C.byref(h))
            assert (rc == 0) == bool(h.value)
            return rc, lambda: tab_arrays(w.dev, h)
        return call
    return make


def s_tab_from_csr(w):
    def call():
        h = C.c_void_p()
        rc = w.c8.create(h)
        assert (rc == 0) == bool(h.value)
        return rc, lambda: tab_arrays(w.dev, h)
    return call


def s_select_gene_first_use(w):
    """The row partition of a tabulation is built by the first call that asks for it: a fresh tabulation per call."""
    rows = w.dev.alloc(8, np.int32).zero()
    made = []

    def call():
        n = C.c_int64()
        rc = lib().gk_select_gene(w.dev.ctx, made[-1], 0, 0, rows.ptr, C.byref(n))

        def finish():
            out = [np.array([n.value]), rows.download()]
            call.discard()
            return out
        return rc, finish
    call.before = lambda: made.append(w.c8.make())      # with nothing armed
    call.discard = lambda: lib().gk_tab_destroy(made.pop())
    return call


def s_mates_compact(w):
    def call():
        p, nbytes = C.c_uint64(), C.c_int64()
        rc = lib().gk_mates_compact(w.dev.ctx, w.tab.mates.ptr, 2 * w.n_pairs, C.byref(p), C.byref(nbytes))

        def finish():
            out = [w.dev.view(p.value, nbytes.value // 4, np.uint32)]
            lib().gk_free(w.dev.ctx, p.value)
            return out
        return rc, finish
    return call


def s_prepare(exon):
    def make(w):
        dev, nv, n_gene = w.dev, w.nv, len(w.gidx.genes)
        cnt, rows = dev.alloc(2 * nv, np.uint32), dev.alloc(max(w.tab.n_valid, 1), np.int32)
        vflag = dev.alloc(nv, np.uint8)
        off = np.zeros(n_gene + 1, dtype=np.int64)
        o, p, q = (np.zeros(nv, dtype=t) for t in (np.int32, np.uint32, np.uint32))
        keys = np.zeros(max(w.tab.n_novel, 1), dtype=np.uint64)

        def call():
            n_surv = C.c_int64()
            vflag.upload(w.exon_flags) if exon else vflag.zero()
            args = (dev.ctx, w.tab.handle, 0, vflag.ptr, cnt.ptr, rows.ptr, off.ctypes.data, nv, o.ctypes.data, p.ctypes.data,
                    q.ctypes.data, C.byref(n_surv))
            rc = lib().gk_sample_prepare_exon(*args) if exon else lib().gk_sample_prepare_all(*args, keys.ctypes.data)
            k = n_surv.value
            return rc, lambda: [off.copy(), np.array([k]), o[:k].copy(), p[:k].copy(), q[:k].copy(), keys.copy(),
                                vflag.download(), cnt.download(), rows.download(int(off[-1]))]
        return call
    return make


def s_variant_surviving(w):
    o, p, q = (np.zeros(w.nv, dtype=t) for t in (np.int32, np.uint32, np.uint32))

    def call():
        n = C.c_int64()
        rc = lib().gk_variant_surviving(w.dev.ctx, w.tab.handle, w.cnt.ptr, w.vflag.ptr, w.nv, o.ctypes.data, p.ctypes.data,
                                        q.ctypes.data, C.byref(n))
        return rc, lambda: [np.array([n.value]), o[:n.value].copy(), p[:n.value].copy(), q[:n.value].copy()]
    return call


def s_select_nonempty(w):
    rows = w.dev.alloc(w.n, np.int32).zero()

    def call():
        n = C.c_int64()
        rc = lib().gk_select_nonempty(w.dev.ctx, w.tab.handle, w.rows.ptr, w.n, w.vflag.ptr, rows.ptr, C.byref(n))
        return rc, lambda: [np.array([n.value]), rows.download(n.value)]
    return call


def s_compat(form):
    """``gk_compat_log_miss`` of 48 rows x 5 alleles: plain, by row classes, for a column list; the index form; and the
    narrow kernels for a list of 8 columns."""
    def make(w):
        c, dev = w.c48, w.dev
        n_cols = {"cols": 3, "narrow": 8}.get(form, 5)
        args = c.args(8 if form == "narrow" else 5)
        cols = np.array([0, 2, 4] if form == "cols" else range(8), dtype=np.int32)
        L = dev.alloc((n_cols, c.n_rows), np.float64).zero()
        lidx = dev.alloc((n_cols, c.ldm), np.uint16).zero()
        miss8 = dev.alloc((n_cols, c.ldm), np.uint8).zero()
        flags, msum = dev.alloc(1, np.uint32).zero(), dev.alloc(n_cols, np.uint32).zero()

        def call():
            os.environ.pop("GK_TEST_HOOKS", None)
            if form == "plain":
                rc = lib().gk_compat_log_miss(*args, w.logs.handle, L.ptr, miss8.ptr, c.ldm, flags.ptr)
            elif form == "row_classes":
                os.environ["GK_TEST_HOOKS"] = "row_classes=on"
                try:
                    rc = lib().gk_compat_log_miss(*args, w.logs.handle, L.ptr, miss8.ptr, c.ldm, flags.ptr)
                finally:
                    del os.environ["GK_TEST_HOOKS"]
            elif form == "cols":
                rc = lib().gk_compat_log_miss_cols(*args, w.logs.handle, cols.ctypes.data, 3, L.ptr, miss8.ptr, c.ldm, flags.ptr)
            elif form == "index":
                rc = lib().gk_compat_index(*args, w.logs.handle, lidx.ptr, miss8.ptr, c.ldm, flags.ptr)
            else:
                rc = lib().gk_compat_log_miss_narrow(*args, w.logs.handle, cols.ctypes.data, 8, L.ptr, miss8.ptr, c.ldm, flags.ptr,
                                                     msum.ptr)
            return rc, lambda: [b.download() for b in (L, lidx, miss8, flags, msum)]

        def settle():      # the products the first run met get their log10: every later run finds them in the table
            dev.sync()
            w.logs.resolve()
        call.settle = settle
        return call
    return make


def s_em_sets(w):
    out = w.dev.alloc((32, 1), np.uint32).zero()

    def call():
        rc = lib().gk_em_sets(w.dev.ctx, w.c32.tab, w.c32.rows.ptr, 32, 0, 12, w.mask4.ptr, 1, out.ptr)
        return rc, lambda: [out.download()]
    return call


def s_em_distinct(w):
    sets, count = np.zeros((64, 1), np.uint32), np.zeros(64, np.uint32)

    def call():
        n = C.c_int32()
        rc = lib().gk_em_distinct(w.dev.ctx, w.sets32.ptr, 32, 1, 64, sets.ctypes.data, count.ctypes.data, C.byref(n))

        def finish():      # in no particular order: sorted by set
            order = np.argsort(sets[:n.value, 0], kind="stable")
            return [np.array([n.value]), sets[:n.value][order], count[:n.value][order]]
        return rc, finish
    return call


def s_em_run(w):
    weight = w.mult.astype(np.float64)
    prob = np.zeros(4, np.float64)

    def call():
        it = C.c_int32()
        rc = lib().gk_em_run(w.dev.ctx, w.uniq.ctypes.data, weight.ctypes.data, 4, 1, 4, 300, 1e-4, prob.ctypes.data, C.byref(it))
        return rc, lambda: [prob.copy(), np.array([it.value])]
    return call


def s_sample_em(w):
    prob, count = np.zeros(4, np.float64), np.zeros(4, np.int64)

    def call():
        job = (_lib.EmJob * 1)()
        job[0] = _lib.EmJob(d_rows=w.c32.rows.ptr, n_rows=32, d_mask=w.mask4.ptr, vbeg=0, vend=12, words=1, n_allele=4,
                            n_distinct=-1, iterations=-1)
        rc = lib().gk_sample_em(w.dev.ctx, w.c32.tab, job, 1, 300, 1e-4, prob.ctypes.data, count.ctypes.data)
        return rc, lambda: [prob.copy(), count.copy(), np.array([job[0].n_distinct, job[0].iterations])]
    return call


def s_em_bootstrap(w):
    prob, iters, counts = np.zeros(12, np.float64), np.zeros(3, np.int32), np.zeros(12, np.uint32)
    job = (_lib.BootJob * 1)()
    job[0] = _lib.BootJob(sets=w.uniq.ctypes.data, count=w.mult.ctypes.data, n_sets=4, words=1, n_allele=4, stream=0)

    def call():
        rc = lib().gk_em_bootstrap(w.dev.ctx, job, 1, 3, SEED, 300, 1e-4, prob.ctypes.data, iters.ctypes.data, counts.ctypes.data)
        return rc, lambda: [prob.copy(), iters.copy(), counts.copy()]
    return call


def s_depth(w):
    depth = np.zeros(int(w.gene_off[-1]), np.uint32)

    def call():
        rc = lib().gk_depth(w.dev.ctx, w.tab.handle, w.tab.mates.ptr, 0, w.gene_off.ctypes.data, 2, depth.ctypes.data)
        return rc, lambda: [depth.copy()]
    return call


def s_depth_weighted(w):
    total = int(w.gene_off[-1])
    rank = np.zeros((2, 2), np.int64)
    stat, tot, depth = np.zeros(12, np.uint32), np.zeros(6, np.uint64), np.zeros(3 * total, np.uint32)

    def call():
        rc = lib().gk_depth_weighted(w.dev.ctx, w.tab.handle, w.tab.mates.ptr, 0, 0, w.gene_off.ctypes.data, 2, w.W.ptr, w.ldw, 3,
                                     None, rank.ctypes.data, stat.ctypes.data, tot.ctypes.data, depth.ctypes.data)
        return rc, lambda: [stat.copy(), tot.copy(), depth.copy()]
    return call


def s_cn(which):
    def make(w):
        x = np.linspace(0.0, 3.0, 16)
        dens = np.random.default_rng(SEED).random(16)
        bases, dev_ = np.array([1.0, 1.5, 2.0]), np.array([0.1, 0.12, 0.15, 0.2])
        ll, cn = np.zeros(3, np.float64), np.zeros(16, np.int32)

        def call():
            if which == "fit":
                rc = lib().gk_cn_fit(w.dev.ctx, x.ctypes.data, dens.ctypes.data, 16, bases.ctypes.data, 3, dev_.ctypes.data, 4, 0,
                                     0.1, ll.ctypes.data)
            else:
                rc = lib().gk_cn_assign(w.dev.ctx, x.ctypes.data, 16, 1.0, dev_.ctypes.data, 4, 0, 0.1, cn.ctypes.data)
            return rc, lambda: [ll.copy(), cn.copy()]
        return call
    return make


def s_call_coverage(w):
    gene_len = int(w.gene_off[1])
    depth = np.zeros(6 * gene_len, np.uint32)

    def call():
        rc = lib().gk_call_coverage(w.dev.ctx, w.tab.handle, w.tab.mates.ptr, 0, w.rows.ptr, w.n, w.miss8.ptr, w.ldm, 3,
                                    w.fit_cols.ctypes.data, 2, 0, gene_len, depth.ctypes.data)
        return rc, lambda: [depth.copy()]
    return call


def s_weighted_sums(w):
    out = np.zeros(12, np.float64)

    def call():
        rc = lib().gk_weighted_sums(w.dev.ctx, w.V.ptr, 128, 100, 3, w.W100.ptr, 128, 4, out.ctypes.data)
        return rc, lambda: [out.copy()]
    return call


def s_call_fit(w):
    hist, col, m = np.zeros(18, np.uint64), np.zeros(6, np.uint64), np.zeros(1, np.uint64)

    def call():
        rc = w.call_fit(hist, col, m)
        return rc, lambda: [hist.copy(), col.copy(), m.copy(), w.d_min.download()]
    return call


def s_call_fit_extra(w):
    out = np.zeros(3, np.uint64)

    def call():
        rc = lib().gk_call_fit_extra(w.dev.ctx, w.miss8.ptr, w.ldm, w.n, 3, w.d_min.ptr, out.ctypes.data)
        return rc, lambda: [out.copy()]
    return call


def s_call_swap(w):
    """No row state passed in: the call takes its own."""
    loss, rows_for = np.zeros((2, 3), np.uint64), np.zeros((2, 3), np.uint64)
    gain, against, m, beyond = (np.zeros(k, np.uint64) for k in (3, 3, 1, 1))

    def call():
        rc = lib().gk_call_swap(w.dev.ctx, w.miss8.ptr, w.ldm, w.n, 3, w.fit_cols.ctypes.data, 2, loss.ctypes.data,
                                rows_for.ctypes.data, gain.ctypes.data, against.ctypes.data, m.ctypes.data, beyond.ctypes.data, 0)
        return rc, lambda: [a.copy() for a in (loss, rows_for, gain, against, m, beyond)]
    return call


def s_call_patterns(w):
    slots = 64
    patterns, counts = np.zeros((slots, 16), np.uint8), np.zeros(slots, np.uint64)
    n, beyond, unplaced = np.zeros(1, np.int64), np.zeros(1, np.uint64), np.zeros(1, np.uint64)

    def call():
        rc = lib().gk_call_patterns(w.dev.ctx, w.miss8.ptr, w.ldm, w.n, 3, w.fit_cols.ctypes.data, 2, slots, patterns.ctypes.data,
                                    counts.ctypes.data, n.ctypes.data, beyond.ctypes.data, unplaced.ctypes.data)

        def finish():      # in the order of the hash table's slots, which the schedule may change: sorted by pattern
            k = int(n[0])
            order = np.lexsort(patterns[:k, ::-1].T)
            return [np.array([k]), patterns[:k][order], counts[:k][order], beyond.copy(), unplaced.copy()]
        return rc, finish
    return call


def s_novel_assign(w):
    code, count, first = np.zeros(w.n, np.uint16), np.zeros(4, np.uint32), np.zeros(4, np.int32)

    def call():
        rc = w.novel_assign(code, count, first)
        return rc, lambda: [code.copy(), count.copy(), np.where(count > 0, first, 0)]
    return call


def s_novel_confusion(w):
    cap = 256
    col, slot_of = np.array([0, 1], np.int32), np.array([0, 1], np.int32)
    totals = np.zeros(10, np.uint64)
    slot, ordinal, count, key = (np.zeros(cap, t) for t in (np.int32, np.int32, np.uint32, np.uint64))

    def call():
        n = C.c_int64()
        rc = lib().gk_novel_confusion(w.dev.ctx, w.tab.handle, w.rows.ptr, w.n, w.code.ptr, w.vflag.ptr, w.span[0], w.span[1],
                                      w.carry.ptr, col.ctypes.data, slot_of.ctypes.data, 2, 2, totals.ctypes.data, cap,
                                      slot.ctypes.data, ordinal.ctypes.data, count.ctypes.data, key.ctypes.data, C.byref(n))

        def finish():      # in no particular order: sorted by (slot, ordinal)
            k = n.value
            order = np.lexsort((ordinal[:k], slot[:k]))
            return [totals.copy(), np.array([k])] + [a[:k][order] for a in (slot, ordinal, count, key)]
        return rc, finish
    return call


SCENARIOS = {
    "index_create": s_index_create,
    "tabulate_spilled": s_tabulate(False),
    "tabulate_spilled_wide": s_tabulate(True),
    "tab_from_csr": s_tab_from_csr,
    "select_gene_first_use": s_select_gene_first_use,
    "mates_compact": s_mates_compact,
    "sample_prepare_all": s_prepare(False),
    "sample_prepare_exon": s_prepare(True),
    "variant_surviving": s_variant_surviving,
    "select_nonempty": s_select_nonempty,
    "compat_log_miss": s_compat("plain"),
    "compat_log_miss_row_classes": s_compat("row_classes"),
    "compat_log_miss_cols": s_compat("cols"),
    "compat_index": s_compat("index"),
    "compat_log_miss_narrow": s_compat("narrow"),
    "em_sets": s_em_sets,
    "em_distinct": s_em_distinct,
    "em_run": s_em_run,
    "sample_em": s_sample_em,
    "em_bootstrap": s_em_bootstrap,
    "depth": s_depth,
    "depth_weighted": s_depth_weighted,
    "cn_fit": s_cn("fit"),
    "cn_assign": s_cn("assign"),
    "call_coverage": s_call_coverage,
    "weighted_sums": s_weighted_sums,
    "call_fit": s_call_fit,
    "call_fit_extra": s_call_fit_extra,
    "call_swap": s_call_swap,
    "call_patterns": s_call_patterns,
    "novel_assign": s_novel_assign,
    "novel_confusion": s_novel_confusion,
}

# M, the pool allocations of a clean run, per entry point (test_clean_run_takes_the_declared_blocks holds them to the code)
TAKES = {
    "index_create": 9,
    "tabulate_spilled": 23,
    "tabulate_spilled_wide": 26,
    "tab_from_csr": 4,
    "select_gene_first_use": 4,
    "mates_compact": 3,
    "sample_prepare_all": 10,
    "sample_prepare_exon": 10,
    "variant_surviving": 4,
    "select_nonempty": 2,
    "compat_log_miss": 1,
    "compat_log_miss_row_classes": 11,
    "compat_log_miss_cols": 2,
    "compat_index": 1,
    "compat_log_miss_narrow": 1,
    "em_sets": 1,
    "em_distinct": 3,
    "em_run": 9,
    "sample_em": 14,
    "em_bootstrap": 11,
    "depth": 4,
    "depth_weighted": 7,
    "cn_fit": 1,
    "cn_assign": 2,
    "call_coverage": 4,
    "weighted_sums": 2,
    "call_fit": 1,
    "call_fit_extra": 1,
    "call_swap": 2,
    "call_patterns": 2,
    "novel_assign": 2,
    "novel_confusion": 9,
}
assert TAKES.keys() == SCENARIOS.keys()


@pytest.fixture(scope="module")
def world(device):
    hook(device.ctx, 0)
    w = World(device)
    w.clean = {}
    yield w
    hook(device.ctx, 0)
    os.environ.pop("GK_TEST_HOOKS", None)


def run(w, call, nth):
    """One call with allocation ``nth`` failing (``BEYOND``: none) -> (return code, finish, blocks out before, after,
    allocations counted)."""
    ctx = w.dev.ctx
    if hasattr(call, "before"):
        call.before()
    before, _ = hook(ctx, nth)
    try:
        rc, finish = call()
    finally:
        after, taken = hook(ctx, 0)
    return rc, finish, before, after, taken


def clean_run(w, name):
    """(call, M, outputs) of the scenario: from its second clean run, when the pool and the value table have seen the first."""
    if name not in w.clean:
        call = SCENARIOS[name](w)
        m = out = None
        for first in (True, False):
            rc, finish, _, _, m = run(w, call, BEYOND)
            assert rc == 0, lib().gk_last_error()
            out = finish()
            if first and hasattr(call, "settle"):
                call.settle()
        w.clean[name] = (call, m, [np.ascontiguousarray(a).tobytes() for a in out])
    return w.clean[name]


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_clean_run_takes_the_declared_blocks(world, name):
    _, m, _ = clean_run(world, name)
    print(f"{name}: {m} pool allocations")
    assert m == TAKES[name]


@pytest.mark.parametrize("name,nth", [(name, nth) for name in sorted(TAKES) for nth in range(1, TAKES[name] + 1)])
def test_a_failed_allocation_leaves_no_block_out(world, name, nth):
    call, m, want = clean_run(world, name)
    assert nth <= m, "TAKES declares more allocations than the entry point makes"
    rc, finish, before, after, taken = run(world, call, nth)
    if rc != 0 and hasattr(call, "discard"):
        call.discard()
    print(f"{name}, allocation {nth} fails: rc {rc}, {after - before} blocks left out, {taken} allocations")
    assert rc != 0 and taken == nth
    assert lib().gk_last_error()
    assert after == before, f"{after - before} blocks of the context left out"
    rc, finish, _, _, _ = run(world, call, BEYOND)
    assert rc == 0, lib().gk_last_error()
    got = [np.ascontiguousarray(a).tobytes() for a in finish()]
    assert got == want

"""The compatibility kernel (csrc/gk_typing.hip: compat_kernel, patch_pending) driven directly with hand-built CSR tables,
drop flags and bit rows, every output form against the plain reference of tests/compat_reference.py, bit for bit; the
tally behind the drop flags against ``np.bincount``; and the typing drivers on the hand-built sample whose rows
underflow, against the oracle.

What each family of cases is for:

* list shapes  -- chunks of 64 ordinals over the four lists laid end to end (lengths around every multiple of 64; the
  positive / negative boundary inside a chunk, on its edge and one either side), empty sub-lists, empty rows before the
  first listed one, a tabulation without ids, ids of other genes and novel ids on both sides, one ordinal positive here
  and negative there under drop flags 1 and 2;
* drop flags   -- the kept variants of a chunk compacted back to back: 0, 1, 2, 3, 4, 5, 8, 9, 63, 64 kept (rounds of
  four and the tail), a chunk dropped whole inside a row that keeps others, a row that keeps nothing;
* alleles      -- 1 - 4 allele slots per lane, passes of 256 alleles, the last word of a pass beyond the gene's words,
  bits at both ends of every 32- and 64-allele boundary;
* rows / tiles -- 16-row tiles (2 rows per wave), quads of 4 rows on the way out, groups of 8 tiles per XCD, more tiles
  than the grid's 2048 workgroups, the zeroed pad of the mismatch table up to its stride;
* numeric      -- counts of 98 .. 109 and 254 .. 300 mismatches: the byte 255 from 100 on, subnormal products, +0.0 and
  -inf, flag bit 0 (and its absence at 99), the bit-3 route of a +0.0 product met before its log10 is known."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compat_reference as cr  # noqa: E402

from kir_graph_amd._lib import check, lib  # noqa: E402
from kir_graph_amd.engine import LogTable  # noqa: E402

pytestmark = pytest.mark.gpu

NAN_FILL = np.uint64(0x7FF85EA71E5EA71E)      # a NaN no kernel writes: an entry nobody wrote keeps it


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    """One gene's inputs on the host + their reference (computed once, never changed)."""

    def __init__(self, name, off, ids, n_var_total, rows, vflag, vbeg, vend, bits, keep_empty=False):
        self.name = name
        self.off, self.ids = np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(ids, np.uint32)
        self.n_var_total, self.n_csr = int(n_var_total), (len(off) - 1) // 4
        self.rows = np.ascontiguousarray(rows, np.int32)
        self.vflag = np.ascontiguousarray(vflag, np.uint8)
        self.vbeg, self.vend, self.keep_empty = int(vbeg), int(vend), bool(keep_empty)
        self.bits = np.asarray(bits, dtype=bool).reshape(vend - vbeg, -1)
        self.n_allele = self.bits.shape[1]
        self.mask = cr.packMask(self.bits)
        self.words = self.mask.shape[1]
        assert len(self.vflag) == n_var_total and (np.diff(self.rows) > 0).all() and self.rows.max() < self.n_csr
        self._ref = None

    @property
    def ref(self) -> cr.CompatRef:
        if self._ref is None:
            ref = cr.compatReference(self.off, self.ids, self.rows, self.vflag, self.vbeg, self.vend, self.bits, self.keep_empty)
            for a in ref:
                a.setflags(write=False)
            self._ref = ref
        return self._ref


# the list-shape gene: variants [0, 37) and [337, 400) belong to other genes, [400, 440) are novel
VBEG, VEND, N_VAR, N_TOTAL = 37, 337, 400, 440
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]
BOUNDARIES = [0, None, 1, 63, 64, 65]          # ids before the first negative one (None: positives only)
KEPT = [0, 1, 2, 3, 4, 5, 8, 9, 63, 64]


def listShapeFlags():
    """Drop flags of the list-shape gene: the upper 130 variants of the gene are dropped from both sides, a few from one."""
    vflag = np.zeros(N_TOTAL, dtype=np.uint8)
    vflag[VEND - 130:VEND] = 3
    vflag[[50, 60, 61, 62]] = 1
    vflag[[51, 70, 71, 72]] = 2
    vflag[52] = 3
    vflag[[5, 390, 410]] = 1                      # ids outside the gene and a novel one carry flags too
    vflag[[6, 391, 411]] = 2
    return vflag


def listShapeLists(rng):
    """~45 rows: every total length with the boundary cycling through its places, every boundary at two long rows, the
    explicit rows of the docstring."""
    vflag = listShapeFlags()
    local = np.arange(VBEG, VEND - 130)
    common, rare = local[(local - VBEG) % 2 == 0], local[(local - VBEG) % 2 == 1]     # carried by most / by few alleles
    dropped = np.arange(VEND - 130, VEND)
    outside = np.concatenate([np.arange(0, VBEG), np.arange(VEND, N_VAR), np.arange(N_VAR, N_TOTAL)])

    def row(total, n_pos, k):
        """``total`` distinct ids, the first ``n_pos`` positive: agreeing ids first, then the rest; every 16th from
        outside the gene; sub-lists rpv / rnv empty for every third row, lpv / lnv for another third."""
        pool_p = np.concatenate([rng.permutation(common), rng.permutation(dropped), rng.permutation(rare)])
        pos = pool_p[:n_pos].copy()
        used = set(pos.tolist())
        pool_n = np.array([v for v in np.concatenate([rng.permutation(rare), rng.permutation(dropped), rng.permutation(common)])
                           if int(v) not in used])
        neg = pool_n[:total - n_pos].copy()
        out = rng.permutation(outside)
        pos[3::16] = out[:len(pos[3::16])]
        neg[5::16] = out[100:100 + len(neg[5::16])]
        cut = lambda x: (0, len(x), len(x) // 2)[k % 3]      # noqa: E731
        return [pos[:cut(pos)].tolist(), pos[cut(pos):].tolist(), neg[:cut(neg)].tolist(), neg[cut(neg):].tolist()]

    lists = []
    for k, total in enumerate(LENGTHS):
        b = BOUNDARIES[k % len(BOUNDARIES)]
        lists.append(row(total, total if b is None else min(b, total), k))
    for total in (129, 300):
        for k, b in enumerate(BOUNDARIES):
            lists.append(row(total, total if b is None else b, k + 1))
    # ids of other genes, the gene's first and last variant, novel ids: on both sides
    lists.append([[0, 36, VBEG, VEND - 131], [VEND, N_VAR - 1, N_VAR, N_TOTAL - 1], [1, 35, VBEG + 1, VEND - 132],
                  [VEND + 1, N_VAR - 2, N_VAR + 1, N_TOTAL - 2]])
    # one ordinal positive here and negative there, under flags 1 (50), 2 (51) and 3 (52)
    lists.append([[50, 51], [52, 40], [], []])
    lists.append([[], [], [50, 51], [52, 40]])
    # kept ids per chunk: chunk 0 keeps n of its 64 (spread over the chunk), chunk 1 is dropped whole, the tail keeps 5
    kept_pool, drop_pool = local[vflag[local] == 0], dropped
    for n in KEPT:
        where = set(((np.arange(n) * 64) // max(n, 1)).tolist())
        kp, dp = iter(rng.permutation(kept_pool).tolist()), iter(rng.permutation(drop_pool).tolist())
        chunk0 = [next(kp) if t in where else next(dp) for t in range(64)]
        ids = chunk0 + [next(dp) for _ in range(64)] + [next(kp) for _ in range(5)]
        assert sum(1 for v in chunk0 if not vflag[v]) == n
        lists.append([ids[:40], ids[40:70], ids[70:100], ids[100:]])
    lists.append([dropped[:30].tolist(), [], dropped[30:70].tolist(), []])        # nothing kept: nvar == 0
    return lists


def listShapeBits(rng, n_allele=70):
    """Even variants of the gene are carried by nine alleles in ten, odd ones by one in ten; the first variants hold the
    explicit patterns: bit 0, bit 31, the first and last allele, both sides of the 32 and 64 boundaries."""
    n_span = VEND - VBEG
    p = np.where(np.arange(n_span) % 2 == 0, 0.9, 0.1)[:, None]
    bits = rng.random((n_span, n_allele)) < p
    edge = [a for a in (0, 31, 32, 33, 63, 64, 65, n_allele - 1) if a < n_allele]
    bits[0] = False; bits[0, edge] = True
    bits[1] = True; bits[1, edge] = False
    bits[2] = False; bits[2, 0] = True
    bits[3] = False; bits[3, n_allele - 1] = True
    return bits


def interleave(lists, rng, fillers=1):
    """The rows of ``lists`` as CSR rows 2, 2 + (fillers + 1), ...: rows 0 and 1 are empty, unlisted rows lie between."""
    csr, at = [[[], [], [], []], [[], [], [], []]], []
    for row in lists:
        at.append(len(csr))
        csr.append(row)
        for _ in range(fillers):
            csr.append([rng.integers(0, N_TOTAL, 3).tolist(), [], rng.integers(0, N_TOTAL, 2).tolist(), [7]])
    # the last listed row is the last row of the CSR
    csr.append(csr.pop(at[-1]))
    at[-1] = len(csr) - 1
    return csr, at


def listShapeCases():
    rng = np.random.default_rng(20260)
    lists = listShapeLists(rng)
    csr, at = interleave(lists, rng)
    off, ids = cr.packLists(csr)
    bits, vflag = listShapeBits(rng), listShapeFlags()
    zero = np.zeros(N_TOTAL, dtype=np.uint8)
    none_off = np.zeros(4 * 40 + 1, dtype=np.uint32)
    return [
        Case("flags, row 0 listed", off, ids, N_TOTAL, [0] + at, vflag, VBEG, VEND, bits),
        Case("flags, empty rows first, keep_empty", off, ids, N_TOTAL, at, vflag, VBEG, VEND, bits, keep_empty=True),
        Case("no flags", off, ids, N_TOTAL, [0, 1] + at, zero, VBEG, VEND, bits),
        Case("no ids at all", none_off, np.zeros(0, np.uint32), N_TOTAL, np.arange(1, 40, 2), zero, VBEG, VEND, bits),
        Case("no ids at all, keep_empty", none_off, np.zeros(0, np.uint32), N_TOTAL, np.arange(40), vflag, VBEG, VEND, bits, True),
    ]


ALLELES = [1, 2, 3, 8, 31, 32, 33, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 289, 577]


def alleleCase(n_allele):
    """40 short rows (lengths 0 .. 9, 63 .. 65, 129) over 48 variants against ``n_allele`` alleles."""
    rng = np.random.default_rng(7000 + n_allele)
    vbeg, n_span, n_total = 5, 48, 60
    bits = rng.random((n_span, n_allele)) < 0.5
    edge = sorted({a for b in range(0, n_allele + 64, 32) for a in (b - 1, b, b + 1) if 0 <= a < n_allele} | {0, n_allele - 1})
    bits[0] = False; bits[0, edge] = True
    bits[1] = True; bits[1, edge] = False
    bits[2] = False; bits[2, [a for a in edge if a % 32 == 0]] = True          # bit 0 of every word
    bits[3] = False; bits[3, [a for a in edge if a % 32 == 31]] = True         # bit 31 of every word
    lists = []
    for k in range(40):
        total = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 129][k % 14]
        ids = np.concatenate([rng.permutation(n_total) for _ in range(3)])[:total]
        ids[:min(4, total)] = (vbeg + np.arange(4))[:min(4, total)]             # the explicit patterns, in every row
        n_pos = [0, total, total // 2, min(1, total)][k % 4]
        lists.append([ids[:n_pos // 2].tolist(), ids[n_pos // 2:n_pos].tolist(), ids[n_pos:].tolist(), []])
    off, ids = cr.packLists(lists)
    vflag = np.zeros(n_total, dtype=np.uint8)
    vflag[vbeg + 10] = 1; vflag[vbeg + 11] = 2; vflag[vbeg + 12] = 3
    return Case(f"{n_allele} alleles", off, ids, n_total, np.arange(40), vflag, vbeg, vbeg + n_span, bits)


ROWS = [1, 2, 15, 16, 17, 31, 33, 48, 64, 127, 128, 129, 1024, 1025, 2049]
MANY_ROWS = 2048 * 16 + 129


def rowCase(n_rows, n_allele=3):
    """Every 13th pair of a CSR of ``13 n_rows`` rows, the last one included; lists of 0 .. 3 ids each (built as arrays:
    the large case has 400 k rows)."""
    rng = np.random.default_rng(9000 + n_rows)
    vbeg, n_span, n_total = 3, 29, 40
    n_csr = 13 * n_rows
    lens = rng.integers(0, 4, 4 * n_csr)
    lens[rng.random(4 * n_csr) < 0.3] = 0
    off = np.zeros(4 * n_csr + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    ids = rng.integers(0, n_total, int(off[-1])).astype(np.uint32)
    bits = rng.random((n_span, n_allele)) < 0.5
    vflag = (rng.random(n_total) < 0.2).astype(np.uint8) * rng.integers(1, 4, n_total).astype(np.uint8)
    return Case(f"{n_rows} rows", off, ids, n_total, 13 * np.arange(n_rows) + 12, vflag, vbeg, vbeg + n_span, bits,
                keep_empty=bool(n_rows % 2))


def numericCase(gene):
    """The long rows of the hand-built sample (compat_reference.underflowIndex), as lists: per window the ids of a read of
    allele 0 in list order -- mismatching factors first / last / interleaved -- plus a few short rows."""
    sidx, order = cr.underflowIndex()
    ordinal = {(v.ref, v.pos): i for i, v in enumerate(sidx.variants)}
    mine = [i for i, v in enumerate(sidx.variants) if v.ref == gene]
    vbeg, vend = mine[0], mine[-1] + 1
    names = sidx.alleles[gene]
    bits = np.zeros((vend - vbeg, len(names)), dtype=bool)
    for i in mine:
        bits[i - vbeg, [names.index(a) for a in sidx.variants[i].allele]] = True
    lists = []
    for w in range(len(cr.PLACEMENTS)):
        ids = [ordinal[(gene, p)] for p in order[gene][w] if (gene, p) in ordinal]
        pos = [i for i in ids if bits[i - vbeg, 0]]
        assert ids[:len(pos)] == pos
        lists.append([pos[:len(pos) // 2], pos[len(pos) // 2:], ids[len(pos):], []])
        lists.append([ids[:3], [], ids[-4:], []])
    off, ids = cr.packLists(lists)
    n_total = len(sidx.variants)
    return Case(f"numeric {gene}", off, ids, n_total, np.arange(len(lists)), np.zeros(n_total, np.uint8), vbeg, vend, bits)


# ------------------------------------------------------------------------------------------------------------ device
class OnDevice:
    """The tabulation of a case (``gk_tab_from_csr``) and its uploaded rows, flags and bit rows."""

    def __init__(self, device, case: Case):
        self.dev, self.case = device, case
        h = C.c_void_p()
        n = case.n_csr
        gene, nh = np.zeros(max(n, 1), np.uint8), np.ones(max(n, 1), np.uint8)
        check(lib().gk_tab_from_csr(device.ctx, case.n_var_total, n, case.off.ctypes.data,
                                    case.ids.ctypes.data if len(case.ids) else None, gene.ctypes.data, nh.ctypes.data,
                                    C.byref(h)))
        self.tab = h
        self.rows, self.vflag, self.mask = device.put(case.rows), device.put(case.vflag), device.put(case.mask)
        self.n_rows = len(case.rows)
        self.ldm = (self.n_rows + 63) // 64 * 64

    def args(self):
        c = self.case
        return (self.dev.ctx, self.tab, self.rows.ptr, self.n_rows, self.vflag.ptr, c.vbeg, c.vend, self.mask.ptr, c.words,
                c.n_allele, int(c.keep_empty))

    def filled(self, shape, dtype):
        fill = {np.float64: NAN_FILL, np.uint8: 0xFF, np.uint16: 0xFFFF, np.uint32: 0xFFFFFFFF}[dtype]
        host = np.full(shape, fill, dtype=np.uint64 if dtype is np.float64 else dtype)
        buf = self.dev.alloc(shape, dtype)
        check(lib().gk_h2d(self.dev.ctx, buf.ptr, host.ctypes.data, host.nbytes))
        return buf

    def close(self):
        for b in (self.rows, self.vflag, self.mask):
            b.free()
        lib().gk_tab_destroy(self.tab)


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_products(gpu: OnDevice):
    """``gk_compat``: products, saturated u8 counts, kept ids per row -- the whole of every buffer."""
    c, ref = gpu.case, gpu.case.ref
    probs = gpu.filled((c.n_allele, gpu.n_rows), np.float64)
    miss = gpu.filled((c.n_allele, gpu.n_rows), np.uint8)
    nvar = gpu.filled(gpu.n_rows, np.uint16)
    check(lib().gk_compat(*gpu.args(), probs.ptr, miss.ptr, nvar.ptr))
    got = probs.download()
    assert np.array_equal(bits_of(got), bits_of(ref.probs.T)), c.name
    assert np.array_equal(miss.download(), ref.miss_u8.T), c.name
    assert np.array_equal(nvar.download(), np.minimum(ref.nvar, 65535).astype(np.uint16)), c.name
    for b in (probs, miss, nvar):
        b.free()


def settle_log_miss(gpu: OnDevice, logs: LogTable, cols=None):
    """``gk_compat_log_miss`` (``_cols`` with ``cols``) into sentinel-filled buffers, then resolve + ``gk_compat_patch``
    (or the whole table again after bit 3) until bit 2 is clear, bit 0 carried over a patch -- the way
    ``DeviceModel.finishLog`` does.  Returns (L, miss8, final flags, patches taken, tables written again)."""
    c = gpu.case
    n_cols = c.n_allele if cols is None else len(cols)
    L = gpu.filled((n_cols, gpu.n_rows), np.float64)
    miss8 = gpu.filled((n_cols, gpu.ldm), np.uint8)
    flags = gpu.filled(1, np.uint32)

    def launch():
        if cols is None:
            check(lib().gk_compat_log_miss(*gpu.args(), logs.handle, L.ptr, miss8.ptr, gpu.ldm, flags.ptr))
        else:
            cc = np.ascontiguousarray(cols, dtype=np.int32)
            check(lib().gk_compat_log_miss_cols(*gpu.args(), logs.handle, cc.ctypes.data, len(cc), L.ptr, miss8.ptr, gpu.ldm,
                                                flags.ptr))
    launch()
    sticky = patches = again = 0
    for _ in range(16):
        gpu.dev.sync()
        f = int(flags.download()[0]) | sticky
        if not f & 4:
            break
        logs.resolve()
        if f & 8:
            sticky = 0
            again += 1
            launch()
        else:
            sticky = f & 1
            patches += 1
            check(lib().gk_compat_patch(gpu.dev.ctx, logs.handle, L.ptr, gpu.n_rows, n_cols, miss8.ptr, gpu.ldm, flags.ptr))
    else:
        raise AssertionError(f"{c.name}: the value table did not settle")
    out = L.download(), miss8.download(), f, patches, again
    for b in (L, miss8, flags):
        b.free()
    return out


def assert_log_table(gpu: OnDevice, got, cols=None):
    """L, the mismatch bytes (zero from n_rows up to the stride) and flag bit 0 against the reference's columns."""
    c, ref = gpu.case, gpu.case.ref
    L, miss8, f = got[:3]
    sel = slice(None) if cols is None else np.asarray(cols)
    want_log, want_m = ref.log[:, sel], ref.miss[:, sel]
    assert not np.isnan(L).any(), c.name                                   # a settled table holds no NaN
    assert np.array_equal(bits_of(L), bits_of(want_log.T)), c.name
    assert np.array_equal(np.isneginf(L), (ref.probs[:, sel] == 0.0).T), c.name
    assert np.array_equal(miss8[:, :gpu.n_rows], np.where(want_m < cr.MISS_CAP, want_m, 255).astype(np.uint8).T), c.name
    assert not miss8[:, gpu.n_rows:].any(), c.name
    want0 = bool((want_m >= cr.MISS_CAP).any() or (ref.nvar >= cr.NVAR_CAP).any())
    assert f & 3 == int(want0), (c.name, f)
    assert not f & 0xC, (c.name, f)


def check_index_form(gpu: OnDevice, logs: LogTable):
    """``gk_compat_index`` (called again while a value had no log10) + ``gk_expand_index``: the float form's L, bytes and
    bit 0."""
    c = gpu.case
    lidx = gpu.filled((c.n_allele, gpu.ldm), np.uint16)
    miss8 = gpu.filled((c.n_allele, gpu.ldm), np.uint8)
    flags = gpu.filled(1, np.uint32)
    for _ in range(16):
        check(lib().gk_compat_index(*gpu.args(), logs.handle, lidx.ptr, miss8.ptr, gpu.ldm, flags.ptr))
        gpu.dev.sync()
        f = int(flags.download()[0])
        if not f & 4:
            break
        logs.resolve()
    else:
        raise AssertionError(f"{c.name}: the value table did not settle")
    assert not f & 2, c.name
    idx = lidx.download()[:, :gpu.n_rows]
    assert idx.max() < 0xFFFF, c.name
    L = gpu.filled((c.n_allele, gpu.n_rows), np.float64)
    check(lib().gk_expand_index(gpu.dev.ctx, logs.handle, lidx.ptr, gpu.ldm, gpu.n_rows, c.n_allele, L.ptr, gpu.n_rows))
    assert_log_table(gpu, (L.download(), miss8.download(), f))
    for b in (lidx, miss8, flags, L):
        b.free()


def columnLists(n_allele):
    """Ascending column lists of 1, 2, 3, 4, 8, 33, 64 and 65 alleles: allele 0, the last one and the neighbours of 31 / 32
    first, then the rest from the front."""
    first = [a for a in (0, n_allele - 1, 31, 32, 30, 33, 63, 64) if 0 <= a < n_allele]
    order = list(dict.fromkeys(first + list(range(n_allele))))
    return [sorted(order[:k]) for k in (1, 2, 3, 4, 8, 33, 64, 65) if k <= n_allele]


def check_every_form(device, case: Case, with_cols=False, expect=None):
    """All output forms of one case against its reference.  ``expect``: "patch" / "again" -- which way a fresh value
    table must have settled."""
    gpu = OnDevice(device, case)
    try:
        check_products(gpu)
        logs = LogTable(device, log2_capacity=16)
        fresh = settle_log_miss(gpu, logs)
        assert_log_table(gpu, fresh)
        if expect == "patch":
            assert fresh[3] >= 1 and fresh[4] == 0, fresh[3:]
        if expect == "again":
            assert fresh[4] >= 1, fresh[3:]
        warm = settle_log_miss(gpu, logs)                 # the table knows every value now: same bits, nothing to settle
        assert warm[3] == 0 and warm[4] == 0, warm[3:]
        assert_log_table(gpu, warm)
        assert np.array_equal(bits_of(warm[0]), bits_of(fresh[0])) and np.array_equal(warm[1], fresh[1])
        check_index_form(gpu, logs)
        logs.close()
        logs = LogTable(device, log2_capacity=16)         # the index form on a table that knows nothing
        check_index_form(gpu, logs)
        if with_cols:
            for k, cols in enumerate(columnLists(case.n_allele)):
                if k % 3 == 0:                            # now and then from a fresh table: the patch of a column table
                    logs.close()
                    logs = LogTable(device, log2_capacity=16)
                assert_log_table(gpu, settle_log_miss(gpu, logs, cols), cols)
        logs.close()
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def list_cases():
    return listShapeCases()


def test_list_shape_generator_covers_what_it_claims(list_cases):
    """The kept count of a chunk takes each of 0, 1, 2, 3, 4, 5, 63, 64; a chunk is dropped whole inside a row that keeps
    others; a row keeps nothing; rows keep 4 k and 4 k + 1 ids; the boundary lies 0, 1, 63, 64, 65 ids after the start
    and at the end of rows long enough; every total length occurs."""
    case = list_cases[0]
    off = case.off.astype(np.int64)
    per_chunk, totals, bounds, nvar = set(), set(), set(), set()
    whole = False
    for r in case.rows:
        b, mid, e = off[4 * r], off[4 * r + 2], off[4 * r + 4]
        keep = np.array([not case.vflag[case.ids[k]] & (1 if k < mid else 2) for k in range(b, e)], dtype=bool)
        chunks = [int(keep[s:s + 64].sum()) for s in range(0, len(keep), 64) if len(keep[s:s + 64]) == 64]
        per_chunk |= set(chunks)
        whole |= 0 in chunks and keep.any()
        totals.add(int(e - b)); nvar.add(int(keep.sum()))
        if e - b >= 129:
            bounds.add(int(mid - b) if mid < e else None)
    assert {0, 1, 2, 3, 4, 5, 63, 64} <= per_chunk and whole and 0 in nvar
    assert set(LENGTHS) <= totals and set(BOUNDARIES) <= bounds
    assert any(n and n % 4 == 0 for n in nvar) and any(n % 4 == 1 for n in nvar)
    assert np.array_equal(case.ref.nvar, [sum(1 for k in range(off[4 * r], off[4 * r + 4])
                                              if not case.vflag[case.ids[k]] & (1 if k < off[4 * r + 2] else 2))
                                          for r in case.rows])


@pytest.mark.parametrize("k", range(5))
def test_list_shapes_and_drop_flags(device, list_cases, k):
    check_every_form(device, list_cases[k], with_cols=(k == 0))


@pytest.mark.parametrize("n_allele", ALLELES)
def test_allele_slots_passes_and_word_edges(device, n_allele):
    check_every_form(device, alleleCase(n_allele), with_cols=(n_allele == 577), expect="patch")


@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_tiles_and_the_pad_of_the_mismatch_table(device, n_rows):
    """Row counts around the 16-row tile, the quads of the way out and the groups of 8 tiles; 64, 48, 16 and 1 rows leave
    0, 16, 48 and 63 bytes of pad per column of the mismatch table."""
    check_every_form(device, rowCase(n_rows), expect="patch")


def test_more_tiles_than_workgroups(device):
    """2048 * 16 + 129 rows x 2 alleles: 2065 tiles on a grid capped at 2048 workgroups, so workgroups take several
    tiles of their XCD's groups."""
    check_every_form(device, rowCase(MANY_ROWS, n_allele=2), expect="patch")


def test_counts_around_100_subnormal_products_and_zero(device):
    """The three long rows (mismatching factors first, last, interleaved): products bit-equal down to the subnormals and
    +0.0, L == -inf there, the u8 count saturated at 255, the byte 255 from 100 mismatches on (98 and 99 themselves), bit 0
    up; a fresh value table meets +0.0 before its log10 is known (bit 3: the table is written again) and ends in the
    warmed table's bits."""
    case = numericCase(cr.HEAVY_GENE)
    ref = case.ref
    assert ref.miss[0].tolist() == ref.miss[2].tolist() == ref.miss[4].tolist() == cr.HEAVY_COUNTS
    tiny = np.finfo(np.float64).tiny
    assert ((ref.probs > 0) & (ref.probs < tiny)).any() and (ref.probs == 0).any() and ref.flag0
    assert sorted(set(ref.miss8[0].tolist())) == [0, 30, 60, 90, 98, 99, 255]
    check_every_form(device, case, with_cols=True, expect="again")


def test_a_gene_capped_at_99_mismatches_leaves_bit_0_clear(device):
    case = numericCase(cr.CAPPED_GENE)
    assert case.ref.miss.max() == 99 and not case.ref.flag0
    check_every_form(device, case, expect="patch")


@pytest.mark.parametrize("flags", ["none", "hand-chosen"])
def test_tally_behind_the_drop_flags(device, list_cases, flags):
    """``gk_variant_count`` and ``gk_variant_count_range`` (LDS counters for [vbeg, vend), global atomics for the rest)
    equal ``np.bincount`` of the surviving positive and negative ids -- ids of other genes and novel ordinals included."""
    case = list_cases[0 if flags == "hand-chosen" else 2]
    gpu = OnDevice(device, case)
    try:
        want = np.concatenate(cr.tally(case.off, case.ids, case.rows, case.vflag, case.n_var_total))
        assert want[:VBEG].any() and want[N_VAR:N_TOTAL].any() and want[N_TOTAL:N_TOTAL + VBEG].any()
        for span in ((0, 0), (case.vbeg, case.vend), (VBEG + 10, VBEG + 40), (0, case.n_var_total)):
            cnt = gpu.filled(2 * case.n_var_total, np.uint32)
            if span == (0, 0):
                check(lib().gk_variant_count(device.ctx, gpu.tab, gpu.rows.ptr, gpu.n_rows, gpu.vflag.ptr, cnt.ptr))
            else:
                check(lib().gk_variant_count_range(device.ctx, gpu.tab, gpu.rows.ptr, gpu.n_rows, gpu.vflag.ptr, cnt.ptr,
                                                   span[0], span[1]))
            assert np.array_equal(cnt.download(), want), span
            cnt.free()
    finally:
        gpu.close()


# ------------------------------------------------------------------------------- the drivers on rows that underflow
GENE_CN = {cr.CAPPED_GENE: 2, cr.HEAVY_GENE: 2}
TOP_N = 40


def same_step(a, b):
    """Every field of one copy-number step, GPU result against the oracle's (``np.array_equal``: -inf equals -inf)."""
    assert a.n == b.n
    for f in ("value", "value_sum_indv", "allele_id", "fraction"):
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape, (f, x.shape, y.shape)
        assert not np.isnan(x).any(), f
        assert np.array_equal(x, y), f
    assert [list(r) for r in a.allele_name] == [list(r) for r in b.allele_name]


@pytest.fixture(scope="module")
def underflow():
    """Per sample ("a": some -inf entries, the best sets finite; "b": every set of the heavy gene -inf): the SAM lines, the
    oracle's tabulation and the oracle's results of the plain strategy."""
    from kir_graph_amd.index import GkIndex
    from oracle import tabulate as ot, typing as oty
    sidx, _ = cr.underflowIndex()
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    out = {}
    for which in ("a", "b"):
        lines = cr.underflowLines(sidx, which)
        ref = ot.tabulateLines(lines, gidx.variants)
        cpu = oty.makeTyper("full", copy.deepcopy(ref), top_n=TOP_N, variant_correction=True)
        calls = cpu.typing(GENE_CN)
        heavy = cpu.results[cr.HEAVY_GENE]
        if which == "a":
            assert np.isfinite(heavy[-1].value).all() and np.isneginf(heavy[0].value).any()      # -inf columns, finite best sets
        else:
            assert all(np.isneginf(step.value).all() for step in heavy)
        assert np.isfinite(cpu.results[cr.CAPPED_GENE][-1].value).all()
        out[which] = (lines, ref, cpu, calls)
    return gidx, out


def device_model(steps):
    return steps[-1].allele_prob.parts[0][0]


@pytest.mark.parametrize("driver", ["whole sample", "index tables", "gene after gene", "host lists"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_drivers_equal_the_oracle_where_rows_underflow(device, underflow, monkeypatch, which, driver):
    """The whole-sample driver (pipelined gene loop), the same under GK_INDEX_TABLE=1 (lock-step loop, index tables), the
    per-gene driver, and the per-gene driver on host lists (``SampleData.fromHost``): every field of every copy-number
    step, the names and the calls equal the oracle's; the heavy gene leaves the integer bound (``boundOk`` false), the
    gene capped at 99 mismatches keeps it."""
    from kir_graph_amd.hisat2 import PairRead, SampleData, extractVariant, pairLines
    from kir_graph_amd.kir_typing import Typing, selectKirTypingModel
    from oracle import typing as oty
    monkeypatch.setenv("GK_SEARCH", "bound")
    monkeypatch.setenv("GK_INDEX_TABLE", "1" if driver == "index tables" else "0")
    gidx, samples = underflow
    lines, ref, cpu, want_calls = samples[which]
    if driver == "host lists":
        reads = [PairRead(lpv=list(r["lpv"]), lnv=list(r["lnv"]), rpv=list(r["rpv"]), rnv=list(r["rnv"]),
                          multiple=r["multiple"], backbone=r["backbone"]) for r in ref["reads"]]
        data = SampleData.fromHost(device, {"variants": list(ref["variants"]), "reads": reads})
    else:
        data = extractVariant(pairLines(lines), gidx, dev=device)
    typer = selectKirTypingModel("full", data, top_n=TOP_N, variant_correction=True)
    assert typer._wholeSample()
    calls = Typing.typing(typer, GENE_CN) if driver == "gene after gene" else typer.typing(GENE_CN)
    for gene, steps in cpu.results.items():
        got = typer._result[gene]
        assert len(got) == len(steps), gene
        for a, b in zip(got, steps):
            same_step(a, b)
        assert got[-1].selectBest() == oty.selectBest(steps[-1]), gene
    assert calls == want_calls
    assert device_model(typer._result[cr.HEAVY_GENE]).boundOk is False
    assert device_model(typer._result[cr.CAPPED_GENE]).boundOk is True
    if driver == "index tables":
        assert device_model(typer._result[cr.CAPPED_GENE])._indexed
    data.tab.close()


@pytest.mark.parametrize("which", ["a", "b"])
def test_list_constructors_equal_the_oracle_where_rows_underflow(device, underflow, monkeypatch, which):
    """``AlleleTyping(reads, variants)`` and ``AlleleTypingExonFirst(reads, variants)`` (a part of the variants lies in
    exons) on the reads of each gene against ``oracle.typing.GeneModel`` / ``ExonFirstModel``."""
    from kir_graph_amd.hisat2 import PairRead
    from kir_graph_amd.typing_mulit_allele import AlleleTyping, AlleleTypingExonFirst
    from oracle import typing as oty
    monkeypatch.setenv("GK_SEARCH", "bound")
    _, samples = underflow
    _, ref, _, _ = samples[which]
    for gene in (cr.HEAVY_GENE, cr.CAPPED_GENE):
        variants = [v for v in ref["variants"] if v.ref == gene]
        assert any(v.in_exon for v in variants) and not all(v.in_exon for v in variants)
        reads = [r for r in ref["reads"] if r["backbone"] == gene]
        pairs = [PairRead(lpv=list(r["lpv"]), lnv=list(r["lnv"]), rpv=list(r["rpv"]), rnv=list(r["rnv"]),
                          multiple=r["multiple"], backbone=r["backbone"]) for r in reads]
        cpu = oty.GeneModel(copy.deepcopy(reads), variants, force_homo=False, top_n=TOP_N, variant_correction=True)
        gpu = AlleleTyping(pairs, variants, force_homo=False, top_n=TOP_N, variant_correction=True, device=device)
        want, got = cpu.typing(2), gpu.typing(2)
        assert np.array_equal(bits_of(gpu.probs), bits_of(cpu.probs)) and np.array_equal(bits_of(gpu.log_probs), bits_of(cpu.log_probs))
        for a, b in zip(gpu.result, cpu.result):
            same_step(a, b)
        assert got.selectBest() == oty.selectBest(want)
        assert gpu._model.boundOk is (gene == cr.CAPPED_GENE)
        cpu_e = oty.ExonFirstModel(copy.deepcopy(reads), variants, top_n=TOP_N, candidate_set_threshold=1.0)
        gpu_e = AlleleTypingExonFirst(pairs, variants, top_n=TOP_N, candidate_set_threshold=1.0, device=device)
        want, got = cpu_e.typing(2), gpu_e.typing(2)
        assert gpu_e.allele_group == cpu_e.allele_group and len(gpu_e.result) == len(cpu_e.result)
        for a, b in zip(gpu_e.result, cpu_e.result):
            same_step(a, b)
        assert got.selectBest() == oty.selectBest(want)
        assert gpu_e.full_model._model.boundOk is (gene == cr.CAPPED_GENE)

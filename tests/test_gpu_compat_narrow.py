"""The table of at most 8 listed alleles written 8 rows per wavefront (csrc/gk_compat_narrow.hip: cols_bytes, compat_rows8;
``gk_compat_log_miss_narrow``) against the plain reference of tests/compat_reference.py AND against what
``gk_compat_log_miss_cols`` + ``gk_miss_colsum`` leave on the same inputs, bit for bit: d_log, the mismatch bytes up to
their stride, the flag word, the column sums.  Every output buffer starts as a NaN pattern or garbage, the flag word and
the column sums included.

Each case is run on a value table that knows nothing (products in place, bit 2; +0.0 stores a NaN and raises bit 3), then
settled (resolve + ``gk_compat_patch`` + ``gk_miss_colsum``, or the table again after bit 3), then run on the warmed
table.  The case builders are those of tests/test_gpu_compat_edges.py.

* columns  -- lists of 1, 2, 3, 4, 5, 7 and 8 alleles of genes of 70 and 289 alleles, ordinals 0, 31, 32, 63, 64 and the
  last one; a list of 9 is an argument error, and a job of 9 columns in ``gk_sample_search`` takes compat_kernel.  Lists
  of at most 4 alleles run the kernel's form of 4 lanes per row (16 rows per wavefront), longer ones that of 8 lanes
  (8 rows): every family below has lists of both kinds;
* rows     -- around the 8 and 16 rows of a lane group, the 16 of a wave and the 128 of a tile; 257 tiles and one row;
  strides that end in the middle of a tile's line, at its end, and a tile beyond the last one;
* lists    -- the list shapes and drop flags of the existing module; groups of 8 rows of lengths 300, 0, 1 and 64 side by
  side (rounds in which most rows of a group have ended);
* numeric  -- 98 - 109 and 254 - 300 mismatches, subnormal products, +0.0, rows of 4095 and 4096 kept ids;
* driver   -- exon-first typing in fresh child processes with and without ``GK_TEST_HOOKS=wide_compat``."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compat_reference as cr  # noqa: E402
import test_gpu_compat_edges as ce  # noqa: E402
import test_gpu_exonfirst_columns as xc  # noqa: E402

from kir_graph_amd._lib import GkError, check, lib  # noqa: E402
from kir_graph_amd.engine import LogTable  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUIET_NAN = np.uint64(0x7FF8000000000000)      # what an entry holds whose +0.0 product has no log10 yet


# ------------------------------------------------------------------------------------------------------------ launches
class Outputs:
    """d_log, d_miss8, the flag word and d_msum of one case and column list, prefilled with sentinels."""

    def __init__(self, gpu: ce.OnDevice, n_cols: int):
        self.gpu, self.n_cols = gpu, n_cols
        self.L = gpu.filled((n_cols, gpu.n_rows), np.float64)
        self.miss8 = gpu.filled((n_cols, gpu.ldm), np.uint8)
        self.flags = gpu.filled(1, np.uint32)
        self.msum = gpu.filled(n_cols, np.uint32)

    def refill(self):
        for b in (self.L, self.miss8, self.flags, self.msum):
            b.free()
        self.__init__(self.gpu, self.n_cols)

    def download(self):
        self.gpu.dev.sync()
        return ce.bits_of(self.L.download()), self.miss8.download(), int(self.flags.download()[0]), self.msum.download()

    def close(self):
        for b in (self.L, self.miss8, self.flags, self.msum):
            b.free()


def launch_narrow(gpu, logs, cols, out: Outputs):
    cc = np.ascontiguousarray(cols, dtype=np.int32)
    check(lib().gk_compat_log_miss_narrow(*gpu.args(), logs.handle, cc.ctypes.data, len(cc), out.L.ptr, out.miss8.ptr,
                                          gpu.ldm, out.flags.ptr, out.msum.ptr))


def launch_wide(gpu, logs, cols, out: Outputs):
    cc = np.ascontiguousarray(cols, dtype=np.int32)
    check(lib().gk_compat_log_miss_cols(*gpu.args(), logs.handle, cc.ctypes.data, len(cc), out.L.ptr, out.miss8.ptr, gpu.ldm,
                                        out.flags.ptr))
    check(lib().gk_miss_colsum(gpu.dev.ctx, out.miss8.ptr, gpu.ldm, len(cc), out.msum.ptr))


def same(a, b, what):
    for x, y, name in zip(a, b, ("L", "miss8", "flags", "msum")):
        assert np.array_equal(x, y), (what, name)


def check_sums(got, n_rows, what):
    _, miss8, _, msum = got
    assert np.array_equal(msum, miss8[:, :n_rows].astype(np.uint64).sum(axis=1).astype(np.uint32)), what
    assert not miss8[:, n_rows:].any(), what


def check_case(device, case: ce.Case, col_lists, ldm=None):
    """Every column list of ``col_lists`` on ``case``: fresh table, settled, warmed table -- narrow against wide against
    the reference."""
    gpu = ce.OnDevice(device, case)
    if ldm is not None:
        gpu.ldm = ldm
    ref = case.ref
    try:
        for cols in col_lists:
            what = (case.name, list(cols))
            sel = np.asarray(cols)
            logs = LogTable(device, log2_capacity=16)
            n, w = Outputs(gpu, len(cols)), Outputs(gpu, len(cols))
            # ---- a value table that knows nothing: every entry holds its product (NaN for +0.0), bit 2 (and 3)
            launch_narrow(gpu, logs, cols, n)
            fresh = n.download()
            launch_wide(gpu, logs, cols, w)
            same(fresh, w.download(), what + ("fresh",))
            want_p = ce.bits_of(ref.probs[:, sel].T)
            zero = want_p == 0
            assert np.array_equal(fresh[0], np.where(zero, QUIET_NAN, want_p)), what
            nvar_cap = bool((ref.nvar >= cr.NVAR_CAP).any())
            assert fresh[2] == (4 | (8 if zero.any() else 0) | int(nvar_cap)), (what, fresh[2])
            assert np.array_equal(fresh[1][:, :gpu.n_rows], np.where(zero, 255, 0).astype(np.uint8)), what
            check_sums(fresh, gpu.n_rows, what)
            # ---- settle what the narrow launch left, the way the search does
            logs.resolve()
            if fresh[2] & 8:
                n.refill()
                launch_narrow(gpu, logs, cols, n)
                sticky = 0
            else:
                sticky = fresh[2] & 1
                check(lib().gk_compat_patch(device.ctx, logs.handle, n.L.ptr, gpu.n_rows, len(cols), n.miss8.ptr, gpu.ldm,
                                            n.flags.ptr))
                check(lib().gk_miss_colsum(device.ctx, n.miss8.ptr, gpu.ldm, len(cols), n.msum.ptr))
            settled = n.download()
            settled = (settled[0], settled[1], settled[2] | sticky, settled[3])
            # ---- the warmed table: nothing to settle
            n.refill(); w.refill()
            launch_narrow(gpu, logs, cols, n)
            warm = n.download()
            launch_wide(gpu, logs, cols, w)
            same(warm, w.download(), what + ("warm",))
            same(settled, warm, what + ("settled",))
            ce.assert_log_table(gpu, (warm[0].view(np.float64), warm[1], warm[2]), cols)
            assert np.array_equal(warm[1][:, :gpu.n_rows], ref.miss8[:, sel].T), what
            check_sums(warm, gpu.n_rows, what)
            n.close(); w.close()
            logs.close()
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------------------------------ cases
def columnLists(n_allele):
    """Ascending lists of 1, 2, 3, 4, 5, 7 and 8 alleles over ordinals 0, 31, 32, 63, 64 and the last one."""
    last = n_allele - 1
    return [[last], [0, 64], [31, 32, 63], [0, 31, 32, last], [0, 32, 63, 64, last], [0, 1, 31, 32, 63, 64, last],
            [0, 30, 31, 32, 33, 63, 64, last]]


@pytest.fixture(scope="module")
def list_cases():
    return ce.listShapeCases()


def unevenGroupsCase(keep_empty):
    """Rows of 300, 0, 1 and 64 ids side by side, 27 of them (three full groups of 8 and a part of one), every row listed;
    the list-shape gene with its drop flags."""
    rng = np.random.default_rng(8801)
    lists = []
    for k in range(27):
        total = (300, 0, 1, 64)[k % 4]
        ids = rng.permutation(ce.N_TOTAL)[:total]
        n_pos = (total, 0, total // 2, min(total, 63))[(k // 4) % 4]
        lists.append([ids[:n_pos // 3].tolist(), ids[n_pos // 3:n_pos].tolist(), ids[n_pos:].tolist(), []])
    off, ids = cr.packLists(lists)
    return ce.Case("uneven groups", off, ids, ce.N_TOTAL, np.arange(27), ce.listShapeFlags(), ce.VBEG, ce.VEND,
                   ce.listShapeBits(rng), keep_empty=keep_empty)


def longRowCase(n_kept):
    """One row that keeps ``n_kept`` ids (a few more are dropped) between short ones: ids recur, nearly all agree."""
    rng = np.random.default_rng(8900 + n_kept)
    vbeg, n_span, n_total, n_allele = 2, 40, 50, 6
    bits = np.ones((n_span, n_allele), dtype=bool)
    bits[:3] = rng.random((3, n_allele)) < 0.5
    vflag = np.zeros(n_total, dtype=np.uint8)
    vflag[vbeg + 39] = 3
    kept = rng.integers(vbeg + 3, vbeg + 39, n_kept)
    kept[::500] = vbeg + np.arange(len(kept[::500])) % 3
    ids = np.insert(kept, [10, 70, 4000], vbeg + 39)
    lists = [[[vbeg], [], [vbeg + 1], []], [ids.tolist(), [], [], []], [[], [], [], []], [[vbeg + 2], [], [], []]]
    off, flat = cr.packLists(lists)
    return ce.Case(f"{n_kept} kept", off, flat, n_total, np.arange(4), vflag, vbeg, vbeg + n_span, bits)


# ------------------------------------------------------------------------------------------------------------ tests
def test_column_lists_of_a_70_allele_gene(device, list_cases):
    check_case(device, list_cases[0], columnLists(70))


def test_column_lists_of_a_289_allele_gene(device):
    check_case(device, ce.alleleCase(289), columnLists(289))


def test_a_list_of_nine_columns_is_an_argument_error(device, list_cases):
    gpu = ce.OnDevice(device, list_cases[0])
    logs = LogTable(device, log2_capacity=16)
    out = Outputs(gpu, 9)
    try:
        with pytest.raises(GkError, match="at most 8 columns"):
            launch_narrow(gpu, logs, list(range(9)), out)
        launch_narrow(gpu, logs, list(range(8)), out)      # the context serves the corrected call
        device.sync()
    finally:
        out.close(); logs.close(); gpu.close()


@pytest.mark.parametrize("n_rows", [1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 257])
def test_rows_around_groups_waves_and_tiles(device, n_rows):
    """64, 128, 192 and 320 bytes of stride: the pad ends in the middle of a tile's line (``ldm % 128 == 64``) and at its
    end."""
    check_case(device, ce.rowCase(n_rows, n_allele=8), [[0, 1, 2, 3, 4, 5, 6, 7], [1, 4, 6]])


def test_a_stride_beyond_the_last_tile(device):
    """129 rows in a stride of 448: the pad runs over a tile nobody computes."""
    check_case(device, ce.rowCase(129, n_allele=8), [[0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6, 7]], ldm=448)


def test_257_tiles_and_one_row(device):
    case = ce.rowCase(128 * 257 + 1, n_allele=5)
    assert (len(case.rows) + 63) // 64 * 64 % 128 == 64
    check_case(device, case, [[0, 1, 2, 3, 4], [1, 3]])


@pytest.mark.parametrize("k", range(5))
def test_list_shapes_and_drop_flags(device, list_cases, k):
    """Lengths 0 - 300, the sign boundary at 0 / 1 / 63 / 64 / 65, foreign and novel ids on both sides, one ordinal positive
    here and negative there, 0 / 1 / 4 / 5 / 63 / 64 kept per chunk, a chunk dropped whole, a row that keeps nothing --
    with both values of keep_empty (cases 0 and 1), without flags, without ids."""
    check_case(device, list_cases[k], [[0, 31, 32, 69], [0, 1, 2, 3, 33, 63, 64, 65]])


@pytest.mark.parametrize("keep_empty", [False, True])
def test_groups_of_rows_that_differ_most(device, keep_empty):
    check_case(device, unevenGroupsCase(keep_empty), [[0, 69], [0, 31, 32, 33, 63, 64, 65, 69]])


def test_counts_around_100_subnormal_products_and_zero(device):
    """Byte 255 from 100 mismatches on and bit 0; subnormal products in place on a fresh table; +0.0 before its log10 is
    known stores a NaN and raises bit 3."""
    case = ce.numericCase(cr.HEAVY_GENE)
    ref = case.ref
    assert ref.miss[0].tolist() == cr.HEAVY_COUNTS
    tiny = np.finfo(np.float64).tiny
    # alleles by their count in the long rows: 0, 98 - 101, 103, 107, 108 (subnormal products at 103 and 107, +0.0 at 108);
    # 102, 109, 120 and 254 - 300 (every long row +0.0); 99 alone (bit 0 stays clear)
    first, second, alone, four = [0, 4, 5, 6, 7, 9, 10, 11], [8, 12, 13, 14, 15, 16, 17], [5], [0, 5, 10, 11]
    p = ref.probs[:, first]
    assert ((p > 0) & (p < tiny)).any() and (p == 0).any() and ref.flag0
    assert {98, 99, 255} <= set(ref.miss8[:, first].ravel().tolist()) and ref.miss[:, alone].max() == 99
    p = ref.probs[:, four]
    assert ((p > 0) & (p < tiny)).any() and (p == 0).any()      # the same for the kernel of at most four columns
    check_case(device, case, [first, second, alone, four])


def test_a_gene_capped_at_99_mismatches_leaves_bit_0_clear(device):
    case = ce.numericCase(cr.CAPPED_GENE)
    assert case.ref.miss.max() == 99 and not case.ref.flag0
    check_case(device, case, [list(range(min(8, case.n_allele)))])


@pytest.mark.parametrize("n_kept", [4095, 4096])
def test_a_row_of_4096_kept_ids_raises_bit_0(device, n_kept):
    case = longRowCase(n_kept)
    assert case.ref.nvar.max() == n_kept and case.ref.miss.max() < cr.MISS_CAP
    assert case.ref.flag0 == (n_kept >= cr.NVAR_CAP)
    check_case(device, case, [[0, 1, 2, 3, 4, 5], [2]])


def test_in_the_search_eight_columns_take_the_new_kernel_and_nine_the_old(device):
    """``gk_sample_search`` on a table job over 8 and over 9 of a gene's alleles: the kernels the context timed, and the
    search results of the whole table."""
    run, n_allele, close = xc._tableAndSearch(device, 7150001, (12, 13), 600)
    assert n_allele >= 10
    offered = [1, 3, 4]
    want = run(None, offered)
    for n_cols, kernel, other in ((8, "compat_rows8", "compat_kernel"), (9, "compat_kernel", "compat_rows8")):
        listed = np.arange(n_cols, dtype=np.int32)
        device.sync()
        device.profEnable(True)
        device.profCollect()
        try:
            got = run(listed, offered)
            device.sync()
            prof = device.profCollect()
        finally:
            device.profEnable(False)
        assert prof.get(kernel, (0, 0.0))[0] >= 1 and other not in prof, (n_cols, sorted(prof))
        assert ("cols_bytes" in prof) == (n_cols == 8), (n_cols, sorted(prof))
        assert len(got) == len(want) == 2
        for x, y in zip(got, want):
            for f in xc.FIELDS:
                assert np.array_equal(x[f], y[f]), (n_cols, f)
    close()


# ------------------------------------------------------------------------------------------------------------ driver
DRIVER_SEEDS = (7110002, 7110003)      # their candidate unions hold 1, 3 and 42 / 23, 1 and 4 alleles


def typeDriverCases(out_path: str) -> None:
    """Child process: exon-first typing of the small synthetic samples of tests/test_gpu_exonfirst_columns.py -> one .npz
    with every step's arrays and a JSON record of the calls and of the kernels that wrote the tables."""
    sys.path.insert(0, ROOT)
    from kir_graph_amd import _lib, packed
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.index import GkIndex
    from kir_graph_amd.kir_typing import selectKirTypingModel
    os.environ["GK_SEARCH"] = "bound"
    dev = _lib.Device(0)
    arrays, record = {}, []

    def typeOne(seed, recording):
        sidx, gene_cn, lines, top_n = xc.makeCase(seed, False)
        gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
        rec, table, _, counts = packed.packText([("\n".join(lines) + "\n").encode()], gidx)
        tab = Tabulation(DeviceIndex(dev, gidx), dev.put(rec), spill=counts.get("spill"))
        data = SampleData(tab, gidx, None, ins_strings=table.strings)
        typer = selectKirTypingModel("exonfirst_1", data, top_n=top_n, variant_correction=True)
        calls, warnings = typer.typing(gene_cn)
        if recording:
            columns = {}
            for gene in gene_cn:
                columns[gene] = dict(getattr(typer, "exon_info", {}).get(gene, {})).get("table_columns")
                for k, step in enumerate(typer._result.get(gene) or []):
                    for f in xc.FIELDS:
                        arrays[f"{seed}/{gene}/{k}/{f}"] = np.asarray(getattr(step, f))
            record.append({"seed": seed, "calls": list(calls), "warnings": list(warnings), "columns": columns})
        tab.close()

    typeOne(DRIVER_SEEDS[0], False)      # makes the contexts the typing uses; from here on they record their launches
    for d in _lib.Device.instances:
        d.call_log = []
        d.profEnable(True)
        d.profCollect()
    for seed in DRIVER_SEEDS:
        typeOne(seed, True)
    labels = sorted({c[0] for d in _lib.Device.instances for c in d.call_log or [] if c[0].startswith("compat_")})
    kernels = sorted({k for d in _lib.Device.instances for k in d.profCollect() if k.startswith(("compat_", "cols_"))})
    np.savez(out_path, record=np.array(json.dumps({"cases": record, "labels": labels, "kernels": kernels})), **arrays)


def _child(tmp_path, name, hooks):
    out = str(tmp_path / f"{name}.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("GK_TEST_HOOKS", None)
    if hooks:
        env["GK_TEST_HOOKS"] = hooks
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "type", out], env=env, capture_output=True, text=True,
                          timeout=600)
    assert done.returncode == 0, done.stderr[-3000:]
    got = np.load(out)
    return json.loads(str(got["record"])), got


def test_exon_first_typing_is_the_same_with_the_kernel_of_the_wide_tables(device, tmp_path):
    rec_n, arr_n = _child(tmp_path, "narrow", None)
    rec_w, arr_w = _child(tmp_path, "wide", "wide_compat")
    assert rec_n["cases"] == rec_w["cases"]
    narrow = [n for case in rec_n["cases"] for n in case["columns"].values() if n is not None and 0 < n <= 8]
    assert narrow, rec_n["cases"]                                   # some gene's candidates were at most 8 alleles
    assert "compat_rows8" in rec_n["labels"] and "compat_rows8" not in rec_w["labels"]
    assert {"compat_rows8", "cols_bytes"} <= set(rec_n["kernels"]) and rec_w["kernels"] == ["compat_kernel"]
    keys = sorted(k for k in arr_n.files if k != "record")
    assert keys and keys == sorted(k for k in arr_w.files if k != "record")
    for k in keys:
        a, b = arr_n[k], arr_w[k]
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), k


if __name__ == "__main__":
    if sys.argv[1] == "type":
        typeDriverCases(sys.argv[2])

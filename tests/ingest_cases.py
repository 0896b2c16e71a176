"""Inputs and the comparison shared by the tests of the split ingest routes (test_ingest_plain_host.py,
test_gpu_ingest_decode.py): the awkward-record files of test_host.py's
``test_bam_binary_hand_over_equals_text_path_on_awkward_records`` (its case list, copied), and ``outcome``: everything
a pack call leaves -- records, strings, pair_lines, counts, spill -- or the kind, line and reason of its exception."""
from kir_graph_amd import synth
from kir_graph_amd.index import GkIndex


def outcome(run):
    """``run()`` -> (records, table, pair_lines, counts) as a comparable tuple; the decode report and the device
    records, which only the split routes add, come back beside it."""
    try:
        rec, table, pl, counts = run()
    except Exception as e:    # noqa: BLE001 -- the kind, the line and the reason are what is compared
        return (type(e).__name__, str(e).split(":")[0].split()[-1], str(e).split(":", 1)[-1]), None, None
    counts = dict(counts)
    decode, mates = counts.pop("decode", None), counts.pop("mates", None)
    spill = counts.pop("spill", None)
    spill = (spill[0].tobytes(), spill[1].tolist()) if spill else None
    return ("ok", rec.tobytes(), list(table.strings), pl.tolist(), counts, spill), decode, mates


def smallIndex():
    sidx = synth.makeIndex(seed=5, n_genes=3, var_range=(200, 300), allele_range=(10, 20))
    return sidx, GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)


def headerOf(sidx, order="queryname"):
    return [f"@HD\tVN:1.0\tSO:{order}"] + [f"@SQ\tSN:{g}\tLN:{len(sidx.backbone[g])}" for g in sidx.genes]


def edit(lines, k, **kw):
    """Pair k with fields of its first mate replaced (cigar / seq / md / zs / nm)."""
    f = lines[2 * k].split("\t")
    if "cigar" in kw:
        f[5] = kw["cigar"]
    if "seq" in kw:
        f[9] = kw["seq"]
        f[10] = "I" * len(f[9]) if f[9] != "*" else "*"
    for i in range(11, len(f)):
        for tag, key in (("MD:Z:", "md"), ("Zs:Z:", "zs"), ("NM:i:", "nm")):
            if f[i].startswith(tag) and key in kw:
                f[i] = tag + str(kw[key])
    f = [c for c in f if not (c.startswith("Zs:Z:") and kw.get("zs") == "")]
    lines[2 * k] = "\t".join(f)


def awkwardFiles(tmp_path):
    """[(tag, path of the BAM file, expected kind or None)] and the index they are packed against."""
    from bamwriter import samToBam
    sidx, gidx = smallIndex()
    sample = synth.makeSample(sidx, seed=21, n_pairs=400)
    records = synth.toSamLines(sample)
    header = headerOf(sidx)
    n = 150
    files = []

    def write(lines, tag, kind=None):
        path = str(tmp_path / f"{tag}.bam")
        samToBam(header + lines, path, block=20000)
        files.append((tag, path, kind))

    # shapes that must come out as records: clips (short, long, too many ops to keep), long runs, many ops
    good = list(records)
    edit(good, 3, cigar=f"10S{n - 10}M", md=str(n - 10), zs="", nm=0)
    edit(good, 5, cigar=f"5S{n - 12}M7S", md=str(n - 12), zs="", nm=0)
    edit(good, 7, cigar="1S" + "1M1I" * 8 + f"{n - 17}M", md=str(n - 17 + 8), zs="", nm=0)      # 18 ops, clipped
    edit(good, 9, cigar="2M1I" * 6 + f"{n - 18}M", md=str(n - 18 + 12), zs="", nm=0)            # 13 ops, 6 strings
    edit(good, 11, cigar=f"{n}M", md="0A0C0G" + str(n - 3), seq="TTT" + "A" * (n - 3), zs="", nm=3)
    write(good, "good", "ok")
    # shapes the reference raises on, or that only the text walk spells right: one file each, the bad pair in the middle
    cases = {
        "hard_clip": dict(cigar=f"5H{n}M", md=str(n), zs="", nm=0),          # H: NotImplementedError
        "pad": dict(cigar=f"70M2P{n - 70}M", md=str(n), zs="", nm=0),
        "eq_single_digit": dict(cigar=f"{n - 5}M5=", md=str(n - 5), zs="", nm=0),   # "5=" is skipped by (\d+)(\w)
        "eq_two_digits": dict(cigar=f"{n - 15}M15=", md=str(n - 15), zs="", nm=0),  # "15=" reads as op '5' of length 1
        "x_op": dict(cigar=f"{n - 5}M5X", md=str(n - 5), zs="", nm=0),
        "splice": dict(cigar=f"70M100N{n - 70}M", md=str(n), zs="", nm=0),
        "no_cigar": dict(cigar="*", md=str(n), zs="", nm=0),
        "no_seq": dict(cigar=f"{n}M", seq="*", md=str(n), zs="", nm=0),
        "short_cigar": dict(cigar=f"{n - 1}M", md=str(n - 1), zs="", nm=0),
        "md_short": dict(cigar=f"{n}M", md=str(n - 1), zs="", nm=0),
        "md_same_base": dict(cigar=f"{n}M", md="0A" + str(n - 1), seq="A" * n, zs="", nm=1),
        "md_no_deletion": dict(cigar=f"70M2D{n - 70}M", md=str(n), zs="", nm=0),
        "zs_unused": dict(cigar=f"{n}M", md=str(n), zs="3|S|hv1", nm=0),
        "too_many_ops": dict(cigar="2M1I" * 8 + f"{n - 24}M", md=str(n - 24 + 16), zs="", nm=0),   # 17 ops, not clipped
        "long_insert_run": dict(cigar=f"4M4096I{n - 4}M", md=str(n), zs="", nm=0),
    }
    expected = {"splice": "NotImplementedError", "hard_clip": "NotImplementedError", "md_short": "AssertionError",
                "md_same_base": "AssertionError", "too_many_ops": "ok"}
    for tag, kw in cases.items():
        lines = list(records)
        edit(lines, 200, **kw)
        write(lines, tag, expected.get(tag))
    # beyond the wide format too: the capacity error stays
    lines = list(records)
    edit(lines, 200, cigar="1M1I" * 70 + f"{n - 140}M", md=str(n - 70), zs="", nm=0)     # 141 ops
    write(lines, "beyond_wide", "PackCapacityError")
    return files, gidx

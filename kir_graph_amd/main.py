"""
``graphkir`` command line -- drop-in for the typing stages of ``graphkir/main.py``.

Same flags, defaults, file naming and TSV schemas (createParser 258-420, main 423-606,
readMapping 124-168, alleleTyping 171-220, getCommonName 223-250).  What differs:

* tabulation, read depth, copy-number fit and allele typing run on the GPU; a sample's tabulation
  is handed to typing in memory (the ``.variant.json`` is still written unless
  ``--no-variant-json``);
* additive flags: ``--alignment`` (use existing name-collated SAM/BAM instead of running hisat2),
  ``--no-variant-json``, ``--ingest-decode device`` (the plain pairs of a ``.bam`` sample decoded by a kernel,
  csrc/gk_ingest_decode.hip), ``--novel-discovery`` (novel_discover.py after typing: ``{result}.novel.*``); ``--allele-strategy`` also accepts ``pv`` (= full) and maps ``report`` to
  the EM strategy (the reference forwards ``report`` to a factory that rejects it, main.py:192);
* launched with RANK / WORLD_SIZE / LOCAL_RANK set (``torchrun`` or any launcher) the samples are sharded over
  the ranks (one GPU each, largest inputs first); ``--cn-cohort`` then pools the gene depths with one
  all-gather (``cohort.Comm`` -> ``gk_allgather_f64``, RCCL), rank 0 merges the outputs;
* ``--ranks N`` starts the N rank processes itself (no launcher needed);
* a sample is typed and released as soon as its copy numbers are known (memory does not grow with the cohort);
* index building, WGS extraction and plotting are outside this build: the index files must exist.
"""
from __future__ import annotations

import argparse
import os
import logging
from pathlib import Path

import numpy as np
import pandas as pd

from . import cohort
from .call_report import CALL_REPORTS, callReport
from .external_tools import setEngine
from .hisat2 import (ParkedRecords, SampleData, extractVariant, extractVariantFromPacked, extractVariantFromText,  # noqa: F401
                     packAlignments, readExons, readPair,
                     saveReadsToBam, writeCompact, writeCompactRecords,
                     writeReadsAndVariantsData, writeSampleJson)
from .index import GkIndex
from .kir_cn import filterDepth, loadCN, predictSamplesCN
from .kir_typing import defaultDevice, selectKirTypingModel
from .samtools_utils import depthOfSample, readLocusLengths
from .utils import testHook, getThreads, logger, mergeAllele, mergeCN, setThreads


def getCommonName(r1: str, r2: str) -> str:
    """Longest common dot-separated prefix of the two read file names (main.py:223-250)."""
    name = ""
    for s1, s2 in zip(r1.split("."), r2.split(".")):
        if s1 != s2:
            return name
        name = name + "." + s1 if name else s1
    return name


def replaceParentFolder(filename: str, new_folder: str) -> str:
    return str(Path(new_folder) / Path(filename).name)


def hisatMap(index: str, f1: str, f2: str, output_file: str, threads: int = 1) -> None:
    """External aligner, unchanged from the reference (hisat2.py:68-92); needs hisat2 + samtools."""
    from .external_tools import runTool
    assert output_file.endswith(".bam")
    name = output_file.rsplit(".", 1)[0]
    runTool("hisat", ["hisat2", "--threads", str(threads), "-x", index, "-1", f1, "-2", f2,
                      "--no-spliced-alignment", "--max-altstried", "64", "--haplotype", "-S", f"{name}.sam"])
    runTool("samtools", ["samtools", "sort", f"-@{threads}", f"{name}.sam", "-o", f"{name}.bam"])
    runTool("samtools", ["samtools", "index", f"-@{threads}", f"{name}.bam"])


def mapSamples(names, reads, index, index_ref, exon_region_only=False, alignments=None, write_json=True,
               keep_records=False, keep_text=False, cn_bootstrap=None, ingest_decode="host"):
    """Graph mapping (external) -> tabulation (GPU) -> depth (GPU), one sample at a time (main.py:124-168).

    Yields ``(alignment file, "{name}.variant", SampleData, depth file)`` per sample, in order.  When a sample
    is yielded its by-products are on disk and its depth is computed, so what only they needed -- the SAM
    text of the pairs and the packed records in HBM -- has been released: the consumer holds the CSR of the
    tabulation only (and closes it after typing), whatever the size of the cohort.  ``keep_records``: the packed
    records stay in HBM with the sample (``--cn-cohort`` parks a sample as its compact records, ``ParkedRecords``).
    ``keep_text``: the SAM lines of the pairs stay with the sample (``--novel-discovery`` writes them grouped).
    ``cn_bootstrap`` (``--cn-bootstrap``): ``{"n_boot", "seed", "select_mode"}`` and optionally ``"samples"``, one flag per
    sample -- right after a flagged sample's depth, while its records are still in HBM, the read bootstrap of its gene
    depths is written next to the depth file (``{depth_name}.boot.tsv``, ``cn_bootstrap.bootstrapGeneDepths``).
    ``ingest_decode`` (``--ingest-decode``): ``"device"`` decodes the plain pairs of a ``.bam`` sample in a kernel
    (``hisat2.packAlignments(decode="device")``) and tabulates from the records that kernel left in HBM."""
    gk = GkIndex.load(index_ref)
    gene_len = readLocusLengths(index_ref)
    dev = defaultDevice()
    from .engine import DeviceIndex
    dindex = DeviceIndex(dev, gk)
    # the staging contexts of the sample pipeline (cohort.stagingContexts, the ones bench.py stages with): the records go
    # to HBM on the copier's stream, the tabulation and the depth run on a high-priority stream of their own -- beside the
    # typing lanes (cohort.SampleTyper), which are typing the samples before this one
    copier, ingest = cohort.stagingContexts(dev)
    ahead = max(1, int(testHook("ingest_ahead") or 3))       # samples packed ahead of the typing (the hook: tools/ingest_cli_sweep.sh)
    # --ingest-decode device: prepare() runs on `ahead` helper threads, and a context serves one thread at a time -- each
    # call checks one of `ahead` worker contexts (beyond the staging ones) out of this queue and returns it afterwards.
    # Only the FREE of a sample's device records crosses threads: they come from the decoder context's pool and go back
    # to it from this thread (releaseInputs) while a helper may be packing on that context -- the pool takes frees from
    # any thread (gk_pool_free); nothing else of a decoder context is touched from here
    import queue
    decoders: queue.Queue = queue.Queue()
    if ingest_decode == "device":
        for i in range(ahead):
            decoders.put(dev.worker(cohort.sampleLanes() + 2 + i))

    def prepare(k: int):
        """External mapping (when needed) + native packing of sample k: host work, off the GPU's path."""
        name = names[k] + "." + index.replace(".", "_").replace("/", "_")
        if alignments:
            source = alignments[k]
        else:
            logger.info(f"[Graph] Run graph mapping on index {index} ({name})")
            hisatMap(index, reads[k][0], reads[k][1], name + ".bam", threads=getThreads())
            source = name + ".bam"
        pack = None
        if source.endswith((".sam", ".sam.gz")) or testHook("bam_reader") != "samtools":
            # SAM text, or BAM decoded + name-collated natively (packed.bamChunks / packBam), packed natively
            if ingest_decode == "device":
                decoder = decoders.get()
                try:
                    pack = packAlignments(source, gk, keep_text=write_json, decode="device", dev=decoder)
                finally:
                    decoders.put(decoder)
            else:
                pack = packAlignments(source, gk, keep_text=write_json)
            # the records cross PCIe in compact form (~30 bytes per mate instead of 128), like the bench's steps (with
            # the records in HBM already, the compact form is still what the hand-off file holds)
            from .packed import CompactMates
            pack["compact"] = CompactMates(pack["records"], threads=2)
        return name, source, pack

    # the next sample is mapped / packed on a helper thread while this one is tabulated and written out
    # (three samples ahead on three threads: the serial stretches of one ingest leave cores to the others)
    from concurrent.futures import ThreadPoolExecutor
    writer = ThreadPoolExecutor(max_workers=2, thread_name_prefix="gk-write")   # compact hand-off files, off this thread
    writes = []
    try:
        yield from _mapLoop(names, prepare, ahead, gk, gene_len, (copier, ingest), dindex, index_ref, exon_region_only,
                            write_json, writer, writes, keep_records, keep_text, cn_bootstrap)
    finally:
        for w in writes:
            w.result()          # every hand-off file is complete (and any write error surfaces) before we return
        writer.shutdown()


def _mapLoop(names, prepare, ahead, gk, gene_len, staging, dindex, index_ref, exon_region_only, write_json, writer, writes,
             keep_records=False, keep_text=False, cn_bootstrap=None):
    copier, dev = staging
    warned = False
    for k, (name, source, pack) in enumerate(cohort.prefetched(range(len(names)), prepare, depth=ahead, workers=ahead)):
        name += ".variant"
        packed_records = pack is not None
        logger.info(f"[Graph] Filter mapping ({name})")
        handed_off = False
        if pack is not None:
            # pinned records -> HBM on the copier's stream: the compact words as they are, or the 128-byte records
            compact = pack.pop("compact", None)
            mates = pack.pop("mates", None)      # --ingest-decode device: the 128-byte records are in HBM already
            if mates is None:
                mates = compact.toDevice(copier, wait=True) if compact is not None else copier.put(pack["records"])
            data = extractVariantFromPacked(pack, gk, dev=dev, dindex=dindex, mates=mates)
            if compact is not None and not write_json and os.environ.get("GK_HANDOFF", "always") != "lazy":
                # the hand-off as the compact records that are in host memory anyway (70 MB for 2 M reads) instead of the
                # tabulated lists fetched back from the device (250 MB): hisat2.writeCompactRecords / loadCompact
                writes.append(writeCompactRecords(compact, pack, data.tab.novel_base, gk, name + ".npz",
                                                  index_ref=index_ref, background=writer))
                handed_off = True
        else:   # BAM name-collated through samtools like the reference (hisat2.readBam)
            data = extractVariant(readPair(source), gk, dev=dev, dindex=dindex)
        del pack
        if write_json:
            writeSampleJson(data, name + ".json")
            # the reference also rewrites the filtered pairs as BAM (hisat2.py:936-940)
            saveReadsToBam(data, name, source)
            saveReadsToBam(data, name + ".no_multi", source, filter_multi_mapped=True)
        elif handed_off:
            pass
        elif os.environ.get("GK_HANDOFF", "always") != "lazy":
            # compact hand-off instead: CSR + string table, no SAM text (hisat2.writeCompact).  GK_HANDOFF=lazy: only
            # for a sample that has to leave HBM before it is typed (main(): the --cn-cohort retention budget) -- a
            # cohort of 64 x 5 M reads would otherwise leave 42 GB of files that nothing reads
            writes.append(writeCompact(data, name + ".npz", index_ref=index_ref, background=writer))
        depth_name = name + ".no_multi"
        logger.info(f"[Graph] Calculate read depth to {depth_name}.depth.tsv")
        depthOfSample(data, gene_len, depth_name + ".depth.tsv", want_frame=False)
        depth_name += ".depth"
        if exon_region_only:
            logger.info(f"[Graph] Filter exon read to {depth_name}.exon.tsv")
            filterDepth(depth_name + ".tsv", depth_name + ".exon.tsv", readExons(index_ref))
            depth_name += ".exon"
        if cn_bootstrap and (cn_bootstrap.get("samples") is None or cn_bootstrap["samples"][k]):
            from .cn_bootstrap import bootstrapGeneDepths, hasRecords, writeDepthBootstrap
            if packed_records and hasRecords(data):
                logger.info(f"[CN] Read bootstrap of the gene depths to {depth_name}.boot.tsv")
                boot = bootstrapGeneDepths(data, gene_len, cn_bootstrap["n_boot"], seed=cn_bootstrap["seed"],
                                           select_mode=cn_bootstrap["select_mode"],
                                           regions=readExons(index_ref) if exon_region_only else None)
                writeDepthBootstrap(boot, depth_name + ".boot.tsv")
            elif not warned:
                logger.warning("[CN] cn bootstrap: a sample arrived without packed records (alignments read as text pairs); "
                               "no .boot.tsv for it")
                warned = True
        releaseInputs(data, keep_records, keep_text)
        yield source, name, data, depth_name + ".tsv"


def releaseInputs(data: SampleData, keep_records: bool = False, keep_text: bool = False) -> None:
    """Drop what only the by-products and the depth needed: the SAM text of the pairs (host; unless ``keep_text``) and
    the packed records (HBM: the compact words, ~60 B per pair, or 256 B per pair where a sample arrived as 128-byte
    records; unless ``keep_records``).  The tabulation's lists stay for typing."""
    if not keep_text:
        data.pairs_text = None
    data._reads = None
    mates = getattr(data.tab, "mates", None)
    if mates is not None and not keep_records:
        mates.free()
        data.tab.mates = None


def readMapping(names, reads, index, index_ref, exon_region_only=False, alignments=None, write_json=True):
    """List form of ``mapSamples`` with the reference's return value (bam files, processed, depth files)."""
    bam_files, processed, depth_files = [], [], []
    for source, name, data, depth_file in mapSamples(names, reads, index, index_ref, exon_region_only,
                                                     alignments, write_json):
        bam_files.append(source)
        processed.append((name, data))
        depth_files.append(depth_file)
    return bam_files, processed, depth_files


def typingSuffix(name: str, cn_file: str, method: str) -> str:
    """``.cn<what the CN file's name adds to the sample's>.<method>`` (main.py:182-187)."""
    if method == "exonfirst":
        method += "_1"
    return ".cn" + cn_file[len(getCommonName(name, cn_file)):].replace("/", "_").replace(".", "_") + "." + method


def _plainField(x) -> bool:
    """A cell pandas' ``to_csv`` (tab separated, minimal quoting) writes as it is."""
    return isinstance(x, str) and not any(c in x for c in '\t"\n\r')


def writeTyping(name: str, typer, called_alleles: list[str], warning_genes: list[str]) -> str:
    """``{name}.tsv`` (name, alleles, warnings) and ``{name}.possible.tsv`` of one typed sample (main.py:203-219).

    The bytes are pandas' (``DataFrame.to_csv(sep="\\t", index=False)``, what the reference calls); for plain cells they
    are written directly -- the two frames cost 2.4 ms of interpreter time per sample, a third of the sample's GPU time
    with three typing lanes behind one interpreter lock -- anything else (a quote or a tab in a name, no rows) goes
    through pandas."""
    alleles, warnings = "_".join(called_alleles), "_".join(warning_genes)
    if all(_plainField(x) for x in (name, alleles, warnings)):
        with open(name + ".tsv", "w") as f:
            f.write(f"name\talleles\twarnings\n{name}\t{alleles}\t{warnings}\n")
    else:
        pd.DataFrame({"name": [name], "alleles": [alleles], "warnings": [warnings]}).to_csv(name + ".tsv", sep="\t", index=False)
    try:
        possible = typer.getAllPossibleTyping()       # reads the ranked results on the host only
    except NotImplementedError:      # EM strategy has no possible-set table (kir_typing.py:63-68)
        possible = []
    cols: list[str] = []
    for row in possible:                  # the frame's columns: keys in order of first appearance
        for k in row:
            if k not in cols:
                cols.append(k)
    plain = bool(possible) and cols[:3] == ["gene", "rank", "value"] and all(
        _plainField(r["gene"]) and isinstance(r["rank"], int) and isinstance(r["value"], (float, np.floating)) and
        np.isfinite(r["value"]) and all(_plainField(r[k]) and r[k] != "" for k in r if k not in ("gene", "rank", "value"))
        for r in possible)
    if plain:
        lines = ["\t".join(cols)]
        for r in possible:
            cells = [r["gene"], str(r["rank"]), repr(float(r["value"]))] + [r.get(k, "") for k in cols[3:]]
            lines.append("\t".join(cells))
        with open(name + ".possible.tsv", "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        pd.DataFrame(possible).fillna("").to_csv(name + ".possible.tsv", index=False, sep="\t")
    return name + ".tsv"


def writeConfidence(name: str, bootstrap: dict) -> str:
    """``{name}.confidence.tsv`` of one sample typed with ``--em-bootstrap``: per allele of every gene's EM report the
    point values, the replicates' mean / sd / 2.5 % / 97.5 % abundance and the support of the call
    (``typing_em.confidenceText``)."""
    from .typing_em import confidenceText
    with open(name + ".confidence.tsv", "w") as f:
        f.write(confidenceText(bootstrap))
    return name + ".confidence.tsv"


def writeCallReport(key: str, name: str, entries: dict, **options) -> list[str]:
    """The files of the per-call report ``key`` (``call_report.CALL_REPORTS``: ``"call_fit"`` writes ``{name}.fit.tsv``, ...)
    of one sample typed by a likelihood strategy, from the typer's ``{gene: entry}``; ``options``: the report's keywords
    (``call_coverage_depth`` asks for ``{name}.coverage.depth.tsv`` as well).  A gene whose report could not be made (None)
    is left out: a sample without records in HBM gets the headers alone."""
    entries = {gene: e for gene, e in entries.items() if e is not None}
    files = []
    for suffix, text, asked in callReport(key).files:
        if asked is None or options.get(asked):
            files.append(name + suffix)
            with open(files[-1], "w") as f:
                f.write(text(entries))
    return files


def discoverAfterTyping(typer, called_alleles: list[str], name: str, result: str, index_ref: str) -> None:
    """Novel-variant discovery of one typed sample, on its tabulation in HBM (novel_discover.discoverSample):
    ``{result}.novel.variant.tsv / .tsv / .fa / .bam / .txt``, the reads piled up from ``{name}.no_multi.bam``."""
    from .novel_discover import discoverSample
    data = typer._data
    tab = typer._context()[0]
    output = result + ".novel"
    logger.info(f"[Novel] Discover novel variants ({output})")
    with open(output + ".txt", "w") as descr:
        discoverSample(data, list(called_alleles), index_ref, name + ".no_multi.bam", output, novel_descr=descr, tab=tab)
    data.pairs_text = None


def sampleTyper(method: str, release: bool = True, novel_index: str | None = None, bootstrap: int = 0,
                bootstrap_seed: int = 2022, **call_options) -> "cohort.SampleTyper":
    """The typing stage of this process (``cohort.SampleTyper``: the sample lanes, search slots, urgent preamble and
    blocking waits that ``bench.py`` measures), finishing every sample the reference's way: its two files written, its
    tabulation released.  Submit ``(SampleData or hand-off file, copy numbers, (name, cn_file))``.
    ``novel_index`` (``--novel-discovery``): the index prefix; every typed sample then goes through novel_discover.py
    (``{result}.novel.*``, typingNovelWrap of the reference's research/kg_main.py) before its tabulation is released.
    ``bootstrap`` > 0 (``--em-bootstrap``, EM strategy): the typer also runs that many read-bootstrap replicates and the
    finish step writes ``{result}.confidence.tsv``.
    ``call_options``: the keywords of the per-call reports of the likelihood strategies (``call_report.CALL_REPORTS``;
    ``callReportArgs`` makes them from the command line): ``call_bootstrap`` > 0, ``call_fit``, ``call_alternatives``,
    ``call_dosage``, ``call_coverage`` and their options.  The typer gets the keywords of the reports that are switched
    on, and the finish step writes their files: ``{result}.call_confidence.tsv``, ``.fit.tsv``, ``.alternatives.tsv``,
    ``.dosage.tsv``, ``.coverage.tsv`` (with ``call_coverage_depth`` also ``.coverage.depth.tsv``).  ``call_coverage``
    needs ``gene_len``, the backbone lengths, and the sample's records still in HBM (``mapSamples(keep_records=True)``)."""
    unknown = set(call_options) - {o.name for report in CALL_REPORTS for o in report.options}
    if unknown:
        raise TypeError(f"sampleTyper() got an unexpected keyword argument {sorted(unknown)[0]!r}")
    reports = [report for report in CALL_REPORTS if report.switchedOn(call_options)]

    def finish(typer, called_alleles, warning_genes, item):
        name, cn_file, source = item
        result = name + typingSuffix(name, cn_file, method)
        try:
            if novel_index is not None:
                discoverAfterTyping(typer, called_alleles, name, result, novel_index)
        finally:       # a failed discovery still leaves the sample's typing files written and its HBM released
            if release or not isinstance(source, SampleData):      # done with this sample: free its HBM
                tab = typer._data.tab
                mates = getattr(tab, "mates", None)
                if mates is not None:
                    mates.free()
                    tab.mates = None
                tab.close()
            logger.info(f"[Allele] {called_alleles} ({name})")
            written = writeTyping(result, typer, called_alleles, warning_genes)
            if bootstrap > 0:
                writeConfidence(result, typer.bootstrap)
            for report in reports:
                writeCallReport(report.key, result, getattr(typer, report.key), **call_options)
        return written

    extra = {"bootstrap": bootstrap, "bootstrap_seed": bootstrap_seed} if bootstrap > 0 else {}
    for report in reports:
        extra.update(report.typerKeywords(call_options))
    return cohort.SampleTyper(method, finish=finish, **extra)


def alleleTyping(processed_bam, cn_files: list[str], method: str = "full", release: bool = False) -> list[str]:
    """Allele typing of every sample; writes ``{name}{suffix}.tsv`` and ``.possible.tsv`` (171-220).

    ``processed_bam`` entries are names (the ``.json`` next to them is loaded) or (name, SampleData);
    ``release``: close every SampleData's tabulation once its results are taken (the pipeline does).
    The samples go through the process's typing lanes (``sampleTyper``): up to GK_SAMPLE_LANES at a time, results in
    order -- the reference types them one after the other (main.py:178-220), the files are the same.
    As many samples again wait behind the lanes: the results are taken in order, so with only ``lanes`` samples handed
    in, a lane that finishes before the oldest sample has nothing to start until that one is done and collected here
    (the samples are tabulated already or come from files: one that waits holds nothing more than it held before)."""
    allele_files = []
    with sampleTyper(method, release=release) as lanes:
        for entry, cn_file in zip(processed_bam, cn_files):
            name, source = entry if isinstance(entry, tuple) else (entry, entry + ".json")
            logger.debug(f"[Allele] Allele typing ({method}) with CN {cn_file} ({name})")
            lanes.submit(source, (lambda f=cn_file: loadCN(f)), (name, cn_file, source))
            if lanes.inFlight() >= 2 * lanes.lanes:
                allele_files.append(lanes.next())
        allele_files.extend(lanes.drain())
    return allele_files


class _Parser(argparse.ArgumentParser):
    """Rejects flag combinations that cannot work, at argument time."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        if getattr(ns, "novel_discovery", False) and getattr(ns, "no_variant_json", False):
            self.error("--novel-discovery needs the {name}.variant.no_multi.bam that --no-variant-json does not write")
        return ns, rest


def _cnBootstrapCount(text: str) -> int:
    """``--cn-bootstrap N``: a count outside 1 .. 10000 is a parser error."""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not 1 <= n <= 10000:
        raise argparse.ArgumentTypeError(f"the number of replicates must lie in 1 .. 10000, got {n}")
    return n


def createParser() -> argparse.ArgumentParser:
    p = _Parser(description="Run Graph-KIR (MI355X typing path)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--thread", default=1, help="Number of threads")
    p.add_argument("--engine", default="local", choices=["podman", "docker", "singularity", "local"],
                   help="How external tools (hisat2 / samtools) are run; only 'local' is supported here.")
    p.add_argument("--log-level", default="INFO", choices=logging._nameToLevel.keys(), help="Set the log level")
    p.add_argument("--r1", action="append", help="Paths to paired-end Read 1 FASTQ files")
    p.add_argument("--r2", action="append", help="Paths to paired-end Read 2 FASTQ files (in order)")
    p.add_argument("--input-csv", help="CSV with columns name, r1, r2 [, cnfile]")
    p.add_argument("--output-folder", help="Output folder (default: same folder as input reads)")
    p.add_argument("--output-cohort-name", help="Output prefix of the cohort files (default {output-folder}/cohort)")
    p.add_argument("--plot", action="store_true", help="(not supported in this build)")
    p.add_argument("--ipd-version", default="2100", help="IPD*KIR version")
    p.add_argument("--msa-type", default="ab_2dl1s1", choices=["merge", "split", "ab", "ab_2dl1s1"],
                   help="Type of MSA setup of the index")
    p.add_argument("--msa-no-exon-only-allele", action="store_true", help="Index without exon-only alleles")
    p.add_argument("--index-folder", default="index", help="Folder of the HISAT2-indexed KIR reference")
    p.add_argument("--index-wgs", help="(WGS extraction is outside this build)")
    p.add_argument("--ref-genome", default="hg19", choices=["hg19", "hg38"], help="(WGS extraction only)")
    p.add_argument("--cn-diploid-gene", choices=["", "VDR", "RYR1", "EGFR"], default="", help="(WGS extraction only)")
    p.add_argument("--cn-exon", action="store_true", help="Use exon-only depths for CN prediction")
    p.add_argument("--cn-cohort", action="store_true", help="Predict CN cohort-wise instead of sample-wise")
    p.add_argument("--cn-select", default="p75", choices=["p75", "mean", "median"], help="Gene depth statistic")
    p.add_argument("--cn-algorithm", default="LCND", choices=["LCND", "KDE"], help="CN prediction model")
    p.add_argument("--cn-dist-dev", default=0.08, help="Deviation of distributions in LCND")
    p.add_argument("--cn-3dl3-not-diploid", action="store_true", help="Do not assume KIR3DL3 is diploid")
    p.add_argument("--cn-provided", nargs="*", help="Provided CN TSVs (one per sample, in order)")
    p.add_argument("--allele-strategy", default="full", choices=["full", "pv", "exonfirst", "report", "em"],
                   help="full (alias pv): likelihood over all variants; exonfirst: exon variants first; "
                        "report (alias em): EM abundance typing")
    p.add_argument("--step-skip-extraction", action="store_true", help="Skip extracting KIR reads from WGS")
    p.add_argument("--step-skip-typing", action="store_true", help="Skip allele typing")
    # additive
    p.add_argument("--alignment", action="append",
                   help="Existing name-collated alignments (SAM / SAM.gz / BAM), one per sample: skips hisat2")
    p.add_argument("--no-variant-json", action="store_true", help="Do not write {name}.variant.json")
    p.add_argument("--ingest-decode", choices=["host", "device"], default="host",
                   help="Who decodes the alignment records of a .bam sample into packed records: the host (default), or "
                        "the device for the plain pairs (M and D operations only) with the host taking the rest; the "
                        "device route needs --no-variant-json (the SAM text is not kept), the results are the same")
    p.add_argument("--novel-discovery", action="store_true",
                   help="After typing, look for novel variants of the called alleles in their reads: writes "
                        "{result}.novel.variant.tsv / .tsv / .fa / .bam / .txt per sample (needs the .no_multi.bam, so "
                        "not with --no-variant-json)")
    p.add_argument("--em-bootstrap", type=int, default=0,
                   help="EM strategy only: this many read-bootstrap replicates per gene after typing; writes "
                        "{result}.confidence.tsv (abundance spread per allele, support of the call)")
    p.add_argument("--em-bootstrap-seed", type=int, default=2022, help="Seed of the bootstrap draws")
    p.add_argument("--call-bootstrap", type=int, default=None,
                   help="Likelihood strategies (full / pv / exonfirst) only: rescore every gene's candidate sets in this "
                        "many read-bootstrap replicates after typing; writes {result}.call_confidence.tsv (share of "
                        "replicates each candidate wins, spread of its distance to the called set)")
    p.add_argument("--call-bootstrap-seed", type=int, default=2022, help="Seed of the call bootstrap's draws")
    p.add_argument("--call-bootstrap-top", type=int, default=32,
                   help="Candidate sets of a gene the call bootstrap rescores (1 .. 256, in rank order)")
    p.add_argument("--call-fit", action="store_true",
                   help="Likelihood strategies (full / pv / exonfirst) only: report how the called set of every gene explains "
                        "the reads; writes {result}.fit.tsv (reads without / with mismatches, per called allele the reads it "
                        "explains best and alone, the alleles that would explain the most as one more copy)")
    p.add_argument("--call-fit-extra", type=int, default=3,
                   help="Extra alleles the fit report lists per gene (0 .. 64; 0: none are looked for)")
    p.add_argument("--call-alternatives", action="store_true",
                   help="Likelihood strategies (full / pv / exonfirst) only: report for every called allele the alleles that "
                        "could stand in for it -- better, identical (no read tells them apart), balanced, near -- and the field "
                        "of its name the reads resolve; writes {result}.alternatives.tsv")
    p.add_argument("--call-alternatives-within", type=int, default=1,
                   help="The largest number of mismatches a swap may cost and still be listed as near (0 .. 64)")
    p.add_argument("--call-alternatives-max", type=int, default=20,
                   help="Alternatives listed per called allele (1 .. 256); every class is always counted in full")
    p.add_argument("--call-dosage", action="store_true",
                   help="Likelihood strategies (full / pv / exonfirst) only: report how many copies of each called allele the "
                        "reads support (a mixture fit the search's max cannot make) and the best integer compositions at one "
                        "copy fewer, the called number and one more; writes {result}.dosage.tsv")
    p.add_argument("--call-coverage", action="store_true",
                   help="Likelihood strategies (full / pv / exonfirst) only: report where along every gene the reads lie that "
                        "its called set explains; writes {result}.coverage.tsv (per region -- upstream, exons, introns, "
                        "downstream -- and called allele the bases of the reads it explains best and alone, and its private "
                        "sites no read of its own covers).  The sample's records stay in HBM until it is typed")
    p.add_argument("--call-coverage-depth", action="store_true",
                   help="Also write {result}.coverage.depth.tsv: every coverage track as runs of equal depth (implies "
                        "--call-coverage)")
    p.add_argument("--cn-bootstrap", type=_cnBootstrapCount, default=None, metavar="N",
                   help="Read bootstrap of the copy-number stage, N replicates (1 .. 10000): every replicate draws the sample's "
                        "pairs again, recomputes every gene's depth statistic and is assigned a copy number by the fitted "
                        "model; writes {depth}.boot.tsv, {cn}.confidence.tsv per sample and {cohort}.cn.confidence.tsv")
    p.add_argument("--cn-bootstrap-seed", type=int, default=2022, help="Seed of the copy-number bootstrap's draws")
    p.add_argument("--ranks", type=int, default=1,
                   help="Start this many rank processes (samples are sharded over them; ranks map to GPUs round robin, "
                        "so 3 x the GPU count keeps every GPU busy).  Not needed under torchrun / any launcher that "
                        "sets RANK and WORLD_SIZE.")
    return p


def callReportArgs(args: argparse.Namespace, index_ref: str | None = None, report: str | None = None) -> dict:
    """The ``sampleTyper`` keywords of the per-call reports the command line asks for (of the one with the key ``report``,
    when given); nothing for a report whose flag is not given, whatever its options say.  An option out of its range or the
    EM strategy is an error.  ``index_ref``: what a report needs of the index is read (``gene_len`` for ``--call-coverage``)."""
    out: dict = {}
    for entry in CALL_REPORTS:
        if report in (None, entry.key):
            out.update(entry.fromArgs(args, index_ref))
    return out


def _cnBootstrapArgs(args: argparse.Namespace) -> dict | None:
    """The ``mapSamples`` keyword of ``--cn-bootstrap`` (None when the flag is not given)."""
    n = getattr(args, "cn_bootstrap", None)
    if n is None:
        return None
    if not 1 <= int(n) <= 10000:
        raise ValueError("--cn-bootstrap needs a count in 1 .. 10000")
    return {"n_boot": int(n), "seed": int(getattr(args, "cn_bootstrap_seed", 2022)), "select_mode": args.cn_select}


def main(args: argparse.Namespace) -> None:
    if getattr(args, "cn_cohort", False):
        os.environ.setdefault("GK_SAMPLE_LANES", "3")      # samples wait in HBM for the pooled fit: the lanes' working sets stay small
    cohort.pipelineDefaults()       # before the first HIP call: blocking waits, sample lanes, search slots (as bench.py)
    setThreads(args.thread)
    setEngine(args.engine)
    logger.setLevel(args.log_level)
    logger.debug(f"[Main] {args}")
    if not args.step_skip_extraction and not args.alignment:
        raise NotImplementedError("WGS extraction (bwa) is outside this build: pass --step-skip-extraction")
    if args.plot:
        raise NotImplementedError("--plot is outside this build")
    n_boot = int(getattr(args, "em_bootstrap", 0) or 0)
    if n_boot < 0 or (n_boot > 0 and args.allele_strategy not in ("em", "report")):
        raise ValueError("--em-bootstrap needs a positive count and --allele-strategy em (or report)")
    callReportArgs(args)
    _cnBootstrapArgs(args)

    if not args.input_csv:
        if not args.r1 and not args.alignment:
            raise ValueError("At least one paired-end read 1 FASTQ file must be provided")
        if args.r1:
            if len(args.r1) != len(args.r2 or []):
                raise ValueError("The number of paired-end read 1 and read 2 FASTQ files must be equal")
            reads = list(zip(args.r1, args.r2))
            names = [getCommonName(a, b) for a, b in reads]
        else:
            reads = [("", "")] * len(args.alignment)
            names = [a.rsplit(".", 2 if a.endswith(".gz") else 1)[0] for a in args.alignment]
        cn_files = list(args.cn_provided) if args.cn_provided else [""] * len(names)
    else:
        df = pd.read_csv(args.input_csv)
        names = list(df["name"])
        reads = list(zip(df["r1"], df["r2"]))
        cn_files = list(df["cnfile"].fillna("")) if "cnfile" in df.columns else [""] * len(names)
    if not names:
        raise ValueError("No samples found in input")
    if len(cn_files) != len(names):
        raise ValueError("Mismatch between number of samples and copy number files")
    if args.alignment and len(args.alignment) != len(names):
        raise ValueError("--alignment must be given once per sample")
    logger.info(f"[Main] Samples: {names}")

    if args.output_folder:
        Path(args.output_folder).mkdir(exist_ok=True)
        names = [replaceParentFolder(n, args.output_folder) for n in names]
        output_folder = args.output_folder
    else:
        output_folder = str(Path(names[0]).parent)
    cohort_name = args.output_cohort_name or str(Path(output_folder) / "cohort")
    Path(cohort_name).parent.mkdir(exist_ok=True)

    # index (must exist: building it needs the network, pyhlamsa and muscle -- out of scope)
    if args.msa_no_exon_only_allele:
        index_msa = f"{args.index_folder}/kir_{args.ipd_version}_{args.msa_type}.leftalign"
    else:
        index_msa = f"{args.index_folder}/kir_{args.ipd_version}_withexon_{args.msa_type}.leftalign"
    index_ref = index_msa + ".mut01"
    index = index_ref + ".graph"
    if not Path(index_ref + ".snp").exists():
        raise FileNotFoundError(f"{index_ref}.snp/.link/.locus not found: building the index is outside this build")

    # shard the cohort over ranks (one GPU per process): longest processing time first by input size
    transport = cohort.initFromEnv()
    comm = None
    if transport is not None:
        inputs = args.alignment if args.alignment else [list(r) for r in reads]
        comm = cohort.Comm(len(names), transport, weights=cohort.sampleWeights(inputs))
        try:
            return _runCohort(args, names, reads, cn_files, index, index_ref, cohort_name, comm)
        except BaseException as e:     # the other ranks must not wait out their timeouts for this one
            if transport.store is not None:
                transport.store.abort(f"rank {transport.rank}: {type(e).__name__}: {e}")
            raise
    return _runCohort(args, names, reads, cn_files, index, index_ref, cohort_name, comm)


def _runCohort(args, names, reads, cn_files, index, index_ref, cohort_name, comm) -> None:
    """Tabulation, depth, copy numbers, typing and the merges for this rank's share of the cohort (main.py:124-250,
    572-603)."""
    mine = comm.mine if comm else list(range(len(names)))
    pick = lambda xs: [xs[i] for i in mine]   # noqa: E731

    my_cn = pick(cn_files)
    kwargs = {"base_dev": float(args.cn_dist_dev), "start_base": 2}
    method = {"pv": "full", "report": "em"}.get(args.allele_strategy, args.allele_strategy)
    pooled_fit = args.cn_cohort and not all(cn_files)
    novel = getattr(args, "novel_discovery", False)
    lanes = sampleTyper(method, novel_index=index_ref if novel else None, bootstrap=int(getattr(args, "em_bootstrap", 0) or 0),
                        bootstrap_seed=int(getattr(args, "em_bootstrap_seed", 2022)), **callReportArgs(args, index_ref))
    try:
        confidence: list | None = [] if _cnBootstrapArgs(args) else None
        allele_files, my_cn = _typeShare(args, lanes, pick(names), pick(reads), my_cn, pick, index, index_ref, cohort_name,
                                         comm, kwargs, pooled_fit, keep_records=bool(callReportArgs(args, report="call_coverage")),
                                         confidence=confidence)
    finally:
        lanes.close()
    _mergeShare(my_cn, allele_files, cohort_name, comm, confidence)


def _typeShare(args, lanes, names, reads, my_cn, pick, index, index_ref, cohort_name, comm, kwargs, pooled_fit,
               keep_records=False, confidence=None):
    """Tabulation, depth, copy numbers of this rank's samples, each handed to the typing lanes as soon as its copy
    numbers are known; returns (allele files, CN files) in the rank's sample order.  ``keep_records`` (``--call-coverage``):
    a sample's records stay in HBM until the lane that typed it frees them.  ``confidence`` (``--cn-bootstrap``): a list that
    gets, per sample in the rank's order, its ``{cn_name}.confidence.tsv`` -- written as soon as the model that assigned its
    copy numbers is fitted -- or None for a sample without one (its copy numbers were provided, or it has no ``.boot.tsv``)."""
    cn_boot = _cnBootstrapArgs(args) if confidence is not None else None
    if cn_boot is not None:
        cn_boot["samples"] = [pooled_fit or not c for c in my_cn]
        for c in my_cn:
            if c and not pooled_fit:
                logger.info(f"[CN] cn bootstrap: the copy numbers of {c} are provided; nothing to bootstrap")

    def confide(depth_file: str, cn_file: str, model) -> None:
        if confidence is None:
            return
        boot_file = depth_file[:-len(".tsv")] + ".boot.tsv"
        if model is None or not Path(boot_file).exists():
            confidence.append(None)
            return
        from .cn_bootstrap import writeCnConfidence
        confidence.append(writeCnConfidence(boot_file, model, cn_file, cn_file[:-len(".tsv")] + ".confidence.tsv"))

    allele_files: list[str] = []
    waiting: list[tuple[str, object]] = []      # samples that wait for the pooled copy-number fit
    depth_files: list[str] = []
    retained = 0
    budget = int(float(os.environ.get("GK_RETAIN_GB", "64")) * 2**30)   # tabulations kept in HBM until the pooled fit
    samples = mapSamples(names, reads, index, index_ref, exon_region_only=args.cn_exon,
                         alignments=pick(args.alignment) if args.alignment else None,
                         write_json=not args.no_variant_json,
                         keep_records=(pooled_fit or keep_records) and not args.step_skip_typing,
                         keep_text=getattr(args, "novel_discovery", False) and not args.step_skip_typing,
                         cn_bootstrap=cn_boot, ingest_decode=getattr(args, "ingest_decode", "host"))
    for i, (_, name, data, depth_file) in enumerate(samples):
        depth_files.append(depth_file)
        if pooled_fit:
            # every sample's depth is needed before any can be typed.  What waits in HBM is the sample's packed records in
            # compact form (ParkedRecords: ~150 MB per 5 M reads), not its tabulation (~1 GB): the lists are made again when
            # its turn comes.  Beyond the budget a sample is parked in a hand-off file and reloaded for typing.
            if args.step_skip_typing:
                data.tab.close()
                waiting.append((name, None))
                continue
            size = int(0.12 * 256 * data.tab.n_pairs) + (1 << 20)      # what the compact records will take, roughly
            # a sample whose reads novel discovery writes again waits as its .variant.json (the lines are in it)
            if retained + size > budget or data.tab.mates is None or getattr(args, "novel_discovery", False):
                if args.no_variant_json:
                    parked = name + ".npz"          # already written by mapSamples, unless hand-off files are lazy
                    if os.environ.get("GK_HANDOFF", "always") == "lazy":
                        writeCompact(data, parked, index_ref=index_ref)
                else:
                    parked = name + ".json"
                if data.tab.mates is not None:
                    data.tab.mates.free()
                    data.tab.mates = None
                data.tab.close()
                waiting.append((name, parked))
            else:
                parked = ParkedRecords(data)        # compacts the records, releases them and the tabulation
                retained += parked.nbytes
                waiting.append((name, parked))
            continue
        if not my_cn[i]:
            cn_name = str(Path(depth_file).with_suffix(f".{args.cn_select}.{args.cn_algorithm}"))
            logger.info(f"[CN] Copy number estimation per sample ({cn_name})")
            model = predictSamplesCN([depth_file], [cn_name + ".tsv"], "", cluster_method=args.cn_algorithm,
                                     cluster_method_kwargs=kwargs, assume_3DL3_diploid=not args.cn_3dl3_not_diploid,
                                     save_cn_model_path=cn_name + ".json", select_mode=args.cn_select,
                                     return_model=confidence is not None)
            my_cn[i] = cn_name + ".tsv"
            confide(depth_file, my_cn[i], model)
        else:
            confide(depth_file, my_cn[i], None)
        # copy numbers known: hand the sample to the typing lanes and go on with the next one's tabulation; a lane
        # releases the sample when it is typed (at most GK_SAMPLE_LANES tabulations wait in HBM)
        if not args.step_skip_typing:
            lanes.submit(data, (lambda f=my_cn[i]: loadCN(f)), (name, my_cn[i], data))
            if lanes.inFlight() >= lanes.lanes:
                allele_files.append(lanes.next())
        else:
            data.tab.close()
    if pooled_fit:
        suffix = f".{args.cn_select}.cohort.{args.cn_algorithm}"
        my_cn = [str(Path(p).with_suffix(suffix + ".tsv")) for p in depth_files]
        logger.info(f"[CN] Copy number estimation by cohort ({cohort_name + suffix})")
        model = predictSamplesCN(depth_files, my_cn, cluster_method=args.cn_algorithm, cluster_method_kwargs=kwargs,
                                 save_cn_model_path=cohort_name + suffix + ".json", select_mode=args.cn_select, comm=comm,
                                 return_model=confidence is not None)
        for depth_file, cn_file in zip(depth_files, my_cn):      # every rank ran the identical fit: its own samples' tables
            confide(depth_file, cn_file, model)
        for (name, source), cn_file in zip(waiting, my_cn):
            if args.step_skip_typing:
                continue
            if isinstance(source, ParkedRecords):
                source = source.restore()           # expansion + tabulation, while the lanes type the samples before it
            lanes.submit(source, (lambda f=cn_file: loadCN(f)), (name, cn_file, source))
            if lanes.inFlight() >= lanes.lanes:
                allele_files.append(lanes.next())
    allele_files.extend(lanes.drain())
    return allele_files, my_cn


def _mergeShare(my_cn, allele_files, cohort_name, comm, confidence=None) -> None:
    # merge on rank 0, in cohort order
    if confidence is not None:      # --cn-bootstrap: (CN file, confidence table) of every sample that has one
        confidence = [(cn, c) for cn, c in zip(my_cn, confidence)]
    if comm is not None:
        cn_sorted = comm.gatherInCohortOrder(my_cn)
        al_sorted = comm.gatherInCohortOrder(allele_files)
        conf_sorted = comm.gatherInCohortOrder(confidence) if confidence is not None else None
        if comm.rank == 0:
            my_cn, allele_files, confidence = cn_sorted, [a for a in al_sorted if a], conf_sorted
    if comm is None or comm.rank == 0:
        logger.info(f"[CN] Saved copy number in {cohort_name}.cn.tsv")
        mergeCN(my_cn, cohort_name + ".cn.tsv")
        if allele_files:
            logger.info(f"[Allele] Saved in {cohort_name}.allele.tsv")
            mergeAllele(allele_files, cohort_name + ".allele.tsv")
        if confidence is not None:
            from .cn_bootstrap import mergeCnConfidence
            logger.info(f"[CN] Saved the copy numbers' bootstrap confidence in {cohort_name}.cn.confidence.tsv")
            mergeCnConfidence([(cn, c) for cn, c in confidence if c], cohort_name + ".cn.confidence.tsv")
    if comm is not None:
        comm.barrier()
        comm.close()
    logger.info("[Main] Success")


def spawnRanks(n: int, argv: list[str]) -> int:
    """``--ranks N`` without a launcher: start N copies of this command as ranks 0..N-1 (fresh processes; this
    one never touches the GPU) and supervise them: a rank that fails ends the launch for all (``comm.superviseRanks``),
    the rendezvous directory is removed either way.  Returns 0 or 1."""
    import subprocess
    import sys
    import tempfile
    import uuid
    from .comm import superviseRanks
    rdzv = tempfile.mkdtemp(prefix="gk_rdzv_")
    token = uuid.uuid4().hex
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GK_RDZV_DIR=rdzv, GK_RDZV_TOKEN=token)
        procs.append(subprocess.Popen([sys.executable, "-m", "kir_graph_amd.main"] + argv, env=env))
    return superviseRanks(procs, rdzv, token)


def entrypoint() -> None:
    import sys
    args = createParser().parse_args()
    if args.ranks > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawnRanks(args.ranks, sys.argv[1:]))
    main(args)


if __name__ == "__main__":
    entrypoint()

"""
What the per-call reports of the likelihood strategies share.

1. ``CalledSet``: the called row of a gene's adopted result as the reports read it -- its distinct alleles, ascending, with
   their labels and copies, and the ``u8`` mismatch table ``miss8[column][read]`` the search left in HBM
   (``DeviceModel.missFor``).  ``calledSet`` builds it once, with the warnings of every report that cannot be made.
2. ``CALL_REPORTS``: one entry per report, in launch order, from its typer keywords and command-line flags to the files it
   writes.  ``TypingWithPosNegAllele`` (kir_typing.py), ``selectKirTypingModel`` and the command line (main.py) loop over
   it: a new report is a module, an entry here and its native code ("adding a report").
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, NamedTuple

import numpy as np

from .samtools_utils import readLocusLengths
from .utils import logger

MAX_CALLED = 16                  # distinct alleles of one report's library call (csrc/gk_called.h)
LIKELIHOOD = "a likelihood strategy (--allele-strategy full, pv or exonfirst)"
NO_TABLE = "[Allele] {}: the model has no mismatch table (exact search or 16 M reads or more); skipped"


def modelOf(result):
    """The one ``DeviceModel`` all parts of ``result.allele_prob`` name (forks of one model do), or None."""
    parts = getattr(result.allele_prob, "parts", None)
    if not parts:
        return None
    model = parts[0][0]
    return model if all(m is model for m, _ in parts) else None


class CalledSet(NamedTuple):
    """The called set of one gene's adopted result (a tuple: cheap to make next to the kernels it feeds, and frozen).
    ``ids``: the distinct called ordinals, ascending; ``labels`` / ``copies``: the called row's own name of each and how
    often it is called; ``reads``: the rows of the model's table; ``scope``: ``"all"`` when the table holds every allele
    of the gene, ``"candidates"`` when it holds the exon-first candidates only; ``names``: allele ordinal -> name (None
    when nobody gave the map).  ``miss8`` / ``ldm`` / ``n_table_cols`` / ``cols`` (the called columns): the table, once
    ``withTable`` has asked for it."""

    what: str
    model: Any
    cn: int
    reads: int
    ids: np.ndarray
    labels: tuple[str, ...]
    copies: tuple[int, ...]
    scope: str
    names: Any = None
    miss8: Any = None
    ldm: int = 0
    n_table_cols: int = 0
    cols: np.ndarray | None = None

    def nameOf(self, col: int) -> str:
        """The allele of table column ``col``."""
        table_cols = self.model.tableColumns
        return self.names[col if table_cols is None else int(table_cols[col])]

    def withTable(self) -> "CalledSet | None":
        """The record with the model's mismatch table and the called columns in it; None -- with a warning -- when the
        model has none."""
        held = self.model.missFor(self.ids)
        if held is None:
            logger.warning(NO_TABLE.format(self.what))
            return None
        return self._replace(miss8=held[0], ldm=held[1], n_table_cols=held[2], cols=held[3])


def calledSet(result, what: str, names=None, table: bool = True) -> CalledSet | None:
    """The called set of ``result`` (the last step's ``TypingResult``: the row ``bestRank()``) for the report ``what``
    (``"call fit"``, ...: the name in its warnings).  ``names``: allele ordinal -> name for a result that does not carry
    the map itself (the merged result of exon-first).  ``table=False``: without the mismatch table, for a report that has
    checks of its own to make before ``withTable``.  None -- with a warning -- when the result's sets do not sit on one
    device table, more than 16 distinct alleles are called, or the model has no mismatch table."""
    model = modelOf(result)
    if model is None or not model.n_rows:
        logger.warning(f"[Allele] {what}: the result's sets are not on one device table; skipped")
        return None
    row = int(result.bestRank())
    called_names = list(result.allele_name[row])
    ids, first, copies = np.unique(np.asarray(result.allele_id, dtype=np.int64)[row], return_index=True, return_counts=True)
    if len(ids) > MAX_CALLED:
        logger.warning(f"[Allele] {what}: {len(ids)} distinct alleles called, more than {MAX_CALLED}; skipped")
        return None
    held = (None, 0, 0, None)
    if table:
        held = model.missFor(ids)
        if held is None:
            logger.warning(NO_TABLE.format(what))
            return None
    return CalledSet(what, model, int(result.n), int(model.n_rows), ids, tuple([called_names[f] for f in first.tolist()]),
                     tuple(copies.tolist()), "all" if model.tableColumns is None else "candidates",
                     getattr(result.allele_name, "names", None) or names, *held)


# ------------------------------------------------------------------------------------------------ the table of reports
# The report modules start from the record above and the table below names them: they are imported here, below the record,
# and import this module at their own end -- whichever is imported first finds what it needs of the other already defined.
from . import call_alternatives, call_bootstrap, call_coverage, call_dosage, call_fit  # noqa: E402


@dataclass(frozen=True)
class Option:
    """One keyword of a report: its name at ``main.sampleTyper`` and, with dashes, on the command line.  ``lo`` .. ``hi``:
    the range the typer accepts, ``what``: the words of its ValueError, ``needs``: what the command line's error asks for.
    ``typer``: its name at the typer when that differs, None for an option of the files alone.  ``from_index``: it has
    no flag; the command line reads it from the index (given the index prefix)."""

    name: str
    default: Any
    lo: int | None = None
    hi: int | None = None
    what: str = ""
    needs: str = ""
    typer: str | None = ""
    from_index: Callable | None = None

    @property
    def flag(self) -> str:
        return "--" + self.name.replace("_", "-")

    @property
    def typerName(self) -> str | None:
        return self.name if self.typer == "" else self.typer


@dataclass(frozen=True)
class CallReport:
    """One per-call report.  ``key``: the keyword that switches it on (``options[0]``: a flag, or with ``count`` a number
    of replicates) and the typer attribute ``{gene: entry}`` that holds its results; ``does``: the words of the EM
    strategy's refusal; ``make(typer, gene, g, cn, result, options)``: the entry of one gene (``g``: its ordinal in the
    index; ``options``: the typer's keywords of the report), None when it cannot be made -- kept as None with
    ``keeps_none``; ``files``: (suffix, text function, the option that asks for it or None) of every ``{result}{suffix}``
    it writes; ``implied_by``: further flags that switch it on; ``check(options)``: what the typer refuses beyond the
    options' ranges."""

    key: str
    does: str
    options: tuple[Option, ...]
    make: Callable
    files: tuple[tuple[str, Callable, str | None], ...]
    count: bool = False
    keeps_none: bool = False
    implied_by: tuple[str, ...] = ()
    check: Callable | None = None

    @property
    def flag(self) -> str:
        return self.options[0].flag

    def switchedOn(self, options: dict) -> bool:
        value = options.get(self.key)
        return int(value or 0) > 0 if self.count else bool(value)

    def typerOptions(self, given: dict) -> dict:
        """The typer's keywords of this report taken out of ``given``: defaults filled in, ranges checked."""
        out = {}
        for o in self.options:
            if o.typerName is None:
                continue
            value = given.pop(o.typerName, o.default)
            if o.lo is not None:
                value = int(value or 0)      # a count that is not given: none
                if not o.lo <= value <= o.hi:
                    raise ValueError(f"{o.name}: {o.what} must lie in {o.lo} .. {o.hi}")
            out[o.typerName] = value
        if self.check is not None:
            self.check(out)
        return out

    def typerKeywords(self, options: dict) -> dict:
        """The typer's keywords of this report from ``main.sampleTyper``'s."""
        return {o.typerName: options.get(o.name, o.default) for o in self.options if o.typerName is not None}

    def fromArgs(self, args, index_ref: str | None = None) -> dict:
        """``main.sampleTyper``'s keywords of this report from the parsed command line: none when it is not asked for;
        an option out of range or the EM strategy is a ValueError.  ``index_ref``: the index prefix, for what is read
        from the index."""
        flags = [o for o in self.options if o.from_index is None]
        values = {o.name: getattr(args, o.name, o.default) for o in flags}
        switch = values[self.key]
        if not (switch is not None if self.count else bool(switch) or any(values[name] for name in self.implied_by)):
            return {}
        ranged = [o for o in flags if o.lo is not None]
        bad = any(not o.lo <= int(values[o.name]) <= o.hi for o in ranged) or (self.count and int(switch) < 1)
        if bad or args.allele_strategy in ("em", "report"):
            needs = ", ".join(o.needs for o in ranged)
            raise ValueError(f"{self.flag} needs {needs + ' and ' if needs else ''}{LIKELIHOOD}")
        out = {o.name: bool(values[o.name]) if isinstance(o.default, bool) else int(values[o.name]) for o in flags}
        if not self.count:
            out[self.key] = True
        if index_ref is not None:
            out.update({o.name: o.from_index(index_ref) for o in self.options if o.from_index is not None})
        return out


def _bootstrap(typer, gene, g, cn, result, o):
    # the replicates are drawn on the stream numbered like the gene in the index: the same whichever genes are typed
    # with it, and whichever driver path typed it
    return call_bootstrap.bootstrapCall(result, call_bootstrap.homoFactor(result), o["call_bootstrap"],
                                        o["call_bootstrap_seed"], g, o["call_bootstrap_top"])


def _names(typer, g):
    return typer._data.index.tables[g].alleles


def _fit(typer, gene, g, cn, result, o):
    return call_fit.fitCall(result, o["call_fit_extra"], names=_names(typer, g))


def _alternatives(typer, gene, g, cn, result, o):
    return call_alternatives.alternativesOfCall(result, o["call_alternatives_within"], o["call_alternatives_max"],
                                                names=_names(typer, g))


def _dosage(typer, gene, g, cn, result, o):
    return call_dosage.dosageOfCall(result, names=_names(typer, g))


def _coverage(typer, gene, g, cn, result, o):
    """The sample's records must still be in HBM (``tab.mates``): a hand-off file, or released, is said once per sample
    and gives None for every gene."""
    lengths = o["call_coverage_len"]
    if gene not in lengths:
        raise ValueError(f"call_coverage: no backbone length for {gene}")
    if getattr(typer._data.tab, "mates", None) is None:
        if not getattr(typer, "_coverage_warned", False):
            typer._coverage_warned = True
            logger.warning("[Allele] call coverage: the sample's records are not in HBM (a hand-off file, or released); "
                           "no gene of it is reported")
        return None
    index = typer._data.index
    return call_coverage.coverCall(result, lengths[gene], index.exons.get(gene, []), index.tables[g], names=_names(typer, g))


def _coverageNeedsLengths(options: dict) -> None:
    if options["call_coverage"] and not options["call_coverage_len"]:
        raise ValueError("call_coverage: needs call_coverage_len, the backbone length of every gene")


CALL_REPORTS = (
    CallReport("call_bootstrap", "rescore candidate sets", count=True, make=_bootstrap,
               options=(Option("call_bootstrap", None, 0, call_bootstrap.MAX_BOOT, "the number of replicates",
                               f"a count in 1 .. {call_bootstrap.MAX_BOOT}"),
                        Option("call_bootstrap_seed", 2022),
                        Option("call_bootstrap_top", 32, 1, call_bootstrap.MAX_TOP, "the candidate sets kept",
                               f"a --call-bootstrap-top in 1 .. {call_bootstrap.MAX_TOP}")),
               files=((".call_confidence.tsv", call_bootstrap.callConfidenceText, None),)),
    CallReport("call_fit", "report the fit of a call", make=_fit,
               options=(Option("call_fit", False),
                        Option("call_fit_extra", 3, 0, call_fit.MAX_EXTRA, "the extra alleles listed",
                               f"a --call-fit-extra in 0 .. {call_fit.MAX_EXTRA}")),
               files=((".fit.tsv", call_fit.callFitText, None),)),
    CallReport("call_alternatives", "report the alternatives of a call", make=_alternatives,
               options=(Option("call_alternatives", False),
                        Option("call_alternatives_within", 1, 0, call_alternatives.MAX_WITHIN, "the largest delta listed",
                               f"a --call-alternatives-within in 0 .. {call_alternatives.MAX_WITHIN}"),
                        Option("call_alternatives_max", 20, 1, call_alternatives.MAX_LISTED, "the alternatives listed per allele",
                               f"a --call-alternatives-max in 1 .. {call_alternatives.MAX_LISTED}")),
               files=((".alternatives.tsv", call_alternatives.callAlternativesText, None),)),
    CallReport("call_dosage", "report the dosage of a call", make=_dosage, options=(Option("call_dosage", False),),
               files=((".dosage.tsv", call_dosage.callDosageText, None),)),
    CallReport("call_coverage", "report the coverage of a call", make=_coverage, keeps_none=True,
               implied_by=("call_coverage_depth",), check=_coverageNeedsLengths,
               options=(Option("call_coverage", False),
                        Option("call_coverage_depth", False, typer=None),
                        Option("gene_len", None, typer="call_coverage_len", from_index=readLocusLengths)),
               files=((".coverage.tsv", call_coverage.callCoverageText, None),
                      (".coverage.depth.tsv", call_coverage.callCoverageDepthText, "call_coverage_depth"))),
)


def callReport(key: str) -> CallReport:
    """The entry of ``CALL_REPORTS`` with that key."""
    return next(r for r in CALL_REPORTS if r.key == key)

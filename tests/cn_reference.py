"""The grid of the copy-number fit (csrc/gk_cn.hip, include/graphkir_hip.h) in exact decimal arithmetic, and its case list.

    loglik(b) = sum_x log(max_k N(x; b (first_cn + k), dev_k) space + 1e-9) density[x]

with N(x; m, s) = exp(-((x - m) / s)^2 / 2) / C / s and C the double 2.5066282746310002 that the kernel divides by.  The inputs
are doubles and enter as the exact decimals of those doubles (1e-9 too); every operation then runs at 40 digits
(``Decimal.exp`` and ``Decimal.ln`` are correctly rounded), so the result is the formula's value on the given inputs to far more
than a double's precision.  ``float64Loglik`` is the same formula in numpy's doubles, operation for operation what scipy's
``norm.pdf`` and oracle/cn.py do.

``python tests/cn_reference.py`` prints the largest |float64 - decimal| / S over the case list, which sets the tolerance of
tests/test_gpu_cn_fit.py."""
import decimal
import functools
from decimal import Decimal

import numpy as np

SQRT_2PI = 2.5066282746310002          # scipy's _norm_pdf_C, as the kernel writes it
EPS = 1e-9
EXCUSE_GAP = 1e-12                     # a bin whose two largest candidates are closer than this (relative) is excused
CTX = decimal.Context(prec=40, Emin=-999999999, Emax=999999999)

BINS = (1, 2, 255, 256, 257, 300, 513)
N_BASES = (1, 3, 8)
N_CN = (1, 7, 16)
FIRST_CN = (0, 1, 2)


class Case:
    def __init__(self, name, kind, x, density, bases, dev, first_cn, space):
        self.name, self.kind = name, kind
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.density = np.ascontiguousarray(density, dtype=np.float64)
        self.bases = np.ascontiguousarray(bases, dtype=np.float64)
        self.dev = np.ascontiguousarray(dev, dtype=np.float64)
        self.first_cn, self.space = int(first_cn), float(space)
        self.bins, self.n_bases, self.n_cn = len(self.x), len(self.bases), len(self.dev)
        assert len(self.density) == self.bins and (self.dev > 0).all()


class Reference:
    """loglik [n_bases] and S = sum |term| [n_bases] as Decimals; argmax int64 [n_bases][bins] (first maximum) and gap float
    [n_bases][bins], the relative distance (v1 - v2) / v1 of a bin's two largest candidates (inf with one candidate)."""

    def __init__(self, loglik, total_abs, argmax, gap):
        self.loglik, self.S, self.argmax, self.gap = loglik, total_abs, argmax, gap


def deviations(first_cn, n_cn, base_dev):
    """dev_k of copy numbers first_cn .. first_cn + n_cn - 1: the model's own (CNgroup._deviations, start_base == 1)."""
    from kir_graph_amd.cn_model import CNgroup
    model = CNgroup.__new__(CNgroup)
    model.start_base, model.base_dev, model.y0_dev, model.dev_decay, model.max_cn = 1, base_dev, 1.5, 0.5, first_cn + n_cn
    return model._deviations()[first_cn:]


def reference(case):
    D = lambda v: Decimal(float(v))      # noqa: E731  (exact)
    with decimal.localcontext(CTX):
        C, eps, space = D(SQRT_2PI), D(EPS), D(case.space)
        x, dens, dev = [D(v) for v in case.x], [D(v) for v in case.density], [D(v) for v in case.dev]
        loglik, total_abs = [], []
        argmax = np.zeros((case.n_bases, case.bins), dtype=np.int64)
        gap = np.full((case.n_bases, case.bins), np.inf)
        for j, b in enumerate(case.bases):
            loc = [D(b) * (case.first_cn + k) for k in range(case.n_cn)]
            acc = tot = Decimal(0)
            for i in range(case.bins):
                v = []
                for k in range(case.n_cn):
                    z = (x[i] - loc[k]) / dev[k]
                    v.append((-(z * z) / 2).exp() / C / dev[k] * space)
                best = max(v)
                argmax[j, i] = v.index(best)
                if case.n_cn > 1:
                    second = sorted(v)[-2]
                    gap[j, i] = float((best - second) / best)
                term = (best + eps).ln() * dens[i]
                acc += term
                tot += abs(term)
            loglik.append(acc)
            total_abs.append(tot)
    return Reference(loglik, total_abs, argmax, gap)


def float64Table(case, base):
    """[n_cn][bins]: pdf * space in doubles, as scipy's norm.pdf(x, loc, scale) * space computes it."""
    loc = base * (case.first_cn + np.arange(case.n_cn, dtype=np.float64))
    z = (case.x[None, :] - loc[:, None]) / case.dev[:, None]
    return np.exp(-z ** 2 / 2.0) / SQRT_2PI / case.dev[:, None] * case.space


def float64Loglik(case):
    return np.array([np.sum(np.log(float64Table(case, b).max(axis=0) + EPS) * case.density) for b in case.bases])


def relativeError(values, ref):
    """max_j |values[j] - loglik[j]| / S[j] as a float; a base with S == 0 must give exactly 0.0."""
    worst = 0.0
    with decimal.localcontext(CTX):
        for v, want, s in zip(values, ref.loglik, ref.S):
            if s == 0:
                assert float(v) == 0.0
                continue
            worst = max(worst, float(abs(Decimal(float(v)) - want) / s))
    return worst


# ------------------------------------------------------------------------------------------------------------ cases
def twoPeaks(rng, bins, x_max, unit):
    """The histogram of depths around one and two copies of ``unit``, as CNgroup.fit bins them."""
    values = np.concatenate([rng.normal(unit, 0.05 * unit, 40), rng.normal(2 * unit, 0.07 * unit, 60)])
    return np.histogram(values, bins=bins, range=(0, x_max))[0]


def makeCase(name, kind, bins, n_bases, n_cn, first_cn, seed):
    rng = np.random.default_rng(seed)
    x_max = float(rng.uniform(40.0, 90.0)) * 1.2
    unit = x_max / 1.2 / 2.3
    x = np.linspace(0, x_max, bins)
    space = x_max / bins
    dev = deviations(first_cn, n_cn, 0.08 * x_max)
    bases = np.linspace(0.55 * unit, 1.45 * unit, n_bases) if n_bases > 1 else np.array([unit])
    density = twoPeaks(rng, bins, x_max, unit)
    if kind == "zeros":
        density = np.zeros(bins)
    elif kind in ("lane255", "lane256"):
        density = np.zeros(bins)
        density[int(kind[4:])] = 37
    elif kind == "underflow_all":            # equal deviations, every mean ~1000 deviations away: the nearest mean is k = 0
        dev = np.full(n_cn, 0.08 * x_max)
        bases = np.linspace(100 * x_max, 130 * x_max, n_bases)
        assert first_cn > 0
    elif kind == "underflow_part":           # a narrow candidate: bins beyond ~38 deviations underflow, the others do not
        dev = dev / 40
    elif kind == "base0":
        bases = np.zeros(n_bases)
        assert len(set(dev.tolist())) == n_cn
    elif kind == "tie":
        bases = np.zeros(n_bases)
        dev = np.full(n_cn, 0.08 * x_max)
    else:
        assert kind == "two_peak"
    return Case(name, kind, x, density, bases, dev, first_cn, space)


# (kind, bins, n_bases, n_cn, first_cn): every value of every axis, the kinds spread over them
SHAPES = [
    ("two_peak", 1, 1, 1, 0), ("two_peak", 2, 3, 7, 1), ("two_peak", 255, 8, 7, 0), ("two_peak", 256, 3, 16, 2),
    ("two_peak", 257, 3, 7, 0), ("two_peak", 300, 8, 7, 0), ("two_peak", 513, 3, 16, 1), ("two_peak", 513, 1, 7, 2),
    ("zeros", 300, 3, 7, 0), ("zeros", 2, 1, 1, 1),
    ("lane255", 256, 3, 7, 0), ("lane255", 513, 1, 16, 1), ("lane256", 257, 3, 7, 0), ("lane256", 300, 1, 7, 2),
    ("underflow_all", 300, 3, 7, 1), ("underflow_all", 255, 1, 16, 2),
    ("underflow_part", 513, 3, 1, 1), ("underflow_part", 257, 8, 1, 2),
    ("base0", 300, 1, 7, 1), ("base0", 255, 1, 16, 2), ("base0", 1, 1, 7, 1),
    ("tie", 300, 1, 7, 0), ("tie", 257, 3, 16, 1), ("tie", 2, 1, 7, 2),
]


@functools.lru_cache(maxsize=None)
def cases():
    out = [makeCase(f"{kind}-{bins}x{n_bases}x{n_cn}+{first_cn}", kind, bins, n_bases, n_cn, first_cn, seed=7000 + k)
           for k, (kind, bins, n_bases, n_cn, first_cn) in enumerate(SHAPES)]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def referenceOf(name):
    return reference(next(c for c in cases() if c.name == name))


def productionCase():
    """bins = n_bases = 300, n_cn = 7, first_cn = 0, the grid from 0 as CNgroup.fit makes it."""
    rng = np.random.default_rng(300)
    x_max = 71.5 * 1.2
    x = np.linspace(0, x_max, 300)
    return Case("production-300x300x7+0", "two_peak", x, twoPeaks(rng, 300, x_max, x_max / 1.2 / 2.3), np.linspace(0, x_max, 300),
                deviations(0, 7, 0.08 * x_max), 0, x_max / 300)


def measure():
    """The largest |float64 restatement - decimal reference| / S over the case list."""
    return max(relativeError(float64Loglik(c), referenceOf(c.name)) for c in cases())


if __name__ == "__main__":
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for c in cases():
        t0 = time.time()
        ref = referenceOf(c.name)
        print(f"{c.name:32s} {relativeError(float64Loglik(c), ref):.3e}  excused bins {int((ref.gap <= EXCUSE_GAP).sum()):4d}"
              f"  {time.time() - t0:.2f} s")
    print("measured", repr(measure()), " 8 x measured", repr(8 * measure()), " floor 8 * 2^-53", repr(8 * 2.0 ** -53))

"""Helpers of the subsample tests: the exact distribution of one block's stored draw, and chi-square tests on samples."""
import itertools
from math import comb

import numpy as np
from scipy import stats


def block_pmf(counts, mirrored, sample):
    """Exact distribution of the stored counts of one block drawn as DeviceCool.subsampled draws it: the pool holds every
    pixel's count, plus a mirror copy of the pixels flagged `mirrored` (off-diagonal pixels of an intra block);
    keep = int(sample * pool total) contacts are drawn without replacement (multivariate hypergeometric) and a pixel stores the
    draw of its upper copy.  Returns {tuple of stored counts: probability}."""
    counts = [int(c) for c in counts]
    pool = counts + [c for c, m in zip(counts, mirrored) if m]
    total = sum(pool)
    keep = min(int(sample * total), total)
    norm = comb(total, keep)
    out = {}
    for x in itertools.product(*[range(c + 1) for c in pool]):
        if sum(x) != keep:
            continue
        p = 1
        for c, xi in zip(pool, x):
            p *= comb(c, xi)
        key = tuple(x[:len(counts)])
        out[key] = out.get(key, 0) + p / norm
    return out


def chi2_against_pmf(observed, pmf, min_expected=5.0):
    """Pearson chi-square p-value of the observed outcomes (tuples) against an exact pmf; outcomes of small expected count are
    pooled into one class (and so are observations outside the support, which give p = 0 when the pmf says they cannot occur)."""
    n = len(observed)
    keys = sorted(pmf, key=lambda k: -pmf[k])
    seen = {}
    for o in observed:
        seen[tuple(o)] = seen.get(tuple(o), 0) + 1
    if any(k not in pmf for k in seen):
        return 0.0
    big = [k for k in keys if pmf[k] * n >= min_expected]
    rest = [k for k in keys if pmf[k] * n < min_expected]
    obs = [seen.get(k, 0) for k in big]
    exp = [pmf[k] * n for k in big]
    if rest:
        obs.append(sum(seen.get(k, 0) for k in rest))
        exp.append(sum(pmf[k] for k in rest) * n)
    if len(obs) < 2:
        return 1.0
    return float(stats.chisquare(np.asarray(obs, dtype=np.float64), np.asarray(exp, dtype=np.float64)).pvalue)


def two_sample_chi2(a, b, n_bins=20):
    """Chi-square p-value of the homogeneity of two integer samples, binned at the quantiles of the pooled sample."""
    pooled = np.concatenate([a, b])
    edges = np.unique(np.quantile(pooled, np.linspace(0, 1, n_bins + 1)))
    edges[-1] += 1
    ha = np.histogram(a, edges)[0]
    hb = np.histogram(b, edges)[0]
    keep = (ha + hb) > 0
    return float(stats.chi2_contingency(np.vstack([ha[keep], hb[keep]]))[1])

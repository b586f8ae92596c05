"""The pileup of `detect --iterations` on the device, the parts that need no GPU: the documented summation order of
cs_pileup_blocks restated in numpy (tests/pileup_util.py) against np.nanmean, the chunk rule cs_pileup_chunk, and
parallel.detect_genome with an injected stage / detect, which keeps the host mean."""
import numpy as np
import pytest

from chromosight_amd import _lib, engine, parallel, pipeline

from pileup_util import restated_pileup, sum_bound


def test_symbols_are_part_of_the_abi():
    assert "cs_pileup_blocks" in _lib.ABI_SYMBOLS and "cs_pileup_chunk" in _lib.ABI_SYMBOLS


def test_chunk_is_positive_and_non_decreasing():
    ns = list(range(0, 70)) + [4095, 4096, 4097, 4104, 4105, 10_000, 10 ** 6, 10 ** 6 + 1, 2 ** 31 - 1]
    chunks = [engine.pileup_chunk(n) for n in ns]
    assert all(c > 0 for c in chunks)
    assert all(a <= b for a, b in zip(chunks, chunks[1:]))
    # the partial sums stay a bounded scratch: a call never has more chunks than a compile-time constant
    n_chunks = [-(-n // c) for n, c in zip(ns, chunks)]
    assert max(n_chunks) <= 512
    assert engine.pileup_chunk(10_000) > engine.pileup_chunk(10)         # (both regimes of the rule are in the list)


@pytest.mark.parametrize("n,shape,seed", [(0, (3, 3), 0), (1, (5, 7), 1), (7, (3, 3), 2), (8, (3, 3), 3), (9, (7, 7), 4), (29, (9, 15), 5),
                                          (1000, (5, 5), 6), (5003, (3, 3), 7)])
def test_restated_order_against_nanmean(n, shape, seed):
    rng = np.random.default_rng(seed)
    stack = rng.gamma(2.0, 1.0, size=(n,) + shape) * rng.choice([1.0, -1.0, 1e6, 1e-6], size=(n,) + shape)
    stack[rng.random(stack.shape) < 0.2] = np.nan
    if n > 2:
        stack[:, 0, 0] = np.nan                      # a pixel no window covers: 0 / 0
        stack[2] = np.nan                            # a window that left the map
    total, count = restated_pileup(stack)
    assert total.shape == shape and count.dtype == np.int64
    assert np.array_equal(count, np.sum(~np.isnan(stack), axis=0))
    want = np.nansum(stack, axis=0)
    bound = sum_bound(stack)
    assert (np.abs(total - want) <= bound).all(), float(np.max(np.abs(total - want) - bound))
    with np.errstate(all="ignore"):
        mean = total / count
    if n == 0:
        assert np.isnan(mean).all()
        return
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = np.nanmean(stack, axis=0)
    assert np.array_equal(np.isnan(mean), np.isnan(ref))
    ok = ~np.isnan(ref)
    # the mean: the sums' bound over the count, and one rounding of each division
    assert (np.abs(mean - ref)[ok] <= (bound / np.maximum(count, 1))[ok] + 2.0 ** -52 * np.abs(ref[ok])).all()


def test_restated_order_is_the_chunked_one():
    """A stack on which the order shows: 1 + 2^-53 + 2^-53 is 1 when added one by one and 1 + 2^-52 when the two small
    terms meet in their own chunk first."""
    tiny = 2.0 ** -53
    stack = np.array([1.0] + [0.0] * 7 + [tiny, tiny]).reshape(10, 1, 1)
    assert engine.pileup_chunk(10) == 8
    total, _ = restated_pileup(stack)
    assert total[0, 0] == 1.0 + 2.0 ** -52
    total, _ = restated_pileup(stack, chunk=16)
    assert total[0, 0] == 1.0


def test_injected_stage_and_detect_keep_the_host_mean(monkeypatch):
    """parallel.detect_genome with injected stage / detect (the stand-ins of tests/test_parallel.py) does not enter the
    device route: its windows are on the host already."""
    import pandas as pd

    class Genome:
        binsize = 1000
        n_chrom = 5

        def chrom_size(self, ci):
            return 50 + 13 * ci

    def stage(genome, ci, max_dist, largest):
        return {"ci": ci, "n": genome.chrom_size(ci)}

    seen = []

    def detect(genome, block, cfg, kernel, tsvd):
        seen.append(np.array(kernel))
        rng = np.random.default_rng(block["ci"])
        wins = rng.random((3, 3, 3))
        wins[0, 1, 1] = np.nan
        return pd.DataFrame({"bin1": rng.integers(0, block["n"], 3), "bin2": rng.integers(0, block["n"], 3), "score": rng.random(3),
                             "pvalue": rng.random(3)}), wins

    def refuse(*args, **kwargs):
        raise AssertionError("the device route was entered")

    monkeypatch.setattr(pipeline, "pileup_blocks", refuse)
    monkeypatch.setattr(engine, "run_pileup_blocks", refuse)
    cfg = {"max_dist": 20_000, "max_iterations": 2, "kernels": [np.arange(9.0).reshape(3, 3)]}
    rec = parallel.detect_genome(Genome(), cfg, stage=stage, detect=detect)
    assert rec.shape[0] == 2 * 5 * 3 and set(rec[:, 6]) == {0.0, 1.0}
    # the second iteration's template is the host mean of the first one's windows
    stack = np.concatenate([np.random.default_rng(ci).random((3, 3, 3)) for ci in range(5)])
    stack[0::3, 1, 1] = np.nan
    assert np.array_equal(seen[-1], np.nanmean(stack, axis=0))

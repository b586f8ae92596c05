#!/usr/bin/env python3
"""Golden vectors of the reference's quantify mode -- pattern_detector(coords=...) -- on the positions where its rules
are subtle, by IMPORTING THE REFERENCE (authoring container only, as make_golden.py does).

    PYTHONPATH=/root/reference python tests/golden/make_golden_quantify.py

quantify_edges.npz  one tiny intra block (80 bins, missing-bin clusters at both ends and inside, an empty region, regions
                    with a zero share just under and just over max_perc_zero) and one tiny trans block (44 x 60), each
                    with loops 17 x 17 and the non-square 5 x 9 template of nonsquare.npz: the requested coordinates and
                    the reference's table (bin1, bin2, score, pvalue) and windows, drop=False, under the loops preset's
                    tolerances and under loose ones (where the window bounds alone decide at the edges).  Positions: corners and
                    edges on either side of the strict window bounds, on / next to / inside the missing clusters, the
                    main diagonal, below it within and beyond max(km, kn) sub-diagonals, max_dist - 1 .. max_dist + 1
                    and far beyond, the crafted zero-share regions, horizontal runs, duplicates.
Arrays only; tests/test_quantify_oracle.py pins oracle/foci_oracle.py quantify_table / quantify_table_band on it."""
import pathlib
import sys

import numpy as np
import scipy.sparse as sp

REF = pathlib.Path("/root/reference")
sys.path.insert(0, str(REF))
import chromosight.utils.detection as cud  # noqa: E402

HERE = pathlib.Path(__file__).resolve().parent
LOOPS = np.loadtxt(REF / "chromosight" / "kernels" / "artificial_template_loops_type1.txt")
RECT = dict(np.load(HERE / "nonsquare.npz"))["d2_59_kernel"]
# (max_dist != 0: a 2-D pattern.)  "loops": the preset's tolerances; "loose": tolerances under which the zero frame of an edge
# window does not drop it, so that the strict window bounds alone decide there
CFGS = {"loops": dict(pearson=0.3, max_perc_undetected=50.0, max_perc_zero=10.0, max_dist=90),
        "loose": dict(pearson=0.3, max_perc_undetected=90.0, max_perc_zero=95.0, max_dist=90)}


class RefMap:
    def __init__(self, matrix, detectable_bins, max_dist, inter):
        self.matrix, self.detectable_bins, self.max_dist, self.inter, self.name = matrix, detectable_bins, max_dist, inter, "blk"


def zero_some(a, centre, count, rng, half=8):
    """`count` zero pixels in the 17 x 17 window around `centre` (none on its middle row / column, so the window of the
    5 x 9 template keeps its values)."""
    r, c = centre
    cells = [(i, j) for i in range(r - half, r + half + 1) for j in range(c - half, c + half + 1) if abs(i - r) > 2 and abs(j - c) > 4]
    for k in rng.choice(len(cells), count, replace=False):
        a[cells[k]] = 0.0


def intra_case():
    n, max_dist = 80, 45
    rng = np.random.default_rng(7)
    ii, jj = np.indices((n, n))
    a = rng.gamma(8.0, 0.125, size=(n, n))
    a[(jj < ii) | (jj - ii > max_dist + 17)] = 0.0               # prepared block: upper band of keep = max_dist + 17 diagonals
    zero_some(a, (12, 42), 28, rng)                                # 28 / 289 = 9.69 %: valid
    zero_some(a, (34, 64), 29, rng)                                # 29 / 289 = 10.03 %: dropped
    a[50:67, 62:79] = 0.0                                          # an empty region
    miss = np.zeros(n, dtype=bool)
    miss[[0, 1, 2, 40, 41, 42, 43, 44, 77, 78, 79]] = True
    a[miss, :] = 0.0
    a[:, miss] = 0.0
    edge = list(range(0, 11)) + list(range(n - 11, n))
    pts = [(r, c) for r in edge for c in edge]                     # the four corners and edges, both sides of the bounds
    pts += [(r, c) for r in range(33, 52, 2) for c in range(r - 2, r + 14, 3)]      # on / next to / inside the inner cluster
    pts += [(r, r) for r in range(9, 72, 7)]                       # the main diagonal
    pts += [(r, r - d) for r in (30, 55, 70) for d in (1, 2, 8, 16, 17, 18, 25)]   # below it, within and beyond 17 sub-diagonals
    pts += [(r, r + d) for r in (10, 20, 28) for d in (max_dist - 1, max_dist, max_dist + 1, max_dist + 9, max_dist + 30) if r + d < n]
    pts += [(12, 42), (34, 64), (58, 70), (58, 71), (13, 42), (34, 65)]            # the crafted regions
    pts += [(20, c) for c in range(22, 48)] + [(60, c) for c in range(55, 80)]     # runs: into max_dist, into the end
    pts += [(12, 42), (20, 30), (0, 0)]                            # duplicates
    return a, miss, miss, max_dist, np.array(pts, dtype=np.int64), False


def inter_case():
    shape = (44, 60)
    rng = np.random.default_rng(11)
    a = rng.gamma(2.0, 0.5, size=shape) * (rng.random(shape) < 0.97)
    a[20:40, 30:52] = 0.0                                          # an empty region
    zero_some(a, (10, 14), 20, rng)
    mr, mc = np.zeros(shape[0], dtype=bool), np.zeros(shape[1], dtype=bool)
    mr[[0, 1, 25, 26, 27, 43]] = True
    mc[[0, 12, 13, 14, 15, 16, 58, 59]] = True
    a[mr, :] = 0.0
    a[:, mc] = 0.0
    er = list(range(0, 11)) + list(range(shape[0] - 11, shape[0]))
    ec = list(range(0, 11)) + list(range(shape[1] - 11, shape[1]))
    pts = [(r, c) for r in er for c in ec[::2]] + [(r, c) for r in er[::3] for c in ec]
    pts += [(r, c) for r in range(18, 34, 3) for c in range(8, 24, 2)]
    pts += [(30, 41), (29, 40), (10, 14), (22, 22), (30, 10)]
    pts += [(15, c) for c in range(5, 55)]                         # a run across the missing columns
    pts += [(30, 41), (5, 5)]
    return a, mr, mc, None, np.array(pts, dtype=np.int64), True


def main():
    out = {f"cfg_{c}": np.array([v["pearson"], v["max_perc_undetected"], v["max_perc_zero"], v["max_dist"]]) for c, v in CFGS.items()}
    for name, case in (("intra", intra_case()), ("inter", inter_case())):
        a, mr, mc, max_dist, pts, inter = case
        m = sp.coo_matrix(a)
        m.eliminate_zeros()
        out[f"{name}_prepared"] = a
        out[f"{name}_miss_rows"], out[f"{name}_miss_cols"] = mr, mc
        out[f"{name}_max_dist"] = np.int64(-1 if max_dist is None else max_dist)
        out[f"{name}_coords"] = pts
        for kname, kern in (("loops", LOOPS), ("rect", RECT)):
            out[f"{name}_{kname}_kernel"] = kern
            for cname, cfg in CFGS.items():
                det = (np.flatnonzero(~mr), np.flatnonzero(~mc))
                cmap = RefMap(m.tocsr().copy(), det, max_dist, inter)
                tab, wins = cud.pattern_detector(cmap, dict(cfg), kern, coords=pts.copy(), full=True)
                out[f"{name}_{kname}_{cname}_table"] = tab[["bin1", "bin2", "score", "pvalue"]].to_numpy(dtype=np.float64)
                out[f"{name}_{kname}_{cname}_windows"] = wins
                print(name, kname, cname, len(pts), "positions,", int(np.isnan(tab.score).sum()), "invalid,", int((tab.score == 0).sum()), "scored 0")
    # blocks not larger than the template: nothing (:236-238)
    small = sp.csr_matrix(np.ones((17, 17)))
    tab, wins = cud.pattern_detector(RefMap(small, (np.arange(17), np.arange(17)), 5, False), dict(CFGS["loops"]), LOOPS,
                                     coords=np.array([[8, 8]]), full=True)
    assert tab is None and wins is None
    np.savez_compressed(HERE / "quantify_edges.npz", **out)


if __name__ == "__main__":
    main()

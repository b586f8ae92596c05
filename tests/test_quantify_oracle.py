"""Pins the quantify oracle (oracle/foci_oracle.py quantify_table / quantify_table_band, the point entry of oracle/oracle.c and
the CPU pipeline of tests/quantify_oracle_util.py) to the reference's own outputs: tests/golden/quantify_edges.npz
(make_golden_quantify.py: the positions where the rules are subtle), the quantify captures of example_blocks.npz and the
per-block, per-template tables of yeast_quantify.npz.  CPU only: the device grades nothing here."""
import numpy as np
import pytest

from oracle import c_oracle, foci_oracle
import quantify_oracle_util as qo

TIGHT = 1e-12


def _same(q, ref_table, ref_windows, what):
    """Scores within 1e-12, NaN patterns exact, windows exact, p-values to 1e-9 relative (log10 p through erfc)."""
    assert np.array_equal(np.column_stack([q["bin1"], q["bin2"]]), ref_table[:, :2]), what
    assert np.array_equal(np.isnan(q["score"]), np.isnan(ref_table[:, 2])), what
    ok = ~np.isnan(ref_table[:, 2])
    assert np.array_equal(ok, q["valid"]), what
    if ok.any():
        assert np.abs(q["score"][ok] - ref_table[ok, 2]).max() < TIGHT, what
    if ref_windows is not None:
        assert np.array_equal(q["windows"], ref_windows, equal_nan=True), what
    assert np.allclose(q["pvalue"], ref_table[:, 3], rtol=1e-9, atol=1e-300), what


def _edge_case(g, name, kname, cname):
    a = g[f"{name}_prepared"]
    mr, mc = g[f"{name}_miss_rows"], g[f"{name}_miss_cols"]
    md = int(g[f"{name}_max_dist"])
    kern = g[f"{name}_{kname}_kernel"]
    _, pu, pz, _ = g[f"cfg_{cname}"]
    return a, mr, mc, (None if md < 0 else md), kern, pu / 100, pz / 100


@pytest.mark.parametrize("cname", ["loops", "loose"])
@pytest.mark.parametrize("kname", ["loops", "rect"])
@pytest.mark.parametrize("name", ["intra", "inter"])
def test_quantify_oracle_on_the_edge_capture(golden, name, kname, cname):
    g = golden("quantify_edges")
    a, mr, mc, md, kern, mtol, ztol = _edge_case(g, name, kname, cname)
    inter = name == "inter"
    coords = g[f"{name}_coords"]
    ref, ref_w = g[f"{name}_{kname}_{cname}_table"], g[f"{name}_{kname}_{cname}_windows"]
    corr, nobs = c_oracle.normxcorr2(a, kern, max_dist=md, sym_upper=not inter, full=True, miss_row=mr, miss_col=mc, missing_tol=mtol)
    q = foci_oracle.quantify_table(a, corr, coords, mr, mc, kern.shape, ztol, mtol, inter=inter, max_dist=md, n_obs=nobs)
    _same(q, ref, ref_w, (name, kname, cname))
    # the point entry of the C oracle == its map entry, bit for bit; the pipeline helpers through it == the capture
    rr, cc = np.repeat(np.arange(-2, a.shape[0] + 2), a.shape[1] + 4), np.tile(np.arange(-2, a.shape[1] + 2), a.shape[0] + 4)
    pc, pn, _, _ = c_oracle.normxcorr2_points(a, a.shape, kern, rr, cc, max_dist=md, sym_upper=not inter, full=True, miss_row=mr,
                                              miss_col=mc, missing_tol=mtol)
    inside = (rr >= 0) & (rr < a.shape[0]) & (cc >= 0) & (cc < a.shape[1])
    assert np.array_equal(pc[inside], corr.ravel()) and np.array_equal(pn[inside], nobs.ravel()) and not pc[~inside].any()
    cfg = dict(max_perc_undetected=mtol * 100, max_perc_zero=ztol * 100, max_dist=90)
    if inter:
        q2 = qo.quantify_inter(a, mr, mc, kern, coords, cfg)
    else:
        n = a.shape[0]
        band = np.zeros((n, n))
        for d in range(n):
            band[:n - d, d] = np.diagonal(a, d)
        q2 = qo.quantify_intra(band, mr, kern, coords, cfg, md)
        lo = -8                      # (a template wider than tall has coefficients on its first kn - km sub-diagonals)
        cb = np.zeros((n, n - lo))
        nb = np.full((n, n - lo), float(kern.size))
        for d in range(lo, n):
            i = np.arange(max(0, -d), min(n, n - d))
            cb[i, d - lo], nb[i, d - lo] = corr[i, i + d], nobs[i, i + d]
        q3 = foci_oracle.quantify_table_band(band, 0, cb, lo, n, coords, mr, kern.shape, ztol, mtol, md, n_obs_band=nb)
        _same(q3, ref, ref_w, (name, kname, cname, "band"))
    _same(q2, ref, ref_w, (name, kname, cname, "points"))
    for f in ("inside", "n_zero", "n_missing", "score"):
        assert np.array_equal(q[f], q2[f], equal_nan=True)


def test_edge_capture_holds_every_position_class(golden):
    """The capture is only a pin if both sides of every rule occur in it (statistics from the pinned oracle)."""
    g = golden("quantify_edges")
    a, mr, mc, md, kern, mtol, ztol = _edge_case(g, "intra", "loops", "loops")
    n = a.shape[0]
    coords = g["intra_coords"]
    corr, nobs = c_oracle.normxcorr2(a, kern, max_dist=md, sym_upper=True, full=True, miss_row=mr, miss_col=mc, missing_tol=mtol)
    q = foci_oracle.quantify_table(a, corr, coords, mr, mc, kern.shape, ztol, mtol, max_dist=md, n_obs=nobs)
    loose = g["intra_loops_loose_table"]
    r, c = coords[:, 0], coords[:, 1]
    d = c - r
    tot = kern.size
    with np.errstate(all="ignore"):
        pu, pz = q["n_missing"] / tot, q["n_zero"] / (tot - q["n_missing"])
    # strict bounds: inside for rows 0 .. n - 2, outside at n - 1 (low < H), and both occur with a VALID loose score beside
    assert q["inside"][(r == 0) & (c == 0)].all() and not q["inside"][r == n - 1].any() and not q["inside"][c == n - 1].any()
    assert q["inside"][(r == n - 2) & (c == n - 2)].all()
    assert (~np.isnan(loose[:, 2]) & ((r <= 8) | (c >= n - 10))).any()
    assert (q["inside"] & (pu >= 0.4) & (pu < mtol)).any() and (q["inside"] & (pu >= mtol) & (pu < 0.6)).any()
    assert (q["inside"] & (pu < mtol) & (pz > 0.09) & (pz < ztol)).any() and (q["inside"] & (pu < mtol) & (pz >= ztol) & (pz < 0.11)).any()
    assert (q["inside"] & (pz == 1.0)).any()
    assert (d == 0).any() and ((d < 0) & (d >= -17)).any() and (d < -17).any()
    for dd in (md - 1, md, md + 1):
        assert (d == dd).any()
    assert (d > md + 20).any()
    # a valid window beyond max_dist, or below the diagonal, scores 0.0 -- not NaN
    assert (~np.isnan(loose[:, 2]) & (d > md) & (loose[:, 2] == 0)).any() and (~np.isnan(loose[:, 2]) & (d < 0) & (loose[:, 2] == 0)).any()
    assert (~np.isnan(loose[:, 2]) & (d == md) & (loose[:, 2] != 0)).any()
    assert len(coords) > len(np.unique(coords, axis=0))                     # duplicates
    # blocks not larger than the template return nothing
    q0 = foci_oracle.quantify_table(np.ones((17, 17)), np.ones((17, 17)), np.array([[8, 8]]), np.zeros(17, bool), np.zeros(17, bool),
                                    (17, 17), 0.1, 0.5, max_dist=5)
    assert not q0["scanned"] and np.isnan(q0["score"]).all() and np.isnan(q0["windows"]).all()


def test_quantify_oracle_on_the_example_captures(golden, templates):
    g = golden("example_blocks")
    kern = np.asarray(templates["loops"], dtype=np.float64)

    def dense(prefix):
        import scipy.sparse as sp
        return sp.coo_matrix((g[f"{prefix}_val"], (g[f"{prefix}_row"], g[f"{prefix}_col"])), shape=tuple(g[f"{prefix}_shape"])).toarray()
    m = dense("quant_prepared")
    n = m.shape[0]
    miss = np.ones(n, dtype=bool)
    miss[g["quant_det"]] = False
    md = int(g["quant_max_dist"])
    corr, nobs = c_oracle.normxcorr2(m, kern, max_dist=md, sym_upper=True, full=True, miss_row=miss, miss_col=miss, missing_tol=0.5)
    q = foci_oracle.quantify_table(m, corr, g["quant_coords"], miss, miss, kern.shape, 0.1, 0.5, max_dist=md, n_obs=nobs)
    _same(q, g["quant_table"], g["quant_windows"], "example intra")
    m = dense("inter_prepared")
    mr, mc = np.ones(m.shape[0], bool), np.ones(m.shape[1], bool)
    mr[g["inter_det_rows"]] = False
    mc[g["inter_det_cols"]] = False
    corr, nobs = c_oracle.normxcorr2(m, kern, full=True, miss_row=mr, miss_col=mc, missing_tol=0.5)
    q = foci_oracle.quantify_table(m, corr, g["inter_coords"], mr, mc, kern.shape, 0.1, 0.5, inter=True, n_obs=nobs)
    _same(q, g["inter_table"], g["inter_windows"], "example inter")


def test_quantify_pipeline_oracle_on_the_yeast_capture(golden):
    """Every block and template of yeast_quantify.npz (11 x 11 borders templates, 17 intra and 7 trans blocks) rebuilt from the
    decoded .cool by the oracle pipeline (balancing, distance law, detrend, median scaling included): NaN pattern exact, scores
    within 1e-12, p-values to 1e-6 relative."""
    cool, g = golden("yeast_cool"), golden("yeast_quantify")
    md = int(g["max_dist"])
    cfg = dict(max_perc_undetected=75.0, max_perc_zero=10.0, max_dist=int(g["cfg_max_dist_bp"]))
    n_rows, worst = 0, 0.0
    for bi in range(int(g["n_blocks"])):
        ca, cb = (int(x) for x in g[f"b{bi}_chroms"])
        coords = g[f"b{bi}_coords"]
        if ca == cb:
            prepared, miss = qo.intra_block(cool, ca, md, 11)
        else:
            dense, mr, mc = qo.inter_block(cool, ca, cb)
        for ki in range(3):
            if f"b{bi}_k{ki}_table" not in g or not g[f"b{bi}_k{ki}_table"].shape[0]:
                continue
            ref = g[f"b{bi}_k{ki}_table"]
            kern = g[f"kernel{ki}"]
            q = qo.quantify_intra(prepared, miss, kern, coords, cfg, md) if ca == cb else qo.quantify_inter(dense, mr, mc, kern, coords, cfg)
            assert np.array_equal(np.column_stack([q["bin1"], q["bin2"]]), ref[:, :2])
            assert np.array_equal(np.isnan(q["score"]), np.isnan(ref[:, 2])), (bi, ki)
            ok = ~np.isnan(ref[:, 2])
            if ok.any():
                worst = max(worst, float(np.abs(q["score"][ok] - ref[ok, 2]).max()))
            assert np.allclose(q["pvalue"], ref[:, 3], rtol=1e-6, atol=1e-300), (bi, ki)
            n_rows += ref.shape[0]
    print(f"yeast capture: {n_rows} rows, max |score - reference| {worst:.2e}")
    assert n_rows > 6000 and worst < TIGHT


def test_pipeline_oracle_selection_on_the_reference_capture(golden):
    """quantify_oracle_util.quantify_genome end to end -- midpoints scored, three templates, cmd_quantify's sort / groupby /
    tail selection, bins of the interval starts, final order -- against yeast_quantify_select.npz (the reference's selection on
    its own per-template tables): rows, order and picked template exact, scores within 1e-12, p-values to 1e-6 relative."""
    import pandas as pd
    cool, q, g = golden("yeast_cool"), golden("yeast_quantify"), golden("yeast_quantify_select")
    num = g["positions_num"]
    positions = pd.DataFrame({"chrom1": g["positions_chrom1"], "start1": num[:, 0], "end1": num[:, 1],
                              "chrom2": g["positions_chrom2"], "start2": num[:, 2], "end2": num[:, 3]})
    cfg = dict(max_perc_undetected=75.0, max_perc_zero=10.0, max_dist=0, kernels=[q[f"kernel{ki}"] for ki in range(3)])
    res, pick = qo.quantify_genome(cool, positions, cfg, inter=True, max_dist_bp=int(q["cfg_max_dist_bp"]))
    assert len(pick) == g["final_num"].shape[0]
    assert pick["chrom1"].tolist() == g["final_chrom1"].tolist() and pick["chrom2"].tolist() == g["final_chrom2"].tolist()
    assert np.array_equal(pick[["start1", "end1", "start2", "end2", "bin1", "bin2"]].to_numpy(dtype=np.int64), g["final_num"])
    got, ref = pick[["score", "pvalue"]].to_numpy(dtype=np.float64), g["final_val"]
    assert np.array_equal(np.isnan(got), np.isnan(ref[:, :2]))
    assert np.nanmax(np.abs(got[:, 0] - ref[:, 0])) < TIGHT
    assert np.allclose(got[:, 1], ref[:, 1], equal_nan=True, rtol=1e-6, atol=1e-300)
    assert np.array_equal(pick["qvalue_nan"].to_numpy(), np.isnan(ref[:, 2]))
    fin = ~np.isnan(ref[:, 0])
    # (the picked template where it is decided by more than rounding: two of these templates tie to 1e-15 on some windows)
    src = pick["src"].to_numpy()
    per_template = np.sort(np.nan_to_num(np.column_stack([d["score"][src] for d in res]), nan=-np.inf), axis=1)
    clear = fin & (per_template[:, 2] - per_template[:, 1] > 1e-9)
    assert clear.sum() > 900 and np.array_equal(pick["kernel_id"].to_numpy()[clear], g["picked_template"][clear])
    assert len(set(g["picked_template"][clear])) == 3


def test_tsvd_kernel_oracle(golden, templates):
    from oracle import pearson_oracle as orc
    g = golden("xcorr2")
    k = np.asarray(templates["loops"], dtype=np.float64)
    assert np.abs(orc.tsvd_kernel_oracle(k, 0.999) - g["loops_tsvd999_u"] @ g["loops_tsvd999_v"]).max() < TIGHT
    assert np.abs(orc.tsvd_kernel_oracle(k, 1.0 - 1e-15) - k).max() < TIGHT        # every triplet: the template itself


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_smooth_and_tsvd_oracles_on_the_reference_detect_tables(golden, templates, ci):
    """The isotonic law (detrend_oracle.prepare_band(smooth=True)) and the truncated template (pearson_oracle.tsvd_kernel_oracle,
    for the correlation sums and, from the squared template, for the masked square sums) through the detect oracles against
    the reference's `--smooth-trend` / `--tsvd` tables of options.npz: same foci in the same order; scores within 1e-9, the
    bound of the other detect-oracle comparisons (a law refitted in another pooling order moves a coefficient by 1e-15)."""
    from oracle import detrend_oracle, pearson_oracle as orc
    cool, g = golden("example_cool"), golden("options")
    kern = np.asarray(templates["loops"], dtype=np.float64)
    md = 2000000 // int(cool["binsize"])
    n = int(cool["chrom_offset"][ci + 1] - cool["chrom_offset"][ci])
    for tag in ("smooth", "tsvd"):
        prepared, miss = qo.intra_block(cool, ci, md, 17, smooth=tag == "smooth")
        dense = np.zeros((n, n))
        for d in range(min(prepared.shape[1], n)):
            dense[np.arange(n - d), np.arange(n - d) + d] = prepared[:n - d, d]
        kc, k2 = (orc.tsvd_kernel_oracle(kern), orc.tsvd_kernel_oracle(kern ** 2)) if tag == "tsvd" else (None, None)
        corr, _ = c_oracle.normxcorr2(dense, kern, max_dist=md, sym_upper=True, full=True, miss_row=miss, miss_col=miss,
                                      missing_tol=0.5, kernel_conv=kc, kernel_sq=k2)
        ii, jj = np.indices((n, n))
        trimmed = np.where((jj - ii >= 0) & (jj - ii <= md), corr, 0.0)
        tab = foci_oracle.detect_table(dense, trimmed, miss, miss, kern.shape, 0.3, 0.1, 0.5)
        ref = g[f"loops_{tag}_c{ci}_k0"]
        assert ref.shape[0] > 5 and tab.shape[0] == ref.shape[0], (tag, ci)
        assert np.array_equal(tab[:, :2], ref[:, :2]), (tag, ci)
        worst = float(np.abs(tab[:, 2] - ref[:, 2]).max())
        print(f"{tag} chr{ci}: {ref.shape[0]} foci, max |score - reference| {worst:.2e}")
        assert worst < 1e-9, (tag, ci, worst)
        # the same coefficients from the point entry (what the quantify pipeline uses)
        pc, _, _, _ = c_oracle.normxcorr2_points(prepared, (n, n), kern, tab[:, 0].astype(int), tab[:, 1].astype(int), band_lo=0,
                                                 max_dist=md, sym_upper=True, full=True, miss_row=miss, miss_col=miss,
                                                 missing_tol=0.5, kernel_conv=kc, kernel_sq=k2)
        assert np.array_equal(pc, tab[:, 2]), (tag, ci)

"""Plain reference of focus labelling, and candidate lists of known shape for the tests of the device labelling
(tests/test_gpu_label_foci.py).  numpy / scipy only, nothing of chromosight_amd.

The operation (pick_foci / label_foci / filter_foci of the reference): the 4-connected components of a set of pixels, the ones of
fewer than min_size pixels dropped, each reported at the first row-major pixel that holds its maximum together with its size, in
the order of the components' first pixels (label order).  With diag_only = d (odd codes of the 1-D patterns) the reported row is
col + (d >> 1).  Pinned to oracle/foci_oracle.pick_foci_dense by tests/test_label_reference.py.
"""
import numpy as np
from scipy import ndimage as ndi

FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def label_reference(shape, rows, cols, vals, min_size=2, diag_only=0):
    """Foci of the candidate list (distinct in-range pixels, any order) -> (rows, cols, sizes), int64 arrays in label order.
    Only the rows between the first and the last candidate are held densely, so a matrix of 65 536 x 65 536 is fine as long as the
    candidates span a few rows."""
    ms, ns = int(shape[0]), int(shape[1])
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    empty = np.zeros(0, dtype=np.int64)
    if rows.size == 0:
        return empty, empty, empty
    assert rows.min() >= 0 and rows.max() < ms and cols.min() >= 0 and cols.max() < ns
    r0 = int(rows.min())
    h = int(rows.max()) - r0 + 1
    mask = np.zeros((h, ns), dtype=bool)
    mask[rows - r0, cols] = True
    assert int(mask.sum()) == rows.size, "duplicate pixels are outside the contract"
    dense = np.zeros((h, ns), dtype=np.float64)
    dense[rows - r0, cols] = vals
    labels, n_lab = ndi.label(mask, structure=FOUR)          # numbered in raster order of each component's first pixel
    rr, cc = np.nonzero(mask)                                # row-major
    lab = labels[rr, cc]
    v = dense[rr, cc]
    order = np.argsort(lab, kind="stable")                   # by label, row-major inside a label
    rr, cc, lab, v = rr[order], cc[order], lab[order], v[order]
    starts = np.flatnonzero(np.concatenate([[True], lab[1:] != lab[:-1]]))
    ends = np.concatenate([starts[1:], [lab.size]])
    out_r, out_c, out_s = [], [], []
    for s, e in zip(starts, ends):
        if e - s < min_size:
            continue
        k = s + int(np.argmax(v[s:e]))                       # first maximum in row-major order
        out_r.append(cc[k] + (diag_only >> 1) if diag_only else rr[k] + r0)
        out_c.append(cc[k])
        out_s.append(e - s)
    return np.array(out_r, dtype=np.int64), np.array(out_c, dtype=np.int64), np.array(out_s, dtype=np.int64)


# ---- candidate lists of known shape: each returns ((ms, ns), rows, cols) in row-major order ------------------------------------
def _from_mask(mask):
    rows, cols = np.nonzero(mask)
    return mask.shape, rows.astype(np.int64), cols.astype(np.int64)


def solid(h, w, margin=(1, 2)):
    """An h x w rectangle inside a matrix with a margin."""
    mask = np.zeros((h + 2 * margin[0], w + 2 * margin[1]), dtype=bool)
    mask[margin[0]:margin[0] + h, margin[1]:margin[1] + w] = True
    return _from_mask(mask)


def snake(ms, ns):
    """A one-pixel serpentine that fills the matrix: every even row, joined to the next one at alternating ends.  One component
    whose union-find tree has to be built from ms / 2 long runs meeting at single pixels."""
    mask = np.zeros((ms, ns), dtype=bool)
    mask[0::2] = True
    odd = np.arange(1, ms, 2)
    mask[odd, np.where((odd // 2) % 2 == 0, ns - 1, 0)] = True
    return _from_mask(mask)


def comb(ms, ns):
    """Vertical teeth on the even columns, joined by the last row only: the one component is known only once the last row's
    unions have gone through."""
    mask = np.zeros((ms, ns), dtype=bool)
    mask[:, 0::2] = True
    mask[ms - 1] = True
    return _from_mask(mask)


def spiral(s):
    """A square spiral, one pixel wide with one-pixel gaps, from the corner inwards (one component): walk ahead while the next
    cell is free and the one beyond it is not part of an older arm, else turn right; stop when neither is possible."""
    mask = np.zeros((s, s), dtype=bool)

    def inside(r, c):
        return 0 <= r < s and 0 <= c < s

    r, c, dr, dc = 0, 0, 0, 1
    mask[0, 0] = True
    while True:
        for _ in range(2):
            nr, nc = r + dr, c + dc
            if inside(nr, nc) and not mask[nr, nc] and not (inside(nr + dr, nc + dc) and mask[nr + dr, nc + dc]):
                break
            dr, dc = dc, -dr                                 # right turn
        else:
            break
        r, c = nr, nc
        mask[r, c] = True
    assert ndi.label(mask, structure=FOUR)[1] == 1
    return _from_mask(mask)


def column(ms, ns=3, col=1):
    mask = np.zeros((ms, ns), dtype=bool)
    mask[:, col] = True
    return _from_mask(mask)


def row(ns, ms=3, at=1):
    mask = np.zeros((ms, ns), dtype=bool)
    mask[at, :] = True
    return _from_mask(mask)


def checkerboard(ms, ns):
    """Nothing merges: every pixel is a focus of its own."""
    ii, jj = np.indices((ms, ns))
    return _from_mask((ii + jj) % 2 == 0)


def diagonal_touch(s):
    """Two s x s squares that touch only at a corner: two components under the 4-neighbourhood."""
    mask = np.zeros((2 * s, 2 * s), dtype=bool)
    mask[:s, :s] = True
    mask[s:, s:] = True
    return _from_mask(mask)


def random_pixels(n, density, seed):
    """Exactly n pixels of a square matrix of about n / density pixels, in row-major order."""
    side = int(np.ceil(np.sqrt(n / density)))
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(side * side, size=n, replace=False))
    return (side, side), (keys // side).astype(np.int64), (keys % side).astype(np.int64)


def corner_l(ms, ns, arm=4):
    """For the key widths: an L-shaped focus whose last pixel is the last pixel of the matrix (arms along the last column and the
    last row, cut to the matrix), and one row-wrap pair (r, ns - 1), (r + 1, 0) -- consecutive keys, not neighbours -- above it.
    Everything lies in the last few rows.  A matrix of one column has no wrap pair (its consecutive keys ARE neighbours)."""
    px = {(ms - 1 - k, ns - 1) for k in range(min(arm, ms))} | {(ms - 1, ns - 1 - k) for k in range(min(arm + 1, ns))}
    if ns >= 2 and ms >= arm + 4:
        px |= {(ms - arm - 3, ns - 1), (ms - arm - 2, 0)}
    px = sorted(px)
    return (ms, ns), np.array([p[0] for p in px], dtype=np.int64), np.array([p[1] for p in px], dtype=np.int64)

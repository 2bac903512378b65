"""NumPy / SciPy restatements of the class-map clean-up (K20), written from the semantics in the feature's description, not
from the kernels.

Majority filter: k x k window (k odd), centred on the pixel and clipped to the image (cells outside do not vote).  `ignore`
pixels never vote and never change; `fill` pixels never vote and take the window's winner when the window has a voter;
fill_only: every pixel that is not `fill` keeps its value.  Winner: most votes; on a tie the centre's own label when it votes
and is among the maxima, else the smallest tied label.  Counters: n_changed (output != input), n_unfilled (`fill` pixels still
`fill`).

Sieve: pixels are connected when they are 8- (or 4-) neighbours, hold the same label, and the label is not `ignore`; components
of fewer than min_area pixels become removed_value; n_removed counts their pixels.

clean: sieve to a temporary hole value (the largest byte value that neither occurs nor is nodata), fill_only majority passes
until no hole is left / a pass fills none / max_fill_iterations, leftovers to nodata, then ordinary majority passes."""
import numpy as np


def voters(q, ignore=-1, fill=-1):
    v = np.ones(q.shape, bool)
    if ignore >= 0:
        v &= q != ignore
    if fill >= 0:
        v &= q != fill
    return v


def box_count(onehot, k):
    """k x k box counts of a 0 / 1 plane by shifted adds over a zero-padded copy (outside cells do not vote): k shifts along
    the rows, then k along the columns."""
    H, W = onehot.shape
    R = k // 2
    pad = np.zeros((H + 2 * R, W + 2 * R), np.int32)
    pad[R:R + H, R:R + W] = onehot
    rows = np.zeros((H + 2 * R, W), np.int32)
    for dx in range(k):
        rows += pad[:, dx:dx + W]
    cnt = np.zeros((H, W), np.int32)
    for dy in range(k):
        cnt += rows[dy:dy + H]
    return cnt


def tie_kinds(q, k, ignore=-1, fill=-1):
    """(pixels that vote, share the largest count with another label and so keep their label by the centre rule,
        pixels whose window's largest count is shared by several labels none of which is the pixel's own voting label:
        the smallest-label rule decides) — counted from the box counts alone."""
    q = np.asarray(q, np.uint8)
    voter = voters(q, ignore, fill)
    labels = np.unique(q[voter])
    cnts = np.stack([box_count(voter & (q == lab), k) for lab in labels])
    best = cnts.max(axis=0)
    n_max = (cnts == best).sum(axis=0)
    own = np.zeros(q.shape, np.int32)
    for i, lab in enumerate(labels):
        mine = voter & (q == lab)
        own[mine] = cnts[i][mine]
    tied = (n_max > 1) & (best > 0)
    centre = tied & voter & (own == best)
    decides = tied & ~centre & ((q != ignore) if ignore >= 0 else True)
    return int(centre.sum()), int(decides.sum())


def majority_ref(q, k, ignore=-1, fill=-1, fill_only=False):
    q = np.asarray(q, np.uint8)
    H, W = q.shape
    voter = voters(q, ignore, fill)
    labels = np.unique(q[voter])                         # ascending: the first maximum is the smallest tied label
    best = np.zeros((H, W), np.int32)
    win = np.zeros((H, W), np.int32)
    own = np.zeros((H, W), np.int32)                     # votes for the centre's own label (0 where the centre does not vote)
    for lab in labels:
        cnt = box_count(voter & (q == lab), k)
        better = cnt > best
        win[better] = lab
        best[better] = cnt[better]
        mine = voter & (q == lab)
        own[mine] = cnt[mine]
    keep_centre = voter & (own == best)                  # own >= 1 there, so best >= 1
    winner = np.where(keep_centre, q, win).astype(np.uint8)
    has_voter = best > 0
    out = q.copy()
    if fill >= 0:
        f = (q == fill) & has_voter
        out[f] = winner[f]
    if not fill_only:
        out[voter] = winner[voter]                        # a voter's window holds itself
    n_changed = int((out != q).sum())
    n_unfilled = int(((q == fill) & (out == fill)).sum()) if fill >= 0 else 0
    return out, n_changed, n_unfilled


def sieve_ref(q, min_area, connectivity=8, ignore=0, removed_value=0):
    from scipy import ndimage
    q = np.asarray(q, np.uint8)
    out = q.copy()
    n_removed = 0
    if min_area <= 1:
        return out, 0
    structure = np.ones((3, 3), int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    for lab in np.unique(q):
        if lab == ignore:
            continue
        comp, n = ndimage.label(q == lab, structure=structure)
        area = np.bincount(comp.ravel(), minlength=n + 1)
        small = (area[comp] < min_area) & (comp > 0)
        out[small] = removed_value
        n_removed += int(small.sum())
    return out, n_removed


def hole_value_ref(q, nodata):
    present = set(np.unique(q).tolist())
    for v in range(255, -1, -1):
        if v not in present and v != nodata:
            return v
    raise ValueError("no free byte value")


def clean_ref(q, min_area=0, window=3, nodata=0, max_fill_iterations=64, majority_iterations=0, connectivity=8):
    q = np.asarray(q, np.uint8)
    hole = hole_value_ref(q, nodata)
    cur, removed = sieve_ref(q, min_area, connectivity, ignore=nodata, removed_value=hole)
    unfilled, fill_iterations = removed, 0
    while unfilled > 0 and fill_iterations < max_fill_iterations:
        cur, _, left = majority_ref(cur, window, ignore=nodata, fill=hole, fill_only=True)
        fill_iterations += 1
        stalled = left >= unfilled
        unfilled = left
        if stalled:
            break
    if unfilled:
        cur = cur.copy()
        cur[cur == hole] = nodata
    changed = []
    for _ in range(majority_iterations):
        cur, nc, _ = majority_ref(cur, window, ignore=nodata)
        changed.append(nc)
        if nc == 0:
            break
    stats = {"removed": removed, "filled": removed - unfilled, "left_as_nodata": unfilled, "fill_iterations": fill_iterations, "changed": changed}
    return cur, stats

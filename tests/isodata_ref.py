"""NumPy / Python-int restatement of K26 (rsseg_isodata_sweep, include/rsseg.h), operation for operation.

A pixel is counted when its mask byte is non-zero (mask None: all).
float32 planes: v_f = the value, NaN read as +0; u_f = v_f * 2^plane_exp[f] in float64 (exact); a counted pixel with any
|u_f| > 1 (+-inf included) is left out.  uint8 planes: u_f = v_f (plane_exp None, Q 0), no pixel is left out.
Per counted pixel that is not left out, in float64, every operation rounded once:
  z_f = u_f * weight[f];  d_j = +0.0, then for f ascending  t = z_f - c_jf;  d_j = d_j + t * t
  label = the lowest j with the strictly smallest d_j (np.argmin: the first minimum);  n_changed += label != labels_in
  row label:  column 0 += 1;  column 1 + f += rint(u_f * 2^Q);  column 1 + F + f += rint((u_f * 2^Q) * u_f)
Every other pixel gets label 255, enters no column and is not counted in n_changed.  The sums are Python ints."""
import numpy as np


def n_columns(F: int) -> int:
    return 1 + 2 * F


def sweep_ref(planes, mask, plane_exp, Q, weight, centers, labels_in):
    """planes: (F, n) float32 or uint8; mask: None or (n,); weight (F,); centers (k, F) in weighted units; labels_in (n,) uint8
    -> (labels uint8 (n,), table: k rows of 1 + 2 F Python ints, n_changed, n_left_out)."""
    planes = np.asarray(planes)
    F, n = planes.shape
    weight = np.asarray(weight, np.float64).reshape(F)
    centers = np.asarray(centers, np.float64)
    k = centers.shape[0]
    assert centers.shape == (k, F) and 1 <= k <= 64 and 0 <= Q <= 50 and (n << Q) < 2 ** 62
    assert np.all(np.isfinite(weight)) and np.all(np.isfinite(centers))
    labels_in = np.asarray(labels_in, np.uint8).reshape(-1)
    assert labels_in.size == n
    counted = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if planes.dtype == np.uint8:
        assert plane_exp is None and Q == 0
        u = planes.astype(np.float64)
        out_of_range = np.zeros(n, bool)
    else:
        assert planes.dtype == np.float32
        x = planes.astype(np.float64)
        x[np.isnan(x)] = 0.0
        with np.errstate(over="ignore"):
            u = np.ldexp(x, np.asarray(plane_exp, np.int64).reshape(F, 1))
        out_of_range = np.any(~(np.abs(u) <= 1.0), axis=0)
    n_left = int((counted & out_of_range).sum())
    keep = np.flatnonzero(counted & ~out_of_range)
    u = u[:, keep]
    with np.errstate(over="ignore"):
        z = u * weight.reshape(F, 1)
        d = np.zeros((k, keep.size))
        for j in range(k):
            for f in range(F):
                t = z[f] - centers[j, f]
                d[j] = d[j] + t * t
    lab = np.argmin(d, axis=0).astype(np.uint8) if keep.size else np.zeros(0, np.uint8)
    labels = np.full(n, 255, np.uint8)
    labels[keep] = lab
    n_changed = int((lab != labels_in[keep]).sum())
    two_q = float(2 ** Q)
    table = [[0] * n_columns(F) for _ in range(k)]
    xq = u * two_q
    s1 = np.rint(xq).astype(np.int64)
    s2 = np.rint(xq * u).astype(np.int64)
    for j in np.unique(lab):
        sel = lab == j
        row = table[int(j)]
        row[0] = int(sel.sum())
        for f in range(F):
            row[1 + f] = int(s1[f, sel].sum())        # |term| <= 2^Q and n 2^Q < 2^62: the int64 sum is the exact one
            row[1 + F + f] = int(s2[f, sel].sum())
    return labels, table, n_changed, n_left


def table_array(table) -> np.ndarray:
    """The Python-int table as int64 (every entry is below 2^62 by the limits)."""
    return np.array(table, dtype=np.int64).reshape(len(table), -1)


def ref_sweep(planes, labels, centers, weight, plane_exp, Q, mask=None, want_table=True):
    """Context.isodata_sweep's signature on host arrays: planes a sequence of flat float32 or uint8 arrays, `labels` a uint8
    array rewritten in place.  What isodata(..., sweep=ref_sweep) runs without a GPU."""
    P = np.stack([np.asarray(p).reshape(-1) for p in planes])
    lab, table, changed, left = sweep_ref(P, mask, plane_exp, Q, weight, centers, labels)
    labels[...] = lab
    return (table_array(table) if want_table else None), changed, left

"""NumPy restatement of K30 (rsseg_mlp_classify): multi-layer perceptron classification, in float32 unless said otherwise,
every operation one IEEE operation.

A model is a dict: widths (F, the hidden widths, the output units: k for k >= 3, 1 for k = 2); weights, a list of W_l
[widths[l-1]][widths[l]] float32 (scikit-learn's coefs_); biases, a list of b_l [widths[l]] float32; offset[F], scale[F]
float32; activation 'relu' | 'identity' | 'logistic' | 'tanh'; class_values[k] (uint8, distinct, 1..255).  Per pixel:
  x_f = the plane value, a NaN read as +0; a pixel with any +-inf x_f gets label 0 and margin, confidence, probabilities NaN
  z_f = (x_f - offset_f) * scale_f;  h_0 = z
  layer l, unit j: a = b_l[j]; i ascending: a = fmaf(h_(l-1)[i], W_l[i][j], a);  h_l[j] = activation(a) on the hidden layers
    relu a > 0 ? a : +0;  identity a
    logistic, in float64 on the widened a: e = svm_exp(-|a|); d = 1 + e; a >= 0 ? 1 / d : e / d; rounded once to float32
    tanh: |a| < 2^-13 gives a; otherwise in float64 e = svm_exp(-(2 |a|)); t = (1 - e) / (1 + e); a < 0 ? -t : t; rounded once
  o_j = the last layer's a, for k = 2 the logits (+0, o_0)
  winner: w = 0, j ascending replaces w when o_j > o_w or when o_w is a NaN and o_j is not; second: the same over the others
  label = class_values[winner];  margin = o_win - o_second (float32)
  in float64: d_j = o_j - o_win; s = +0, j ascending s = s + svm_exp(d_j);  conf = float32(1 / s);  p_j = float32(svm_exp(d_j) / s)
svm_exp is svm_ref's (K28's).

fma32 is the float32 fused multiply-add: the product of two float32 is exact in float64 (48 bits); TwoSum gives the float64 sum
of it and the accumulator with its error; the sum is rounded TO ODD in float64 (53 >= 24 + 2 bits, so the second rounding, to
float32, is the one rounding of the exact value, also onto float32 subnormals); a plain (a * b + c).astype(float32) rounds twice
and goes wrong on an exact tie of the float64 sum (tests/test_mlp_host.py builds such operands).

`reverse=True` runs every chain with i DESCENDING: not the contract, but what an instruction that summed in another order
would give; the tests use it to show that a case can tell the orders apart."""
import numpy as np

from svm_ref import svm_exp

ACTIVATIONS = ("relu", "identity", "logistic", "tanh")


def fma32(a, b, c) -> np.ndarray:
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)      # exact
        c = c.astype(np.float64)
        s = np.ascontiguousarray(p + c)
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                        # TwoSum: p + c = s + e exactly (finite s)
        bits = s.view(np.int64)
        fix = np.isfinite(s) & (e != 0) & ((bits & 1) == 0)
        # s + e lies between s and its neighbour on e's side; that neighbour's last bit is odd.  Away from zero raises the bit
        # pattern, towards zero lowers it (s == 0 with e != 0 cannot occur: the sum would be e itself)
        step = np.where((e > 0) == (s > 0), 1, -1)
        odd = np.where(fix, bits + step, bits).view(np.float64)
        return odd.astype(np.float32)


def activation(a, name: str) -> np.ndarray:
    a = np.asarray(a, np.float32)
    with np.errstate(all="ignore"):
        if name == "relu":
            return np.where(a > 0, a, np.float32(0.0)).astype(np.float32)
        if name == "identity":
            return a
        x = a.astype(np.float64)
        ax = np.abs(x)
        if name == "logistic":
            e = svm_exp(-ax)
            d = 1.0 + e
            return np.where(x >= 0.0, 1.0 / d, e / d).astype(np.float32)
        if name == "tanh":
            e = svm_exp(-(2.0 * ax))
            t = (1.0 - e) / (1.0 + e)
            return np.where(ax < 2.0 ** -13, a, np.where(x < 0.0, -t, t).astype(np.float32)).astype(np.float32)
    raise ValueError(name)


def scaled(X, model):
    """(z (n, F) float32 with the refused pixels' rows from x = 0, refused (n,) bool)."""
    x = np.array(X, dtype=np.float32)
    x[np.isnan(x)] = 0.0
    bad = np.isinf(x).any(axis=1)
    x[bad] = 0.0
    with np.errstate(all="ignore"):
        z = (x - np.asarray(model["offset"], np.float32)) * np.asarray(model["scale"], np.float32)
    return z.astype(np.float32), bad


def layer_sums(h, W, b, reverse=False) -> np.ndarray:
    """a[n][units]: from the bias, i ascending (descending with reverse), a = fmaf(h[:, i], W[i, :], a)."""
    W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
    a = np.broadcast_to(b, (h.shape[0], b.size)).astype(np.float32)
    order = range(W.shape[0] - 1, -1, -1) if reverse else range(W.shape[0])
    for i in order:
        a = fma32(h[:, i, None], W[i][None, :], a)
    return a


def forward(z, model, reverse=False):
    """(logits o (n, k) float32, the sums a of every layer, a list of (n, widths[l]))."""
    h, sums = z, []
    L = len(model["weights"])
    for l in range(L):
        a = layer_sums(h, model["weights"][l], model["biases"][l], reverse)
        sums.append(a)
        h = activation(a, model["activation"]) if l + 1 < L else a
    o = sums[-1]
    if o.shape[1] == 1:
        o = np.concatenate([np.zeros_like(o), o], axis=1)
    return o, sums


def _best(o, skip=None):
    """Per row the index chosen by the winner rule among the columns (without column skip[row])."""
    n, k = o.shape
    win = np.full(n, -1, np.int64)
    best = np.full(n, np.nan, np.float32)
    with np.errstate(all="ignore"):
        for j in range(k):
            v = o[:, j]
            allowed = np.ones(n, bool) if skip is None else skip != j
            take = allowed & ((win < 0) | (v > best) | (np.isnan(best) & ~np.isnan(v)))
            win = np.where(take, j, win)
            best = np.where(take, v, best)
    return win, best


def decide(o, class_values, bad=None):
    """The epilogue over logits o (n, k) -> dict(labels uint8, margin, conf float32 (n,), proba float32 (k, n), win)."""
    o = np.asarray(o, np.float32)
    cv = np.asarray(class_values, np.uint8)
    win, best = _best(o)
    _, second = _best(o, skip=win)
    with np.errstate(all="ignore"):
        margin = (best - second).astype(np.float32)
        d = o.astype(np.float64) - best.astype(np.float64)[:, None]
        ex = svm_exp(d)
        s = np.zeros(o.shape[0], np.float64)
        for j in range(o.shape[1]):
            s = s + ex[:, j]
        conf = (1.0 / s).astype(np.float32)
        proba = (ex / s[:, None]).astype(np.float32).T
    labels = cv[win]
    if bad is not None:
        nan = np.float32(np.nan)
        labels = np.where(bad, 0, labels).astype(np.uint8)
        margin = np.where(bad, nan, margin).astype(np.float32)
        conf = np.where(bad, nan, conf).astype(np.float32)
        proba = np.where(bad[None, :], nan, proba).astype(np.float32)
    return dict(labels=labels, margin=margin, conf=conf, proba=np.ascontiguousarray(proba), win=win)


def classify(X, model, reverse=False):
    """dict(labels, margin, conf, proba, win, o (n, k), sums (per layer), bad) of the rows of X (n, F)."""
    z, bad = scaled(X, model)
    o, sums = forward(z, model, reverse)
    return dict(decide(o, model["class_values"], bad), o=o, sums=sums, bad=bad)

"""Restatement of K1 (csrc/k1_select.hip) in NumPy, for the sweep of tests/select_cases.py: what a call must return
(np.sort), and which of the kernel's paths it takes — the route (one small-integer pass or three radix passes), the
number of `k1_hist` launches, the live prefixes of every pass-2 launch and which of the three loops of the kernel
execute.  No GPU, no product code: only the constants below are shared with the kernel, and
tests/test_select_cases_host.py checks them against the source text.

Zero signs: np.sort does not order -0.0 against +0.0 (they compare equal, so either may stand at a rank), while the
kernel folds -0.0 onto +0.0 and returns +0.0.  Values are therefore compared with np.array_equal(..., equal_nan=True),
which treats the two zeros as equal, never through their bytes.
"""
import numpy as np

SEL_BINS = 2048          # small-integer route: every non-NaN value is an integer in [0, SEL_BINS)
SEL_BATCH = 8            # live prefixes per pass-1 / pass-2 launch
SEL_THREADS = 1024       # lanes per workgroup of k1_hist
SEL_UNR = 4              # 16-byte loads in flight per lane in the batched loop
SEL_GRID = 512           # workgroup cap of k1_hist unless RSSEG_K1_GRID names another
MAX_RANKS = 16           # RSSEG_MAX_RANKS
U8_GRID = 2048           # workgroup cap of k1_hist_u8
U8_THREADS = 1024


def f32_key(a):
    """(key, is_nan) of a float32 array: the monotone uint32 key of k1_select.hip's f32_key.  -0.0 has the key of +0.0;
    the key of a NaN means nothing and is_nan says so."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).copy()
    is_nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32), is_nan


def expected(a, ranks):
    """(np.sort(a)[ranks] as float32, number of NaNs).  np.sort puts NaN of any sign or payload last.  uint8 planes (tens
    of MB) are counted, not sorted."""
    a = np.asarray(a).reshape(-1)
    ranks = np.asarray(ranks, dtype=np.int64)
    if a.dtype == np.uint8:
        step = 1 << 23      # np.bincount widens its input to intp: block by block, not 800 MB at once
        cum = sum(np.bincount(a[i:i + step], minlength=256) for i in range(0, max(a.size, 1), step)).cumsum()
        return np.searchsorted(cum, ranks, side="right").astype(np.float32), 0
    assert a.dtype == np.float32
    return np.sort(a)[ranks], int(np.isnan(a).sum())


def small_int_plane(a):
    """Whether the one-pass route applies to this plane: every non-NaN value an integer in [0, 2048); -0.0 counts as 0."""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    v = a[~np.isnan(a)]
    return bool(np.all((v >= 0) & (v < SEL_BINS) & (np.trunc(v) == v)))


def live_prefixes(a, ranks):
    """(p1, p2): the 11-bit (key >> 21) and 22-bit (key >> 10) prefixes the host keeps alive after pass 0 / pass 1, in
    the order the host lists them: first appearance in rank order, non-NaN ranks only."""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    n_valid = a.size - int(np.isnan(a).sum())
    s = np.sort(a)
    live = [int(r) for r in ranks if r < n_valid]
    key, _ = f32_key(s[live]) if live else (np.zeros(0, np.uint32), None)
    p1, p2 = [], []
    for k in key:
        k = int(k)
        if k >> 21 not in p1:
            p1.append(k >> 21)
        if k >> 10 not in p2:
            p2.append(k >> 10)
    return p1, p2


def ndp(a, ranks):
    """(ndp1, ndp2): how many tables pass 1 and pass 2 keep for this plane; both 0 when every rank is a NaN rank."""
    p1, p2 = live_prefixes(a, ranks)
    return len(p1), len(p2)


def pass2_batches(a, ranks):
    """One (nprefix, n1, p1s) per pass-2 launch: its live 22-bit prefixes, the distinct 11-bit prefixes among them (the
    tab1 slots, each with its own tab2 plane) and those 11-bit prefixes."""
    _, p2 = live_prefixes(a, ranks)
    out = []
    for b0 in range(0, len(p2), SEL_BATCH):
        batch = p2[b0:b0 + SEL_BATCH]
        p1s = sorted({p >> 11 for p in batch})
        out.append((len(batch), len(p1s), tuple(p1s)))
    return out


def _ceil_div(a, b):
    return -(-a // b)


def predicted_launches(planes, ranks):
    """`select` launches of ONE order_stats_multi call over float32 `planes` (ranks: one list per plane): one per plane
    for the small-integer pass; unless every plane of the group is a small-integer plane, also one per plane for pass 0
    and ceil(ndp / 8) per plane for pass 1 and for pass 2."""
    total = len(planes)
    if all(small_int_plane(p) for p in planes):
        return total
    for p, r in zip(planes, ranks):
        n1, n2 = ndp(p, r)
        total += 1 + _ceil_div(n1, SEL_BATCH) + _ceil_div(n2, SEL_BATCH)
    return total


def grid_of(n, cap=None):
    """Workgroups of a k1_hist launch over n floats."""
    return min(SEL_GRID if cap is None else cap, max(1, _ceil_div(n >> 2, SEL_THREADS)))


def loop_positions(n, cap=None):
    """Which loop of k1_hist reads each float4 of an n-float plane: (batched, tail) boolean arrays over the n >> 2 whole
    float4, restated lane by lane from the kernel's two `for` statements (without the early stop of the small-integer
    pass).  Every float4 is read by exactly one of them."""
    n4 = n >> 2
    S = grid_of(n, cap) * SEL_THREADS
    batched = np.zeros(n4, dtype=bool)
    tail = np.zeros(n4, dtype=bool)
    i = np.arange(S, dtype=np.int64)
    while True:
        go = i + (SEL_UNR - 1) * S < n4
        if not go.any():
            break
        for u in range(SEL_UNR):
            batched[i[go] + u * S] = True
        i = np.where(go, i + SEL_UNR * S, i)
    while True:
        go = i < n4
        if not go.any():
            break
        assert not (batched[i[go]] | tail[i[go]]).any()
        tail[i[go]] = True
        i = np.where(go, i + S, i)
    assert np.all(batched ^ tail)
    return batched, tail


def loops(n, cap=None):
    """(batched loop executes, one-load tail loop executes, scalar tail executes) for a plane of n floats."""
    b, t = loop_positions(n, cap)
    return bool(b.any()), bool(t.any()), (n & 3) != 0


def u8_loops(n):
    """k1_hist_u8 over n bytes: (lanes that make two iterations of the two-load loop, lanes that make one iteration and
    then enter the tail loop, lanes that never enter the two-load loop)."""
    n16 = n >> 4
    S = min(U8_GRID, max(1, _ceil_div(n16, U8_THREADS))) * U8_THREADS
    i = np.arange(S, dtype=np.int64)
    iters = np.zeros(S, dtype=np.int64)
    while True:
        go = i + S < n16
        if not go.any():
            break
        iters += go
        i = np.where(go, i + 2 * S, i)
    tail = i < n16
    return int((iters == 2).sum()), int(((iters == 1) & tail).sum()), int((iters == 0).sum())

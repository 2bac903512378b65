"""K6-K8 (LDS stencils of csrc/k5_window.hip) and K13 (csrc/k13_texture.hip) against oracle/ref_np.py across tile seams,
load / store paths, launch shapes and grid rounds.

The shape list is derived from the kernel's own #define lines, so the sweep follows the tile if it ever changes; a CPU
test checks that the list covers every geometry class and that the inputs put their extrema where the docstrings say.
Every comparison is bit for bit (np.array_equal on the raw planes); entropies within the bar DESIGN.md section 4 sets for
K13 (atol 1e-12, rtol 0).  A mismatch is reported with shape, operator, the first differing (row, column) and whether it
lies on a tile seam.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K5_SOURCE = os.path.join(ROOT, "rs-image-segmentation_amd", "csrc", "k5_window.hip")


# ------------------------------------------------------------------------------------------------ geometry
def kernel_constants(path=K5_SOURCE):
    with open(path) as f:
        text = f.read()
    out = {}
    for name in ("TW", "TH", "CPT", "RPT", "TPAD", "WIN_MAXP"):
        m = re.search(r"^#define[ \t]+%s[ \t]+(\d+)\b" % name, text, re.M)
        if m is None:
            raise RuntimeError(f"{path}: no '#define {name} <integer>' line — the geometry sweep cannot follow the kernel")
        out[name] = int(m.group(1))
    return out


KC = kernel_constants()
TW, TH, CPT, RPT, TPAD, WIN_MAXP = (KC[n] for n in ("TW", "TH", "CPT", "RPT", "TPAD", "WIN_MAXP"))


def tile_map(nrows, W):
    """stencil_launch of k5_window.hip: (tile columns, tiles, tiles per XCD); the launch has 8 * chunk blocks."""
    ntx = (W + TW - 1) // TW
    nt = ntx * ((nrows + TH - 1) // TH)
    return ntx, nt, (nt + 7) // 8


W_CLASSES = {"TW-1": TW - 1, "TW": TW, "TW+1": TW + 1, "TW+3": TW + 3, "TW+4": TW + 4, "2TW-1": 2 * TW - 1, "2TW": 2 * TW,
             "2TW+1": 2 * TW + 1, "4TW+3": 4 * TW + 3, "8TW+1": 8 * TW + 1}
H_CLASSES = {"1": 1, "RPT-1": RPT - 1, "RPT": RPT, "RPT+1": RPT + 1, "TH-1": TH - 1, "TH": TH, "TH+1": TH + 1, "2TH+1": 2 * TH + 1,
             "3TH+4": 3 * TH + 4, "8TH+1": 8 * TH + 1}
LAST_COLUMN_WIDTHS = (1, 3, 4, TW - 1, TW)

# (H, W).  With TW = 256, TH = 32, RPT = 8, CPT = 4: (1,1) (7,1) (1,300) (33,255) (32,256) (33,257) (7,258) (31,259) (65,260)
# (40,511) (64,512) (65,513) (100,513) (100,1027) (9,2049) (8,2048) (256,4) (257,257) (130,516)
SHAPES = [
    (1, 1), (RPT - 1, 1), (1, TW + 44),
    (TH + 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (RPT - 1, TW + 2), (TH - 1, TW + 3), (2 * TH + 1, TW + 4),
    (TH + RPT, 2 * TW - 1), (2 * TH, 2 * TW), (2 * TH + 1, 2 * TW + 1), (3 * TH + 4, 2 * TW + 1), (3 * TH + 4, 4 * TW + 3),
    (RPT + 1, 8 * TW + 1), (RPT, 8 * TW), (8 * TH, CPT), (8 * TH + 1, TW + 1), (4 * TH + 2, 2 * TW + 4),
]


def classify(H, W):
    ntx, nt, chunk = tile_map(H, W)
    cls = set()
    cls.update("W=" + n for n, v in W_CLASSES.items() if v == W)
    cls.update("H=" + n for n, v in H_CLASSES.items() if v == H)
    if ntx > 1:
        cls.add("last tile column %d wide" % (W - (ntx - 1) * TW))
        cls.add("W%%4=%d beyond one tile" % (W % 4))
    if nt == 1:
        cls.add("nt=1")
    elif nt < 8:
        cls.add("nt<8")
    elif nt in (8, 9, 12, 20):
        cls.add("nt=%d" % nt)
    elif nt in (15, 18):
        cls.add("nt=15|18")
    if nt > 8 and nt % 8:
        cls.add("idle blocks inside the chunked map")
    if nt == ntx and nt >= 8:
        cls.add(">=8 tiles in one row")
    if ntx == 1 and nt >= 8:
        cls.add(">=8 tiles in one column")
    return cls


REQUIRED_CLASSES = (["W=" + n for n in W_CLASSES] + ["H=" + n for n in H_CLASSES]
                    + ["last tile column %d wide" % w for w in LAST_COLUMN_WIDTHS]
                    + ["W%%4=%d beyond one tile" % r for r in range(4)]
                    + ["nt=1", "nt<8", "nt=8", "nt=9", "nt=12", "nt=15|18", "nt=20", "idle blocks inside the chunked map",
                       ">=8 tiles in one row", ">=8 tiles in one column"])

BORDERS = (("reflect", 0), ("reflect101", 1))                      # oracle name, rsseg border code
MORPH_OPS = (("erosion", 0), ("dilation", 1), ("opening", 2), ("closing", 3), ("gradient", 4))
INSTANTIATIONS = ([("box", k, b, sq) for k in (3, 5, 7, 9) for b in BORDERS for sq in (False, True)]
                  + [("std", k) for k in (3, 5, 7)] + [("var", k) for k in (3, 5, 7)]
                  + [("morph", k, op) for k in (3, 5, 7) for op in MORPH_OPS] + [("sobel",), ("laplacian",)])
FLOAT_KINDS = ("box", "std", "var")


def spans_seam(H, W):
    return H > TH or W > TW


# ------------------------------------------------------------------------------------------------ inputs
def _seed(H, W, salt):
    return [H, W, salt]


def float_plane(H, W, salt=0):
    """Bounded away from zero (a pad cell left at 0 shows in every sum it wrongly enters); a constant block straddles the
    seam at column TW and row TH (variance exactly 0 inside)."""
    x = (0.5 + 0.5 * np.random.default_rng(_seed(H, W, salt)).random((H, W))).astype(np.float32)
    x[TH - 6:TH + 6, TW - 8:TW + 8] = np.float32(0.75)
    return x


def nonfinite_plane(H, W):
    """float_plane with a NaN and a +inf next to the column seam and next to the row seam."""
    x = float_plane(H, W, salt=1)
    if W > TW:
        x[min(2, H - 1), TW - 1] = np.nan
        x[min(12, H - 1), TW] = np.inf
    if H > TH:
        x[TH, min(3, W - 1)] = np.nan
        x[TH - 1, min(40, W - 1)] = np.inf
    return x


def u8_plane(H, W, lo, salt=0):
    """lo = 128: a zero pad cell wins every minimum it wrongly enters; lo = 0: full range.  Constant block on the seams:
    exact ties in the morphology."""
    q = np.random.default_rng(_seed(H, W, 100 + lo + salt)).integers(lo, 256, (H, W)).astype(np.uint8)
    q[TH - 6:TH + 6, TW - 8:TW + 8] = 200
    return q


def _flat_base(H, W, salt):
    q = np.random.default_rng(_seed(H, W, 300 + salt)).integers(128, 141, (H, W)).astype(np.uint8)
    q[TH - 6:TH + 6, TW - 8:TW + 8] = 135
    return q


def _clip(v, lo, hi):
    return max(lo, min(hi, v))


def sobel_extreme_plane(H, W, variant):
    """A low-contrast plane in [128, 140] with ONE place where the Sobel magnitude reaches 4 * 127 / 255, the largest a
    plane in [128, 255] can give: 'a' in column W - 1 (needs H >= 3), 'b' in row H - 1 (needs W >= 3), 'c' in the interior
    (needs H >= 3).  Returns (plane, target or None)."""
    q = _flat_base(H, W, ord(variant))
    if variant == "b":
        if W < 3:
            return q, None
        r, c = H - 1, _clip(W // 2, 1, W - 2)
        q[max(r - 1, 0):r + 1, c + 1] = 255
        q[max(r - 1, 0):r + 1, c - 1] = 128
        return q, (r, c)
    if H < 3:
        return q, None
    r = _clip(H // 2, 1, H - 2)
    c = W - 1 if variant == "a" else _clip(W // 2 + 1, 0, W - 1)
    q[r + 1, max(c - 1, 0):c + 2] = 255
    q[r - 1, max(c - 1, 0):c + 2] = 128
    return q, (r, c)


def laplacian_extreme_plane(H, W, variant):
    """The same base with one 255 pixel: the Laplacian's minimum, alone, at that pixel — 'a' column W - 1, 'b' row H - 1,
    'c' interior."""
    q = _flat_base(H, W, 7 + ord(variant))
    r, c = {"a": (H // 2, W - 1), "b": (H - 1, W // 2), "c": (H // 2, W // 2)}[variant]
    q[r, c] = 255
    return q, ((r, c) if H * W > 1 else None)


def normalise_sobel(mag, ref):
    """filter_rows, KIND 0: value / (max + 1e-10) in float32, the maximum taken over `ref`."""
    return mag / (np.float32(ref.max()) + np.float32(1e-10))


def normalise_laplacian(lap, ref):
    """filter_rows, KIND 1: (value - min) / (max - min + 1e-10), float32 throughout, extrema over `ref`."""
    mn, mx = np.float32(ref.min()), np.float32(ref.max())
    return ((lap - mn) / np.float32(np.float32(mx - mn) + np.float32(1e-10))).astype(np.float32)


def expected(O, inst, x=None, q=None):
    kind = inst[0]
    if kind == "box":
        _, k, (name, _code), sq = inst
        return O.box_mean(x * x if sq else x, k, name)
    if kind in ("std", "var"):
        k = inst[1]
        mean = O.box_mean(x, k, "reflect101")
        var = O.box_mean(x * x, k, "reflect101") - mean * mean
        var[var < 0] = 0
        return np.sqrt(var) if kind == "std" else var
    if kind == "morph":
        _, k, (name, _code) = inst
        return O.morph_u8(q, k, name)
    if kind == "sobel":
        mag = O.sobel_mag_u8(q)
        return normalise_sobel(mag, mag)
    if kind == "laplacian":
        lap = O.laplacian_u8(q)
        return normalise_laplacian(lap, lap)
    raise ValueError(inst)


def label(inst):
    kind = inst[0]
    if kind == "box":
        return "box k=%d %s%s" % (inst[1], inst[2][0], " square" if inst[3] else "")
    if kind == "morph":
        return "morph k=%d %s" % (inst[1], inst[2][0])
    return kind if len(inst) == 1 else "%s k=%d" % inst


def first_difference(got, want, equal_nan=False):
    """None if equal, else a sentence naming the first differing pixel and whether it lies on a tile seam."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s against %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    ne = got != want
    if equal_nan:
        ne &= ~(np.isnan(got) & np.isnan(want))
    if not ne.any():
        return None
    r, c = (int(v) for v in np.argwhere(ne)[0])
    seam = []
    if c % TW in (0, TW - 1) and got.shape[1] > TW:
        seam.append("column seam")
    if r % TH in (0, TH - 1) and got.shape[0] > TH:
        seam.append("row seam")
    return "%d differing, first at (row %d, column %d) [%s]: got %r, want %r" % (int(ne.sum()), r, c, " + ".join(seam) or "no seam",
                                                                                 got[r, c], want[r, c])


# ------------------------------------------------------------------------------------------------ CPU: the list covers the classes
def test_shape_list_covers_every_geometry_class():
    assert 15 <= len(SHAPES) <= 20 and len(set(SHAPES)) == len(SHAPES)
    table = {s: classify(*s) for s in SHAPES}
    print("\n(H, W)        ntx   nt  grid.x  classes")
    for (H, W), cls in table.items():
        ntx, nt, chunk = tile_map(H, W)
        print("%-13s %3d %4d %7d  %s" % ((H, W), ntx, nt, 8 * chunk, ", ".join(sorted(cls))))
    cover = {c: [s for s, cls in table.items() if c in cls] for c in REQUIRED_CLASSES}
    print("\nclass -> shapes")
    for c, ss in cover.items():
        print("%-40s %s" % (c, ss))
    missing = [c for c, ss in cover.items() if not ss]
    assert not missing, missing
    # the two seam-spanning vector-path shapes of the alignment test and the rows-form shapes belong to the list
    for s in ALIGN_SHAPES + ROWS_SHAPES + [MULTI_SHAPE]:
        assert s in SHAPES, s
    for H, W in ALIGN_SHAPES:
        assert W % 4 == 0 and W > TW and H > TH
    assert MULTI_SHAPE[1] % 4 and MULTI_SHAPE[1] > TW
    assert TPAD == 9 // 2, "k = 9 no longer reads the whole register window: revisit INSTANTIATIONS"
    assert len(INSTANTIATIONS) == 16 + 3 + 3 + 15 + 2


def test_oracle_takes_every_shape_and_inputs_place_their_extrema(oracle):
    """No (shape, operator) pair has to be skipped: the oracle's functions accept every shape of the list, windows and
    Gaussians wider than the plane included; and the Sobel / Laplacian planes put the extremum where they claim."""
    for H, W in SHAPES:
        for variant in "abc":
            q, at = sobel_extreme_plane(H, W, variant)
            mag = oracle.sobel_mag_u8(q)
            assert mag.dtype == np.float32 and mag.shape == (H, W)
            if at is not None:
                rest = mag.copy()
                assert mag[at] == mag.max() > 1.9, (H, W, variant)
                if variant == "a":
                    rest[:, W - 1] = -1
                elif variant == "b":
                    rest[H - 1, :] = -1
                else:
                    rest[at] = -1
                    assert 0 < at[0] < H - 1
                assert rest.max(initial=-1) < mag.max(), (H, W, variant)
            q, at = laplacian_extreme_plane(H, W, variant)
            lap = oracle.laplacian_u8(q)
            assert lap.dtype == np.float32 and lap.shape == (H, W)
            if at is not None:
                assert lap[at] == lap.min() and int((lap == lap.min()).sum()) == 1, (H, W, variant)
    for H, W in [s for s in SHAPES if s[0] * s[1] <= 300]:
        x, q = float_plane(H, W), u8_plane(H, W, 128)
        for inst in INSTANTIATIONS:
            if inst[0] not in ("sobel", "laplacian"):
                assert expected(oracle, inst, x, q).shape == (H, W)
        assert oracle.gaussian_blur_u8(q, 31).shape == (H, W)
    x = nonfinite_plane(2 * TH + 1, TW + 4)
    assert np.isnan(x).sum() == 2 and np.isinf(x).sum() == 2


# ------------------------------------------------------------------------------------------------ GPU helpers
def dev(ctx, a, dtype=None):
    return ctx.to_device(np.ascontiguousarray(a).reshape(-1), dtype)


def host(t, shape=None):
    a = t.cpu().numpy()
    return a if shape is None else a.reshape(shape)


def run(ctx, inst, plane, H, W, rows=None, edges=3):
    """One instantiation on a device plane of H rows; the full plane, or rows [y0, y1) of it."""
    kind = inst[0]
    kw = dict(rows=rows, edges=edges)
    if kind == "box":
        return ctx.box_mean(plane, H, W, inst[1], inst[2][1], inst[3], **kw)
    if kind == "std":
        return ctx.local_std(plane, H, W, inst[1], **kw)
    if kind == "var":
        return ctx.local_var(plane, H, W, inst[1], **kw)
    if kind == "morph":
        return ctx.morph(plane, H, W, inst[1], inst[2][1], **kw)
    if kind == "sobel":
        return ctx.sobel_mag(plane, H, W, **kw)
    if kind == "laplacian":
        return ctx.laplacian_norm(plane, H, W, **kw)
    raise ValueError(inst)


def report(bad):
    return "%d mismatches\n" % len(bad) + "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------ 2. every instantiation at every shape
@pytest.mark.gpu
def test_every_instantiation_at_every_shape_vs_oracle(ctx, oracle):
    """Nothing is skipped: every (shape, instantiation) pair is compared and counted.  Morphology runs on a plane in
    [128, 255] and on a full-range one; Sobel / Laplacian on the three planes that place the extremum of the PASS 0
    reduction in the last column, the last row and the interior, and on the full-range plane."""
    bad, done = [], 0
    for H, W in SHAPES:
        x = float_plane(H, W)
        dx = dev(ctx, x)
        u8s = [("[128,255]", u8_plane(H, W, 128)), ("[0,255]", u8_plane(H, W, 0))]
        du8 = [dev(ctx, q) for _, q in u8s]
        for inst in INSTANTIATIONS:
            kind = inst[0]
            cases = []   # (input tag, got, want)
            if kind in FLOAT_KINDS:
                cases.append(("float", host(run(ctx, inst, dx, H, W), (H, W)), expected(oracle, inst, x=x)))
            elif kind == "morph":
                for (tag, q), dq in zip(u8s, du8):
                    cases.append((tag, host(run(ctx, inst, dq, H, W), (H, W)), expected(oracle, inst, q=q)))
            else:
                make = sobel_extreme_plane if kind == "sobel" else laplacian_extreme_plane
                for variant in "abc":
                    q, _at = make(H, W, variant)
                    cases.append(("extremum " + variant, host(run(ctx, inst, dev(ctx, q), H, W), (H, W)), expected(oracle, inst, q=q)))
                q = u8s[1][1]
                cases.append(("[0,255]", host(run(ctx, inst, du8[1], H, W), (H, W)), expected(oracle, inst, q=q)))
            for tag, got, want in cases:
                d = first_difference(got, want)
                if d:
                    bad.append("%dx%d %s on %s: %s" % (H, W, label(inst), tag, d))
            done += 1
    assert not bad, report(bad)
    assert done == len(SHAPES) * len(INSTANTIATIONS)


@pytest.mark.gpu
def test_nan_and_inf_next_to_the_seams(ctx, oracle):
    """The oracle's float64 sums carry a NaN / +inf to exactly the windows that contain it (inf - inf in the variance
    included); so must the kernels, across a tile seam as inside a tile."""
    shapes = [s for s in SHAPES if spans_seam(*s)]
    insts = [i for i in INSTANTIATIONS if i[0] in FLOAT_KINDS]
    bad, done = [], 0
    with np.errstate(all="ignore"):
        for H, W in shapes:
            x = nonfinite_plane(H, W)
            dx = dev(ctx, x)
            for inst in insts:
                want = expected(oracle, inst, x=x)
                assert not np.isfinite(want).all()
                d = first_difference(host(run(ctx, inst, dx, H, W), (H, W)), want, equal_nan=True)
                if d:
                    bad.append("%dx%d %s with NaN / inf: %s" % (H, W, label(inst), d))
                done += 1
    assert not bad, report(bad)
    assert done == len(shapes) * len(insts) and len(shapes) >= 12


# ------------------------------------------------------------------------------------------------ 2b. more workgroups than replica slots
WRAP_SHAPE = (8 * TH + 1, 7 * TW + 1)


def mm_replicas():
    with open(os.path.join(os.path.dirname(K5_SOURCE), "common.h")) as f:
        return int(re.search(r"^#define[ \t]+RSSEG_MM_REPL[ \t]+(\d+)\b", f.read(), re.M).group(1))


def block_of_pixel(r, c, H, W):
    """tile_of_block of k5_window.hip inverted: the workgroup that owns pixel (r, c) of an H x W launch."""
    ntx, _nt, chunk = tile_map(H, W)
    t = (r // TH) * ntx + c // TW
    return (t % chunk) * 8 + t // chunk


def wrap_planes(H, W):
    """Flat planes (128) whose extrema come from the two last workgroups of the launch, a weaker copy of each feature in
    tile 0.  The last tile of this shape is the single corner pixel, where reflect-101 makes the Sobel magnitude 0 whatever
    the plane holds: it can carry the Laplacian's minimum (a 255 pixel) but not the Sobel maximum, which therefore lies,
    with the Laplacian's maximum (a 0 pixel), in the last full tile — the tile of the last workgroup but one."""
    ntx, nt, chunk = tile_map(H, W)
    r, c = (H - 2) // TH * TH + TH // 2, (ntx - 2) * TW + TW // 2       # centre of tile nt - ntx - 2
    sob = np.full((H, W), 128, np.uint8)
    sob[r + 1, c - 1:c + 2] = 255
    sob[TH // 2 + 1, TW // 2 - 1:TW // 2 + 2] = 200
    lap = np.full((H, W), 128, np.uint8)
    lap[H - 1, W - 1] = 255
    lap[r, c] = 0
    lap[TH // 2, TW // 2] = 200
    lap[TH // 2, TW // 2 + 12] = 60
    return sob, lap


@pytest.mark.gpu
def test_extrema_committed_by_workgroups_beyond_the_replica_slots(ctx, oracle):
    """PASS 0 of k8_filter commits to replica slot blockIdx.x % RSSEG_MM_REPL: with more workgroups than slots the last ones
    share a slot with the first.  Here the extrema are produced ONLY by such workgroups (checked on the CPU first), so a lost
    or misrouted commit normalises the whole plane with the weaker extrema of tile 0."""
    H, W = WRAP_SHAPE
    repl = mm_replicas()
    ntx, nt, chunk = tile_map(H, W)
    assert nt == 8 * chunk == 72 > repl and block_of_pixel(H - 1, W - 1, H, W) == nt - 1
    sob, lap = wrap_planes(H, W)
    mag, l = oracle.sobel_mag_u8(sob), oracle.laplacian_u8(lap)
    assert mag[H - 1, W - 1] == 0                      # why the Sobel maximum cannot sit in the last tile
    owners = {}
    for name, plane, where in (("sobel max", mag, mag == mag.max()), ("laplacian min", l, l == l.min()), ("laplacian max", l, l == l.max())):
        owners[name] = {block_of_pixel(int(r), int(c), H, W) for r, c in np.argwhere(where)}
        assert min(owners[name]) >= repl, (name, owners[name])
    assert owners["laplacian min"] == {nt - 1} and owners["sobel max"] == owners["laplacian max"] == {nt - 2}
    first = np.zeros((H, W), bool)
    first[:TH, :TW] = True                             # tile 0: weaker, but not flat
    assert 0 < mag[first].max() < mag.max() and l.min() < l[first].min() < 0 < l[first].max() < l.max()
    bad = []
    for inst, q in ((("sobel",), sob), (("laplacian",), lap)):
        d = first_difference(host(run(ctx, inst, dev(ctx, q), H, W), (H, W)), expected(oracle, inst, q=q))
        if d:
            bad.append("%dx%d %s: %s" % (H, W, label(inst), d))
    assert not bad, report(bad)


# ------------------------------------------------------------------------------------------------ 3. alignment branches
ALIGN_SHAPES = [(2 * TH + 1, TW + 4), (2 * TH, 2 * TW)]
GUARD = 8
F32_SENTINEL, U8_SENTINEL = np.float32(-12345.5), np.uint8(0xA5)


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _pp(t):
    arr = (C.c_void_p * 1)()
    arr[0] = t.data_ptr()
    return arr


def _abi_call(ctx, inst, din, dout, H, W):
    lib, h, kind = ctx.lib, ctx.h, inst[0]
    if kind == "box":
        return lib.rsseg_box_mean_rows_f32(h, _pp(din), 1, H, W, 0, H, 3, inst[1], inst[2][1], int(inst[3]), _pp(dout))
    if kind in ("std", "var"):
        return lib.rsseg_local_std_rows_f32(h, _vp(din), H, W, 0, H, 3, inst[1], int(kind == "var"), _vp(dout))
    if kind == "morph":
        return lib.rsseg_morph_rows_u8(h, _vp(din), H, W, 0, H, 3, inst[1], inst[2][1], _vp(dout))
    if kind == "sobel":
        return lib.rsseg_sobel_mag_rows_u8(h, _vp(din), H, W, 0, H, 3, _vp(dout))
    return lib.rsseg_laplacian_norm_rows_u8(h, _vp(din), H, W, 0, H, 3, _vp(dout))


ALIGN_INSTANTIATIONS = [("box", 9, BORDERS[0], False), ("std", 5), ("morph", 5, MORPH_OPS[0]), ("morph", 7, MORPH_OPS[2]), ("sobel",),
                        ("laplacian",)]


@pytest.mark.gpu
def test_planes_aligned_to_the_element_but_not_to_the_vector(ctx, oracle):
    """load_tile and store4 choose the 16-byte (float) / 4-byte (uint8) path from the POINTERS as well as from W % 4: planes
    that start 1, 2, 3 elements into an allocation take the scalar loads and / or stores at a width that otherwise takes
    the vector ones.  Same values; nothing written outside the plane."""
    bad, done = [], 0
    for H, W in ALIGN_SHAPES:
        n = H * W
        x, q = float_plane(H, W), u8_plane(H, W, 128)
        for inst in ALIGN_INSTANTIATIONS:
            f_in = inst[0] in FLOAT_KINDS
            src = (x if f_in else q).reshape(-1)
            want = expected(oracle, inst, x=x, q=q)
            out_dtype, sentinel = (np.uint8, U8_SENTINEL) if inst[0] == "morph" else (np.float32, F32_SENTINEL)
            vec_bytes = lambda dt: 16 if dt == np.float32 else 4  # noqa: E731
            for off_in, off_out in [(0, 0)] + [(o, 0) for o in (1, 2, 3)] + [(0, o) for o in (1, 2, 3)] + [(o, o) for o in (1, 2, 3)] + [(1, 3)]:
                hin = np.zeros(n + GUARD, src.dtype)
                hin[off_in:off_in + n] = src
                bin_ = ctx.to_device(hin)
                bout = ctx.to_device(np.full(n + GUARD, sentinel, out_dtype))
                assert bin_.data_ptr() % 16 == 0 and bout.data_ptr() % 16 == 0
                vin, vout = bin_[off_in:off_in + n], bout[off_out:off_out + n]
                assert (vin.data_ptr() % vec_bytes(src.dtype) != 0) == (off_in != 0)
                assert (vout.data_ptr() % vec_bytes(out_dtype) != 0) == (off_out != 0)
                rc = _abi_call(ctx, inst, vin, vout, H, W)
                assert rc == 0, (rc, ctx.lib.rsseg_last_error(ctx.h))
                res = host(bout)
                tag = "%dx%d %s, input +%d, output +%d elements" % (H, W, label(inst), off_in, off_out)
                if not (np.all(res[:off_out] == sentinel) and np.all(res[off_out + n:] == sentinel)):
                    bad.append(tag + ": wrote outside the output plane")
                d = first_difference(res[off_out:off_out + n].reshape(H, W), want)
                if d:
                    bad.append(tag + ": " + d)
                done += 1
    assert not bad, report(bad)
    assert done == len(ALIGN_SHAPES) * len(ALIGN_INSTANTIATIONS) * 11


# ------------------------------------------------------------------------------------------------ 4. multi-plane launches
MULTI_SHAPE = (2 * TH + 1, 2 * TW + 1)


@pytest.mark.gpu
def test_box_mean_of_one_to_eight_planes_per_launch(ctx, oracle):
    H, W = MULTI_SHAPE
    planes = [float_plane(H, W, salt=10 + p) for p in range(WIN_MAXP)]
    dplanes = [dev(ctx, p) for p in planes]
    bad, done = [], 0
    for k, (name, code) in ((7, BORDERS[0]), (9, BORDERS[0]), (9, BORDERS[1])):
        want = [oracle.box_mean(p, k, name) for p in planes]
        for n in range(1, WIN_MAXP + 1):
            first = WIN_MAXP - n          # a different plane leads every launch
            outs = ctx.box_mean_multi(dplanes[first:], H, W, k, code)
            assert len(outs) == n
            for p, o in enumerate(outs):
                d = first_difference(host(o, (H, W)), want[first + p])
                if d:
                    bad.append("%d planes, k=%d %s, plane %d: %s" % (n, k, name, p, d))
                done += 1
    assert not bad, report(bad)
    assert done == 3 * WIN_MAXP * (WIN_MAXP + 1) // 2
    # one plane too many: refused, as rsseg_box_mean_rows_f32 documents
    import torch
    n = WIN_MAXP + 1
    ins = dplanes + [dplanes[0]]
    outs = [torch.empty(H * W, dtype=torch.float32, device=dplanes[0].device) for _ in range(n)]
    rc = ctx.lib.rsseg_box_mean_rows_f32(ctx.h, ctx._pp(ins), n, H, W, 0, H, 3, 7, 0, 0, ctx._pp(outs))
    assert rc == -1, rc   # RSSEG_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 5. rows forms against the oracle
ROWS_SHAPES = [(3 * TH + 4, 4 * TW + 3), (4 * TH + 2, 2 * TW + 4)]
ROWS_INSTANTIATIONS = ([("box", 7, BORDERS[0], False), ("box", 9, BORDERS[1], False), ("box", 9, BORDERS[0], True), ("std", 5)]
                       + [("morph", k, op) for k in (5, 7) for op in MORPH_OPS] + [("sobel",), ("laplacian",)])


def stripes(H):
    rng = np.random.default_rng([H, 5])
    out = [(TH + 5, TH + 6),                 # one row
           (TH, 2 * TH),                     # both boundaries on a tile row
           (RPT + 5, TH + RPT + 3),          # neither a multiple of RPT
           (0, TH - 3), (H - TH + 5, H),     # first and last stripe: image edges
           (TH + 13, 2 * TH + 7)]            # interior
    for _ in range(2):
        r0 = int(rng.integers(0, H - 1))
        out.append((r0, int(rng.integers(r0 + 1, H + 1))))
    return out


def halo_rows(inst):
    r = inst[1] // 2 if len(inst) > 1 else 1
    return 2 * r if inst[0] == "morph" and inst[2][0] in ("opening", "closing") else r


@pytest.mark.gpu
def test_rows_forms_equal_the_oracle_on_the_full_plane(ctx, oracle):
    """A stripe [r0, r1) computed from the rows [r0 - h, r1 + h) clipped to the plane, h the halo rows_check requires and
    once more than that, equals oracle(full plane)[r0:r1].  Sobel / Laplacian normalise with the extrema of the rows they
    produce (one rank), so their expectation is the un-normalised oracle normalised by the stripe's own extrema."""
    bad, done, expect_done = [], 0, 0
    for H, W in ROWS_SHAPES:
        x, q = float_plane(H, W, salt=2), u8_plane(H, W, 0, salt=2)
        full = {}
        for inst in ROWS_INSTANTIATIONS:
            if inst[0] == "sobel":
                full[inst] = oracle.sobel_mag_u8(q)
            elif inst[0] == "laplacian":
                full[inst] = oracle.laplacian_u8(q)
            else:
                full[inst] = expected(oracle, inst, x=x, q=q)
        ss = stripes(H)
        assert all(0 <= a < b <= H for a, b in ss), ss
        expect_done += len(ss) * 2 * len(ROWS_INSTANTIATIONS)
        for r0, r1 in ss:
            for extra in (0, 3):
                for inst in ROWS_INSTANTIATIONS:
                    h = halo_rows(inst) + extra
                    a, b = max(r0 - h, 0), min(r1 + h, H)
                    edges = (1 if a == 0 else 0) | (2 if b == H else 0)
                    src = (x if inst[0] in FLOAT_KINDS else q)[a:b]
                    got = host(run(ctx, inst, dev(ctx, src), b - a, W, rows=(r0 - a, r1 - a), edges=edges), (r1 - r0, W))
                    want = full[inst][r0:r1]
                    if inst[0] == "sobel":
                        want = normalise_sobel(want, want)
                    elif inst[0] == "laplacian":
                        want = normalise_laplacian(want, want)
                    d = first_difference(got, want)
                    if d:
                        bad.append("%dx%d %s rows [%d,%d) from local rows [%d,%d) edges %d: %s" % (H, W, label(inst), r0, r1, a, b, edges, d))
                    done += 1
    assert not bad, report(bad)
    assert done == expect_done and done > 0


# ------------------------------------------------------------------------------------------------ 6. K13
ENTROPY_ATOL = 1e-12
ENTROPY_GRID_PIXELS = 8192 * 256         # k13_entropy: 8192 blocks of 256 threads per round
ENTROPY_SHAPE = (2100, 2001)             # 4 202 100 pixels: three rounds


def disk_population(H, W, radius):
    """Pixels of the disk x^2 + y^2 <= radius^2 that lie inside the image, per pixel (no oracle involved)."""
    pop = np.zeros((H, W), np.int64)
    rows, cols = np.arange(H), np.arange(W)
    for dy in range(-radius, radius + 1):
        w = math.isqrt(radius * radius - dy * dy)
        row_ok = ((rows + dy >= 0) & (rows + dy < H)).astype(np.int64)
        col_cnt = np.minimum(cols + w, W - 1) - np.maximum(cols - w, 0) + 1
        pop += row_ok[:, None] * col_cnt[None, :]
    return pop


def entropy_crops(H, W):
    """Compared regions (row range, column range): the first rows, the rows around every round boundary of the grid, the
    last rows; each at the left border (wide enough to hold the boundary pixels themselves), mid-row and the right border."""
    bands = [(0, 6), (H - 6, H)]
    marks = []
    for b in range(ENTROPY_GRID_PIXELS, H * W, ENTROPY_GRID_PIXELS):
        r, c = divmod(b, W)
        marks.append((r, c))
        bands.append((max(r - 3, 0), min(r + 3, H)))
    bands = sorted(set(bands))
    merged = [bands[0]]
    for a, b in bands[1:]:
        if a <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(merged[-1][1], b))
        else:
            merged.append((a, b))
    left = max([c for _, c in marks] + [0]) + 16
    col_ranges = [(0, min(left, W)), (W // 2 - 40, W // 2 + 40), (W - 80, W)]
    return [(rb, cb) for rb in merged for cb in col_ranges], marks


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2, 3, 5, 7])
def test_rank_entropy_beyond_one_grid_round(ctx, oracle, radius):
    H, W = ENTROPY_SHAPE
    assert H * W > 2 * ENTROPY_GRID_PIXELS
    rng = np.random.default_rng([radius, 77])
    q = rng.integers(0, 256, (H, W)).astype(np.uint8)
    q[:, W // 3:W // 2] >>= 5                                   # few grey levels: repeated bins
    # constant blocks larger than any disk: one on each round boundary (the second reaches the last row), two elsewhere
    marks = entropy_crops(H, W)[1]
    blocks = [(40, 80, 300, 340), (marks[0][0] - 20, marks[0][0] + 20, marks[0][1] - 20, marks[0][1] + 20),
              (H - 40, H, marks[1][1] - 20, marks[1][1] + 20), (1500, 1540, W - 40, W)]
    for r0, r1, c0, c1 in blocks:
        q[r0:r1, c0:c1] = 91
    e = host(ctx.rank_entropy(dev(ctx, q), H, W, radius), (H, W))
    assert e.dtype == np.float64
    bad = []
    # properties that need no oracle, on the whole plane
    pop = disk_population(H, W, radius)
    assert pop.max() == int(oracle.disk(radius).sum()) and pop.min() >= 1
    neg = ~(e >= 0)
    if neg.any():
        bad.append("%d entropies negative or NaN, first at %s" % (int(neg.sum()), tuple(np.argwhere(neg)[0])))
    over = e > np.log2(pop) + ENTROPY_ATOL
    if over.any():
        bad.append("%d entropies above log2(population), first at %s" % (int(over.sum()), tuple(np.argwhere(over)[0])))
    for r0, r1, c0, c1 in blocks:   # a side on the image border needs no margin: the disk is clipped there
        inner = e[r0 + radius:r1 if r1 == H else r1 - radius, c0 + radius:c1 if c1 == W else c1 - radius]
        assert inner.size >= 26 * 26
        if not (inner == 0).all():
            bad.append("entropy not 0 inside the constant block rows [%d,%d) columns [%d,%d)" % (r0, r1, c0, c1))
    # crops against the oracle: a margin of `radius` on artificial crop sides, true image borders kept
    crops, marks = entropy_crops(H, W)
    assert len(marks) == 2 and len(crops) >= 9
    compared, seen_marks = 0, set()
    for (ra, rb), (ca, cb) in crops:
        a, b, c0, c1 = max(ra - radius, 0), min(rb + radius, H), max(ca - radius, 0), min(cb + radius, W)
        want = oracle.rank_entropy(q[a:b, c0:c1], radius)[ra - a:rb - a, ca - c0:cb - c0]
        got = e[ra:rb, ca:cb]
        ne = ~np.isclose(got, want, rtol=0, atol=ENTROPY_ATOL)
        if ne.any():
            r, c = (int(v) for v in np.argwhere(ne)[0])
            bad.append("crop rows [%d,%d) columns [%d,%d) against the oracle: %d differing, first at pixel index %d (row %d, column %d): got %r, want %r"
                       % (ra, rb, ca, cb, int(ne.sum()), (ra + r) * W + ca + c, ra + r, ca + c, got[r, c], want[r, c]))
        compared += got.size
        for r, c in marks:   # pixel indices boundary - 1, boundary, boundary + 1
            if ra <= r < rb and ca <= c - 1 and c + 1 < cb:
                seen_marks.add((r, c))
    assert not bad, report(bad)
    assert seen_marks == set(marks), (marks, seen_marks)
    assert 5000 <= compared <= 20000, compared


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [2, 7])
def test_rank_entropy_small_plane_in_full(ctx, oracle, radius):
    H, W = 23, 37
    q = np.random.default_rng([radius, 3]).integers(0, 256, (H, W)).astype(np.uint8)
    q[:, :12] >>= 6
    q[5:22, 18:36] = 7
    got = host(ctx.rank_entropy(dev(ctx, q), H, W, radius), (H, W))
    want = oracle.rank_entropy(q, radius)
    assert np.allclose(got, want, rtol=0, atol=ENTROPY_ATOL), float(np.abs(got - want).max())


@pytest.mark.gpu
@pytest.mark.parametrize("P,R", [(32, 3), (1, 1), (4, 1.5), (24, 3), (8, 1)])
def test_lbp_uniform_point_counts(ctx, oracle, P, R):
    H, W = 2 * TH + 1, 2 * TW + 1
    q = np.random.default_rng([P, 11]).integers(0, 256, (H, W)).astype(np.uint8)
    q[:, 100:220] >>= 4
    q[20:50, 240:300] = 128                 # ties: sample - centre >= 0 counts as set
    got = host(ctx.lbp_uniform(dev(ctx, q), H, W, P, R), (H, W))
    want = oracle.lbp_uniform(q, P, R)
    assert got.dtype == np.uint8 and want.max() <= P + 1
    d = first_difference(got.astype(np.float64), want)
    assert d is None, d


@pytest.mark.gpu
def test_gaussian_every_odd_size_to_31(ctx, oracle):
    bad, done = [], 0
    shapes = [(2 * TH + 1, 2 * TW + 1), (20, 40), (3, 2 * TW + 1)]   # the last two are smaller than the widest kernels
    planes = [np.random.default_rng([H, W, 13]).integers(0, 256, (H, W)).astype(np.uint8) for H, W in shapes]
    dplanes = [dev(ctx, q) for q in planes]
    sizes = list(range(1, 32, 2))
    for ksize in sizes:
        taps = (C.c_int * ksize)()
        assert ctx.lib.rsseg_host_gaussian_kernel_fixed(ksize, taps) == 0
        want_taps = oracle.gaussian_taps_fixed(ksize)
        assert list(taps) == [int(t) for t in want_taps] and sum(taps) == 256, (ksize, list(taps), want_taps)
        for (H, W), q, dq in zip(shapes, planes, dplanes):
            d = first_difference(host(ctx.gaussian_blur_u8(dq, H, W, ksize), (H, W)), oracle.gaussian_blur_u8(q, ksize))
            if d:
                bad.append("gaussian %d taps at %dx%d: %s" % (ksize, H, W, d))
            done += 1
    assert not bad, report(bad)
    assert done == len(sizes) * len(shapes) == 48
    for ksize in (0, 2, 33):
        assert ctx.lib.rsseg_host_gaussian_kernel_fixed(ksize, (C.c_int * 40)()) == -1

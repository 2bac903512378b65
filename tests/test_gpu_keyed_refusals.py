"""The argument checks that the keyed-table entry points share (rsseg_segment_sums, rsseg_class_moments, rsseg_segment_features,
rsseg_isodata_sweep, rsseg_segment_adjacency): every one as a row (one wrong argument, status, message) of a table, the
messages literal; one doubly-wrong call per entry point, which must name the fault that is tested first; the one sentence of
the labels outside 0 ... n_segments.  Then the two sizes at which the tile sort of K24 / K26 has an edge: one label in the
whole tile, the first and the last of the histogram."""
import ctypes as C

import numpy as np
import pytest

import isodata_ref as IR
import moments_ref as MR

pytestmark = pytest.mark.gpu

F32, U8, I32 = 0, 3, 6
INVALID, UNSUPPORTED = -1, -5
RASTERS = ((1, 1), (3, 4))


class Bed:
    """Valid arguments of the five entry points on an H x W raster with one plane; call(name, **wrong) replaces some."""

    def __init__(self, ctx, H, W):
        import torch
        self.ctx, self.H, self.W, self.n = ctx, H, W, H * W
        n = self.n
        self.nseg = min(3, n)
        self.seg = ctx.to_device((np.arange(n) % self.nseg + 1).astype(np.int32))
        self.u8 = ctx.to_device((np.arange(n) * 7 % 256).astype(np.uint8))
        self.f32 = ctx.to_device(np.linspace(-1.0, 1.0, n).astype(np.float32))
        self.lab = ctx.to_device((np.arange(n) % 2).astype(np.uint8))
        self.out = torch.zeros(4096, dtype=torch.int64, device=ctx.device)
        self.exp = (C.c_int * 1)(0)
        self.weight = (C.c_double * 1)(1.0)
        self.centers = (C.c_double * 2)(-0.5, 0.5)
        self.i64 = [C.c_int64(0) for _ in range(3)]

    def planes(self, *ptrs):
        arr = (C.c_void_p * max(1, len(ptrs)))()
        for i, p in enumerate(ptrs):
            arr[i] = p
        return arr

    def good(self, name):
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        raster = dict(d_seg=p(self.seg), H=self.H, W=self.W, n_segments=self.nseg)
        fixed = dict(d_planes=self.planes(self.f32.data_ptr()), F=1, dtype=F32, n_local=self.n)
        return {
            "segment_sums": dict(**raster, d_planes=self.planes(self.u8.data_ptr()), P=1, dtype=U8, d_mask=None, d_sums=p(self.out)),
            "segment_features": dict(**raster, d_planes=self.planes(self.u8.data_ptr()), P=1, dtype=U8, d_mask=None, flags=1, d_table=p(self.out)),
            "segment_adjacency": dict(**raster, d_mask=None, d_planes=self.planes(self.u8.data_ptr()), P=1, max_edges=64, d_edges=p(self.out),
                                      n_edges=C.byref(self.i64[0])),
            "class_moments": dict(**fixed, d_labels=p(self.lab), label_dtype=U8, n_classes=2, ignore=-1, d_mask=None, plane_exp=self.exp, Q=4,
                                  d_out=p(self.out), n_left_out=C.byref(self.i64[0])),
            "isodata_sweep": dict(**fixed, d_mask=None, plane_exp=self.exp, Q=4, weight=self.weight, k=2, centers=self.centers, d_labels=p(self.lab),
                                  d_table=p(self.out), n_changed=C.byref(self.i64[1]), n_left_out=C.byref(self.i64[2])),
        }[name]

    def call(self, name, **wrong):
        args = self.good(name)
        assert set(wrong) <= set(args), (name, wrong)
        args.update(wrong)
        rc = getattr(self.ctx.lib, "rsseg_" + name)(self.ctx.h, *args.values())
        return rc, self.ctx.lib.rsseg_last_error(self.ctx.h).decode() if rc else ""


def raster_rows(b, name, max_text):
    """the checks of the segment raster; max_text: how the entry point writes the largest n_segments it takes"""
    over = b.n + 1 if max_text is None else 2 ** 31
    top = str(b.n) if max_text is None else max_text
    return [
        (dict(H=0), INVALID, f"{name}: H = 0, W = {b.W}: both must be at least 1"),
        (dict(W=-2), INVALID, f"{name}: H = {b.H}, W = -2: both must be at least 1"),
        (dict(H=65536, W=32768), INVALID, f"{name}: 2147483648 pixels, must be 1 ... 2^31 - 1"),
        (dict(d_seg=None), INVALID, f"{name}: d_seg null or not aligned to its element"),
        (dict(d_seg=C.c_void_p(b.seg.data_ptr() + 2)), INVALID, f"{name}: d_seg null or not aligned to its element"),
        (dict(n_segments=-1), INVALID, f"{name}: n_segments = -1 is not in 0 ... {top}"),
        (dict(n_segments=over), INVALID, f"{name}: n_segments = {over} is not in 0 ... {top}"),
    ]


def plane_rows(b, name, floats=True):
    """the checks of a list of at most 16 planes"""
    rows = [
        (dict(P=-1), INVALID, f"{name}: P = -1 planes, must be 0 ... 16"),
        (dict(P=17), UNSUPPORTED, f"{name}: P = 17 planes, must be 0 ... 16"),
        (dict(d_planes=None), INVALID, f"{name}: d_planes is null"),
    ]
    if floats:
        elem = f"{name}: d_planes[0] null or not aligned to its element"
        rows += [
            (dict(dtype=99), INVALID, f"{name}: dtype must be RSSEG_U8 or RSSEG_F32"),
            (dict(d_planes=b.planes(None)), INVALID, elem),
            (dict(d_planes=b.planes(b.f32.data_ptr() + 1), dtype=F32), INVALID, elem),
            (dict(d_planes=b.planes(b.u8.data_ptr(), None), P=2), INVALID, f"{name}: d_planes[1] null or not aligned to its element"),
        ]
    else:
        rows += [(dict(d_planes=b.planes(None)), INVALID, f"{name}: d_planes[0] is null"),
                 (dict(d_planes=b.planes(b.u8.data_ptr(), None), P=2), INVALID, f"{name}: d_planes[1] is null")]
    return rows


def fixed_rows(b, name):
    """the checks of the feature planes and of the fixed point of K24 / K26"""
    elem = f"{name}: d_planes[0] null or not aligned to its element"
    return [
        (dict(d_planes=None), INVALID, f"{name}: d_planes is empty (F=1)"),
        (dict(F=0), INVALID, f"{name}: d_planes is empty (F=0)"),
        (dict(F=65), UNSUPPORTED, f"{name}: F=65 feature planes, the kernel takes at most 64"),
        (dict(dtype=99), INVALID, f"{name}: dtype must be RSSEG_F32 or RSSEG_U8"),
        (dict(Q=-1), INVALID, f"{name}: Q=-1, must be 0 ... 50"),
        (dict(Q=51), INVALID, f"{name}: Q=51, must be 0 ... 50"),
        (dict(n_local=2 ** 61, Q=1), INVALID, f"{name}: n_local={2 ** 61} times 2^Q (Q=1) reaches 2^62"),
        (dict(n_local=2 ** 12, Q=50), INVALID, f"{name}: n_local=4096 times 2^Q (Q=50) reaches 2^62"),
        (dict(dtype=U8, d_planes=b.planes(b.u8.data_ptr()), Q=0), INVALID, f"{name}: RSSEG_U8 planes take plane_exp = NULL and Q = 0"),
        (dict(dtype=U8, d_planes=b.planes(b.u8.data_ptr()), plane_exp=None, Q=1), INVALID, f"{name}: RSSEG_U8 planes take plane_exp = NULL and Q = 0"),
        (dict(plane_exp=None), INVALID, f"{name}: plane_exp is null"),
        (dict(plane_exp=(C.c_int * 1)(301)), INVALID, f"{name}: plane_exp[0]=301, must be -300 ... 300"),
        (dict(plane_exp=(C.c_int * 1)(-301)), INVALID, f"{name}: plane_exp[0]=-301, must be -300 ... 300"),
        (dict(d_planes=b.planes(None)), INVALID, elem),
        (dict(d_planes=b.planes(b.f32.data_ptr() + 2)), INVALID, elem),
    ]


def table(b, name):
    """(wrong arguments, status, message); the last rows of an entry point are its doubly-wrong calls"""
    if name == "segment_sums":
        return raster_rows(b, name, None) + plane_rows(b, name) + [
            (dict(n_segments=-1, P=17), INVALID, f"{name}: n_segments = -1 is not in 0 ... {b.n}"),
            (dict(d_seg=None, H=65536, W=32768), INVALID, f"{name}: d_seg null or not aligned to its element"),
            (dict(P=17, dtype=99), UNSUPPORTED, f"{name}: P = 17 planes, must be 0 ... 16")]
    if name == "segment_features":
        return raster_rows(b, name, "2^31 - 1") + plane_rows(b, name) + [
            (dict(n_segments=-1, P=17), INVALID, f"{name}: n_segments = -1 is not in 0 ... 2^31 - 1"),
            (dict(d_seg=None, H=65536, W=32768), INVALID, f"{name}: 2147483648 pixels, must be 1 ... 2^31 - 1"),
            (dict(flags=2, d_planes=b.planes(None)), INVALID, f"{name}: flags = 2 holds unknown bits"),
            (dict(dtype=99, d_table=None), INVALID, f"{name}: dtype must be RSSEG_U8 or RSSEG_F32")]
    if name == "segment_adjacency":
        return raster_rows(b, name, "2^31 - 1") + plane_rows(b, name, floats=False) + [
            (dict(n_segments=-1, P=17), INVALID, f"{name}: n_segments = -1 is not in 0 ... 2^31 - 1"),
            (dict(d_seg=None, H=65536, W=32768), INVALID, f"{name}: 2147483648 pixels, must be 1 ... 2^31 - 1"),
            (dict(d_planes=b.planes(None), max_edges=-1), INVALID, f"{name}: d_planes[0] is null")]
    second = {"class_moments": "n_classes", "isodata_sweep": "k"}[name]
    many = {"class_moments": f"{name}: n_classes=257, the kernel takes at most 256", "isodata_sweep": f"{name}: k=65 clusters, the kernel takes at most 64"}[name]
    return fixed_rows(b, name) + [
        (dict(Q=51, d_planes=b.planes(None)), INVALID, f"{name}: Q=51, must be 0 ... 50"),
        (dict(plane_exp=(C.c_int * 1)(301), d_planes=b.planes(None)), INVALID, f"{name}: plane_exp[0]=301, must be -300 ... 300"),
        (dict(F=65, **{second: 0}), INVALID, f"{name}: {second}=0, must be >= 1"),
        (dict(dtype=99, **{second: 65 if second == "k" else 257}), UNSUPPORTED, many),
        (dict(n_local=-1, Q=51), INVALID, f"{name}: n_local=-1 is negative")]


NAMES = ("segment_sums", "class_moments", "segment_features", "isodata_sweep", "segment_adjacency")


@pytest.mark.parametrize("shape", RASTERS)
@pytest.mark.parametrize("name", NAMES)
def test_argument_checks(ctx, name, shape):
    b = Bed(ctx, *shape)
    assert b.call(name) == (0, "")
    rows = table(b, name)
    assert len(rows) >= 12
    for wrong, status, message in rows:
        got = b.call(name, **wrong)
        assert got == (status, message), (wrong, got)
    assert b.call(name) == (0, "")                             # the context works on after the refusals


@pytest.mark.parametrize("name", ("segment_sums", "segment_features", "segment_adjacency"))
def test_labels_outside_the_range_have_one_sentence(ctx, name):
    b = Bed(ctx, 3, 4)
    for bad in (-1, b.nseg + 1):
        seg = (np.arange(12) % b.nseg + 1).astype(np.int32)
        seg[7] = bad
        d = ctx.to_device(seg)
        got = b.call(name, d_seg=C.c_void_p(d.data_ptr()))
        assert got == (INVALID, f"{name}: d_seg holds 1 labels outside 0 ... n_segments = {b.nseg}"), got
    assert b.call(name) == (0, "")


# ---- the tile sort: every pixel of a tile under one label, the first and the last entry of the histogram ------------------
@pytest.mark.parametrize("label", (0, 100, 255))
def test_moments_tile_of_one_label(ctx, label):
    k = 256
    path, tile = ctx.class_moments_plan(1, k)
    n = tile + 1
    rng = np.random.default_rng(240 + label)
    x = rng.uniform(-1.0, 1.0, (1, n)).astype(np.float32)
    lab = np.full(n, label, np.int32)
    pe = np.zeros(1, np.int64)
    want, wleft = MR.moments_table(x, lab, k, pe, 20)
    got, left = ctx.class_moments([ctx.to_device(x[0])], ctx.to_device(lab), k, pe, 20)
    assert left == wleft == 0 and want[label, 0] == n
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("label", (0, 63))
def test_isodata_tile_of_one_label(ctx, label):
    k = 64
    path, tile = ctx.isodata_plan(1, k)
    n = tile + 1
    centers = (np.arange(k, dtype=np.float64) / k).reshape(k, 1)
    x = np.full((1, n), label / k, np.float32)                 # every pixel on centre `label`
    x[0, ::3] += np.float32(1.0 / 512)                         # ... or a quarter of the way to the next one
    pe, w = np.zeros(1, np.int64), np.ones(1)
    lab_in = np.full(n, 255, np.uint8)
    want = IR.sweep_ref(x, None, pe, 20, w, centers, lab_in)
    assert (want[0] == label).all()
    lab = ctx.to_device(lab_in)
    tab, changed, left = ctx.isodata_sweep([ctx.to_device(x[0])], lab, centers, w, pe, 20)
    assert np.array_equal(lab.cpu().numpy(), want[0]) and (changed, left) == (want[2], want[3]) == (n, 0)
    assert np.array_equal(tab.cpu().numpy(), IR.table_array(want[1]))

"""K25 without a GPU: the NumPy restatement of the object table against closed forms and hand counts, the derived feature
columns of rsseg.objects against exact rational arithmetic, the shape limit, and the refusals that need no device."""
import math
from fractions import Fraction

import numpy as np
import pytest

import objects_ref as O
import slic_ref as R


def moments(row):
    n, sy, sx, syy, sxx, syx = (int(v) for v in row[:6])
    return n * syy - sy * sy, n * sxx - sx * sx, n * syx - sy * sx


@pytest.mark.parametrize("h,w,y0,x0", [(1, 1, 0, 0), (5, 9, 3, 2), (9, 5, 0, 0), (1, 7, 4, 4), (12, 12, 1, 1), (3, 200, 2, 30)])
def test_rectangle_closed_forms(h, w, y0, x0):
    seg = np.zeros((y0 + h + 2, x0 + w + 3), np.int32)
    seg[y0:y0 + h, x0:x0 + w] = 1
    t = O.object_table_ref(seg)
    n = h * w
    assert t.shape == (2, 11) and t[1, 0] == n and t[1, 10] == 2 * (h + w)
    assert tuple(t[1, 6:10]) == (y0, y0 + h - 1, x0, x0 + w - 1)
    assert t[1, 1] * 2 == n * (2 * y0 + h - 1) and t[1, 2] * 2 == n * (2 * x0 + w - 1)
    myy, mxx, mxy = moments(t[1])
    assert 12 * myy == n * n * (h * h - 1) and 12 * mxx == n * n * (w * w - 1) and mxy == 0
    H, W = seg.shape
    assert tuple(t[0]) == (0, 0, 0, 0, 0, 0, H, -1, W, -1, 0)


def test_ring_single_pixel_and_l_shape():
    ring = np.ones((5, 5), np.int32)
    ring[2, 2] = 0
    assert O.object_table_ref(ring)[1, 10] == 24               # 20 outside, 4 around the hole
    ring[2, 2] = 2
    t = O.object_table_ref(ring)
    assert t[1, 10] == 24 and t[2, 10] == 4 and t[2, 0] == 1 and tuple(t[2, 1:6]) == (2, 2, 4, 4, 4)
    masked = np.ones((5, 5), np.uint8)
    masked[2, 2] = 0                                           # a masked pixel inside counts as a hole too
    t = O.object_table_ref(np.ones((5, 5), np.int32), mask=masked)
    assert t[1, 0] == 24 and t[1, 10] == 24
    # an L: rows 0..3 of column 0 and row 3 of columns 1..2 -> 6 pixels, counted by hand
    L = np.zeros((4, 3), np.int32)
    L[:, 0] = 1
    L[3, 1:] = 1
    v = np.array([[1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 5, 250]], np.uint8)
    t = O.object_table_ref(L, [v])
    assert tuple(t[1]) == (6, 0 + 1 + 2 + 3 + 3 + 3, 0 + 0 + 0 + 0 + 1 + 2, 0 + 1 + 4 + 9 + 9 + 9, 0 + 0 + 0 + 0 + 1 + 4, 3 * 1 + 3 * 2, 0, 3, 0, 2, 14,
                           265, 1 + 4 + 9 + 16 + 25 + 62500, 1, 250)
    bare = O.object_table_ref(L, [v], geometry=False)
    assert tuple(bare[1]) == (6, 0, 0, 0, 0, 0, 4, -1, 3, -1, 0, 265, 62555, 1, 250)


def test_shared_columns_equal_segment_sums_ref():
    shape = (45, 83)
    mask = np.ones(shape, np.uint8)
    mask[:2] = 0
    mask[20:24, 30:50] = 0
    seg, n, _, _ = R.slic_ref(R.scene(90, shape, 3, cell=6, noise=0.15), 8, 0.3, 3, 16, mask)
    rs = np.random.RandomState(261)
    planes = [rs.randint(0, 256, shape).astype(np.uint8), rs.uniform(-2047, 2047, shape).astype(np.float32),
              (rs.uniform(-1, 1, shape) * 2.0 ** -18).astype(np.float32)]
    keep = rs.rand(*shape) < 0.7
    for m in (None, keep):
        t = O.object_table_ref(seg, planes, mask=m, n_segments=n + 2)
        s = R.segment_sums_ref(seg, planes, mask=m, n_segments=n + 2)
        assert np.array_equal(t[:, :3], s[:, :3]) and np.array_equal(t[:, O.GEO::4], s[:, 3:])
        assert (t[n + 1:, 0] == 0).all() and (t[n + 1:, O.GEO + 2::4] == O.I64_MAX).all() and (t[n + 1:, O.GEO + 3::4] == O.I64_MIN).all()
    # the float terms: one rounding each, the square from the exact float64 product
    x = np.float32(1.2345678)
    assert O.sq_fixed24([x])[0] == round(Fraction(float(x)) ** 2 * 2 ** 24) and O.fixed40([x])[0] == round(Fraction(float(x)) * 2 ** 40)


def test_means_and_deviations_are_the_exact_statistics_correctly_rounded():
    from rsseg import objects as OB
    rs = np.random.RandomState(262)
    shape = (30, 41)
    seg = (rs.randint(0, 6, (5, 7)).repeat(6, 0).repeat(6, 1)[:30, :41]).astype(np.int32)    # label 0 among them; label 6 stays empty
    u8 = [rs.randint(0, 256, shape).astype(np.uint8), np.full(shape, 255, np.uint8), (rs.randint(0, 2, shape) * 255).astype(np.uint8)]
    f32 = [rs.uniform(-2047, 2047, shape).astype(np.float32), (rs.uniform(-1, 1, shape) * 2.0 ** -18).astype(np.float32)]
    planes = u8 + f32
    table = O.object_table_ref(seg, planes, n_segments=6)
    f = OB.features_from_table(table, [True] * 3 + [False] * 2, names=["a", "b", "c", "x", "y"], shape=False)
    assert f.columns[:4] == ["a_mean", "a_std", "a_min", "a_max"] and f.X.shape == (7, 20) and np.array_equal(f.area, table[:, 0])
    assert np.isnan(f.X[0]).all() and np.isnan(f.X[6]).all() and np.isfinite(f.X[1:6]).all()
    for s in range(1, 6):
        sel = seg == s
        n = int(sel.sum())
        for p, plane in enumerate(u8):                         # uint8: the population statistics of the pixels themselves
            px = [Fraction(int(v)) for v in plane[sel]]
            mean = sum(px) / n
            var = sum(v * v for v in px) / n - mean * mean
            assert f.X[s, 4 * p] == float(mean) and f.X[s, 4 * p + 1] == math.sqrt(float(var))
            assert f.X[s, 4 * p + 2] == plane[sel].min() and f.X[s, 4 * p + 3] == plane[sel].max()
        for j, plane in enumerate(f32):                        # float32: the same of the table's fixed-point terms ...
            p = 3 + j
            q = [Fraction(int(v), 2 ** 40) for v in O.fixed40(plane[sel])]
            q2 = [Fraction(int(v), 2 ** 24) for v in O.sq_fixed24(plane[sel])]
            mean = sum(q) / n
            var = max(sum(q2) / n - mean * mean, 0)
            assert f.X[s, 4 * p] == float(mean) and f.X[s, 4 * p + 1] == math.sqrt(float(var))
            # ... which is within 2^-24 of the population variance of the inputs (2^-25 per square, 2^-41 per mean term)
            px = [Fraction(float(v)) for v in plane[sel]]
            pm = sum(px) / n
            pv = sum(v * v for v in px) / n - pm * pm
            assert abs(Fraction(f.X[s, 4 * p + 1]) ** 2 - pv) <= Fraction(1, 2 ** 24) + abs(pv) * Fraction(1, 2 ** 50)
    assert (f.X[1:6, 4 * 1 + 1] == 0).all()                    # a constant plane: the variance is exactly 0


@pytest.mark.parametrize("h,w", [(1, 1), (4, 4), (3, 11), (17, 2), (1, 9)])
def test_shape_columns_of_a_rectangle(h, w):
    from rsseg import objects as OB
    y0, x0 = 2, 5
    seg = np.zeros((y0 + h + 1, x0 + w + 1), np.int32)
    seg[y0:y0 + h, x0:x0 + w] = 1
    f = OB.features_from_table(O.object_table_ref(seg), [], stats=())
    assert f.columns == list(OB.SHAPE_COLUMNS) and np.isnan(f.X[0]).all()
    n = h * w
    lo, hi = sorted((h * h - 1, w * w - 1))
    want = [n, y0 + (h - 1) / 2, x0 + (w - 1) / 2, h, w, 1.0, 2 * (h + w), 4 * math.pi * n / (2 * (h + w)) ** 2,
            math.sqrt(lo / hi) if hi else 1.0, 0.0 if w > h else (math.pi / 2 if h > w else 0.0)]
    assert np.allclose(f.X[1], want, rtol=1e-12, atol=0.0), (f.X[1], want)


def test_shape_columns_of_a_diagonal():
    from rsseg import objects as OB
    seg = np.eye(9, dtype=np.int32)                            # y = x: a line at 45 degrees, no width
    f = OB.features_from_table(O.object_table_ref(seg), [], stats=())
    x = dict(zip(f.columns, f.X[1]))
    assert x["area"] == 9 and x["perimeter"] == 36 and x["extent"] == 9 / 81 and x["axis_ratio"] == 0.0
    assert math.isclose(x["orientation"], math.pi / 4, rel_tol=1e-12) and math.isclose(x["compactness"], 4 * math.pi * 9 / 36 ** 2, rel_tol=1e-12)


def test_shape_limit_is_a_function_of_the_shape():
    from rsseg import objects as OB
    from rsseg.runtime import RssegUnsupported
    OB.check_moment_range((32768, 32768))
    OB.check_moment_range((1, 2 ** 21 - 1))
    for shape in ((65536, 65536), (1, 3_000_000), (2 ** 31 - 1, 1)):
        with pytest.raises(RssegUnsupported, match="2\\^63"):
            OB.check_moment_range(shape)


def test_refusals_that_need_no_device():
    from rsseg import objects as OB
    seg = np.ones((4, 5), np.int32)
    with pytest.raises(ValueError, match="integer labels"):
        OB.object_table(seg.astype(np.float32))
    with pytest.raises(ValueError, match=r"planes\[1\] has shape"):
        OB.object_table(seg, [np.zeros((4, 5), np.uint8), np.zeros((4, 6), np.uint8)])
    with pytest.raises(ValueError, match=r"planes\[0\] must be uint8 or float32"):
        OB.object_table(seg, [np.zeros((4, 5), np.float64)])
    with pytest.raises(ValueError, match="mask has shape"):
        OB.object_table(seg, (), mask=np.ones((5, 4), np.uint8))
    with pytest.raises(ValueError, match="method"):
        OB.classify_objects(seg, [np.zeros((4, 5), np.uint8)], seg, method="kmeans")
    with pytest.raises(ValueError, match="roi has shape"):
        OB.training_segments(seg, np.ones((5, 4), np.uint8))
    table = O.object_table_ref(seg, [np.zeros((4, 5), np.uint8)])
    with pytest.raises(ValueError, match="stats"):
        OB.features_from_table(table, [True], stats=("median",))
    with pytest.raises(ValueError, match="names"):
        OB.features_from_table(table, [True], names=["a", "b"])
    with pytest.raises(ValueError, match="table must be"):
        OB.features_from_table(table[:, :12], [True])


def test_training_segments_restated():
    seg = np.array([[1, 1, 2, 2, 3, 3, 4, 4, 0, 0]] * 2, np.int32)
    roi = np.array([[5, 9, 7, 7, 0, 0, 3, 0, 8, 8],
                    [9, 5, 7, 2, 0, 0, 0, 0, 8, 8]], np.uint8)
    idx, y = O.training_segments_ref(seg, roi)
    assert idx.tolist() == [1, 2, 4] and y.tolist() == [5, 7, 3]      # a tie goes to the smaller label; no ROI, no sample; label 0 never
    mask = np.ones(seg.shape, np.uint8)
    mask[0, 6] = 0                                                      # the only ROI pixel of segment 4 masked out
    mask[:, 2] = 0                                                      # segment 2 keeps a 7 and the 2: a tie, to the 2
    idx, y = O.training_segments_ref(seg, roi, mask=mask)
    assert idx.tolist() == [1, 2] and y.tolist() == [5, 2]
    idx, y = O.training_segments_ref(seg, np.zeros_like(roi))
    assert idx.size == 0 and y.size == 0

"""K23 without a GPU: the NumPy restatement (tests/slic_ref.py) has the properties the specification promises, so that the
yardstick the GPU tests compare against is itself checked; and the Python layer refuses bad arguments before it touches a device."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

import slic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def noisy_case(seed=5, shape=(45, 70), P=3, S=8):
    planes = R.scene(seed, shape, P, cell=6, noise=0.25)
    mask = np.ones(shape, np.uint8)
    mask[:3] = 0
    mask[20:26, 30:41] = 0
    return planes, mask, S


CASES = [dict(min_area=16, max_iter=5, masked=True), dict(min_area=16, max_iter=5, masked=False), dict(min_area=0, max_iter=3, masked=True),
         dict(min_area=10 ** 6, max_iter=2, masked=True)]


@pytest.fixture(scope="module")
def results():
    planes, mask, S = noisy_case()
    return [(c, mask if c["masked"] else None, R.slic_ref(planes, S, 0.3, c["max_iter"], c["min_area"], mask if c["masked"] else None)) for c in CASES]


def test_every_segment_is_one_connected_component(results):
    for c, mask, (lab, n, _, _) in results:
        assert n >= 1
        for s in range(1, n + 1):
            _, k = ndimage.label(lab == s, structure=R.FOUR)
            assert k == 1, (c, s, k)


def test_labels_are_consecutive_in_first_appearance_order(results):
    for c, mask, (lab, n, _, _) in results:
        flat = lab.reshape(-1)
        seen = flat[flat > 0]
        u, first = np.unique(seen, return_index=True)
        assert u.tolist() == list(range(1, n + 1)), c
        assert np.all(np.diff(first) > 0), c            # label s + 1 first appears after label s
        assert lab.dtype == np.int32


def test_masked_pixels_are_zero_and_only_they(results):
    for c, mask, (lab, n, _, _) in results:
        if mask is None:
            assert (lab > 0).all()
        else:
            assert np.array_equal(lab == 0, mask == 0), c


def test_regrowth_happens_and_small_pieces_vanish(results):
    c, mask, (lab, n, n_iter, n_regrown) = results[0]
    assert n_regrown > 0
    area = np.bincount(lab.reshape(-1))[1:]
    # what is left below min_area could not be reached from an assigned pixel: with this mask every valid pixel can be
    assert area.min() >= c["min_area"]
    # min_area larger than the image: nothing is assigned, nothing grows, every component stays
    c3, _, (lab3, n3, _, r3) = results[3]
    assert r3 == 0 and n3 >= n


def test_max_iter_zero_gives_the_grid():
    H, W, S = 23, 31, 5
    planes = R.scene(1, (H, W), 2)
    lab, n, n_iter, n_regrown = R.slic_ref(planes, S, 1.0, 0, 0)
    grid = R.grid_labels(H, W, S)
    assert n_iter == 0 and n_regrown == 0 and n == grid.max() + 1
    assert np.array_equal(lab, grid + 1)               # cell ids are already in first-appearance order


def test_exact_tie_goes_to_the_smaller_id():
    # S = 4, one row of 8 pixels, the last two masked: centres at x = 1.5 and x = 4.5, pixel 3 is 1.5 from both; constant colour
    mask = np.array([[1, 1, 1, 1, 1, 1, 0, 0]], np.uint8)
    planes = [np.full((1, 8), 77, np.uint8)]
    lab, n_iter = R.iterate(planes, 4, 1.0, 5, mask)
    assert lab.tolist() == [[0, 0, 0, 0, 1, 1, -1, -1]] and n_iter == 1


def test_fixed_point_means_match_float64_means():
    """Within 2^-40 of the mean in exact rational arithmetic (every float32 is a fraction), so that no rounding of the yardstick
    is part of the bound.  Below 2^-17 a float32 times 2^40 is no integer: those cases exercise the rounding step."""
    rs = np.random.RandomState(3)
    seg = R.slic_ref(R.scene(2, (40, 50), 2), 8, 0.5, 3, 16)[0]
    for lo, hi in ((-1.0, 1.0), (2040.0, 2047.0), (-2047.0, -2040.0), (-2.0 ** -18, 2.0 ** -18), (0.0, 2.0 ** -30)):
        x = rs.uniform(lo, hi, seg.shape).astype(np.float32)
        if max(abs(lo), abs(hi)) < 2.0 ** -17:
            assert np.any(x.astype(np.float64) * 2.0 ** 40 != np.rint(x.astype(np.float64) * 2.0 ** 40))
        got = R.segment_means_ref(seg, [x])[1:, 0]
        for s in range(1, seg.max() + 1):
            vals = [Fraction(float(v)) for v in x[seg == s]]
            want = sum(vals) / len(vals)
            assert abs(Fraction(float(got[s - 1])) - want) <= Fraction(1, 2 ** 40), (lo, hi, s)


def test_fixed_point_rounds_half_to_even():
    q = 2.0 ** -40
    x = np.array([0.5 * q, 1.5 * q, 2.5 * q, -0.5 * q, -1.5 * q, 0.75 * q, 1.25 * q, 3.0 * q, 2047.0, -2047.9998779296875], np.float32)
    assert np.array_equal(x.astype(np.float64), [0.5 * q, 1.5 * q, 2.5 * q, -0.5 * q, -1.5 * q, 0.75 * q, 1.25 * q, 3.0 * q, 2047.0, -2047.9998779296875])
    assert R.fixed40(x).tolist() == [0, 2, 2, 0, -2, 1, 1, 3, 2047 * 2 ** 40, -(2 ** 51) + 2 ** 27]


def test_majority_restatement_ties_ignore_and_voterless():
    seg = np.array([[1, 1, 2, 2, 3, 3, 0, 4]], np.int32)
    cm = np.array([[5, 3, 9, 9, 0, 0, 7, 255]], np.uint8)
    assert R.segment_majority_ref(seg, cm, ignore=0, fill=200).tolist() == [200, 3, 9, 200, 255]
    assert R.segment_majority_ref(seg, cm, ignore=-1, fill=1).tolist() == [1, 3, 9, 0, 255]


def test_header_declares_what_the_binding_declares():
    from rsseg import _lib
    hdr = open(os.path.join(ROOT, "include", "rsseg.h")).read()
    for name in ("rsseg_slic_u8", "rsseg_slic_tile", "rsseg_segment_sums", "rsseg_segment_majority_u8", "rsseg_segment_paint"):
        m = re.search(r"\b(int|void) %s\(([^;]*)\);" % name, hdr)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == m.group(2).count(",") + 1, name
        assert (res is None) == (m.group(1) == "void"), name
    lib = _lib.load()
    tw, th = C.c_int(0), C.c_int(0)
    lib.rsseg_slic_tile(C.byref(tw), C.byref(th))
    assert tw.value >= 1 and th.value >= 1


# ---- argument checks of rsseg/segment.py: every one is raised before a context is needed ------------------------------------
def test_slic_argument_errors():
    from rsseg import segment as SG
    p = np.zeros((6, 7), np.uint8)
    bad = [
        (dict(features=[p]), "step"),                                     # neither step nor n_segments
        (dict(features=[p], step=4, n_segments=3), "step"),
        (dict(features=[p], step=1), "step"),
        (dict(features=[p], step=4097), "step"),
        (dict(features=[p], step=2.5), "step"),
        (dict(features=[p], n_segments=0), "n_segments"),
        (dict(features=[p], step=4, compactness=-1.0), "compactness"),
        (dict(features=[p], step=4, compactness=float("nan")), "compactness"),
        (dict(features=[p], step=4, max_iter=-1), "max_iter"),
        (dict(features=[p], step=4, min_area=-2), "min_area"),
        (dict(features=[p], step=4, mask=np.ones((6, 6), np.uint8)), "mask"),
        (dict(features=[p, np.zeros((6, 8), np.uint8)], step=4), "features[1]"),
        (dict(features=[p] * 17, step=4), "features"),
        (dict(features=[], step=4), "features"),
        (dict(features=np.zeros((2, 2, 2, 2), np.uint8), step=4), "features"),
        (dict(features=[p], step=4, ranges=[(0, 1), (0, 1)]), "ranges"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=re.escape(word)):
            SG.slic(**kw)
    assert SG.slic_step((100, 100), 100) == 10 and SG.slic_step((3, 3), 100) == 2
    assert SG.slic_weight(10.0, 5) == 4.0


def test_reduction_argument_errors():
    from rsseg import segment as SG
    seg = np.ones((4, 5), np.int32)
    with pytest.raises(ValueError, match="segments"):
        SG.segment_means(seg.astype(np.float32), [np.zeros((4, 5), np.uint8)])
    with pytest.raises(ValueError, match="segments"):
        SG.segment_means(seg - 2, [np.zeros((4, 5), np.uint8)])
    with pytest.raises(ValueError, match=re.escape("planes[0]")):
        SG.segment_means(seg, [np.zeros((4, 6), np.uint8)])
    with pytest.raises(ValueError, match="mask"):
        SG.segment_means(seg, [np.zeros((4, 5), np.uint8)], mask=np.ones((5, 4)))
    with pytest.raises(ValueError, match="class_map"):
        SG.object_majority(seg, np.zeros((4, 6), np.uint8))
    with pytest.raises(ValueError, match="class_map"):
        SG.object_majority(seg, np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="nodata"):
        SG.object_majority(seg, np.zeros((4, 5), np.uint8), nodata=256)
    with pytest.raises(ValueError, match="fill"):
        SG.object_majority(seg, np.zeros((4, 5), np.uint8), fill=-1)
    with pytest.raises(ValueError, match="table"):
        SG.paint(seg, np.zeros(2, np.float64))
    with pytest.raises(ValueError, match="table"):
        SG.paint(seg, np.zeros((2, 2), np.uint8))


def test_command_line_options():
    from rsseg import stages
    ap = stages.build_parser()
    a = stages.parse_args(ap, ["x.tif", "out", "--classify", "kmeans", "--segment", "8", "--compactness", "5", "--segment-iterations", "3", "--object-based"])
    assert (a.segment, a.compactness, a.segment_iterations, a.object_based) == (8, 5.0, 3, True)
    for argv in (["x.tif", "out", "--segment", "8"], ["x.tif", "out", "--classify", "kmeans", "--object-based"],
                 ["x.tif", "out", "--classify", "kmeans", "--segment", "1"], ["x.tif", "out", "--classify", "kmeans", "--compactness", "3"],
                 ["x.tif", "out", "--classify", "kmeans", "--segment", "8", "--compactness", "-1"]):
        with pytest.raises(SystemExit):
            stages.parse_args(ap, argv)

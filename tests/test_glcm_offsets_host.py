"""CPU suite for the texture function's (distance, angle) entries: the offset plan (rsseg.pipeline.glcm_offset_plan)
on scikit-image's rounding cases, and the two NumPy restatements of tests/glcm_offsets_ref.py — the kernel's integer
formulation (spec) against scikit-image's published values and against the literal float64 graycomatrix / graycoprops,
and the literal form against the pinned CPU oracle for the default entries."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glcm_offsets_ref as R  # noqa: E402
from rsseg.pipeline import glcm_offset_plan  # noqa: E402

PI = math.pi
DEFAULT_ANGLES = [0, PI / 4, PI / 2, 3 * PI / 4]
# skimage/feature/tests/test_texture.py (0.18.x)
SK_IMAGE = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]], np.uint8)


def test_plan_default_entries():
    entries, distinct, index = glcm_offset_plan([1], DEFAULT_ANGLES)
    assert entries == [(0, 1), (1, 1), (1, 0), (1, -1)]
    assert distinct == entries and index == [0, 1, 2, 3]


def test_plan_rounding_cases():
    # sin(pi/6) = 0.49999999999999994 rounds to 0; d = 2 at pi/4 -> (1, 1); d = 2 at 3 pi/4 -> (1, -1); 4 rad, 6 rad
    assert math.sin(PI / 6) < 0.5
    assert glcm_offset_plan([1], [PI / 6])[0] == [(0, 1)]
    assert glcm_offset_plan([2], [PI / 4])[0] == [(1, 1)]
    assert glcm_offset_plan([2], [3 * PI / 4])[0] == [(1, -1)]
    assert glcm_offset_plan([1], [4.0])[0] == [(-1, -1)]
    assert glcm_offset_plan([1], [6.0])[0] == [(0, 1)]


def test_plan_ties_follow_python_round():
    # sin(pi/2) * 2.5 = 2.5 -> 2 (ties to even), * 3.5 -> 4, * 0.5 -> 0; cos(0) * -1.5 -> -2
    assert glcm_offset_plan([2.5, 3.5, 0.5], [PI / 2])[0] == [(2, 0), (4, 0), (0, 0)]
    assert glcm_offset_plan([-1.5], [0])[0] == [(0, -2)]


def test_plan_dedup_ten_of_twelve():
    entries, distinct, index = glcm_offset_plan([1, 2, 3], DEFAULT_ANGLES)
    assert len(entries) == 12 and len(distinct) == 10
    assert all(distinct[i] in (e, (-e[0], -e[1])) for e, i in zip(entries, index))
    # o and -o merge: angle pi maps (0, 1) to (0, -1)
    e, d, i = glcm_offset_plan([1], [0, PI])
    assert e == [(0, 1), (0, -1)] and d == [(0, 1)] and i == [0, 0]


@pytest.mark.parametrize("distances,angles", [([], [0]), ([1], []), ([float("nan")], [0]), ([1], [float("inf")]),
                                              ([1], [0, float("nan")])])
def test_plan_refuses_empty_and_nonfinite(distances, angles):
    with pytest.raises(ValueError):
        glcm_offset_plan(distances, angles)


def _spec_one(img, distances, angles, levels):
    entries, _, _ = glcm_offset_plan(distances, angles)
    return R.spec_windows(np.asarray(img, np.uint8)[None], entries)[:, 0]


def test_spec_matches_published_skimage_values():
    # float64 before the float32 cast: the per-entry values of the spec
    for dist, prop, want in [(1, 4, 0.71953255), (2, 4, 0.41176470), (1, 2, 0.80833333), (1, 3, 0.38188131)]:
        entries, _, _ = glcm_offset_plan([dist], [0])
        st = R.offset_stats(SK_IMAGE[None], *entries[0])
        got = R.entry_values(st)[prop][0]
        assert abs(got - want) < 1e-7, (dist, prop, got, want)
    # distance 10: the empty matrix
    np.testing.assert_array_equal(_spec_one(SK_IMAGE, [10], [0], 4), np.float32([0, 0, 0, 0, 1]))
    # the mean of the two entries
    got = _spec_one(SK_IMAGE, [1, 2], [0], 4)[4]
    assert abs(float(got) - (0.71953255 + 0.41176470) / 2) < 1e-7


def _random_window(rng, win, levels):
    kind = rng.integers(0, 4)
    if kind == 0:
        return np.full((win, win), rng.integers(0, levels), np.uint8)
    w = rng.integers(0, levels, (win, win))
    if kind == 1:      # 95 % constant
        w = np.where(rng.random((win, win)) < 0.95, int(rng.integers(0, levels)), w)
    elif kind == 2:    # smooth
        w = (np.add.outer(np.arange(win), np.arange(win)) * int(rng.integers(1, 5)) // 3) % levels
    return w.astype(np.uint8)


@pytest.mark.parametrize("seed", range(12))
def test_spec_matches_literal(seed):
    rng = np.random.default_rng(9100 + seed)
    levels = int(rng.choice([2, 3, 8, 32, 64, 65, 130, 256]))
    win = int(rng.integers(2, 14))
    nd, na = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    distances = [float(v) for v in rng.choice([0, 1, 2, 3, -1, -2, 1.5, 2.5, win, win + 3, 40], nd)]
    angles = [float(v) for v in rng.uniform(-7, 14, na)]
    entries, _, _ = glcm_offset_plan(distances, angles)
    for _ in range(4):
        w = _random_window(rng, win, levels)
        spec = R.spec_windows(w[None], entries)[:, 0]
        lit = R.literal_props(w, entries, levels).mean(axis=1)
        np.testing.assert_allclose(spec.astype(np.float64), lit, rtol=1e-6, atol=1e-6, err_msg=str((levels, win, distances, angles)))


def test_spec_matches_literal_large_window_many_levels():
    rng = np.random.default_rng(9200)
    entries, _, _ = glcm_offset_plan([1, 3, 5], [0, PI / 3, 2.0])
    for win, levels in [(33, 256), (40, 200), (48, 64)]:
        for kind in range(3):
            w = _random_window(np.random.default_rng(9300 + win + kind), win, levels) if kind else rng.integers(0, levels, (win, win)).astype(np.uint8)
            spec = R.spec_windows(w[None], entries)[:, 0]
            lit = R.literal_props(w, entries, levels).mean(axis=1)
            np.testing.assert_allclose(spec.astype(np.float64), lit, rtol=1e-6, atol=1e-6)


def test_literal_matches_oracle_mode0(oracle):
    rng = np.random.default_rng(9400)
    entries, _, _ = glcm_offset_plan([1], DEFAULT_ANGLES)
    for levels, win, step in [(8, 5, 2), (32, 9, 4), (64, 7, 3)]:
        q = rng.integers(0, levels, (win + 9, win + 11)).astype(np.uint8)
        q[:win, :win] = 3 % levels
        want = oracle.glcm_small_maps(q, levels, win, step, mode=0)
        lit = R.literal_maps(q, levels, win, step, entries)
        for k in R.PROPS:
            np.testing.assert_allclose(lit[k], want[k], rtol=1e-6, atol=1e-6, err_msg=k)

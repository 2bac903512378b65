"""CPU checks of the Gabor bank's host side (rsseg/gabor.py), of the restatement the GPU tests compare against
(tests/gabor_ref.py), and of the NumPy helpers of modules/features/indices.py against the reference's recorded results."""
import json
import os

import numpy as np
import pytest

import gabor_ref as R
import indices_helpers_cases as HC

PLANS = [(4, 6), (1, 1), (3, 4), (7, 2)]


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32))


@pytest.mark.parametrize("ns,no", PLANS)
def test_plan_sizes_counts_and_taps(ns, no):
    """gabor_plan: one group per scale in the reference's order, an odd size 5..15 by the reference's rule, one kernel per
    orientation; every kernel has centre tap 1.0, is point-symmetric bit for bit, and is within 1 float32 ulp of the scalar
    restatement (the two evaluate the same float64 formula with differently associated products)."""
    from rsseg.gabor import MAX_KSIZE, gabor_plan
    plan = gabor_plan(ns, no)
    params = R.bank_params(ns, no)
    norient = len(np.arange(0, np.pi, np.pi / no))
    assert len(plan) == ns and sum(len(t) for _, t in plan) == len(params) == ns * norient
    if (ns, no) == (4, 6):
        assert [k for k, _ in plan] == [5, 5, 5, 15] and [len(t) for _, t in plan] == [6, 6, 6, 6]
    if (ns, no) == (7, 2):
        assert 9 in [k for k, _ in plan]
    it = iter(params)
    for ksize, taps in plan:
        assert taps.dtype == np.float32 and taps.shape == (norient, ksize, ksize)
        assert ksize % 2 == 1 and 5 <= ksize <= MAX_KSIZE
        for k in taps:
            p = next(it)
            assert p[0] == ksize
            m = ksize // 2
            assert k[m, m] == np.float32(1.0)
            assert k.tobytes() == np.ascontiguousarray(k[::-1, ::-1]).tobytes()
            want = R.gabor_kernel_ref(*p)
            assert np.all(np.abs(k.astype(np.float64) - want.astype(np.float64)) <= np.maximum(_ulp32(k), _ulp32(want)))


def test_default_bank_keeps_subnormal_taps():
    """The scale-0.1 kernels (sigma 0.1 on a 5 x 5 grid) reach below the smallest normal float32: 4 subnormal taps each, which a
    flushing multiply would lose."""
    from rsseg.gabor import gabor_plan
    ksize, taps = gabor_plan()[0]
    tiny = np.finfo(np.float32).tiny
    for k in taps:
        assert int(((k != 0) & (np.abs(k) < tiny)).sum()) == 4


def test_num_scales_zero_is_an_empty_plan():
    from rsseg.gabor import gabor_plan
    assert gabor_plan(0, 6) == []


@pytest.mark.parametrize("ksize", [5, 9, 15])
def test_float32_restatement_within_the_rounding_bound_of_float64(ksize):
    """correlate_ref in float32 (the contract) stays within gamma_n * sum|k x| of the same sum in float64, on a seeded 37 x 41
    plane; 15 x 15 measured 1.0e-2 against a bound of 1.6e-1."""
    from rsseg.gabor import gabor_kernel
    rng = np.random.default_rng(7)
    u8 = rng.integers(0, 256, (37, 41), dtype=np.uint8)
    sigma = ksize / 5.0
    for theta in (0.0, np.pi / 6, np.pi / 2):
        k = gabor_kernel(ksize, sigma, theta, 10 * sigma, 0.5, 0)
        r32, r64 = R.correlate_ref(u8, k, np.float32), R.correlate_ref(u8, k, np.float64)
        assert r32.dtype == np.float32 and r64.dtype == np.float64
        err, bound = np.abs(r32.astype(np.float64) - r64), R.gamma_bound(u8, k)
        print(f"ksize {ksize} theta {theta:.3f}: max error {err.max():.3e}, bound there {bound.flat[err.argmax()]:.3e}")
        assert np.all(err <= bound)


def test_reflect101_repeats_on_tiny_planes():
    assert [R.reflect101(i, 3) for i in range(-7, 8)] == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert [R.reflect101(i, 1) for i in (-7, 0, 7)] == [0, 0, 0]
    assert [R.reflect101(i, 2) for i in range(-3, 4)] == [1, 0, 1, 0, 1, 0, 1]
    u8 = np.arange(6, dtype=np.uint8).reshape(2, 3)
    p = R.pad101(u8, 2)
    assert p.shape == (6, 7) and np.array_equal(p[2:4, 2:5], u8) and np.array_equal(p[0], [2, 1, 0, 1, 2, 1, 0])


def test_one_pixel_response_is_the_reflected_kernel():
    """A single 255 on zeros: the response around it is 255 * the kernel turned by 180 degrees (correlation), rounding nothing."""
    k = np.arange(1, 26, dtype=np.float32).reshape(5, 5)
    u8 = np.zeros((11, 12), np.uint8)
    u8[5, 6] = 255
    r = R.correlate_ref(u8, k, np.float32)
    assert np.array_equal(r[3:8, 4:9], 255.0 * k[::-1, ::-1]) and r.sum() == 255.0 * k.sum()


def test_normalise_ref_constant_plane_is_zero():
    n = R.normalise_ref(np.full((3, 4), 7.5, np.float32))
    assert n.dtype == np.float32 and np.array_equal(n, np.zeros((3, 4), np.float32))


def test_numpy_helpers_equal_the_reference_bit_for_bit(golden_dir):
    """feature_selection_by_variance, feature_fusion_for_segmentation, hierarchical_feature_fusion and
    semantic_merge_water_classes against tests/golden/indices_helpers.npz (the reference's own results,
    tests/make_indices_helpers_golden.py): members, order, dtypes, bytes, and the exceptions' types and texts."""
    import modules.features.indices as M
    D, seg, manifest, z = HC.load(os.path.join(golden_dir, "indices_helpers.npz"))
    before = {k: v.copy() for k, v in HC.flatten(D).items()}
    seg0 = seg.copy()
    n = 0
    for i, entry in enumerate(manifest):
        if entry["fn"] in HC.GPU_FUNCTIONS:
            continue
        HC.check(i, entry, HC.replay(M, entry, D, seg), z)
        n += 1
    assert n == 11 and {e["fn"] for e in manifest} - set(HC.GPU_FUNCTIONS) == {
        "feature_selection_by_variance", "feature_fusion_for_segmentation", "hierarchical_feature_fusion", "semantic_merge_water_classes"}
    assert all(np.array_equal(v, before[k]) for k, v in HC.flatten(D).items()) and np.array_equal(seg, seg0)   # inputs untouched


def test_mirror_defines_every_reference_function_but_the_unseeded_forest(golden_dir):
    """Every function name of the reference's indices.py (tests/golden/star_import_names.json) is defined by the mirror and
    exported by its __all__, except evaluate_feature_importance_for_classes."""
    import modules.features.indices as M
    spec = json.load(open(os.path.join(golden_dir, "star_import_names.json")))["modules.features.indices"]["signatures"]
    missing = sorted(n for n in spec if not callable(getattr(M, n, None)))
    assert missing == ["evaluate_feature_importance_for_classes"]
    assert sorted(n for n in spec if n not in M.__all__) == ["evaluate_feature_importance_for_classes"]

"""GPU suite for the texture function with any (distance, angle) entries and up to 256 grey levels
(rsseg_glcm_offsets_u8, csrc/k4_glcm_offsets.hip; rsseg_glcm_u8 for 65..256 levels): the kernel against the spec of
tests/glcm_offsets_ref.py bit for bit and against the literal graycomatrix / graycoprops within 1e-6, the default
entries at 65..256 levels against the CPU oracle, the homogeneity of large smooth windows, scikit-image's published
vectors, the mirror end to end, one plane at size, and the refusals."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glcm_offsets_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = int(os.environ.get("RSSEG_FUZZ_N", "0"))
SEED0 = int(os.environ.get("RSSEG_FUZZ_SEED0", "0"))
PI = math.pi
DEFAULT_ANGLES = [0, PI / 4, PI / 2, 3 * PI / 4]


def seeds(default):
    return list(range(SEED0, SEED0 + (N or default)))


def dev(ctx, a):
    return ctx.to_device(np.ascontiguousarray(a).reshape(-1))


def host(t, shape):
    return t.cpu().numpy().reshape(shape)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(ctx, q, levels, win, step, entries):
    H, W = q.shape
    got, (oh, ow) = ctx.glcm(dev(ctx, q), H, W, levels, win, step, offsets=entries)
    return {k: host(g, (oh, ow)) for k, g in zip(R.PROPS, got)}


def plane(rng, H, W, levels):
    base = rng.integers(0, levels, (H, W))
    smooth = (np.add.outer(int(rng.integers(1, 4)) * np.arange(H), np.arange(W)) // int(rng.integers(2, 12))) % levels
    q = np.where(rng.random((H, W)) < rng.random(), base, smooth).astype(np.uint8)
    if rng.random() < 0.3:
        q[: H // 2, : W // 2] = int(rng.integers(0, levels))
    return q


def assert_spec(got, q, levels, win, step, entries, tag, literal=False):
    want = R.spec_maps(q, levels, win, step, entries)
    for k in R.PROPS:
        assert got[k].shape == want[k].shape, (tag, k)
        bad = np.flatnonzero(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, (tag, k, bad[:5], got[k].reshape(-1)[bad[:5]], want[k].reshape(-1)[bad[:5]])
    if literal:
        lit = R.literal_maps(q, levels, win, step, entries)
        for k in R.PROPS:
            np.testing.assert_allclose(got[k], lit[k], rtol=1e-6, atol=1e-6, err_msg=str((tag, k)))


@pytest.mark.parametrize("seed", seeds(8))
def test_fuzz_glcm_offsets(ctx, seed):
    """Random levels (2..256), window (2..40), step (1..win+2), distance and angle lists: bit for bit against the spec,
    within 1e-6 of the literal formulas on a few windows."""
    from rsseg.pipeline import glcm_offset_plan
    rng = np.random.default_rng(8100 + seed)
    levels = int(rng.choice([2, 5, 16, 32, 33, 64, 65, 100, 200, 256]))
    win = int(rng.choice([2, 3, 4, 5, 7, 9, 13, 21, 33, 40]))
    step = int(rng.integers(1, win + 3))
    nd, na = int(rng.integers(1, 4)), int(rng.integers(1, 6))
    distances = [float(v) for v in rng.choice([0, 1, 1, 2, 3, 5, -1, -2, 1.5, 2.5, win, win + 7], nd)]
    angles = [float(v) for v in rng.choice([0, PI / 6, PI / 4, PI / 2, 3 * PI / 4, PI, 4.0, 6.0, -1.0, 9.5], na)]
    entries, _, _ = glcm_offset_plan(distances, angles)
    H, W = int(rng.integers(win, win + 70)), int(rng.integers(win, win + 120))
    q = plane(rng, H, W, levels)
    tag = dict(seed=seed, levels=levels, win=win, step=step, H=H, W=W, distances=distances, angles=angles)
    got = run(ctx, q, levels, win, step, entries)
    assert_spec(got, q, levels, win, step, entries, tag)
    # literal on a corner of the plane (the float64 graycomatrix is slow)
    h2, w2 = min(H, win + 2 * step), min(W, win + 2 * step)
    sub = np.ascontiguousarray(q[:h2, :w2])
    assert_spec(run(ctx, sub, levels, win, step, entries), sub, levels, win, step, entries, tag, literal=True)


@pytest.mark.parametrize("win,levels", [(64, 16), (100, 64), (180, 256), (255, 200)])
def test_glcm_offsets_large_windows(ctx, win, levels):
    from rsseg.pipeline import glcm_offset_plan
    rng = np.random.default_rng(8200 + win)
    entries, _, _ = glcm_offset_plan([1, 4, 50], [0, 1.0, PI / 2])
    q = plane(rng, win + 9, win + 13, levels)
    q[:win, :win] = 7
    assert_spec(run(ctx, q, levels, win, 3, entries), q, levels, win, 3, entries, (win, levels))


@pytest.mark.parametrize("seed", seeds(6))
def test_default_offsets_many_levels_match_oracle(ctx, oracle, seed):
    """The default entries at 65..256 levels (rsseg_glcm_u8 and the default list of rsseg_glcm_offsets_u8): oracle.c mode 1
    bit for bit while its int64 homogeneity sum cannot overflow (win <= 32), mode 0 within 1e-6 above."""
    rng = np.random.default_rng(8300 + seed)
    levels = int(rng.choice([65, 96, 128, 200, 255, 256]))
    win = int(rng.choice([2, 3, 5, 7, 11, 21, 32, 33, 40]))
    step = int(rng.integers(1, win + 3))
    H, W = int(rng.integers(win, win + 60)), int(rng.integers(win, win + 90))
    q = plane(rng, H, W, levels)
    tag = dict(seed=seed, levels=levels, win=win, step=step)
    default = [(0, 1), (1, 1), (1, 0), (1, -1)]
    a = run(ctx, q, levels, win, step, None)
    b = run(ctx, q, levels, win, step, default)
    if win <= 32:
        want = oracle.glcm_small_maps(q, levels, win, step, mode=1)
        for k in R.PROPS:
            assert np.array_equal(bits(a[k]), bits(want[k])), (tag, k)
    else:
        want = oracle.glcm_small_maps(q, levels, win, step, mode=0)
        for k in R.PROPS:
            np.testing.assert_allclose(a[k], want[k], rtol=1e-6, atol=1e-6, err_msg=str((tag, k)))
    for k in R.PROPS:
        assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k)


@pytest.mark.parametrize("win", [33, 46, 64, 255])
@pytest.mark.parametrize("levels", [32, 48])
def test_homogeneity_large_smooth_windows(ctx, oracle, win, levels):
    """The int64 sum of 2^-52 homogeneity terms overflowed from window 33 on smooth windows (negative homogeneity): the
    wave kernel (levels <= 32) and the workgroup kernel (33..64) now sum exactly."""
    rng = np.random.default_rng(8400 + win)
    H, W = win + 2, 2 * win + 1
    q = np.full((H, W), 5, np.uint8)
    noisy = rng.random((H, W)) < 0.05
    q[:, win:] = np.where(noisy[:, win:], rng.integers(0, levels, (H, W - win)), 5)   # right half: 95 % constant
    got = run(ctx, q, levels, win, 1, None)
    want = oracle.glcm_small_maps(q, levels, win, 1, mode=0)
    np.testing.assert_allclose(got["homogeneity"], want["homogeneity"], rtol=0, atol=1e-6)
    assert got["homogeneity"][0, 0] == 1.0


def test_skimage_vectors_through_gpu(ctx):
    from rsseg.pipeline import glcm_offset_plan
    img = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]], np.uint8)
    entries, _, _ = glcm_offset_plan([1, 2], [0])
    got = run(ctx, img, 4, 4, 1, entries)
    assert abs(float(got["correlation"][0, 0]) - (0.71953255 + 0.41176470) / 2) < 1e-7
    entries, _, _ = glcm_offset_plan([10], [0])
    got = run(ctx, img, 4, 4, 1, entries)
    assert [float(got[k][0, 0]) for k in R.PROPS] == [0.0, 0.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("levels,win,step", [(32, 21, 21), (64, 7, 1), (256, 21, 21), (100, 7, 1)])
def test_mirror_glcm_offsets_end_to_end(ctx, oracle, golden_dir, levels, win, step):
    from modules.features import indices as I
    from rsseg.pipeline import glcm_offset_plan
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    band = crop["bands"][3]
    H, W = band.shape
    got = I.calculate_glcm_features(band, distances=[1, 2, 3], levels=levels, window_size=win, step_size=step)
    entries, _, _ = glcm_offset_plan([1, 2, 3], DEFAULT_ANGLES)
    q = oracle.to_u8(oracle.robust_normalize(band), levels - 1)
    small = R.spec_maps(q, levels, win, step, entries)
    for k in R.PROPS:
        want = oracle.resize_bilinear(small[k], H, W)
        assert np.array_equal(bits(got[k]), bits(want)), (levels, win, step, k)
    a = I.calculate_glcm_features(band, levels=levels, window_size=win, step_size=step)
    b = I.calculate_glcm_features(band, distances=[1], angles=DEFAULT_ANGLES, levels=levels, window_size=win, step_size=step)
    for k in R.PROPS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_glcm_offsets_at_size(ctx):
    """4096^2, 7 x 7 step 1, [1, 2, 3] x 4 angles: 2000 seeded windows against the spec, bit for bit."""
    from rsseg.pipeline import glcm_offset_plan
    rng = np.random.default_rng(8500)
    H = W = 4096
    win, levels = 7, 32
    q = plane(rng, H, W, levels)
    entries, _, _ = glcm_offset_plan([1, 2, 3], DEFAULT_ANGLES)
    got = run(ctx, q, levels, win, 1, entries)
    oh, ow = H - win + 1, W - win + 1
    ys, xs = rng.integers(0, oh, 2000), rng.integers(0, ow, 2000)
    wins = np.stack([q[y:y + win, x:x + win] for y, x in zip(ys, xs)])
    want = R.spec_windows(wins, entries)
    for t, k in enumerate(R.PROPS):
        assert np.array_equal(bits(got[k][ys, xs]), bits(want[t])), k


def test_glcm_offsets_refusals(ctx):
    from modules.features import indices as I
    from rsseg.runtime import RssegUnsupported
    q = np.zeros((300, 300), np.uint8)
    with pytest.raises(RssegUnsupported, match="levels"):
        run(ctx, q, 257, 21, 21, [(0, 2)])
    with pytest.raises(RssegUnsupported, match="levels"):
        run(ctx, q, 257, 21, 21, None)
    with pytest.raises(RssegUnsupported):
        run(ctx, q, 32, 256, 10, [(0, 2), (2, 0)])
    with pytest.raises(ValueError):
        I.calculate_glcm_features(np.ones((64, 64), np.float32), angles=[0, float("nan")])
    with pytest.raises(RssegUnsupported, match="astype"):
        I.calculate_glcm_features(np.ones((64, 64), np.float64), angles=[float("nan")])

"""GPU suite of K17 (csrc/k17_correlate.hip) and of calculate_gabor_features: the raw responses against the float32
restatement of cv2.filter2D's direct path (tests/gabor_ref.py) bit for bit and against its float64 form within the rounding
bound, the extrema, the in-place normalisation, the bank on the golden crop, and prepare_features_for_segmentation against
the reference's recorded results."""
import ctypes as C
import os

import numpy as np
import pytest

import gabor_ref as R
import indices_helpers_cases as HC

pytestmark = pytest.mark.gpu

KSIZES = [1, 3, 5, 7, 9, 11, 13, 15]
NFS = [1, 6, 8]
NFS_EVERY = [1, 2, 3, 4, 5, 6, 7, 8]   # 3, 5, 7 run in a launch compiled for 4, 6, 8 kernels: zero taps and no plane beyond nf


def _tile():
    from rsseg.gabor import tile_shape
    return tile_shape()


def _shapes():
    th, tw = _tile()
    return [(1, 1), (1, 17), (17, 1), (3, 3), (7, 7), (8, 8), (15, 16), (37, 41), (257, 259), (th - 1, tw + 1), (th, tw), (th + 1, 2 * tw + 1)]


def random_taps(ksize, nf=8, seed=0):
    """Seeded taps with zeros, negatives and one subnormal per kernel (where the kernel has room for them)."""
    rng = np.random.default_rng(1000 * ksize + seed)
    t = rng.uniform(-1.0, 1.0, (nf, ksize, ksize)).astype(np.float32)
    if ksize >= 3:
        t[rng.uniform(size=t.shape) < 0.2] = 0.0
        for f in range(nf):
            i, j = rng.integers(0, ksize, 2)
            t[f, i, j] = np.float32((-1) ** f * 3e-41)   # subnormal: the smallest normal float32 is 1.18e-38
            t[f, (i + 1) % ksize, j] = -0.75
    else:
        t[0] = -0.625
    return t


def contents(h, w, seed):
    th, tw = _tile()
    rng = np.random.default_rng(seed)
    out = {"random": rng.integers(0, 256, (h, w), dtype=np.uint8), "zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8),
           "ramp": np.broadcast_to((np.arange(w) * 3 % 256).astype(np.uint8), (h, w)).copy()}
    for name, (y, x) in (("pixel_interior", (h // 2, w // 3)), ("pixel_corner", (0, w - 1)), ("pixel_seam", (th - 1, tw))):
        p = np.zeros((h, w), np.uint8)
        p[y, x] = 255
        out[name] = p
    return out


def run_raw(ctx, u8, taps):
    h, w = u8.shape
    planes, mm = ctx.correlate_u8(ctx.to_device(u8.reshape(-1)), h, w, taps, minmax=True)
    return [p.cpu().numpy().reshape(h, w) for p in planes], mm


def check_raw(ctx, u8, taps, refs32, refs64, what, nfs=NFS):
    """The planes of taps[:nf] for every nf of nfs: bit-equal to the float32 restatement, extrema equal to the planes' own,
    and within gamma_n * sum|k x| of the float64 restatement."""
    bounds = [R.gamma_bound(u8, k) for k in taps]
    for nf in nfs:
        got, mm = run_raw(ctx, u8, taps[:nf])
        assert len(got) == nf and mm.shape == (nf, 2)
        for f in range(nf):
            assert got[f].dtype == np.float32
            assert got[f].tobytes() == refs32[f].tobytes(), f"{what} nf={nf} kernel {f}: {int((got[f] != refs32[f]).sum())} pixels differ"
            assert mm[f, 0] == got[f].min() and mm[f, 1] == got[f].max(), (what, nf, f, mm[f], got[f].min(), got[f].max())
            assert np.all(np.abs(got[f].astype(np.float64) - refs64[f]) <= bounds[f]), (what, nf, f)


@pytest.mark.parametrize("ksize", KSIZES)
def test_raw_responses_every_shape(ctx, ksize):
    """Seeded random bytes on every shape (1 x 1 up to several tiles, the tile's own size and one off it), seeded taps."""
    taps = random_taps(ksize)
    for n, (h, w) in enumerate(_shapes()):
        u8 = np.random.default_rng(50 + n).integers(0, 256, (h, w), dtype=np.uint8)
        refs32 = [R.correlate_ref(u8, k, np.float32) for k in taps]
        refs64 = [R.correlate_ref(u8, k, np.float64) for k in taps]
        check_raw(ctx, u8, taps, refs32, refs64, f"ksize {ksize} shape {h}x{w}")


@pytest.mark.parametrize("ksize", KSIZES)
def test_raw_responses_every_content(ctx, ksize):
    """All 0 (every output +0), all 255, a column ramp, and one 255 on zeros — interior, in a corner, on a tile seam — where the
    response is the kernel turned by 180 degrees: a transposed or reversed tap order, or a flushed subnormal, shows.  At 5 x 5
    and 15 x 15 every count of kernels from 1 to 8, so that each compiled width also runs partly filled."""
    th, tw = _tile()
    h, w = th + 1, 2 * tw + 1
    taps = random_taps(ksize, seed=1)
    m = ksize // 2
    for name, u8 in contents(h, w, 3).items():
        refs32 = [R.correlate_ref(u8, k, np.float32) for k in taps]
        refs64 = [R.correlate_ref(u8, k, np.float64) for k in taps]
        if name == "zeros":
            assert all(r.tobytes() == bytes(4 * h * w) for r in refs32)
        if name == "pixel_interior":
            y, x = h // 2, w // 3
            for k, r in zip(taps, refs32):
                assert np.array_equal(r[y - m:y + m + 1, x - m:x + m + 1], np.float32(255) * k[::-1, ::-1])
        check_raw(ctx, u8, taps, refs32, refs64, f"ksize {ksize} content {name}", NFS_EVERY if ksize in (5, 15) else NFS)


@pytest.mark.parametrize("ns,no,group", [(4, 6, 0), (4, 6, 3), (7, 2, 5), (3, 4, 1)])
def test_raw_responses_gabor_taps(ctx, ns, no, group):
    """The product's own Gabor taps (the scale-0.1 group holds subnormal taps; (4, 6, 3) is 15 x 15, (7, 2, 5) is 9 x 9)."""
    from rsseg.gabor import gabor_plan
    th, tw = _tile()
    ksize, taps = gabor_plan(ns, no)[group]
    h, w = th + 1, 2 * tw + 1
    m = ksize // 2
    for name, u8 in contents(h, w, 9).items():
        got, mm = run_raw(ctx, u8, taps)
        for f, k in enumerate(taps):
            want = R.correlate_ref(u8, k, np.float32)
            assert got[f].tobytes() == want.tobytes(), (name, ksize, f)
            assert mm[f, 0] == want.min() and mm[f, 1] == want.max()
            assert np.all(np.abs(got[f].astype(np.float64) - R.correlate_ref(u8, k, np.float64)) <= R.gamma_bound(u8, k))
            if name == "pixel_interior":
                y, x = h // 2, w // 3
                # the sum starts at +0, so the -0 product of a -0 tap comes out +0
                want_k = np.float32(0) + np.float32(255) * k[::-1, ::-1]
                assert got[f][y - m:y + m + 1, x - m:x + m + 1].tobytes() == np.ascontiguousarray(want_k).tobytes()


def test_more_kernels_than_one_launch_holds(ctx):
    """19 kernels: three launches (8, 8, 3), planes and extrema in the caller's order."""
    taps = np.concatenate([random_taps(5, seed=2), random_taps(5, seed=3), random_taps(5, seed=4)[:3]])
    u8 = np.random.default_rng(11).integers(0, 256, (37, 41), dtype=np.uint8)
    got, mm = run_raw(ctx, u8, taps)
    assert len(got) == 19
    for f, k in enumerate(taps):
        want = R.correlate_ref(u8, k, np.float32)
        assert got[f].tobytes() == want.tobytes() and mm[f, 0] == want.min() and mm[f, 1] == want.max()


@pytest.mark.parametrize("ksize", [1, 5, 15])
def test_normalised_planes(ctx, ksize):
    """filter_bank_norm equals normalise_ref of the raw planes bit for bit; a constant plane gives zeros, not NaN."""
    th, tw = _tile()
    taps = random_taps(ksize, seed=5)
    for h, w in ((37, 41), (th + 1, 2 * tw + 1), (16, 16)):
        cs = contents(h, w, 21) if h > th and w > tw else {"random": np.random.default_rng(h).integers(0, 256, (h, w), dtype=np.uint8),
                                                "full": np.full((h, w), 255, np.uint8), "zeros": np.zeros((h, w), np.uint8)}
        for name, u8 in cs.items():
            for nf in NFS:
                q = ctx.to_device(u8.reshape(-1))
                raw = [p.cpu().numpy().reshape(h, w) for p in ctx.correlate_u8(q, h, w, taps[:nf])]
                got = [p.cpu().numpy().reshape(h, w) for p in ctx.filter_bank_norm(q, h, w, taps[:nf])]
                assert len(got) == nf
                for f in range(nf):
                    want = R.normalise_ref(raw[f])
                    assert got[f].dtype == np.float32 and got[f].tobytes() == want.tobytes(), (ksize, name, h, w, nf, f)
                    if name in ("full", "zeros"):
                        assert got[f].tobytes() == bytes(4 * h * w)


@pytest.fixture(scope="module")
def crop(golden_dir):
    return np.load(os.path.join(golden_dir, "crop96.npz"))


@pytest.mark.parametrize("ns,no", [(4, 6), (1, 1), (3, 4), (7, 2)])
def test_calculate_gabor_features_on_the_golden_crop(ctx, oracle, crop, ns, no):
    """The mirror on the NIR plane of the golden crop: oracle.robust_normalize -> oracle.to_u8 -> the restated bank, bit for bit;
    length, order, dtype; the input untouched; two calls identical."""
    from modules.features import indices as I
    nir = crop["norm"][3].copy()
    keep = nir.copy()
    got = I.calculate_gabor_features(nir) if (ns, no) == (4, 6) else I.calculate_gabor_features(nir, ns, no)
    assert np.array_equal(nir, keep)
    want = R.bank_ref(oracle.to_u8(oracle.robust_normalize(nir)), ns, no)
    assert isinstance(got, list) and len(got) == len(want) == ns * len(np.arange(0, np.pi, np.pi / no))
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == (96, 96)
        assert g.tobytes() == w_.tobytes(), f"filter {i}: {int((g != w_).sum())} pixels differ"
        assert g.min() == 0.0 and 0.99 < g.max() <= 1.0
    again = I.calculate_gabor_features(nir, num_scales=ns, num_orientations=no)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_calculate_gabor_features_edges(ctx, crop):
    from modules.features import indices as I
    from rsseg.runtime import RssegUnsupported
    nir = crop["norm"][3]
    assert I.calculate_gabor_features(nir, num_scales=0) == []
    with pytest.raises(RssegUnsupported, match="astype"):
        I.calculate_gabor_features(nir.astype(np.float64))


def test_prepare_features_for_segmentation_equals_the_reference(ctx, golden_dir):
    """Against tests/golden/indices_helpers.npz bit for bit (the reference's robust_normalize is NumPy; the mirror's runs on the
    GPU), the exception's text included."""
    import modules.features.indices as M
    D, seg, manifest, z = HC.load(os.path.join(golden_dir, "indices_helpers.npz"))
    n = 0
    for i, entry in enumerate(manifest):
        if entry["fn"] in HC.GPU_FUNCTIONS:
            HC.check(i, entry, HC.replay(M, entry, D, seg), z)
            n += 1
    assert n == 3


def test_invalid_arguments_return_the_error_code_and_a_message(ctx):
    lib = ctx.lib
    q = ctx.to_device(np.zeros(64, np.uint8))
    out = ctx.empty(8 * 64, __import__("torch").float32)
    taps = np.ones(16 * 16 * 2, np.float32)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))

    def both(h, w, ksize, nf, word):
        for rc in (lib.rsseg_correlate_u8_f32(ctx.h, C.c_void_p(q.data_ptr()), h, w, tp, ksize, nf, C.c_void_p(out.data_ptr()), None),
                   lib.rsseg_filter_bank_norm_u8(ctx.h, C.c_void_p(q.data_ptr()), h, w, tp, ksize, nf, C.c_void_p(out.data_ptr()))):
            assert rc == -1
            assert word in lib.rsseg_last_error(ctx.h).decode(), lib.rsseg_last_error(ctx.h).decode()

    both(8, 8, 4, 1, "kernel size 4")
    both(8, 8, 17, 1, "kernel size 17")
    both(8, 8, 0, 1, "kernel size 0")
    both(8, 8, -3, 1, "kernel size -3")
    both(8, 8, 3, 0, "0 kernels")
    both(0, 8, 3, 1, "0 x 8")
    both(8, 0, 3, 1, "8 x 0")
    for bad in (np.nan, np.inf, -np.inf):
        taps[9 + 4] = bad
        both(8, 8, 3, 2, "tap 4 of kernel 1 is not finite")
    taps[9 + 4] = 1.0
    with pytest.raises(ValueError, match="kernel size 4"):
        ctx.correlate_u8(q, 8, 8, np.ones((1, 4, 4), np.float32))
    got = ctx.correlate_u8(q, 8, 8, np.ones((1, 3, 3), np.float32))   # the context still works after the refusals
    assert np.array_equal(got[0].cpu().numpy(), np.zeros(64, np.float32))

"""K19 on the GPU, bit for bit against its NumPy restatement (tests/compact_ref.py): rsseg_compact_plan / _compact_planes /
_expand_plane across the tile and scan seams, mask shapes, element sizes, plane counts and alignments, and rsseg_valid_mask
across its flags and dtypes.  Data movement only: every comparison is exact, on integer bit patterns."""
import ctypes as C

import numpy as np
import pytest

import compact_ref as CR

pytestmark = pytest.mark.gpu

G = 16   # guard elements on either side of an output (16 elements are a multiple of 16 bytes for every element size)
SENTINEL = {1: 0xA5, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
NP = {1: np.uint8, 4: np.int32, 8: np.int64}


@pytest.fixture(scope="module")
def seams(ctx):
    return ctx.lib.rsseg_compact_tile(), ctx.lib.rsseg_compact_scan_span()


def pixel_counts(T, S):
    return [1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5, 70 * T + 3, (S + 1) * T + 1]


N_IDS = ["1", "15", "16", "17", "T-1", "T", "T+1", "2T+5", "70T+3", "(S+1)T+1"]
MASKS = ["all", "none", "first", "last", "alternating", "half", "sparse", "rectangle", "bytes"]


def make_mask(kind, n, rng):
    m = np.zeros(n, np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[-1] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "half":
        m = (rng.random(n) < 0.5).astype(np.uint8)
    elif kind == "sparse":
        m = (rng.random(n) < 0.01).astype(np.uint8)
    elif kind == "rectangle":     # a rectangle inside an H x W raster whose row length (37) is no multiple of 16; the rest is a tail
        W = 37 if n >= 74 else n
        H = n // W
        r = np.zeros((H, W), np.uint8)
        r[H // 5: H - H // 7, W // 6: W - W // 4] = 1
        m[:H * W] = r.reshape(-1)
    elif kind == "bytes":         # any non-zero byte means valid
        m = np.where(rng.random(n) < 0.5, rng.choice(np.array([1, 2, 255], np.uint8), n), 0).astype(np.uint8)
    return m


def random_elems(rng, n, eb):
    return np.frombuffer(rng.bytes(n * eb), NP[eb]).copy()


class Raw:
    """The C entry points on buffers one element off a 16-byte boundary, with guards around every output."""

    def __init__(self, ctx):
        import torch
        self.ctx, self.torch = ctx, torch

    def upload(self, a, misalign):
        """`a` on the device at `misalign` elements past an aligned address -> (keep-alive tensor, address)"""
        buf = self.torch.zeros(a.size + misalign + 1, dtype=self.torch.from_numpy(a[:0].copy()).dtype, device=self.ctx.device)
        buf[misalign:misalign + a.size] = self.torch.from_numpy(a).to(self.ctx.device)
        return buf, buf.data_ptr() + misalign * a.itemsize

    def guarded(self, count, eb, misalign):
        t = self.torch.from_numpy(np.full(count + 2 * G + misalign, SENTINEL[eb], np.uint64).astype(NP[eb])).to(self.ctx.device)
        return t, t.data_ptr() + (G + misalign) * eb

    def read_guarded(self, t, count, misalign):
        a = t.cpu().numpy()
        lo, body, hi = a[:G + misalign], a[G + misalign:G + misalign + count], a[G + misalign + count:]
        want = np.uint64(SENTINEL[a.itemsize]).astype(a.dtype)
        assert np.all(lo == want) and np.all(hi == want), "a guard element was written"
        return body

    def plan(self, mask_addr, n, T):
        off = self.torch.full(((n + T - 1) // T + 1,), -1, dtype=self.torch.int64, device=self.ctx.device)
        nv = C.c_int64(-1)
        self.ctx._chk(self.ctx.lib.rsseg_compact_plan(self.ctx.h, C.c_void_p(mask_addr), n, C.c_void_p(off.data_ptr()), C.byref(nv)))
        return off, nv.value

    def compact(self, mask_addr, off, n, in_addrs, eb, out_addrs):
        arr_in = (C.c_void_p * len(in_addrs))(*in_addrs)
        arr_out = (C.c_void_p * len(out_addrs))(*out_addrs)
        self.ctx._chk(self.ctx.lib.rsseg_compact_planes(self.ctx.h, C.c_void_p(mask_addr), C.c_void_p(off.data_ptr()), n, arr_in, len(in_addrs), eb,
                                                        arr_out))

    def expand(self, mask_addr, off, n, in_addr, eb, fill, out_addr):
        fb = np.array(fill, NP[eb]).tobytes()
        self.ctx._chk(self.ctx.lib.rsseg_expand_plane(self.ctx.h, C.c_void_p(mask_addr), C.c_void_p(off.data_ptr()), n, C.c_void_p(in_addr), eb, fb,
                                                      C.c_void_p(out_addr)))


def run_case(raw, T, n, mask, eb, P, rng, misalign):
    """plan + compact + expand of P planes against compact_ref; inputs, mask and outputs `misalign` elements off alignment"""
    nv_want = int((mask != 0).sum())
    mkeep, maddr = raw.upload(mask, misalign)
    off, nv = raw.plan(maddr, n, T)
    offs = off.cpu().numpy()
    ntiles = (n + T - 1) // T
    counts = np.add.reduceat((mask != 0).astype(np.int64), np.arange(0, n, T))
    assert nv == nv_want and offs[-1] == nv_want
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(counts)])) and offs.size == ntiles + 1
    planes = [random_elems(rng, n, eb) for _ in range(P)]
    ins = [raw.upload(p, misalign) for p in planes]
    outs = [raw.guarded(nv, eb, misalign) for _ in range(P)]
    raw.compact(maddr, off, n, [a for _, a in ins], eb, [a for _, a in outs])
    for p, (t, _) in zip(planes, outs):
        got = raw.read_guarded(t, nv, misalign)
        assert np.array_equal(got, CR.compact(p, mask))
        if nv == n:
            assert np.array_equal(got, p)                 # every pixel valid: a plain copy
    # expand(compact(x)) == x where valid, fill elsewhere (the first and the last plane)
    fill = int(np.uint64(0x1122334455667788).astype(NP[eb]))
    for i in sorted({0, P - 1}):
        cbuf, caddr = raw.upload(CR.compact(planes[i], mask), misalign) if nv else (None, 0)
        et, eaddr = raw.guarded(n, eb, misalign)
        raw.expand(maddr, off, n, caddr, eb, fill, eaddr)
        got = raw.read_guarded(et, n, misalign)
        assert np.array_equal(got, np.where(mask != 0, planes[i], np.array(fill, NP[eb])))
        assert np.array_equal(got, CR.expand(CR.compact(planes[i], mask), mask, fill))


@pytest.mark.parametrize("ni", range(10), ids=N_IDS)
def test_compact_and_expand_bit_for_bit(ctx, seams, ni):
    """Every mask kind x every element size with one plane, buffers one element off a 16-byte boundary; then 15 and 19 planes
    (aligned, as the classifiers' planes are, and misaligned) on the random mask."""
    T, S = seams
    n = pixel_counts(T, S)[ni]
    raw = Raw(ctx)
    rng = np.random.default_rng(100 + ni)
    big = n > 100 * T
    for kind in (["all", "none", "last", "half"] if big else MASKS):   # the scan's second pass: the masks that move its carry
        mask = make_mask(kind, n, rng)
        for eb in (1, 4, 8):
            run_case(raw, T, n, mask, eb, 1, rng, misalign=1)
    mask = make_mask("half", n, rng)
    for P, eb, mis in ([(15, 4, 0)] if big else [(15, 4, 0), (19, 8, 0), (19, 1, 1), (15, 8, 1), (19, 4, 1)]):
        run_case(raw, T, n, mask, eb, P, rng, misalign=mis)


def test_context_methods_and_corner_cases(ctx, seams):
    import torch
    T, S = seams
    rng = np.random.default_rng(5)
    n = 3 * T + 77
    mask = make_mask("bytes", n, rng)
    x32, x64, xi = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n), rng.integers(-5, 5, n).astype(np.int32)
    u8 = rng.integers(0, 256, n).astype(np.uint8)
    plan = ctx.compact_plan(ctx.to_device(mask))
    assert (plan.n, plan.n_valid) == (n, int((mask != 0).sum())) and plan.tile_off.numel() == 4 + 1
    outs = ctx.compact(plan, [ctx.to_device(a) for a in (x32, x64, xi, u8)])     # mixed element sizes: one launch per size
    for a, o in zip((x32, x64, xi, u8), outs):
        assert o.dtype == torch.from_numpy(a[:1]).dtype and np.array_equal(o.cpu().numpy(), CR.compact(a, mask))
    back = ctx.expand(plan, outs[0], float("nan")).cpu().numpy()
    assert np.array_equal(back[mask != 0], x32[mask != 0]) and np.all(np.isnan(back[mask == 0]))
    assert np.array_equal(ctx.expand(plan, outs[2], -1).cpu().numpy(), CR.expand(CR.compact(xi, mask), mask, -1))
    assert np.array_equal(ctx.expand(plan, outs[1], 0.0).cpu().numpy(), CR.expand(CR.compact(x64, mask), mask, 0.0))
    # the plan survives a call that uses the context's workspace
    ctx.kmeans_fit_predict([ctx.to_device(x32), ctx.to_device(x32 * 2)], 3)
    assert np.array_equal(ctx.expand(plan, outs[3], 7).cpu().numpy(), CR.expand(CR.compact(u8, mask), mask, 7))
    # n == 0, n_valid == 0
    empty = ctx.compact_plan(torch.zeros(0, dtype=torch.uint8, device=ctx.device))
    assert (empty.n, empty.n_valid) == (0, 0) and empty.tile_off.cpu().numpy().tolist() == [0]
    assert ctx.compact(empty, [torch.zeros(0, dtype=torch.float32, device=ctx.device)])[0].numel() == 0
    assert ctx.expand(empty, torch.zeros(0, dtype=torch.float32, device=ctx.device), 1.0).numel() == 0
    none = ctx.compact_plan(ctx.to_device(np.zeros(n, np.uint8)))
    assert none.n_valid == 0 and ctx.compact(none, [ctx.to_device(x32)])[0].numel() == 0
    assert np.all(ctx.expand(none, torch.zeros(0, dtype=torch.int32, device=ctx.device), -1).cpu().numpy() == -1)
    # errors name the argument
    d = ctx.to_device(x32)
    pp = ctx._pp([d])
    lib, h = ctx.lib, ctx.h
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    one = np.float32(1).tobytes()

    def refused(rc, text):
        assert rc == -1 and text in lib.rsseg_last_error(h).decode(), lib.rsseg_last_error(h).decode()

    refused(lib.rsseg_expand_plane(h, ptr(plan.mask), ptr(plan.tile_off), n, ptr(d), 4, one, ptr(d)), "d_out aliases d_in")
    refused(lib.rsseg_expand_plane(h, ptr(plan.mask), ptr(plan.tile_off), n, C.c_void_p(d.data_ptr() + 400), 4, one, ptr(d)), "d_out aliases d_in")
    refused(lib.rsseg_expand_plane(h, ptr(plan.mask), ptr(plan.tile_off), n, ptr(d), 2, one, ptr(outs[0])), "elem_bytes=2")
    refused(lib.rsseg_compact_planes(h, ptr(plan.mask), ptr(plan.tile_off), n, pp, 1, 3, pp), "elem_bytes=3")
    refused(lib.rsseg_compact_planes(h, ptr(plan.mask), ptr(plan.tile_off), n, pp, 1, 4, pp), "d_out[0] aliases d_in[0]")
    refused(lib.rsseg_compact_planes(h, None, ptr(plan.tile_off), n, pp, 1, 4, ctx._pp([outs[0]])), "d_mask is null")
    refused(lib.rsseg_compact_plan(h, ptr(plan.mask), n, None, C.byref(C.c_int64())), "d_tile_off null")
    refused(lib.rsseg_compact_plan(h, ptr(plan.mask), -1, ptr(plan.tile_off), C.byref(C.c_int64())), "n=-1")
    refused(lib.rsseg_valid_mask(h, pp, 1, 2, n, 1, C.c_double(0), None, ptr(plan.mask), C.byref(C.c_int64())), "dtype must be")
    refused(lib.rsseg_valid_mask(h, pp, 1, 0, n, 8, C.c_double(0), None, ptr(plan.mask), C.byref(C.c_int64())), "flags=8")
    refused(lib.rsseg_valid_mask(h, pp, 0, 0, n, 1, C.c_double(0), None, ptr(plan.mask), C.byref(C.c_int64())), "d_planes is empty")


# ---- rsseg_valid_mask -------------------------------------------------------------------------------------------------------
def mask_planes(rng, n, P, dt):
    """P planes with NaN, +-inf and the nodata value (5) scattered, in different planes of the same pixel too"""
    if dt == np.uint8:
        planes = [rng.integers(0, 256, n).astype(np.uint8) for _ in range(P)]
        for p in planes:
            p[rng.random(n) < 0.05] = 5
        return planes
    planes = [rng.standard_normal(n).astype(dt) for _ in range(P)]
    for p in planes:
        for v in (np.nan, np.inf, -np.inf, 5.0):
            p[rng.random(n) < 0.03] = v
    for j, v in enumerate((np.nan, np.inf, 5.0, -np.inf)):     # one pixel, a different reason in every plane it has
        planes[j % P][min(7, n - 1)] = v
    return planes


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.uint8], ids=["float32", "float64", "uint8"])
@pytest.mark.parametrize("P", [1, 7])
def test_valid_mask(ctx, seams, dt, P):
    T, _ = seams
    rng = np.random.default_rng(17 + P)
    for n in (1, 17, 2 * T + 5):
        planes = mask_planes(rng, n, P, dt)
        dev = [ctx.to_device(p) for p in planes]
        am = (rng.random(n) < 0.8).astype(np.uint8) * 3
        for nan, inf, nodata in [(True, False, None), (False, True, None), (False, False, 5.0), (True, True, 5.0), (False, False, None)]:
            flags = (CR.VALID_NAN if nan else 0) | (CR.VALID_INF if inf else 0) | (CR.VALID_VALUE if nodata is not None else 0)
            for and_mask in (None, am):
                got, nv = ctx.valid_mask(dev, nan=nan, inf=inf, nodata=nodata, and_mask=None if and_mask is None else ctx.to_device(and_mask))
                want = CR.valid_mask(planes, flags, 0.0 if nodata is None else nodata, and_mask)
                assert got.dtype.__str__() == "torch.uint8" and np.array_equal(got.cpu().numpy(), want), (n, flags, and_mask is not None)
                assert nv == int(want.sum())
    # planes and mask one element off a 16-byte boundary
    n = T + 9
    planes = mask_planes(rng, n, P, dt)
    import torch
    bufs = [torch.zeros(n + 1, dtype=torch.from_numpy(p[:1]).dtype, device=ctx.device) for p in planes]
    for b, p in zip(bufs, planes):
        b[1:] = torch.from_numpy(p).to(ctx.device)
    mbuf = torch.full((n + 1 + 2 * G,), 9, dtype=torch.uint8, device=ctx.device)
    nv = C.c_int64(0)
    arr = (C.c_void_p * P)(*[b.data_ptr() + p.itemsize for b, p in zip(bufs, planes)])
    code = {np.float32: 0, np.float64: 1, np.uint8: 3}[dt]
    ctx._chk(ctx.lib.rsseg_valid_mask(ctx.h, arr, P, code, n, 7, C.c_double(5.0), None, C.c_void_p(mbuf.data_ptr() + G + 1), C.byref(nv)))
    got = mbuf.cpu().numpy()
    want = CR.valid_mask(planes, 7, 5.0)
    assert np.array_equal(got[G + 1:G + 1 + n], want) and np.all(got[:G + 1] == 9) and np.all(got[G + 1 + n:] == 9) and nv.value == int(want.sum())
    # a value the type cannot hold matches nothing
    if dt == np.uint8:
        got, nv = ctx.valid_mask([ctx.to_device(p) for p in planes], nodata=300.0)
        assert nv == n and bool(got.cpu().numpy().all())

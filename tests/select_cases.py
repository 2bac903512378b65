"""The case table of the K1 sweep (tests/test_gpu_select.py runs it on the GPU, tests/test_select_cases_host.py checks
on the CPU that every case belongs to the classes it claims).  NumPy only; every input comes from a seeded generator.

A case is (name, planes, ranks, grid_cap): float32 planes of equal length, one rank list per plane, and the workgroup
cap to put into RSSEG_K1_GRID (None: the kernel's own 512).  CLAIMS, at the end of the file, holds for every case the
classes it was written for, as plain data:

    name: (fast, loops, ((ndp1, ndp2, ((nprefix, n1), ...), shared11), ...))

fast    the small-integer route: "taken", "refused", or "refused@first" / "@last" / "@wg" / "@tail" for the planes whose
        only disqualifying value sits at one of the four positions of the geometry family;
loops   which loops of k1_hist execute: B batched, T one-load tail, S scalar tail (lower case: not);
per plane: the tables of pass 1 and pass 2, per pass-2 launch its live 22-bit prefixes and the distinct 11-bit
        prefixes among them, and whether one 11-bit prefix occurs in two pass-2 launches.

`python tests/select_cases.py` prints CLAIMS as tests/select_ref.py computes it — for writing a new case down, not
for the tests, which compare the two.
"""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name planes ranks grid_cap")

WG = 1024                      # float4 per workgroup and stride step of k1_hist
BAD = np.float32(7.5)          # the one value of a `bad@p` plane that is no small integer
# (G, n4 as a multiple of S = G * 1024 plus a rest, t, a float4 only the one-load tail loop reads or None, loops)
GEOMETRIES = [
    (1, (3, 0), 0, 1500, "bTs"),      # the largest plane that still skips the batched loop
    (1, (3, 1), 1, 1500, "BTS"),      # only lane 0 enters it
    (1, (4, 0), 2, None, "BtS"),      # every lane one batch, nothing left for the tail loop
    (1, (4, 1), 3, 4096, "BTS"),      # one float4 left, for lane 0
    (2, (4, -1), 1, 4095, "BTS"),     # the last lane of the grid makes no batch: three tail steps instead
    (2, (8, 777), 3, 16500, "BTS"),   # two batches per lane: the stop flag of the small-integer pass can be SEEN
    (3, (4, 1), 0, 12288, "BTs"),     # one float4 beyond the batches and no scalar tail
    (3, (11, 5), 2, 24676, "BTS"),    # lanes 0..4 make three batches, the others two and three tail steps
]
PREFIX_N = 40003


def ranks16(n):
    """0, n - 1 and 14 evenly spaced ranks between them (fewer when n < 16: every rank)."""
    return sorted({int(r) for r in np.linspace(0, n - 1, 16).round()})


def geometry_n(g):
    G, (mul, rest), t = g[0], g[1], g[2]
    return 4 * (mul * G * WG + rest) + t


def geometry_name(g):
    G, (mul, rest), t = g[0], g[1], g[2]
    return f"g{G}_{mul}S{rest:+d}_t{t}"


def bad_positions(g):
    """{tag: float index} of the four places a lone 7.5 is put at (fewer where two coincide or none exists)."""
    G, tail4 = g[0], g[3]
    n = geometry_n(g)
    pos = {"first": 0, "last": n - 1}
    if G > 1:
        pos["wg"] = 4 * (G - 1) * WG      # first float4 of the last workgroup (G == 1: that is position 0)
    if tail4 is not None:
        pos["tail"] = 4 * tail4 + 1
    return pos


def _ints(rng, n):
    return rng.integers(0, 256, n).astype(np.float32)


def _normal(rng, n):
    return (rng.standard_normal(n) * 1e3).astype(np.float32)


def _geometry_cases():
    out = []
    for gi, g in enumerate(GEOMETRIES):
        n, name = geometry_n(g), geometry_name(g)
        rng = np.random.default_rng(100 + gi)
        ints, normal = _ints(rng, n), _normal(rng, n)
        nan = normal.copy()
        nan[rng.choice(n, n // 100, replace=False)] = np.nan
        contents = [("ints", ints), ("normal", normal), ("nan", nan)]
        for tag, p in bad_positions(g).items():
            a = ints.copy()
            a[p] = BAD
            contents.append((f"bad@{tag}", a))
        for tag, a in contents:
            out.append(Case(f"{name}-{tag}", [a], [ranks16(n)], g[0]))
    return out


def prefix_planes():
    """The five planes of the prefix family, each from its own default_rng(0)."""
    n = PREFIX_N
    f32 = np.float32
    r = np.random.default_rng(0)
    one22 = (1.0 + r.integers(0, 1024, n) * 2.0 ** -23).astype(f32)
    r = np.random.default_rng(0)
    one11 = (1.0 + 0.25 * r.random(n)).astype(f32)
    r = np.random.default_rng(0)
    three11 = (r.choice([1.0, 1.25, -3.0], n) * (1.0 + 0.1 * r.random(n))).astype(f32)
    r = np.random.default_rng(0)
    wide = (r.choice([-1.0, 1.0], n) * np.ldexp(1.0 + r.random(n), r.integers(-12, 13, n))).astype(f32)
    r = np.random.default_rng(0)
    subnormal = (r.integers(-500, 500, n).astype(np.float64) * 1e-45).astype(f32)
    return {"one22": one22, "one11": one11, "three11": three11, "wide": wide, "subnormal": subnormal}


def _prefix_cases():
    n = PREFIX_N
    planes = prefix_planes()
    out = [Case(f"prefix-{k}", [a], [ranks16(n)], None) for k, a in planes.items()]
    group = list(planes.values()) + [_ints(np.random.default_rng(1), n)]
    out.append(Case("prefix-group6", group, [ranks16(n)] * len(group), None))
    return out


def specials_plane():
    """37 values at the edges of the key: both infinities, +-FLT_MAX, subnormals and the smallest normals on both sides of
    both zeros, +-1, the neighbours of 1 and of the small-integer bound, and five NaNs of three bit patterns (quiet,
    quiet with the sign bit, signalling).  Shuffled, so that neither loads nor ranks meet them in order."""
    f = np.finfo(np.float32)
    one_up, one_dn = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))
    vals = np.array([np.inf, -np.inf, f.max, -f.max, 1e-45, -1e-45, f.tiny, -f.tiny, 0.0, -0.0, 1.0, -1.0,
                     f.tiny - 1e-45, -(f.tiny - 1e-45), one_up, -one_up, one_dn, -one_dn, 2047.0, 2048.0, -2047.0, 0.5, -0.5,
                     np.inf, -np.inf, 0.0, -0.0, 1.0, 3e-45, -3e-45, f.max / 2, -f.max / 2], dtype=np.float32)
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffc00000, 0x7f800001], dtype=np.uint32).view(np.float32)
    a = np.concatenate([vals, nans])
    assert a.size == 37
    a = a[np.random.default_rng(37).permutation(37)]
    assert np.isnan(a).sum() == 5
    return np.ascontiguousarray(a)


def _lone(value):
    """A 4099-element plane of 8-bit integers with one `value`, and ranks around the place it sorts to."""
    rng = np.random.default_rng(5)
    a = _ints(rng, 4099)
    a[1234] = value
    at = int(np.searchsorted(np.sort(a), np.float32(value)))
    ranks = sorted({int(r) for r in np.linspace(0, 4098, 12).round()} | {max(at - 1, 0), at, min(at + 1, 4098)})
    return a, ranks


def _edge_cases():
    out = []
    sp = specials_plane()
    for lo, hi in [(0, 16), (16, 32), (32, 37)]:     # the last call: every requested rank is a NaN rank
        out.append(Case(f"edge-specials{lo}to{hi - 1}", [sp], [list(range(lo, hi))], None))
    nanv = np.float32(np.nan)
    for n in (1, 5, 4099):
        out.append(Case(f"edge-allnan{n}", [np.full(n, nanv)], [ranks16(n)], None))
    tenth, seven = np.full(4099, np.float32(0.1)), np.full(4099, np.float32(7.0))
    out.append(Case("edge-equal0.1", [tenth], [ranks16(4099)], None))
    out.append(Case("edge-equal7", [seven], [ranks16(4099)], None))
    # an all-NaN plane is a small-integer plane (it has no other value), so on its own it never reaches pass 0; next to a
    # general plane it does, and leaves after it (no live rank) while its neighbour goes on
    out.append(Case("edge-allnan+equal0.1", [np.full(4099, nanv), tenth], [ranks16(4099)] * 2, None))
    for n in range(1, 8):
        rng = np.random.default_rng(n)
        out.append(Case(f"edge-n{n}-normal", [_normal(rng, n)], [list(range(n))], None))
        out.append(Case(f"edge-n{n}-ints", [_ints(rng, n)], [list(range(n))], None))
    for tag, v in [("1e-45", 1e-45), ("2047.5", 2047.5), ("-1e-45", -1e-45)]:
        a, ranks = _lone(np.float32(v))
        out.append(Case(f"edge-lone{tag}", [a], [ranks], None))
    out.append(Case("edge-negzeros", [np.full(133, np.float32(-0.0))], [ranks16(133)], None))
    return out


def build_cases():
    cases = _geometry_cases() + _prefix_cases() + _edge_cases()
    for c in cases:
        assert all(p.dtype == np.float32 and p.ndim == 1 and p.size == c.planes[0].size for p in c.planes), c.name
        assert len(c.planes) == len(c.ranks) and all(1 <= len(r) <= 16 and len(r) == len(c.ranks[0]) for r in c.ranks), c.name
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}

# Refusals: (name, plane length, ranks, offset of the plane in floats from a 16-byte boundary, text of the error)
REFUSALS = [
    ("rank-1", 1000, [0, -1], 0, r"rank -1 outside \[0,1000\)"),
    ("rank-n", 1000, [999, 1000], 0, r"rank 1000 outside \[0,1000\)"),
    ("rank-n-ints", 1000, [1000], 0, r"rank 1000 outside \[0,1000\)"),
    ("17ranks", 1000, list(range(17)), 0, r"bad arguments \(.*nranks=17\)"),
    ("misaligned", 1000, [0], 1, r"16-byte aligned"),
]

# uint8: the smallest plane that sends some lanes of k1_hist_u8 through two iterations of the two-load loop and the
# others through one iteration plus the tail loop, and the smaller one (one two-load iteration for 1031 lanes)
U8_N16 = 3 * 2048 * 1024 + 1031
U8_N16_SMALL = 2048 * 1024 + 1031
U8_REST = 11


def u8_plane(n16=U8_N16):
    """Random bytes, 0 and 255 both present, 16 * n16 + 11 of them."""
    n = 16 * n16 + U8_REST
    a = np.random.default_rng(8).integers(0, 256, n, dtype=np.uint8)
    a[-1], a[-2] = 0, 255            # in the scalar tail
    return a


def sharded_case():
    """The `wide` plane cut at (0, 5, 5, n): a rank of five elements, a rank of none, a rank with the rest."""
    a = prefix_planes()["wide"]
    return a, ranks16(a.size), (0, 5, 5, a.size)


# ---- the classes every case claims (see the module docstring) -------------------------------------------------------
CLAIMS = {
    'g1_3S+0_t0-ints': ('taken', 'bTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_3S+0_t0-normal': ('refused', 'bTs', ((16, 16, ((8, 8), (8, 8)), False),)),
    'g1_3S+0_t0-nan': ('refused', 'bTs', ((15, 15, ((8, 8), (7, 7)), False),)),
    'g1_3S+0_t0-bad@first': ('refused@first', 'bTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_3S+0_t0-bad@last': ('refused@last', 'bTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_3S+0_t0-bad@tail': ('refused@tail', 'bTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_3S+1_t1-ints': ('taken', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_3S+1_t1-normal': ('refused', 'BTS', ((16, 16, ((8, 8), (8, 8)), False),)),
    'g1_3S+1_t1-nan': ('refused', 'BTS', ((15, 15, ((8, 8), (7, 7)), False),)),
    'g1_3S+1_t1-bad@first': ('refused@first', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_3S+1_t1-bad@last': ('refused@last', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_3S+1_t1-bad@tail': ('refused@tail', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_4S+0_t2-ints': ('taken', 'BtS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_4S+0_t2-normal': ('refused', 'BtS', ((16, 16, ((8, 8), (8, 8)), False),)),
    'g1_4S+0_t2-nan': ('refused', 'BtS', ((15, 15, ((8, 8), (7, 7)), False),)),
    'g1_4S+0_t2-bad@first': ('refused@first', 'BtS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_4S+0_t2-bad@last': ('refused@last', 'BtS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_4S+1_t3-ints': ('taken', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_4S+1_t3-normal': ('refused', 'BTS', ((16, 16, ((8, 8), (8, 8)), False),)),
    'g1_4S+1_t3-nan': ('refused', 'BTS', ((15, 15, ((8, 8), (7, 7)), False),)),
    'g1_4S+1_t3-bad@first': ('refused@first', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_4S+1_t3-bad@last': ('refused@last', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g1_4S+1_t3-bad@tail': ('refused@tail', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_4S-1_t1-ints': ('taken', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_4S-1_t1-normal': ('refused', 'BTS', ((16, 16, ((8, 8), (8, 8)), False),)),
    'g2_4S-1_t1-nan': ('refused', 'BTS', ((15, 15, ((8, 8), (7, 7)), False),)),
    'g2_4S-1_t1-bad@first': ('refused@first', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_4S-1_t1-bad@last': ('refused@last', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_4S-1_t1-bad@wg': ('refused@wg', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_4S-1_t1-bad@tail': ('refused@tail', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_8S+777_t3-ints': ('taken', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_8S+777_t3-normal': ('refused', 'BTS', ((16, 16, ((8, 8), (8, 8)), False),)),
    'g2_8S+777_t3-nan': ('refused', 'BTS', ((15, 15, ((8, 8), (7, 7)), False),)),
    'g2_8S+777_t3-bad@first': ('refused@first', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_8S+777_t3-bad@last': ('refused@last', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_8S+777_t3-bad@wg': ('refused@wg', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g2_8S+777_t3-bad@tail': ('refused@tail', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_4S+1_t0-ints': ('taken', 'BTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_4S+1_t0-normal': ('refused', 'BTs', ((16, 16, ((8, 8), (8, 8)), False),)),
    'g3_4S+1_t0-nan': ('refused', 'BTs', ((15, 15, ((8, 8), (7, 7)), False),)),
    'g3_4S+1_t0-bad@first': ('refused@first', 'BTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_4S+1_t0-bad@last': ('refused@last', 'BTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_4S+1_t0-bad@wg': ('refused@wg', 'BTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_4S+1_t0-bad@tail': ('refused@tail', 'BTs', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_11S+5_t2-ints': ('taken', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_11S+5_t2-normal': ('refused', 'BTS', ((16, 16, ((8, 8), (8, 8)), False),)),
    'g3_11S+5_t2-nan': ('refused', 'BTS', ((15, 15, ((8, 8), (7, 7)), False),)),
    'g3_11S+5_t2-bad@first': ('refused@first', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_11S+5_t2-bad@last': ('refused@last', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_11S+5_t2-bad@wg': ('refused@wg', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'g3_11S+5_t2-bad@tail': ('refused@tail', 'BTS', ((12, 16, ((8, 8), (8, 4)), False),)),
    'prefix-one22': ('refused', 'bTS', ((1, 1, ((1, 1),), False),)),
    'prefix-one11': ('refused', 'bTS', ((1, 16, ((8, 1), (8, 1)), True),)),
    'prefix-three11': ('refused', 'bTS', ((3, 16, ((8, 2), (8, 2)), True),)),
    'prefix-wide': ('refused', 'bTS', ((16, 16, ((8, 8), (8, 8)), False),)),
    'prefix-subnormal': ('refused', 'bTS', ((2, 2, ((2, 2),), False),)),
    'prefix-group6': ('refused', 'bTS', ((1, 1, ((1, 1),), False), (1, 16, ((8, 1), (8, 1)), True), (3, 16, ((8, 2), (8, 2)), True), (16, 16, ((8, 8), (8, 8)), False), (2, 2, ((2, 2),), False), (12, 16, ((8, 8), (8, 4)), False))),
    'edge-specials0to15': ('refused', 'bTS', ((11, 11, ((8, 8), (3, 3)), False),)),
    'edge-specials16to31': ('refused', 'bTS', ((11, 11, ((8, 8), (3, 3)), False),)),
    'edge-specials32to36': ('refused', 'bTS', ((0, 0, (), False),)),
    'edge-allnan1': ('taken', 'btS', ((0, 0, (), False),)),
    'edge-allnan5': ('taken', 'bTS', ((0, 0, (), False),)),
    'edge-allnan4099': ('taken', 'bTS', ((0, 0, (), False),)),
    'edge-equal0.1': ('refused', 'bTS', ((1, 1, ((1, 1),), False),)),
    'edge-equal7': ('taken', 'bTS', ((1, 1, ((1, 1),), False),)),
    'edge-allnan+equal0.1': ('refused', 'bTS', ((0, 0, (), False), (1, 1, ((1, 1),), False))),
    'edge-n1-normal': ('refused', 'btS', ((1, 1, ((1, 1),), False),)),
    'edge-n1-ints': ('taken', 'btS', ((1, 1, ((1, 1),), False),)),
    'edge-n2-normal': ('refused', 'btS', ((2, 2, ((2, 2),), False),)),
    'edge-n2-ints': ('taken', 'btS', ((2, 2, ((2, 2),), False),)),
    'edge-n3-normal': ('refused', 'btS', ((3, 3, ((3, 3),), False),)),
    'edge-n3-ints': ('taken', 'btS', ((3, 3, ((3, 3),), False),)),
    'edge-n4-normal': ('refused', 'bTs', ((4, 4, ((4, 4),), False),)),
    'edge-n4-ints': ('taken', 'bTs', ((4, 4, ((4, 4),), False),)),
    'edge-n5-normal': ('refused', 'bTS', ((5, 5, ((5, 5),), False),)),
    'edge-n5-ints': ('taken', 'bTS', ((4, 5, ((5, 4),), False),)),
    'edge-n6-normal': ('refused', 'bTS', ((6, 6, ((6, 6),), False),)),
    'edge-n6-ints': ('taken', 'bTS', ((5, 6, ((6, 5),), False),)),
    'edge-n7-normal': ('refused', 'bTS', ((7, 7, ((7, 7),), False),)),
    'edge-n7-ints': ('taken', 'bTS', ((4, 7, ((7, 4),), False),)),
    'edge-lone1e-45': ('refused', 'bTS', ((11, 13, ((8, 8), (5, 3)), False),)),
    'edge-lone2047.5': ('refused', 'bTS', ((11, 13, ((8, 8), (5, 4)), True),)),
    'edge-lone-1e-45': ('refused', 'bTS', ((11, 13, ((8, 8), (5, 3)), False),)),
    'edge-negzeros': ('taken', 'bTS', ((1, 1, ((1, 1),), False),)),
}


def _print_claims():
    import select_ref as R
    print("CLAIMS = {")
    for c in CASES:
        b, t, s = R.loops(c.planes[0].size, c.grid_cap)
        loops = ("B" if b else "b") + ("T" if t else "t") + ("S" if s else "s")
        if all(R.small_int_plane(p) for p in c.planes):
            fast = "taken"
        else:
            fast = "refused" + (c.name[c.name.index("@"):] if "@" in c.name else "")
        per = []
        for p, r in zip(c.planes, c.ranks):
            n1, n2 = R.ndp(p, r)
            bt = R.pass2_batches(p, r)
            p1s = [x for _, _, ps in bt for x in ps]
            per.append((n1, n2, tuple((np_, k1) for np_, k1, _ in bt), len(p1s) != len(set(p1s))))
        print(f"    {c.name!r}: ({fast!r}, {loops!r}, {tuple(per)!r}),")
    print("}")


if __name__ == "__main__":
    _print_claims()

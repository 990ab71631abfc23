"""Floating-point extremes on the CPU: the C oracle (oracle/orc.py) against the independent restatement (oracle/pyref.py)
on subnormal, huge, zero and signed-zero inputs, byte for byte (two NaNs count as equal).  This pins the reference side
before tests/test_gpu_fp_extremes.py compares the GPU with it."""
import numpy as np
import pytest

from oracle import orc, pyref

DTYPES = [np.float32, np.float64]


def same(a, b) -> bool:
    """byte equality, except that two NaNs are equal whatever their sign and payload"""
    a = np.atleast_1d(np.asarray(a))
    b = np.atleast_1d(np.asarray(b, dtype=a.dtype))
    if a.shape != b.shape:
        return False
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn)) and a[~an].tobytes() == b[~bn].tobytes()


def special(ft):
    """named magnitudes of the dtype: smallest subnormal, smallest normal, largest finite, and powers of two whose squares
    overflow (h), are subnormal (s) or round to zero (q)"""
    fi = np.finfo(ft)
    two = ft(2.0)
    return dict(sub=fi.smallest_subnormal, mn=fi.tiny, mx=fi.max, h=two ** (fi.maxexp // 2),
                s=two ** (fi.minexp // 2 - 2), q=two ** ((fi.minexp - fi.nmant) // 2 - 1))


def ray_new_dirs(ft):
    v = special(ft)
    sub, mn, mx, h, s, q = v["sub"], v["mn"], v["mx"], v["h"], v["s"], v["q"]
    return [[sub, 0, 0], [sub, sub, -sub], [-sub, 0, sub], [mn, -mn, mn], [s, s, -s], [s, 0, 0], [q, 0, 0], [q, q, q],
            [h, 0, 0], [h, h, 0], [-h, h, h], [mx, mx, mx], [mx, 0, 0], [0, 0, 0], [-0.0, -0.0, -0.0], [-0.0, 1, 0],
            [0, -0.0, -1], [1, -0.0, -0.0], [-4 * mn, sub, 0], [1, 1, 1], [3, -4, 12], [1, q, -q], [1, h, 0]]


def _py(ray):
    return ray["o"], ray["d"], ray["inv"]


# ---- Ray::new -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ray_new_extreme_directions(dtype):
    dirs = np.array(ray_new_dirs(dtype), dtype=dtype)
    origins = np.zeros_like(dirs)
    origins[::2] = np.array([-0.0, 0.0, 1.0], dtype=dtype)
    rays = orc.make_rays(origins, dirs, dtype)
    for i, (o, d) in enumerate(zip(origins, dirs)):
        po, pd, pinv = pyref.ray_new(o, d, dtype)
        assert same(rays[i]["o"], po) and same(rays[i]["d"], pd) and same(rays[i]["inv"], pinv), (i, d, rays[i], pd, pinv)
    inv = rays["inv"]
    assert np.isnan(inv).any() and np.isinf(inv).any() and (np.isfinite(inv) & (np.abs(inv) != 1)).any()
    # -0 components give -inf inverses: the sign of a zero reaches inv_direction
    assert (inv == -np.inf).any() and (inv == np.inf).any()


# ---- slab test and t-slice ------------------------------------------------------------------------------------------------------
def _raw_ray(o, inv, dtype):
    """a caller-built ray (Ray's fields are public): inv is stored as given, not 1/d"""
    r = np.zeros(1, dtype=orc.RAY_F32 if dtype == np.float32 else orc.RAY_F64)
    r["o"] = np.asarray(o, dtype=dtype)
    inv = np.asarray(inv, dtype=dtype)
    with np.errstate(all="ignore"):
        r["d"] = np.where(inv == 0, dtype(1), dtype(1) / inv)
    r["inv"] = inv
    return r[0]


def _slab_cases(dtype, n, seed):
    v = special(dtype)
    sub, mn, mx = v["sub"], v["mn"], v["mx"]
    big = dtype(2.0) ** (104 if dtype == np.float32 else 1000)
    ovals = [0.0, -0.0, 0.25, -0.5, 1.0, -mx, mx, sub, -sub, mn, big, -big, 3.0]
    ivals = [1.0, -1.0, 0.5, -3.0, 0.0, -0.0, np.inf, -np.inf, sub, -sub, mx, -mx, 2.0 ** -100, 7.0]
    boxes1 = [(-0.0, 0.0), (-0.0, -0.0), (0.0, 0.0), (0.0, -0.0), (1.0, 2.0), (-2.0, -1.0), (-mx, mx), (sub, 2 * sub),
              (big, big), (-1.0, 1.0), (0.25, 0.25), (-np.inf, np.inf), (mn, 4 * mn)]
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        o = [ovals[i] for i in rng.integers(0, len(ovals), 3)]
        inv = [ivals[i] for i in rng.integers(0, len(ivals), 3)]
        b = [boxes1[i] for i in rng.integers(0, len(boxes1), 3)]
        cases.append((o, inv, [b[0][0], b[1][0], b[2][0], b[0][1], b[1][1], b[2][1]]))
    # pinned: the flat box at the origin's plane (l = -0, h = +0) in each axis, both directions, both origin signs
    for ax in range(3):
        for sgn in (1.0, -1.0):
            for oz in (0.0, -0.0):
                o = [0.25, 0.25, 0.25]; o[ax] = oz
                inv = [np.inf, np.inf, np.inf]; inv[ax] = sgn
                box = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]; box[ax] = -0.0; box[3 + ax] = 0.0
                cases.append((o, inv, box))
                box2 = list(box); box2[3 + ax] = -0.0
                cases.append((o, inv, box2))
    # pinned: inv = 0 with an origin so far from the box that b - o rounds to +inf (inf * 0 = NaN: a miss)
    cases.append(([-mx, 0.25, 0.25], [0.0, 1.0, 1.0], [big, 0.0, 0.0, big, 1.0, 1.0]))
    cases.append(([mx, 0.25, 0.25], [-0.0, 1.0, 1.0], [-big, 0.0, 0.0, -big, 1.0, 1.0]))
    return cases


@pytest.mark.parametrize("dtype", DTYPES)
def test_slab_hit_and_slice_agree_on_extremes(dtype):
    cases = _slab_cases(dtype, 4000, seed=3 if dtype == np.float32 else 4)
    hits = misses = neg_zero_tmax = zero_slices = 0
    for o, inv, box in cases:
        r = _raw_ray(o, inv, dtype)
        box = np.asarray(box, dtype=dtype)
        h = orc.ray_intersects_aabb(r, box)
        assert h == pyref.ray_hit(_py(r), box), (o, inv, box)
        cs, ps = orc.ray_slice(r, box), pyref.ray_slice(_py(r), box)
        assert (cs is None) == (ps is None), (o, inv, box, cs, ps)
        if cs is not None:
            assert same(np.array(cs, dtype=dtype), np.array(ps, dtype=dtype)), (o, inv, box, cs, ps)
            assert not np.signbit(cs[0])                                         # fast_max(x, 0) never returns -0
            neg_zero_tmax += int(cs[1] == 0 and np.signbit(cs[1]))
            zero_slices += int(cs[0] == 0 and cs[1] == 0)
        hits += int(h)
        misses += int(not h)
    assert hits > 300 and misses > 300, (hits, misses)
    assert neg_zero_tmax >= 6 and zero_slices >= 12, (neg_zero_tmax, zero_slices)


@pytest.mark.parametrize("dtype", DTYPES)
def test_slice_zero_signs_pinned(dtype):
    """the flat box [-0, +0] on x and a +x ray from x = +0: inf_sup gives (-0, +0), so the slice is (+0, +0); a box
    [-0, -0] gives (+0, -0)"""
    r = orc.make_rays([[0.0, 0.0, 0.0]], [[1.0, 0.0, 0.0]], dtype)[0]
    box = np.array([-0.0, -1.0, -1.0, 0.0, 1.0, 1.0], dtype=dtype)
    for got in (orc.ray_slice(r, box), pyref.ray_slice(_py(r), box)):
        assert np.array(got, dtype=dtype).tobytes() == np.array([0.0, 0.0], dtype=dtype).tobytes(), got
    box[3] = -0.0
    for got in (orc.ray_slice(r, box), pyref.ray_slice(_py(r), box)):
        assert np.array(got, dtype=dtype).tobytes() == np.array([0.0, -0.0], dtype=dtype).tobytes(), got


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_inv_overflow_is_a_miss(dtype):
    """o.x = -MAX, inv.x = 0 and a box far on +x: (b - o) rounds to +inf and inf * 0 is NaN, which the reference turns into a
    miss; IEEE minNum/maxNum would drop the NaN and let the y and z slabs report a hit"""
    big = dtype(2.0) ** (104 if dtype == np.float32 else 1000)
    r = _raw_ray([-np.finfo(dtype).max, 0.25, 0.25], [0.0, 1.0, 1.0], dtype)
    box = np.array([big, 0.0, 0.0, big, 1.0, 1.0], dtype=dtype)
    with np.errstate(all="ignore"):
        assert np.isnan((box[0] - r["o"][0]) * r["inv"][0])
    assert not orc.ray_intersects_aabb(r, box) and not pyref.ray_hit(_py(r), box)
    assert orc.ray_slice(r, box) is None and pyref.ray_slice(_py(r), box) is None
    box[0] = box[3] = dtype(0.5)                                                 # a box near the origin: b - o stays finite, a hit
    assert orc.ray_intersects_aabb(r, box) and pyref.ray_hit(_py(r), box)


# ---- triangles --------------------------------------------------------------------------------------------------------------
def degenerate_triangles(dtype):
    """a regular triangle and degenerate ones: two or three coincident vertices, collinear vertices in every order"""
    a, b, c = np.array([0.0, 0.0, 0.0]), np.array([4.0, 0.0, 0.0]), np.array([0.0, 4.0, 0.0])
    m = np.array([2.0, 2.0, 0.0])
    tris = [(a, b, c), (a, a, c), (a, b, b), (c, b, c), (a, a, a), (a, m, c * 0.5 + b * 0.5), (a, b, 0.5 * b),
            (0.5 * b, a, b), (b, 0.5 * b, a), (a, b, -b)]
    return np.array([np.stack(t) for t in tris], dtype=np.float64)


def voronoi_points(tri):
    """points around a triangle in every region: near each vertex, past each edge, inside, above and below, far away"""
    a, b, c = tri
    pts = []
    for s in (-1.0, -0.25, 0.0, 0.2, 0.5, 1.0, 1.5):
        for t in (-1.0, -0.25, 0.0, 0.3, 0.5, 1.0, 1.5):
            for hgt in (0.0, 1.0, -2.0):
                pts.append(a + s * (b - a) + t * (c - a) + np.array([0.3 * hgt, -0.2 * hgt, hgt]))
    pts += [a, b, c, (a + b + c) / 3.0, np.array([-5.0, 7.0, 3.0])]
    return np.array(pts)


# scales 2^k of the triangle checks (coordinates up to 7 · 2^k)
F32_SCALES = [-150, -130, -126, -100, 0, 60, 100, 120]
F64_SCALES = [-1070, -1030, -1022, -600, 0, 500, 1000, 1018]
# scales of the cube scenes (coordinates up to 1e5 · 2^k): every coordinate subnormal, straddling the smallest normal,
# surface areas overflowing in the top levels only / in every level above the cubes, and the root's centroid extent overflowing
BANDS = {np.float32: dict(subnormal=-150, straddle=-138, others=[-126, -100, 0], sa_overflow=[60, 100], overflow=111),
         np.float64: dict(subnormal=-1070, straddle=-1030, others=[-1022, -600, 0], sa_overflow=[500, 1000], overflow=1007)}


def band_scales(dtype):
    b = BANDS[dtype]
    return [b["subnormal"], b["straddle"]] + b["others"] + b["sa_overflow"] + [b["overflow"]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_triangle_distance_and_intersection_on_degenerate_and_scaled(dtype):
    finite_hits = inf_hits = 0
    for k in (F32_SCALES if dtype == np.float32 else F64_SCALES):
        sc = 2.0 ** k
        for t64 in degenerate_triangles(dtype):
            tri = (t64 * sc).astype(dtype)
            for p64 in voronoi_points(t64):
                p = (p64 * sc).astype(dtype)
                assert same(orc.triangle_dist2(tri, p, dtype), pyref.triangle_dist2(tri, p, dtype)), (k, tri, p)
            # rays from above and below the triangle's plane through a point of every region (Möller–Trumbore)
            for p64 in voronoi_points(t64)[::3]:
                for oz in (3.0, -3.0):
                    o = (np.array([p64[0], p64[1], oz]) * sc).astype(dtype)
                    r = orc.make_rays([o], [[0.0, 0.0, -oz]], dtype)[0]
                    want = orc.ray_triangle(r, tri[0], tri[1], tri[2])
                    got = pyref.ray_triangle(_py(r), tri[0], tri[1], tri[2])
                    assert same(np.array(want, dtype=dtype), np.array(got, dtype=dtype)), (k, tri, o, want, got)
                    finite_hits += int(np.isfinite(want[0]))
                    inf_hits += int(not np.isfinite(want[0]))
    assert finite_hits >= 10 and inf_hits > 50, (finite_hits, inf_hits)


# ---- build + flatten on scaled scenes ----------------------------------------------------------------------------------------
def scaled_scene(k, dtype, n_cubes=6):
    """cubes of the benchmark generator (coordinates up to 1e5) scaled by 2^k in f64, plus three degenerate triangles"""
    tris, _ = orc.create_n_cubes(n_cubes)
    t = tris.astype(np.float64)
    t = np.concatenate([t, degenerate_triangles(dtype)[[1, 4, 5]] * 1000.0])
    t = (t * 2.0 ** k).astype(dtype)
    aabbs = np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1)
    return t, aabbs


def root_centroid_extent_overflows(aabbs) -> bool:
    with np.errstate(all="ignore"):
        c = aabbs[:, :3] * aabbs.dtype.type(0.5) + aabbs[:, 3:] * aabbs.dtype.type(0.5)
        ext = c.max(axis=0) - c.min(axis=0)
    return bool(np.isinf(ext).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_build_and_flatten_on_scaled_scenes(dtype):
    accepted = []
    for k in band_scales(dtype):
        _, aabbs = scaled_scene(k, dtype)
        if root_centroid_extent_overflows(aabbs):
            continue                                                     # the reference panics there (no oracle call)
        accepted.append(k)
        tree = orc.build(aabbs)
        py_nodes, py_sn = pyref.build(aabbs)
        assert len(tree.nodes) == len(py_nodes)
        for cn, pn in zip(tree.nodes, py_nodes):
            assert cn["parent"] == pn["parent"]
            if pn["leaf"]:
                assert cn["shape"] == pn["shape"]
            else:
                assert cn["l"] == pn["l"] and cn["r"] == pn["r"], k
                assert np.concatenate([cn["l_min"], cn["l_max"]]).tobytes() == np.asarray(pn["l_aabb"], dtype=dtype).tobytes(), k
                assert np.concatenate([cn["r_min"], cn["r_max"]]).tobytes() == np.asarray(pn["r_aabb"], dtype=dtype).tobytes(), k
        assert tree.shape_node.tolist() == py_sn
        flat = orc.flatten(tree.nodes)
        py_flat = pyref.flatten(py_nodes, dtype)
        assert len(flat) == len(py_flat)
        for cf, pf in zip(flat, py_flat):
            assert (cf["entry"], cf["exit"], cf["shape"]) == pf[1:]
            assert np.concatenate([cf["min"], cf["max"]]).tobytes() == np.asarray(pf[0], dtype=dtype).tobytes(), k
    assert accepted == band_scales(dtype)[:-1], accepted                  # every band but the overflowing extent is built


@pytest.mark.parametrize("dtype", DTYPES)
def test_scaled_scene_bands(dtype):
    """the scales reach the bands they are named for"""
    fi = np.finfo(dtype)
    b = BANDS[dtype]
    _, tiny = scaled_scene(b["subnormal"], dtype)
    assert np.all(np.abs(tiny) < fi.tiny) and (tiny != 0).any()                     # every coordinate subnormal
    _, straddle = scaled_scene(b["straddle"], dtype)
    nz = np.abs(straddle[straddle != 0])
    assert (nz < fi.tiny).any() and (nz >= fi.tiny).any()                           # both sides of the smallest normal
    for k in b["sa_overflow"]:
        _, sa = scaled_scene(k, dtype)
        with np.errstate(over="ignore"):
            ext = sa[:, 3:].max(axis=0) - sa[:, :3].min(axis=0)
            assert np.isinf(dtype(2) * (ext * ext).sum()) and not root_centroid_extent_overflows(sa)
            small = sa[:-3, 3:] - sa[:-3, :3]
            if k == b["sa_overflow"][0]:                                        # the cubes' own areas stay finite
                assert np.isfinite(dtype(2) * (small * small).sum(axis=1)).all()
    _, over = scaled_scene(b["overflow"], dtype)
    assert np.isfinite(over).all() and root_centroid_extent_overflows(over)

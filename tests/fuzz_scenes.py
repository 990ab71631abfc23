"""The random scenes of the two fuzz tests, and what the second one adds to them; not a test file.

`draw` is the scene draw of tests/test_gpu_parity.py::test_fuzz_all_queries — shapes, rays, points, queries — as a function of
(seed, dtype, kind, k_scale), so that the combination no longer has to follow from the seed: `historic` is the old map (8 of the 32
combinations, whatever the number of seeds), `combo` one that reaches all 32.  `with_whole_duplicates` and `extras` are what
tests/test_gpu_fuzz_queries.py needs beyond that — identical shapes, spheres, segment ends, k, distance limits — each from a generator of
its own, so that the old stream is never disturbed.  `case` puts a seed's scene, the oracle's arrays and every family's records together
once; tests/test_fuzz_queries_cpu.py asserts on exactly these what the default seeds contain."""
import functools

import numpy as np

import knn_ref as kr
from oracle import orc
from sphere_ref import list_hits

NONE = 0xFFFFFFFF
KINDS = ("spread", "clustered", "grid", "duplicated")
SCALES = ("1", "subnormal", "overflow", "2^-20")
LEAVES = ("box", "triangle", "sphere")
TMAX_PINS = ("nan", "zero", "minus_one", "inf", "first", "later")
LIMIT_PINS = ("zero", "minus_one", "nan", "inf")
SPHERE_FACTORS = (0.25, 0.5, 1.0)
SPHERE_ODDITIES = ("r_zero", "r_negative", "r_nan", "r_inf", "r_tenfold")
DEFAULT_SEEDS = 16       # of tests/test_gpu_fuzz_queries.py (BVH_FUZZ_SEEDS overrides it); tests/test_fuzz_queries_cpu.py proves these
SMALL_N = {15: 37}      # seed → a pinned shape count below 64 (rows of k = 64 end in padding): the default seeds draw none on their own


def k_scales(dtype):
    """the four scale bands as powers of two: 1, all-subnormal, surface areas overflow, 2^-20"""
    return (0, -140 if dtype == np.float32 else -1040, 70 if dtype == np.float32 else 520, -20)


def historic(seed):
    """(dtype, kind, k_scale) as test_fuzz_all_queries has always derived them: all three depend on seed % 8 alone"""
    dtype = np.float32 if seed % 2 == 0 else np.float64
    return dtype, seed % 4, k_scales(dtype)[(seed // 2) % 4]


def combo(seed):
    """(dtype, kind, k_scale): 16 consecutive seeds give every kind x scale pair and both dtypes for every kind and every scale, 32 give
    all 32 combinations"""
    j = seed % 16
    dtype = np.float32 if (j + j // 4 + seed // 16) % 2 == 0 else np.float64
    return dtype, j % 4, k_scales(dtype)[j // 4]


# (dtype, kind, index into k_scales): eight of the 24 combinations the historic map cannot reach — with its eight they cover every
# kind x scale, every kind x dtype and every scale x dtype pair
OTHER_COMBOS = [
    (np.float64, 0, 1), (np.float64, 0, 3), (np.float32, 1, 1), (np.float32, 1, 3),
    (np.float64, 2, 0), (np.float64, 2, 2), (np.float32, 3, 0), (np.float32, 3, 2),
]


def draw(seed, dtype, kind, k_scale, n_pin=None):
    """random scenes of random size and character (spread, clustered, grid-aligned with exact ties, duplicated anchors), random rays and
    points, scaled by 2^k_scale; a tenth of the rays are caller-built (inv = +-0, subnormal, huge, or not 1/d).  n_pin replaces the drawn
    shape count (the draw itself is still consumed)."""
    rng = np.random.default_rng(1000 + seed)
    sc = 2.0 ** k_scale
    n = int(rng.integers(1, 6000 if seed % 7 else 60000))
    if n_pin is not None:
        n = n_pin
    if kind == 0:
        a = rng.uniform(-50, 50, size=(n, 3))
    elif kind == 1:
        c = rng.uniform(-50, 50, size=(max(n // 40, 1), 3))
        a = c[rng.integers(0, len(c), n)] + rng.normal(scale=0.5, size=(n, 3))
    elif kind == 2:
        a = rng.integers(-8, 8, size=(n, 3)).astype(float)
    else:
        a = rng.uniform(-50, 50, size=(n, 3)); a[n // 3:] = a[: n - n // 3][rng.integers(0, max(n - n // 3, 1), n - n // 3)]
    a = a.astype(dtype).astype(np.float64)
    tri64 = np.stack([a, a + rng.uniform(0, 2, size=(n, 3)).astype(dtype), a + rng.uniform(0, 2, size=(n, 3)).astype(dtype)], axis=1)
    tri = (tri64 * sc).astype(dtype)
    aabbs = np.concatenate([tri.min(axis=1), tri.max(axis=1)], axis=1).astype(dtype)
    m = 120 if k_scale < -100 else 1500                # (x86 arithmetic on subnormals is slow: the oracle's share of the time)
    o64 = rng.uniform(-60, 60, size=(m, 3))
    o = (o64 * sc).astype(dtype)
    d = (tri64[rng.integers(0, n, m)].mean(axis=1) - o64).astype(dtype)
    d[: m // 5] = rng.normal(size=(m // 5, 3))
    d[m // 5: m // 4] = rng.integers(-1, 2, size=(m // 4 - m // 5, 3)); d[np.all(d == 0, axis=1)] = [1, 0, 0]
    rays = orc.make_rays(o, d, dtype)
    cb = rng.random(m) < 0.1                            # caller-built rays: Ray's fields are public
    fi = np.finfo(dtype)
    pick = np.array([0.0, -0.0, fi.smallest_subnormal, fi.max, 0.5, 3.0])[rng.integers(0, 6, size=(m, 3))]
    keep = rng.random((m, 3)) < 0.5
    with np.errstate(over="ignore", invalid="ignore"):
        inv_cb = np.where(keep, rays["inv"].astype(np.float64), np.where(pick < 1.0, pick, pick * rays["inv"]))
        rays["inv"][cb] = inv_cb[cb].astype(dtype)
    pts = (rng.uniform(-60, 60, size=(800 if m == 1500 else 60, 3)) * sc).astype(dtype)
    tmax_u = rng.uniform(0.3, 1.7, size=m)              # any hit: segment ends around the nearest hit, as a factor of its distance
    cq = (a[rng.integers(0, n, 150)] + rng.normal(size=(150, 3)))   # AABB / point / ball queries around random shapes
    e = rng.uniform(0, 3, size=(150, 3))
    return dict(seed=seed, dtype=dtype, kind=kind, k_scale=k_scale, sc=sc, n=n, m=m, a=a, tri64=tri64, tri=tri, aabbs=aabbs, rays=rays,
                pts=pts, tmax_u=tmax_u, cq=cq, e=e)


def with_whole_duplicates(scene, seed):
    """kinds 2 and 3 only: a third of the shapes become exact copies — all three vertices — of a randomly chosen shape among the others,
    and the boxes are taken again.  The draw alone never makes two shapes equal (kind 3 repeats anchors only), so no two triangle or
    sphere records of a ray were ever equal."""
    if scene["kind"] not in (2, 3):
        return scene
    rng = np.random.default_rng(3000 + seed)
    n, dtype = scene["n"], scene["dtype"]
    perm = rng.permutation(n)
    dst, pool = perm[: n // 3], perm[n // 3:]
    src = pool[rng.integers(0, len(pool), size=len(dst))]
    a, tri64 = scene["a"].copy(), scene["tri64"].copy()
    a[dst], tri64[dst] = a[src], tri64[src]
    tri = (tri64 * scene["sc"]).astype(dtype)
    aabbs = np.concatenate([tri.min(axis=1), tri.max(axis=1)], axis=1).astype(dtype)
    return dict(scene, a=a, tri64=tri64, tri=tri, aabbs=aabbs)


def _row_of(off):
    counts = np.diff(off.astype(np.int64))
    return counts, np.repeat(np.arange(len(counts)), counts)


def _row_min(off, dist):
    """the smallest distance per row (+inf for an empty row or a row of misses)"""
    counts, _ = _row_of(off)
    out = np.full(len(counts), np.inf, dtype=dist.dtype)
    rows = counts > 0
    if rows.any():
        out[rows] = np.minimum.reduceat(dist, off[:-1].astype(np.int64)[rows])
    return out


def draw_spheres(rng, aabbs):
    """one sphere per shape at the centre of its box, r = half the largest extent x one of SPHERE_FACTORS; about 3 % are SPHERE_ODDITIES.
    Factor and oddity are drawn per distinct box, so identical shapes get identical spheres.  → (spheres[n, 4], oddity[n]: -1 or the
    index into SPHERE_ODDITIES)"""
    dtype = aabbs.dtype.type
    b = aabbs.astype(np.float64)
    _, inverse = np.unique(aabbs, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    groups = int(inverse.max()) + 1
    factor = np.asarray(SPHERE_FACTORS)[rng.integers(0, len(SPHERE_FACTORS), size=groups)][inverse]
    odd = np.where(rng.random(groups) < 0.03, rng.integers(0, len(SPHERE_ODDITIES), size=groups), -1)[inverse]
    c = (b[:, :3] + b[:, 3:]) * 0.5
    r = (b[:, 3:] - b[:, :3]).max(axis=1) * 0.5 * factor
    r = np.select([odd == 0, odd == 1, odd == 2, odd == 3, odd == 4], [0.0, -r, np.nan, np.inf, 10.0 * r], r)
    with np.errstate(over="ignore"):
        return np.concatenate([c, r[:, None]], axis=1).astype(dtype), odd


def draw_tmax(rng, off, dist, miss_span, dtype):
    """per ray the nearest distance of `dist` x U(0.3, 1.7) (miss_span where the row has no candidate), the convention of the families'
    own tmax draws; then a quarter of the rays that have candidates are pinned, in turn, to NaN, 0, -1, +inf, exactly the distance of the
    row's first candidate and exactly that of a later one (the first one's where there is no other).  → (tmax[n], {pin name: rays})"""
    c = _row_min(off, dist).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        tmax = (np.where(np.isfinite(c), c, miss_span) * rng.uniform(0.3, 1.7, size=len(c))).astype(dtype)
    have = np.nonzero(np.isfinite(c))[0]
    chosen = have[rng.permutation(len(have))[: (len(have) + 3) // 4]]
    later_u = rng.random(len(chosen))
    pins = {name: [] for name in TMAX_PINS}
    o = off.astype(np.int64)
    for j, r in enumerate(chosen):
        name = TMAX_PINS[j % len(TMAX_PINS)]
        finite = dist[o[r]:o[r + 1]]
        finite = finite[np.isfinite(finite)]
        if name == "later" and len(finite) < 2:
            name = "first"
        if name == "first":
            tmax[r] = finite[0]
        elif name == "later":
            tmax[r] = finite[1 + int(later_u[j] * (len(finite) - 1))]
        else:
            tmax[r] = dict(nan=np.nan, zero=0.0, minus_one=-1.0, inf=np.inf)[name]
        pins[name].append(int(r))
    return tmax, {name: np.asarray(rows, dtype=np.int64) for name, rows in pins.items()}


def draw_limits(rng, kth, miss_span, dtype):
    """per point the k-th nearest distance x U(0.3, 1.7); a fifth of the points (one at least) are pinned, in turn, to 0, -1, NaN and +inf"""
    c = kth.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        m = (np.where(np.isfinite(c), c, miss_span) * rng.uniform(0.3, 1.7, size=len(c))).astype(dtype)
    chosen = rng.permutation(len(c))[: max(len(c) // 5, 1)]
    first = int(rng.integers(0, len(LIMIT_PINS)))                 # (which pin a scene of few points gets is drawn too)
    pins = {name: chosen[(j - first) % len(LIMIT_PINS)::len(LIMIT_PINS)] for j, name in enumerate(LIMIT_PINS)}
    for name, value in zip(LIMIT_PINS, (0.0, -1.0, np.nan, np.inf)):
        m[pins[name]] = value
    return m, pins


def extras(scene, seed, oracle):
    """what the families added after the first fuzz need, from default_rng(2000 + seed).  oracle: dict(oflat, off, idx, box, triangle) —
    the flat array, FlatBvh::traverse's CSR of the scene's rays, its t-slices and the triangle stage's records.
    → dict(spheres, oddity, sphere: list_hits' records, ks, tmax / tmax_pins per leaf, kpts, and per shape distance (0: the shape's box,
    1: its triangle) knn_flat: {k: knn_ref.knearest's rows} (the limits are drawn around them), max_dist, limit_pins)"""
    rng = np.random.default_rng(2000 + seed)
    dtype, sc, n = scene["dtype"], scene["sc"], scene["n"]
    spheres, oddity = draw_spheres(rng, scene["aabbs"])
    records = dict(box=oracle["box"], triangle=oracle["triangle"], sphere=list_hits(oracle["off"], oracle["idx"], scene["rays"], spheres))
    ks = (1, int(rng.integers(2, 64)), 64)
    tmax, tmax_pins = {}, {}
    for leaf in LEAVES:
        tmax[leaf], tmax_pins[leaf] = draw_tmax(rng, oracle["off"], records[leaf][:, 0], 200.0 * sc, dtype)
    # points of the k-nearest families: the scene's own (anywhere in the ray origins' cube), beside shapes, and on shape vertices
    # (distance 0 to that shape and to every copy of it).  Their number follows the cost of the Python references, which compute every
    # shape's distance per point: at most 250 000 point x shape pairs per scene
    count = max(8, min(100 if scene["m"] == 1500 else 40, 250000 // n))
    near = (scene["a"][rng.integers(0, n, size=2 * count // 5)] + rng.normal(size=(2 * count // 5, 3))) * sc
    on = scene["tri64"][rng.integers(0, n, size=count // 5), rng.integers(0, 3, size=count // 5)] * sc
    kpts = np.concatenate([scene["pts"][: count - len(near) - len(on)], near.astype(dtype), on.astype(dtype)])
    knn_flat, max_dist, limit_pins = {}, {}, {}
    for kind in (0, 1):
        knn_flat[kind] = kr.knearest(oracle["oflat"], scene["aabbs"], kpts, ks, scene["tri"] if kind else None)
        kth = knn_flat[kind][ks[1]][1][:, min(ks[1], n) - 1]
        max_dist[kind], limit_pins[kind] = draw_limits(rng, kth, 200.0 * sc, dtype)
    return dict(spheres=spheres, oddity=oddity, sphere=records["sphere"], ks=ks, tmax=tmax, tmax_pins=tmax_pins, kpts=kpts,
                knn_flat=knn_flat, max_dist=max_dist, limit_pins=limit_pins)


def has_empty_child_bounds(oflat):
    """a split without SAH winner left EMPTY bounds (+inf / -inf) on a navigator entry: the wide walk does not take such a tree"""
    nav = oflat["entry"] != NONE
    return bool(np.isposinf(oflat["min"][nav]).all(axis=1).any())


@functools.lru_cache(maxsize=32)
def case(seed):
    """seed → the scene of combo(seed) with whole duplicates, the oracle's arrays on it and the extras: dict(scene, nodes, shape_node,
    oflat, off, idx, records {leaf: [total, W]}, extras, wide_eligible)"""
    scene = with_whole_duplicates(draw(seed, *combo(seed), n_pin=SMALL_N.get(seed)), seed)
    ot = orc.build(scene["aabbs"])
    oflat = orc.flatten(ot.nodes)
    off, idx, ts, _ = orc.traverse_flat(oflat, scene["aabbs"], scene["rays"], want_t=True, threads=orc.max_threads())
    isect, _, _ = orc.triangle_stage(scene["tri"], scene["rays"], off, idx)
    ex = extras(scene, seed, dict(oflat=oflat, off=off, idx=idx, box=ts, triangle=isect))
    return dict(scene=scene, nodes=ot.nodes, shape_node=ot.shape_node, oflat=oflat, off=off, idx=idx,
                records=dict(box=ts, triangle=isect, sphere=ex["sphere"]), extras=ex, wide_eligible=not has_empty_child_bounds(oflat))


@functools.lru_cache(maxsize=32)
def knn_rows(seed):
    """the rows of the two k-nearest families for case(seed)'s points, per shape distance (0: box, 1: triangle):
    dict(flat={kind: {k: (shape, dist)}}, tree={kind: {"none" | "limit": {k: (shape, dist)}}})"""
    import knn_tree_ref as ktr
    c = case(seed)
    scene, ex = c["scene"], c["extras"]
    tree = {}
    for kind in (0, 1):
        tris = scene["tri"] if kind else None
        rows = ktr.knearest_tree_limits(c["nodes"], scene["aabbs"], ex["kpts"], ex["ks"], tris, (None, ex["max_dist"][kind]))
        tree[kind] = dict(none=rows[0], limit=rows[1])
    return dict(flat=ex["knn_flat"], tree=tree)


def label(seed):
    dtype, kind, k_scale = combo(seed)
    return f"seed {seed}: {'f32' if dtype == np.float32 else 'f64'}, {KINDS[kind]}, 2^{k_scale}"

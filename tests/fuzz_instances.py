"""The random instanced scenes of tests/test_gpu_fuzz_instances.py; not a test file.

`case(seed)` draws, as a pure function of the seed, a set of member trees, two poses of n instances of them, rays with segment ends, points
with limits, k and regions, and computes every instanced family's reference answer on them (tests/instances_*_ref.py over the oracle).
`combo(seed)` maps 16 consecutive seeds onto both dtypes x four scene characters:
  posed       test_instances_cpu.transforms, the translations spread with n^(1/3)
  lattice     signed permutations (with signed zeros) x powers of two, integer translations, half of the instances whole duplicates, half of the rays on the
              integer grid: every transform operation is exact — ties across instances, d'[k] == +-0, world rays that are not finite
  scaled      members stored at 2^e and 2^-e whose instances carry the compensating scale: Y_i and the object frames span 2^+-e
  degenerate  posed, with a tenth of the instances of rank 2, rank 1, rank 0, or scaled by 2^+-70 (2^+-520 in f64): cofactors that
              overflow and underflow, inverses that hold inf and NaN; no NaN or infinity is put INTO a transform
Every ingredient draws from a generator of its own (default_rng(BASE + seed)), so that adding one never disturbs the others.
tests/test_fuzz_instances_cpu.py asserts on exactly these cases what the default seeds contain."""
import copy
import functools
import time

import numpy as np

import fuzz_scenes as fs
import instances_knn_ref as iknn
import instances_ref as ir
import instances_region_ref as irr
import instances_within_ref as iwr
from oracle import orc
from test_instances_cpu import SPREAD, transforms

NONE = 0xFFFFFFFF
KINDS = ("posed", "lattice", "scaled", "degenerate")
DEGENERATE = ("rank2", "rank1", "zero", "huge", "tiny")
MEMBER_COUNTS = (1, 12, 240, 257, 700, 1100)
DEFAULT_SEEDS = 16      # of tests/test_gpu_fuzz_instances.py (BVH_FUZZ_SEEDS overrides it); tests/test_fuzz_instances_cpu.py proves these
# seed → a pinned instance count: one lane, the smallest top level, the wave tier's last and the workgroup tier's first size, one and two
# workgroups of k_instances_prep<T, 1> and three; seed 8 draws from 800 .. 1000 (the level tier builds its top level)
N_PINS = {0: 1, 1: 2, 2: 64, 3: 65, 6: 256, 4: 257, 5: 513}
LEVEL_TIER_SEED = 8
SMALL_SETS = (1,)       # seeds whose instances all copy the SMALLEST member: fewer than 64 pairs in all, so that rows of k = 64 end in padding
                        # (a lattice seed: its second instance duplicates the first, so a ray that hits has two candidates to pin tmax on)
PAIR_BUDGET = 1_000_000  # point x (instance, shape) pairs per scene: the cost of the Python references of the point families
MAX_POINTS, MIN_POINTS = 60, 16
PAIR_LIMIT = PAIR_BUDGET // MIN_POINTS   # pairs per scene at which 16 points spend the budget: draw_tree_of steers towards it
N_REGIONS = 24
DEGENERATE_SHIFT = 12.0
LATTICE_REACH = 2.0      # lattice translations are 4 x integers in +-ceil(this x growth(n))
EDGE = 0.8               # a random member's triangle edges are U(-EDGE, EDGE)^3: a ray meets a few boxes per instance, not dozens
HALF_SPACE_PAIRS = 20_000  # a one-plane region reports about half of the scene's pairs: drawn only where the scene has at most this many
PLANE_COUNTS = (1, 6, 8, 32)
ORDINARY = 1e6           # |coordinate| of a world box below which small_balls takes it (the 2^70 instances would blow the balls up)


def combo(seed):
    """(dtype, kind): 16 consecutive seeds give every kind four times, twice per dtype"""
    j = seed % 16
    dtype = np.float32 if (j + j // 4 + seed // 16) % 2 == 0 else np.float64
    return dtype, j % 4


def label(seed):
    dtype, kind = combo(seed)
    return f"seed {seed}: {'f32' if dtype == np.float32 else 'f64'}, {KINDS[kind]}"


def scale_exponent(dtype):
    """e of the `scaled` character"""
    return 20 if dtype == np.float32 else 200


def extreme_exponent(dtype):
    """the `huge` / `tiny` classes of the `degenerate` character: 3x3 part x 2^+-this"""
    return 70 if dtype == np.float32 else 520


def _tris_aabbs(tris):
    t = tris.reshape(-1, 3, 3)
    return np.ascontiguousarray(np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1))


def integer_cube(rng, first_octant):
    """the 12 triangles of an axis-aligned cube with integer corners inside [-3, 3]^3 (inside [0, 3]^3, touching x = 0, for the lattice's
    member 0), facing outwards"""
    size = int(rng.integers(1, 4))
    lo = rng.integers(0 if first_octant else -3, 4 - size, size=3).astype(np.float64)
    if first_octant:
        lo[0] = 0.0
    v = lo + size * np.array([[(c >> k) & 1 for k in range(3)] for c in range(8)], dtype=np.float64)
    faces = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    return np.stack([v[[a, b, c]] for q in faces for a, b, c in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])


# ---- members ----------------------------------------------------------------------------------------------------------------------------
def draw_members(seed, dtype, kind, n_instances):
    """2 .. 5 members: MEMBER_COUNTS[seed % 6], further listed counts at random, and one count from 2 .. 1100.  Small triangles anchored in
    about [-3, 3]^3; 12 and 240 are orc.create_n_cubes' cubes.  On the lattice they are cubes with integer corners, and the other members
    have integer anchors and half-integer edges; its member 0 lives in x >= 0 with one vertex at x = 0 exactly, so that a mirrored copy has a world box that ends at
    -0 / +0.  In a degenerate scene member 0 is moved by DEGENERATE_SHIFT on every axis: its bounds lie in a narrow cone off the origin, and it is the member the 2^70 class
    copies — a 2^70 copy of a member AROUND the origin has a world box that swallows every ray, one in a narrow cone takes those that point its way.  → ([(aabbs, tris)] in dtype, counts)"""
    rng = np.random.default_rng(11000 + seed)
    m = int(rng.integers(2, 6))
    counts = [MEMBER_COUNTS[seed % len(MEMBER_COUNTS)]] + [int(MEMBER_COUNTS[int(rng.integers(0, len(MEMBER_COUNTS)))]) for _ in range(m - 2)]
    drawn = int(rng.integers(2, 1101))
    counts.append(min(drawn, max(2, PAIR_LIMIT // n_instances)))    # (a set of many instances has a small member to be many instances OF)
    out = []
    for t, n in enumerate(counts):
        sub = np.random.default_rng([11500 + seed, t])
        if kind == 1 and n in (12, 240):
            tris = np.concatenate([integer_cube(sub, t == 0) for _ in range(n // 12)])
        elif kind == 1:
            a = sub.integers(-3, 4, size=(n, 3)).astype(np.float64)
            if t == 0:
                a[:, 0] = np.abs(a[:, 0]); a[0, 0] = 0.0
            e = sub.integers(0, 4, size=(n, 2, 3)) * 0.5
            if t == 0:
                e[0, :, 0] = [0.5, 1.0]
            tris = np.stack([a, a + e[:, 0], a + e[:, 1]], axis=1)
        elif n in (12, 240):
            small = np.array([-3.0] * 3 + [3.0] * 3, dtype=np.float32)
            tris = orc.create_n_cubes(n // 12, small)[0].astype(np.float64)
        else:
            a = sub.uniform(-3, 3, size=(n, 3))
            tris = np.stack([a, a + sub.uniform(-EDGE, EDGE, size=(n, 3)), a + sub.uniform(-EDGE, EDGE, size=(n, 3))], axis=1)
        if kind == 3 and t == 0:
            tris = tris + DEGENERATE_SHIFT
        tris = np.ascontiguousarray(tris.astype(dtype)).reshape(-1, 3, 3)
        out.append((_tris_aabbs(tris), tris))
    return out, counts


def draw_instance_count(seed, kind):
    rng = np.random.default_rng(12000 + seed)
    n = int(rng.integers(1, 601))
    high = int(rng.integers(800, 1001))
    if seed in N_PINS:
        return N_PINS[seed]
    if seed == LEVEL_TIER_SEED:
        return high
    return max(n, (1, 2, 1, 8)[kind])      # (a lattice has a duplicate, a degenerate set its four classes and ordinary instances beside them)


def draw_tree_of(seed, n, counts, kind):
    """random members, every member used once when n allows — the largest ones where it does not, the smallest one alone in a SMALL_SETS seed.
    Once the scene holds PAIR_LIMIT (instance, shape) pairs, every further instance copies the smallest member.  In a degenerate scene
    one instance in 25 (two at least) copies member 0."""
    rng = np.random.default_rng(13000 + seed)
    m = len(counts)
    of = rng.integers(0, m, size=n)
    by_size = np.argsort(-np.asarray(counts), kind="stable")
    first = by_size[-1:].repeat(n) if seed in SMALL_SETS else by_size[:min(n, m)]
    slots = rng.permutation(n)
    of[slots[:len(first)]] = first
    pairs = int(sum(counts[int(t)] for t in first))
    smallest = int(np.argmin(counts))
    for i in slots[len(first):]:
        if pairs + counts[int(of[i])] > PAIR_LIMIT:
            of[i] = smallest
        pairs += counts[int(of[i])]
    if kind == 3:
        of[slots[::-1][:max(2, n // 25)]] = 0
    return of.astype(np.uint32)


# ---- poses ------------------------------------------------------------------------------------------------------------------------------
def growth(n):
    """the factor on SPREAD: the cluster's volume follows the instance count, so that a ray meets a handful of world boxes, not all"""
    return max(1.0, (n / 37.0) ** (1.0 / 3.0))


def posed(n, dtype, rng_seed):
    x = transforms(n, dtype, rng_seed).astype(np.float64)
    x[:, :, 3] *= growth(n)
    return np.ascontiguousarray(x.astype(dtype))


def lattice(n, dtype, rng_seed, tree_of):
    """→ (x, tree_of): tree_of changes, since a whole duplicate copies its source's member too"""
    rng = np.random.default_rng(rng_seed)
    x = np.zeros((n, 3, 4))
    reach = int(np.ceil(LATTICE_REACH * growth(n)))
    for i in range(n):
        p = rng.permutation(3)
        s = rng.choice([-1.0, 1.0], size=3) * rng.choice([0.5, 1.0, 2.0], size=3)
        x[i, :, :3] = rng.choice([-0.0, 0.0], size=(3, 3), p=[0.7, 0.3])                                          # (signed zeros beside the permutation)
        for k in range(3):
            x[i, k, p[k]] = s[k]
        steps = np.where(rng.random(3) < 0.3, 0, rng.integers(0, reach + 1, size=3))
        x[i, :, 3] = rng.choice([-1.0, 1.0], size=3) * (steps * 4.0)                                  # (-0.0 occurs)
    of = np.array(tree_of, dtype=np.uint32)
    perm = rng.permutation(n)
    dst, pool = perm[: n // 2], perm[n // 2:]
    src = pool[rng.integers(0, len(pool), size=len(dst))]
    x[dst], of[dst] = x[src], of[src]
    return np.ascontiguousarray(x.astype(dtype)), of


def scaled_members(tree_of, m):
    """the two members with the most instances (the lower index on a draw): the first is stored x 2^e, the second x 2^-e"""
    return [int(t) for t in np.argsort(-np.bincount(tree_of, minlength=m), kind="stable")[:2]]


def scaled(n, dtype, rng_seed, tree_of, counts):
    """posed, and the instances of the two scaled members carry 2^-e and 2^e on their 3x3 part: exact"""
    x = posed(n, dtype, rng_seed)
    e = scale_exponent(dtype)
    for t, f in zip(scaled_members(tree_of, len(counts)), (2.0 ** -e, 2.0 ** e)):
        x[tree_of == t, :, :3] *= dtype(f)
    return x


def degenerate(n, dtype, rng_seed, tree_of):
    """posed, with max(4, n // 10) instances (never all of them) replaced, in turn, by the five classes; the 2^70 class takes instances
    of member 0 (draw_members), the others take the rest first → (x, klass[n]: -1 or the index into DEGENERATE)"""
    x = posed(n, dtype, rng_seed)
    rng = np.random.default_rng([rng_seed, 1])
    order = rng.permutation(n)
    of_zero = [int(i) for i in order if tree_of[i] == 0]
    others = [int(i) for i in order if tree_of[i] != 0]
    klass = np.full(n, -1)
    big = 2.0 ** extreme_exponent(dtype)
    for j in range(min(max(4, n // 10), n - 1)):
        c = j % len(DEGENERATE)
        pool = of_zero if c == 3 or not others else others
        if not pool:
            continue
        i = pool.pop()
        klass[i] = c
        col = int(rng.integers(0, 3))
        if c == 0:
            x[i, :, col] = 0
        elif c == 1:
            x[i, :, col] = 0
            x[i, (col + 1) % 3, :3] = x[i, (col + 2) % 3, :3]
        elif c == 2:
            x[i, :, :3] = 0
        elif c == 3:
            x[i, :, :3] *= dtype(big)
        else:
            x[i, :, :3] *= dtype(1.0 / big)
    return x, klass


def draw_pose(seed, which, dtype, kind, n, tree_of, counts):
    """pose `which` (0: create, 1: update) → (x, tree_of, klass or None); only the lattice touches tree_of, and only in pose 0"""
    rng_seed = 14000 + 1000 * which + seed
    if kind == 0:
        return posed(n, dtype, rng_seed), tree_of, None
    if kind == 1:
        x, of = lattice(n, dtype, rng_seed, tree_of)
        if which == 1:          # (update() takes transforms alone: the duplicates of pose 1 copy among instances of one member)
            rng = np.random.default_rng([rng_seed, 2])
            for t in np.unique(tree_of):
                idx = np.nonzero(tree_of == t)[0]
                dst = idx[rng.permutation(len(idx))[: len(idx) // 2]]
                rest = np.setdiff1d(idx, dst)
                x[dst] = x[rest[rng.integers(0, len(rest), size=len(dst))]]
            return x, tree_of, None
        return x, of, None
    if kind == 2:
        return scaled(n, dtype, rng_seed, tree_of, counts), tree_of, None
    x, klass = degenerate(n, dtype, rng_seed, tree_of)
    return x, tree_of, klass


# ---- rays -------------------------------------------------------------------------------------------------------------------------------
def draw_rays(seed, dtype, kind, x, wtris):
    """450 .. 700 rays, never a multiple of 64: aimed into the cluster as test_instances_cpu.cluster_rays does — a quarter of them at a
    point within 2.5 of an instance's translation, the others at a point of a world-space triangle (wtris: per instance its triangles
    under X_i), so that a set of two small instances is hit as often as a set of hundreds; a tenth in random directions, a tenth
    axis-parallel, a tenth caller-built (fuzz_scenes.draw's inv fields); on the lattice half of all rays have integer origins and
    directions in {-1, 0, 1}^3 \\ {0} and pass through the grid point next to a point of a triangle.  Shuffled, so that every 64-ray
    group mixes the kinds."""
    rng = np.random.default_rng(15000 + seed)
    m = int(rng.integers(450, 701))
    if m % 64 == 0:
        m += 1
    n = len(x)
    at = x[:, :, 3].astype(np.float64)
    reach = float(np.abs(at).max()) + 4
    o64 = rng.uniform(-(reach + 30), reach + 30, size=(m, 3))
    target = at[rng.integers(0, n, size=m)] + rng.uniform(-2.5, 2.5, size=(m, 3))
    on_triangle = np.zeros((m, 3))
    for j in range(m):
        tri = wtris[int(rng.integers(0, n))]
        b = rng.dirichlet([1.0, 1.0, 1.0])
        p = b @ tri[int(rng.integers(0, len(tri)))].astype(np.float64)
        on_triangle[j] = p if np.abs(p).max() < ORDINARY else target[j]
        if j % 4 != 3:
            target[j] = on_triangle[j]
    o = o64.astype(dtype)
    d = (target - o64).astype(dtype)
    t = m // 10
    d[:t] = rng.normal(size=(t, 3))
    axis = np.zeros((t, 3)); axis[np.arange(t), rng.integers(0, 3, size=t)] = rng.choice([-1.0, 1.0], size=t)
    d[t:2 * t] = axis
    o[t:2 * t] = np.where(axis != 0, -axis * (reach + 5), target[t:2 * t]).astype(dtype)    # (from outside, through the cluster)
    if kind == 1:
        h = m // 2
        gi = int(np.ceil(reach))
        di = rng.integers(-1, 2, size=(h, 3)).astype(np.float64)
        di[np.all(di == 0, axis=1)] = [0, 0, 1]
        oi = np.round(on_triangle[m - h:]) - di * (2 * gi + 8)   # through the grid point next to a point of a triangle, from outside the cluster
        o[m - h:], d[m - h:] = oi, di
    rays = orc.make_rays(o, d, dtype)
    cb = np.zeros(m, dtype=bool); cb[2 * t:3 * t] = True     # caller-built rays: Ray's fields are public
    fi = np.finfo(dtype)
    pick = np.array([0.0, -0.0, fi.smallest_subnormal, fi.max, 0.5, 3.0])[rng.integers(0, 6, size=(m, 3))]
    keep = rng.random((m, 3)) < 0.5
    with np.errstate(over="ignore", invalid="ignore"):
        inv_cb = np.where(keep, rays["inv"].astype(np.float64), np.where(pick < 1.0, pick, pick * rays["inv"]))
        rays["inv"][cb] = inv_cb[cb].astype(dtype)
    return np.ascontiguousarray(rays[rng.permutation(m)])


# ---- points -----------------------------------------------------------------------------------------------------------------------------
def draw_points(seed, sc, n_pairs):
    """scene-wide points, points beside transformed shapes and points exactly on world-space triangle vertices (distance 0 to that pair
    and to every duplicate of it); their number follows the cost of the Python references: PAIR_BUDGET point x pair products per scene"""
    rng = np.random.default_rng(16000 + seed)
    dtype = sc.ft
    n = len(sc.x)
    count = int(max(MIN_POINTS, min(MAX_POINTS, PAIR_BUDGET // max(n_pairs, 1))))
    reach = SPREAD * growth(n) + 3
    wt = iwr.world_triangles(sc)
    third = count // 3
    inst = rng.integers(0, n, size=2 * third)
    verts = np.stack([wt[i][int(rng.integers(0, len(wt[i]))), int(rng.integers(0, 3))] for i in inst]).astype(np.float64)
    ok = np.abs(verts).max(axis=1) < ORDINARY              # (a vertex of a 2^70 instance stays a point ON a vertex; beside it means nothing)
    near = np.where(ok[:third, None], verts[:third] + rng.normal(scale=0.5, size=(third, 3)), verts[:third])
    wide = rng.uniform(-reach, reach, size=(count - 2 * third, 3))
    return np.ascontiguousarray(np.concatenate([wide, near, verts[third:]]).astype(dtype))


# ---- regions ----------------------------------------------------------------------------------------------------------------------------
def draw_regions(seed, sc, n_pairs):
    rng = np.random.default_rng(17000 + seed)
    m = int(PLANE_COUNTS[int(rng.integers(0, len(PLANE_COUNTS)))])
    if m == 1 and n_pairs > HALF_SPACE_PAIRS:
        m = int(PLANE_COUNTS[1 + seed % 3])
    w = sc.w[np.abs(sc.w).max(axis=1) < ORDINARY]
    half = N_REGIONS // 2
    return np.ascontiguousarray(np.concatenate([irr.cutting_regions(sc, half, 17100 + seed, m),
                                                irr.small_balls(w, N_REGIONS - half, 17200 + seed, m)]).astype(sc.ft))


# ---- the case ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=32)
def case(seed):
    """seed → dict(seed, dtype, kind, trees, counts, uploaded (a member index or None), n, tree_of, x, x2, klass, klass2, scene, scene2,
    rays, free, cut, tmax, tmax_pins, points, limits, limit_pins, scalar_limit, scalar_points, ks, planes, and per pose the answers:
    free / cut = Scene.trace without / with tmax; within, within_scalar, knn {k: rows}; region; cut2, within2, knn2, region2; seconds)"""
    t0 = time.perf_counter()
    dtype, kind = combo(seed)
    n = draw_instance_count(seed, kind)
    trees, counts = draw_members(seed, dtype, kind, n)
    tree_of = draw_tree_of(seed, n, counts, kind)
    if kind == 2:
        e = scale_exponent(dtype)
        for t, f in zip(scaled_members(tree_of, len(counts)), (2.0 ** e, 2.0 ** -e)):
            tris = np.ascontiguousarray(trees[t][1] * dtype(f))
            trees[t] = (_tris_aabbs(tris), tris)
    x, tree_of, klass = draw_pose(seed, 0, dtype, kind, n, tree_of, counts)
    x2, _, klass2 = draw_pose(seed, 1, dtype, kind, n, tree_of, counts)
    sc = ir.Scene(trees, tree_of, x, dtype)
    sc2 = copy.copy(sc).pose(x2)
    up_rng = np.random.default_rng(18000 + seed)
    uploaded = int(up_rng.integers(0, len(trees))) if seed % 3 == 1 else None

    rays = draw_rays(seed, dtype, kind, x, iwr.world_triangles(sc))
    free = sc.trace(rays)
    tab = free["table"]
    tmax, tmax_pins = fs.draw_tmax(np.random.default_rng(19000 + seed), tab["cand_off"], tab["vals"][:, 0], 50.0, dtype)
    cut = sc.trace(rays, tmax)
    cut2 = sc2.trace(rays, tmax)

    n_pairs = int(sum(counts[int(t)] for t in sc.tree_of))
    pts = draw_points(seed, sc, n_pairs)
    prng = np.random.default_rng(20000 + seed)
    ks = (1, int(prng.integers(2, 64)), 64)
    cache = {}
    knn = {k: iknn.rows(sc, pts, k, cache=cache) for k in ks}
    mid = knn[ks[1]]
    with np.errstate(invalid="ignore"):
        kth = np.sqrt(np.array([r[-1][0] if len(r) else np.inf for r in mid], dtype=dtype))
    limits, limit_pins = fs.draw_limits(prng, kth, 4.0, dtype)
    fin = kth[np.isfinite(kth)]
    scalar_limit = float(dtype(np.median(fin))) if len(fin) else 1.0
    scalar_points = np.ascontiguousarray(pts[::max(1, len(pts) // MIN_POINTS)][:MIN_POINTS])   # (of all three kinds of point)
    planes = draw_regions(seed, sc, n_pairs)
    out = dict(seed=seed, dtype=dtype, kind=kind, trees=trees, counts=counts, uploaded=uploaded, n=n, tree_of=tree_of, x=x, x2=x2,
               klass=klass, klass2=klass2, scene=sc, scene2=sc2, rays=rays, free=free, cut=cut, cut2=cut2, tmax=tmax, tmax_pins=tmax_pins,
               points=pts, limits=limits, limit_pins=limit_pins, scalar_limit=scalar_limit, scalar_points=scalar_points, ks=ks,
               n_pairs=n_pairs, planes=planes, knn=knn, within=iwr.rows(sc, pts, limits),
               within_scalar=iwr.rows(sc, scalar_points, scalar_limit), region=irr.reference(sc, planes),
               within2=iwr.rows(sc2, pts, limits), knn2=iknn.rows(sc2, pts, ks[1]), region2=irr.reference(sc2, planes))
    out["seconds"] = time.perf_counter() - t0
    return out

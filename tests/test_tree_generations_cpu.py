"""Scenes, inputs, the reader table and the expected answers of tests/test_gpu_tree_generations.py, and — on the CPU alone — the proof that
those expectations can tell one tree generation from another.

A build, rebuild, refit or flatten writes what the wide walk reads; the FlatNode array, the folded binary array and the binary LDS slot
table are owed until something reads them, and every host function that reads one has to ask for them first (engine.hpp
ensure_flat_arrays; with BVHGPU_TUNE_FLATTEN_LAZY = 2 that call is also the join with the side stream).  A reader that forgets would
answer from the arrays of the generation before.  The GPU module makes every batch entry of the Python API the first reader of a new
generation; this module owns what it compares against:

  scenes      spheres in one cube, per dtype: A (1500, above the builder's BVH_MID_SMALL_MAXN = 768: every tier and the wave tier's inline
              flatten take part), B (1500 from another seed: another tree in buffers of the same size), A' (A with every sphere moved by up
              to one radius: the refit target), C (700: buffers shrink), D (2300: buffers grow).  Boxes are spheres_aabbs, one triangle per
              box is test_gpu_refit._tris_of
  inputs      ONE set per dtype, the same for every generation, so that two expectations differ through the tree alone: 1500 rays
              (test_gpu_refit._rays around A), a tmax per ray drawn around A's closest triangle hit, 64 / 300 points, 150 AABB / point /
              ball queries
  READERS     name -> (API method, the call, the reference), as data.  The references are the suite's own: the oracle and the Python
              restatements the family suites pin
  sensitivity for every reader want(A) != want(B) and want(A) != want(A'); the previous generation's flat array walked over the new
              generation's shape boxes — the stale-array model — is not the new CSR; every expectation is non-trivial

and the completeness check: a batch entry added to the API fails here until it has a row."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import allhits_ref as ar
import khits_ref as khr
import knn_ref as kr
import knn_tree_ref as ktr
import query_ref as qr
import sphere_ref as sr
import within_ref as wr
from oracle import orc
from test_box_hit_cpu import box_match
from test_gpu_any_hit import first_match
from test_gpu_refit import _points, _rays, _tris_of

NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
COUNTS = dict(A=1500, B=1500, C=700, D=2300)
SEEDS = dict(A=101, B=202, C=303, D=404)
SIDE = 40.0                                         # the cube every scene lies in
N_RAYS, N_POINTS, N_NEAREST, N_QUERIES = 1500, 64, 300, 150
K_HITS, K_NN = 4, 5
WITHIN_DIST, TREE_DIST = 4.0, 3.0
GENERATIONS = ("A", "B", "A1", "C", "D")            # A1: the tree of A refitted to the spheres of A'


def same(a, b) -> bool:
    """the suites' byte equality (two NaNs are equal whatever their sign and payload); node records are compared as bytes"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    return kr.same(a, b)


def same_all(got, want) -> bool:
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


def spheres_of(name, dtype):
    """the spheres of scene A, B, C, D or A' ("A1"): centres uniform in the cube, radii in [0.5, 2)"""
    if name == "A1":
        s = spheres_of("A", dtype).astype(np.float64)
        rng = np.random.default_rng(505)
        step = rng.normal(size=(len(s), 3))
        step *= (rng.uniform(0.2, 1.0, size=(len(s), 1)) * s[:, 3:4]) / np.linalg.norm(step, axis=1, keepdims=True)   # up to one radius
        return np.ascontiguousarray(np.concatenate([s[:, :3] + step, s[:, 3:4]], axis=1).astype(dtype))
    rng = np.random.default_rng(SEEDS[name])
    n = COUNTS[name]
    c = rng.uniform(0, SIDE, size=(n, 3))
    r = rng.uniform(0.5, 2.0, size=(n, 1))
    return np.ascontiguousarray(np.concatenate([c, r], axis=1).astype(dtype))


class Gen:
    """one tree generation: the caller's arrays (spheres, their boxes, one triangle per box) and the oracle's tree over the boxes"""

    def __init__(self, name, dtype):
        from bvh_amd.api import spheres_aabbs
        self.name, self.dtype = name, dtype
        self.spheres = spheres_of(name, dtype)
        self.aabbs = spheres_aabbs(self.spheres)
        assert self.aabbs.dtype == dtype
        self.tris = _tris_of(self.aabbs)
        if name == "A1":                            # a refit keeps the topology of the tree it finds
            built = gen("A", dtype)
            self.nodes, self.shape_node = orc.refit(built.nodes, self.aabbs), built.shape_node
        else:
            t = orc.build(self.aabbs)
            self.nodes, self.shape_node = t.nodes, t.shape_node
        self.flat = orc.flatten(self.nodes)
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    # what several references share: the CSR of the ray batch with its t-slices, and the leaf-stage records of its members
    def csr(self, I):
        return self.memo("csr", lambda: orc.traverse_flat(self.flat, self.aabbs, I.rays, want_t=True))

    def tri_stage(self, I):
        off, idx, _, _ = self.csr(I)
        return self.memo("tri", lambda: orc.triangle_stage(self.tris, I.rays, off, idx))

    def records(self, I, leaf):
        off, idx, ts, _ = self.csr(I)
        if leaf == "box":
            return ts
        if leaf == "triangle":
            return self.tri_stage(I)[0]
        return self.memo("sph", lambda: sr.list_hits(off, idx, I.rays, self.spheres))


@functools.lru_cache(maxsize=None)
def gen(name, dtype):
    """built once per scene and dtype, shared by the tests of both modules, never written to"""
    return Gen(name, dtype)


@functools.lru_cache(maxsize=None)
def inputs(dtype):
    """the one set of arguments every generation of `dtype` is asked with"""
    a = gen("A", dtype)
    rays = _rays(orc, a.aabbs, 1.0, N_RAYS, dtype, 7)
    I = SimpleNamespace(dtype=dtype, rays=rays)
    rng = np.random.default_rng(8)
    cd = a.tri_stage(I)[1][:, 0].astype(np.float64)                         # around A's closest hit, as the family suites draw it
    I.tmax = (np.where(np.isfinite(cd), cd, 0.5 * SIDE) * rng.uniform(0.3, 1.7, size=len(cd))).astype(dtype)
    I.points = _points(a.aabbs, 1.0, N_POINTS, dtype, 9)
    I.near_points = _points(a.aabbs, 1.0, N_NEAREST, dtype, 10)
    I.within_dist, I.tree_dist = dtype(WITHIN_DIST), dtype(TREE_DIST)
    b = a.aabbs[rng.integers(0, len(a.aabbs), N_QUERIES)].astype(np.float64)
    cq = (b[:, :3] + b[:, 3:]) * 0.5 + rng.normal(size=(N_QUERIES, 3))
    e = rng.uniform(0, 3, size=(N_QUERIES, 3))
    I.queries = {qr.AABB: np.ascontiguousarray(np.concatenate([cq - e, cq + e], axis=1).astype(dtype)),
                 qr.POINT: np.ascontiguousarray(cq.astype(dtype)),
                 qr.BALL: np.ascontiguousarray(np.concatenate([cq, e[:, :1]], axis=1).astype(dtype))}
    return I


# ---- the reader table -----------------------------------------------------------------------------------------------------------
# call(T, I):  T.bvh / T.flat the tree under test and its flat view, T.ctx their context; I the inputs plus I.rb, the RayBatch the GPU
#              module makes of I.rays.  Returns a tuple of arrays.
# want(G, I):  the same tuple from the references, for generation G.
class Reader:
    def __init__(self, name, method, call, want, kind="csr", needs=None):
        self.name, self.method, self.call, self.want, self.kind = name, method, call, want, kind
        self.needs = needs                          # "triangles" / "spheres": the caller-owned array the entry reads, None: the boxes alone

    def __repr__(self):
        return self.name


def _wide_csr(T, I):
    from bvh_amd._lib import TUNE_TRAVERSE_LDS_MIN_RAYS
    keep = T.ctx.get_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS)
    T.ctx.set_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS, 0)                        # the wide walk takes the small batch
    try:
        off, idx, _, st = T.flat.traverse_batch(I.rb)
    finally:
        T.ctx.set_tuning(TUNE_TRAVERSE_LDS_MIN_RAYS, keep)
    assert "k_traverse_wide" in st["kernel"], st["kernel"]
    return off, idx


def _stats_vec(st):
    return np.asarray([st["visited"], st["leaf_visits"], st["hits"]], dtype=np.uint64)


def _stats_csr(T, I):
    off, idx, _, st = T.flat.traverse_batch(I.rb, stats=True)
    return off, idx, _stats_vec(st)


def _query(kind, variant):
    def call(T, I):
        from bvh_amd._lib import TUNE_QUERY_VARIANT
        keep = T.ctx.get_tuning(TUNE_QUERY_VARIANT)
        T.ctx.set_tuning(TUNE_QUERY_VARIANT, variant)
        try:
            return T.flat.query_batch(kind, I.queries[kind])
        finally:
            T.ctx.set_tuning(TUNE_QUERY_VARIANT, keep)
    return call


def _scene_peer(T, I):
    from bvh_amd import FlatBvh
    blob = np.zeros(T.flat.scene_nbytes(), dtype=np.uint8)
    T.flat.scene_export(blob)
    peer = FlatBvh.scene_import(blob, len(blob), T.ctx)
    try:
        off, idx, _, st = peer.traverse_batch(I.rb, stats=True)
    finally:
        peer.close()
    return off, idx, _stats_vec(st)


def _host_batch(T, I):
    rays = np.ascontiguousarray(I.rays).copy()                              # pageable memory
    off = np.zeros(len(rays) + 1, np.uint32)
    idx = np.zeros(64 * len(rays), np.uint32)
    total = T.bvh.traverse_host(rays, None, off, idx)
    assert total <= len(idx), total
    return off, idx[:total].copy()


def _csr_want(G, I):
    return G.csr(I)[:2]


def _stats_want(G, I):
    off, idx, _, st = G.csr(I)
    return off, idx, _stats_vec(st)


NEEDS = dict(box=None, triangle="triangles", sphere="spheres")


def _khits(leaf):
    return Reader(f"khits_{leaf}", "khits_batch", lambda T, I: T.flat.khits_batch(I.rb, K_HITS, leaf, I.tmax),
                  lambda G, I: khr.khits_match(*G.csr(I)[:2], G.records(I, leaf), I.tmax, K_HITS), kind="rows", needs=NEEDS[leaf])


def _allhits(leaf, sort):
    return Reader(f"allhits_{leaf}_{'sorted' if sort else 'list'}", "allhits_batch", lambda T, I: T.flat.allhits_batch(I.rb, leaf, I.tmax, sort),
                  lambda G, I: ar.allhits_match(*G.csr(I)[:2], G.records(I, leaf), I.tmax, sort), kind="rows", needs=NEEDS[leaf])


def _within(tag, sort, count_only, triangles=False):
    def want(G, I):
        off, shape, dist = wr.within(G.flat, G.aabbs, I.points, I.within_dist, tris=G.tris if triangles else None, sort=sort)
        return (off, shape[:0], dist[:0]) if count_only else (off, shape, dist)
    return Reader(f"within_{tag}", "within_batch",
                  lambda T, I: T.flat.within_batch(I.points, I.within_dist, triangles=triangles, sort=sort, count_only=count_only),
                  want, kind="counts" if count_only else "rows", needs="triangles" if triangles else None)


READERS = [
    Reader("csr_wide", "traverse_batch", _wide_csr, _csr_want),
    Reader("csr_t", "traverse_batch", lambda T, I: T.flat.traverse_batch(I.rb, want_t=True)[:3], lambda G, I: G.csr(I)[:3]),
    Reader("csr_stats", "traverse_batch", _stats_csr, _stats_want),
    Reader("intersect_triangles", "intersect_triangles", lambda T, I: T.flat.intersect_triangles(I.rb)[:3],
           lambda G, I: G.csr(I)[:2] + (G.tri_stage(I)[0],), needs="triangles"),
    Reader("closest_hits", "closest_hits", lambda T, I: T.flat.closest_hits(I.rb)[:2], lambda G, I: G.tri_stage(I)[1:], kind="first",
           needs="triangles"),
    Reader("any_hits", "any_hits", lambda T, I: T.flat.any_hits(I.rb, I.tmax),
           lambda G, I: first_match(*G.csr(I)[:2], G.tri_stage(I)[0], I.tmax), kind="first", needs="triangles"),
    Reader("closest_box_hits", "closest_box_hits", lambda T, I: T.flat.closest_box_hits(I.rb, I.tmax),
           lambda G, I: box_match(*G.csr(I)[:3], I.tmax, False), kind="first"),
    Reader("first_box_hits", "first_box_hits", lambda T, I: T.flat.first_box_hits(I.rb, I.tmax),
           lambda G, I: box_match(*G.csr(I)[:3], I.tmax, True), kind="first"),
    Reader("closest_sphere_hits", "closest_sphere_hits", lambda T, I: T.flat.closest_sphere_hits(I.rb, I.tmax),
           lambda G, I: sr.sphere_match(*G.csr(I)[:2], I.rays, G.spheres, I.tmax, False, hits=G.records(I, "sphere")), kind="first",
           needs="spheres"),
    Reader("first_sphere_hits", "first_sphere_hits", lambda T, I: T.flat.first_sphere_hits(I.rb, I.tmax),
           lambda G, I: sr.sphere_match(*G.csr(I)[:2], I.rays, G.spheres, I.tmax, True, hits=G.records(I, "sphere")), kind="first",
           needs="spheres"),
    Reader("order_nearest", "traverse_batch", lambda T, I: T.flat.traverse_batch(I.rb, order="nearest")[:2],
           lambda G, I: orc.traverse_child_ordered(G.nodes, G.aabbs, I.rays, True)),
    Reader("order_nearest_heap", "traverse_batch", lambda T, I: T.flat.traverse_batch(I.rb, order="nearest_heap")[:2],
           lambda G, I: orc.traverse_distance(G.nodes, G.aabbs, I.rays, True)),
    _khits("box"), _khits("sphere"), _khits("triangle"),
    _allhits("box", True), _allhits("box", False), _allhits("sphere", True), _allhits("triangle", True),
    Reader("nearest_boxes", "nearest_batch", lambda T, I: T.flat.nearest_batch(I.near_points),
           lambda G, I: orc.nearest(G.flat, G.aabbs, I.near_points), kind="points"),
    Reader("nearest_triangles", "nearest_batch", lambda T, I: T.flat.nearest_batch(I.near_points, triangles=True),
           lambda G, I: orc.nearest(G.flat, G.aabbs, I.near_points, G.tris), kind="points", needs="triangles"),
    Reader("knearest", "knearest_batch", lambda T, I: T.flat.knearest_batch(I.points, K_NN),
           lambda G, I: kr.knearest(G.flat, G.aabbs, I.points, (K_NN,))[K_NN], kind="points"),
    Reader("knearest_tree", "knearest_tree_batch", lambda T, I: T.bvh.knearest_tree_batch(I.points, K_NN),
           lambda G, I: ktr.knearest_tree(G.nodes, G.aabbs, I.points, (K_NN,))[K_NN], kind="points"),
    Reader("knearest_tree_max_dist", "knearest_tree_batch", lambda T, I: T.bvh.knearest_tree_batch(I.points, K_NN, max_dist=I.tree_dist),
           lambda G, I: ktr.knearest_tree(G.nodes, G.aabbs, I.points, (K_NN,), max_dist=I.tree_dist)[K_NN], kind="points"),
    Reader("knearest_triangles", "knearest_batch", lambda T, I: T.flat.knearest_batch(I.points, K_NN, triangles=True),
           lambda G, I: kr.knearest(G.flat, G.aabbs, I.points, (K_NN,), tris=G.tris)[K_NN], kind="points", needs="triangles"),
    Reader("knearest_tree_triangles", "knearest_tree_batch", lambda T, I: T.bvh.knearest_tree_batch(I.points, K_NN, triangles=True),
           lambda G, I: ktr.knearest_tree(G.nodes, G.aabbs, I.points, (K_NN,), tris=G.tris)[K_NN], kind="points", needs="triangles"),
    _within("sorted", True, False), _within("list", False, False), _within("count_only", True, True), _within("triangles", True, False, True),
] + [
    Reader(f"query_{tag}_v{variant}", "query_batch", _query(kind, variant), lambda G, I, kind=kind: qr.walk(G.flat, G.aabbs, kind, I.queries[kind]))
    for tag, kind in (("aabb", qr.AABB), ("point", qr.POINT), ("ball", qr.BALL)) for variant in (0, 1)
] + [
    Reader("self_overlaps", "self_overlaps", lambda T, I: T.flat.self_overlaps(), lambda G, I: qr.walk(G.flat, G.aabbs, qr.AABB, G.aabbs),
           kind="rows"),                                                   # (row i holds i: no empty row)
    Reader("flat_nodes", "nodes", lambda T, I: (T.flat.nodes,), lambda G, I: (G.flat,), kind="array"),
    Reader("bvh_nodes", "nodes", lambda T, I: (T.bvh.nodes, T.bvh.shape_nodes), lambda G, I: (G.nodes, G.shape_node), kind="array"),
    Reader("scene_peer", "scene_export", _scene_peer, _stats_want),
    Reader("traverse_host", "traverse_host", _host_batch, _csr_want),
]
READER_IDS = [r.name for r in READERS]

# Public methods that run no batch of their own — the only kind this list may hold: they call a batch entry that has a row.
EXCLUDED = {
    "occluded": "any_hits(...)[1] != NONE",
    "box_occluded": "first_box_hits(...)[1] != NONE",
    "sphere_occluded": "first_sphere_hits(...)[1] != NONE",
    "nearest_to": "nearest_batch of one point",
    "traverse": "traverse_batch / query_batch of one query, mapped to the caller's shapes",
    "nearest_traverse": "traverse_batch(order='nearest_heap') of one ray",
    "farthest_traverse": "traverse_batch(order='farthest_heap') of one ray: the kernel of order_nearest_heap",
    "nearest_child_traverse": "traverse_batch(order='nearest') of one ray",
    "farthest_child_traverse": "traverse_batch(order='farthest') of one ray: the kernel of order_nearest",
    "traverse_async": "enqueues only; tests/test_gpu_async_order.py covers it and its wait",
}
# ... and what is no query at all: how a generation is made, what the caller hands over, and sizes.  The GPU module drives these.
LIFECYCLE = {
    "build", "build_par", "build_with_executor", "from_aabbs", "from_flat_nodes", "scene_import", "rebuild", "rebuild_async", "refit", "wait",
    "flatten", "flatten_in_place", "close", "set_triangles", "set_spheres", "info", "build_levels", "shape_nodes", "scene_nbytes",
    "hits_device", "query_kernel", "traverse_host_indices",
}
# the batch entries the table must hold whatever the API looks like
ENTRIES = {"traverse_batch", "intersect_triangles", "closest_hits", "any_hits", "closest_box_hits", "first_box_hits", "closest_sphere_hits",
           "first_sphere_hits", "khits_batch", "allhits_batch", "nearest_batch", "knearest_batch", "knearest_tree_batch", "within_batch",
           "query_batch", "self_overlaps", "traverse_host", "nodes", "scene_export"}


def want(reader, name, dtype):
    """the expectation of `reader` on generation `name`: computed once, shared, never written to"""
    return _want(reader.name, name, dtype)


@functools.lru_cache(maxsize=None)
def _want(reader_name, name, dtype):
    r = READERS[READER_IDS.index(reader_name)]
    out = tuple(np.ascontiguousarray(x) for x in r.want(gen(name, dtype), inputs(dtype)))
    for x in out:
        x.setflags(write=False)
    return out


# ---- no silent omission ---------------------------------------------------------------------------------------------------------
def test_every_batch_entry_has_a_row():
    from bvh_amd import api
    public = set()
    for cls in (api._TreeBase, api.FlatBvh, api.Bvh):
        public |= {k for k, v in vars(cls).items() if not k.startswith("_") and (callable(v) or isinstance(v, (property, staticmethod)))}
    rows = {r.method for r in READERS}
    assert ENTRIES <= rows, sorted(ENTRIES - rows)
    assert rows <= public, sorted(rows - public)
    assert not (rows & set(EXCLUDED)) and not (rows & LIFECYCLE) and not (set(EXCLUDED) & LIFECYCLE)
    assert set(EXCLUDED) <= public and LIFECYCLE <= public, sorted((set(EXCLUDED) | LIFECYCLE) - public)
    missing = public - rows - set(EXCLUDED) - LIFECYCLE
    assert not missing, f"no row in READERS and no reason in EXCLUDED for {sorted(missing)}"
    assert all(isinstance(why, str) and why for why in EXCLUDED.values())
    assert len(set(READER_IDS)) == len(READER_IDS)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_scenes_are_what_the_transitions_need(dtype):
    a, b, a1, c, d = (gen(n, dtype) for n in GENERATIONS)
    assert len(a.aabbs) == len(b.aabbs) == len(a1.aabbs) == 1500 > 768 and len(c.aabbs) == 700 and len(d.aabbs) == 2300
    assert a.nodes.tobytes() != b.nodes.tobytes() and len(a.flat) == len(b.flat) and a.flat.tobytes() != b.flat.tobytes()
    # A': every sphere moved, none by more than its radius; the refit keeps the topology and changes the boxes
    step = np.linalg.norm(a1.spheres[:, :3].astype(np.float64) - a.spheres[:, :3].astype(np.float64), axis=1)
    assert (step > 0).all() and (step <= a.spheres[:, 3] * (1 + 1e-6)).all() and np.array_equal(a1.spheres[:, 3], a.spheres[:, 3])
    for f in ("parent", "l", "r", "shape"):
        assert np.array_equal(a.nodes[f], a1.nodes[f])
    assert np.array_equal(a.flat["entry"], a1.flat["entry"]) and np.array_equal(a.flat["exit"], a1.flat["exit"])
    assert np.array_equal(a.flat["shape"], a1.flat["shape"]) and a.flat.tobytes() != a1.flat.tobytes()
    assert orc.check_tree(a1.nodes, a1.aabbs) == 0
    assert a1.nodes.tobytes() != orc.build(a1.aabbs).nodes.tobytes()      # (a rebuild of A' would be another tree: the expectation is the refit's)
    for g in (a, b, a1, c, d):                                            # the child-ordered iterator's 32-entry stack
        assert orc.tree_stats(g.nodes, g.aabbs)["max_depth"] < 31


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reader", READERS, ids=READER_IDS)
def test_expectations_tell_the_generations_apart(reader, dtype):
    """a reader that answered from generation A after the transition fails the GPU test: A's answer is not B's, nor the refitted tree's,
    nor D's (whose predecessor is C)"""
    wa = want(reader, "A", dtype)
    for other in ("B", "A1", "C", "D"):
        assert not same_all(wa, want(reader, other, dtype)), other
    assert not same_all(want(reader, "C", dtype), want(reader, "D", dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stale_arrays_over_new_boxes_are_not_the_new_answer(dtype):
    """the model of a reader that skipped ensure_flat_arrays: the walk runs over the previous generation's flat array while the shape
    boxes — rewritten by every build and refit at once — are the new ones"""
    I = inputs(dtype)
    a = gen("A", dtype)
    for new in ("B", "A1"):
        g = gen(new, dtype)
        soff, sidx, _, _ = orc.traverse_flat(a.flat, g.aabbs, I.rays)
        off, idx = g.csr(I)[:2]
        assert not (np.array_equal(soff, off) and np.array_equal(sidx, idx)), new
        for kind, q in I.queries.items():
            assert not same_all(qr.walk(a.flat, g.aabbs, kind, q), qr.walk(g.flat, g.aabbs, kind, q)), (new, kind)
    c, d = gen("C", dtype), gen("D", dtype)
    assert len(c.flat) < len(a.flat) < len(d.flat)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["B", "A1", "D"])
def test_expectations_are_not_trivial(name, dtype):
    """on every generation a reader is checked on: CSR totals above zero, rows with two members and more for the multi-hit and radius
    families, hits and misses for the one-record-per-ray variants"""
    for r in READERS:
        w = want(r, name, dtype)
        if r.kind == "csr":
            off = w[0].astype(np.int64)
            assert off[-1] > 0 and len(w[1]) == off[-1] and (np.diff(off) >= 2).any() and (np.diff(off) == 0).any(), r
        elif r.kind == "rows" and r.method == "khits_batch":
            shape = w[1]
            assert ((shape != NONE).sum(axis=1) >= 2).any() and (shape == NONE).all(axis=1).any(), r
        elif r.kind == "rows":
            off = w[0].astype(np.int64)
            assert off[-1] > 0 and len(w[1]) == off[-1] and (np.diff(off) >= 2).any(), r
        elif r.kind == "counts":
            assert w[0][-1] > 0 and len(w[1]) == 0 and (np.diff(w[0].astype(np.int64)) >= 2).any(), r
        elif r.kind == "first":
            shape = w[1]
            assert (shape == NONE).any() and (shape != NONE).any(), r
        elif r.kind == "points":
            assert (w[0] != NONE).any() and np.isfinite(w[1]).any(), r
        else:
            assert all(len(x) > 0 for x in w), r
    # a sorted row is not its list order, and the limit of knearest_tree does cut rows
    assert not same_all(want(READERS[READER_IDS.index("allhits_box_sorted")], name, dtype), want(READERS[READER_IDS.index("allhits_box_list")], name, dtype))
    assert not same_all(want(READERS[READER_IDS.index("within_sorted")], name, dtype), want(READERS[READER_IDS.index("within_list")], name, dtype))
    assert not same_all(want(READERS[READER_IDS.index("knearest_tree")], name, dtype), want(READERS[READER_IDS.index("knearest_tree_max_dist")], name, dtype))

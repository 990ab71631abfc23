"""Which refusal a C entry point gives, with which message, and which one wins when two apply — for the batch entry points whose front
ends capi.hip shares (bvhgpu_traverse_*, _traverse_async_*, _traverse_any_*, _traverse_box_*, _query_*, _nearest_*, _knearest_*,
_knearest_tree_*, the per-ray fetches, _rebuild*/_refit_*), and the precedence alone for bvhgpu_traverse_sphere_* and bvhgpu_region_*,
whose own suites assert each refusal by itself.  The other suites assert refusal STATUSES; this one pins the message
and the precedence, through ctypes, so that arguments the Python layer would reject reach the C entry point.  After every refused call a
valid call on the same tree and result object must still give the oracle's answer: a refusal leaves no half-set state.
Not here: an uploaded tree given to bvhgpu_knearest_tree_* ("BvhNode" in the message) is asserted by test_gpu_knn_tree.test_errors, and
the 2^32-2 limits are not run at all (a lost check would go on to read 4 G elements)."""
import ctypes as C

import numpy as np
import pytest

import knn_ref as kr
import knn_tree_ref as ktr
import query_ref as qr
import region_ref as rr
from test_box_hit_cpu import box_match
from test_gpu_any_hit import first_match

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, DTYPE_MISMATCH, NOT_FLATTENED = 0, 1, 6, 7
HOST, DEVICE = 0, 1
N, K = 4, 3
FT = {"f32": np.float32, "f64": np.float64}
TREE_SFX = {"f32": "f32", "f64": "f64", "unflat": "f32"}   # the three trees: flattened f32 (with triangles), flattened f64, built f32 never flattened

ASYNC_PENDING = "the result object still holds an asynchronous batch"
MEM_MSG = "mem must be BVHGPU_HOST or BVHGPU_DEVICE"
ANY_FLAGS = "any-hit flags: 0 or BVHGPU_TRAVERSE_COHERENT"
BOX_FLAGS = "box-hit flags: BVHGPU_TRAVERSE_COHERENT and BVHGPU_TRAVERSE_FIRST only"
FLATTEN_FIRST = "call bvhgpu_flatten first"
K_MSG = "k must be between 1 and BVHGPU_KNN_MAX_K"
KIND_MSG = "shape kind must be 0 (AABB) or 1 (triangle)"
TRI_DIST = "triangle distance needs bvhgpu_tree_set_triangles first"
SPHERE_FLAGS = "sphere-hit flags: BVHGPU_TRAVERSE_COHERENT and BVHGPU_TRAVERSE_FIRST only"
PLANES_MAX, PLANE_DTYPE = "more than BVHGPU_REGION_MAX_PLANES planes per region", "tree dtype differs from plane dtype"
M = 6                                                      # planes per region of the valid region call
RAY_DTYPE, QUERY_DTYPE, POINT_DTYPE = "tree dtype differs from ray dtype", "tree dtype differs from query dtype", "tree dtype differs from point dtype"

# (entry point, tree, arguments that differ from a valid call — None is a NULL pointer, expected status, expected part of bvhgpu_last_error)
SINGLE = [
    # hits == NULL
    ("traverse_f32", "f32", dict(hits=None), INVALID_ARG, "hits is NULL"),
    ("traverse_async_f32", "f32", dict(hits=None), INVALID_ARG, "hits is NULL"),
    ("traverse_any_f32", "f32", dict(hits=None), INVALID_ARG, "hits is NULL"),
    ("traverse_box_f32", "f32", dict(hits=None), INVALID_ARG, "hits is NULL"),
    ("query_f32", "f32", dict(hits=None), INVALID_ARG, "hits is NULL"),
    # a bad mem value
    ("traverse_async_f32", "f32", dict(mem=HOST), INVALID_ARG, "asynchronous traversal takes rays that are resident in HBM"),
    ("traverse_any_f32", "f32", dict(mem=7), INVALID_ARG, MEM_MSG),
    ("traverse_box_f32", "f32", dict(mem=7), INVALID_ARG, MEM_MSG),
    ("query_f32", "f32", dict(mem=7), INVALID_ARG, MEM_MSG),
    # a bad flag
    ("traverse_any_f32", "f32", dict(flags=1), INVALID_ARG, ANY_FLAGS),
    ("traverse_any_f32", "f32", dict(flags=1024), INVALID_ARG, ANY_FLAGS),
    ("traverse_box_f32", "f32", dict(flags=1), INVALID_ARG, BOX_FLAGS),
    ("query_f32", "f32", dict(flags=1), INVALID_ARG, "query flags are reserved (0)"),
    ("query_f32", "f32", dict(kind=7), INVALID_ARG, "unknown query kind"),
    ("traverse_f32", "f32", dict(flags=128), INVALID_ARG, "BEST_FIRST needs NEAREST_FIRST or FARTHEST_FIRST"),
    ("traverse_f32", "f32", dict(flags=1 | 4), INVALID_ARG, "T_SLICE cannot be combined with TRIANGLES / CLOSEST"),
    # wrong dtype
    ("traverse_f32", "f64", {}, DTYPE_MISMATCH, RAY_DTYPE),
    ("traverse_async_f32", "f64", {}, DTYPE_MISMATCH, RAY_DTYPE),
    ("traverse_any_f64", "f32", {}, DTYPE_MISMATCH, RAY_DTYPE),
    ("traverse_box_f32", "f64", {}, DTYPE_MISMATCH, RAY_DTYPE),
    ("query_f32", "f64", {}, DTYPE_MISMATCH, QUERY_DTYPE),
    ("nearest_f32", "f64", {}, DTYPE_MISMATCH, POINT_DTYPE),
    ("knearest_f64", "f32", {}, DTYPE_MISMATCH, POINT_DTYPE),
    ("knearest_tree_f32", "f64", {}, DTYPE_MISMATCH, POINT_DTYPE),
    # not flattened
    ("traverse_f32", "unflat", {}, NOT_FLATTENED, FLATTEN_FIRST),
    ("traverse_async_f32", "unflat", {}, NOT_FLATTENED, FLATTEN_FIRST),
    ("traverse_box_f32", "unflat", {}, NOT_FLATTENED, FLATTEN_FIRST),
    ("query_f32", "unflat", {}, NOT_FLATTENED, FLATTEN_FIRST),
    ("nearest_f32", "unflat", {}, NOT_FLATTENED, FLATTEN_FIRST),
    ("knearest_f32", "unflat", {}, NOT_FLATTENED, FLATTEN_FIRST),
    # NULL input with n > 0
    ("traverse_f32", "f32", dict(rays=None), INVALID_ARG, "rays is NULL"),
    ("traverse_async_f32", "f32", dict(rays=None), INVALID_ARG, "rays is NULL"),
    ("traverse_any_f32", "f32", dict(rays=None), INVALID_ARG, "rays is NULL"),
    ("traverse_box_f64", "f64", dict(rays=None), INVALID_ARG, "rays is NULL"),
    ("query_f32", "f32", dict(queries=None), INVALID_ARG, "queries is NULL: only BVHGPU_QUERY_AABB with n = the tree's shape count"),
    ("nearest_f32", "f32", dict(points=None), INVALID_ARG, "NULL argument"),
    ("knearest_f32", "f32", dict(out_shape=None), INVALID_ARG, "NULL argument"),
    ("knearest_tree_f32", "unflat", dict(out_dist=None), INVALID_ARG, "NULL argument"),
    # triangles missing
    ("traverse_any_f64", "f64", {}, INVALID_ARG, "any-hit queries need bvhgpu_tree_set_triangles first"),
    ("traverse_f64", "f64", dict(flags=4), INVALID_ARG, "TRIANGLES / CLOSEST need bvhgpu_tree_set_triangles first"),
    ("nearest_f64", "f64", dict(kind=1), INVALID_ARG, TRI_DIST),
    ("knearest_f64", "f64", dict(kind=1), INVALID_ARG, TRI_DIST),
    ("knearest_tree_f32", "unflat", dict(kind=1), INVALID_ARG, TRI_DIST),
    # k
    ("knearest_f32", "f32", dict(k=0), INVALID_ARG, K_MSG),
    ("knearest_f32", "f32", dict(k=65), INVALID_ARG, K_MSG),
    ("knearest_tree_f32", "f32", dict(k=0), INVALID_ARG, K_MSG),
    ("knearest_tree_f64", "f64", dict(k=65), INVALID_ARG, K_MSG),
    # kind == 2
    ("nearest_f32", "f32", dict(kind=2), INVALID_ARG, KIND_MSG),
    ("knearest_f32", "f32", dict(kind=2), INVALID_ARG, KIND_MSG),
    ("knearest_tree_f32", "f32", dict(kind=2), INVALID_ARG, KIND_MSG),
    # the rebuild / refit exports guard their dtype
    ("rebuild_f32", "f64", {}, DTYPE_MISMATCH, "tree is f64"),
    ("rebuild_flat_f32", "f64", {}, DTYPE_MISMATCH, "tree is f64"),
    ("rebuild_flat_async_f32", "f64", {}, DTYPE_MISMATCH, "tree is f64"),
    ("refit_f32", "f64", {}, DTYPE_MISMATCH, "tree is f64"),
    ("rebuild_f64", "f32", {}, DTYPE_MISMATCH, "tree is f32"),
    ("rebuild_flat_f64", "f32", {}, DTYPE_MISMATCH, "tree is f32"),
    ("rebuild_flat_async_f64", "f32", {}, DTYPE_MISMATCH, "tree is f32"),
    ("refit_f64", "f32", {}, DTYPE_MISMATCH, "tree is f32"),
]

# two rules violated at once: the caller gets the one the entry point tests first
PRECEDENCE = [
    ("traverse_any_f32", "f32", dict(flags=1, mem=7), INVALID_ARG, ANY_FLAGS),                      # flags before mem
    ("traverse_any_f32", "f32", dict(flags=1, hits=None), INVALID_ARG, "hits is NULL"),             # hits before flags
    ("traverse_any_f32", "f64", dict(mem=7), INVALID_ARG, MEM_MSG),                                 # mem before dtype
    ("traverse_any_f64", "unflat", {}, DTYPE_MISMATCH, RAY_DTYPE),                                  # dtype before flattened
    ("traverse_any_f32", "unflat", {}, NOT_FLATTENED, FLATTEN_FIRST),                               # flattened before triangles
    ("traverse_any_f64", "f64", dict(rays=None), INVALID_ARG, "rays is NULL"),                      # NULL rays before triangles
    ("traverse_box_f32", "unflat", dict(rays=None), NOT_FLATTENED, FLATTEN_FIRST),                  # flattened before NULL rays
    ("traverse_box_f32", "f32", dict(flags=1, mem=7), INVALID_ARG, BOX_FLAGS),
    ("traverse_f32", "f64", dict(rays=None), DTYPE_MISMATCH, RAY_DTYPE),                            # dtype before NULL rays
    ("traverse_f64", "f64", dict(rays=None, flags=4), INVALID_ARG, "rays is NULL"),                 # NULL rays before the flags' needs
    ("traverse_async_f32", "f64", dict(mem=HOST), INVALID_ARG, "asynchronous traversal takes rays"),  # mem before dtype
    ("query_f32", "f32", dict(kind=7, flags=1), INVALID_ARG, "unknown query kind"),                 # kind before flags
    ("query_f32", "f64", dict(flags=1), INVALID_ARG, "query flags are reserved (0)"),               # flags before dtype
    ("query_f32", "unflat", dict(queries=None), NOT_FLATTENED, FLATTEN_FIRST),                      # flattened before NULL queries
    ("knearest_f32", "f32", dict(k=0, points=None), INVALID_ARG, K_MSG),                            # k before NULL
    ("knearest_f32", "unflat", dict(k=0), NOT_FLATTENED, FLATTEN_FIRST),                            # flattened before k
    ("knearest_f32", "f32", dict(points=None, kind=2), INVALID_ARG, "NULL argument"),               # NULL before kind
    ("knearest_tree_f32", "f64", dict(k=0), DTYPE_MISMATCH, POINT_DTYPE),                           # dtype before k
    ("knearest_tree_f32", "f32", dict(k=0, kind=2), INVALID_ARG, K_MSG),                            # k before kind
    ("nearest_f32", "f32", dict(points=None, kind=2), INVALID_ARG, "NULL argument"),                # NULL before kind
    ("nearest_f64", "f64", dict(kind=2, out_dist=None), INVALID_ARG, "NULL argument"),
    ("nearest_f32", "unflat", dict(points=None), NOT_FLATTENED, FLATTEN_FIRST),                     # flattened before NULL
    # bvhgpu_traverse_sphere_*: the any-hit and box-hit order (no tree here has spheres: that rule is the last one)
    ("traverse_sphere_f32", "f32", dict(flags=1, mem=7), INVALID_ARG, SPHERE_FLAGS),                # flags before mem
    ("traverse_sphere_f32", "f32", dict(flags=1, hits=None), INVALID_ARG, "hits is NULL"),          # hits before flags
    ("traverse_sphere_f32", "f64", dict(mem=7), INVALID_ARG, MEM_MSG),                              # mem before dtype
    ("traverse_sphere_f64", "unflat", {}, DTYPE_MISMATCH, RAY_DTYPE),                               # dtype before flattened
    ("traverse_sphere_f32", "unflat", dict(rays=None), NOT_FLATTENED, FLATTEN_FIRST),               # flattened before NULL rays
    ("traverse_sphere_f32", "f32", dict(rays=None), INVALID_ARG, "rays is NULL"),                   # NULL rays before the spheres
    ("traverse_sphere_f32", "f32", {}, INVALID_ARG, "sphere queries need bvhgpu_tree_set_spheres first"),
    # bvhgpu_region_*: hits, dtype, flattened, the plane count, NULL planes, mem, flags
    ("region_f32", "f64", dict(hits=None), INVALID_ARG, "hits is NULL"),                            # hits before dtype
    ("region_f64", "unflat", {}, DTYPE_MISMATCH, PLANE_DTYPE),                                      # dtype before flattened
    ("region_f32", "unflat", dict(m=33), NOT_FLATTENED, FLATTEN_FIRST),                             # flattened before the plane count
    ("region_f32", "f32", dict(m=33, planes=None), INVALID_ARG, PLANES_MAX),                        # the plane count before NULL planes
    ("region_f32", "f32", dict(planes=None, mem=7), INVALID_ARG, "planes is NULL"),                 # NULL planes before mem
    ("region_f32", "f32", dict(mem=7, flags=4), INVALID_ARG, MEM_MSG),                              # mem before flags
    ("region_f32", "f32", dict(flags=4), INVALID_ARG, "region flags: BVHGPU_REGION_COUNT_ONLY and BVHGPU_REGION_CLASSIFY only"),
]


class World:
    """three trees of 8 unit boxes on one ctx, 4 rays and 4 points per dtype, and the oracle's answers for them"""

    def __init__(self, eng, orc):
        from bvh_amd import Context, _lib, region
        self.lib, self.ptr = _lib.load(), _lib.ptr
        self.ctx = Context(0)
        boxes = np.array([[2 * i, 0, 0, 2 * i + 1, 1, 1] for i in range(8)], dtype=np.float64)
        tris = np.array([[[2 * i + 0.5, 0, 0], [2 * i + 0.5, 0, 1], [2 * i + 0.5, 1, 0]] for i in range(8)], dtype=np.float64)
        origins = np.array([[-1, 0.25, 0.25], [4.5, 0.5, -1], [-1, 5, 5], [-1, 0.75, 0.5]])
        dirs = np.array([[1, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0.01, 0]])
        points = np.array([[0.25, 0.25, 0.25], [5.5, 2, 0.5], [20, 0, 0], [6.5, 0.5, 0.5]])
        self.inp, self.ref, self.trees = {}, {}, {}
        for sfx, ft in FT.items():
            a, p = boxes.astype(ft), points.astype(ft)
            rays = np.ascontiguousarray(orc.make_rays(origins, dirs, ft))
            tmax = np.full(N, 9.25, dtype=ft)
            planes = np.ascontiguousarray(np.stack([region.aabb_planes(q - 1.5, q + 1.5, ft) for q in points]))   # (N, M, 4): a box about each point
            rays_dev = C.c_void_p()
            _lib.check(self.lib.bvhgpu_device_alloc(self.ctx._h, rays.nbytes, C.byref(rays_dev)), self.ctx._h)
            _lib.check(self.lib.bvhgpu_device_copy(self.ctx._h, rays_dev, DEVICE, self.ptr(rays), HOST, rays.nbytes), self.ctx._h)
            self.inp[sfx] = dict(aabbs=a, rays=rays, rays_dev=rays_dev, tmax=tmax, points=p, tris=tris.astype(ft), planes=planes)
            tree = orc.build(a)
            oflat = orc.flatten(tree.nodes)
            off, idx, ts, _ = orc.traverse_flat(oflat, a, rays, want_t=True)
            ref = dict(csr=(off, idx), box=box_match(off, idx, ts, tmax, False), query=qr.walk(oflat, a, qr.POINT, p), region=rr.walk(oflat, a, planes),
                       nearest=orc.nearest(oflat, a, p), knearest=kr.knearest(oflat, a, p, [K])[K],
                       knearest_tree=ktr.knearest_tree(tree.nodes, a, p, [K])[K])
            if sfx == "f32":
                oisect, _, _ = orc.triangle_stage(tris.astype(ft), rays, off, idx)
                ref["any"] = first_match(off, idx, oisect, tmax)
            self.ref[sfx] = ref
            self.trees[sfx] = eng.Bvh.from_aabbs(a, self.ctx).flatten()
        self.trees["f32"].set_triangles(self.inp["f32"]["tris"])                  # triangles on one tree only
        self.trees["unflat"] = eng.Bvh.from_aabbs(self.inp["f32"]["aabbs"], self.ctx)   # the same f32 tree before bvhgpu_flatten
        self.out = {sfx: (np.zeros((N, 64), np.uint32), np.zeros((N, 64), ft)) for sfx, ft in FT.items()}

    def close(self):
        for i in self.inp.values():
            self.lib.bvhgpu_device_free(self.ctx._h, i["rays_dev"])

    def hits(self, tree):
        return self.trees[tree]._hits.h

    def call(self, entry, tree, over=None, hits_of=None):
        """the entry point with valid arguments of ITS dtype, except those in `over`; the result object is the tree's own, or tree hits_of's"""
        over = over or {}
        hits_of = hits_of or tree
        family, sfx = entry.rsplit("_", 1)
        i, t, p = self.inp[sfx], self.trees[tree]._t, self.ptr
        g = over.get
        h = C.byref(self.hits(hits_of)) if g("hits", 1) is not None else None
        n, out_s, out_d = g("n", N), self.out[sfx][0], self.out[sfx][1]
        if family in ("traverse", "traverse_async"):
            rays = g("rays", i["rays_dev"] if family == "traverse_async" else p(i["rays"]))
            args = (t, rays, n, g("mem", DEVICE if family == "traverse_async" else HOST), g("flags", 0), h)
        elif family in ("traverse_any", "traverse_box", "traverse_sphere"):
            args = (t, g("rays", p(i["rays"])), g("tmax", p(i["tmax"])), n, g("mem", HOST), g("flags", 0), h)
        elif family == "query":
            args = (t, g("kind", qr.POINT), g("queries", p(i["points"])), n, g("mem", HOST), g("flags", 0), h)
        elif family == "region":
            args = (t, g("planes", p(i["planes"])), n, g("m", M), g("mem", HOST), g("flags", 0), h)
        elif family in ("nearest", "knearest", "knearest_tree"):
            args = (t, g("points", p(i["points"])), n, HOST, g("kind", 0))
            args += {"nearest": (), "knearest": (g("k", K),), "knearest_tree": (g("k", K), None)}[family]
            args += (g("out_shape", p(out_s)), g("out_dist", p(out_d)))
        else:   # rebuild* / refit
            args = (t, p(i["aabbs"]), 8, HOST)
        return getattr(self.lib, "bvhgpu_" + entry)(*args)

    def error(self):
        return self.lib.bvhgpu_last_error(self.ctx._h).decode()

    def fetch_csr(self, tree):
        return self.trees[tree]._hits.fetch(N)

    def fetch_rows(self, kind, tree, sfx):
        per = 2 if kind == "box" else 3
        vals, shape = np.zeros((N, per), FT[sfx]), np.zeros(N, np.uint32)
        assert getattr(self.lib, "bvhgpu_hits_fetch_" + kind)(self.hits(tree), self.ptr(vals), self.ptr(shape), HOST) == OK, self.error()
        return vals, shape

    def still_works(self, entry, tree):
        """a valid call of the refused entry point's family with the refused call's result object — on the same tree where the family
        can run on it, else on the flattened f32 tree — gives the oracle's answer"""
        family = entry.rsplit("_", 1)[0]
        if family in ("nearest", "knearest", "knearest_tree"):
            if tree == "unflat":
                family = "knearest_tree"                       # (the one point walk that needs no flatten)
            sfx = TREE_SFX[tree]
            assert self.call(f"{family}_{sfx}", tree) == OK, self.error()
            want = self.ref[sfx][family]
            cols = 1 if family == "nearest" else K
            got_s, got_d = (o.reshape(-1)[:N * cols].reshape(want[0].shape) for o in self.out[sfx])
            assert np.array_equal(got_s, want[0]) and kr.same(np.ascontiguousarray(got_d), want[1]), (entry, tree)
            return
        hits_of = tree                                          # the result object the refused call was given
        if tree == "unflat":
            tree = "f32"                                        # no ray or query batch can run on that tree: the flattened f32 tree takes its place
        sfx = TREE_SFX[tree]
        if family.startswith(("rebuild", "refit")) or family in ("traverse_async", "traverse_sphere") or (family == "traverse_any" and tree != "f32"):
            family = "traverse"                                 # (rebuild / refit refusals: the tree still answers; any-hit needs triangles, sphere hits spheres)
        assert self.call(f"{family}_{sfx}", tree, hits_of=hits_of) == OK, self.error()
        if family == "traverse":
            off, idx = self.fetch_csr(hits_of)
            assert np.array_equal(off, self.ref[sfx]["csr"][0]) and np.array_equal(idx, self.ref[sfx]["csr"][1]), (entry, tree)
        elif family == "query":
            off, idx = self.fetch_csr(hits_of)
            assert off.tobytes() == self.ref[sfx]["query"][0].tobytes() and idx.tobytes() == self.ref[sfx]["query"][1].tobytes(), (entry, tree)
        elif family == "region":
            want = self.ref[sfx]["region"]
            off, idx = np.zeros(N + 1, np.uint32), np.zeros(len(want[1]) + 1, np.uint32)
            assert self.lib.bvhgpu_hits_fetch_region(self.hits(hits_of), self.ptr(off), self.ptr(idx), None, HOST) == OK, self.error()
            assert off.tobytes() == want[0].tobytes() and idx[:-1].tobytes() == want[1].tobytes() and len(want[1]) > N, (entry, tree)
        else:
            kind = family.split("_")[1]
            vals, shape = self.fetch_rows(kind, hits_of, sfx)
            assert vals.tobytes() == self.ref[sfx][kind][0].tobytes() and np.array_equal(shape, self.ref[sfx][kind][1]), (entry, tree)


@pytest.fixture(scope="module")
def world():
    import bvh_amd
    from oracle import orc
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    w = World(bvh_amd, orc)
    yield w
    w.close()


def _row_id(row):
    return f"{row[0]}-{row[1]}-" + ",".join(f"{k}={v}" for k, v in row[2].items())


@pytest.mark.parametrize("row", SINGLE + PRECEDENCE, ids=_row_id)
def test_refusal_status_message_and_aftermath(world, row):
    entry, tree, over, status, message = row
    rc = world.call(entry, tree, over)
    err = world.error()
    print(f"{entry} on {tree} {over}: status {rc}, message {err!r}")
    assert rc == status and message in err
    world.still_works(entry, tree)


def test_knearest_tree_needs_no_flatten(world):
    """the nearest-first descent on a built, unflattened tree with valid arguments is no refusal (where bvhgpu_knearest_* answers NOT_FLATTENED)"""
    assert world.call("knearest_tree_f32", "unflat") == OK, world.error()
    world.still_works("knearest_tree_f32", "unflat")


def test_async_traverse_still_works_after_its_refusals(world):
    """the valid asynchronous call itself (the rows above follow a refused asynchronous call with a synchronous one)"""
    for over in (dict(mem=HOST), dict(rays=None), dict(hits=None)):
        assert world.call("traverse_async_f32", "f32", over) == INVALID_ARG
        assert world.call("traverse_async_f32", "f32") == OK, world.error()
        assert world.lib.bvhgpu_hits_wait(world.hits("f32")) == OK, world.error()
        off, idx = world.fetch_csr("f32")
        assert np.array_equal(off, world.ref["f32"]["csr"][0]) and np.array_equal(idx, world.ref["f32"]["csr"][1])


def test_result_object_with_a_batch_in_flight_is_refused_by_every_family(world):
    """one rule in every result-object front end: status, message, and the batch in flight completes untouched afterwards"""
    assert world.call("traverse_async_f32", "f32") == OK, world.error()
    for entry in ("traverse_f32", "traverse_async_f32", "traverse_any_f32", "traverse_box_f32", "query_f32"):
        rc = world.call(entry, "f32")
        print(f"{entry} on a result object in flight: status {rc}, message {world.error()!r}")
        assert rc == INVALID_ARG and ASYNC_PENDING in world.error(), entry
    # a second refusal applies as well: the family's own flags / mem test comes first, the shared dtype test later
    assert world.call("traverse_any_f32", "f32", dict(flags=1)) == INVALID_ARG and ANY_FLAGS in world.error()
    assert world.call("query_f32", "f32", dict(mem=7)) == INVALID_ARG and MEM_MSG in world.error()
    vals, shape = np.zeros((N, 3), np.float32), np.zeros(N, np.uint32)
    for kind in ("closest", "any", "box"):
        fetch = getattr(world.lib, "bvhgpu_hits_fetch_" + kind)
        assert fetch(world.hits("f32"), world.ptr(vals), world.ptr(shape), HOST) == INVALID_ARG
        assert "has not been completed: call bvhgpu_hits_wait first" in world.error(), kind
    assert world.lib.bvhgpu_hits_wait(world.hits("f32")) == OK, world.error()
    off, idx = world.fetch_csr("f32")
    assert np.array_equal(off, world.ref["f32"]["csr"][0]) and np.array_equal(idx, world.ref["f32"]["csr"][1])


FETCH_OTHER = {"closest": "traverse was run without BVHGPU_TRAVERSE_CLOSEST", "any": "the result object holds no bvhgpu_traverse_any_* batch",
               "box": "the result object holds no bvhgpu_traverse_box_* batch"}


@pytest.mark.parametrize("held", ["traverse", "traverse_any", "traverse_box"])
def test_fetch_refuses_a_result_object_of_another_kind(world, held):
    """each per-ray fetch on a CSR, an any-hit and a box batch: its own message, and the batch's own fetch still gives the oracle's answer"""
    assert world.call(held + "_f32", "f32") == OK, world.error()
    vals, shape = np.zeros((N, 3), np.float32), np.zeros(N, np.uint32)
    for kind, message in FETCH_OTHER.items():
        if held == "traverse_" + kind:
            continue
        rc = getattr(world.lib, "bvhgpu_hits_fetch_" + kind)(world.hits("f32"), world.ptr(vals), world.ptr(shape), HOST)
        print(f"fetch_{kind} on a {held} batch: status {rc}, message {world.error()!r}")
        assert rc == INVALID_ARG and message in world.error(), (held, kind)
    if held == "traverse":
        off, idx = world.fetch_csr("f32")
        assert np.array_equal(off, world.ref["f32"]["csr"][0]) and np.array_equal(idx, world.ref["f32"]["csr"][1])
    else:
        kind = held.split("_")[1]
        got = world.fetch_rows(kind, "f32", "f32")
        assert got[0].tobytes() == world.ref["f32"][kind][0].tobytes() and np.array_equal(got[1], world.ref["f32"][kind][1])

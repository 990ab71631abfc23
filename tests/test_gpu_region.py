"""Convex-region (plane-set) queries on the GPU (bvhgpu_region_*, bvh_amd/csrc/region.hip): row q is every shape whose box passes the planes
of region q, in FlatBvh::traverse's order, as a CSR without padding, with a byte per shape (BVHGPU_REGION_CLASSIFY) that says whether its box
lies wholly inside.  Every check compares offsets, shapes and bytes byte for byte against the definition restated over the oracle's
FlatNode array (tests/region_ref.py); tests/test_region_cpu.py shows on the oracle alone that the scenes used here cross every branch of the
kernel's schedule (several chunks per region, units killed by an ancestor, the deep-path descent, both `inside` values)."""
import ctypes as C

import numpy as np
import pytest

import fuzz_scenes as fz
import region_ref as rr
from test_gpu_refit import _device, _rb
from test_within_cpu import far_scene

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g
    g.build()
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


@pytest.fixture(scope="module")
def ctx(eng):
    return eng.Context(0)


def _cubes(orc, n, dtype):
    tris, a = orc.create_n_cubes(n)
    return np.ascontiguousarray(a.astype(dtype)), np.ascontiguousarray(tris.astype(dtype))


def _call(eng, tree, planes, classify=True, count_only=False, device=False):
    """region_batch → (offsets u32, indices u32, inside u8 | None, chunks, chunk_entries) as numpy, whichever memory the planes are in"""
    if not device:
        r = eng.region_batch(tree, planes, classify=classify, count_only=count_only)
        assert r["offsets"].dtype == np.uint32 and r["indices"].dtype == np.uint32
        ins = r.get("inside")
        assert (ins is not None) == (classify and not count_only) and (ins is None or ins.dtype == np.uint8)
        return r["offsets"], r["indices"], ins, r["chunks"], r["chunk_entries"]
    import torch
    tp = torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    r = eng.region_batch(tree, tp, classify=classify, count_only=count_only)
    o, s, ins = r["offsets"], r["indices"], r.get("inside")
    assert o.is_cuda and s.is_cuda and o.dtype == torch.int64 and s.dtype == torch.int32
    assert (ins is not None) == (classify and not count_only) and (ins is None or (ins.is_cuda and ins.dtype == torch.uint8))
    on = o.cpu().numpy()
    assert on.min(initial=0) >= 0
    return on.astype(np.uint32), s.cpu().numpy().view(np.uint32), None if ins is None else ins.cpu().numpy(), r["chunks"], r["chunk_entries"]


def _same(got, want, label):
    o, s, ins = got[:3]
    assert o.shape == want[0].shape and o.tobytes() == want[0].tobytes(), (label, "offsets", np.nonzero(o != want[0])[0][:5])
    assert s.shape == want[1].shape, (label, s.shape, want[1].shape)
    bad = np.nonzero(s != want[1])[0]
    assert len(bad) == 0, (label, "shapes differ at", bad[:5], "row", np.searchsorted(o, bad[:5], side="right") - 1, s[bad[:5]], want[1][bad[:5]])
    if ins is not None:
        assert ins.tobytes() == want[2].tobytes(), (label, "inside", np.nonzero(ins != want[2])[0][:5])


def _check(eng, tree, planes, want, label, mems=(False, True)):
    """classified, unclassified and count-only, in host and device memory, against the rows of the definition"""
    chunks = None
    for device in mems:
        got = _call(eng, tree, planes, device=device)
        _same(got, want, (label, device))
        chunks = got[3:]
        assert got[2] is not None
        plain = _call(eng, tree, planes, classify=False, device=device)
        _same(plain, want, (label, device, "no classify"))
        assert plain[2] is None and plain[3:] == chunks
        co = _call(eng, tree, planes, count_only=True, device=device)
        assert co[0].tobytes() == want[0].tobytes() and len(co[1]) == 0 and co[2] is None, (label, device, "count only")
    return chunks


# ---- 1. the rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_region_rows_on_small_trees(eng, orc, ctx, dtype):
    """trees of 1, 2, 3 and 70 cubes (12 .. 840 shapes; the last is two chunks), 40 regions of 1 - 6 planes padded to 6"""
    for n in (1, 2, 3, 70):
        a, _ = _cubes(orc, n, dtype)
        oflat = rr.oracle_tree(a)
        tree = eng.Bvh.from_aabbs(a, ctx).flatten()
        assert tree.nodes.tobytes() == oflat.tobytes()
        planes = rr.random_regions(a, 40, 5)
        want = rr.walk(oflat, a, planes)
        assert want[0][-1] > 0
        chunks, ce = _check(eng, tree, planes, want, (n, "cubes"))
        assert ce == 1024 and chunks == (2 * len(a) - 2 + 1023) // 1024
        t = "float" if dtype == np.float32 else "double"
        assert tree._hits.walk_kernel() == f"bvhgpu::k_region_walk<{t}, false, false, false>"     # (the last call was count-only)


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_main_scene_and_one_region_over_many_chunks(eng, orc, ctx, dtype):
    """900 cubes, 21 598 folded entries, 64 regions (region_ref.main_scene: test_region_cpu qualifies it); then the longest row alone, which
    the walk must spread over at least 8 chunks"""
    m = rr.main_scene(dtype)
    tree = eng.Bvh.from_aabbs(m["aabbs"], ctx).flatten()
    assert tree.nodes.tobytes() == m["flat"].tobytes()
    want = (m["off"], m["idx"], m["ins"])
    chunks, ce = _check(eng, tree, m["planes"], want, "main")
    assert ce == 1024 and chunks == 22
    n = np.diff(m["off"].astype(np.int64))
    for q in (int(np.argmax(n)), int(np.argmin(n)), len(n) - 1):
        one = (np.array([0, n[q]], np.uint32), m["idx"][m["off"][q]:m["off"][q + 1]], m["ins"][m["off"][q]:m["off"][q + 1]])
        for device in (False, True):
            got = _call(eng, tree, m["planes"][q], device=device)                  # a single (m, 4) array is one region
            _same(got, one, ("one region", q, device))
            assert got[3] >= 8 and got[3] * got[4] >= 21598 and got[4] % 64 == 0
    assert n.max() > 3000


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_plane_counts(eng, orc, ctx, dtype):
    """m = 0 (every shape, wholly inside), 1, 6 and 32 on the 70-cube tree.  32 three times: padded, 1 - 32 random planes (mostly empty
    rows), and 32 REAL planes tangent to a ball, whose rows are non-empty and in which every plane index 0 .. 31 alone rejects a shape
    of some region (tests/test_region_cpu.py test_ball_regions_make_every_one_of_32_planes_decide)"""
    a, _ = _cubes(orc, 70, dtype)
    oflat = rr.oracle_tree(a)
    tree = eng.Bvh.from_aabbs(a, ctx).flatten()
    batches = {"m0": np.zeros((5, 0, 4), dtype), "m1": rr.random_regions(a, 30, 1, max_planes=1), "m6": rr.random_regions(a, 30, 2),
               "m32 padded": rr.random_regions(a, 30, 3, pad_to=32), "m32": rr.random_regions(a, 30, 4, max_planes=32),
               "m32 ball": rr.ball_regions(a, rr.BALL_REGIONS, rr.BALL_SEED)}
    assert [b.shape[1] for b in batches.values()] == [0, 1, 6, 32, 32, 32]
    for label, planes in batches.items():
        want = rr.walk(oflat, a, planes)
        _check(eng, tree, planes, want, label)
        if label == "m0":
            assert np.array_equal(np.diff(want[0].astype(np.int64)), [len(a)] * 5) and want[2].all()
        elif label == "m32 ball":
            assert (np.diff(want[0].astype(np.int64)) > 0).sum() >= 200 and (planes[:, :, :3] != 0).all()
        elif label != "m32":
            assert want[0][-1] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_many_regions_few_chunks(eng, orc, ctx, dtype):
    """2 500 regions on the 70-cube tree: two chunks per region, 5 000 units"""
    a, _ = _cubes(orc, 70, dtype)
    oflat = rr.oracle_tree(a)
    tree = eng.Bvh.from_aabbs(a, ctx).flatten()
    planes = rr.random_regions(a, 2500, 6, max_planes=3, pad_to=3)
    want = rr.walk(oflat, a, planes)
    n = np.diff(want[0].astype(np.int64))
    assert (n > 0).sum() > 1000 and (n == 0).sum() > 100
    for device in (False, True):
        got = _call(eng, tree, planes, device=device)
        _same(got, want, ("2500", device))
        assert got[3:] == (2, 1024)
    co = _call(eng, tree, planes, count_only=True)
    assert co[0].tobytes() == want[0].tobytes() and len(co[1]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_one_shape_empty_tree_and_no_regions(eng, orc, ctx, dtype):
    a, _ = _cubes(orc, 1, dtype)
    planes = rr.random_regions(a, 30, 8)
    one = eng.Bvh.from_aabbs(a[:1], ctx).flatten()
    oflat1 = rr.oracle_tree(a[:1])
    assert len(oflat1) == 1
    want = rr.walk(oflat1, a[:1], planes)
    assert 0 < want[0][-1] < 30
    assert _check(eng, one, planes, want, "one shape") == (1, 1024)
    empty = eng.Bvh.from_aabbs(np.zeros((0, 6), dtype), ctx).flatten()
    zero = (np.zeros(31, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert _check(eng, empty, planes, zero, "empty tree") == (0, 0)
    tree = eng.Bvh.from_aabbs(a, ctx).flatten()
    none = (np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert _check(eng, tree, np.zeros((0, 6, 4), dtype), none, "no regions") == (0, 0)


# ---- 2. the anchor that does not go through the new reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_region_aabb_planes_equal_the_aabb_query(eng, orc, ctx, dtype):
    """GPU against GPU: aabb_planes of a box gives query_batch("aabb") of the same box, rows and order, on the boxes of
    test_region_cpu.test_aabb_planes_give_the_aabb_query_rows (half-integer corners: no sum rounds)"""
    a, _ = _cubes(orc, 70, dtype)
    a = np.ascontiguousarray((np.round(a * 2) / 2).astype(dtype))
    tree = eng.Bvh.from_aabbs(a, ctx).flatten()
    rng = np.random.default_rng(3)
    c = a[rng.integers(0, len(a), 30), :3]
    half = rng.integers(1, 400000, size=(30, 3)) / 2
    boxes = np.ascontiguousarray(np.concatenate([c - half, c + half], axis=1).astype(dtype))
    planes = np.stack([eng.aabb_planes(b[:3], b[3:], dtype) for b in boxes])
    qo, qi = tree.query_batch("aabb", boxes)
    r = eng.region_batch(tree, planes)
    assert r["offsets"].tobytes() == np.asarray(qo, np.uint32).tobytes() and r["indices"].tobytes() == np.asarray(qi, np.uint32).tobytes()
    assert len(qi) > 500


# ---- 3. the other kinds of tree ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_region_uploaded_flat_bvh_and_deep_chain(eng, orc, ctx, dtype):
    """from_flat_nodes: the oracle's array of 70 cubes (the UNFOLDED rule, 3 chunks), and a hand-made right-leaning chain of 800 shapes:
    2 398 entries, 3 chunks, the last two behind ancestor paths of several hundred entries — more than the ancestor table holds, so
    their waves descend from entry 0 themselves"""
    a, _ = _cubes(orc, 70, dtype)
    oflat = rr.oracle_tree(a)
    up = eng.FlatBvh.from_flat_nodes(oflat, a, ctx)
    planes = rr.random_regions(a, 40, 5)
    assert _check(eng, up, planes, rr.walk(oflat, a, planes), "uploaded") == (3, 1024)
    t = "float" if dtype == np.float32 else "double"
    assert up._hits.walk_kernel() == f"bvhgpu::k_region_walk<{t}, true, false, false>"
    b = a[:800]
    chain = rr.chain_flat(b)
    ent = rr.entries(chain, b, False)
    assert len(chain) == 2398 and len(rr.ancestors(ent, 1024)) > 64 and len(rr.ancestors(ent, 2048)) > 64
    planes = rr.random_regions(b, 40, 7)
    want = rr.walk(chain, b, planes)
    assert (np.diff(want[0].astype(np.int64)) > 0).sum() >= 10
    up2 = eng.FlatBvh.from_flat_nodes(chain, b, ctx)
    assert _check(eng, up2, planes, want, "chain") == (3, 1024)


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_tree_with_empty_child_bounds(eng, orc, ctx, dtype):
    """boxes so far apart that no bucket wins a split: the engine walks an unfolded mirror of the FlatNode array, the empty navigator
    boxes are never entered, and m = 0 enters everything.  The same tree after scene export / import carries the folded array only: refused"""
    far = far_scene(dtype)[0]
    oflat = rr.oracle_tree(far)
    assert fz.has_empty_child_bounds(oflat)
    tree = eng.Bvh.from_aabbs(far, ctx).flatten()
    planes = rr.random_regions(far, 40, 9)
    want = rr.walk(oflat, far, planes)
    _check(eng, tree, planes, want, "empty child bounds")
    t = "float" if dtype == np.float32 else "double"
    assert tree._hits.walk_kernel() == f"bvhgpu::k_region_walk<{t}, true, false, false>"
    all_of = rr.walk(oflat, far, np.zeros((2, 0, 4), dtype))
    assert all_of[0][-1] == 2 * len(far)
    _check(eng, tree, np.zeros((2, 0, 4), dtype), all_of, "empty child bounds, m = 0")
    blob = np.zeros(tree.scene_nbytes(), np.uint8)
    tree.scene_export(blob)
    imp = eng.FlatBvh.scene_import(blob, len(blob), ctx)
    with pytest.raises(eng.BvhGpuError) as e:
        eng.region_batch(imp, planes)
    assert e.value.status == 1 and "split without SAH winner" in str(e.value)


# ---- 4. first reader of a new generation ---------------------------------------------------------------------------------------------------
def _moved(a, seed):
    """the same shapes somewhere else: every box translated by its own random vector of up to a tenth of the scene"""
    rng = np.random.default_rng(seed)
    ext = float(np.abs(a).max())
    d = (rng.uniform(-0.1, 0.1, size=(len(a), 3)) * ext).astype(a.dtype)
    return np.ascontiguousarray(np.concatenate([a[:, :3] + d, a[:, 3:] + d], axis=1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transition", ["rebuild", "rebuild_async", "refit", "shrink_then_grow"])
def test_region_is_first_reader_of_a_new_generation(eng, orc, ctx, dtype, transition):
    """scene A is read once, then the tree goes to scene B and region_batch is the FIRST call that reads the new arrays (the ancestor
    table is per batch: nothing of A may survive)"""
    a, _ = _cubes(orc, 70, dtype)
    b = _moved(a, 21)
    planes = rr.random_regions(a, 40, 5)
    want_a = rr.walk(rr.oracle_tree(a), a, planes)
    bvh = eng.Bvh.from_aabbs(a, ctx)
    _same(_call(eng, bvh, planes), want_a, "scene A")
    if transition == "rebuild":
        bvh.rebuild(b, flatten=True)
    elif transition == "rebuild_async":
        bvh.rebuild_async(_device(b)).wait()
    elif transition == "refit":
        bvh.refit(b)
    else:
        bvh.rebuild(a[:120], flatten=True)
        bvh.rebuild(b, flatten=True)
    got = _call(eng, bvh, planes)
    if transition == "refit":                                # A's topology with B's boxes: the ORACLE's refit of its own tree of A (the engine's
        flat_b = orc.flatten(orc.refit(orc.build(a).nodes, b))   # array is compared with it afterwards, not used), and (fact 1: refitted
        assert bvh.flatten().nodes.tobytes() == flat_b.tobytes()  # boxes are exact joins) the brute-force sets of B
        for q in range(len(planes)):
            assert sorted(got[1][got[0][q]:got[0][q + 1]].tolist()) == rr.brute(b, planes[q], dtype).tolist(), q
    else:
        flat_b = rr.oracle_tree(b)
    want_b = rr.walk(flat_b, b, planes)
    assert want_b[1].tobytes() != want_a[1].tobytes() and want_b[0].tobytes() != want_a[0].tobytes()   # the old boxes give other rows
    _same(got, want_b, transition)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_region_refusals_leave_everything_untouched(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import DEVICE, DTYPE_MISMATCH, HOST, INVALID_ARG, NOT_FLATTENED, OK, OVERFLOW, ptr
    lib = _lib.load()
    m = rr.main_scene(np.float32)
    a = m["aabbs"]
    tree = eng.Bvh.from_aabbs(a, ctx).flatten()
    planes = np.ascontiguousarray(m["planes"][:4])
    want = rr.walk(m["flat"], a, planes)

    def err():
        return lib.bvhgpu_last_error(ctx._h).decode()

    def refused(rc, status, text, h):
        assert rc == status and text in err(), (rc, err())
        assert not h.value                                   # *hits stays NULL

    h = C.c_void_p()
    p64 = planes.astype(np.float64)
    refused(lib.bvhgpu_region_f64(tree._t, ptr(p64), 4, 6, HOST, 0, C.byref(h)), DTYPE_MISMATCH, "tree dtype differs from plane dtype", h)
    raw = eng.Bvh.from_aabbs(a[:500], ctx)
    refused(lib.bvhgpu_region_f32(raw._t, ptr(planes), 4, 6, HOST, 0, C.byref(h)), NOT_FLATTENED, "call bvhgpu_flatten first", h)
    refused(lib.bvhgpu_region_f32(tree._t, ptr(planes), 1, 33, HOST, 0, C.byref(h)), INVALID_ARG, "BVHGPU_REGION_MAX_PLANES", h)
    refused(lib.bvhgpu_region_f32(tree._t, None, 4, 6, HOST, 0, C.byref(h)), INVALID_ARG, "planes is NULL", h)
    refused(lib.bvhgpu_region_f32(tree._t, ptr(planes), 4, 6, 7, 0, C.byref(h)), INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE", h)
    refused(lib.bvhgpu_region_f32(tree._t, ptr(planes), 4, 6, HOST, 4, C.byref(h)), INVALID_ARG, "region flags", h)
    assert lib.bvhgpu_region_f32(tree._t, ptr(planes), 4, 6, HOST, 0, None) == INVALID_ARG and "hits is NULL" in err()
    assert lib.bvhgpu_region_f32(None, ptr(planes), 4, 6, HOST, 0, C.byref(h)) == INVALID_ARG
    # NULL planes are fine where there is nothing to read
    assert lib.bvhgpu_region_f32(tree._t, None, 3, 0, HOST, 0, C.byref(h)) == OK and h.value
    # a result without CLASSIFY has no inside bytes: refused, outputs untouched; a refused batch leaves the result object as it was
    assert lib.bvhgpu_region_f32(tree._t, ptr(planes), 4, 6, HOST, 0, C.byref(h)) == OK
    total = int(want[0][-1])
    so, ss, si = np.full(5, 0xABABABAB, np.uint32), np.full(total, 0xABABABAB, np.uint32), np.full(total, 0xAB, np.uint8)
    assert lib.bvhgpu_hits_fetch_region(h, ptr(so), ptr(ss), ptr(si), HOST) == INVALID_ARG and "without BVHGPU_REGION_CLASSIFY" in err()
    assert lib.bvhgpu_hits_fetch_region(h, ptr(so), ptr(ss), None, 9) == INVALID_ARG and "mem must be" in err()
    assert (so == 0xABABABAB).all() and (ss == 0xABABABAB).all() and (si == 0xAB).all()
    keep = h.value
    assert lib.bvhgpu_region_f32(tree._t, ptr(planes), 4, 33, HOST, 0, C.byref(h)) == INVALID_ARG and h.value == keep
    assert lib.bvhgpu_region_f32(tree._t, ptr(planes), 4, 6, DEVICE + 5, 0, C.byref(h)) == INVALID_ARG and h.value == keep
    assert lib.bvhgpu_hits_fetch_region(h, ptr(so), ptr(ss), None, HOST) == OK
    assert so.tobytes() == want[0].tobytes() and ss.tobytes() == want[1].tobytes()
    # more than 2^32 - 1 reported shapes: 400 000 regions without planes report all 10 800 shapes each.  The total is checked before anything
    # is sized by it; the result object is then an empty region result
    nr, tot = C.c_size_t(), C.c_uint64()
    assert 400000 * len(a) > 0xFFFFFFFF
    assert lib.bvhgpu_region_f32(tree._t, None, 400000, 0, HOST, 0, C.byref(h)) == OVERFLOW and "2^32-1" in err()
    assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(tot), None) == OK and (nr.value, tot.value) == (0, 0)
    nc, ce = C.c_uint32(7), C.c_uint32(7)
    assert lib.bvhgpu_hits_region_info(h, C.byref(nc), C.byref(ce)) == OK and (nc.value, ce.value) == (0, 0)
    so[:] = 0xABABABAB
    assert lib.bvhgpu_hits_fetch_region(h, ptr(so), None, None, HOST) == OK and so[0] == 0 and (so[1:] == 0xABABABAB).all()
    lib.bvhgpu_hits_destroy(h)


def test_region_result_is_a_kind_of_its_own(eng, orc, ctx):
    """a region result handed to every existing fetch, and every existing kind of result handed to fetch_region: INVALID_ARG, each with a
    message that names the right entry, outputs untouched"""
    from bvh_amd import _lib
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    lib = _lib.load()
    dtype = np.float32
    a, tris = _cubes(orc, 70, dtype)
    tree = eng.Bvh.from_aabbs(a, ctx).flatten()
    tree.set_triangles(tris)
    c = (a[:, :3] + a[:, 3:]) / 2
    tree.set_spheres(np.ascontiguousarray(np.concatenate([c, np.full((len(a), 1), 0.5, dtype)], axis=1)))
    rays = _rb(eng, np.ascontiguousarray(orc.create_rays(0, 500)))
    pts = np.ascontiguousarray(c[:50])
    planes = rr.random_regions(a, 10, 5)
    so, ss, sv = np.full(600, 0xABABABAB, np.uint32), np.full(200000, 0xABABABAB, np.uint32), np.full((200000, 3), 7.0, dtype)
    h = tree._hits

    def untouched():
        return (so == 0xABABABAB).all() and (ss == 0xABABABAB).all() and (sv == 7.0).all()

    others = {
        "traverse": (lambda: tree.traverse_batch(rays), "no bvhgpu_region_"),
        "query": (lambda: tree.query_batch("aabb", a[:50]), "no bvhgpu_region_"),
        "closest": (lambda: tree.closest_hits(rays), "bvhgpu_hits_fetch_closest"),
        "any": (lambda: tree.any_hits(rays), "bvhgpu_hits_fetch_any"),
        "box": (lambda: tree.closest_box_hits(rays), "bvhgpu_hits_fetch_box"),
        "sphere": (lambda: tree.closest_sphere_hits(rays), "bvhgpu_hits_fetch_sphere"),
        "allhits": (lambda: tree.allhits_batch(rays), "bvhgpu_hits_fetch_allhits"),
        "within": (lambda: tree.within_batch(pts, 100.0), "bvhgpu_hits_fetch_within"),
    }
    for kind, (run, text) in others.items():
        run()
        assert lib.bvhgpu_hits_fetch_region(h.h, ptr(so), ptr(ss), None, HOST) == INVALID_ARG, kind
        assert text in lib.bvhgpu_last_error(ctx._h).decode(), (kind, lib.bvhgpu_last_error(ctx._h).decode())
        assert lib.bvhgpu_hits_region_info(h.h, None, None) == INVALID_ARG, kind
        assert untouched(), kind
    want = rr.walk(rr.oracle_tree(a), a, planes)
    got = _call(eng, tree, planes)
    _same(got, want, "region after every other kind")
    fetches = {
        "fetch": lambda: lib.bvhgpu_hits_fetch(h.h, ptr(so), ptr(ss), None, HOST),
        "triangles": lambda: lib.bvhgpu_hits_fetch_triangles(h.h, ptr(sv), HOST),
        "closest": lambda: lib.bvhgpu_hits_fetch_closest(h.h, ptr(sv), ptr(ss), HOST),
        "any": lambda: lib.bvhgpu_hits_fetch_any(h.h, ptr(sv), ptr(ss), HOST),
        "box": lambda: lib.bvhgpu_hits_fetch_box(h.h, ptr(sv), ptr(ss), HOST),
        "sphere": lambda: lib.bvhgpu_hits_fetch_sphere(h.h, ptr(sv), ptr(ss), HOST),
        "allhits": lambda: lib.bvhgpu_hits_fetch_allhits(h.h, ptr(so), ptr(ss), ptr(sv), HOST),
        "within": lambda: lib.bvhgpu_hits_fetch_within(h.h, ptr(so), ptr(ss), ptr(sv), HOST),
        "device": lambda: lib.bvhgpu_hits_device(h.h, None, None, None),
    }
    for name, f in fetches.items():
        assert f() == INVALID_ARG, name
        assert "bvhgpu_hits_fetch_region" in lib.bvhgpu_last_error(ctx._h).decode(), name
        assert untouched(), name
    # and the result object goes on to the next kind of batch
    off, idx, _, _ = tree.traverse_batch(rays)
    ooff, oidx, _, _ = orc.traverse_flat(rr.oracle_tree(a), a, np.ascontiguousarray(orc.create_rays(0, 500)))
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    assert lib.bvhgpu_hits_wait(h.h) == OK

"""The oracle's refit (orc.refit: fix_aabbs_ascending, optimization.rs:355-391, applied to every node) against an independent numpy
restatement — every child box is the min / max over the moved AABBs of the leaves below that child, the leaf sets read off the node array
itself, zeros ordered -0 < +0 — on the trees that exercise every builder tier: identical centroids (the halving path), the exponentially
spaced deep tree, the band where surface areas overflow (splits without SAH winner leave empty child boxes), ragged sizes around 64 and
1024, and boxes with signed zeros.  orc.refit is the reference of tests/test_gpu_refit.py, which takes its scenes from here."""
import numpy as np
import pytest

from oracle import orc

RAGGED = (2, 3, 65, 1025, 4097)
SCENES = ("dup", "same", "deep", "overflow", "zeros") + tuple(f"ragged{n}" for n in RAGGED)


def overflow_scale(dtype):
    """the band of test_fuzz_all_queries in which surface areas overflow"""
    return 2.0 ** (70 if dtype == np.float32 else 520)


def scene(name, dtype):
    """(aabbs, scale) of a named scene: what the parity tests of the builders use, at their sizes"""
    if name in ("dup", "same"):       # test_parity_degenerate_and_collisions
        rng = np.random.default_rng(11)
        n = 3000
        lo = rng.integers(-20, 20, size=(n, 3)).astype(dtype)
        ext = rng.integers(0, 3, size=(n, 3)).astype(dtype)
        lo[500:1400] = lo[500]; ext[500:1400] = ext[500]
        lo[2000:2040] = lo[2000]; ext[2000:2040] = ext[2000]
        aabbs = np.concatenate([lo, lo + ext], axis=1)
        return (aabbs, 1.0) if name == "dup" else (np.tile(aabbs[500], (777, 1)), 1.0)
    if name == "deep":                # test_parity_unbalanced_deep_tree
        n = 12000
        x = np.float32(1.004) ** np.arange(n, dtype=np.float32)
        lo = np.stack([x, np.zeros(n, np.float32), np.zeros(n, np.float32)], axis=1)
        return np.concatenate([lo, lo + np.float32(0.5)], axis=1).astype(dtype), 1.0
    if name == "overflow":
        rng = np.random.default_rng(70)
        sc = overflow_scale(dtype)
        lo = rng.uniform(-50, 50, size=(2000, 3))
        ext = rng.uniform(0, 2, size=(2000, 3))
        return (np.concatenate([lo, lo + ext], axis=1) * sc).astype(dtype), sc
    if name == "zeros":
        aabbs = orc.create_n_cubes(40)[1].astype(dtype)
        return aabbs, 1.0
    n = int(name[len("ragged"):])     # test_parity_ragged_sizes
    rng = np.random.default_rng(n)
    lo = rng.uniform(-100, 100, size=(n, 3)).astype(dtype)
    ext = rng.uniform(0, 10, size=(n, 3)).astype(dtype)
    return np.concatenate([lo, lo + ext], axis=1), 1.0


def moved(name, aabbs, scale, dtype, seed):
    """(moved AABBs, shift per shape): every shape shifted rigidly by up to three units of the scene, as test_refit_moved_shapes moves them;
    the scene "zeros" also gets that test's signed zeros"""
    n = len(aabbs)
    rng = np.random.default_rng(seed)
    shift = (rng.uniform(-3, 3, size=(n, 1, 3)) * scale).astype(dtype)
    a1 = (aabbs.reshape(n, 2, 3) + shift).reshape(n, 6)
    if name == "zeros":
        a1[::7, 0] = -0.0; a1[::7, 3] = 0.0
        a1[3::11, 1] = 0.0; a1[3::11, 4] = 0.0
    assert np.isfinite(a1).all()
    return np.ascontiguousarray(a1), shift


def has_empty_child(nodes) -> bool:
    """some inner node holds an empty child box (a split without SAH winner, bvh_node.rs:114-124)"""
    inner = nodes[nodes["shape"] == orc.NONE]
    return bool(np.any(inner["l_min"] > inner["l_max"]) or np.any(inner["r_min"] > inner["r_max"]))


def _key(a):
    """floats as integers of the same order, -0 below +0 (an involution: applying it to the keys gives the floats back)"""
    i = np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64)
    return np.where(i >= 0, i, i ^ np.iinfo(i.dtype).max)


def restated_refit(nodes, aabbs):
    """the refitted node array without any join of boxes: the leaves below every node from a walk of l / r, then per child one min / max
    over the AABBs of those leaves"""
    out = nodes.copy()
    nn = len(nodes)
    if nn <= 1:
        return out
    l, r, shape = nodes["l"].tolist(), nodes["r"].tolist(), nodes["shape"].tolist()
    start, count, order = [0] * nn, [0] * nn, []
    stack = [(0, False)]
    while stack:
        i, done = stack.pop()
        if done:
            count[i] = len(order) - start[i]
        elif shape[i] != orc.NONE:
            start[i] = len(order); count[i] = 1; order.append(shape[i])
        else:
            start[i] = len(order)
            stack += [(i, True), (r[i], False), (l[i], False)]
    assert sorted(order) == list(range(len(aabbs)))
    k = _key(aabbs)[np.asarray(order)]
    k = np.concatenate([k, k[-1:]])                                     # (reduceat wants every index inside the array)
    inner = np.flatnonzero(nodes["shape"] == orc.NONE)
    start, count = np.asarray(start), np.asarray(count)
    for side, lo_f, hi_f in (("l", "l_min", "l_max"), ("r", "r_min", "r_max")):
        c = nodes[side][inner]
        assert (count[c] > 0).all()
        pairs = np.stack([start[c], start[c] + count[c]], axis=1).reshape(-1)
        out[lo_f][inner] = _key(np.minimum.reduceat(k[:, :3], pairs)[::2]).view(aabbs.dtype)
        out[hi_f][inner] = _key(np.maximum.reduceat(k[:, 3:], pairs)[::2]).view(aabbs.dtype)
    return out


def test_key_orders_signed_zeros():
    for dtype in (np.float32, np.float64):
        v = np.array([-np.inf, -1.0, -np.finfo(dtype).smallest_subnormal, -0.0, 0.0, np.finfo(dtype).smallest_subnormal, 2.0, np.inf], dtype)
        k = _key(v)
        assert (np.diff(k) > 0).all()
        assert _key(k).view(dtype).tobytes() == v.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", SCENES)
def test_oracle_refit_equals_restatement(name, dtype):
    a0, sc = scene(name, dtype)
    n = len(a0)
    built = orc.build(a0).nodes
    if not has_empty_child(built):                                      # (an empty child box contains nothing: not consistent as built)
        assert orc.check_tree(built, a0) == 0
    # refit with the boxes of the build: the built tree exactly where every split had an SAH winner — an empty child box becomes the exact join
    same = orc.refit(built, a0)
    assert same.tobytes() == restated_refit(built, a0).tobytes()
    assert orc.check_tree(same, a0) == 0
    assert (same.tobytes() == built.tobytes()) == (not has_empty_child(built)), (name, has_empty_child(built))
    assert not has_empty_child(same)
    if name == "overflow" or (name == "deep" and dtype == np.float32):
        assert has_empty_child(built)                                   # the scenes are there for this
    # moved shapes, twice on the same tree
    cur = built
    for seed in (41, 42):
        a1, _ = moved(name, a0, sc, dtype, seed)
        new = orc.refit(cur, a1)
        assert new.tobytes() == restated_refit(cur, a1).tobytes(), (name, seed)
        assert new.tobytes() == restated_refit(built, a1).tobytes()    # ... which forgets the boxes it finds
        assert orc.check_tree(new, a1) == 0
        for f in ("parent", "l", "r", "shape"):
            assert np.array_equal(new[f], built[f]), f
        leaves = new["shape"] != orc.NONE                               # a leaf stores no box (bvh_node.rs:38-46): untouched
        assert new[leaves].tobytes() == built[leaves].tobytes()
        if name == "zeros" and n >= 12:
            boxes = np.concatenate([new[f] for f in ("l_min", "l_max", "r_min", "r_max")])
            assert np.any((boxes == 0) & np.signbit(boxes)) and np.any((boxes == 0) & ~np.signbit(boxes))
        cur = new

"""Reference for the ray queries of an instance set of BOX or SPHERE leaves (include/bvh_mi355x.h, bvhgpu_instances_create_leaf_*):
tests/instances_ref.py's Scene with the leaf stage swapped.  The two levels are walked as Scene.trace walks them — the same object_rays, the
same orc.traverse_flat on the top level and on every member — and the record of a candidate (instance, shape) is
  "sphere"  sphere_ref.ray_sphere on the object-space ray and the member's sphere: {distance, exit};
  "box"     the t-slice of the object-space ray on the shape's own AABB as the oracle's traverse returns it (what box_match is given):
            {enter, exit}.
The candidate table keeps Scene.trace's layout — vals[., 3] with the third scalar 0 — so that instances_allhits_ref.rows,
instances_khits_ref.definition / incremental and instances_masks_ref's filters run over it unchanged; the engine's records are the first
two columns.  The scenes of tests/test_instances_leaf_cpu.py and tests/test_gpu_instances_leaf.py are drawn here too."""
import numpy as np

import instances_ref as ir
from instances_masks_ref import select
from oracle import orc
from sphere_ref import ray_sphere, tmax_draw

NONE = 0xFFFFFFFF
LEAVES = ("box", "sphere")
N_RAYS = 1500
N_INSIDE = 120    # the last rays of a batch start inside an instance's ellipsoid
SPREAD = 6.0      # tests/test_instances_cpu.py's: translations U(-SPREAD, SPREAD)^3 around members of extent ~ +-3.5, so world boxes overlap
SIZES = (1, 2, 37)
MEMBER_SHAPES = (1, 12, 240)


class LeafScene(ir.Scene):
    """trees: [(aabbs[n,6], spheres[n,4])] in T (the spheres are read by leaf == "sphere" only)"""

    def __init__(self, trees, tree_of, xforms, ft, leaf):
        assert leaf in LEAVES
        self.leaf = leaf
        self.ft = np.dtype(ft).type
        self.trees = [(np.ascontiguousarray(a, dtype=ft).reshape(-1, 6), np.ascontiguousarray(s, dtype=ft).reshape(-1, 4)) for a, s in trees]
        self.flats = [orc.flatten(orc.build(a).nodes) for a, _ in self.trees]
        self.tree_of = np.asarray(tree_of, dtype=np.int64).reshape(-1)
        self.bounds = np.stack([ir.tree_bounds(a) for a, _ in self.trees]) if self.trees else np.zeros((0, 6), dtype=ft)
        self.pose(xforms)

    def records(self, member, orays, off, idx):
        """the leaf stage for every entry of the member's CSR → vals[total, 3], third scalar 0"""
        aabbs, spheres = self.trees[member]
        cnt = np.diff(off.astype(np.int64))
        row = np.repeat(np.arange(len(cnt)), cnt)
        out = np.zeros((len(idx), 3), dtype=self.ft)
        if self.leaf == "sphere":
            out[:, :2] = ray_sphere(np.ascontiguousarray(orays["o"][row]), np.ascontiguousarray(orays["d"][row]),
                                    np.ascontiguousarray(spheres[idx.astype(np.int64)]))
        else:
            _, idx2, ts, _ = orc.traverse_flat(self.flats[member], aabbs, orays, want_t=True)
            assert np.array_equal(idx2, idx)
            out[:, :2] = ts
        return out

    def trace(self, rays, tmax=None):
        """Scene.trace's dict (top, table, closest, first) with this scene's leaf stage"""
        ft = self.ft
        n = len(rays)
        rays = np.ascontiguousarray(rays)
        toff, tidx, _, _ = orc.traverse_flat(self.top, self.w, rays)
        ray_of = np.repeat(np.arange(n), np.diff(toff.astype(np.int64)))
        pos_of = np.arange(len(tidx)) - toff.astype(np.int64)[ray_of]
        c_ray, c_pos, c_k, c_inst, c_shape, c_vals = [], [], [], [], [], []
        for i in np.unique(tidx):
            sel = np.nonzero(tidx == i)[0]
            rid = ray_of[sel]
            orays = self.object_rays(rays[rid], int(i))
            member = int(self.tree_of[i])
            off, idx, _, _ = orc.traverse_flat(self.flats[member], self.trees[member][0], orays)
            cnt = np.diff(off.astype(np.int64))
            c_ray.append(np.repeat(rid, cnt)); c_pos.append(np.repeat(pos_of[sel], cnt))
            c_k.append(np.arange(len(idx)) - np.repeat(off.astype(np.int64)[:-1], cnt))
            c_inst.append(np.full(len(idx), i, dtype=np.uint32)); c_shape.append(idx.astype(np.uint32))
            c_vals.append(self.records(member, orays, off, idx))
        if c_ray:
            c_ray, c_pos, c_k = np.concatenate(c_ray), np.concatenate(c_pos), np.concatenate(c_k)
            c_inst, c_shape, c_vals = np.concatenate(c_inst), np.concatenate(c_shape), np.concatenate(c_vals)
            order = np.lexsort((c_k, c_pos, c_ray))
            c_ray, c_inst, c_shape, c_vals = c_ray[order], c_inst[order], c_shape[order], c_vals[order]
        else:
            c_ray = np.zeros(0, dtype=np.int64); c_inst = np.zeros(0, dtype=np.uint32); c_shape = np.zeros(0, dtype=np.uint32)
            c_vals = np.zeros((0, 3), dtype=ft)
        cand_off = np.concatenate([[0], np.cumsum(np.bincount(c_ray, minlength=n))]).astype(np.int64)
        table = dict(ray=c_ray, instance=c_inst, shape=c_shape, vals=c_vals, cand_off=cand_off)
        return dict(top=(toff, tidx), table=table, closest=select(table, n, tmax, ft, False), first=select(table, n, tmax, ft, True))


def two(res):
    """a reference result with vals[..., 3] → the engine's: the first two scalars (the third is 0 for these kinds)"""
    res = tuple(res)
    k = [i for i, a in enumerate(res) if a.dtype.kind == "f"][0]
    assert not res[k][..., 2].any()
    return res[:k] + (np.ascontiguousarray(res[k][..., :2]),) + res[k + 1:]


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------
def member_trees(dtype):
    """members of 1, 12 and 240 spheres inside [-3, 3]^3, each shape's box the box of its sphere computed in dtype → [(aabbs, spheres)]"""
    out = []
    for m, (rlo, rhi) in zip(MEMBER_SHAPES, ((1.5, 1.5001), (0.4, 0.9), (0.25, 0.7))):
        rng = np.random.default_rng(50 + m)
        r = rng.uniform(rlo, rhi, size=(m, 1))
        c = rng.uniform(-3, 3, size=(m, 3)) * (1 - r / 3)
        s = np.ascontiguousarray(np.concatenate([c, r], axis=1).astype(dtype))
        out.append((np.ascontiguousarray(np.concatenate([s[:, :3] - s[:, 3:], s[:, :3] + s[:, 3:]], axis=1)), s))
    return out


def tree_slots(n, seed):
    """which member each instance copies: the one-instance set is the 240-shape member, larger sets start 1, 12, 240 and go on at random"""
    if n == 1:
        return np.array([2], dtype=np.uint32)
    of = np.random.default_rng(seed).integers(0, 3, size=n)
    of[:min(n, 3)] = [0, 1, 2][:min(n, 3)]
    return of.astype(np.uint32)


def leaf_rays(trees, tree_of, x, n, dtype, seed):
    """tests/test_instances_cpu.py's cluster rays, the last N_INSIDE of them starting INSIDE a sphere of an instance (at the world image of
    a point half a radius off its centre) in a random direction"""
    from test_instances_cpu import cluster_rays
    rays = cluster_rays(orc, n, dtype, seed)
    rng = np.random.default_rng(seed + 1)
    o = np.array(rays["o"], dtype=np.float64)
    d = np.array(rays["d"], dtype=np.float64)
    for j in range(n - N_INSIDE, n):
        i = int(rng.integers(0, len(tree_of)))
        s = trees[int(tree_of[i])][1]
        sp = s[int(rng.integers(0, len(s)))].astype(np.float64)
        u = rng.normal(size=3)
        p = sp[:3] + 0.5 * sp[3] * u / np.linalg.norm(u)
        o[j] = x[i].astype(np.float64)[:, :3] @ p + x[i].astype(np.float64)[:, 3]
        d[j] = rng.normal(size=3)
    return orc.make_rays(o.astype(dtype), d.astype(dtype), dtype)


_CASES = {}


def case(dtype, n, leaf):
    """the set of `n` instances with `leaf` leaves: its rays, drawn tmax, per-ray masks and reference answers (computed once, never modified)"""
    from test_instances_cpu import transforms
    key = (np.dtype(dtype).name, n, leaf)
    if key not in _CASES:
        trees = member_trees(dtype)
        of, x = tree_slots(n, 100 + n), transforms(n, dtype, 200 + n)
        sc = LeafScene(trees, of, x, dtype, leaf)
        rays = leaf_rays(trees, of, x, N_RAYS, dtype, 300 + n)
        free = sc.trace(rays)
        rng = np.random.default_rng(400 + n)
        tmax = tmax_draw(rng, free["closest"][0][:, 0], dtype)
        inst_mask = rng.integers(1, 16, size=n).astype(np.uint32)
        ray_mask = rng.integers(0, 16, size=N_RAYS).astype(np.uint32)
        _CASES[key] = dict(trees=trees, tree_of=of, x=x, scene=sc, rays=rays, tmax=tmax, free=free, cut=sc.trace(rays, tmax),
                           inst_mask=inst_mask, ray_mask=ray_mask)
    return _CASES[key]

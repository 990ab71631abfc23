"""Instanced scenes over the C ABI (include/bvh_mi355x.h, bvhgpu_instances_*): ray queries over transformed copies of trees.

An instance is (member tree, 3x4 object -> world transform); the set keeps a top-level tree over the instances' world boxes.  Everything
that computes runs on the GPU; this file only marshals, through api._rows_in / api._side_in like every other batch call.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib, api
from ._lib import DEVICE, NONE, BvhGpuError, check, ptr
from .api import Context, RayBatch, _Typed
from .region import _plane_dims


class InstancesTreeForm:
    """The nearest-first ("tree form") point queries of an instance set, which Instances inherits: they read the BvhNode arrays of the top
    level and of the members where every other entry of the set reads the flattened arrays.  Kept apart from Instances' own methods so
    that the call recording of those (tests/golden/instances_calls.json) stays as it is; tests/test_instances_tree_marshal_cpu.py holds
    these two to what they hand to the C ABI."""

    def knearest_tree_batch(self, points, k: int, max_dist=None):
        """bvhgpu_instances_knearest_tree_*: the rows of knearest_batch found nearest child first on both levels — the top-level BvhNode
        array with the world point, every member's with the point in the object's frame — so the first pairs a point meets are near ones
        and the bound that prunes is small from the start.  Equal distances stay in the order this walk meets them, which is not knearest_batch's: the two
        may name different pairs at tied distances; their distances agree.
        max_dist: None, a scalar (the same limit for every point) or n values in the points' memory — a numpy array for numpy points, a
        torch GPU tensor for tensor points.  Nothing farther than max_dist[i] enters row i (d <= max_dist[i]^2); a negative or NaN limit
        gives a row of padding, 0 keeps only distance 0.  Every member must have been built here (a Bvh's flatten(), not an uploaded
        FlatBvh or an imported scene: those have no BvhNode array and raise INVALID_ARG; knearest_batch takes them).
        points / k / returns: as knearest_batch."""
        k = int(k)
        rows = k if 1 <= k <= _lib.INSTANCES_KNN_MAX_K else 0   # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        keep, pp, n, mem = api._rows_in(points, 3, self.ft, "point")
        _m, mp = api._side_in(max_dist, keep, n, mem, self.ft, "max_dist", "points", scalar_ok=True)
        out, (ip, sp, dp) = api._out_cols(keep.device if mem == DEVICE else None, self.ft, ((n, rows), "index"), ((n, rows), "index"), ((n, rows), "float"))
        fn = getattr(_lib.load(), f"bvhgpu_instances_knearest_tree_{self.sfx}")
        check(fn(self._s, pp, n, mem, k & 0xFFFFFFFF, mp, ip, sp, dp), self.ctx._h)
        return tuple(out)

    def nearest_tree_batch(self, points, max_dist=None):
        """knearest_tree_batch with k = 1 and the last axis dropped: (instance[n], shape[n], dist[n]); a point with nothing within its
        limit, and a set without instances, give NONE, NONE and +inf."""
        inst, shape, dist = self.knearest_tree_batch(points, 1, max_dist)
        return inst[:, 0], shape[:, 0], dist[:, 0]


class InstancesMasks:
    """Per-instance visibility masks (bvhgpu_instances_set_masks and the *_masked_* ray entries), which Instances inherits.  Every instance
    i carries a 32-bit mask M[i] (all ones in a new set), a masked batch one 32-bit mask R[j] per ray, and instance i is visible to ray j
    iff M[i] & R[j] != 0.  A masked method answers what its unmasked counterpart would over the set without the instances hidden from
    that ray — same order of ties, same bits — and the walk passes over a hidden instance without entering its tree.  The masks are no
    part of the pose: update() keeps them, setting them commits nothing.  Every other method of the set (closest_hits, any_hits, occluded,
    khits_batch, allhits_batch and the unmasked point and region queries) ignores the masks: every instance is visible to it; the point
    and region queries have masked forms of their own in InstancesMaskedQueries.
    Kept apart from Instances' own methods so that the call recording of those (tests/golden/instances_calls.json) stays as it is;
    tests/test_instances_masks_marshal_cpu.py holds these to what they hand to the C ABI.

    ray_mask, everywhere: None (all ones for every ray), a Python int in [0, 2^32) (the same mask for every ray) or n values in the rays'
    memory — numpy integers for HOST rays, a torch.int32 tensor on the rays' device for rays in HBM (its bits are the masks)."""

    def set_masks(self, masks) -> "InstancesMasks":
        """bvhgpu_instances_set_masks: one 32-bit mask per instance — numpy integers / a list (HOST) or a torch.int32 GPU tensor — or None
        for all ones again.  In place when it returns; needs no update() and is allowed on a set whose last update failed."""
        if masks is None:
            mp, mem = None, _lib.HOST
        elif api._is_device_tensor(masks):
            keep, mp = api._mask_in(masks, masks, self.n, DEVICE, "masks", "instances")
            mem = DEVICE
            api._torch_sync(keep.device)
        else:
            keep, mp = api._mask_in(np.asarray(masks), None, self.n, _lib.HOST, "masks", "instances")
            mem = _lib.HOST
        check(_lib.load().bvhgpu_instances_set_masks(self._s, mp, self.n, mem), self.ctx._h)
        return self

    @property
    def masks(self) -> np.ndarray:
        """M, uint32[n]"""
        out = np.zeros(self.n, dtype=np.uint32)
        check(_lib.load().bvhgpu_instances_masks(self._s, ptr(out), _lib.HOST), self.ctx._h)
        return out

    def _trace_masked(self, rays: RayBatch, ray_mask, tmax, flags: int):
        self._check_rays(rays)
        _keep, tp = api._side_in(tmax, rays.device, rays.n, rays.mem, self.ft, "tmax", "rays")
        _mk, mp = api._mask_in(ray_mask, rays.device, rays.n, rays.mem, "ray_mask", "rays")
        n = rays.n
        out, (vp, ip, sp) = api._out_cols(rays.device.device if rays.mem == DEVICE else None, self.ft, ((n, _lib.LEAF_WIDTH[_lib.LEAF_KINDS[self.leaf]]), "float"), (n, "index"), (n, "index"))
        fn = getattr(_lib.load(), f"bvhgpu_instances_trace_masked_{self.sfx}")
        check(fn(self._s, rays._ptr(), tp, mp, n, rays.mem, flags, vp, ip, sp), self.ctx._h)
        return tuple(out)

    def closest_hits_masked(self, rays: RayBatch, ray_mask, tmax=None):
        """closest_hits over the instances visible to each ray; returns what closest_hits returns"""
        return self._trace_masked(rays, ray_mask, tmax, 0)

    def any_hits_masked(self, rays: RayBatch, ray_mask, tmax=None):
        """any_hits over the instances visible to each ray: the first candidate in walk order that is left; returns what any_hits returns"""
        return self._trace_masked(rays, ray_mask, tmax, _lib.TRAVERSE_FIRST)

    def occluded_masked(self, rays: RayBatch, ray_mask, tmax=None):
        """bool[n]: does segment i hit any triangle of any instance visible to ray i"""
        _, inst, _ = self.any_hits_masked(rays, ray_mask, tmax)
        return inst != (NONE if isinstance(inst, np.ndarray) else -1)

    def khits_masked_batch(self, rays: RayBatch, k: int, ray_mask, tmax=None):
        """bvhgpu_instances_khits_masked_*: khits_batch over the instances visible to each ray; k and the returns are khits_batch's"""
        self._check_rays(rays)
        k = int(k)
        rows = k if 1 <= k <= _lib.INSTANCES_KHITS_MAX_K else 0   # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        _keep, tp = api._side_in(tmax, rays.device, rays.n, rays.mem, self.ft, "tmax", "rays")
        _mk, mp = api._mask_in(ray_mask, rays.device, rays.n, rays.mem, "ray_mask", "rays")
        n = rays.n
        out, (ip, sp, vp) = api._out_cols(rays.device.device if rays.mem == DEVICE else None, self.ft,
                                          ((n, rows), "index"), ((n, rows), "index"), ((n, rows, _lib.LEAF_WIDTH[_lib.LEAF_KINDS[self.leaf]]), "float"))
        fn = getattr(_lib.load(), f"bvhgpu_instances_khits_masked_{self.sfx}")
        check(fn(self._s, rays._ptr(), tp, mp, n, rays.mem, k & 0xFFFFFFFF, ip, sp, vp), self.ctx._h)
        return tuple(out)

    def allhits_masked_batch(self, rays: RayBatch, ray_mask, tmax=None, sort: bool = True, count_only: bool = False) -> dict:
        """bvhgpu_instances_allhits_masked_*: allhits_batch over the instances visible to each ray; sort, count_only and the returns are
        allhits_batch's"""
        self._check_rays(rays)
        _keep, tp = api._side_in(tmax, rays.device, rays.n, rays.mem, self.ft, "tmax", "rays")
        _mk, mp = api._mask_in(ray_mask, rays.device, rays.n, rays.mem, "ray_mask", "rays")
        flags = (0 if sort else _lib.INSTANCES_ALLHITS_LIST_ORDER) | (_lib.INSTANCES_ALLHITS_COUNT_ONLY if count_only else 0)
        offsets, instance, shape, vals = self._csr("allhits_masked", (rays._ptr(), tp, mp, rays.n, rays.mem, flags), rays.n,
                                                   rays.device.device if rays.mem == DEVICE else None, count_only,
                                                   ((), "index"), ((), "index"), ((_lib.LEAF_WIDTH[_lib.LEAF_KINDS[self.leaf]],), "float"), fetch="instances_allhits")
        if count_only:
            return dict(offsets=offsets)
        return dict(offsets=offsets, instance=instance, shape=shape, vals=vals)


class InstancesMaskedQueries:
    """The point and region queries over the instances visible to each row (bvhgpu_instances_within_masked_*, _knearest_masked_*,
    _knearest_tree_masked_*, _region_masked_*), which Instances inherits.  M[i] is InstancesMasks' instance mask; a masked point batch
    carries one 32-bit mask per point, a masked region batch one per region, and instance i is visible to row j iff M[i] & mask[j] != 0.
    Each method answers what its unmasked counterpart would over the set without the instances hidden from that row — same order of
    ties, same bits, same outputs — and the walk passes over a hidden instance at its top-level leaf.  For k-nearest that is NOT a filter
    of the unmasked row: the k slots go to visible pairs only.  The unmasked methods keep ignoring the masks.
    Kept apart from Instances' own methods so that the call recording of those (tests/golden/instances_calls.json) stays as it is;
    tests/test_instances_point_masks_marshal_cpu.py holds these to what they hand to the C ABI.

    point_mask / region_mask, everywhere: None (all ones for every row), a Python int in [0, 2^32) (the same mask for every row) or n
    values in the main input's memory — numpy integers for HOST input, a torch.int32 tensor on the input's device for input in HBM."""

    def within_masked_batch(self, points, max_dist, point_mask, sort: bool = True, count_only: bool = False) -> dict:
        """bvhgpu_instances_within_masked_*: within_batch over the instances visible to each point — its row without the hidden instances'
        pairs; sort, count_only and the returns are within_batch's"""
        api._needs(max_dist, "within_masked_batch needs max_dist (a scalar or one value per point)")
        keep, pp, n, mem = api._rows_in(points, 3, self.ft, "point")
        _m, mp = api._side_in(max_dist, keep, n, mem, self.ft, "max_dist", "points", scalar_ok=True)
        _mk, kp = api._mask_in(point_mask, keep, n, mem, "point_mask", "points")
        flags = (0 if sort else _lib.INSTANCES_WITHIN_LIST_ORDER) | (_lib.INSTANCES_WITHIN_COUNT_ONLY if count_only else 0)
        offsets, instance, shape, dist = self._csr("within_masked", (pp, mp, kp, n, mem, flags), n, keep.device if mem == DEVICE else None, count_only,
                                                   ((), "index"), ((), "index"), ((), "float"), fetch="instances_within")
        if count_only:
            return dict(offsets=offsets)
        return dict(offsets=offsets, instance=instance, shape=shape, dist=dist)

    def knearest_masked_batch(self, points, k: int, point_mask):
        """bvhgpu_instances_knearest_masked_*: knearest_batch over the instances visible to each point — the first k of the stable ascending
        sort of all VISIBLE pairs (a hidden pair takes no slot and moves no bound); k and the returns are knearest_batch's"""
        k = int(k)
        rows = k if 1 <= k <= _lib.INSTANCES_KNN_MAX_K else 0   # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        keep, pp, n, mem = api._rows_in(points, 3, self.ft, "point")
        _mk, kp = api._mask_in(point_mask, keep, n, mem, "point_mask", "points")
        out, (ip, sp, dp) = api._out_cols(keep.device if mem == DEVICE else None, self.ft, ((n, rows), "index"), ((n, rows), "index"), ((n, rows), "float"))
        fn = getattr(_lib.load(), f"bvhgpu_instances_knearest_masked_{self.sfx}")
        check(fn(self._s, pp, kp, n, mem, k & 0xFFFFFFFF, ip, sp, dp), self.ctx._h)
        return tuple(out)

    def nearest_masked_batch(self, points, point_mask):
        """knearest_masked_batch with k = 1 and the last axis dropped: (instance[n], shape[n], dist[n]); a point that sees no instance gives
        NONE, NONE and +inf"""
        inst, shape, dist = self.knearest_masked_batch(points, 1, point_mask)
        return inst[:, 0], shape[:, 0], dist[:, 0]

    def knearest_tree_masked_batch(self, points, k: int, point_mask, max_dist=None):
        """bvhgpu_instances_knearest_tree_masked_*: knearest_tree_batch's descent over the same top level, a hidden instance's leaf
        contributing nothing; ties stay in that walk's order.  k, max_dist and the returns are knearest_tree_batch's"""
        k = int(k)
        rows = k if 1 <= k <= _lib.INSTANCES_KNN_MAX_K else 0   # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        keep, pp, n, mem = api._rows_in(points, 3, self.ft, "point")
        _m, mp = api._side_in(max_dist, keep, n, mem, self.ft, "max_dist", "points", scalar_ok=True)
        _mk, kp = api._mask_in(point_mask, keep, n, mem, "point_mask", "points")
        out, (ip, sp, dp) = api._out_cols(keep.device if mem == DEVICE else None, self.ft, ((n, rows), "index"), ((n, rows), "index"), ((n, rows), "float"))
        fn = getattr(_lib.load(), f"bvhgpu_instances_knearest_tree_masked_{self.sfx}")
        check(fn(self._s, pp, kp, n, mem, k & 0xFFFFFFFF, mp, ip, sp, dp), self.ctx._h)
        return tuple(out)

    def nearest_tree_masked_batch(self, points, point_mask, max_dist=None):
        """knearest_tree_masked_batch with k = 1 and the last axis dropped: (instance[n], shape[n], dist[n])"""
        inst, shape, dist = self.knearest_tree_masked_batch(points, 1, point_mask, max_dist)
        return inst[:, 0], shape[:, 0], dist[:, 0]

    def region_masked_batch(self, planes, region_mask, classify: bool = False, count_only: bool = False, instances_only: bool = False) -> dict:
        """bvhgpu_instances_region_masked_*: region_batch over the instances visible to each region (a camera's culling mask against the
        objects' layers): the visible instances among those whose world box passes, in the top level's order, each walked as region_batch
        walks it.  classify, count_only, instances_only and the returns are region_batch's"""
        n, m = _plane_dims(planes)
        keep, pp, _rows, mem = api._rows_in(planes, 4, self.ft, "plane")
        _mk, kp = api._mask_in(region_mask, keep, n, mem, "region_mask", "regions")
        classify = bool(classify) and not count_only
        flags = ((_lib.REGION_COUNT_ONLY if count_only else 0) | (_lib.REGION_CLASSIFY if classify else 0) |
                 (_lib.REGION_INSTANCES_ONLY if instances_only else 0))
        index, byte = ((), "index"), ((), "byte")
        offsets, instance, shape, inside = self._csr("region_masked", (pp, kp, n, m, mem, flags), n, keep.device if mem == DEVICE else None, count_only,
                                                     index, None if instances_only else index, byte if classify else None, fetch="instances_region")
        out = dict(offsets=offsets, instance=instance)
        if not instances_only:
            out["shape"] = shape
        if classify:
            out["inside"] = inside
        return out


class Instances(InstancesTreeForm, InstancesMasks, InstancesMaskedQueries, _Typed):
    """bvhgpu_instances: `trees` (Bvh / FlatBvh objects of one context and dtype, with set_triangles done; kept referenced), `tree_of[i]`
    the member of instance i, `transforms` n x 12 or n x 3 x 4 (row-major 3x4, object -> world) in the trees' dtype.
    leaf: "triangle" (the default), "sphere" (the members need set_spheres instead: an instance's sphere is the ellipsoid its transform maps
    it to) or "box" (the shapes' own boxes, as parallelepipeds; the members need neither).  Every ray query of the set — closest_hits,
    any_hits, occluded, khits_batch, allhits_batch and their masked forms — answers with that kind's record: {distance, u, v} for triangles,
    {enter, exit} for boxes and {distance, exit} for spheres, in the world ray's parameter, so `vals` is 3 or 2 wide
    (_lib.LEAF_WIDTH).  region_batch serves every kind; the point queries measure triangle distance and raise INVALID_ARG on a box or sphere
    set.  update() is the
    re-pose and the re-sync: call it after moving instances and after any rebuild, refit or set_triangles of a member tree; a trace on a
    set whose member was rebuilt since raises INVALID_ARG ("instances are stale").  The *_masked methods (InstancesMasks for rays,
    InstancesMaskedQueries for points and regions) see only the instances whose mask shares a bit with the row's; every other method
    ignores the masks."""

    def __init__(self, trees: Sequence, tree_of, transforms, ctx: Optional[Context] = None, leaf: str = "triangle"):
        if leaf not in _lib.LEAF_KINDS:
            raise ValueError(f"leaf must be one of {sorted(_lib.LEAF_KINDS)}, not {leaf!r}")
        self.leaf = leaf                 # the leaf stage of every ray query of the set, fixed here
        trees = list(trees)
        self.trees = trees               # (the set borrows their device arrays)
        self.ctx = ctx or (trees[0].ctx if trees else api.default_context())
        f64 = isinstance(transforms, np.ndarray) and transforms.dtype == np.float64
        self.sfx = trees[0].sfx if trees else ("f64" if f64 else "f32")   # (a set without members has no instances either)
        self._s = None
        for t in trees:
            t._ready()                   # (a Bvh flattens here)
        handles = (C.c_void_p * max(len(trees), 1))(*[t._t for t in trees])
        _keep, xp, n, mem = api._rows_in(transforms, 12, self.ft, "transform")
        of = self._tree_of_in(tree_of, n, mem, _keep)
        h = C.c_void_p()
        if leaf == "triangle":
            fn = getattr(_lib.load(), f"bvhgpu_instances_create_{self.sfx}")
            check(fn(self.ctx._h, handles, len(trees), of[1], xp, n, mem, C.byref(h)), self.ctx._h)
        else:
            fn = getattr(_lib.load(), f"bvhgpu_instances_create_leaf_{self.sfx}")
            check(fn(self.ctx._h, handles, len(trees), of[1], xp, n, mem, _lib.LEAF_KINDS[leaf], C.byref(h)), self.ctx._h)
        self._s = h
        self.n = n
        self._counted = True
        self.ctx._child_add()
        api._live.add(self)

    @staticmethod
    def _tree_of_in(tree_of, n: int, mem: int, main):
        """n u32 in the transforms' memory → (the object kept alive, its c_void_p)"""
        if mem == DEVICE:   # 32-bit integers on the transforms' device (a host list is put there), then the one way in
            import torch
            tree_of = torch.as_tensor(tree_of, device=main.device).to(torch.int32).contiguous()
            api._torch_sync(main.device)
        elif api._is_device_tensor(tree_of):
            raise BvhGpuError(_lib.INVALID_ARG, "tree_of is a GPU tensor but the transforms are in host memory")
        keep, p, m, _ = api._rows_in(tree_of, 1, np.uint32, "tree_of", check_tensor=False, convert=True)
        if m != n:
            raise BvhGpuError(_lib.INVALID_ARG, f"tree_of has {m} values for {n} transforms")
        return keep, p

    def update(self, transforms) -> "Instances":
        """bvhgpu_instances_update_*: commit a new pose (and whatever the member trees hold now).  A failed update (a NaN in a transform)
        leaves the set uncommitted: every trace raises until an update succeeds."""
        for t in self.trees:
            t._ready()
        _keep, xp, n, mem = api._rows_in(transforms, 12, self.ft, "transform")
        if mem == DEVICE:
            api._torch_sync(_keep.device)
        check(getattr(_lib.load(), f"bvhgpu_instances_update_{self.sfx}")(self._s, xp, n, mem), self.ctx._h)
        return self

    def _check_rays(self, rays: RayBatch) -> None:
        if rays.sfx != self.sfx:
            raise BvhGpuError(_lib.DTYPE_MISMATCH, "ray dtype differs from the instance set's dtype")

    def _csr(self, entry: str, args, n: int, dev, count_only: bool, *cols, fetch: Optional[str] = None):
        """one CSR batch into the set's own result object (made on first use: its buffers are reused by every batch) and its fetch:
        bvhgpu_instances_<entry>_* with `args`, then api._fetch_csr with the columns given as (shape of one row, kind) or None.  fetch:
        the fetch entry of an <entry> whose result is of another entry's kind (allhits_masked: instances_allhits)"""
        if dev is not None:
            api._torch_sync(dev)
        if getattr(self, "_hits", None) is None:
            self._hits = api._Hits(self.ctx)
        hits = self._hits
        check(getattr(_lib.load(), f"bvhgpu_instances_{entry}_{self.sfx}")(self._s, *args, C.byref(hits.h)), self.ctx._h)
        rows = 0 if count_only else hits._total()
        return api._fetch_csr(fetch or f"instances_{entry}", hits, n, rows, self.ft, dev, *[c and ((rows,) + c[0], c[1]) for c in cols])

    def _trace(self, rays: RayBatch, tmax, flags: int):
        self._check_rays(rays)
        _keep, tp = api._side_in(tmax, rays.device, rays.n, rays.mem, self.ft, "tmax", "rays")
        n = rays.n
        out, (vp, ip, sp) = api._out_cols(rays.device.device if rays.mem == DEVICE else None, self.ft, ((n, _lib.LEAF_WIDTH[_lib.LEAF_KINDS[self.leaf]]), "float"), (n, "index"), (n, "index"))
        fn = getattr(_lib.load(), f"bvhgpu_instances_trace_{self.sfx}")
        check(fn(self._s, rays._ptr(), tp, n, rays.mem, flags, vp, ip, sp), self.ctx._h)
        return tuple(out)

    def closest_hits(self, rays: RayBatch, tmax=None):
        """per ray the nearest triangle hit over all instances with distance < tmax[i] (None: +inf): (vals[n,3] = Intersection{distance, u,
        v} in the world ray's parameter, instance[n], shape[n] within that instance's tree); a miss is (+inf, 0, 0), NONE, NONE.  HOST rays:
        numpy out, indices as uint32.  Rays in HBM: torch tensors on the same device, indices as torch.int32 (NONE reads as -1).
        Ignores the visibility masks (every instance is visible): closest_hits_masked looks at them."""
        return self._trace(rays, tmax, 0)

    def any_hits(self, rays: RayBatch, tmax=None):
        """BVHGPU_TRAVERSE_FIRST: the FIRST candidate in walk order (instances in the top level's order, shapes in the member's order) with
        distance < tmax[i]; returns what closest_hits returns.  Ignores the visibility masks (any_hits_masked looks at them)."""
        return self._trace(rays, tmax, _lib.TRAVERSE_FIRST)

    def occluded(self, rays: RayBatch, tmax=None):
        """bool[n]: does segment i hit any triangle of any instance (visibility masks ignored: occluded_masked)"""
        _, inst, _ = self.any_hits(rays, tmax)
        return inst != (NONE if isinstance(inst, np.ndarray) else -1)

    def region_batch(self, planes, classify: bool = False, count_only: bool = False, instances_only: bool = False) -> dict:
        """bvhgpu_instances_region_*: per region of m WORLD-space planes (bvh_amd.frustum_planes / aabb_planes; (n, m, 4) in the set's
        dtype, or (m, 4) for one region, m <= 32) the (instance, shape) pairs whose box passes, as a CSR: the instances whose world box
        passes, in the top level's order, each walked with the planes re-expressed in its object frame.  classify: also `inside`, one byte
        per pair, 1 iff the shape's box lies wholly inside.  count_only: offsets alone.  instances_only: the rows hold the instances
        whose world box passes and no shapes (`inside`: the world box lies wholly inside).
        returns {offsets[n+1], instance[total], shape[total] (not with instances_only), inside[total] (classify)}.  numpy in: numpy out,
        offsets and indices as uint32, inside as uint8.  torch in: torch tensors on the same device, indices as torch.int32, offsets as
        torch.int64, inside as torch.uint8."""
        n, m = _plane_dims(planes)
        keep, pp, _rows, mem = api._rows_in(planes, 4, self.ft, "plane")
        classify = bool(classify) and not count_only
        flags = ((_lib.REGION_COUNT_ONLY if count_only else 0) | (_lib.REGION_CLASSIFY if classify else 0) |
                 (_lib.REGION_INSTANCES_ONLY if instances_only else 0))
        index, byte = ((), "index"), ((), "byte")
        offsets, instance, shape, inside = self._csr("region", (pp, n, m, mem, flags), n, keep.device if mem == DEVICE else None, count_only,
                                                     index, None if instances_only else index, byte if classify else None)
        out = dict(offsets=offsets, instance=instance)
        if not instances_only:
            out["shape"] = shape
        if classify:
            out["inside"] = inside
        return out

    def allhits_batch(self, rays: RayBatch, tmax=None, sort: bool = True, count_only: bool = False) -> dict:
        """bvhgpu_instances_allhits_*: per ray EVERY (instance, shape) whose triangle it hits with distance < tmax[i] (None: +inf), as a
        CSR.  sort=True: each row ascending by distance, ties in walk order (instances in the top level's order, shapes in the member's
        order) — its head is closest_hits' answer; sort=False: walk order, no sort pass — its head is any_hits' answer.  count_only:
        offsets alone (the hit counts).
        returns {offsets[n+1], instance[total], shape[total], vals[total, 3] = {distance, u, v}} (offsets only with count_only).  HOST rays:
        numpy out, offsets and indices as uint32.  Rays in HBM: torch tensors on the same device, indices as torch.int32, offsets as
        torch.int64.  Ignores the visibility masks (allhits_masked_batch looks at them)."""
        self._check_rays(rays)
        _keep, tp = api._side_in(tmax, rays.device, rays.n, rays.mem, self.ft, "tmax", "rays")
        flags = (0 if sort else _lib.INSTANCES_ALLHITS_LIST_ORDER) | (_lib.INSTANCES_ALLHITS_COUNT_ONLY if count_only else 0)
        offsets, instance, shape, vals = self._csr("allhits", (rays._ptr(), tp, rays.n, rays.mem, flags), rays.n,
                                                   rays.device.device if rays.mem == DEVICE else None, count_only,
                                                   ((), "index"), ((), "index"), ((_lib.LEAF_WIDTH[_lib.LEAF_KINDS[self.leaf]],), "float"))
        if count_only:
            return dict(offsets=offsets)
        return dict(offsets=offsets, instance=instance, shape=shape, vals=vals)

    def khits_batch(self, rays: RayBatch, k: int, tmax=None):
        """bvhgpu_instances_khits_*: per ray the k nearest (instance, shape) hits with distance < tmax[i] (None: +inf), ascending by
        distance — the head of allhits_batch(sort=True)'s row, byte for byte, in fixed-width rows and one walk.  Equal distances stay in
        walk order (instances in the top level's order, shapes in the member's order), and a tie at the k-th distance keeps the pairs met
        first; k = 1 is closest_hits.  1 <= k <= _lib.INSTANCES_KHITS_MAX_K.
        returns (instance[n, k], shape[n, k], vals[n, k, 3] = {distance, u, v}); slots beyond the number of hits hold NONE, NONE and
        (+inf, 0, 0).  HOST rays: numpy out, indices as uint32.  Rays in HBM: torch tensors on the same device, written by the kernel,
        indices as torch.int32 — so NONE reads as -1 there.  Ignores the visibility masks (khits_masked_batch looks at them)."""
        self._check_rays(rays)
        k = int(k)
        rows = k if 1 <= k <= _lib.INSTANCES_KHITS_MAX_K else 0   # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        _keep, tp = api._side_in(tmax, rays.device, rays.n, rays.mem, self.ft, "tmax", "rays")
        n = rays.n
        out, (ip, sp, vp) = api._out_cols(rays.device.device if rays.mem == DEVICE else None, self.ft,
                                          ((n, rows), "index"), ((n, rows), "index"), ((n, rows, _lib.LEAF_WIDTH[_lib.LEAF_KINDS[self.leaf]]), "float"))
        fn = getattr(_lib.load(), f"bvhgpu_instances_khits_{self.sfx}")
        check(fn(self._s, rays._ptr(), tp, n, rays.mem, k & 0xFFFFFFFF, ip, sp, vp), self.ctx._h)
        return tuple(out)

    def within_batch(self, points, max_dist, sort: bool = True, count_only: bool = False) -> dict:
        """bvhgpu_instances_within_*: per point EVERY (instance, shape) whose world-space triangle lies within max_dist[i] of it (<=, the
        limit itself is inside; a negative or NaN limit gives an empty row, +inf keeps every pair whose distance is not NaN), as a CSR.
        The distance is the true world distance to the transformed triangle, whatever the transform.  sort=True: each row ascending by
        distance, ties in walk order (instances in the top level's order, shapes in the member's order); sort=False: walk order, no sort
        pass.  count_only: offsets alone.
        points: (n, 3) in the set's dtype — a numpy array (HOST) or a torch GPU tensor (DEVICE).  max_dist: a scalar (the same limit for
        every point) or n values in the points' memory.
        returns {offsets[n+1], instance[total], shape[total], dist[total]} (offsets only with count_only).  numpy in: numpy out, offsets
        and indices as uint32.  Points in HBM: torch tensors on the same device, indices as torch.int32, offsets as torch.int64."""
        if max_dist is None:
            raise BvhGpuError(_lib.INVALID_ARG, "within_batch needs max_dist (a scalar or one value per point)")
        keep, pp, n, mem = api._rows_in(points, 3, self.ft, "point")
        _m, mp = api._side_in(max_dist, keep, n, mem, self.ft, "max_dist", "points", scalar_ok=True)
        flags = (0 if sort else _lib.INSTANCES_WITHIN_LIST_ORDER) | (_lib.INSTANCES_WITHIN_COUNT_ONLY if count_only else 0)
        offsets, instance, shape, dist = self._csr("within", (pp, mp, n, mem, flags), n, keep.device if mem == DEVICE else None, count_only,
                                                   ((), "index"), ((), "index"), ((), "float"))
        if count_only:
            return dict(offsets=offsets)
        return dict(offsets=offsets, instance=instance, shape=shape, dist=dist)

    def knearest_batch(self, points, k: int):
        """bvhgpu_instances_knearest_*: per point the k (instance, shape) pairs whose world-space triangles are nearest — bvhgpu_knearest_*'s
        list and strict < over the two-level walk, the distance the true world distance to the transformed triangle.  Rows are ascending
        in dist (a row that holds a NaN need not be sorted); equal distances stay in walk order (instances in the top level's order,
        shapes in the member's order), and a tie at the k-th distance keeps the pairs met first.  1 <= k <= _lib.INSTANCES_KNN_MAX_K.
        points: (n, 3) in the set's dtype — a numpy array (HOST) or a torch GPU tensor (DEVICE).
        returns (instance[n, k], shape[n, k], dist[n, k]); slots beyond the number of pairs hold NONE, NONE and +inf.  numpy in: numpy
        out, indices as uint32.  torch in: torch tensors on the same device, written by the kernel, indices as torch.int32 — so NONE
        reads as -1 there."""
        k = int(k)
        rows = k if 1 <= k <= _lib.INSTANCES_KNN_MAX_K else 0   # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        keep, pp, n, mem = api._rows_in(points, 3, self.ft, "point")
        out, (ip, sp, dp) = api._out_cols(keep.device if mem == DEVICE else None, self.ft, ((n, rows), "index"), ((n, rows), "index"), ((n, rows), "float"))
        fn = getattr(_lib.load(), f"bvhgpu_instances_knearest_{self.sfx}")
        check(fn(self._s, pp, n, mem, k & 0xFFFFFFFF, ip, sp, dp), self.ctx._h)
        return tuple(out)

    def nearest_batch(self, points):
        """knearest_batch with k = 1 and the last axis dropped: (instance[n], shape[n], dist[n]) — the reference's nearest_to over the
        instanced scene; a set without instances gives NONE, NONE and +inf."""
        inst, shape, dist = self.knearest_batch(points, 1)
        return inst[:, 0], shape[:, 0], dist[:, 0]

    @property
    def world_boxes(self) -> np.ndarray:
        """W_i of the committed pose, (n, 6) [min xyz, max xyz]"""
        out = np.zeros((self.n, 6), dtype=self.ft)
        check(_lib.load().bvhgpu_instances_boxes(self._s, ptr(out), _lib.HOST), self.ctx._h)
        return out

    def info(self) -> Tuple[int, int]:
        """(member trees, instances)"""
        dt, nt, n = C.c_int(), C.c_size_t(), C.c_size_t()
        check(_lib.load().bvhgpu_instances_info(self._s, C.byref(dt), C.byref(nt), C.byref(n)), self.ctx._h)
        return int(nt.value), int(n.value)

    def close(self):
        if getattr(self, "_hits", None) is not None:
            self._hits.close()
            self._hits = None
        if getattr(self, "_s", None):
            if not api._closing:
                _lib.load().bvhgpu_instances_destroy(self._s)   # (frees what the set owns; never looks at a member tree)
        self._s = None
        if getattr(self, "_counted", False):
            self._counted = False
            self.ctx._child_drop()

    def __enter__(self) -> "Instances":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

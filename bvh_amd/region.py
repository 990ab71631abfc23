"""Convex-region (plane-set) queries over the C ABI (include/bvh_mi355x.h, bvhgpu_region_*): which shapes does this frustum see.

A region is m planes (nx, ny, nz, d); a point x is inside a plane when n.x + d >= 0 (normals point inward, any length).  Everything
that computes runs on the GPU; this file marshals, through api._rows_in like every other batch call, and builds plane sets on the host.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, api
from ._lib import DEVICE, BvhGpuError, check


def frustum_planes(eye, look_at, up=(0.0, 1.0, 0.0), fov_y_deg: float = 60.0, aspect: float = 1.6, near: float = 0.1, far: float = 1000.0,
                   dtype=np.float32) -> np.ndarray:
    """(6, 4) planes of the view frustum of api.camera(eye, look_at, up, fov_y_deg, aspect) between the depths `near` and `far` along the
    forward axis: left, right, bottom, top, near, far.  Computed in float64 and cast to `dtype`."""
    e = np.asarray(eye, dtype=np.float64); f = np.asarray(look_at, dtype=np.float64) - e
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, dtype=np.float64)); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    ty = np.tan(np.radians(fov_y_deg) / 2)
    tx = ty * aspect
    out = np.zeros((6, 4), dtype=np.float64)
    for k, nrm in enumerate((r + tx * f, -r + tx * f, u + ty * f, -u + ty * f)):   # the side planes pass through the eye
        out[k, :3] = nrm
        out[k, 3] = -np.dot(nrm, e)
    out[4, :3] = f; out[4, 3] = -np.dot(f, e) - near
    out[5, :3] = -f; out[5, 3] = np.dot(f, e) + far
    return out.astype(dtype)


def aabb_planes(mn, mx, dtype=np.float32) -> np.ndarray:
    """(6, 4) planes of the box [mn, mx]: x >= mn.x, x <= mx.x, then y, then z.  A box passes them exactly when Aabb::intersects_aabb
    says it touches [mn, mx] (the sums are hi - mn and mx - lo, whose sign is exact), as long as no coordinate is infinite or NaN."""
    mn = np.asarray(mn, dtype=np.float64).reshape(3); mx = np.asarray(mx, dtype=np.float64).reshape(3)
    out = np.zeros((6, 4), dtype=np.float64)
    for k in range(3):
        out[2 * k, k] = 1.0; out[2 * k, 3] = -mn[k]
        out[2 * k + 1, k] = -1.0; out[2 * k + 1, 3] = mx[k]
    return out.astype(dtype)


def _plane_dims(planes):
    """(n, m) of a plane array (n, m, 4), or (m, 4) for one region"""
    shp = tuple(planes.shape) if hasattr(planes, "shape") else np.shape(planes)
    if len(shp) == 2:
        shp = (1,) + shp
    if len(shp) != 3 or shp[2] != 4:
        raise BvhGpuError(_lib.INVALID_ARG, f"planes must be (n, m, 4) or (m, 4), not {shp}")
    return int(shp[0]), int(shp[1])


def region_batch(tree, planes, classify: bool = False, count_only: bool = False) -> dict:
    """bvhgpu_region_*: per region the shapes whose box passes every plane (the corner farthest along the normal is on the inner side), in
    the order of FlatBvh::traverse, as a CSR.  tree: a Bvh (flattened here) or FlatBvh.  planes: (n, m, 4) in the tree's dtype, or (m, 4) for
    one region, m <= 32 — a numpy array (HOST) or a torch GPU tensor (DEVICE); rows of zeros are padding planes.  classify: also `inside`,
    one byte per reported shape, 1 iff its AABB lies wholly inside the region.  count_only: offsets alone (indices is empty).
    returns {offsets[n+1], indices[total], inside[total] (classify), chunks, chunk_entries}: the last two say how the walk cut the tree's
    entry array (a region is walked by `chunks` wavefronts).  numpy in: numpy out, offsets and indices as uint32, inside as uint8.  torch
    in: torch tensors on the same device, indices as torch.int32, offsets as torch.int64, inside as torch.uint8."""
    tree._ready()
    n, m = _plane_dims(planes)
    keep, pp, _rows, mem = api._rows_in(planes, 4, tree.ft, "plane")
    classify = bool(classify) and not count_only
    flags = (_lib.REGION_COUNT_ONLY if count_only else 0) | (_lib.REGION_CLASSIFY if classify else 0)
    dev = keep.device if mem == DEVICE else None
    if dev is not None:
        api._torch_sync(dev)
    lib = _lib.load()
    hits = tree._hits
    check(getattr(lib, f"bvhgpu_region_{tree.sfx}")(tree._t, pp, n, m, mem, flags, C.byref(hits.h)), tree.ctx._h)
    nc, ce = C.c_uint32(), C.c_uint32()
    check(lib.bvhgpu_hits_region_info(hits.h, C.byref(nc), C.byref(ce)), tree.ctx._h)
    rows = 0 if count_only else hits._total()
    offsets, indices, inside = api._fetch_csr("region", hits, n, rows, tree.ft, dev, (rows, "index"), (rows, "byte") if classify else None)
    out = dict(offsets=offsets, indices=indices, chunks=int(nc.value), chunk_entries=int(ce.value))
    if classify:
        out["inside"] = inside
    return out

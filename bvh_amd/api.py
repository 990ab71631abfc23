"""Host-side mirror of the reference's operator surface for the hot path, over the C ABI.

Names, argument meaning and error behaviour follow the Rust crate (paths under /root/reference/src):
  Bounded.aabb()                     aabb/aabb_impl.rs:28-56
  BHShape.set_bh_node_index / bh_node_index   bounding_hierarchy.rs:53-65
  BoundingHierarchy.build / build_par / build_with_executor / traverse   bounding_hierarchy.rs:89-336
  Bvh, Bvh.flatten, FlatBvh          bvh/bvh_impl.rs:27-119, flat_bvh.rs:240-431
  Ray.new / intersects_aabb / intersection_slice_for_aabb   ray/ray_impl.rs:70-145
Conventions kept: empty input → empty structure, no error (bvh_impl.rs:57-59); `traverse` returns the
hit shapes themselves, in the reference's order; shapes are only borrowed.
Everything that computes runs on the GPU through libbvh_mi355x.so; this file only marshals.
"""
from __future__ import annotations

import atexit
import ctypes as C
import weakref
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import (DEVICE, F32, FLAT_F32, FLAT_F64, HOST, NODE_F32, NODE_F64, NONE, RAY_F32, RAY_F64,
                   TRAVERSE_CLOSEST, TRAVERSE_COHERENT, TRAVERSE_STATS, TRAVERSE_T_SLICE, TRAVERSE_TRIANGLES, BvhGpuError, check, ptr)


def _sfx(dtype) -> str:
    dt = np.dtype(dtype)
    if dt == np.float32:
        return "f32"
    if dt == np.float64:
        return "f64"
    raise TypeError(f"BHValue must be f32 or f64, got {dt}")


def _ray_dtype(s):
    return RAY_F32 if s == "f32" else RAY_F64


_FT = {"f32": np.float32, "f64": np.float64}


class _Typed:
    """what follows from `sfx` ("f32" / "f64"), the scalar type of a tree or a ray batch"""
    sfx: str

    @property
    def ft(self):
        """the numpy scalar type"""
        return _FT[self.sfx]


def _is_torch_ft(t, ft) -> bool:
    """is torch tensor `t` of the numpy scalar type `ft` (torch itself is not needed to tell)"""
    return str(t.dtype) == "torch." + ft.__name__


def _torch_ft(ft):
    """the torch dtype outputs for the numpy scalar type `ft` are allocated in"""
    import torch
    return torch.float32 if np.dtype(ft) == np.float32 else torch.float64


def _torch_sync(device) -> None:
    """the engine works on its own stream: what torch has enqueued on `device` (the inputs, the outputs' memory) must be there"""
    import torch
    torch.cuda.current_stream(device).synchronize()


# Native handles must be released while the HIP runtime is still alive: at interpreter shutdown the
# runtime's own static destructors may already have run when Python finalises leftover objects.
_live = weakref.WeakSet()
_closing = False


def _shutdown():
    global _closing
    for kind in ("_Hits", "tree", "Context"):
        for obj in list(_live):
            k = type(obj).__name__
            if (kind == "tree" and k not in ("_Hits", "Context")) or k == kind:
                try:
                    obj.close()
                except Exception:
                    pass
    _closing = True


atexit.register(_shutdown)


def _ray_flags(coherent: bool, first: bool = False) -> int:
    return (TRAVERSE_COHERENT if coherent else 0) | (_lib.TRAVERSE_FIRST if first else 0)


def _is_device_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and bool(x.is_cuda)


def _rows_in(x, width: int, ft, what: str, check_tensor: bool = True, convert: bool = False, device: bool = True, exact: bool = True):
    """The one way an input array reaches the C ABI: `x`, an array-like of rows of `width` scalars that must be in the tree's dtype `ft`
    → (the object to keep alive over the call, its c_void_p, the row count, HOST or DEVICE).  A torch GPU tensor is used in place, anything
    else becomes a contiguous numpy array.  Where the call sites differ, they say so:
      check_tensor  a tensor of another dtype raises DTYPE_MISMATCH and a strided one is made contiguous; False: a tensor is taken as it
                    is, its dtype unchecked (set_triangles, rebuild, refit, from_aabbs)
      convert       a numpy array of another dtype is converted; False: it raises DTYPE_MISMATCH (lists and scalars are always converted)
      device        False: host input only, a tensor is handed to numpy like any other object (nearest_batch)
      exact         a size that is no multiple of `width` raises numpy's ValueError; False: the partial row is dropped (query_batch)"""
    if device and _is_device_tensor(x):
        if check_tensor:
            if not _is_torch_ft(x, ft):
                raise BvhGpuError(_lib.DTYPE_MISMATCH, f"{what} dtype differs from tree dtype")
            x = x.contiguous()
        return x, ptr(x.data_ptr()), x.numel() // width, DEVICE
    if not convert and isinstance(x, np.ndarray) and x.dtype != ft:
        raise BvhGpuError(_lib.DTYPE_MISMATCH, f"{what} dtype differs from tree dtype")
    a = np.ascontiguousarray(x, dtype=ft)
    a = a.reshape(-1, width) if exact else a.reshape(-1)
    return a, ptr(a), a.size // width, HOST


def _out_cols(device, ft, *cols):
    """The one way output arrays are made: one per column (shape, "index" | "float" | "byte").  device None: numpy arrays (uint32 / `ft` /
    uint8).  Else torch tensors on that device (int32 — so NONE reads as -1 — / `ft` / uint8), and torch's stream is waited for: the engine
    writes them on its own.  → (the arrays, their c_void_p's)"""
    if device is None:
        arrs = [np.zeros(shape, dtype={"index": np.uint32, "float": ft, "byte": np.uint8}[kind]) for shape, kind in cols]
        return arrs, [ptr(a) for a in arrs]
    import torch
    dtypes = {"index": torch.int32, "float": _torch_ft(ft), "byte": torch.uint8}
    arrs = [torch.empty(shape, dtype=dtypes[kind], device=device) for shape, kind in cols]
    _torch_sync(device)
    return arrs, [ptr(a.data_ptr()) for a in arrs]


def _fetch_csr(entry: str, hits: "_Hits", n: int, rows: int, ft, device, *cols):
    """The one way a CSR leaves a result object: bvhgpu_hits_fetch_<entry> of the completed batch in `hits` → [offsets[n+1], one array per
    column].  A column is (shape, kind) as for _out_cols, or None for one this batch does not have: the engine gets NULL and the caller
    None.  With no rows the engine gets NULL for every column.  device None: copied to the host, offsets as uint32.  Else device-to-device
    copies into torch tensors there, and the offsets are widened to torch.int64 on the device."""
    arrs, ptrs = _out_cols(device, ft, (n + 1, "index"), *[c for c in cols if c is not None])
    made = iter(zip(arrs[1:], ptrs[1:]))
    got = [next(made) if c is not None else (None, None) for c in cols]
    fn = getattr(_lib.load(), f"bvhgpu_hits_fetch_{entry}")
    check(fn(hits.h, ptrs[0], *[p if rows else None for _, p in got], HOST if device is None else DEVICE), hits.ctx._h)
    if device is not None:
        import torch
        arrs[0] = arrs[0].to(torch.int64) & 0xFFFFFFFF
    return [arrs[0]] + [a for a, _ in got]


def _bytes_in(x):
    """a scene blob's buffer as it is, a torch GPU tensor or a numpy array → (its c_void_p, DEVICE or HOST)"""
    return (ptr(x.data_ptr()), DEVICE) if _is_device_tensor(x) else (ptr(x), HOST)


def _side_in(v, main, n: int, mem: int, ft, what: str, of: str, scalar_ok: bool = False):
    """The per-row side array of a batch (tmax of rays, max_dist of points): n values in the tree's dtype in the memory `mem` of the main
    input `main` → (the object to keep alive, its c_void_p); None → (None, None).  scalar_ok: a scalar is the same value for every row."""
    if v is None:
        return None, None
    if scalar_ok and not _is_device_tensor(v) and np.ndim(v) == 0:
        if mem == DEVICE:
            import torch
            keep = torch.full((n,), float(v), dtype=main.dtype, device=main.device)
            return keep, ptr(keep.data_ptr())
        keep = np.full(n, v, dtype=ft)
        return keep, ptr(keep)
    if _is_device_tensor(v) != (mem == DEVICE):
        raise BvhGpuError(_lib.INVALID_ARG, f"{what} is a GPU tensor but the {of} are in host memory" if mem == HOST else
                          f"{what} is in host memory but the {of} are in HBM")
    keep, p, m, _ = _rows_in(v, 1, ft, what)
    if m != n:
        raise BvhGpuError(_lib.INVALID_ARG, f"{what} has {m} values for {n} {of}")
    return keep, p


def _needs(v, msg: str) -> None:
    """an argument that has no default in the C ABI (max_dist of a within batch) must be given"""
    if v is None:
        raise BvhGpuError(_lib.INVALID_ARG, msg)


def _mask_in(v, main, n: int, mem: int, what: str, of: str):
    """The per-row 32-bit mask array of a batch (ray_mask of rays, point_mask of points, region_mask of regions): n u32 in the memory `mem` of the main input `main` → (the object to keep
    alive, its c_void_p); None → (None, None).  A Python int in [0, 2^32) is the same mask for every row.  HOST: numpy integers (or a
    list of them), int32 taken by its bits, anything else by its value.  DEVICE: a torch.int32 tensor on the main input's device, its bits
    taken as they are."""
    if v is None:
        return None, None
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        v = int(v)
        if not 0 <= v < 1 << 32:
            raise BvhGpuError(_lib.INVALID_ARG, f"{what} must be in [0, 2^32), not {v}")
        if mem == DEVICE:
            import torch
            keep = torch.full((n,), v - (1 << 32) if v >= 1 << 31 else v, dtype=torch.int32, device=main.device)
            return keep, ptr(keep.data_ptr())
        keep = np.full(n, v, dtype=np.uint32)
        return keep, ptr(keep)
    if _is_device_tensor(v) != (mem == DEVICE):
        raise BvhGpuError(_lib.INVALID_ARG, f"{what} is a GPU tensor but the {of} are in host memory" if mem == HOST else
                          f"{what} is in host memory but the {of} are in HBM")
    if mem == DEVICE:
        if str(v.dtype) != "torch.int32":
            raise BvhGpuError(_lib.DTYPE_MISMATCH, f"{what} must be a torch.int32 tensor (its bits are the masks)")
        v = v.contiguous()
        if v.numel() != n:
            raise BvhGpuError(_lib.INVALID_ARG, f"{what} has {v.numel()} values for {n} {of}")
        return v, ptr(v.data_ptr())
    a = np.asarray(v)
    if a.size and a.dtype.kind not in "iu":
        raise BvhGpuError(_lib.DTYPE_MISMATCH, f"{what} must be integers")
    if a.dtype == np.int32:
        a = a.view(np.uint32)
    elif a.size and (int(a.min()) < 0 or int(a.max()) >= 1 << 32):
        raise BvhGpuError(_lib.INVALID_ARG, f"{what} values must be in [0, 2^32)")
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    if a.size != n:
        raise BvhGpuError(_lib.INVALID_ARG, f"{what} has {a.size} values for {n} {of}")
    return a, ptr(a)


# ------------------------------------------------------------------------------------------------
class Context:
    """One GPU + one HIP stream + scratch (bvhgpu_ctx).  `stream` may be a raw hipStream_t
    (e.g. torch.cuda.current_stream().cuda_stream) so that work is ordered with the caller's."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        lib = _lib.load()
        if _lib.device_count() <= 0:
            raise BvhGpuError(_lib.NO_DEVICE, "no MI355X / HIP device visible: the engine has no CPU fallback")
        h = C.c_void_p()
        check(lib.bvhgpu_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
        self._h = h
        self.device = int(device)
        # The C ABI wants a ctx to outlive what was made on it (bvhgpu_tree_destroy / bvhgpu_hits_destroy / bvhgpu_comm_destroy look at
        # their ctx).  Reference counts normally give that order, but objects caught in a reference cycle (a pytest.raises traceback is
        # enough) are finalised by the cyclic collector in ARBITRARY order — so the ctx counts its children and, if it is closed while
        # some are alive, hands its destruction to the last of them.
        self._nchildren = 0
        self._deferred = False
        _live.add(self)

    def _child_add(self):
        self._nchildren += 1

    def _child_drop(self):
        self._nchildren -= 1
        if self._nchildren <= 0 and self._deferred:
            self._destroy()

    def _destroy(self):
        if getattr(self, "_h", None) and not _closing:
            _lib.load().bvhgpu_destroy(self._h)
        self._h = None
        self._deferred = False

    def synchronize(self):
        check(_lib.load().bvhgpu_synchronize(self._h), self._h)

    def enable_timing(self, on: bool = True):
        check(_lib.load().bvhgpu_enable_timing(self._h, int(on)), self._h)

    def last_timings(self) -> dict:
        t = _lib.Timings()
        check(_lib.load().bvhgpu_last_timings(self._h, C.byref(t)), self._h)
        return dict(build_ms=t.build_ms, flatten_ms=t.flatten_ms, traverse_kernel_ms=t.traverse_kernel_ms,
                    traverse_total_ms=t.traverse_total_ms)

    def set_tuning(self, knob: int, value: int):
        """performance knobs (include/bvh_mi355x.h bvhgpu_tune); results never change."""
        check(_lib.load().bvhgpu_set_tuning(self._h, int(knob), int(value)), self._h)

    def get_tuning(self, knob: int) -> int:
        v = C.c_int(0)
        check(_lib.load().bvhgpu_get_tuning(self._h, int(knob), C.byref(v)), self._h)
        return int(v.value)

    def close(self):
        if getattr(self, "_h", None) is None:
            return
        if getattr(self, "_nchildren", 0) > 0 and not _closing:
            self._deferred = True      # the last tree / result object / communicator made on it destroys it
            return
        self._destroy()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: Optional[Context] = None


class PinnedArray(np.ndarray):
    """numpy view of pinned host memory (bvhgpu_host_alloc): the DMA engines read and write it directly"""
    _bvhgpu_pinned = True


def pinned_array(ctx: "Context", shape, dtype) -> np.ndarray:
    """an uninitialised array in pinned host memory; freed (bvhgpu_host_free) when the last view of it is gone"""
    lib = _lib.load()
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dt.itemsize
    p = C.c_void_p()
    check(lib.bvhgpu_host_alloc(ctx._h, max(nbytes, 1), C.byref(p)), ctx._h)
    buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
    ctx._child_add()

    def release(addr=p.value, c=ctx):
        if not _closing and getattr(c, "_h", None):
            lib.bvhgpu_host_free(c._h, C.c_void_p(addr))
        c._child_drop()
    weakref.finalize(buf, release)
    a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape).view(PinnedArray)
    return a


class HostStep:
    """What a host-resident caller of the drop-in boundary does per frame, with everything in pinned memory: shapes' AABBs, ray origins
    and directions in; CSR offsets / indices out.  run() = GpuBvh::build + traverse_batch of the Rust shim in one call
    (bvhgpu_build_traverse_host_*): the ray upload overlaps the build, Ray::new runs on the device."""

    def __init__(self, bvh: "Bvh", n_shapes: int, n_rays: int, dtype=np.float32, index_cap: Optional[int] = None, od6: bool = False):
        """od6: origin and direction of a ray side by side in ONE pinned array (`od`, n x 6; `origins` / `directions` are views of its
        halves) — BVHGPU_TRAVERSE_RAYS_OD6: one transfer per chunk instead of two"""
        self.bvh, ctx = bvh, bvh.ctx
        self.aabbs = pinned_array(ctx, (n_shapes, 6), dtype)
        self.od = pinned_array(ctx, (n_rays, 6), dtype) if od6 else None
        self.origins = self.od[:, :3] if od6 else pinned_array(ctx, (n_rays, 3), dtype)
        self.directions = self.od[:, 3:] if od6 else pinned_array(ctx, (n_rays, 3), dtype)
        self.offsets = pinned_array(ctx, (n_rays + 1,), np.uint32)
        self.indices = pinned_array(ctx, (index_cap or max(n_rays, 1 << 16),), np.uint32)
        self.total = 0

    def run(self, coherent: bool = False, fused: bool = True):
        """fused: bvhgpu_build_traverse_host_* (one call, the ray upload enqueued before the build); else the two calls
        bvhgpu_rebuild_flat_async_*(HOST) + bvhgpu_traverse_host_*"""
        if not fused:
            self.bvh.rebuild_async(self.aabbs)
        if self.od is not None:
            self.total = self.bvh.traverse_host(self.od, None, self.offsets, self.indices, coherent=coherent, aabbs=self.aabbs if fused else None,
                                                od6=True)
        else:
            self.total = self.bvh.traverse_host(self.origins, self.directions, self.offsets, self.indices, coherent=coherent,
                                                aabbs=self.aabbs if fused else None)
        if self.total > self.indices.size:
            self.indices = pinned_array(self.bvh.ctx, (self.total + self.total // 8,), np.uint32)
            self.bvh.traverse_host_indices(self.indices)
        return self.offsets, self.indices[:self.total]

    def close(self):
        self.aabbs = self.origins = self.directions = self.od = self.offsets = self.indices = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ------------------------------------------------------------------------------------------------
class Aabb:
    """Aabb<T,3> {min, max} (aabb_impl.rs:10-16) as a host value type.  Only construction helpers
    live here (a shape needs them to answer Bounded.aabb()); all hot-path arithmetic is on the GPU."""
    __slots__ = ("min", "max")

    def __init__(self, mn, mx, dtype=np.float32):
        self.min = np.asarray(mn, dtype=dtype).reshape(3)
        self.max = np.asarray(mx, dtype=dtype).reshape(3)

    @staticmethod
    def with_bounds(mn, mx, dtype=np.float32) -> "Aabb":  # aabb_impl.rs:97-99
        return Aabb(mn, mx, dtype)

    @staticmethod
    def empty(dtype=np.float32) -> "Aabb":  # aabb_impl.rs:119-124
        return Aabb([np.inf] * 3, [-np.inf] * 3, dtype)

    def join(self, other: "Aabb") -> "Aabb":  # aabb_impl.rs:303-308
        return Aabb(np.minimum(self.min, other.min), np.maximum(self.max, other.max), self.min.dtype)

    def grow(self, p) -> "Aabb":  # aabb_impl.rs:375-380
        p = np.asarray(p, dtype=self.min.dtype)
        return Aabb(np.minimum(self.min, p), np.maximum(self.max, p), self.min.dtype)

    def as6(self) -> np.ndarray:
        return np.concatenate([self.min, self.max])

    def __repr__(self):
        return f"Aabb(min={self.min.tolist()}, max={self.max.tolist()})"


class Ball:
    """struct Ball<T,3> (ball.rs:13-19): centre + radius; Sphere = Ball (ball.rs:23).  A point query is a length-3 sequence or array."""

    def __init__(self, center, radius, dtype=np.float32):
        self.center = np.asarray(center, dtype=dtype).reshape(3).copy()
        self.radius = np.dtype(dtype).type(radius)

    @staticmethod
    def new(center, radius, dtype=np.float32) -> "Ball":  # ball.rs:30-32
        return Ball(center, radius, dtype)

    def as4(self) -> np.ndarray:
        return np.concatenate([self.center, np.asarray([self.radius], dtype=self.center.dtype)])

    def __repr__(self):
        return f"Ball(center={self.center.tolist()}, radius={float(self.radius)})"


Sphere = Ball


def spheres_aabbs(spheres) -> np.ndarray:
    """the AABBs a sphere scene is built from, [c - r, c + r] as (n,6) in the input's dtype (the reference's examples/simple.rs, Sphere::aabb)"""
    s = np.asarray(spheres)
    if s.dtype not in (np.float32, np.float64):
        s = s.astype(np.float64)
    s = s.reshape(-1, 4)
    r = s[:, 3:4]
    return np.ascontiguousarray(np.concatenate([s[:, :3] - r, s[:, :3] + r], axis=1))


def _query_row(query, ft):
    """(kind, one row of scalars) of an Aabb / Ball / point query in the tree's dtype"""
    if isinstance(query, Aabb):
        return _lib.QUERY_AABB, np.asarray(query.as6(), dtype=ft)
    if isinstance(query, Ball):
        return _lib.QUERY_BALL, np.asarray(query.as4(), dtype=ft)
    p = np.asarray(query, dtype=ft).reshape(-1)
    if p.shape != (3,):
        raise TypeError("traverse takes a Ray, an Aabb, a Ball / Sphere or a point (3 coordinates)")
    return _lib.QUERY_POINT, p


class Bounded:
    """trait Bounded (aabb_impl.rs:28-56)."""

    def aabb(self) -> Aabb:
        raise NotImplementedError


class BHShape(Bounded):
    """trait BHShape (bounding_hierarchy.rs:53-65)."""

    def set_bh_node_index(self, index: int) -> None:
        raise NotImplementedError

    def bh_node_index(self) -> int:
        raise NotImplementedError


# ------------------------------------------------------------------------------------------------
class RayBatch(_Typed):
    """A batch of Ray<T,3> (ray_impl.rs:17-29) in host memory (structured array) or in HBM."""

    def __init__(self, n: int, dtype, host: Optional[np.ndarray] = None, device=None, device_ptr: int = 0):
        self.n = int(n)
        self.sfx = _sfx(dtype)
        self.host = host          # numpy structured array or None
        self.device = device      # object that owns the device memory (e.g. torch tensor) or None
        self.device_ptr = int(device_ptr)

    @property
    def mem(self) -> int:
        return DEVICE if self.host is None else HOST

    def _ptr(self):
        return ptr(self.device_ptr) if self.host is None else ptr(self.host)

    @staticmethod
    def new(origins, directions, dtype=np.float32, ctx: Optional[Context] = None) -> "RayBatch":
        """Ray::new for every row (ray_impl.rs:70-80): normalise the direction, cache 1/d — on the GPU."""
        ctx = ctx or default_context()
        s = _sfx(dtype)
        o = np.ascontiguousarray(origins, dtype=dtype).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=dtype).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("origins and directions differ in length")
        out = np.zeros(len(o), dtype=_ray_dtype(s))
        fn = getattr(_lib.load(), f"bvhgpu_rays_new_{s}")
        check(fn(ctx._h, ptr(o), ptr(d), len(o), HOST, ptr(out), HOST), ctx._h)
        return RayBatch(len(o), dtype, host=out)

    @staticmethod
    def from_device(device_obj, n: int, dtype=np.float32) -> "RayBatch":
        """Wrap rays already resident in HBM (torch uint8/float tensor holding n Ray structs)."""
        return RayBatch(n, dtype, host=None, device=device_obj, device_ptr=device_obj.data_ptr())

    @staticmethod
    def generate(first: int, n: int, bounds, device_obj, dtype=np.float32, ctx: Optional[Context] = None) -> "RayBatch":
        """The bench ray stream create_ray(seed 0) (testbase.rs:687-691, :825), rays [first, first+n),
        written straight into `device_obj` (a torch tensor of >= n*sizeof(Ray) bytes on the GPU)."""
        ctx = ctx or default_context()
        s = _sfx(dtype)
        b = np.ascontiguousarray(bounds, dtype=np.float32).reshape(6)
        fn = getattr(_lib.load(), f"bvhgpu_gen_rays_{s}")
        check(fn(ctx._h, C.c_uint64(first), n, ptr(b), ptr(device_obj.data_ptr())), ctx._h)
        return RayBatch(n, dtype, host=None, device=device_obj, device_ptr=device_obj.data_ptr())


def intersect_triangle_pairs(rays: "RayBatch", tris, ctx: Optional["Context"] = None) -> np.ndarray:
    """Ray::intersects_triangle (ray_impl.rs:154-213) for ray i against triangle i, on the GPU.
    tris: (n,3,3) or (n,9).  returns (n,3) = Intersection{distance,u,v}."""
    ctx = ctx or default_context()
    ft = rays.ft
    t = np.ascontiguousarray(tris, dtype=ft).reshape(-1, 9)
    if len(t) != rays.n or rays.host is None:
        raise ValueError("one host triangle per host ray is required")
    out = np.zeros((rays.n, 3), dtype=ft)
    fn = getattr(_lib.load(), f"bvhgpu_ray_triangle_pairs_{rays.sfx}")
    check(fn(ctx._h, rays._ptr(), ptr(t), rays.n, HOST, ptr(out)), ctx._h)
    return out


def camera(eye, look_at, up=(0.0, 1.0, 0.0), fov_y_deg: float = 60.0, aspect: float = 1.6) -> np.ndarray:
    """cam[14] for RayBatch.primary: eye, right, up, forward (orthonormal, f32), tan_x, tan_y."""
    e = np.asarray(eye, dtype=np.float64); f = np.asarray(look_at, dtype=np.float64) - e
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, dtype=np.float64)); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    ty = np.tan(np.radians(fov_y_deg) / 2)
    return np.concatenate([e, r, u, f, [ty * aspect, ty]]).astype(np.float32)


def _primary(cam, width, height, first, n, device_obj, dtype, ctx):
    s = _sfx(dtype)
    c = np.ascontiguousarray(cam, dtype=np.float32).reshape(14)
    fn = getattr(_lib.load(), f"bvhgpu_gen_primary_rays_{s}")
    check(fn(ctx._h, ptr(c), width, height, C.c_uint64(first), n, ptr(device_obj.data_ptr())), ctx._h)
    return RayBatch(n, dtype, host=None, device=device_obj, device_ptr=device_obj.data_ptr())


RayBatch.primary = staticmethod(lambda cam, width, height, first, n, device_obj, dtype=np.float32, ctx=None:
                               _primary(cam, width, height, first, n, device_obj, dtype, ctx or default_context()))


class Ray:
    """struct Ray (ray_impl.rs:17-29).  Ray(origin, direction) == Ray::new."""

    def __init__(self, origin, direction, dtype=np.float32, ctx: Optional[Context] = None):
        self._batch = RayBatch.new([origin], [direction], dtype, ctx)
        r = self._batch.host[0]
        self.origin, self.direction, self.inv_direction = r["o"].copy(), r["d"].copy(), r["inv"].copy()
        self.dtype = np.dtype(dtype)

    @staticmethod
    def new(origin, direction, dtype=np.float32) -> "Ray":
        return Ray(origin, direction, dtype)

    def _probe(self, aabb: Aabb, want_t: bool):
        # one-box scene: a single-shape Bvh traversed by this ray is exactly one
        # Ray::intersects_aabb (flat_bvh.rs:411-418 / bvh_node.rs:314)
        bvh = Bvh.from_aabbs(aabb.as6().reshape(1, 6).astype(self.dtype))
        off, idx, ts, _ = bvh.flatten().traverse_batch(self._batch, want_t=want_t)
        return (len(idx) == 1), (ts[0] if want_t and len(idx) else None)

    def intersects_triangle(self, a, b, c):  # ray_impl.rs:154-213 → Intersection(distance, u, v)
        t = np.concatenate([np.asarray(v, dtype=self.dtype).reshape(3) for v in (a, b, c)]).reshape(1, 9)
        r = intersect_triangle_pairs(self._batch, t)[0]
        return r[0], r[1], r[2]

    def intersects_aabb(self, aabb: Aabb) -> bool:  # ray_impl.rs:105-110, intersect_default.rs:16-37
        return self._probe(aabb, False)[0]

    def intersection_slice_for_aabb(self, aabb: Aabb):  # ray_impl.rs:118-145
        hit, ts = self._probe(aabb, True)
        return (ts[0], ts[1]) if hit else None


# ------------------------------------------------------------------------------------------------
class _Hits:
    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.h = C.c_void_p()
        self._counted = True
        ctx._child_add()
        _live.add(self)

    def wait(self) -> dict:
        """bvhgpu_hits_wait: complete an asynchronous batch; returns the stats dict of traverse_batch."""
        check(_lib.load().bvhgpu_hits_wait(self.h), self.ctx._h)
        total, sd = self._stats()
        sd["total"] = total
        return sd

    def info(self) -> dict:
        """stats of the completed batch (bvhgpu_hits_info)"""
        total, sd = self._stats()
        sd["total"] = total
        return sd

    def _stats(self, want_total: bool = True):
        """one bvhgpu_hits_info → (the hit total, or None when it is not asked for; the stats dict of the batch calls)"""
        total = C.c_uint64() if want_total else None
        st = _lib.TraverseStats()
        check(_lib.load().bvhgpu_hits_info(self.h, None, C.byref(total) if want_total else None, C.byref(st)), self.ctx._h)
        return (int(total.value) if want_total else None), dict(hits=int(st.hits), visited=int(st.visited), leaf_visits=int(st.leaf_visits),
                                                                device_steps=int(st.device_steps), wave_steps=int(st.wave_steps))

    def _total(self) -> int:
        """the hit total alone (bvhgpu_hits_info): what the CSR fetches size their outputs by"""
        total = C.c_uint64()
        check(_lib.load().bvhgpu_hits_info(self.h, None, C.byref(total), None), self.ctx._h)
        return int(total.value)

    def walk_kernel(self) -> str:
        """bvhgpu_hits_walk_kernel: the kernel the completed batch was walked by, spelled as rocprofv3 prints it"""
        buf = C.create_string_buffer(160)
        check(_lib.load().bvhgpu_hits_walk_kernel(self.h, buf, 160), self.ctx._h)
        return buf.value.decode()

    def walk_flags(self) -> int:
        f = C.c_uint(0)
        check(_lib.load().bvhgpu_hits_walk_info(self.h, C.byref(f)), self.ctx._h)
        return int(f.value)

    def _fetch_per_ray(self, entry: str, width: int, n_rays: int, dtype):
        """bvhgpu_hits_fetch_<entry>: one record of `width` scalars and one shape per ray, copied to the host"""
        vals = np.zeros((n_rays, width), dtype=dtype)
        shape = np.zeros(n_rays, dtype=np.uint32)
        check(getattr(_lib.load(), f"bvhgpu_hits_fetch_{entry}")(self.h, ptr(vals), ptr(shape), HOST), self.ctx._h)
        return vals, shape

    def fetch_closest(self, n_rays: int, dtype=np.float32):
        """CLOSEST batches: (Intersection{distance,u,v}[n,3], shape[n]) of the completed batch, copied to the host"""
        return self._fetch_per_ray("closest", 3, n_rays, dtype)

    def fetch_any(self, n_rays: int, dtype=np.float32):
        """any-hit batches: (Intersection{distance,u,v}[n,3], shape[n]) of the completed batch, copied to the host"""
        return self._fetch_per_ray("any", 3, n_rays, dtype)

    def fetch_box(self, n_rays: int, dtype=np.float32):
        """box batches: (slice{enter,exit}[n,2], shape[n]) of the completed batch, copied to the host"""
        return self._fetch_per_ray("box", 2, n_rays, dtype)

    def fetch_sphere(self, n_rays: int, dtype=np.float32):
        """sphere batches: (hit{distance,exit}[n,2], shape[n]) of the completed batch, copied to the host"""
        return self._fetch_per_ray("sphere", 2, n_rays, dtype)

    def fetch_triangles(self, dtype=np.float32):
        """TRIANGLES batches: Intersection{distance,u,v} of every candidate, CSR order"""
        isect = np.zeros((self._total(), 3), dtype=dtype)
        check(_lib.load().bvhgpu_hits_fetch_triangles(self.h, ptr(isect), HOST), self.ctx._h)
        return isect

    def fetch(self, n_rays: int):
        """(offsets, indices) of the completed batch, copied to the host."""
        offsets = np.zeros(n_rays + 1, dtype=np.uint32)
        indices = np.zeros(self._total(), dtype=np.uint32)
        check(_lib.load().bvhgpu_hits_fetch(self.h, ptr(offsets), ptr(indices), None, HOST), self.ctx._h)
        return offsets, indices

    def _fetch_rows(self, entry: str, n: int, rows: int, vshape, dtype, device):
        """bvhgpu_hits_fetch_<entry> of a CSR-rows batch: (offsets[n+1], shape[rows], vals[vshape]), as _fetch_csr hands them over"""
        return tuple(_fetch_csr(entry, self, n, rows, dtype, device, (rows, "index"), (vshape, "float")))

    def fetch_allhits(self, n_rays: int, leaf: str = "box", dtype=np.float32, device=None):
        """all-hits batches (bvhgpu_hits_fetch_allhits): (offsets[n+1], shape[total], vals[total, W]) of the completed batch.  device None:
        copied to the host, offsets and shape as uint32.  device: torch tensors there, filled by device-to-device copies — shape as
        torch.int32, offsets widened to torch.int64 on the device."""
        total = self._total()
        return self._fetch_rows("allhits", n_rays, total, (total, _lib.LEAF_WIDTH[_lib.LEAF_KINDS[leaf]]), dtype, device)

    def fetch_within(self, n: int, dtype=np.float32, device=None, count_only: bool = False):
        """within batches (bvhgpu_hits_fetch_within): (offsets[n+1], shape[total], dist[total]) of the completed batch; a count-only batch
        has empty shape and dist.  device None: copied to the host, offsets and shape as uint32.  device: torch tensors there, filled by
        device-to-device copies — shape as torch.int32, offsets widened to torch.int64 on the device."""
        total = self._total()
        rows = 0 if count_only else total
        return self._fetch_rows("within", n, rows, rows, dtype, device)

    def close(self):
        if getattr(self, "h", None) and not _closing:
            _lib.load().bvhgpu_hits_destroy(self.h)
        self.h = None
        if getattr(self, "_counted", False):
            self._counted = False
            self.ctx._child_drop()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SpherePointQueries:
    """The point families against the tree's spheres (set_spheres): bvhgpu_knearest_sphere_*, _knearest_tree_sphere_* and _within_sphere_*,
    which _TreeBase inherits.  The shape distance is sqrt(d), d the squared distance from the point to the solid ball {cx, cy, cz, r}:
    len = |p - c| rounded as dot3 and one sqrt, g = len - r, d = max(g, 0)^2 with a NaN kept (0 inside and on the ball; r is taken
    literally).  Everything else — the loops, the strict comparisons, padding, memory rules, dtypes, returns — is knearest_batch's,
    knearest_tree_batch's and within_batch's.  Nodes are pruned by their boxes: the rows are the k nearest / all within in the geometric
    sense when every sphere lies inside its shape's box, as with spheres_aabbs.  A tree without spheres raises INVALID_ARG."""

    def _knearest_sphere(self, entry: str, points, k: int, max_dist, with_limit: bool):
        """_knearest's marshalling for the entries without a kind argument"""
        fn = getattr(_lib.load(), f"bvhgpu_{entry}_{self.sfx}")
        k = int(k)
        rows = k if 1 <= k <= _lib.KNN_MAX_K else 0       # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        p, pp, n, mem, _m, mp = self._points_in(points, max_dist)   # (p, _m: what the pointers point into stays alive over the call)
        shape, dist, sp, dp = self._alloc_out(p.device if mem == DEVICE else None, (n, rows), (n, rows))
        limit = (mp,) if with_limit else ()
        check(fn(self._t, pp, n, mem, k & 0xFFFFFFFF, *limit, sp, dp), self.ctx._h)
        return shape, dist

    def knearest_sphere_batch(self, points, k: int):
        """bvhgpu_knearest_sphere_*: the k nearest spheres of every point, knearest_batch's loop and returns — (shape[n, k], dist[n, k]),
        rows ascending, equal distances in leaf pre-order, padding NONE and +inf.  1 <= k <= _lib.KNN_MAX_K."""
        self._ready()
        return self._knearest_sphere("knearest_sphere", points, k, None, False)

    def nearest_sphere_batch(self, points):
        """knearest_sphere_batch with k = 1 and the last axis dropped: (shape[n], dist[n]); NONE and +inf for an empty hierarchy"""
        shape, dist = self.knearest_sphere_batch(points, 1)
        return shape[:, 0], dist[:, 0]

    def knearest_tree_sphere_batch(self, points, k: int, max_dist=None):
        """bvhgpu_knearest_tree_sphere_*: the same rows found nearest child first over the BvhNode array, knearest_tree_batch's descent,
        max_dist (None, a scalar or n values in the points' memory) and returns.  The tree must have been built here; no flatten is
        needed.  Ties stay in the order this walk meets them."""
        return self._knearest_sphere("knearest_tree_sphere", points, k, max_dist, True)

    def within_sphere_batch(self, points, max_dist, sort: bool = True, count_only: bool = False):
        """bvhgpu_within_sphere_*: every sphere within max_dist[i] of point i (d <= max_dist[i]^2), as a CSR — within_batch's loop, flags
        and returns: (offsets[n+1], shape[total], dist[total]), rows in a stable ascending sort by distance unless sort=False;
        count_only=True gives the offsets alone."""
        self._ready()
        flags = (0 if sort else _lib.WITHIN_LIST_ORDER) | (_lib.WITHIN_COUNT_ONLY if count_only else 0)
        if max_dist is None:
            raise BvhGpuError(_lib.INVALID_ARG, "within_sphere_batch needs max_dist (a scalar or one value per point)")
        p, pp, n, mem, _m, mp = self._points_in(points, max_dist)   # (p, _m: what the pointers point into stays alive over the call)
        dev = p.device if mem == DEVICE else None
        if dev is not None:
            _torch_sync(dev)
        fn = getattr(_lib.load(), f"bvhgpu_within_sphere_{self.sfx}")
        check(fn(self._t, pp, mp, n, mem, flags, C.byref(self._hits.h)), self.ctx._h)
        return self._hits.fetch_within(n, self.ft, dev, count_only)


class _TreeBase(_SpherePointQueries, _Typed):
    def __init__(self, ctx: Context, handle, sfx: str):
        self.ctx = ctx
        self._t = handle
        self.sfx = sfx
        self._hits = _Hits(ctx)
        self._counted = True
        ctx._child_add()
        _live.add(self)

    def close(self):
        if getattr(self, "_t", None):
            if getattr(self, "_hits", None) is not None:
                self._hits.close()
            if not _closing:
                _lib.load().bvhgpu_tree_destroy(self._t)
        self._t = None
        if getattr(self, "_counted", False):
            self._counted = False
            self.ctx._child_drop()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> Tuple[int, int, int]:
        n, nn, nf = C.c_size_t(), C.c_size_t(), C.c_size_t()
        dt = C.c_int()
        check(_lib.load().bvhgpu_tree_info(self._t, C.byref(dt), C.byref(n), C.byref(nn), C.byref(nf)), self.ctx._h)
        return int(n.value), int(nn.value), int(nf.value)

    def _ready(self) -> None:
        """called first by traverse, query_batch, nearest_batch and knearest_batch, which walk the flat arrays: a Bvh flattens here, a
        FlatBvh has nothing to do.  (khits_batch, allhits_batch and within_batch flatten in overrides on Bvh, which their tests pin.)"""

    # ---- traversal -------------------------------------------------------------------------
    def traverse_batch(self, rays: RayBatch, want_t: bool = False, stats: bool = False, fetch: bool = True,
                       coherent: bool = False, order: Optional[str] = None):
        """<FlatBvh as BoundingHierarchy>::traverse for a batch (flat_bvh.rs:396-431).
        returns (offsets[n+1], indices[total], tslice[total,2]|None, stats dict)."""
        if rays.sfx != self.sfx:
            raise BvhGpuError(_lib.DTYPE_MISMATCH, "ray dtype differs from tree dtype")
        lib = _lib.load()
        flags = (TRAVERSE_T_SLICE if want_t else 0) | (TRAVERSE_STATS if stats else 0) | (TRAVERSE_COHERENT if coherent else 0)
        flags |= _lib.ORDER_FLAGS[order]
        fn = getattr(lib, f"bvhgpu_traverse_{self.sfx}")
        check(fn(self._t, rays._ptr(), rays.n, rays.mem, flags, C.byref(self._hits.h)), self.ctx._h)
        total, sd = self._hits._stats()
        sd["walk"] = self._hits.walk_flags()        # _lib.WALK_* bits (diagnostic)
        sd["kernel"] = self._hits.walk_kernel()     # ... and the kernel's name
        if not fetch:
            return None, None, None, sd
        offsets = np.zeros(rays.n + 1, dtype=np.uint32)
        indices = np.zeros(total, dtype=np.uint32)
        ts = np.zeros((total, 2), dtype=self.ft) if want_t else None
        check(lib.bvhgpu_hits_fetch(self._hits.h, ptr(offsets), ptr(indices), ptr(ts), HOST), self.ctx._h)
        return offsets, indices, ts, sd

    def traverse_async(self, rays: RayBatch, hits: Optional["_Hits"] = None, flags: int = 0) -> "_Hits":
        """bvhgpu_traverse_async_*: enqueue the batch (rays resident in HBM) and return at once; the tree may still be
        building on the same stream.  `hits.wait()` completes it (and returns the stats dict)."""
        if rays.sfx != self.sfx:
            raise BvhGpuError(_lib.DTYPE_MISMATCH, "ray dtype differs from tree dtype")
        hits = hits or self._hits
        fn = getattr(_lib.load(), f"bvhgpu_traverse_async_{self.sfx}")
        check(fn(self._t, rays._ptr(), rays.n, rays.mem, flags, C.byref(hits.h)), self.ctx._h)
        return hits

    # ---- triangle stage -------------------------------------------------------------------
    def set_triangles(self, tris) -> None:
        """vertices of the shapes, (n,3,3) or (n,9) [a, b, c] (testbase.rs Triangle :316-323); numpy or torch GPU tensor."""
        _keep, p, n, mem = _rows_in(tris, 9, self.ft, "triangle", check_tensor=False, convert=True)
        check(getattr(_lib.load(), f"bvhgpu_tree_set_triangles_{self.sfx}")(self._t, p, n, mem), self.ctx._h)

    def intersect_triangles(self, rays: RayBatch, stats: bool = False, coherent: bool = False, order: Optional[str] = None):
        """traverse + Ray::intersects_triangle on every returned shape (testbase.rs:826-836).
        returns (offsets, indices, isect[total,3] = Intersection{distance,u,v}, stats)"""
        lib = _lib.load()
        flags = TRAVERSE_TRIANGLES | (TRAVERSE_STATS if stats else 0) | (TRAVERSE_COHERENT if coherent else 0)
        flags |= _lib.ORDER_FLAGS[order]
        check(getattr(lib, f"bvhgpu_traverse_{self.sfx}")(self._t, rays._ptr(), rays.n, rays.mem, flags,
                                                           C.byref(self._hits.h)), self.ctx._h)
        total, sd = self._hits._stats()
        offsets = np.zeros(rays.n + 1, dtype=np.uint32)
        indices = np.zeros(total, dtype=np.uint32)
        isect = np.zeros((total, 3), dtype=self.ft)
        check(lib.bvhgpu_hits_fetch(self._hits.h, ptr(offsets), ptr(indices), None, HOST), self.ctx._h)
        check(lib.bvhgpu_hits_fetch_triangles(self._hits.h, ptr(isect), HOST), self.ctx._h)
        return offsets, indices, isect, sd

    def closest_hits(self, rays: RayBatch, stats: bool = False, fetch: bool = True, coherent: bool = False,
                     order: Optional[str] = None):
        """triangle stage fused into the walk: per ray the nearest Intersection and its shape
        (distance +inf / shape NONE when nothing is hit).  returns (isect[n,3], shape[n], stats)"""
        lib = _lib.load()
        flags = TRAVERSE_CLOSEST | (TRAVERSE_STATS if stats else 0) | (TRAVERSE_COHERENT if coherent else 0)
        flags |= _lib.ORDER_FLAGS[order]
        check(getattr(lib, f"bvhgpu_traverse_{self.sfx}")(self._t, rays._ptr(), rays.n, rays.mem, flags,
                                                           C.byref(self._hits.h)), self.ctx._h)
        _, sd = self._hits._stats(want_total=False)
        if not fetch:
            return None, None, sd
        return self._hits.fetch_closest(rays.n, self.ft) + (sd,)

    def _tmax_arg(self, rays: RayBatch, tmax):
        """per-ray segment ends of any_hits / the box queries → (array kept alive, pointer or None): n values in the tree's dtype in the
        rays' memory — a numpy array for HOST rays, a torch GPU tensor for rays in HBM"""
        return _side_in(tmax, rays.device, rays.n, rays.mem, self.ft, "tmax", "rays")

    def _tmax_batch(self, entry: str, fetcher, rays: RayBatch, tmax, flags: int, fetch: bool):
        """bvhgpu_traverse_<entry>_*, the ray batches with a per-ray tmax and one record per ray; `fetcher`: the _Hits.fetch_* of that entry"""
        if rays.sfx != self.sfx:
            raise BvhGpuError(_lib.DTYPE_MISMATCH, "ray dtype differs from tree dtype")
        keep, tp = self._tmax_arg(rays, tmax)   # (keep: the array tp points into stays alive over the call)
        fn = getattr(_lib.load(), f"bvhgpu_traverse_{entry}_{self.sfx}")
        check(fn(self._t, rays._ptr(), tp, rays.n, rays.mem, flags, C.byref(self._hits.h)), self.ctx._h)
        if not fetch:
            return None, None
        return fetcher(rays.n, self.ft)

    def any_hits(self, rays: RayBatch, tmax=None, fetch: bool = True, coherent: bool = False):
        """bvhgpu_traverse_any_*: occlusion of the segments o .. o + tmax[i]·d.  Per ray the FIRST shape of FlatBvh::traverse's list
        (flat_bvh.rs:396-431, in its order) whose Ray::intersects_triangle distance is < tmax[i], with that Intersection; shape NONE and
        (+inf, 0, 0) when there is none.  tmax: None (+inf for every ray), or n values in the tree's dtype in the rays' memory — a numpy
        array for HOST rays, a torch GPU tensor for rays in HBM.  Needs set_triangles.  returns (isect[n,3], shape[n]); fetch=False
        returns (None, None) and leaves the result on the tree's result object."""
        return self._tmax_batch("any", self._hits.fetch_any, rays, tmax, _ray_flags(coherent), fetch)

    def occluded(self, rays: RayBatch, tmax=None) -> np.ndarray:
        """bool[n]: does segment i hit any triangle (any_hits(...) shape != NONE)"""
        _, shape = self.any_hits(rays, tmax)
        return shape != NONE

    # ---- ray queries against the shapes' own boxes (no triangles) ---------------------------
    def closest_box_hits(self, rays: RayBatch, tmax=None, fetch: bool = True, coherent: bool = False):
        """bvhgpu_traverse_box_*: per ray the shape of FlatBvh::traverse's list (flat_bvh.rs:396-431) whose own AABB the ray enters first,
        among those with enter < tmax[i] (strict; the first of the list on equal entries), with Ray::intersection_slice_for_aabb's
        (enter, exit) on that box; shape NONE and (+inf, 0) when there is none.  No triangles needed.  tmax as for any_hits.
        returns (slice[n,2], shape[n]); fetch=False returns (None, None) and leaves the result on the tree's result object."""
        return self._tmax_batch("box", self._hits.fetch_box, rays, tmax, _ray_flags(coherent), fetch)

    def first_box_hits(self, rays: RayBatch, tmax=None, fetch: bool = True, coherent: bool = False):
        """bvhgpu_traverse_box_* with BVHGPU_TRAVERSE_FIRST: the FIRST shape of the ray's list with enter < tmax[i] instead of the
        nearest one (any-hit: every walk stops at it).  returns (slice[n,2], shape[n]) like closest_box_hits."""
        return self._tmax_batch("box", self._hits.fetch_box, rays, tmax, _ray_flags(coherent, first=True), fetch)

    def box_occluded(self, rays: RayBatch, tmax=None) -> np.ndarray:
        """bool[n]: does ray i enter any shape's box before tmax[i] (first_box_hits(...) shape != NONE)"""
        _, shape = self.first_box_hits(rays, tmax)
        return shape != NONE

    # ---- ray queries against sphere shapes (no triangles) -----------------------------------
    def set_spheres(self, spheres) -> None:
        """bvhgpu_tree_set_spheres_*: one sphere per shape, (n,4) [cx, cy, cz, r] in the tree's dtype; numpy or torch GPU tensor.  Independent
        of the AABBs the tree was built from (normally spheres_aabbs(spheres)); never validated."""
        _keep, p, n, mem = _rows_in(spheres, 4, self.ft, "sphere")
        check(getattr(_lib.load(), f"bvhgpu_tree_set_spheres_{self.sfx}")(self._t, p, n, mem), self.ctx._h)

    def closest_sphere_hits(self, rays: RayBatch, tmax=None, fetch: bool = True, coherent: bool = False):
        """bvhgpu_traverse_sphere_*: per ray the shape of FlatBvh::traverse's list (flat_bvh.rs:396-431) whose sphere (set_spheres) the ray
        hits nearest, among those with distance < tmax[i] (strict; the first of the list on equal distances), with (distance, exit) on
        that sphere; shape NONE and (+inf, 0) when there is none.  Needs set_spheres, no triangles.  tmax as for any_hits.
        returns (hit[n,2], shape[n]); fetch=False returns (None, None) and leaves the result on the tree's result object."""
        return self._tmax_batch("sphere", self._hits.fetch_sphere, rays, tmax, _ray_flags(coherent), fetch)

    def first_sphere_hits(self, rays: RayBatch, tmax=None, fetch: bool = True, coherent: bool = False):
        """bvhgpu_traverse_sphere_* with BVHGPU_TRAVERSE_FIRST: the FIRST shape of the ray's list whose sphere is hit with distance <
        tmax[i] instead of the nearest one (any-hit: every walk stops at it).  returns (hit[n,2], shape[n]) like closest_sphere_hits."""
        return self._tmax_batch("sphere", self._hits.fetch_sphere, rays, tmax, _ray_flags(coherent, first=True), fetch)

    def sphere_occluded(self, rays: RayBatch, tmax=None) -> np.ndarray:
        """bool[n]: does ray i hit any shape's sphere before tmax[i] (first_sphere_hits(...) shape != NONE)"""
        _, shape = self.first_sphere_hits(rays, tmax)
        return shape != NONE

    # ---- multi-hit ray queries ---------------------------------------------------------------
    def _leaf_kind(self, rays: RayBatch, leaf: str):
        """what khits_batch and allhits_batch check alike → (BVHGPU_LEAF_* kind, the rays' torch device or None for HOST rays)"""
        if rays.sfx != self.sfx:
            raise BvhGpuError(_lib.DTYPE_MISMATCH, "ray dtype differs from tree dtype")
        if leaf not in _lib.LEAF_KINDS:
            raise BvhGpuError(_lib.INVALID_ARG, f"leaf must be one of {sorted(_lib.LEAF_KINDS)}")
        return _lib.LEAF_KINDS[leaf], rays.device.device if rays.mem == DEVICE else None

    def _alloc_out(self, device, ishape, fshape):
        """the (shape, values) outputs a kernel writes in place → (shape, values, their two pointers), as _out_cols makes them"""
        (shape, vals), (sp, vp) = _out_cols(device, self.ft, (ishape, "index"), (fshape, "float"))
        return shape, vals, sp, vp

    def khits_batch(self, rays: RayBatch, k: int, leaf: str = "box", tmax=None):
        """bvhgpu_traverse_khits_*: the k nearest hits of every ray.  Row i is the candidates of FlatBvh::traverse's list (flat_bvh.rs:396-431)
        — the members whose leaf-stage distance is < tmax[i], strict — in a stable ascending sort by distance (equal distances in list
        order), cut to the first k.  leaf: "box" ({enter, exit} on the shape's own AABB), "triangle" (Intersection{distance, u, v}; needs
        set_triangles) or "sphere" ({distance, exit}; needs set_spheres).  1 <= k <= _lib.KHITS_MAX_K.  tmax as for any_hits.
        returns (vals[n, k, W], shape[n, k]), W = 3 for triangles, else 2; slots beyond the number of candidates hold NONE and (+inf, 0[, 0]).
        HOST rays: numpy out, shape as uint32.  Rays in HBM: torch tensors on the same device, written by the kernel with no host round
        trip, shape as torch.int32 — so NONE reads as -1 there."""
        kind, dev = self._leaf_kind(rays, leaf)
        k = int(k)
        rows = k if 1 <= k <= _lib.KHITS_MAX_K else 0     # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        _keep, tp = self._tmax_arg(rays, tmax)   # (_keep: the array tp points into stays alive over the call)
        shape, vals, sp, vp = self._alloc_out(dev, (rays.n, rows), (rays.n, rows, _lib.LEAF_WIDTH[kind]))
        fn = getattr(_lib.load(), f"bvhgpu_traverse_khits_{self.sfx}")
        check(fn(self._t, rays._ptr(), tp, rays.n, rays.mem, kind, k & 0xFFFFFFFF, sp, vp), self.ctx._h)
        return vals, shape

    def allhits_batch(self, rays: RayBatch, leaf: str = "box", tmax=None, sort: bool = True):
        """bvhgpu_traverse_allhits_*: every hit of every ray, as a CSR.  Row i is ALL candidates of FlatBvh::traverse's list (flat_bvh.rs:396-431)
        — the members whose leaf-stage distance is < tmax[i], strict — in a stable ascending sort by distance (equal distances in list
        order); sort=False (BVHGPU_ALLHITS_LIST_ORDER) leaves them in list order.  leaf and tmax as for khits_batch.
        returns (offsets[n+1], shape[total], vals[total, W]), W = 3 for triangles, else 2; no padding.  The first min(k, len) entries of a
        sorted row are khits_batch's row.  HOST rays: numpy out, offsets and shape as uint32.  Rays in HBM: torch tensors on the same
        device, shape as torch.int32, offsets as torch.int64."""
        kind, dev = self._leaf_kind(rays, leaf)
        _keep, tp = self._tmax_arg(rays, tmax)   # (_keep: the array tp points into stays alive over the call)
        if dev is not None:
            _torch_sync(dev)
        fn = getattr(_lib.load(), f"bvhgpu_traverse_allhits_{self.sfx}")
        check(fn(self._t, rays._ptr(), tp, rays.n, rays.mem, kind, 0 if sort else _lib.ALLHITS_LIST_ORDER, C.byref(self._hits.h)), self.ctx._h)
        return self._hits.fetch_allhits(rays.n, leaf, self.ft, dev)

    # ---- point query ---------------------------------------------------------------------
    def nearest_batch(self, points, triangles: bool = False):
        """<FlatBvh as BoundingHierarchy>::nearest_to (flat_bvh.rs:513-562) for many points.  Shape distance: the
        shape's own AABB (UnitBox, testbase.rs:101-105) or, with triangles=True, the closest point on the triangle
        (testbase.rs:436-443; needs set_triangles).  returns (shape[n] u32 — NONE for an empty hierarchy, dist[n]).
        On a Bvh this is Bvh::nearest_to answered by the flat loop: the distance is the same as the recursive form's
        (bvh_node.rs:327-374); on exact ties the two reference forms may name different shapes."""
        self._ready()
        _keep, pp, n, mem = _rows_in(points, 3, self.ft, "point", convert=True, device=False)
        shape, dist, sp, dp = self._alloc_out(None, n, n)
        fn = getattr(_lib.load(), f"bvhgpu_nearest_{self.sfx}")
        check(fn(self._t, pp, n, mem, 1 if triangles else 0, sp, dp), self.ctx._h)
        return shape, dist

    def _points_in(self, points, max_dist):
        """(n, 3) query points with their per-point limit (None, a scalar or n values in the points' memory) → (points kept alive, their
        pointer, n, HOST or DEVICE, max_dist kept alive, its pointer or None)"""
        p, pp, n, mem = _rows_in(points, 3, self.ft, "point")
        m, mp = _side_in(max_dist, p, n, mem, self.ft, "max_dist", "points", scalar_ok=True)
        return p, pp, n, mem, m, mp

    def _knearest(self, entry: str, points, k: int, triangles: bool, max_dist, with_limit: bool):
        """marshalling of knearest_batch (entry "knearest": no limit argument) and knearest_tree_batch ("knearest_tree": max_dist or NULL)"""
        fn = getattr(_lib.load(), f"bvhgpu_{entry}_{self.sfx}")
        k = int(k)
        rows = k if 1 <= k <= _lib.KNN_MAX_K else 0       # (out of range: the engine answers INVALID_ARG before it touches a buffer)
        p, pp, n, mem, _m, mp = self._points_in(points, max_dist)   # (p, _m: what the pointers point into stays alive over the call)
        shape, dist, sp, dp = self._alloc_out(p.device if mem == DEVICE else None, (n, rows), (n, rows))
        limit = (mp,) if with_limit else ()   # (bvhgpu_knearest_* has no max_dist argument)
        check(fn(self._t, pp, n, mem, 1 if triangles else 0, k & 0xFFFFFFFF, *limit, sp, dp), self.ctx._h)
        return shape, dist

    def knearest_batch(self, points, k: int, triangles: bool = False):
        """bvhgpu_knearest_*: the k nearest shapes of every point — the loop of nearest_to (flat_bvh.rs:524-558) with a list of at most k
        (distance, shape) pairs in place of best_element, every comparison the strict <.  1 <= k <= _lib.KNN_MAX_K.  Shape distance as
        for nearest_batch (triangles=True needs set_triangles; a point cloud is zero-size boxes with triangles=False).
        points: (n, 3) in the tree's dtype — a numpy array (HOST) or a torch GPU tensor (DEVICE).
        returns (shape[n, k], dist[n, k]): rows ascending in dist (a row that holds a NaN need not be sorted), equal distances in leaf
        pre-order; slots beyond the number of shapes hold NONE and +inf.  numpy in: numpy out, shape as uint32.  torch in: torch tensors on
        the same device, written by the kernel with no host round trip, shape as torch.int32 — so NONE reads as -1 there."""
        self._ready()
        return self._knearest("knearest", points, k, triangles, None, False)

    def knearest_tree_batch(self, points, k: int, triangles: bool = False, max_dist=None):
        """bvhgpu_knearest_tree_*: the rows of knearest_batch found nearest child first — BvhNode::nearest_to_recursive (bvh_node.rs:327-374,
        what Bvh::nearest_to calls) over the BvhNode array with the list of at most k (distance, shape) pairs in place of best_candidate.
        With k = 1 and no max_dist a row is what Bvh::nearest_to returns.  Equal distances stay in the order this walk meets them, which is
        not leaf pre-order: knearest_batch may order ties differently and pick differently among ties at the k-th distance.
        max_dist: None, a scalar (the same limit for every point) or n values in the points' memory — a numpy array for numpy points, a torch
        GPU tensor for tensor points.  Nothing farther than max_dist[i] enters row i (dist2 <= max_dist[i]^2); a negative or NaN limit gives
        a row of padding.  The tree must have been built here (a Bvh or its flatten(); no flatten is needed): an uploaded FlatBvh or an
        imported scene has no BvhNode array and raises INVALID_ARG.  points / returns: as knearest_batch."""
        return self._knearest("knearest_tree", points, k, triangles, max_dist, True)

    def within_batch(self, points, max_dist, triangles: bool = False, sort: bool = True, count_only: bool = False):
        """bvhgpu_within_*: every shape within max_dist[i] of point i, as a CSR — the loop of nearest_to (flat_bvh.rs:524-558) with the
        moving best_dist replaced by the fixed limit r2 = max_dist[i]^2 (one multiplication in the tree's dtype) and every comparison <=,
        so the limit itself is inside; a negative or NaN limit gives an empty row, +inf keeps every shape whose distance is not NaN.  Shape
        distance as for knearest_batch (triangles=True needs set_triangles).  Rows are in a stable ascending sort by distance, equal
        distances in leaf pre-order; sort=False (BVHGPU_WITHIN_LIST_ORDER) leaves them in the order the loop met them; count_only=True
        (BVHGPU_WITHIN_COUNT_ONLY) produces the offsets alone (shape and dist are empty).
        points: (n, 3) in the tree's dtype — a numpy array (HOST) or a torch GPU tensor (DEVICE).  max_dist: a scalar (the same limit for
        every point) or n values in the points' memory.
        returns (offsets[n+1], shape[total], dist[total]); no padding.  numpy in: numpy out, offsets and shape as uint32.  torch in: torch
        tensors on the same device, shape as torch.int32, offsets as torch.int64."""
        flags = (0 if sort else _lib.WITHIN_LIST_ORDER) | (_lib.WITHIN_COUNT_ONLY if count_only else 0)
        if max_dist is None:
            raise BvhGpuError(_lib.INVALID_ARG, "within_batch needs max_dist (a scalar or one value per point)")
        p, pp, n, mem, _m, mp = self._points_in(points, max_dist)   # (p, _m: what the pointers point into stays alive over the call)
        dev = p.device if mem == DEVICE else None
        if dev is not None:
            _torch_sync(dev)
        fn = getattr(_lib.load(), f"bvhgpu_within_{self.sfx}")
        check(fn(self._t, pp, mp, n, mem, 1 if triangles else 0, flags, C.byref(self._hits.h)), self.ctx._h)
        return self._hits.fetch_within(n, self.ft, dev, count_only)

    def nearest_to(self, query, shapes: Sequence, triangles: bool = False):
        """BoundingHierarchy::nearest_to (bounding_hierarchy.rs:262-336): Option<(&Shape, distance)>."""
        s, d = self.nearest_batch([query], triangles)
        return None if s[0] == NONE else (shapes[int(s[0])], d[0])

    def nearest_traverse(self, ray: "Ray", shapes: Sequence) -> List:
        """Bvh::nearest_traverse_iterator (bvh_impl.rs:145-151; DistanceTraverseIterator) collected into a list."""
        _, idx, _, _ = self.traverse_batch(ray._batch, order="nearest_heap")
        return [shapes[int(i)] for i in idx]

    def farthest_traverse(self, ray: "Ray", shapes: Sequence) -> List:
        """Bvh::farthest_traverse_iterator (bvh_impl.rs:162-176) collected into a list."""
        _, idx, _, _ = self.traverse_batch(ray._batch, order="farthest_heap")
        return [shapes[int(i)] for i in idx]

    def nearest_child_traverse(self, ray: "Ray", shapes: Sequence) -> List:
        """Bvh::nearest_child_traverse_iterator (bvh_impl.rs:184-190) collected into a list."""
        _, idx, _, _ = self.traverse_batch(ray._batch, order="nearest")
        return [shapes[i] for i in idx.tolist()]

    def farthest_child_traverse(self, ray: "Ray", shapes: Sequence) -> List:
        """Bvh::farthest_child_traverse_iterator (bvh_impl.rs:206-212) collected into a list."""
        _, idx, _, _ = self.traverse_batch(ray._batch, order="farthest")
        return [shapes[i] for i in idx.tolist()]

    def hits_device(self) -> Tuple[int, int]:
        """device addresses of the last result's (offsets, indices) — valid until the next traverse."""
        o, i, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(_lib.load().bvhgpu_hits_device(self._hits.h, C.byref(o), C.byref(i), C.byref(t)), self.ctx._h)
        return int(o.value or 0), int(i.value or 0)

    def traverse(self, query, shapes: Sequence) -> List:
        """BoundingHierarchy::traverse (bounding_hierarchy.rs:246-250): the shapes whose AABB `query` intersects, in the
        reference's order.  `query`: a Ray, an Aabb, a Ball / Sphere or a point (the crate's four IntersectsAabb types)."""
        self._ready()
        if isinstance(query, Ray):
            _, idx, _, _ = self.traverse_batch(query._batch)
        else:
            kind, row = _query_row(query, self.ft)
            _, idx = self.query_batch(kind, row.reshape(1, -1))
        return [shapes[i] for i in idx.tolist()]

    # ---- AABB / point / ball queries --------------------------------------------------------
    def query_batch(self, kind, queries, fetch: bool = True):
        """bvhgpu_query_*: FlatBvh::traverse (flat_bvh.rs:396-431) for a batch of AABB / point / ball queries.
        kind: "aabb" / "point" / "ball" (or _lib.QUERY_*); queries: (n, 6) / (n, 3) / (n, 4) in the tree's dtype — a numpy array
        (HOST) or a torch GPU tensor (DEVICE), or None with kind "aabb" for the tree's own shape AABBs (self_overlaps).
        returns (offsets[n+1], indices[total]) in the reference's per-query order; fetch=False returns (None, None) and leaves
        the result in HBM (hits_device)."""
        self._ready()
        kind = {"aabb": _lib.QUERY_AABB, "point": _lib.QUERY_POINT, "ball": _lib.QUERY_BALL, "sphere": _lib.QUERY_BALL}.get(kind, kind)
        if queries is None:
            _keep, qp, n, mem = None, None, self.info()[0], HOST
        else:
            _keep, qp, n, mem = _rows_in(queries, _lib.QUERY_WIDTH.get(kind, 1), self.ft, "query", exact=False)
        check(getattr(_lib.load(), f"bvhgpu_query_{self.sfx}")(self._t, kind, qp, n, mem, 0, C.byref(self._hits.h)), self.ctx._h)
        if not fetch:
            return None, None
        return self._hits.fetch(n)

    def self_overlaps(self, fetch: bool = True):
        """every shape's AABB against the tree (broad phase): row i = the shapes whose AABB touches shape i's, in the
        reference's order (row i contains i).  No upload: the tree's own boxes are the queries."""
        return self.query_batch(_lib.QUERY_AABB, None, fetch=fetch)

    def query_kernel(self) -> str:
        """the walk kernel of the last batch on this tree's result object (bvhgpu_hits_walk_kernel)"""
        return self._hits.walk_kernel()

    # ---- multi-GPU scene transport ---------------------------------------------------------
    def scene_nbytes(self) -> int:
        n = C.c_size_t()
        check(_lib.load().bvhgpu_scene_nbytes(self._t, C.byref(n)), self.ctx._h)
        return int(n.value)

    def scene_export(self, dst) -> None:
        """dst: torch uint8 tensor on the GPU (DEVICE) or a numpy uint8 array (HOST)."""
        p, mem = _bytes_in(dst)
        check(_lib.load().bvhgpu_scene_export(self._t, p, mem), self.ctx._h)


class FlatBvh(_TreeBase):
    """type FlatBvh = Vec<FlatNode> (flat_bvh.rs:254) resident in HBM."""

    @staticmethod
    def build(shapes: Sequence, dtype=np.float32, ctx: Optional[Context] = None) -> "FlatBvh":
        return Bvh.build(shapes, dtype, ctx).flatten()  # flat_bvh.rs:328-331

    @staticmethod
    def build_par(shapes: Sequence, dtype=np.float32, ctx: Optional[Context] = None) -> "FlatBvh":
        return Bvh.build_par(shapes, dtype, ctx).flatten()

    @property
    def nodes(self) -> np.ndarray:
        """the FlatNode array in the reference's layout (flat_bvh.rs:17-46)."""
        _, _, nf = self.info()
        out = np.zeros(nf, dtype=FLAT_F32 if self.sfx == "f32" else FLAT_F64)
        check(_lib.load().bvhgpu_flat_nodes(self._t, ptr(out), HOST), self.ctx._h)
        return out

    def __len__(self):
        return self.info()[2]

    @staticmethod
    def from_flat_nodes(flat: np.ndarray, shape_aabbs: np.ndarray, ctx: Optional[Context] = None) -> "FlatBvh":
        """Upload a FlatBvh produced elsewhere (e.g. by the Rust crate via flatten_custom)."""
        ctx = ctx or default_context()
        s = "f32" if flat.dtype == FLAT_F32 else "f64"
        sa = np.ascontiguousarray(shape_aabbs, dtype=_FT[s]).reshape(-1, 6)
        flat = np.ascontiguousarray(flat)
        h = C.c_void_p()
        fn = getattr(_lib.load(), f"bvhgpu_tree_from_flat_{s}")
        check(fn(ctx._h, ptr(flat), len(flat), ptr(sa), len(sa), C.byref(h)), ctx._h)
        return FlatBvh(ctx, h, s)

    @staticmethod
    def scene_import(src, nbytes: int, ctx: Optional[Context] = None, reuse: Optional["FlatBvh"] = None) -> "FlatBvh":
        """Import a scene blob (scene_export) — used on the peers after the RCCL broadcast.
        `reuse`: a FlatBvh from an earlier scene_import whose HBM is overwritten in place."""
        ctx = ctx or default_context()
        h = reuse._t if reuse is not None else C.c_void_p()
        p, mem = _bytes_in(src)
        check(_lib.load().bvhgpu_scene_import(ctx._h, p, nbytes, mem, C.byref(h)), ctx._h)
        dt = C.c_int()
        check(_lib.load().bvhgpu_tree_info(h, C.byref(dt), None, None, None), ctx._h)
        if reuse is not None:
            reuse.sfx = "f32" if dt.value == F32 else "f64"
            return reuse
        return FlatBvh(ctx, h, "f32" if dt.value == F32 else "f64")


class Bvh(_TreeBase):
    """struct Bvh {nodes: Vec<BvhNode>} (bvh_impl.rs:27-33), built and resident on the GPU."""

    # ---- construction ----------------------------------------------------------------------
    @staticmethod
    def from_aabbs(aabbs, ctx: Optional[Context] = None) -> "Bvh":
        """Build from an (n,6) array [min xyz, max xyz] (numpy → uploaded; torch GPU tensor → used in place)."""
        ctx = ctx or default_context()
        lib = _lib.load()
        h = C.c_void_p()
        if _is_device_tensor(aabbs):
            import torch  # only needed when the caller already uses torch
            s = "f32" if aabbs.dtype == torch.float32 else "f64"
        else:
            aabbs = np.asarray(aabbs)
            if aabbs.dtype not in (np.float32, np.float64):
                aabbs = aabbs.astype(np.float32)
            s = _sfx(aabbs.dtype)
        _keep, p, n, mem = _rows_in(aabbs, 6, _FT[s], "aabb", check_tensor=False)      # (the input's dtype is the tree's)
        check(getattr(lib, f"bvhgpu_build_{s}")(ctx._h, p, n, mem, C.byref(h)), ctx._h)
        return Bvh(ctx, h, s)

    def rebuild(self, aabbs, flatten: bool = False) -> "Bvh":
        """Bvh::build again into the same device buffers (no allocation when n fits).  flatten=True: FlatBvh::build
        (flat_bvh.rs:328-331) — build + flatten in one call."""
        fn = getattr(_lib.load(), f"bvhgpu_rebuild_flat_{self.sfx}" if flatten else f"bvhgpu_rebuild_{self.sfx}")
        _keep, p, n, mem = _rows_in(aabbs, 6, self.ft, "aabb", check_tensor=False, convert=True)
        check(fn(self._t, p, n, mem), self.ctx._h)
        return self

    def rebuild_async(self, aabbs) -> "Bvh":
        """bvhgpu_rebuild_flat_async_*: FlatBvh::build enqueued on the context's stream, no wait (`aabbs`: a GPU tensor, or a
        PinnedArray — either stays valid until wait()).  Everything that looks at the tree afterwards completes the build first."""
        fn = getattr(_lib.load(), f"bvhgpu_rebuild_flat_async_{self.sfx}")
        if isinstance(aabbs, np.ndarray) and getattr(aabbs, "_bvhgpu_pinned", False):
            check(fn(self._t, ptr(aabbs), aabbs.size // 6, HOST), self.ctx._h)
            return self
        if not _is_device_tensor(aabbs):
            raise BvhGpuError(_lib.INVALID_ARG, "rebuild_async takes shape AABBs that are resident in HBM (or in pinned host memory: pinned_array)")
        check(fn(self._t, ptr(aabbs.data_ptr()), aabbs.numel() // 6, DEVICE), self.ctx._h)
        return self

    def traverse_host(self, origins, directions, offsets: np.ndarray, indices: np.ndarray, coherent: bool = False, aabbs=None,
                      od6: bool = False) -> int:
        """bvhgpu_traverse_host_*: `for (o, d) in rays { flat.traverse(&Ray::new(o, d), shapes) }` for rays in host memory (n x 3 each;
        directions None: `origins` is an array of Ray structs), CSR written into the caller's `offsets` (n + 1) / `indices`; returns the
        hit total (indices are written when they fit: fetch with traverse_host_indices otherwise).  The tree may still be building.
        aabbs (host array, n x 6): bvhgpu_build_traverse_host_* — the tree is rebuilt from them first, underneath the ray upload.
        od6: `origins` is ONE array n x 6 = [o xyz, d xyz] per ray (BVHGPU_TRAVERSE_RAYS_OD6: one transfer per chunk), directions None."""
        lib = _lib.load()
        ft = self.ft
        if od6:
            assert directions is None and origins.dtype == ft and origins.flags.c_contiguous and origins.size % 6 == 0
            n = origins.size // 6
        elif directions is None:
            assert origins.dtype == _ray_dtype(self.sfx) and origins.flags.c_contiguous
            n = len(origins)
        else:
            assert origins.dtype == ft and directions.dtype == ft and origins.flags.c_contiguous and directions.flags.c_contiguous
            n = origins.size // 3
            assert directions.size == 3 * n
        assert offsets.dtype == np.uint32 and offsets.size >= n + 1 and indices.dtype == np.uint32
        total = C.c_uint64(0)
        tail = (ptr(origins), ptr(directions) if directions is not None else None, n,
                (TRAVERSE_COHERENT if coherent else 0) | (_lib.TRAVERSE_RAYS_OD6 if od6 else 0),
                ptr(offsets), ptr(indices), indices.size, C.byref(total))
        if aabbs is not None:
            assert aabbs.dtype == ft and aabbs.flags.c_contiguous
            check(getattr(lib, f"bvhgpu_build_traverse_host_{self.sfx}")(self._t, ptr(aabbs), aabbs.size // 6, *tail), self.ctx._h)
        else:
            check(getattr(lib, f"bvhgpu_traverse_host_{self.sfx}")(self._t, *tail), self.ctx._h)
        return int(total.value)

    def traverse_host_indices(self, indices: np.ndarray) -> None:
        check(_lib.load().bvhgpu_traverse_host_indices(self.ctx._h, ptr(indices), indices.size), self.ctx._h)

    def wait(self) -> "Bvh":
        check(_lib.load().bvhgpu_tree_wait(self._t), self.ctx._h)
        return self

    def refit(self, aabbs) -> "Bvh":
        """The shapes moved: same topology, every child AABB recomputed from the new shape AABBs
        (Bvh::fix_aabbs_ascending, optimization.rs:355-391, applied to the whole tree); a flattened tree is
        re-flattened.  ~2.5x cheaper than rebuild(flatten=True) (0.08 against 0.20 ms at 120 k shapes); update_shapes' re-insertion (optimization.rs:337-352) is not
        reproduced — rebuild() when the topology should follow the motion.  Input contract as for a build: with two or more
        shapes a NaN or ±inf component raises INVALID_ARG and leaves the tree exactly as it was; the call returns when that check
        has read the input (one host round trip)."""
        _keep, p, n, mem = _rows_in(aabbs, 6, self.ft, "aabb", check_tensor=False, convert=True)
        check(getattr(_lib.load(), f"bvhgpu_refit_{self.sfx}")(self._t, p, n, mem), self.ctx._h)
        return self

    @staticmethod
    def build(shapes: Sequence, dtype=np.float32, ctx: Optional[Context] = None) -> "Bvh":
        """Bvh::build (bvh_impl.rs:40-45).  Calls shape.aabb() ONCE per shape (the reference calls it
        once per level, only observable for impure aabb()), builds on the GPU, then calls
        shape.set_bh_node_index(leaf) for every shape (bvh_node.rs:102)."""
        n = len(shapes)
        a = np.empty((n, 6), dtype=dtype)
        for i, s in enumerate(shapes):
            a[i] = s.aabb().as6()
        bvh = Bvh.from_aabbs(a, ctx)
        if n:
            for s, ni in zip(shapes, bvh.shape_nodes.tolist()):
                s.set_bh_node_index(ni)
        return bvh

    @staticmethod
    def build_par(shapes: Sequence, dtype=np.float32, ctx: Optional[Context] = None) -> "Bvh":
        """BoundingHierarchy::build_par (bounding_hierarchy.rs:170-177): same tree; the GPU build is
        the parallel build."""
        return Bvh.build(shapes, dtype, ctx)

    @staticmethod
    def build_with_executor(shapes: Sequence, executor=None, dtype=np.float32, ctx: Optional[Context] = None) -> "Bvh":
        """bvh_impl.rs:53-96.  The executor only chooses how sub-builds are scheduled on the CPU and
        cannot change the result (node placement is arithmetic); the GPU schedules its own."""
        return Bvh.build(shapes, dtype, ctx)

    # ---- inspection ------------------------------------------------------------------------
    @property
    def nodes(self) -> np.ndarray:
        """Vec<BvhNode> as a structured array (include/bvh_mi355x.h bvhgpu_node_*)."""
        _, nn, _ = self.info()
        out = np.zeros(nn, dtype=NODE_F32 if self.sfx == "f32" else NODE_F64)
        check(_lib.load().bvhgpu_tree_nodes(self._t, ptr(out), HOST), self.ctx._h)
        return out

    @property
    def shape_nodes(self) -> np.ndarray:
        n, _, _ = self.info()
        out = np.zeros(n, dtype=np.uint32)
        check(_lib.load().bvhgpu_tree_shape_nodes(self._t, ptr(out), HOST), self.ctx._h)
        return out

    @property
    def build_levels(self) -> int:
        lv = C.c_int()
        check(_lib.load().bvhgpu_tree_build_levels(self._t, C.byref(lv)), self.ctx._h)
        return int(lv.value)

    # ---- flatten ---------------------------------------------------------------------------
    def flatten(self) -> "FlatBvh":
        """Bvh::flatten (flat_bvh.rs:312-319).  The flat arrays live in the same device object."""
        check(_lib.load().bvhgpu_flatten(self._t), self.ctx._h)
        f = FlatBvh.__new__(FlatBvh)
        f.ctx, f._t, f.sfx, f._hits = self.ctx, self._t, self.sfx, self._hits
        f._owner = self          # shares the handle; the Bvh keeps ownership
        f.__class__ = _FlatView
        return f

    def flatten_in_place(self) -> None:
        check(_lib.load().bvhgpu_flatten(self._t), self.ctx._h)

    # Bvh::traverse (bvh_impl.rs:104-119) and the other batch calls are answered by the flat walks: same hit list, same order
    # (bvh_node.rs:288-319 visits the same boxes in the same order), so a Bvh flattens before each of them
    _ready = flatten_in_place

    def khits_batch(self, rays: RayBatch, k: int, leaf: str = "box", tmax=None):
        self.flatten_in_place()
        return super().khits_batch(rays, k, leaf, tmax)

    def allhits_batch(self, rays: RayBatch, leaf: str = "box", tmax=None, sort: bool = True):
        self.flatten_in_place()
        return super().allhits_batch(rays, leaf, tmax, sort)

    def within_batch(self, points, max_dist, triangles: bool = False, sort: bool = True, count_only: bool = False):
        self.flatten_in_place()
        return super().within_batch(points, max_dist, triangles, sort, count_only)


class _FlatView(FlatBvh):
    """FlatBvh that borrows a Bvh's device object (so flatten() does not copy the tree)."""

    def close(self):  # the owning Bvh destroys the handle
        self._t = None

    def __del__(self):
        self._t = None

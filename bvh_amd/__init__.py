"""bvh_amd — MI355X-native (gfx950) engine for the hot path of the Rust crate `bvh`:
SAH build → flatten → batched ray / AABB / point / ball traversal, behind the C ABI in include/bvh_mi355x.h.

The package holds only what that path needs: csrc/ (HIP kernels + C ABI), _lib (ctypes binding),
api (mirror of the reference's Bounded / BHShape / BoundingHierarchy / Bvh / FlatBvh / Ray surface)
and testbase (the reference's scene and ray generators, used as synthetic inputs).
"""
from ._lib import BvhGpuError, NONE, device_count  # noqa: F401
from .api import (Aabb, Ball, BHShape, Bounded, Bvh, Context, FlatBvh, HostStep, Ray, RayBatch, Sphere,  # noqa: F401
                  default_context, pinned_array, spheres_aabbs)
from .instances import Instances  # noqa: F401
from .region import aabb_planes, frustum_planes, region_batch  # noqa: F401

__all__ = ["Aabb", "Ball", "Sphere", "BHShape", "Bounded", "Bvh", "Context", "FlatBvh", "HostStep", "Instances", "pinned_array", "Ray", "RayBatch", "BvhGpuError",
           "NONE", "device_count", "default_context", "spheres_aabbs", "aabb_planes", "frustum_planes", "region_batch"]

//! `GpuBvh<T>`: the `bvh` crate's `BoundingHierarchy<T, 3>` (src/bounding_hierarchy.rs:89-336) on an MI355X, for `T = f32`
//! and `T = f64`, over the C ABI of libbvh_mi355x.so (include/bvh_mi355x.h).  Build / flatten / batched traversal run on the
//! GPU and give the arrays the crate's own `Bvh::build` + `Bvh::flatten` + `FlatBvh::traverse` give, bit for bit (see
//! DESIGN.md §2), and so do batches of the crate's other query types (`traverse_aabbs` / `traverse_points` / `traverse_balls` /
//! `self_overlaps`); the trait's generic `traverse` (one query of any `IntersectsAabb` type — stable Rust cannot specialise it) and
//! arbitrary `PointDistance` callbacks run the crate's own loops over the downloaded flat array.
//!
//! The scalar type is a sealed trait (`GpuScalar`, implemented for `f32` and `f64` only — the two instantiations the
//! engine has): it names the `#[repr(C)]` images of `BvhNode` / `FlatNode` / `Ray` for that type and the `_f32` / `_f64` entry
//! points, so that `GpuBvh<T>` is written once.  `GpuBvh32` / `GpuBvh64` are the two aliases.
//!
//! Which GPU: `GpuBvh::from_aabbs(aabbs, device)` takes it explicitly; the trait's `build` (whose signature the crate fixes
//! and has no room for it) uses `default_device()`, a process-wide setting (`set_default_device`; initial value 0, or
//! `BVH_MI355X_DEVICE` from the environment).  Every `GpuBvh` remembers its device (`device()`).
//!
//! NOTE: written against bvh 0.12.0 / nalgebra 0.34 by reading their sources; the image this engine was developed in has
//! no cargo/rustc, so this crate has NOT been compiled there.  tests/test_abi_cpu.py checks every `extern "C"` declaration
//! of ffi.rs against the header (names, argument counts, argument and return types) on every CPU run.
#![allow(clippy::missing_safety_doc)]
pub mod ffi;

use bvh::aabb::{Aabb, IntersectsAabb};
use bvh::ball::Ball;
use bvh::bounding_hierarchy::{BHShape, BHValue, BoundingHierarchy};
use bvh::bvh::{Bvh, BvhNode, BvhNodeBuildArgs};
use bvh::flat_bvh::{FlatBvh, FlatNode};
use bvh::point_query::PointDistance;
use bvh::ray::{Intersection, Ray};
use core::ffi::{c_int, c_uint, c_void};
use core::sync::atomic::{AtomicI32, Ordering};
use nalgebra::{Point3, Vector3};

/// Panics with the engine's message: the crate has no error type, contract violations panic there too
/// (e.g. NaN centroids, src/bvh/bvh_node.rs:214-217).
fn check(ctx: *const ffi::bvhgpu_ctx, rc: c_int) {
    if rc != ffi::BVHGPU_OK {
        let msg = unsafe { std::ffi::CStr::from_ptr(ffi::bvhgpu_last_error(ctx)) };
        panic!("bvh_mi355x: status {rc}: {}", msg.to_string_lossy());
    }
}

static DEFAULT_DEVICE: AtomicI32 = AtomicI32::new(-1);

/// The GPU the trait's `build` / `build_par` use (their signatures are the crate's and carry no device argument).
pub fn default_device() -> i32 {
    let d = DEFAULT_DEVICE.load(Ordering::Relaxed);
    if d >= 0 {
        return d;
    }
    std::env::var("BVH_MI355X_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0)
}
/// One process per GPU: call this once with the local rank before the first `build`.
pub fn set_default_device(device: i32) {
    DEFAULT_DEVICE.store(device, Ordering::Relaxed);
}
/// Number of MI355X devices the engine sees (0 ⇒ every call fails with `BVHGPU_NO_DEVICE`: there is no CPU fallback)
pub fn device_count() -> i32 {
    let mut n: c_int = 0;
    unsafe { ffi::bvhgpu_device_count(&mut n) };
    n
}

mod sealed {
    pub trait Sealed {}
    impl Sealed for f32 {}
    impl Sealed for f64 {}
}

/// The two scalar types the engine is instantiated for.  Everything type-dependent at the boundary lives here.
pub trait GpuScalar: BHValue + sealed::Sealed + Default + 'static {
    /// `#[repr(C)]` image of `enum BvhNode<T,3>` (src/bvh/bvh_node.rs:21-47)
    type Node: Copy + Default;
    /// `#[repr(C)]` image of `struct FlatNode<T,3>` (src/flat_bvh.rs:17-46)
    type Flat: Copy + Default;
    /// `#[repr(C)]` image of `struct Ray<T,3>` (src/ray/ray_impl.rs:17-29)
    type RayC: Copy + Default;
    const DTYPE: c_int;

    unsafe fn build_flat(ctx: *mut ffi::bvhgpu_ctx, aabbs: *const Self, n: usize, mem: c_int, out: *mut *mut ffi::bvhgpu_tree) -> c_int;
    unsafe fn rebuild_flat(t: *mut ffi::bvhgpu_tree, aabbs: *const Self, n: usize, mem: c_int) -> c_int;
    unsafe fn rebuild_flat_async(t: *mut ffi::bvhgpu_tree, aabbs: *const Self, n: usize, mem: c_int) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn traverse_host(t: *mut ffi::bvhgpu_tree, origins: *const Self, directions: *const Self, n: usize, flags: c_uint, offsets: *mut u32, indices: *mut u32, cap: usize, total: *mut u64) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn build_traverse_host(t: *mut ffi::bvhgpu_tree, aabbs: *const Self, n_shapes: usize, origins: *const Self, directions: *const Self, n: usize, flags: c_uint, offsets: *mut u32, indices: *mut u32, cap: usize, total: *mut u64) -> c_int;
    unsafe fn refit(t: *mut ffi::bvhgpu_tree, aabbs: *const Self, n: usize, mem: c_int) -> c_int;
    unsafe fn traverse(t: *mut ffi::bvhgpu_tree, rays: *const Self::RayC, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int;
    unsafe fn set_triangles(t: *mut ffi::bvhgpu_tree, verts: *const Self, n: usize, mem: c_int) -> c_int;
    unsafe fn tree_from_flat(ctx: *mut ffi::bvhgpu_ctx, flat: *const Self::Flat, n_flat: usize, shape_aabbs: *const Self, n: usize, out: *mut *mut ffi::bvhgpu_tree) -> c_int;
    unsafe fn query(t: *mut ffi::bvhgpu_tree, kind: c_int, queries: *const Self, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn traverse_any(t: *mut ffi::bvhgpu_tree, rays: *const Self::RayC, tmax: *const Self, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn traverse_box(t: *mut ffi::bvhgpu_tree, rays: *const Self::RayC, tmax: *const Self, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int;
    unsafe fn set_spheres(t: *mut ffi::bvhgpu_tree, spheres: *const Self, n: usize, mem: c_int) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn traverse_sphere(t: *mut ffi::bvhgpu_tree, rays: *const Self::RayC, tmax: *const Self, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn knearest(t: *mut ffi::bvhgpu_tree, points: *const Self, n: usize, mem: c_int, kind: c_int, k: u32, out_shape: *mut u32, out_dist: *mut Self) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn knearest_tree(t: *mut ffi::bvhgpu_tree, points: *const Self, n: usize, mem: c_int, kind: c_int, k: u32, max_dist: *const Self, out_shape: *mut u32, out_dist: *mut Self) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn traverse_khits(t: *mut ffi::bvhgpu_tree, rays: *const Self::RayC, tmax: *const Self, n: usize, mem: c_int, leaf: c_int, k: u32, out_shape: *mut u32, out_vals: *mut Self) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn traverse_allhits(t: *mut ffi::bvhgpu_tree, rays: *const Self::RayC, tmax: *const Self, n: usize, mem: c_int, leaf: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int;
    #[allow(clippy::too_many_arguments)]
    unsafe fn within(t: *mut ffi::bvhgpu_tree, points: *const Self, max_dist: *const Self, n: usize, mem: c_int, kind: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int;
    unsafe fn region(t: *mut ffi::bvhgpu_tree, planes: *const Self, n: usize, m: u32, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int;

    fn node_to_crate(raw: &Self::Node) -> BvhNode<Self, 3>;
    fn flat_to_crate(raw: &Self::Flat) -> FlatNode<Self, 3>;
    fn flat_from_parts(aabb: &Aabb<Self, 3>, entry: u32, exit: u32, shape: u32) -> Self::Flat;
    fn ray_to_ffi(r: &Ray<Self, 3>) -> Self::RayC;
}

macro_rules! impl_gpu_scalar {
    ($t:ty, $dtype:expr, $node:ident, $flat:ident, $ray:ident, $build_flat:ident, $rebuild_flat:ident, $refit:ident, $traverse:ident,
     $set_tris:ident, $from_flat:ident, $rebuild_async:ident, $traverse_host:ident, $build_traverse_host:ident, $query:ident, $traverse_any:ident, $traverse_box:ident, $set_spheres:ident, $traverse_sphere:ident, $knearest:ident, $knearest_tree:ident, $traverse_khits:ident, $traverse_allhits:ident, $within:ident, $region:ident,
     $flat_ctor:expr) => {
        impl GpuScalar for $t {
            type Node = ffi::$node;
            type Flat = ffi::$flat;
            type RayC = ffi::$ray;
            const DTYPE: c_int = $dtype;
            unsafe fn build_flat(ctx: *mut ffi::bvhgpu_ctx, aabbs: *const $t, n: usize, mem: c_int, out: *mut *mut ffi::bvhgpu_tree) -> c_int {
                ffi::$build_flat(ctx, aabbs, n, mem, out)
            }
            unsafe fn rebuild_flat(t: *mut ffi::bvhgpu_tree, aabbs: *const $t, n: usize, mem: c_int) -> c_int {
                ffi::$rebuild_flat(t, aabbs, n, mem)
            }
            unsafe fn rebuild_flat_async(t: *mut ffi::bvhgpu_tree, aabbs: *const $t, n: usize, mem: c_int) -> c_int {
                ffi::$rebuild_async(t, aabbs, n, mem)
            }
            unsafe fn traverse_host(t: *mut ffi::bvhgpu_tree, origins: *const $t, directions: *const $t, n: usize, flags: c_uint, offsets: *mut u32, indices: *mut u32, cap: usize, total: *mut u64) -> c_int {
                ffi::$traverse_host(t, origins, directions, n, flags, offsets, indices, cap, total)
            }
            unsafe fn build_traverse_host(t: *mut ffi::bvhgpu_tree, aabbs: *const $t, n_shapes: usize, origins: *const $t, directions: *const $t, n: usize, flags: c_uint, offsets: *mut u32, indices: *mut u32, cap: usize, total: *mut u64) -> c_int {
                ffi::$build_traverse_host(t, aabbs, n_shapes, origins, directions, n, flags, offsets, indices, cap, total)
            }
            unsafe fn refit(t: *mut ffi::bvhgpu_tree, aabbs: *const $t, n: usize, mem: c_int) -> c_int {
                ffi::$refit(t, aabbs, n, mem)
            }
            unsafe fn traverse(t: *mut ffi::bvhgpu_tree, rays: *const ffi::$ray, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int {
                ffi::$traverse(t, rays, n, mem, flags, hits)
            }
            unsafe fn set_triangles(t: *mut ffi::bvhgpu_tree, verts: *const $t, n: usize, mem: c_int) -> c_int {
                ffi::$set_tris(t, verts, n, mem)
            }
            unsafe fn tree_from_flat(ctx: *mut ffi::bvhgpu_ctx, flat: *const ffi::$flat, n_flat: usize, shape_aabbs: *const $t, n: usize, out: *mut *mut ffi::bvhgpu_tree) -> c_int {
                ffi::$from_flat(ctx, flat, n_flat, shape_aabbs, n, out)
            }
            unsafe fn query(t: *mut ffi::bvhgpu_tree, kind: c_int, queries: *const $t, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int {
                ffi::$query(t, kind, queries, n, mem, flags, hits)
            }
            unsafe fn traverse_any(t: *mut ffi::bvhgpu_tree, rays: *const ffi::$ray, tmax: *const $t, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int {
                ffi::$traverse_any(t, rays, tmax, n, mem, flags, hits)
            }
            unsafe fn traverse_box(t: *mut ffi::bvhgpu_tree, rays: *const ffi::$ray, tmax: *const $t, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int {
                ffi::$traverse_box(t, rays, tmax, n, mem, flags, hits)
            }
            unsafe fn set_spheres(t: *mut ffi::bvhgpu_tree, spheres: *const $t, n: usize, mem: c_int) -> c_int {
                ffi::$set_spheres(t, spheres, n, mem)
            }
            unsafe fn traverse_sphere(t: *mut ffi::bvhgpu_tree, rays: *const ffi::$ray, tmax: *const $t, n: usize, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int {
                ffi::$traverse_sphere(t, rays, tmax, n, mem, flags, hits)
            }
            unsafe fn knearest(t: *mut ffi::bvhgpu_tree, points: *const $t, n: usize, mem: c_int, kind: c_int, k: u32, out_shape: *mut u32, out_dist: *mut $t) -> c_int {
                ffi::$knearest(t, points, n, mem, kind, k, out_shape, out_dist)
            }
            unsafe fn knearest_tree(t: *mut ffi::bvhgpu_tree, points: *const $t, n: usize, mem: c_int, kind: c_int, k: u32, max_dist: *const $t, out_shape: *mut u32, out_dist: *mut $t) -> c_int {
                ffi::$knearest_tree(t, points, n, mem, kind, k, max_dist, out_shape, out_dist)
            }
            unsafe fn traverse_khits(t: *mut ffi::bvhgpu_tree, rays: *const ffi::$ray, tmax: *const $t, n: usize, mem: c_int, leaf: c_int, k: u32, out_shape: *mut u32, out_vals: *mut $t) -> c_int {
                ffi::$traverse_khits(t, rays, tmax, n, mem, leaf, k, out_shape, out_vals)
            }
            unsafe fn traverse_allhits(t: *mut ffi::bvhgpu_tree, rays: *const ffi::$ray, tmax: *const $t, n: usize, mem: c_int, leaf: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int {
                ffi::$traverse_allhits(t, rays, tmax, n, mem, leaf, flags, hits)
            }
            unsafe fn within(t: *mut ffi::bvhgpu_tree, points: *const $t, max_dist: *const $t, n: usize, mem: c_int, kind: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int {
                ffi::$within(t, points, max_dist, n, mem, kind, flags, hits)
            }
            unsafe fn region(t: *mut ffi::bvhgpu_tree, planes: *const $t, n: usize, m: u32, mem: c_int, flags: c_uint, hits: *mut *mut ffi::bvhgpu_hits) -> c_int {
                ffi::$region(t, planes, n, m, mem, flags, hits)
            }
            fn node_to_crate(r: &ffi::$node) -> BvhNode<$t, 3> {
                if r.shape != ffi::BVHGPU_NONE {
                    BvhNode::Leaf { parent_index: r.parent as usize, shape_index: r.shape as usize }
                } else {
                    BvhNode::Node {
                        parent_index: r.parent as usize,
                        child_l_index: r.l as usize,
                        child_l_aabb: Aabb::with_bounds(Point3::from(r.l_min), Point3::from(r.l_max)),
                        child_r_index: r.r as usize,
                        child_r_aabb: Aabb::with_bounds(Point3::from(r.r_min), Point3::from(r.r_max)),
                    }
                }
            }
            fn flat_to_crate(f: &ffi::$flat) -> FlatNode<$t, 3> {
                FlatNode {
                    aabb: Aabb::with_bounds(Point3::from(f.min), Point3::from(f.max)),
                    entry_index: f.entry,
                    exit_index: f.exit,
                    shape_index: f.shape,
                }
            }
            fn flat_from_parts(aabb: &Aabb<$t, 3>, entry: u32, exit: u32, shape: u32) -> ffi::$flat {
                let ctor: fn([$t; 3], [$t; 3], u32, u32, u32) -> ffi::$flat = $flat_ctor;
                ctor([aabb.min.x, aabb.min.y, aabb.min.z], [aabb.max.x, aabb.max.y, aabb.max.z], entry, exit, shape)
            }
            fn ray_to_ffi(r: &Ray<$t, 3>) -> ffi::$ray {
                // Ray { origin, direction, inv_direction } (src/ray/ray_impl.rs:17-29): copied field by field, never transmuted
                ffi::$ray {
                    o: [r.origin.x, r.origin.y, r.origin.z],
                    d: [r.direction.x, r.direction.y, r.direction.z],
                    inv: [r.inv_direction.x, r.inv_direction.y, r.inv_direction.z],
                }
            }
        }
    };
}
impl_gpu_scalar!(f32, ffi::BVHGPU_F32, bvhgpu_node_f32, bvhgpu_flat_f32, bvhgpu_ray_f32, bvhgpu_build_flat_f32, bvhgpu_rebuild_flat_f32,
                 bvhgpu_refit_f32, bvhgpu_traverse_f32, bvhgpu_tree_set_triangles_f32, bvhgpu_tree_from_flat_f32,
                 bvhgpu_rebuild_flat_async_f32, bvhgpu_traverse_host_f32, bvhgpu_build_traverse_host_f32, bvhgpu_query_f32, bvhgpu_traverse_any_f32, bvhgpu_traverse_box_f32, bvhgpu_tree_set_spheres_f32, bvhgpu_traverse_sphere_f32, bvhgpu_knearest_f32, bvhgpu_knearest_tree_f32, bvhgpu_traverse_khits_f32, bvhgpu_traverse_allhits_f32, bvhgpu_within_f32, bvhgpu_region_f32,
                 |min, max, entry, exit, shape| ffi::bvhgpu_flat_f32 { min, max, entry, exit, shape });
impl_gpu_scalar!(f64, ffi::BVHGPU_F64, bvhgpu_node_f64, bvhgpu_flat_f64, bvhgpu_ray_f64, bvhgpu_build_flat_f64, bvhgpu_rebuild_flat_f64,
                 bvhgpu_refit_f64, bvhgpu_traverse_f64, bvhgpu_tree_set_triangles_f64, bvhgpu_tree_from_flat_f64,
                 bvhgpu_rebuild_flat_async_f64, bvhgpu_traverse_host_f64, bvhgpu_build_traverse_host_f64, bvhgpu_query_f64, bvhgpu_traverse_any_f64, bvhgpu_traverse_box_f64, bvhgpu_tree_set_spheres_f64, bvhgpu_traverse_sphere_f64, bvhgpu_knearest_f64, bvhgpu_knearest_tree_f64, bvhgpu_traverse_khits_f64, bvhgpu_traverse_allhits_f64, bvhgpu_within_f64, bvhgpu_region_f64,
                 |min, max, entry, exit, shape| ffi::bvhgpu_flat_f64 { min, max, entry, exit, shape, _pad: 0 });

fn aabb_to_6<T: GpuScalar>(b: &Aabb<T, 3>) -> [T; 6] {
    [b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z]
}

pub fn ray_to_ffi<T: GpuScalar>(r: &Ray<T, 3>) -> T::RayC {
    T::ray_to_ffi(r)
}

pub struct GpuBvh<T: GpuScalar> {
    ctx: *mut ffi::bvhgpu_ctx,
    tree: *mut ffi::bvhgpu_tree,
    device: i32,
    n_shapes: usize,
    /// CPU copy of the flat array in the crate's own layout, for the generic queries of the trait
    flat: FlatBvh<T, 3>,
    /// `rebuild_async` ran and `sync_flat` has not: the CPU copy is the previous tree's
    flat_stale: bool,
}
/// `BoundingHierarchy<f32, 3>` on the GPU (BASELINE configs[1]-[3])
pub type GpuBvh32 = GpuBvh<f32>;
/// `BoundingHierarchy<f64, 3>` on the GPU (BASELINE configs[4]: tree, rays and every test that decides a hit in double precision)
pub type GpuBvh64 = GpuBvh<f64>;

// the handles are only used through &self / &mut self; the engine's ctx is not internally locked: one GpuBvh per thread
unsafe impl<T: GpuScalar> Send for GpuBvh<T> {}

/// CSR result of a batch: ray i hit `indices[offsets[i]..offsets[i+1]]`, in the order `FlatBvh::traverse` returns them
pub struct BatchHits {
    pub offsets: Vec<u32>,
    pub indices: Vec<u32>,
}

/// Result of the reference harness' inner loop for one ray (src/testbase.rs:826-836): the nearest
/// `Ray::intersects_triangle` over the candidates `FlatBvh::traverse` returns; `shape == u32::MAX` and
/// `distance == +inf` when the ray hits nothing
pub struct ClosestHit<T> {
    pub intersection: Intersection<T>,
    pub shape: u32,
}

/// Result of a ray query against the shapes' own boxes (`GpuBvh::traverse_box`): `Ray::intersection_slice_for_aabb`'s `(enter, exit)` on the
/// winning shape's AABB and that shape; `shape == u32::MAX`, `enter == +inf` and `exit == 0` when the ray has no candidate
pub struct BoxHit<T> {
    pub enter: T,
    pub exit: T,
    pub shape: u32,
}

/// Result of a ray query against sphere shapes (`GpuBvh::closest_sphere_hits` / `first_sphere_hits`): the ray parameters at which it enters
/// (`distance`; the exit for an origin inside) and leaves (`exit`) the winning shape's sphere, and that shape; `shape == u32::MAX`,
/// `distance == +inf` and `exit == 0` when the ray has no candidate
pub struct SphereHit<T> {
    pub distance: T,
    pub exit: T,
    pub shape: u32,
}

/// A fixed-length slice in pinned host memory (`bvhgpu_host_alloc` / `bvhgpu_host_free`); derefs to `[U]`.  Must not outlive the
/// `GpuBvh` it came from.
pub struct PinnedVec<U> {
    ctx: *mut ffi::bvhgpu_ctx,
    ptr: *mut U,
    len: usize,
}
impl<U> core::ops::Deref for PinnedVec<U> {
    type Target = [U];
    fn deref(&self) -> &[U] {
        unsafe { core::slice::from_raw_parts(self.ptr, self.len) }
    }
}
impl<U> core::ops::DerefMut for PinnedVec<U> {
    fn deref_mut(&mut self) -> &mut [U] {
        unsafe { core::slice::from_raw_parts_mut(self.ptr, self.len) }
    }
}
impl<U> Drop for PinnedVec<U> {
    fn drop(&mut self) {
        unsafe { ffi::bvhgpu_host_free(self.ctx, self.ptr.cast()) };
    }
}

impl<T: GpuScalar> GpuBvh<T> {
    /// Bvh::build_par + Bvh::flatten on GPU `device` from the shapes' AABBs (n x [min xyz, max xyz])
    pub fn from_aabbs(aabbs: &[[T; 6]], device: i32) -> GpuBvh<T> {
        let mut ctx = core::ptr::null_mut();
        let mut tree = core::ptr::null_mut();
        unsafe {
            check(ctx, ffi::bvhgpu_create(device, core::ptr::null_mut(), &mut ctx));
            check(ctx, T::build_flat(ctx, aabbs.as_ptr().cast(), aabbs.len(), ffi::BVHGPU_HOST, &mut tree));
        }
        let mut me = GpuBvh { ctx, tree, device, n_shapes: aabbs.len(), flat: Vec::new(), flat_stale: false };
        me.flat = me.download_flat();
        me
    }

    /// the GPU this hierarchy lives on
    pub fn device(&self) -> i32 {
        self.device
    }

    /// the argument of `BHShape::set_bh_node_index` for every shape (src/bvh/bvh_node.rs:102)
    pub fn shape_nodes(&self) -> Vec<u32> {
        let mut sn = vec![0u32; self.n_shapes];
        unsafe { check(self.ctx, ffi::bvhgpu_tree_shape_nodes(self.tree, sn.as_mut_ptr(), ffi::BVHGPU_HOST)); }
        sn
    }

    /// `Vec<BvhNode>` exactly as `Bvh::build` produces it (bit-identical AABBs, same indices)
    pub fn to_bvh(&self) -> Bvh<T, 3> {
        let nn = if self.n_shapes == 0 { 0 } else { 2 * self.n_shapes - 1 };
        let mut raw = vec![T::Node::default(); nn];
        unsafe { check(self.ctx, ffi::bvhgpu_tree_nodes(self.tree, raw.as_mut_ptr().cast(), ffi::BVHGPU_HOST)); }
        Bvh { nodes: raw.iter().map(T::node_to_crate).collect() }
    }

    fn download_flat(&self) -> FlatBvh<T, 3> {
        let nf = if self.n_shapes >= 2 { 3 * self.n_shapes - 2 } else { self.n_shapes };
        let mut raw = vec![T::Flat::default(); nf];
        unsafe { check(self.ctx, ffi::bvhgpu_flat_nodes(self.tree, raw.as_mut_ptr().cast(), ffi::BVHGPU_HOST)); }
        raw.iter().map(T::flat_to_crate).collect()
    }

    /// `FlatBvh::traverse` (src/flat_bvh.rs:396-431) for many boxes at once: query i's list is `flat.traverse(&aabbs[i], shapes)`'s
    /// shape indices, in its order (`Aabb::intersects_aabb`, src/aabb/aabb_impl.rs:240-248; touching boxes count)
    pub fn traverse_aabbs(&self, aabbs: &[Aabb<T, 3>]) -> BatchHits {
        let q: Vec<[T; 6]> = aabbs.iter().map(aabb_to_6).collect();
        self.query_batch(ffi::BVHGPU_QUERY_AABB, q.as_ptr().cast(), q.len())
    }

    /// The same for points (`Aabb::contains`, src/aabb/aabb_impl.rs:175-177)
    pub fn traverse_points(&self, points: &[Point3<T>]) -> BatchHits {
        let q: Vec<[T; 3]> = points.iter().map(|p| [p.x, p.y, p.z]).collect();
        self.query_batch(ffi::BVHGPU_QUERY_POINT, q.as_ptr().cast(), q.len())
    }

    /// The same for balls / spheres (`Ball::intersects_aabb`, src/ball.rs:85-99)
    pub fn traverse_balls(&self, balls: &[Ball<T, 3>]) -> BatchHits {
        let q: Vec<[T; 4]> = balls.iter().map(|b| [b.center.x, b.center.y, b.center.z, b.radius]).collect();
        self.query_batch(ffi::BVHGPU_QUERY_BALL, q.as_ptr().cast(), q.len())
    }

    /// Broad phase: every shape's AABB against the hierarchy (row i = the shapes whose AABB touches shape i's, in
    /// `FlatBvh::traverse` order; row i contains i).  The tree's own copy of the boxes is the query batch: nothing is uploaded.
    pub fn self_overlaps(&self) -> BatchHits {
        self.query_batch(ffi::BVHGPU_QUERY_AABB, core::ptr::null(), self.n_shapes)
    }

    fn query_batch(&self, kind: c_int, queries: *const T, n: usize) -> BatchHits {
        assert!(!self.flat_stale, "rebuild_async: call sync_flat() before a query batch");
        let mut hits = core::ptr::null_mut();
        let mut offsets = vec![0u32; n + 1];
        let mut total = 0u64;
        unsafe {
            let rc = T::query(self.tree, kind, queries, n, ffi::BVHGPU_HOST, 0, &mut hits);
            if rc == ffi::BVHGPU_OK {
                check(self.ctx, ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut()));
            }
            let mut indices = vec![0u32; if rc == ffi::BVHGPU_OK { total as usize } else { 0 }];
            let rc2 = if rc == ffi::BVHGPU_OK {
                ffi::bvhgpu_hits_fetch(hits, offsets.as_mut_ptr(), indices.as_mut_ptr(), core::ptr::null_mut(), ffi::BVHGPU_HOST)
            } else {
                rc
            };
            ffi::bvhgpu_hits_destroy(hits);
            check(self.ctx, rc2);
            BatchHits { offsets, indices }
        }
    }

    /// `FlatBvh::traverse` (src/flat_bvh.rs:396-431) for many rays at once — what the GPU is for
    pub fn traverse_batch(&self, rays: &[Ray<T, 3>]) -> BatchHits {
        // `bvhgpu_traverse_host_*` with directions == NULL: the crate's own Ray structs (origin, direction, inv_direction), uploaded in
        // chunks beside the walk of the previous chunk, CSR offsets downloaded behind it — one call, one host wait
        let r: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        self.host_batch(r.as_ptr().cast(), core::ptr::null(), r.len())
    }

    /// The same for rays given as origins and directions (what `Ray::new` takes, src/ray/ray_impl.rs:70-80): `Ray::new` runs on the
    /// device — the correctly rounded divide and square root give its bits — and 24 bytes per ray cross the link instead of 36.
    /// With both slices in pinned memory (`PinnedVec`) the copies are DMA at link speed.
    pub fn traverse_batch_od(&self, origins: &[[T; 3]], directions: &[[T; 3]]) -> BatchHits {
        assert_eq!(origins.len(), directions.len(), "one direction per origin");
        self.host_batch(origins.as_ptr().cast(), directions.as_ptr().cast(), origins.len())
    }

    /// One frame of a host-resident caller in one call: `rebuild(aabbs)` + `traverse_batch_od(origins, directions)`, the ray upload
    /// enqueued before the build so that the build runs underneath it (`bvhgpu_build_traverse_host_*`).  The CPU copy the trait's
    /// generic queries walk is refreshed by `sync_flat()`.
    pub fn rebuild_and_traverse(&mut self, aabbs: &[[T; 6]], origins: &[[T; 3]], directions: &[[T; 3]]) -> BatchHits {
        assert_eq!(origins.len(), directions.len(), "one direction per origin");
        let n = origins.len();
        let mut offsets = vec![0u32; n + 1];
        let mut indices = vec![0u32; n.max(1 << 16)];
        let mut total = 0u64;
        unsafe {
            check(self.ctx, T::build_traverse_host(self.tree, aabbs.as_ptr().cast(), aabbs.len(), origins.as_ptr().cast(), directions.as_ptr().cast(), n, 0,
                                                   offsets.as_mut_ptr(), indices.as_mut_ptr(), indices.len(), &mut total));
            if total as usize > indices.len() {
                indices.resize(total as usize, 0);
                check(self.ctx, ffi::bvhgpu_traverse_host_indices(self.ctx, indices.as_mut_ptr(), indices.len()));
            }
        }
        self.n_shapes = aabbs.len();
        self.flat_stale = true;
        indices.truncate(total as usize);
        BatchHits { offsets, indices }
    }

    /// ... and as ONE slice of `[o.x, o.y, o.z, d.x, d.y, d.z]` per ray (`BVHGPU_TRAVERSE_RAYS_OD6`): one transfer per chunk instead of two
    pub fn traverse_batch_od6(&self, rays: &[[T; 6]]) -> BatchHits {
        self.host_batch_flags(rays.as_ptr().cast(), core::ptr::null(), rays.len(), ffi::BVHGPU_TRAVERSE_RAYS_OD6)
    }

    fn host_batch(&self, origins: *const T, directions: *const T, n: usize) -> BatchHits {
        self.host_batch_flags(origins, directions, n, 0)
    }

    fn host_batch_flags(&self, origins: *const T, directions: *const T, n: usize, flags: c_uint) -> BatchHits {
        let mut offsets = vec![0u32; n + 1];
        let mut indices = vec![0u32; n.max(1 << 16)];
        let mut total = 0u64;
        unsafe {
            check(self.ctx, T::traverse_host(self.tree, origins, directions, n, flags, offsets.as_mut_ptr(), indices.as_mut_ptr(), indices.len(), &mut total));
            if total as usize > indices.len() {
                indices.resize(total as usize, 0);
                check(self.ctx, ffi::bvhgpu_traverse_host_indices(self.ctx, indices.as_mut_ptr(), indices.len()));
            }
        }
        indices.truncate(total as usize);
        BatchHits { offsets, indices }
    }

    /// `rebuild` without the wait: the build is enqueued and the call returns; a `traverse_batch*` that follows uploads its rays
    /// beside it.  `aabbs` must stay untouched until the next call that looks at the tree (pinned memory: the copy is asynchronous).
    pub fn rebuild_async(&mut self, aabbs: &[[T; 6]]) {
        unsafe { check(self.ctx, T::rebuild_flat_async(self.tree, aabbs.as_ptr().cast(), aabbs.len(), ffi::BVHGPU_HOST)); }
        self.n_shapes = aabbs.len();
        self.flat_stale = true;
    }

    /// Pinned host memory for `n` elements on this hierarchy's ctx (`bvhgpu_host_alloc`): read and written by the DMA engines directly
    pub fn pinned<U: Copy + Default>(&self, n: usize) -> PinnedVec<U> {
        let mut p = core::ptr::null_mut();
        unsafe { check(self.ctx, ffi::bvhgpu_host_alloc(self.ctx, n * core::mem::size_of::<U>(), &mut p)); }
        let v = PinnedVec { ctx: self.ctx, ptr: p.cast::<U>(), len: n };
        for i in 0..n {
            unsafe { v.ptr.add(i).write(U::default()) };
        }
        v
    }

    /// The triangle stage needs the vertices (one triangle per shape, n x [a xyz, b xyz, c xyz]): src/testbase.rs:325-333
    pub fn set_triangles(&mut self, verts: &[[T; 9]]) {
        assert_eq!(verts.len(), self.n_shapes, "one triangle per shape");
        unsafe { check(self.ctx, T::set_triangles(self.tree, verts.as_ptr().cast(), verts.len(), ffi::BVHGPU_HOST)); }
    }

    /// The harness loop of the reference's benches for a whole batch (src/testbase.rs:826-836): per ray, `FlatBvh::traverse` then
    /// `Ray::intersects_triangle` (src/ray/ray_impl.rs:154-213) on every candidate, keeping the nearest — fused into the walk on
    /// the GPU (`BVHGPU_TRAVERSE_CLOSEST`).  Needs `set_triangles`.
    pub fn traverse_closest(&self, rays: &[Ray<T, 3>]) -> Vec<ClosestHit<T>> {
        let r: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let mut hits = core::ptr::null_mut();
        let mut isect = vec![[T::default(); 3]; rays.len()];
        let mut shape = vec![0u32; rays.len()];
        unsafe {
            check(self.ctx, T::traverse(self.tree, r.as_ptr(), r.len(), ffi::BVHGPU_HOST, ffi::BVHGPU_TRAVERSE_CLOSEST, &mut hits));
            check(self.ctx, ffi::bvhgpu_hits_fetch_closest(hits, isect.as_mut_ptr() as *mut c_void, shape.as_mut_ptr(), ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        isect.iter().zip(shape).map(|(i, s)| ClosestHit { intersection: Intersection::new(i[0], i[1], i[2]), shape: s }).collect()
    }

    /// Occlusion of ray segments (shadow / visibility rays, `bvhgpu_traverse_any_*`): per ray the FIRST shape of `FlatBvh::traverse`'s
    /// list, in its order, whose `Ray::intersects_triangle` distance is `< tmax[i]` (`tmax: None` = +inf for every ray), with that
    /// Intersection; `shape == u32::MAX` and `distance == +inf` when the segment hits nothing.  Every walk stops at the first such
    /// candidate.  Needs `set_triangles`.
    pub fn traverse_any(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>) -> Vec<ClosestHit<T>> {
        if let Some(tm) = tmax {
            assert_eq!(tm.len(), rays.len(), "one tmax per ray");
        }
        let r: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let mut hits = core::ptr::null_mut();
        let mut isect = vec![[T::default(); 3]; rays.len()];
        let mut shape = vec![0u32; rays.len()];
        let tp = tmax.map_or(core::ptr::null(), |t| t.as_ptr());
        unsafe {
            check(self.ctx, T::traverse_any(self.tree, r.as_ptr(), tp, r.len(), ffi::BVHGPU_HOST, 0, &mut hits));
            check(self.ctx, ffi::bvhgpu_hits_fetch_any(hits, isect.as_mut_ptr() as *mut c_void, shape.as_mut_ptr(), ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        isect.iter().zip(shape).map(|(i, s)| ClosestHit { intersection: Intersection::new(i[0], i[1], i[2]), shape: s }).collect()
    }

    /// `traverse_any` reduced to one flag per ray: does segment i hit any triangle
    pub fn occluded(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>) -> Vec<bool> {
        self.traverse_any(rays, tmax).iter().map(|h| h.shape != ffi::BVHGPU_NONE).collect()
    }

    /// Ray queries against the shapes' own boxes, no triangles needed (`bvhgpu_traverse_box_*`): per ray, among the shapes of
    /// `FlatBvh::traverse`'s list whose `Ray::intersection_slice_for_aabb` entry is `< tmax[i]` (strict; `tmax: None` = +inf for every ray),
    /// the one entered first — the first of the list on equal entries — or, with `first`, the first of the list (any-hit: every walk stops
    /// at it).
    pub fn traverse_box(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, first: bool) -> Vec<BoxHit<T>> {
        if let Some(tm) = tmax {
            assert_eq!(tm.len(), rays.len(), "one tmax per ray");
        }
        let r: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let mut hits = core::ptr::null_mut();
        let mut slice = vec![[T::default(); 2]; rays.len()];
        let mut shape = vec![0u32; rays.len()];
        let tp = tmax.map_or(core::ptr::null(), |t| t.as_ptr());
        let flags = if first { ffi::BVHGPU_TRAVERSE_FIRST } else { 0 };
        unsafe {
            check(self.ctx, T::traverse_box(self.tree, r.as_ptr(), tp, r.len(), ffi::BVHGPU_HOST, flags, &mut hits));
            check(self.ctx, ffi::bvhgpu_hits_fetch_box(hits, slice.as_mut_ptr() as *mut c_void, shape.as_mut_ptr(), ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        slice.iter().zip(shape).map(|(t, s)| BoxHit { enter: t[0], exit: t[1], shape: s }).collect()
    }

    /// One sphere per shape, `[cx, cy, cz, r]` (`bvhgpu_tree_set_spheres_*`): the leaf primitive of the sphere queries.  Independent of the
    /// AABBs the tree was built from — normally `c ∓ r`, as the reference's `examples/simple.rs` builds them; never validated.
    pub fn set_spheres(&mut self, spheres: &[[T; 4]]) {
        assert_eq!(spheres.len(), self.n_shapes, "one sphere per shape");
        unsafe { check(self.ctx, T::set_spheres(self.tree, spheres.as_ptr().cast(), spheres.len(), ffi::BVHGPU_HOST)); }
    }

    fn sphere_hits(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, first: bool) -> Vec<SphereHit<T>> {
        if let Some(tm) = tmax {
            assert_eq!(tm.len(), rays.len(), "one tmax per ray");
        }
        let r: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let mut hits = core::ptr::null_mut();
        let mut hit = vec![[T::default(); 2]; rays.len()];
        let mut shape = vec![0u32; rays.len()];
        let tp = tmax.map_or(core::ptr::null(), |t| t.as_ptr());
        let flags = if first { ffi::BVHGPU_TRAVERSE_FIRST } else { 0 };
        unsafe {
            check(self.ctx, T::traverse_sphere(self.tree, r.as_ptr(), tp, r.len(), ffi::BVHGPU_HOST, flags, &mut hits));
            check(self.ctx, ffi::bvhgpu_hits_fetch_sphere(hits, hit.as_mut_ptr() as *mut c_void, shape.as_mut_ptr(), ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        hit.iter().zip(shape).map(|(t, s)| SphereHit { distance: t[0], exit: t[1], shape: s }).collect()
    }

    /// What `examples/simple.rs` computes on the host after `traverse`, fused into the walk (`bvhgpu_traverse_sphere_*`): per ray, among
    /// the shapes of `FlatBvh::traverse`'s list whose sphere the ray hits with `distance < tmax[i]` (strict; `tmax: None` = +inf for every
    /// ray), the nearest one — the first of the list on equal distances.  Needs `set_spheres`.
    pub fn closest_sphere_hits(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>) -> Vec<SphereHit<T>> {
        self.sphere_hits(rays, tmax, false)
    }

    /// ... the FIRST such shape of the list instead of the nearest one (`BVHGPU_TRAVERSE_FIRST`, any-hit: every walk stops at it)
    pub fn first_sphere_hits(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>) -> Vec<SphereHit<T>> {
        self.sphere_hits(rays, tmax, true)
    }

    /// `first_sphere_hits` reduced to one flag per ray: does ray i hit any sphere before `tmax[i]`
    pub fn sphere_occluded(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>) -> Vec<bool> {
        self.first_sphere_hits(rays, tmax).iter().map(|h| h.shape != ffi::BVHGPU_NONE).collect()
    }

    /// The `k` nearest hits of every ray (`bvhgpu_traverse_khits_*`): the members of `FlatBvh::traverse`'s list whose leaf-stage distance is
    /// `< tmax[i]` (strict; `tmax: None` = +inf for every ray), in a stable ascending sort by distance — equal distances in list order — cut
    /// to the first `k`.  `leaf`: `ffi::BVHGPU_LEAF_BOX` (`{enter, exit}` on the shape's own AABB), `ffi::BVHGPU_LEAF_TRIANGLE`
    /// (`Intersection{distance, u, v}`; needs `set_triangles`) or `ffi::BVHGPU_LEAF_SPHERE` (`{distance, exit}`; needs `set_spheres`).
    /// Returns row-major `rays.len() x k` shape indices and `rays.len() x k x W` record scalars (W = 3 for triangles, else 2); slots beyond
    /// the number of candidates hold `u32::MAX` and `{+inf, 0[, 0]}`.  `1 <= k <= ffi::BVHGPU_KHITS_MAX_K`.
    pub fn traverse_khits(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, leaf: c_int, k: usize) -> (Vec<u32>, Vec<T>) {
        if let Some(tm) = tmax {
            assert_eq!(tm.len(), rays.len(), "one tmax per ray");
        }
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_KHITS_MAX_K).contains(&k32) { rays.len() * k } else { 0 };
        let w = if leaf == ffi::BVHGPU_LEAF_TRIANGLE { 3 } else { 2 };
        let r: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let mut shape = vec![0u32; slots];
        let mut vals = vec![T::default(); slots * w];
        unsafe {
            check(self.ctx, T::traverse_khits(self.tree, r.as_ptr(), tmax.map_or(core::ptr::null(), |t| t.as_ptr()), r.len(), ffi::BVHGPU_HOST,
                                              leaf, k32, shape.as_mut_ptr(), vals.as_mut_ptr()));
        }
        (shape, vals)
    }

    /// EVERY hit of every ray, as a CSR (`bvhgpu_traverse_allhits_*`): row i is all members of `FlatBvh::traverse`'s list whose leaf-stage
    /// distance is `< tmax[i]` (strict; `tmax: None` = +inf for every ray), in a stable ascending sort by distance — equal distances in list
    /// order — or, with `sort: false` (`ffi::BVHGPU_ALLHITS_LIST_ORDER`), in list order.  `leaf` as for `traverse_khits`.  Returns
    /// `(offsets, shape, vals)`: `rays.len() + 1` exclusive prefix sums of the row lengths, `total` shape indices and `total x W` record
    /// scalars (W = 3 for triangles, else 2), with no padding.  The first `min(k, len)` entries of a sorted row are `traverse_khits`' row.
    pub fn traverse_allhits(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, leaf: c_int, sort: bool) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        if let Some(tm) = tmax {
            assert_eq!(tm.len(), rays.len(), "one tmax per ray");
        }
        let w = if leaf == ffi::BVHGPU_LEAF_TRIANGLE { 3 } else { 2 };
        let r: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let mut hits = core::ptr::null_mut();
        let flags = if sort { 0 } else { ffi::BVHGPU_ALLHITS_LIST_ORDER };
        let mut offsets = vec![0u32; rays.len() + 1];
        let (mut shape, mut vals) = (Vec::new(), Vec::new());
        unsafe {
            check(self.ctx, T::traverse_allhits(self.tree, r.as_ptr(), tmax.map_or(core::ptr::null(), |t| t.as_ptr()), r.len(), ffi::BVHGPU_HOST,
                                                leaf, flags, &mut hits));
            let mut total = 0u64;
            check(self.ctx, ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut()));
            shape.resize(total as usize, 0u32);
            vals.resize(total as usize * w, T::default());
            check(self.ctx, ffi::bvhgpu_hits_fetch_allhits(hits, offsets.as_mut_ptr(), shape.as_mut_ptr(), vals.as_mut_ptr() as *mut c_void, ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        (offsets, shape, vals)
    }

    /// EVERY shape within `max_dist[i]` of point i, as a CSR (`bvhgpu_within_*`): the loop of `FlatBvh::nearest_to` (src/flat_bvh.rs:524-558)
    /// with the moving `best_dist` replaced by the fixed limit `max_dist[i]^2` and every comparison `<=`, so the limit itself is inside; a
    /// negative or NaN limit gives an empty row.  Rows are in a stable ascending sort by distance — equal distances in leaf pre-order — or,
    /// with `sort: false` (`ffi::BVHGPU_WITHIN_LIST_ORDER`), in the order the loop met the shapes.  `triangles`: closest point on the
    /// triangle (needs `set_triangles`) instead of the shape's own AABB.  Returns `(offsets, shape, dist)`: `points.len() + 1` exclusive
    /// prefix sums of the row lengths, `total` shape indices and `total` distances (not squared), with no padding.  `count_only`
    /// (`ffi::BVHGPU_WITHIN_COUNT_ONLY`): the offsets alone, `shape` and `dist` stay empty.
    pub fn within_distance(&self, points: &[[T; 3]], max_dist: &[T], triangles: bool, sort: bool, count_only: bool) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        assert_eq!(max_dist.len(), points.len(), "one max_dist per point");
        let mut hits = core::ptr::null_mut();
        let flags = (if sort { 0 } else { ffi::BVHGPU_WITHIN_LIST_ORDER }) | (if count_only { ffi::BVHGPU_WITHIN_COUNT_ONLY } else { 0 });
        let mut offsets = vec![0u32; points.len() + 1];
        let (mut shape, mut dist) = (Vec::new(), Vec::new());
        unsafe {
            check(self.ctx, T::within(self.tree, points.as_ptr().cast(), max_dist.as_ptr(), points.len(), ffi::BVHGPU_HOST, triangles as c_int,
                                      flags, &mut hits));
            let mut total = 0u64;
            check(self.ctx, ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut()));
            if !count_only {
                shape.resize(total as usize, 0u32);
                dist.resize(total as usize, T::default());
            }
            check(self.ctx, ffi::bvhgpu_hits_fetch_within(hits, offsets.as_mut_ptr(), shape.as_mut_ptr(), dist.as_mut_ptr() as *mut c_void, ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        (offsets, shape, dist)
    }

    /// The shapes whose box passes every plane of a convex region, per region, as a CSR (`bvhgpu_region_*`): `FlatBvh::traverse`
    /// (src/flat_bvh.rs:396-431) with the corner test in place of `intersects_aabb`.  `planes`: `n * m` rows `[nx, ny, nz, d]`, a point `x`
    /// is inside a plane when `n.x + d >= 0`; `m <= ffi::BVHGPU_REGION_MAX_PLANES` planes per region, rows of zeros are padding.  Returns
    /// `(offsets, shape, inside)`: `n + 1` exclusive prefix sums, `total` shape indices in the order of `traverse`, and — with `classify`
    /// (`ffi::BVHGPU_REGION_CLASSIFY`) — a byte per shape, 1 iff its AABB lies wholly inside.  `count_only`: the offsets alone.
    pub fn region_query(&self, planes: &[[T; 4]], m: usize, classify: bool, count_only: bool) -> (Vec<u32>, Vec<u32>, Vec<u8>) {
        let n = if m == 0 { 0 } else { planes.len() / m };
        assert_eq!(n * m, planes.len(), "planes.len() must be a multiple of m");
        let classify = classify && !count_only;
        let flags = (if count_only { ffi::BVHGPU_REGION_COUNT_ONLY } else { 0 }) | (if classify { ffi::BVHGPU_REGION_CLASSIFY } else { 0 });
        let mut hits = core::ptr::null_mut();
        let mut offsets = vec![0u32; n + 1];
        let (mut shape, mut inside) = (Vec::new(), Vec::new());
        unsafe {
            check(self.ctx, T::region(self.tree, planes.as_ptr().cast(), n, m as u32, ffi::BVHGPU_HOST, flags, &mut hits));
            let mut total = 0u64;
            check(self.ctx, ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut()));
            if !count_only { shape.resize(total as usize, 0u32); }
            if classify { inside.resize(total as usize, 0u8); }
            let inside_ptr = if classify { inside.as_mut_ptr() as *mut c_void } else { core::ptr::null_mut() };
            check(self.ctx, ffi::bvhgpu_hits_fetch_region(hits, offsets.as_mut_ptr(), shape.as_mut_ptr(), inside_ptr, ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        (offsets, shape, inside)
    }

    /// The `k` nearest shapes of every point (`bvhgpu_knearest_*`): the loop of `FlatBvh::nearest_to` (src/flat_bvh.rs:524-558) with a list of
    /// at most `k` (distance, shape) pairs in place of `best_element`, every comparison the strict `<`.  Returns row-major `points.len() x k`
    /// arrays: shape indices and distances (not squared), ascending per row (a row that holds a NaN distance need not be sorted), equal
    /// distances in leaf pre-order; slots beyond the number of shapes hold `u32::MAX` and `+inf`.  `triangles`: closest point on the
    /// triangle (needs `set_triangles`) instead of the shape's own AABB.  `1 <= k <= ffi::BVHGPU_KNN_MAX_K`; `k = 1` is `nearest_to` per point.
    pub fn nearest_k(&self, points: &[[T; 3]], k: usize, triangles: bool) -> (Vec<u32>, Vec<T>) {
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_KNN_MAX_K).contains(&k32) { points.len() * k } else { 0 };
        let mut shape = vec![0u32; slots];
        let mut dist = vec![T::default(); slots];
        unsafe {
            check(self.ctx, T::knearest(self.tree, points.as_ptr().cast(), points.len(), ffi::BVHGPU_HOST, triangles as c_int, k32,
                                        shape.as_mut_ptr(), dist.as_mut_ptr()));
        }
        (shape, dist)
    }

    /// The rows of `nearest_k` found nearest child first (`bvhgpu_knearest_tree_*`): `BvhNode::nearest_to_recursive` (src/bvh/bvh_node.rs:327-374,
    /// what `Bvh::nearest_to` calls) over the BvhNode array with the list of at most `k` pairs in place of `best_candidate`.  With `k = 1` and
    /// no `max_dist` a row is what `Bvh::nearest_to` returns.  Equal distances stay in the order this walk meets them, which is not leaf
    /// pre-order: `nearest_k` may order ties differently and pick differently among ties at the k-th distance.  `max_dist`: one limit per
    /// point — nothing farther enters its row (`dist2 <= max_dist[i]^2`); a negative or NaN limit gives a row of padding.
    pub fn nearest_k_tree(&self, points: &[[T; 3]], k: usize, triangles: bool, max_dist: Option<&[T]>) -> (Vec<u32>, Vec<T>) {
        if let Some(m) = max_dist {
            assert_eq!(m.len(), points.len(), "max_dist needs one value per point");
        }
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_KNN_MAX_K).contains(&k32) { points.len() * k } else { 0 };
        let mut shape = vec![0u32; slots];
        let mut dist = vec![T::default(); slots];
        unsafe {
            check(self.ctx, T::knearest_tree(self.tree, points.as_ptr().cast(), points.len(), ffi::BVHGPU_HOST, triangles as c_int, k32,
                                             max_dist.map_or(core::ptr::null(), |m| m.as_ptr()), shape.as_mut_ptr(), dist.as_mut_ptr()));
        }
        (shape, dist)
    }

    /// `nearest_k` against the tree's spheres (`set_spheres`; `bvhgpu_knearest_sphere_*`): the same loop, list and rows with the shape
    /// distance of the solid ball — `len = |p - c|`, `g = len - r`, `d = max(g, 0)^2` with a NaN kept, every operation rounded once; a
    /// point inside or on a ball is at distance 0.  Nodes are pruned by their boxes, so the rows are the `k` nearest spheres in the
    /// geometric sense when every sphere lies inside its shape's box.  `k = 1` is the nearest sphere per point.
    pub fn nearest_k_sphere(&self, points: &[[T; 3]], k: usize) -> (Vec<u32>, Vec<T>) {
        self.nearest_k_sphere_rows(points, k, None, false)
    }

    /// `nearest_k_tree` against the tree's spheres (`bvhgpu_knearest_tree_sphere_*`): the nearest-child-first descent over the BvhNode
    /// array with `nearest_k_sphere`'s distance; `max_dist` and ties as for `nearest_k_tree`.
    pub fn nearest_k_tree_sphere(&self, points: &[[T; 3]], k: usize, max_dist: Option<&[T]>) -> (Vec<u32>, Vec<T>) {
        if let Some(m) = max_dist {
            assert_eq!(m.len(), points.len(), "max_dist needs one value per point");
        }
        self.nearest_k_sphere_rows(points, k, max_dist, true)
    }

    fn nearest_k_sphere_rows(&self, points: &[[T; 3]], k: usize, max_dist: Option<&[T]>, tree_form: bool) -> (Vec<u32>, Vec<T>) {
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_KNN_MAX_K).contains(&k32) { points.len() * k } else { 0 };
        let mut shape = vec![0u32; slots];
        let mut dist = vec![T::default(); slots];
        unsafe {
            let mp = max_dist.map_or(core::ptr::null(), |m| m.as_ptr());
            let (pp, n, sp, dp) = (points.as_ptr(), points.len(), shape.as_mut_ptr(), dist.as_mut_ptr());
            let rc = match (T::DTYPE == ffi::BVHGPU_F32, tree_form) {
                (true, false) => ffi::bvhgpu_knearest_sphere_f32(self.tree, pp.cast(), n, ffi::BVHGPU_HOST, k32, sp, dp.cast()),
                (false, false) => ffi::bvhgpu_knearest_sphere_f64(self.tree, pp.cast(), n, ffi::BVHGPU_HOST, k32, sp, dp.cast()),
                (true, true) => ffi::bvhgpu_knearest_tree_sphere_f32(self.tree, pp.cast(), n, ffi::BVHGPU_HOST, k32, mp.cast(), sp, dp.cast()),
                (false, true) => ffi::bvhgpu_knearest_tree_sphere_f64(self.tree, pp.cast(), n, ffi::BVHGPU_HOST, k32, mp.cast(), sp, dp.cast()),
            };
            check(self.ctx, rc);
        }
        (shape, dist)
    }

    /// `within_distance` against the tree's spheres (`bvhgpu_within_sphere_*`): every sphere within `max_dist[i]` of point i, with
    /// `nearest_k_sphere`'s distance (`d <= max_dist[i]^2`; a NaN distance is never a candidate).  Flags and returns as for `within_distance`.
    pub fn within_distance_sphere(&self, points: &[[T; 3]], max_dist: &[T], sort: bool, count_only: bool) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        assert_eq!(max_dist.len(), points.len(), "one max_dist per point");
        let mut hits = core::ptr::null_mut();
        let flags = (if sort { 0 } else { ffi::BVHGPU_WITHIN_LIST_ORDER }) | (if count_only { ffi::BVHGPU_WITHIN_COUNT_ONLY } else { 0 });
        let mut offsets = vec![0u32; points.len() + 1];
        let (mut shape, mut dist) = (Vec::new(), Vec::new());
        unsafe {
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_within_sphere_f32(self.tree, points.as_ptr().cast(), max_dist.as_ptr().cast(), points.len(), ffi::BVHGPU_HOST, flags, &mut hits)
            } else {
                ffi::bvhgpu_within_sphere_f64(self.tree, points.as_ptr().cast(), max_dist.as_ptr().cast(), points.len(), ffi::BVHGPU_HOST, flags, &mut hits)
            };
            check(self.ctx, rc);
            let mut total = 0u64;
            check(self.ctx, ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut()));
            if !count_only {
                shape.resize(total as usize, 0u32);
                dist.resize(total as usize, T::default());
            }
            check(self.ctx, ffi::bvhgpu_hits_fetch_within(hits, offsets.as_mut_ptr(), shape.as_mut_ptr(), dist.as_mut_ptr() as *mut c_void, ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        (offsets, shape, dist)
    }

    /// Build again from new AABBs into the same device buffers (a frame loop: no allocation in the steady state)
    pub fn rebuild(&mut self, aabbs: &[[T; 6]]) {
        unsafe { check(self.ctx, T::rebuild_flat(self.tree, aabbs.as_ptr().cast(), aabbs.len(), ffi::BVHGPU_HOST)); }
        self.n_shapes = aabbs.len();
        self.flat = self.download_flat();
        self.flat_stale = false;
    }

    /// After `rebuild_async`: wait for the build and refresh the CPU copy the trait's generic queries walk
    pub fn sync_flat(&mut self) {
        self.flat = self.download_flat();
        self.flat_stale = false;
    }

    /// the shapes moved, the topology stays: `Bvh::fix_aabbs_ascending` (src/bvh/optimization.rs:355-391) over the whole tree
    pub fn refit(&mut self, aabbs: &[[T; 6]]) {
        unsafe { check(self.ctx, T::refit(self.tree, aabbs.as_ptr().cast(), aabbs.len(), ffi::BVHGPU_HOST)); }
        self.flat = self.download_flat();
    }

    pub fn raw(&self) -> (*mut ffi::bvhgpu_ctx, *mut ffi::bvhgpu_tree) {
        (self.ctx, self.tree)
    }
}

impl<T: GpuScalar> BoundingHierarchy<T, 3> for GpuBvh<T> {
    fn build<Shape: BHShape<T, 3>>(shapes: &mut [Shape]) -> GpuBvh<T> {
        // (1) the only callback the device cannot make: shape.aabb(), gathered once per shape
        let aabbs: Vec<[T; 6]> = shapes.iter().map(|s| aabb_to_6(&s.aabb())).collect();
        // (2) Bvh::build_par + Bvh::flatten on the GPU the process chose (set_default_device)
        let bh = GpuBvh::from_aabbs(&aabbs, default_device());
        // (3) set_bh_node_index for every shape (src/bvh/bvh_node.rs:102)
        for (s, ni) in shapes.iter_mut().zip(bh.shape_nodes()) {
            s.set_bh_node_index(ni as usize);
        }
        bh
    }

    fn build_with_executor<
        Shape: BHShape<T, 3>,
        Executor: FnMut(BvhNodeBuildArgs<'_, Shape, T, 3>, BvhNodeBuildArgs<'_, Shape, T, 3>),
    >(
        shapes: &mut [Shape],
        _executor: Executor,
    ) -> GpuBvh<T> {
        // the executor only schedules CPU sub-builds and cannot change the result (node placement is arithmetic,
        // src/bvh/bvh_node.rs:138-142): the GPU schedules its own.  `build_par` lands here through the trait's default.
        Self::build(shapes)
    }

    fn traverse<'a, Query: IntersectsAabb<T, 3>, Shape: BHShape<T, 3>>(
        &'a self,
        query: &Query,
        shapes: &'a [Shape],
    ) -> Vec<&'a Shape> {
        // one generic query: the crate's own loop over the downloaded flat array (src/flat_bvh.rs:396-431).  Stable Rust cannot
        // specialise this method on the query type, so it stays on the CPU for every `IntersectsAabb`; BATCHES of the crate's own
        // query types run on the GPU through `traverse_batch` (rays), `traverse_aabbs`, `traverse_points`, `traverse_balls`
        // and `self_overlaps`
        assert!(!self.flat_stale, "rebuild_async: call sync_flat() before a generic query");
        self.flat.traverse(query, shapes)
    }

    fn nearest_to<'a, Shape: BHShape<T, 3> + PointDistance<T, 3>>(
        &'a self,
        query: Point3<T>,
        shapes: &'a [Shape],
    ) -> Option<(&'a Shape, T)> {
        self.flat.nearest_to(query, shapes)
    }

    fn pretty_print(&self) {
        self.flat.pretty_print()
    }
}

impl<T: GpuScalar> Drop for GpuBvh<T> {
    fn drop(&mut self) {
        unsafe {
            ffi::bvhgpu_tree_destroy(self.tree);
            ffi::bvhgpu_destroy(self.ctx);
        }
    }
}

/// Result of an instanced ray query (`GpuInstances::trace`): the `Intersection` in the world ray's parameter, the instance and the shape
/// within that instance's tree; `instance == shape == u32::MAX` and `distance == +inf` when the ray hits nothing
pub struct InstanceHit<T> {
    pub intersection: Intersection<T>,
    pub instance: u32,
    pub shape: u32,
}

/// An instanced scene (`bvhgpu_instances_*`): transformed copies of member trees under a top-level tree over their world boxes.  The
/// member trees are raw handles of ONE context (`GpuBvh::raw`, `upload_flat`), flattened and with triangles set; they are only borrowed
/// and must outlive every call except the drop.  Transforms are row-major 3x4, object -> world.
pub struct GpuInstances<T: GpuScalar> {
    ctx: *mut ffi::bvhgpu_ctx,
    set: *mut ffi::bvhgpu_instances,
    n: usize,
    _t: core::marker::PhantomData<T>,
}

impl<T: GpuScalar> GpuInstances<T> {
    /// # Safety
    /// `ctx` and every handle in `trees` are live handles of this library, and the trees were made on `ctx`.
    pub unsafe fn new(ctx: *mut ffi::bvhgpu_ctx, trees: &[*mut ffi::bvhgpu_tree], tree_of: &[u32], xforms: &[[T; 12]]) -> GpuInstances<T> {
        assert_eq!(tree_of.len(), xforms.len(), "one tree slot and one transform per instance");
        let mut set = core::ptr::null_mut();
        let rc = if T::DTYPE == ffi::BVHGPU_F32 {
            ffi::bvhgpu_instances_create_f32(ctx, trees.as_ptr(), trees.len(), tree_of.as_ptr(), xforms.as_ptr().cast(), xforms.len(), ffi::BVHGPU_HOST, &mut set)
        } else {
            ffi::bvhgpu_instances_create_f64(ctx, trees.as_ptr(), trees.len(), tree_of.as_ptr(), xforms.as_ptr().cast(), xforms.len(), ffi::BVHGPU_HOST, &mut set)
        };
        check(ctx, rc);
        GpuInstances { ctx, set, n: xforms.len(), _t: core::marker::PhantomData }
    }

    /// `new` with a leaf kind, fixed for the set's life: `ffi::BVHGPU_LEAF_BOX` (the shapes' own boxes; the members need neither triangles
    /// nor spheres), `ffi::BVHGPU_LEAF_TRIANGLE` (what `new` makes) or `ffi::BVHGPU_LEAF_SPHERE` (the members need `set_spheres`; an
    /// instance's sphere is the ellipsoid its transform maps it to).  Every ray query of the set answers with that kind's record: two
    /// scalars, `{enter, exit}` / `{distance, exit}`, for BOX and SPHERE.  `trace` and `trace_masked` return them as
    /// `Intersection { distance, u: exit, v: 0 }`; the `vals` of the k-hits and all-hits methods are then 2 scalars per record.
    /// # Safety
    /// as `new`
    pub unsafe fn new_with_leaf(ctx: *mut ffi::bvhgpu_ctx, trees: &[*mut ffi::bvhgpu_tree], tree_of: &[u32], xforms: &[[T; 12]], leaf: c_int) -> GpuInstances<T> {
        assert_eq!(tree_of.len(), xforms.len(), "one tree slot and one transform per instance");
        let mut set = core::ptr::null_mut();
        let rc = if T::DTYPE == ffi::BVHGPU_F32 {
            ffi::bvhgpu_instances_create_leaf_f32(ctx, trees.as_ptr(), trees.len(), tree_of.as_ptr(), xforms.as_ptr().cast(), xforms.len(), ffi::BVHGPU_HOST, leaf, &mut set)
        } else {
            ffi::bvhgpu_instances_create_leaf_f64(ctx, trees.as_ptr(), trees.len(), tree_of.as_ptr(), xforms.as_ptr().cast(), xforms.len(), ffi::BVHGPU_HOST, leaf, &mut set)
        };
        check(ctx, rc);
        GpuInstances { ctx, set, n: xforms.len(), _t: core::marker::PhantomData }
    }

    /// The set's leaf kind (`ffi::BVHGPU_LEAF_*`)
    pub fn leaf(&self) -> c_int {
        let mut leaf: c_int = ffi::BVHGPU_LEAF_TRIANGLE;
        check(self.ctx, unsafe { ffi::bvhgpu_instances_leaf(self.set, &mut leaf) });
        leaf
    }

    // scalars per record of the set's ray queries
    fn width(&self) -> usize {
        if self.leaf() == ffi::BVHGPU_LEAF_TRIANGLE { 3 } else { 2 }
    }

    /// The re-pose and the re-sync: after moving instances, and after any rebuild, refit or `set_triangles` of a member tree
    pub fn update(&mut self, xforms: &[[T; 12]]) {
        assert_eq!(xforms.len(), self.n, "one transform per instance");
        let rc = unsafe {
            if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_update_f32(self.set, xforms.as_ptr().cast(), xforms.len(), ffi::BVHGPU_HOST)
            } else {
                ffi::bvhgpu_instances_update_f64(self.set, xforms.as_ptr().cast(), xforms.len(), ffi::BVHGPU_HOST)
            }
        };
        check(self.ctx, rc);
    }

    /// Per ray the nearest candidate over all instances (`first == false`) or the first one in walk order (`first == true`), among those
    /// with `distance < tmax[j]` (`None`: +inf)
    pub fn trace(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, first: bool) -> Vec<InstanceHit<T>> {
        if let Some(m) = tmax {
            assert_eq!(m.len(), rays.len(), "tmax needs one value per ray");
        }
        let raw: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let n = raw.len();
        let w = self.width();
        let mut vals = vec![T::default(); w * n];
        let mut inst = vec![0u32; n];
        let mut shape = vec![0u32; n];
        let flags: c_uint = if first { ffi::BVHGPU_TRAVERSE_FIRST } else { 0 };
        let rc = unsafe {
            if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_trace_f32(self.set, raw.as_ptr().cast(), tmax.map_or(core::ptr::null(), |m| m.as_ptr().cast()), n, ffi::BVHGPU_HOST,
                                                flags, vals.as_mut_ptr().cast(), inst.as_mut_ptr(), shape.as_mut_ptr())
            } else {
                ffi::bvhgpu_instances_trace_f64(self.set, raw.as_ptr().cast(), tmax.map_or(core::ptr::null(), |m| m.as_ptr().cast()), n, ffi::BVHGPU_HOST,
                                                flags, vals.as_mut_ptr().cast(), inst.as_mut_ptr(), shape.as_mut_ptr())
            }
        };
        check(self.ctx, rc);
        (0..n).map(|j| InstanceHit { intersection: Intersection::new(vals[w * j], vals[w * j + 1], if w == 3 { vals[w * j + 2] } else { T::default() }), instance: inst[j], shape: shape[j] }).collect()
    }

    /// Per region of `m` world-space planes `[nx, ny, nz, d]` the `(instance, shape)` pairs whose box passes, as a CSR
    /// (`bvhgpu_instances_region_*`): the instances whose world box passes, in the top level's order, each walked with the planes
    /// re-expressed in its object frame.  Returns `(offsets, instance, shape, inside)`; `instances_only`
    /// (`ffi::BVHGPU_REGION_INSTANCES_ONLY`): the instances alone, `shape` stays empty; `classify`: a byte per row entry, 1 iff the box
    /// lies wholly inside; `count_only`: the offsets alone.
    pub fn region_query(&self, planes: &[[T; 4]], m: usize, classify: bool, count_only: bool, instances_only: bool) -> (Vec<u32>, Vec<u32>, Vec<u32>, Vec<u8>) {
        let n = if m == 0 { 0 } else { planes.len() / m };
        assert_eq!(n * m, planes.len(), "planes.len() must be a multiple of m");
        let classify = classify && !count_only;
        let flags = (if count_only { ffi::BVHGPU_REGION_COUNT_ONLY } else { 0 }) | (if classify { ffi::BVHGPU_REGION_CLASSIFY } else { 0 })
            | (if instances_only { ffi::BVHGPU_REGION_INSTANCES_ONLY } else { 0 });
        let mut hits = core::ptr::null_mut();
        let mut offsets = vec![0u32; n + 1];
        let (mut instance, mut shape, mut inside) = (Vec::new(), Vec::new(), Vec::new());
        unsafe {
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_region_f32(self.set, planes.as_ptr().cast(), n, m as u32, ffi::BVHGPU_HOST, flags, &mut hits)
            } else {
                ffi::bvhgpu_instances_region_f64(self.set, planes.as_ptr().cast(), n, m as u32, ffi::BVHGPU_HOST, flags, &mut hits)
            };
            check(self.ctx, rc);
            let mut total = 0u64;
            check(self.ctx, ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut()));
            let rows = if count_only { 0 } else { total as usize };
            instance.resize(rows, 0u32);
            if !instances_only { shape.resize(rows, 0u32); }
            if classify { inside.resize(rows, 0u8); }
            let shape_ptr = if instances_only { core::ptr::null_mut() } else { shape.as_mut_ptr() };
            let inside_ptr = if classify { inside.as_mut_ptr() as *mut c_void } else { core::ptr::null_mut() };
            check(self.ctx, ffi::bvhgpu_hits_fetch_instances_region(hits, offsets.as_mut_ptr(), instance.as_mut_ptr(), shape_ptr, inside_ptr, ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        (offsets, instance, shape, inside)
    }

    /// Per ray EVERY `(instance, shape)` whose triangle it hits with `distance < tmax[j]` (`None`: +inf), as a CSR
    /// (`bvhgpu_instances_allhits_*`).  `sort`: each row ascending by distance, ties in walk order — its head is `trace(.., false)`'s
    /// answer; otherwise walk order — its head is `trace(.., true)`'s.  Returns `(offsets, instance, shape, vals)`, `vals` holding
    /// `{distance, u, v}` per entry; `count_only`: the offsets alone.
    pub fn allhits(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, sort: bool, count_only: bool) -> (Vec<u32>, Vec<u32>, Vec<u32>, Vec<T>) {
        if let Some(m) = tmax {
            assert_eq!(m.len(), rays.len(), "tmax needs one value per ray");
        }
        let raw: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let n = raw.len();
        let flags: c_uint = (if sort { 0 } else { ffi::BVHGPU_INSTANCES_ALLHITS_LIST_ORDER })
            | (if count_only { ffi::BVHGPU_INSTANCES_ALLHITS_COUNT_ONLY } else { 0 });
        let mut hits = core::ptr::null_mut();
        let mut offsets = vec![0u32; n + 1];
        let (mut instance, mut shape, mut vals) = (Vec::new(), Vec::new(), Vec::new());
        unsafe {
            let tp = tmax.map_or(core::ptr::null(), |m| m.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_allhits_f32(self.set, raw.as_ptr().cast(), tp.cast(), n, ffi::BVHGPU_HOST, flags, &mut hits)
            } else {
                ffi::bvhgpu_instances_allhits_f64(self.set, raw.as_ptr().cast(), tp.cast(), n, ffi::BVHGPU_HOST, flags, &mut hits)
            };
            check(self.ctx, rc);   // (a refused batch made no result object)
            let mut total = 0u64;
            let mut rc = ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut());
            if rc == ffi::BVHGPU_OK {
                let rows = if count_only { 0 } else { total as usize };
                instance.resize(rows, 0u32);
                shape.resize(rows, 0u32);
                vals.resize(self.width() * rows, T::default());
                let (ip, sp, vp) = if count_only {
                    (core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut())
                } else {
                    (instance.as_mut_ptr(), shape.as_mut_ptr(), vals.as_mut_ptr() as *mut c_void)
                };
                rc = ffi::bvhgpu_hits_fetch_instances_allhits(hits, offsets.as_mut_ptr(), ip, sp, vp, ffi::BVHGPU_HOST);
            }
            ffi::bvhgpu_hits_destroy(hits);   // before the check, which panics on a failure
            check(self.ctx, rc);
        }
        (offsets, instance, shape, vals)
    }

    /// Per point EVERY `(instance, shape)` whose world-space triangle lies within `max_dist[j]` of it (`<=`; a negative or NaN limit gives
    /// an empty row), as a CSR (`bvhgpu_instances_within_*`).  The distance is the true world distance to the transformed triangle,
    /// whatever the transform.  `sort`: each row ascending by distance, ties in walk order; otherwise walk order.  Returns
    /// `(offsets, instance, shape, dist)`, distances not squared; `count_only`: the offsets alone.
    pub fn within_distance(&self, points: &[[T; 3]], max_dist: &[T], sort: bool, count_only: bool) -> (Vec<u32>, Vec<u32>, Vec<u32>, Vec<T>) {
        assert_eq!(max_dist.len(), points.len(), "one max_dist per point");
        let n = points.len();
        let flags: c_uint = (if sort { 0 } else { ffi::BVHGPU_INSTANCES_WITHIN_LIST_ORDER })
            | (if count_only { ffi::BVHGPU_INSTANCES_WITHIN_COUNT_ONLY } else { 0 });
        let mut hits = core::ptr::null_mut();
        let mut offsets = vec![0u32; n + 1];
        let (mut instance, mut shape, mut dist) = (Vec::new(), Vec::new(), Vec::new());
        unsafe {
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_within_f32(self.set, points.as_ptr().cast(), max_dist.as_ptr().cast(), n, ffi::BVHGPU_HOST, flags, &mut hits)
            } else {
                ffi::bvhgpu_instances_within_f64(self.set, points.as_ptr().cast(), max_dist.as_ptr().cast(), n, ffi::BVHGPU_HOST, flags, &mut hits)
            };
            check(self.ctx, rc);   // (a refused batch made no result object)
            let mut total = 0u64;
            let mut rc = ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut());
            if rc == ffi::BVHGPU_OK {
                let rows = if count_only { 0 } else { total as usize };
                instance.resize(rows, 0u32);
                shape.resize(rows, 0u32);
                dist.resize(rows, T::default());
                let (ip, sp, dp) = if count_only {
                    (core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut())
                } else {
                    (instance.as_mut_ptr(), shape.as_mut_ptr(), dist.as_mut_ptr() as *mut c_void)
                };
                rc = ffi::bvhgpu_hits_fetch_instances_within(hits, offsets.as_mut_ptr(), ip, sp, dp, ffi::BVHGPU_HOST);
            }
            ffi::bvhgpu_hits_destroy(hits);   // before the check, which panics on a failure
            check(self.ctx, rc);
        }
        (offsets, instance, shape, dist)
    }

    /// Per point the `k` `(instance, shape)` pairs whose world-space triangles are nearest (`bvhgpu_instances_knearest_*`): `nearest_k`'s
    /// list and strict `<` over the two-level walk, the distance the true world distance to the transformed triangle.  Returns row-major
    /// `points.len() x k` arrays `(instance, shape, dist)`, distances not squared, ascending per row (a row that holds a NaN distance need
    /// not be sorted); equal distances stay in walk order (instances in the top level's order, shapes in the member's order) and a tie
    /// at the k-th distance keeps the pairs met first; slots beyond the number of pairs hold `u32::MAX`, `u32::MAX` and `+inf`.
    /// `1 <= k <= ffi::BVHGPU_INSTANCES_KNN_MAX_K`; `k = 1` is `nearest_to` over the instanced scene.
    pub fn knearest(&self, points: &[[T; 3]], k: usize) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_INSTANCES_KNN_MAX_K).contains(&k32) { points.len() * k } else { 0 };
        let (mut instance, mut shape, mut dist) = (vec![0u32; slots], vec![0u32; slots], vec![T::default(); slots]);
        unsafe {
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_knearest_f32(self.set, points.as_ptr().cast(), points.len(), ffi::BVHGPU_HOST, k32, instance.as_mut_ptr(),
                                                   shape.as_mut_ptr(), dist.as_mut_ptr().cast())
            } else {
                ffi::bvhgpu_instances_knearest_f64(self.set, points.as_ptr().cast(), points.len(), ffi::BVHGPU_HOST, k32, instance.as_mut_ptr(),
                                                   shape.as_mut_ptr(), dist.as_mut_ptr().cast())
            };
            check(self.ctx, rc);
        }
        (instance, shape, dist)
    }

    /// The rows of `knearest` found nearest child first on both levels (`bvhgpu_instances_knearest_tree_*`), with an optional search radius
    /// per point: nothing farther than `max_dist[j]` enters row `j` (`d <= max_dist[j]^2`); a negative or NaN limit gives a row of padding.
    /// Equal distances stay in the order this walk meets them, which is not `knearest`'s: the two may name different pairs at tied
    /// distances, their distances agree.  Every member tree must have been built here.  Returns and `k` as for `knearest`.
    pub fn knearest_tree(&self, points: &[[T; 3]], k: usize, max_dist: Option<&[T]>) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        if let Some(m) = max_dist {
            assert_eq!(m.len(), points.len(), "max_dist needs one value per point");
        }
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_INSTANCES_KNN_MAX_K).contains(&k32) { points.len() * k } else { 0 };
        let (mut instance, mut shape, mut dist) = (vec![0u32; slots], vec![0u32; slots], vec![T::default(); slots]);
        unsafe {
            let mp = max_dist.map_or(core::ptr::null(), |m| m.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_knearest_tree_f32(self.set, points.as_ptr().cast(), points.len(), ffi::BVHGPU_HOST, k32, mp.cast(),
                                                        instance.as_mut_ptr(), shape.as_mut_ptr(), dist.as_mut_ptr().cast())
            } else {
                ffi::bvhgpu_instances_knearest_tree_f64(self.set, points.as_ptr().cast(), points.len(), ffi::BVHGPU_HOST, k32, mp.cast(),
                                                        instance.as_mut_ptr(), shape.as_mut_ptr(), dist.as_mut_ptr().cast())
            };
            check(self.ctx, rc);
        }
        (instance, shape, dist)
    }

    /// Per ray the `k` nearest `(instance, shape)` hits with `distance < tmax[j]` (`None`: `+inf`), ascending (`bvhgpu_instances_khits_*`):
    /// the head of `allhits`' sorted row, byte for byte, without the CSR.  Returns row-major `rays.len() x k` arrays `(instance, shape)` and
    /// `rays.len() x k x 3` `vals` = `{distance, u, v}`; equal distances stay in walk order (instances in the top level's order, shapes in
    /// the member's order) and a tie at the k-th distance keeps the pairs met first; slots beyond the number of hits hold `u32::MAX`,
    /// `u32::MAX` and `{+inf, 0, 0}`.  `1 <= k <= ffi::BVHGPU_INSTANCES_KHITS_MAX_K`; `k = 1` is `closest_hits`.
    pub fn khits(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, k: usize) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        if let Some(m) = tmax {
            assert_eq!(m.len(), rays.len(), "tmax needs one value per ray");
        }
        let raw: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let n = raw.len();
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_INSTANCES_KHITS_MAX_K).contains(&k32) { n * k } else { 0 };
        let (mut instance, mut shape, mut vals) = (vec![0u32; slots], vec![0u32; slots], vec![T::default(); self.width() * slots]);
        unsafe {
            let tp = tmax.map_or(core::ptr::null(), |m| m.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_khits_f32(self.set, raw.as_ptr().cast(), tp.cast(), n, ffi::BVHGPU_HOST, k32, instance.as_mut_ptr(),
                                                shape.as_mut_ptr(), vals.as_mut_ptr().cast())
            } else {
                ffi::bvhgpu_instances_khits_f64(self.set, raw.as_ptr().cast(), tp.cast(), n, ffi::BVHGPU_HOST, k32, instance.as_mut_ptr(),
                                                shape.as_mut_ptr(), vals.as_mut_ptr().cast())
            };
            check(self.ctx, rc);
        }
        (instance, shape, vals)
    }

    /// One 32-bit visibility mask per instance (`bvhgpu_instances_set_masks`), or `None` for all ones again — what a new set has.  Instance
    /// `i` is visible to ray `j` of a `*_masked` call iff `masks[i] & ray_mask[j] != 0`.  No part of the pose: `update` keeps the masks,
    /// setting them commits nothing.  `trace`, `khits`, `allhits` and the point and region queries ignore them.
    pub fn set_masks(&mut self, masks: Option<&[u32]>) {
        if let Some(m) = masks {
            assert_eq!(m.len(), self.n, "one mask per instance");
        }
        let rc = unsafe { ffi::bvhgpu_instances_set_masks(self.set, masks.map_or(core::ptr::null(), |m| m.as_ptr()), self.n, ffi::BVHGPU_HOST) };
        check(self.ctx, rc);
    }

    /// `trace` over the instances visible to each ray (`bvhgpu_instances_trace_masked_*`); `ray_mask`: one mask per ray, `None`: all ones
    pub fn trace_masked(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, ray_mask: Option<&[u32]>, first: bool) -> Vec<InstanceHit<T>> {
        if let Some(m) = tmax {
            assert_eq!(m.len(), rays.len(), "tmax needs one value per ray");
        }
        if let Some(m) = ray_mask {
            assert_eq!(m.len(), rays.len(), "ray_mask needs one value per ray");
        }
        let raw: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let n = raw.len();
        let w = self.width();
        let mut vals = vec![T::default(); w * n];
        let mut inst = vec![0u32; n];
        let mut shape = vec![0u32; n];
        let flags: c_uint = if first { ffi::BVHGPU_TRAVERSE_FIRST } else { 0 };
        let mp = ray_mask.map_or(core::ptr::null(), |m| m.as_ptr());
        let rc = unsafe {
            if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_trace_masked_f32(self.set, raw.as_ptr().cast(), tmax.map_or(core::ptr::null(), |m| m.as_ptr().cast()), mp, n,
                                                       ffi::BVHGPU_HOST, flags, vals.as_mut_ptr().cast(), inst.as_mut_ptr(), shape.as_mut_ptr())
            } else {
                ffi::bvhgpu_instances_trace_masked_f64(self.set, raw.as_ptr().cast(), tmax.map_or(core::ptr::null(), |m| m.as_ptr().cast()), mp, n,
                                                       ffi::BVHGPU_HOST, flags, vals.as_mut_ptr().cast(), inst.as_mut_ptr(), shape.as_mut_ptr())
            }
        };
        check(self.ctx, rc);
        (0..n).map(|j| InstanceHit { intersection: Intersection::new(vals[w * j], vals[w * j + 1], if w == 3 { vals[w * j + 2] } else { T::default() }), instance: inst[j], shape: shape[j] }).collect()
    }

    /// `khits` over the instances visible to each ray (`bvhgpu_instances_khits_masked_*`)
    pub fn khits_masked(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, ray_mask: Option<&[u32]>, k: usize) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        if let Some(m) = tmax {
            assert_eq!(m.len(), rays.len(), "tmax needs one value per ray");
        }
        if let Some(m) = ray_mask {
            assert_eq!(m.len(), rays.len(), "ray_mask needs one value per ray");
        }
        let raw: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let n = raw.len();
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_INSTANCES_KHITS_MAX_K).contains(&k32) { n * k } else { 0 };
        let (mut instance, mut shape, mut vals) = (vec![0u32; slots], vec![0u32; slots], vec![T::default(); self.width() * slots]);
        unsafe {
            let tp = tmax.map_or(core::ptr::null(), |m| m.as_ptr());
            let mp = ray_mask.map_or(core::ptr::null(), |m| m.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_khits_masked_f32(self.set, raw.as_ptr().cast(), tp.cast(), mp, n, ffi::BVHGPU_HOST, k32, instance.as_mut_ptr(),
                                                       shape.as_mut_ptr(), vals.as_mut_ptr().cast())
            } else {
                ffi::bvhgpu_instances_khits_masked_f64(self.set, raw.as_ptr().cast(), tp.cast(), mp, n, ffi::BVHGPU_HOST, k32, instance.as_mut_ptr(),
                                                       shape.as_mut_ptr(), vals.as_mut_ptr().cast())
            };
            check(self.ctx, rc);
        }
        (instance, shape, vals)
    }

    /// `allhits` over the instances visible to each ray (`bvhgpu_instances_allhits_masked_*`); the result is read like `allhits`' own
    pub fn allhits_masked(&self, rays: &[Ray<T, 3>], tmax: Option<&[T]>, ray_mask: Option<&[u32]>, sort: bool, count_only: bool) -> (Vec<u32>, Vec<u32>, Vec<u32>, Vec<T>) {
        if let Some(m) = tmax {
            assert_eq!(m.len(), rays.len(), "tmax needs one value per ray");
        }
        if let Some(m) = ray_mask {
            assert_eq!(m.len(), rays.len(), "ray_mask needs one value per ray");
        }
        let raw: Vec<T::RayC> = rays.iter().map(T::ray_to_ffi).collect();
        let n = raw.len();
        let flags: c_uint = (if sort { 0 } else { ffi::BVHGPU_INSTANCES_ALLHITS_LIST_ORDER })
            | (if count_only { ffi::BVHGPU_INSTANCES_ALLHITS_COUNT_ONLY } else { 0 });
        let mut hits = core::ptr::null_mut();
        let mut offsets = vec![0u32; n + 1];
        let (mut instance, mut shape, mut vals) = (Vec::new(), Vec::new(), Vec::new());
        unsafe {
            let tp = tmax.map_or(core::ptr::null(), |m| m.as_ptr());
            let mp = ray_mask.map_or(core::ptr::null(), |m| m.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_allhits_masked_f32(self.set, raw.as_ptr().cast(), tp.cast(), mp, n, ffi::BVHGPU_HOST, flags, &mut hits)
            } else {
                ffi::bvhgpu_instances_allhits_masked_f64(self.set, raw.as_ptr().cast(), tp.cast(), mp, n, ffi::BVHGPU_HOST, flags, &mut hits)
            };
            check(self.ctx, rc);   // (a refused batch made no result object)
            let mut total = 0u64;
            let mut rc = ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut());
            if rc == ffi::BVHGPU_OK {
                let rows = if count_only { 0 } else { total as usize };
                instance.resize(rows, 0u32);
                shape.resize(rows, 0u32);
                vals.resize(self.width() * rows, T::default());
                let (ip, sp, vp) = if count_only {
                    (core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut())
                } else {
                    (instance.as_mut_ptr(), shape.as_mut_ptr(), vals.as_mut_ptr() as *mut c_void)
                };
                rc = ffi::bvhgpu_hits_fetch_instances_allhits(hits, offsets.as_mut_ptr(), ip, sp, vp, ffi::BVHGPU_HOST);
            }
            ffi::bvhgpu_hits_destroy(hits);   // before the check, which panics on a failure
            check(self.ctx, rc);
        }
        (offsets, instance, shape, vals)
    }

    /// `within_distance` over the instances visible to each point (`bvhgpu_instances_within_masked_*`): instance `i` is visible to point `j`
    /// iff `masks[i] & point_mask[j] != 0` (`None`: all ones).  Row `j` is `within_distance`'s row without the hidden instances' pairs.
    pub fn within_masked(&self, points: &[[T; 3]], max_dist: &[T], point_mask: Option<&[u32]>, sort: bool, count_only: bool) -> (Vec<u32>, Vec<u32>, Vec<u32>, Vec<T>) {
        assert_eq!(max_dist.len(), points.len(), "one max_dist per point");
        if let Some(m) = point_mask {
            assert_eq!(m.len(), points.len(), "point_mask needs one value per point");
        }
        let n = points.len();
        let flags: c_uint = (if sort { 0 } else { ffi::BVHGPU_INSTANCES_WITHIN_LIST_ORDER })
            | (if count_only { ffi::BVHGPU_INSTANCES_WITHIN_COUNT_ONLY } else { 0 });
        let mut hits = core::ptr::null_mut();
        let mut offsets = vec![0u32; n + 1];
        let (mut instance, mut shape, mut dist) = (Vec::new(), Vec::new(), Vec::new());
        unsafe {
            let mp = point_mask.map_or(core::ptr::null(), |m| m.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_within_masked_f32(self.set, points.as_ptr().cast(), max_dist.as_ptr().cast(), mp, n, ffi::BVHGPU_HOST, flags, &mut hits)
            } else {
                ffi::bvhgpu_instances_within_masked_f64(self.set, points.as_ptr().cast(), max_dist.as_ptr().cast(), mp, n, ffi::BVHGPU_HOST, flags, &mut hits)
            };
            check(self.ctx, rc);   // (a refused batch made no result object)
            let mut total = 0u64;
            let mut rc = ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut());
            if rc == ffi::BVHGPU_OK {
                let rows = if count_only { 0 } else { total as usize };
                instance.resize(rows, 0u32);
                shape.resize(rows, 0u32);
                dist.resize(rows, T::default());
                let (ip, sp, dp) = if count_only {
                    (core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut())
                } else {
                    (instance.as_mut_ptr(), shape.as_mut_ptr(), dist.as_mut_ptr() as *mut c_void)
                };
                rc = ffi::bvhgpu_hits_fetch_instances_within(hits, offsets.as_mut_ptr(), ip, sp, dp, ffi::BVHGPU_HOST);
            }
            ffi::bvhgpu_hits_destroy(hits);   // before the check, which panics on a failure
            check(self.ctx, rc);
        }
        (offsets, instance, shape, dist)
    }

    /// `knearest` over the instances visible to each point (`bvhgpu_instances_knearest_masked_*`): the first `k` of the stable ascending sort
    /// of all VISIBLE pairs — a hidden pair takes no slot and moves no bound, which a filter of `knearest`'s row cannot give.
    pub fn knearest_masked(&self, points: &[[T; 3]], point_mask: Option<&[u32]>, k: usize) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        if let Some(m) = point_mask {
            assert_eq!(m.len(), points.len(), "point_mask needs one value per point");
        }
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_INSTANCES_KNN_MAX_K).contains(&k32) { points.len() * k } else { 0 };
        let (mut instance, mut shape, mut dist) = (vec![0u32; slots], vec![0u32; slots], vec![T::default(); slots]);
        unsafe {
            let mp = point_mask.map_or(core::ptr::null(), |m| m.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_knearest_masked_f32(self.set, points.as_ptr().cast(), mp, points.len(), ffi::BVHGPU_HOST, k32, instance.as_mut_ptr(),
                                                          shape.as_mut_ptr(), dist.as_mut_ptr().cast())
            } else {
                ffi::bvhgpu_instances_knearest_masked_f64(self.set, points.as_ptr().cast(), mp, points.len(), ffi::BVHGPU_HOST, k32, instance.as_mut_ptr(),
                                                          shape.as_mut_ptr(), dist.as_mut_ptr().cast())
            };
            check(self.ctx, rc);
        }
        (instance, shape, dist)
    }

    /// `knearest_tree` over the instances visible to each point (`bvhgpu_instances_knearest_tree_masked_*`): the same descent over the same
    /// top level, a hidden instance's leaf contributing nothing; ties stay in that walk's order.
    pub fn knearest_tree_masked(&self, points: &[[T; 3]], point_mask: Option<&[u32]>, k: usize, max_dist: Option<&[T]>) -> (Vec<u32>, Vec<u32>, Vec<T>) {
        if let Some(m) = max_dist {
            assert_eq!(m.len(), points.len(), "max_dist needs one value per point");
        }
        if let Some(m) = point_mask {
            assert_eq!(m.len(), points.len(), "point_mask needs one value per point");
        }
        let k32 = u32::try_from(k).unwrap_or(u32::MAX);   // (out of range: the engine answers BVHGPU_INVALID_ARG and `check` panics with its message)
        let slots = if (1..=ffi::BVHGPU_INSTANCES_KNN_MAX_K).contains(&k32) { points.len() * k } else { 0 };
        let (mut instance, mut shape, mut dist) = (vec![0u32; slots], vec![0u32; slots], vec![T::default(); slots]);
        unsafe {
            let dp = max_dist.map_or(core::ptr::null(), |m| m.as_ptr());
            let mp = point_mask.map_or(core::ptr::null(), |m| m.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_knearest_tree_masked_f32(self.set, points.as_ptr().cast(), mp, points.len(), ffi::BVHGPU_HOST, k32, dp.cast(),
                                                               instance.as_mut_ptr(), shape.as_mut_ptr(), dist.as_mut_ptr().cast())
            } else {
                ffi::bvhgpu_instances_knearest_tree_masked_f64(self.set, points.as_ptr().cast(), mp, points.len(), ffi::BVHGPU_HOST, k32, dp.cast(),
                                                               instance.as_mut_ptr(), shape.as_mut_ptr(), dist.as_mut_ptr().cast())
            };
            check(self.ctx, rc);
        }
        (instance, shape, dist)
    }

    /// `region_query` over the instances visible to each region (`bvhgpu_instances_region_masked_*`): a camera's culling mask against the
    /// instances' layers.  `region_mask`: one mask per region, `None`: all ones; everything else as for `region_query`.
    pub fn region_masked(&self, planes: &[[T; 4]], m: usize, region_mask: Option<&[u32]>, classify: bool, count_only: bool, instances_only: bool)
                         -> (Vec<u32>, Vec<u32>, Vec<u32>, Vec<u8>) {
        let n = if m == 0 { 0 } else { planes.len() / m };
        assert_eq!(n * m, planes.len(), "planes.len() must be a multiple of m");
        if let Some(r) = region_mask {
            assert_eq!(r.len(), n, "region_mask needs one value per region");
        }
        let classify = classify && !count_only;
        let flags = (if count_only { ffi::BVHGPU_REGION_COUNT_ONLY } else { 0 }) | (if classify { ffi::BVHGPU_REGION_CLASSIFY } else { 0 })
            | (if instances_only { ffi::BVHGPU_REGION_INSTANCES_ONLY } else { 0 });
        let mut hits = core::ptr::null_mut();
        let mut offsets = vec![0u32; n + 1];
        let (mut instance, mut shape, mut inside) = (Vec::new(), Vec::new(), Vec::new());
        unsafe {
            let mp = region_mask.map_or(core::ptr::null(), |r| r.as_ptr());
            let rc = if T::DTYPE == ffi::BVHGPU_F32 {
                ffi::bvhgpu_instances_region_masked_f32(self.set, planes.as_ptr().cast(), mp, n, m as u32, ffi::BVHGPU_HOST, flags, &mut hits)
            } else {
                ffi::bvhgpu_instances_region_masked_f64(self.set, planes.as_ptr().cast(), mp, n, m as u32, ffi::BVHGPU_HOST, flags, &mut hits)
            };
            check(self.ctx, rc);
            let mut total = 0u64;
            check(self.ctx, ffi::bvhgpu_hits_info(hits, core::ptr::null_mut(), &mut total, core::ptr::null_mut()));
            let rows = if count_only { 0 } else { total as usize };
            instance.resize(rows, 0u32);
            if !instances_only { shape.resize(rows, 0u32); }
            if classify { inside.resize(rows, 0u8); }
            let shape_ptr = if instances_only { core::ptr::null_mut() } else { shape.as_mut_ptr() };
            let inside_ptr = if classify { inside.as_mut_ptr() as *mut c_void } else { core::ptr::null_mut() };
            check(self.ctx, ffi::bvhgpu_hits_fetch_instances_region(hits, offsets.as_mut_ptr(), instance.as_mut_ptr(), shape_ptr, inside_ptr, ffi::BVHGPU_HOST));
            ffi::bvhgpu_hits_destroy(hits);
        }
        (offsets, instance, shape, inside)
    }
}

impl<T: GpuScalar> Drop for GpuInstances<T> {
    fn drop(&mut self) {
        unsafe { ffi::bvhgpu_instances_destroy(self.set) };   // (never looks at a member tree)
    }
}

/// Traverse a crate-built `Bvh` on the GPU: `Bvh::flatten_custom` (src/flat_bvh.rs:240-251) lets the caller choose the node
/// type, so the `#[repr(C)]` layout of the C ABI needs no change to the crate.
pub fn upload_flat<T: GpuScalar>(bvh: &Bvh<T, 3>, shape_aabbs: &[[T; 6]], device: i32) -> (*mut ffi::bvhgpu_ctx, *mut ffi::bvhgpu_tree) {
    let flat: Vec<T::Flat> = bvh.flatten_custom(&|aabb: &Aabb<T, 3>, entry, exit, shape| T::flat_from_parts(aabb, entry, exit, shape));
    let mut ctx = core::ptr::null_mut();
    let mut tree = core::ptr::null_mut();
    unsafe {
        check(ctx, ffi::bvhgpu_create(device, core::ptr::null_mut(), &mut ctx));
        check(ctx, T::tree_from_flat(ctx, flat.as_ptr(), flat.len(), shape_aabbs.as_ptr().cast(), shape_aabbs.len(), &mut tree));
    }
    (ctx, tree)
}

/// `Ray::new` (src/ray/ray_impl.rs:70-80) — re-exported so that callers build rays the crate's way
pub fn ray<T: GpuScalar>(origin: [T; 3], direction: [T; 3]) -> Ray<T, 3> {
    Ray::new(Point3::from(origin), Vector3::from(direction))
}

/*
 * bvh_mi355x.h — C ABI of libbvh_mi355x.so: the MI355X (gfx950 / CDNA4) engine for the hot path
 * of the Rust crate `bvh` 0.12.0 (svenstaro/bvh): SAH build → flatten → batched ray traversal.
 *
 * The reference has no FFI of its own (pure Rust); its extension points for this path are the
 * `BoundingHierarchy` trait (src/bounding_hierarchy.rs:89-336), `Bvh::flatten_custom`
 * (src/flat_bvh.rs:240-251) and `build_with_executor` (src/bvh/bvh_impl.rs:53-56).  Each entry
 * point below names the reference interface it replaces (paths relative to the crate root).  The
 * Rust-side binding a maintainer would add (a `GpuBvh` type that implements `BoundingHierarchy`
 * over these symbols) is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; every function returns a bvhgpu_status (0 = OK) and never throws or
 *    aborts across the boundary; bvhgpu_last_error(ctx) gives the text of the last failure.
 *  - "mem" arguments say where a caller buffer lives: BVHGPU_HOST (pageable or pinned host
 *    memory) or BVHGPU_DEVICE (HBM of the ctx's GPU, e.g. a torch tensor's data_ptr()).
 *  - all work is enqueued on the ctx's HIP stream; host-visible results are complete when the
 *    call returns (the call synchronises the stream), device-side results are ordered on the stream.
 *  - a ctx is not internally locked: one ctx per host thread.  Trees are immutable after
 *    build/flatten and may be traversed from several ctxs of the same device concurrently.
 *  - Semantics are bit-exact with the reference for indices/topology: NUM_BUCKETS
 *    = 6 (src/bvh/bucket.rs:5), pre-order node placement (src/bvh/bvh_node.rs:138-142), stable
 *    bucket-major index rewrite (:250-272), strict-< first-wins SAH argmin (:239), surface_area =
 *    2*dot(size,size) (src/aabb/aabb_impl.rs:551-554), NaN-in-slab = miss
 *    (src/ray/intersect_default.rs:22-28).
 *  - Input contract of the builders: the reference panics on a NaN (or infinite) centroid — `to_usize().unwrap()`,
 *    src/bvh/bvh_node.rs:214-217.  bvhgpu_build_* / rebuild_* detect NaN / ±inf in the shape AABBs (and finite boxes whose
 *    centroid extent overflows) on the device and return BVHGPU_INVALID_ARG without building anything; a single shape
 *    is never bucketed and is accepted as in the reference.
 */
#ifndef BVH_MI355X_H
#define BVH_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BVHGPU_ABI_VERSION 7 /* 7: bvhgpu_host_alloc/free/register/unregister, bvhgpu_traverse_host_*, bvhgpu_build_traverse_host_*, bvhgpu_traverse_host_indices, bvhgpu_query_f32/_f64 + BVHGPU_QUERY_AABB/_POINT/_BALL, bvhgpu_traverse_any_f32/_f64 + bvhgpu_hits_fetch_any, bvhgpu_traverse_box_f32/_f64 + bvhgpu_hits_fetch_box + BVHGPU_TRAVERSE_FIRST, bvhgpu_tree_set_spheres_f32/_f64 + bvhgpu_traverse_sphere_f32/_f64 + bvhgpu_hits_fetch_sphere, bvhgpu_knearest_f32/_f64 + BVHGPU_KNN_MAX_K, bvhgpu_within_f32/_f64 + bvhgpu_hits_fetch_within + BVHGPU_WITHIN_LIST_ORDER / _COUNT_ONLY (symbols only: the ABI stays 7), BVHGPU_TUNE_COUNT 23 (slots 17 = HOST_CHUNKS, 18 = WIDE_MIN_RAYS_PER_WG, 19 = HOST_ZERO_COPY, 20 = BUILD_LEVEL_TILE, 21 = FLATTEN_INLINE, 22 = QUERY_VARIANT).  6: BVHGPU_TUNE_COUNT 17 (slots 15 = FLATTEN_LAZY, 16 = BUILD_LEVEL_PERSIST), bvhgpu_hits_walk_kernel.  5: bvhgpu_rccl_info.  4: BVHGPU_TUNE_COUNT 15 (slot 14 = WIDE_F64_GUIDE), bvhgpu_hits_walk_info.  3: BVHGPU_REBROADCAST, broadcast status header, scene blob BVH6 (exact_only), BVHGPU_TUNE_COUNT 14 (slots 11 = WIDE_EARLY_ITEMS, 12 = WIDE_STAGE_SHIFT, 13 = WIDE_REC8), BVHGPU_TRAVERSE_RAYS_READY, bvhgpu_device_alloc/free/copy */
#define BVHGPU_NONE 0xFFFFFFFFu /* u32::MAX marker (flat_bvh.rs:51-53, :124, :137) */

typedef enum {
    BVHGPU_OK = 0,
    BVHGPU_INVALID_ARG = 1,
    BVHGPU_HIP_ERROR = 2,
    BVHGPU_OOM = 3,
    BVHGPU_OVERFLOW = 4,   /* > (2^32-2)/3 shapes (flat_bvh.rs:136 would truncate silently) or > 2^32-1 hits */
    BVHGPU_NO_DEVICE = 5,
    BVHGPU_DTYPE_MISMATCH = 6,
    BVHGPU_NOT_FLATTENED = 7,
    BVHGPU_RCCL_ERROR = 8, /* an RCCL call of the multi-GPU broadcast failed (bvhgpu_last_error has ncclGetErrorString), or librccl
                              could not be loaded (it is dlopen'ed on first use: single-GPU consumers do not need it) */
    BVHGPU_REBROADCAST = 9 /* returned by a wait (bvhgpu_tree_wait / bvhgpu_hits_wait / any call that inspects the tree) on EVERY rank
                              when bvhgpu_bcast_known sent a tree whose asynchronous build then turned out to need the slow path
                              (unbalanced tree on a first build): the root's tree and results are complete, the peers received
                              nothing usable — every rank calls bvhgpu_bcast_known again */
} bvhgpu_status;

typedef enum { BVHGPU_F32 = 0, BVHGPU_F64 = 1 } bvhgpu_dtype;
typedef enum { BVHGPU_HOST = 0, BVHGPU_DEVICE = 1 } bvhgpu_mem;

/* traversal flags */
#define BVHGPU_TRAVERSE_T_SLICE 1u /* also return (tmin,tmax) per hit: Ray::intersection_slice_for_aabb (ray_impl.rs:118-145) */
#define BVHGPU_TRAVERSE_STATS 2u   /* also count reference-equivalent loop iterations (flat_bvh.rs:408).  Exact for every tree whose
                                      leaves' navigator boxes equal the shapes' AABBs — all but trees with a split that had no SAH
                                      winner (empty child bounds, bvh_node.rs:225-230): there the leaf-entry visits behind an empty
                                      navigator box are not counted (the hit lists are still the reference's) */
#define BVHGPU_TRAVERSE_TRIANGLES 4u /* also run Ray::intersects_triangle (ray_impl.rs:154-213) on every returned shape, as the
                                        reference's harness does after traverse (testbase.rs:826-836): Intersection{distance,u,v} per hit */
#define BVHGPU_TRAVERSE_CLOSEST 8u   /* triangle stage fused into the walk, no CSR: per ray the candidate with the smallest
                                        Intersection.distance (first one on ties) and its shape index */

#define BVHGPU_TRAVERSE_NEAREST_FIRST 32u  /* per-ray order of Bvh::nearest_child_traverse_iterator (bvh_impl.rs:184-190,
                                              child_distance_traverse.rs) instead of flat-array order */
#define BVHGPU_TRAVERSE_FARTHEST_FIRST 64u /* ... of Bvh::farthest_child_traverse_iterator (bvh_impl.rs:206-212) */
#define BVHGPU_TRAVERSE_BEST_FIRST 128u     /* with NEAREST_FIRST / FARTHEST_FIRST: the per-ray order of Bvh::nearest_traverse_iterator /
                                              farthest_traverse_iterator (bvh_impl.rs:145-176) = DistanceTraverseIterator
                                              (distance_traverse.rs:40-158), a best-first walk driven by a BinaryHeap, instead of
                                              the child-ordered depth-first iterator */
#define BVHGPU_TRAVERSE_RAYS_READY 256u /* hint for bvhgpu_traverse_async_*: the rays were complete before the tree's asynchronous rebuild was
                                          enqueued (resident ray buffers of a frame loop).  The engine may then read them while the build
                                          is still running — the wide walk's per-ray item filter runs beside the build on a second
                                          stream instead of in front of the walk.  Results never depend on it */
#define BVHGPU_TRAVERSE_RAYS_OD6 512u /* bvhgpu_traverse_host_* / bvhgpu_build_traverse_host_* only: `origins` points to n_rays x 6 T — origin xyz, direction xyz
                                        per ray, the arguments of Ray::new side by side — and `directions` is ignored.  One transfer per chunk
                                        instead of two: the copy engines idle 10 - 20 µs between two transfers */
#define BVHGPU_TRAVERSE_COHERENT 16u /* hint: neighbouring rays are similar (primary rays).  Large whole-ray batches then hand their hits over
                                        through per-ray slots instead of pool records (BVHGPU_TUNE_WIDE_STAGE_SHIFT); results never depend on it */
#define BVHGPU_TRAVERSE_FIRST 1024u /* bvhgpu_traverse_box_* / bvhgpu_traverse_sphere_* only: the first candidate of the ray's list instead of the nearest one */

/* ---- POD layouts (little-endian, natural alignment, no packing pragmas) ---- */

/* Aabb<T,3> (aabb_impl.rs:10-16) is passed as 6 scalars: min x,y,z, max x,y,z. */

/* enum BvhNode<T,3> (bvh_node.rs:21-47) as a POD.
 * Node: shape == BVHGPU_NONE; l,r = child_l_index, child_r_index; l_min..r_max = child AABBs.
 * Leaf: shape = shape_index; l = r = BVHGPU_NONE; AABB fields are zero. */
typedef struct { float l_min[3], l_max[3], r_min[3], r_max[3]; uint32_t parent, l, r, shape; } bvhgpu_node_f32;  /*  64 B */
typedef struct { double l_min[3], l_max[3], r_min[3], r_max[3]; uint32_t parent, l, r, shape; } bvhgpu_node_f64; /* 112 B */

/* struct FlatNode<T,3> (flat_bvh.rs:17-46), same field order.  Leaf entries carry
 * Aabb::empty() = (+inf,-inf) exactly like flat_bvh.rs:133. */
typedef struct { float min[3], max[3]; uint32_t entry, exit, shape; } bvhgpu_flat_f32;                 /* 36 B */
typedef struct { double min[3], max[3]; uint32_t entry, exit, shape, _pad; } bvhgpu_flat_f64;          /* 64 B */

/* struct Ray<T,3> (ray_impl.rs:17-29), same field order: origin, direction (normalised), inv_direction. */
typedef struct { float o[3], d[3], inv[3]; } bvhgpu_ray_f32;   /* 36 B */
typedef struct { double o[3], d[3], inv[3]; } bvhgpu_ray_f64;  /* 72 B */

typedef struct bvhgpu_ctx bvhgpu_ctx;
typedef struct bvhgpu_tree bvhgpu_tree;
typedef struct bvhgpu_hits bvhgpu_hits;

typedef struct {
    uint64_t hits;        /* total shapes returned                                                  */
    uint64_t visited;     /* reference loop iterations (flat_bvh.rs:408) = slab tests; STATS flag   */
    uint64_t leaf_visits; /* of which leaf entries (second test of a shape AABB, :411-418); STATS   */
    uint64_t device_steps;/* node visits this engine actually performed (folded layout); STATS      */
    uint64_t wave_steps;  /* wavefront iterations of the walk loop: device_steps / (64 * wave_steps) = lane utilisation */
} bvhgpu_traverse_stats;

/* ---- context ---- */
int bvhgpu_abi_version(void);
int bvhgpu_device_count(int *out);
const char *bvhgpu_status_string(int status);
/* One ctx = one GPU + one stream + scratch.  stream == NULL → the ctx creates its own stream;
 * otherwise `stream` is a hipStream_t owned by the caller (e.g. torch's current stream). */
int bvhgpu_create(int device, void *stream, bvhgpu_ctx **out);
void bvhgpu_destroy(bvhgpu_ctx *ctx);
const char *bvhgpu_last_error(const bvhgpu_ctx *ctx);
int bvhgpu_synchronize(bvhgpu_ctx *ctx);
void *bvhgpu_stream(bvhgpu_ctx *ctx); /* the hipStream_t work is enqueued on */

/* ---- device memory for hosts without HIP bindings (a Rust or C caller that keeps rays / AABBs resident in HBM, the
 * BVHGPU_DEVICE form of every `mem` argument): hipMalloc / hipFree / a synchronous hipMemcpy on the ctx's device.
 * Memory from any other allocator of the same device (hipMalloc, a torch tensor) is just as good. ---- */
int bvhgpu_device_alloc(bvhgpu_ctx *ctx, size_t bytes, void **out);
int bvhgpu_device_free(bvhgpu_ctx *ctx, void *ptr);
int bvhgpu_device_copy(bvhgpu_ctx *ctx, void *dst, int dst_mem, const void *src, int src_mem, size_t bytes);

/* ---- pinned host memory (ABI 7).  Every BVHGPU_HOST argument may be ordinary (pageable) memory; memory from
 * bvhgpu_host_alloc — or a range the caller owns and has announced with bvhgpu_host_register, e.g. the allocation behind a
 * Vec that lives as long as the scene — is read and written by the DMA engines directly (≈ 55 GB/s on the PCIe 5 link instead of
 * ≈ 30 through the runtime's staging copies) and lets the asynchronous entry points return before the copy has happened.
 * hipHostMalloc / hipHostFree / hipHostRegister / hipHostUnregister on the ctx's device. ---- */
int bvhgpu_host_alloc(bvhgpu_ctx *ctx, size_t bytes, void **out);
int bvhgpu_host_free(bvhgpu_ctx *ctx, void *ptr);
int bvhgpu_host_register(bvhgpu_ctx *ctx, void *ptr, size_t bytes);
int bvhgpu_host_unregister(bvhgpu_ctx *ctx, void *ptr);

/* ---- build: replaces Bvh::build / Bvh::build_par / build_with_executor (bvh_impl.rs:40-96,
 * bounding_hierarchy.rs:158-177) once the caller has gathered shape.aabb() for every shape
 * (aabb_impl.rs:28-56) into `aabbs` = n x [min xyz, max xyz].  n == 0 → valid empty tree
 * (bvh_impl.rs:57-59).  The caller keeps `aabbs`; the tree owns its own HBM copy. ---- */
int bvhgpu_build_f32(bvhgpu_ctx *ctx, const float *aabbs, size_t n, int mem, bvhgpu_tree **out);
int bvhgpu_build_f64(bvhgpu_ctx *ctx, const double *aabbs, size_t n, int mem, bvhgpu_tree **out);
/* Rebuild in place (same dtype, n <= capacity of the first build): no allocation on the hot loop.  A different shape count
 * drops the triangle vertices of bvhgpu_tree_set_triangles (one triangle per shape); with the same count they are kept and
 * are the caller's to refresh. */
int bvhgpu_rebuild_f32(bvhgpu_tree *tree, const float *aabbs, size_t n, int mem);
int bvhgpu_rebuild_f64(bvhgpu_tree *tree, const double *aabbs, size_t n, int mem);
/* FlatBvh::build (flat_bvh.rs:328-331) = Bvh::build + Bvh::flatten in ONE call (one host round trip): the tree is
 * both built and flattened on return. */
int bvhgpu_build_flat_f32(bvhgpu_ctx *ctx, const float *aabbs, size_t n, int mem, bvhgpu_tree **out);
int bvhgpu_build_flat_f64(bvhgpu_ctx *ctx, const double *aabbs, size_t n, int mem, bvhgpu_tree **out);
int bvhgpu_rebuild_flat_f32(bvhgpu_tree *tree, const float *aabbs, size_t n, int mem);
int bvhgpu_rebuild_flat_f64(bvhgpu_tree *tree, const double *aabbs, size_t n, int mem);
/* The shapes moved but are the same shapes: keep the topology, recompute every child AABB from the new shape AABBs —
 * Bvh::fix_aabbs_ascending (optimization.rs:355-391: child boxes = children's get_node_aabb, bvh_node.rs:616-625)
 * applied to the whole tree.  n must equal the tree's shape count; the tree must have been built here.  If the tree
 * is flattened its flat / traversal arrays are regenerated.  The result is consistent and tight (the properties
 * the reference asserts after update_shapes, optimization.rs tests); refit with the AABBs of the build reproduces
 * the built tree bit for bit, unless a split had no SAH winner (then the empty child boxes become exact joins and the
 * wide walk becomes available).
 * Input contract: the builders'.  For n >= 2 a NaN or +-inf component anywhere in `aabbs` makes the call itself return
 * BVHGPU_INVALID_ARG and the tree — BvhNode array, its copy of the shape AABBs, flat / traversal arrays — is left exactly
 * as it was (the input is checked on the device before anything is written: the call waits for that check, one host round
 * trip; HOST input is staged in the ctx meanwhile).  A single shape (n == 1) is accepted as it is, as the builders accept
 * it.  Bvh::update_shapes itself (optimization.rs:337-352: remove + re-insert, one shape at a
 * time, topology changes) has no device counterpart: moved shapes are answered by this refit or by a rebuild.
 * Triangle vertices (bvhgpu_tree_set_triangles) are the caller's to refresh. */
int bvhgpu_refit_f32(bvhgpu_tree *tree, const float *aabbs, size_t n, int mem);
int bvhgpu_refit_f64(bvhgpu_tree *tree, const double *aabbs, size_t n, int mem);
void bvhgpu_tree_destroy(bvhgpu_tree *tree);

/* ---- asynchronous step.  The calls above return when their result is complete (one host round trip each).  These
 * enqueue the same work on the ctx's stream and return at once, so that ONE host thread can keep several steps in flight
 * (on several ctxs = several streams: the latency-bound build of one step overlaps the traversal of another).
 *   bvhgpu_rebuild_flat_async_*  = bvhgpu_rebuild_flat_* (Bvh::build_par + Bvh::flatten) without the wait.  `aabbs` must stay
 *                                  valid until the wait (BVHGPU_HOST: pinned memory, or the copy is synchronous anyway).
 *   bvhgpu_traverse_async_*      = bvhgpu_traverse_* on rays resident in HBM (mem must be BVHGPU_DEVICE); the tree may
 *                                  still be building on the same stream.
 *   bvhgpu_hits_wait             completes the batch: waits for the stream, completes the tree's build (input validation;
 *                                  an unbalanced tree is finished level by level) and replays the batch if the optimistic
 *                                  launch was not enough (hit pool too small, tree not finished when the walk ran).  The
 *                                  statuses the synchronous calls would have returned are returned here.
 *   bvhgpu_tree_wait             the same for a tree alone.  Every other entry point that looks at a tree waits by itself.
 * Lifetimes: the rays of an asynchronous batch must stay valid until its bvhgpu_hits_wait (a replay reads them again).  The tree
 * may be waited for, traversed again, rebuilt or destroyed in any order: every result object remembers which generation of the tree
 * it walked and whether that generation was still unfinalized, so its wait replays exactly when needed, whoever finalized the
 * build first; a rebuild / refit / import / destroy of the tree first completes the batches still in flight on it (their own
 * bvhgpu_hits_wait then returns what that completion found).  bvhgpu_hits_fetch* / _info / _device return BVHGPU_INVALID_ARG on a
 * result object whose batch has not been waited for. */
int bvhgpu_rebuild_flat_async_f32(bvhgpu_tree *tree, const float *aabbs, size_t n, int mem);
int bvhgpu_rebuild_flat_async_f64(bvhgpu_tree *tree, const double *aabbs, size_t n, int mem);
int bvhgpu_tree_wait(bvhgpu_tree *tree);

int bvhgpu_tree_info(const bvhgpu_tree *tree, int *dtype, size_t *n_shapes, size_t *n_nodes, size_t *n_flat);
/* Vec<BvhNode> (bvh_impl.rs:27-33): 2n-1 entries of bvhgpu_node_f32/_f64. */
int bvhgpu_tree_nodes(bvhgpu_tree *tree, void *out, int mem);
/* the argument of BHShape::set_bh_node_index for every shape (bvh_node.rs:102; bounding_hierarchy.rs:53-65). */
int bvhgpu_tree_shape_nodes(bvhgpu_tree *tree, uint32_t *out, int mem);
/* number of level-synchronous passes the last build needed (diagnostic). */
int bvhgpu_tree_build_levels(const bvhgpu_tree *tree, int *levels);

/* ---- flatten: replaces Bvh::flatten / flatten_custom (flat_bvh.rs:240-251, 312-319).  Produces the
 * reference-layout FlatNode array (3n-2 entries) and the engine's own traversal array in HBM. ---- */
int bvhgpu_flatten(bvhgpu_tree *tree);
int bvhgpu_flat_nodes(bvhgpu_tree *tree, void *out, int mem);
/* Upload a FlatBvh built elsewhere (e.g. by the Rust crate through flatten_custom with a #[repr(C)]
 * constructor) together with the shapes' current AABBs; replaces FlatBvh ownership (flat_bvh.rs:254). */
int bvhgpu_tree_from_flat_f32(bvhgpu_ctx *ctx, const bvhgpu_flat_f32 *flat, size_t n_flat, const float *shape_aabbs,
                              size_t n, bvhgpu_tree **out);
int bvhgpu_tree_from_flat_f64(bvhgpu_ctx *ctx, const bvhgpu_flat_f64 *flat, size_t n_flat, const double *shape_aabbs,
                              size_t n, bvhgpu_tree **out);

/* ---- scene transport for multi-GPU: one contiguous blob (traversal array + shape AABBs + LDS slot
 * table + triangle vertices when set) that the
 * caller broadcasts (RCCL via torch.distributed / ncclBroadcast) and imports on the peers.  A tree
 * imported this way supports traversal only.  For bvhgpu_scene_import *out may point to NULL (a
 * tree is allocated) or to a tree a previous bvhgpu_scene_import returned (its HBM is reused). ---- */
int bvhgpu_scene_nbytes(const bvhgpu_tree *tree, size_t *nbytes);
int bvhgpu_scene_export(bvhgpu_tree *tree, void *dst, int mem);
int bvhgpu_scene_import(bvhgpu_ctx *ctx, const void *src, size_t nbytes, int mem, bvhgpu_tree **out);

/* ---- multi-GPU: rays shard across the GPUs of a node, the tree is read-only after flatten — the path has
 * exactly ONE exchange step, a broadcast of the root's flattened tree to the peers, done here with RCCL over xGMI
 * straight out of / into the trees' own HBM buffers (traversal array, shape AABBs, LDS slot table, optionally the
 * triangle vertices).  Hit lists stay on the GPU that produced them.  The reference has no counterpart (single
 * address space); this is what replaces sharing `&FlatBvh` between rayon workers.
 * A communicator is formed either by ONE process over `ndev` ctxs (one per GPU, ncclCommInitAll), or by one process per
 * GPU: rank 0 calls bvhgpu_comm_unique_id, the launcher carries the 128 bytes to the peers (MPI, a torch.distributed
 * store, a file …) and every rank calls bvhgpu_comm_init_rank.  `trees` has one entry per LOCAL device of the
 * communicator (one entry in the process-per-GPU form); the root's entry is the source, a peer's entry is NULL (a tree
 * is allocated) or the result of an earlier broadcast / scene import on that ctx (its HBM is reused).  Received trees
 * support traversal and point queries only (no BvhNode array).  The calls are collective: every rank must make them. */
typedef struct bvhgpu_comm bvhgpu_comm;
#define BVHGPU_COMM_ID_BYTES 128
#define BVHGPU_BCAST_TRIANGLES 1u
int bvhgpu_comm_unique_id(void *id_out /* BVHGPU_COMM_ID_BYTES */);
int bvhgpu_comm_init_rank(bvhgpu_ctx *ctx, int nranks, int rank, const void *id, bvhgpu_comm **out);
int bvhgpu_comm_init_all(bvhgpu_ctx *const *ctxs, int ndev, bvhgpu_comm **out);
int bvhgpu_comm_info(const bvhgpu_comm *comm, int *nranks, int *first_rank, int *n_local);
void bvhgpu_comm_destroy(bvhgpu_comm *comm);
/* Which RCCL the broadcasts go through: `version` = ncclGetVersion's code (major*10000 + minor*100 + patch; 0 if the library
 * has no such entry point), `shared_with_process` = 1 when the copy was already loaded in the process (PyTorch bundles one) and
 * no second RCCL was opened, `library_path` = the file the entry points were resolved from (truncated to cap).  Loads RCCL on
 * first use like every bvhgpu_comm_* call; BVHGPU_RCCL_ERROR when there is none.  Launchers print it so that a scaling record
 * shows how many ranks over which library it ran (bench.py's "rccl" object). */
int bvhgpu_rccl_info(int *version, int *shared_with_process, char *library_path, size_t cap);
/* peers learn type and size from a 64-byte header that travels first (one host round trip per rank).  If the root has no valid
 * tree (NULL, not flattened, invalid input) it still sends the header: its own call returns the reason, the peers' calls return
 * BVHGPU_INVALID_ARG — nobody is left waiting inside a collective. */
int bvhgpu_bcast(bvhgpu_comm *comm, bvhgpu_tree **trees, int root);
/* every rank already knows dtype and shape count (a frame loop over a scene of constant size): one group of broadcasts
 * (status header + arrays) enqueued on the ctxs' streams, no host round trip on any rank; `what`: BVHGPU_BCAST_TRIANGLES to send
 * the vertices too.  The root's tree must be a tree built (or received) here with exactly that dtype / shape count; it may
 * still be building (bvhgpu_rebuild_flat_async_*): the header is then composed on the device from the build's own status.
 * The peers' trees are usable on their streams at once (bvhgpu_traverse_async_*); the header is looked at when a peer's tree
 * is first waited for: BVHGPU_INVALID_ARG = the root had nothing valid to send (the root's call or wait returned the reason),
 * BVHGPU_REBROADCAST = see the status codes.  A received tree carries the root's `exact_only` property (a split without SAH
 * winner, bvh_node.rs:225-230: no wide walk), as does a scene blob. */
int bvhgpu_bcast_known(bvhgpu_comm *comm, bvhgpu_tree **trees, int root, int dtype, size_t n_shapes, unsigned what);

/* ---- rays ---- */
/* Ray::new (ray_impl.rs:70-80) for a batch: normalise, cache 1/d.  origins/dirs: n x 3. */
int bvhgpu_rays_new_f32(bvhgpu_ctx *ctx, const float *origins, const float *dirs, size_t n, int mem_in,
                        bvhgpu_ray_f32 *out, int mem_out);
int bvhgpu_rays_new_f64(bvhgpu_ctx *ctx, const double *origins, const double *dirs, size_t n, int mem_in,
                        bvhgpu_ray_f64 *out, int mem_out);
/* The bench harness' ray stream create_ray(seed, bounds) (testbase.rs:687-691, seed 0 at :825),
 * rays [first, first+n) generated directly in HBM (`out` is device memory). */
int bvhgpu_gen_rays_f32(bvhgpu_ctx *ctx, uint64_t first, size_t n, const float bounds[6], bvhgpu_ray_f32 *out_dev);
/* same stream widened to f64 AFTER generation (f32 origin/target → f64 Ray::new), for the f64 config. */
int bvhgpu_gen_rays_f64(bvhgpu_ctx *ctx, uint64_t first, size_t n, const float bounds[6], bvhgpu_ray_f64 *out_dev);

/* ---- point query: replaces <FlatBvh as BoundingHierarchy>::nearest_to (flat_bvh.rs:513-562; trait
 * bounding_hierarchy.rs:262-336) for n query points (n x 3).  The shape's PointDistance::distance_squared is a user
 * callback in the reference; the two the reference's harness defines are built in: kind 0 = the shape's own
 * Aabb::min_distance_squared (UnitBox, testbase.rs:101-105; aabb_impl.rs:618-629), kind 1 = closest point on the
 * triangle (testbase.rs:367-443, needs bvhgpu_tree_set_triangles).  out_shape[i] = shape index (BVHGPU_NONE for an
 * empty hierarchy), out_dist[i] = the distance (not squared, :561).  `mem` applies to all three buffers. ---- */
int bvhgpu_nearest_f32(bvhgpu_tree *tree, const float *points, size_t n, int mem, int kind, uint32_t *out_shape, float *out_dist);
int bvhgpu_nearest_f64(bvhgpu_tree *tree, const double *points, size_t n, int mem, int kind, uint32_t *out_shape, double *out_dist);

/* ---- k nearest shapes per point (ABI 7).  The reference has no such query; the engine defines it as the smallest change to the loop of
 * nearest_to over the FlatNode array (flat_bvh.rs:524-558): `best_element` becomes a list L of at most k pairs (dist2, shape).
 *   full = len(L) == k;  bound = L[last].dist2
 *   non-leaf entry (:546-556): md = node.aabb.min_distance_squared(query); go to entry_index iff !full || md < bound, else to exit_index
 *   leaf entry (:533-544): d = shape.distance_squared(query); accept iff !full || d < bound.  On accept: if full, drop L[last]; insert
 *     (d, shape) in front of the first element e with d < e.dist2, or at the end if there is none.  Then exit_index.
 * All comparisons are the strict < of the scalar type.  So a NaN distance is accepted only while the list is not full, goes behind
 * everything the list holds at that moment, and once it is L[last] of a full list nothing replaces it (what nearest_to does with a NaN
 * best_dist).  Entries accepted later that are not smaller than anything in front of the NaN land behind it: a row that holds a NaN
 * need not be sorted.  Rows without a NaN are ascending, and among equal distances the shape met first (leaf pre-order) comes first.
 * Output row i: out_shape[i*k + j] = L[j].shape, out_dist[i*k + j] = sqrt(L[j].dist2) (:561) for j < len(L); the remaining k - len(L)
 * slots (fewer than k shapes, an empty hierarchy) are PADDING: shape BVHGPU_NONE, distance +inf.  (bvhgpu_nearest_* writes distance 0
 * for an empty hierarchy; a padded slot here is +inf so that a NaN-free row stays ascending.)  With k = 1 a row is bit for bit what
 * bvhgpu_nearest_* returns, except that distance of the empty hierarchy.
 * kind as for bvhgpu_nearest_*: 0 = the shape's own Aabb::min_distance_squared (a point cloud is kind 0 on zero-size boxes), 1 = closest
 * point on the triangle (needs bvhgpu_tree_set_triangles).  1 <= k <= BVHGPU_KNN_MAX_K, else BVHGPU_INVALID_ARG; n * k must stay below
 * 2^32 (BVHGPU_OVERFLOW).  `mem` applies to all three buffers; n = 0 is fine.  The tree must be flattened.  The call
 * returns when the rows are complete (BVHGPU_DEVICE too). ---- */
#define BVHGPU_KNN_MAX_K 64u /* the lists of a 64-lane workgroup live in LDS: 64 x 64 x (8 + 4) bytes = 48 KB in f64 */
int bvhgpu_knearest_f32(bvhgpu_tree *tree, const float *points, size_t n, int mem, int kind, uint32_t k,
                        uint32_t *out_shape /* n x k */, float *out_dist /* n x k */);
int bvhgpu_knearest_f64(bvhgpu_tree *tree, const double *points, size_t n, int mem, int kind, uint32_t k,
                        uint32_t *out_shape /* n x k */, double *out_dist /* n x k */);

/* ---- the same rows found nearest child first (the "tree form"; bvhgpu_knearest_* above is the "flat form").  Definition:
 * BvhNode::nearest_to_recursive (bvh_node.rs:327-374, what Bvh::nearest_to calls, bvh_impl.rs:221-238) over the BvhNode array, with the
 * list L above in place of `best_candidate` and an optional limit per point, m = max_dist[i]:
 *   full = len(L) == k;  bound = L[last].dist2;  r2 = m * m (one multiplication in T)
 *   admit(x) = (max_dist == NULL || (m >= 0 && x <= r2)) && (!full || x < bound)
 *   visit(node), starting at node 0:
 *     Leaf{shape}: d = shape.distance_squared(p) (kind as above); if admit(d): drop L[last] of a full list and insert (d, shape) in front
 *       of the first element e with d < e.dist2, or at the end if there is none.
 *     Node{l, l_aabb, r, r_aabb}: c = [(l, l_aabb.min_distance_squared(p)), (r, r_aabb.min_distance_squared(p))]; if c[0].1 > c[1].1
 *       swap them (strict >: ties and NaN keep the left child first); then for (idx, cd) in c: if admit(cd): visit(idx) — the second
 *       test sees the list as the first subtree left it.
 * Every comparison is the <, > or <= of the scalar type exactly as written; a NaN distance behaves as in the flat form (a row that holds
 * a NaN need not be sorted).  Rows without a NaN are ascending.  TIES: equal distances stay in the order THIS walk meets them, which is
 * not leaf pre-order — the flat and the tree form may order equal distances differently, and may pick different shapes among ties at the
 * k-th distance.
 * Output row i as for bvhgpu_knearest_*: out_shape[i*k + j] = L[j].shape, out_dist[i*k + j] = sqrt(L[j].dist2) for j < len(L); the other
 * slots are PADDING: shape BVHGPU_NONE, distance +inf.  An empty hierarchy gives rows of padding.  With k = 1 and max_dist == NULL a row
 * is bit for bit what Bvh::nearest_to returns (except the empty hierarchy's distance, +inf here).
 * max_dist: NULL, or n values of the tree's dtype in the points' memory space.  A shape or subtree farther than max_dist[i] is never
 * admitted (dist2 <= max_dist[i]^2 is the test, so the limit itself is inside); 0 keeps only shapes at distance 0; a negative or NaN
 * max_dist[i] gives a row of padding; +inf differs from NULL only for NaN distances (NaN <= +inf is false).
 * Arguments as for bvhgpu_knearest_*: 1 <= k <= BVHGPU_KNN_MAX_K, else BVHGPU_INVALID_ARG; kind 1 needs bvhgpu_tree_set_triangles;
 * n * k below 2^32 (BVHGPU_OVERFLOW); n = 0 is fine; `mem` applies to all four buffers.  The tree must have been built here
 * (bvhgpu_build_* / rebuild_*, still building or not): an uploaded FlatBvh, a scene import or a broadcast carries no BvhNode array
 * and gets BVHGPU_INVALID_ARG.  It need NOT be flattened, as Bvh::nearest_to needs no FlatBvh.  The walk has no depth limit.  The call
 * returns when the rows are complete (BVHGPU_DEVICE too). ---- */
int bvhgpu_knearest_tree_f32(bvhgpu_tree *tree, const float *points, size_t n, int mem, int kind, uint32_t k,
                             const float *max_dist /* NULL, or n values in the points' memory space */,
                             uint32_t *out_shape /* n x k */, float *out_dist /* n x k */);
int bvhgpu_knearest_tree_f64(bvhgpu_tree *tree, const double *points, size_t n, int mem, int kind, uint32_t k,
                             const double *max_dist /* NULL, or n values in the points' memory space */,
                             uint32_t *out_shape /* n x k */, double *out_dist /* n x k */);

/* Ray::intersects_triangle (ray_impl.rs:154-213) for n independent pairs: ray i against triangle i
 * (tris: n x [a xyz, b xyz, c xyz]); out: n x {distance,u,v}.  `mem` applies to all three buffers. */
int bvhgpu_ray_triangle_pairs_f32(bvhgpu_ctx *ctx, const bvhgpu_ray_f32 *rays, const float *tris, size_t n, int mem, float *out);
int bvhgpu_ray_triangle_pairs_f64(bvhgpu_ctx *ctx, const bvhgpu_ray_f64 *rays, const double *tris, size_t n, int mem, double *out);

/* Coherent primary rays (BASELINE.json configs[2]; the reference has no camera, this is the engine's definition,
 * which the tests' CPU checker restates operation by operation).  cam = eye[3], right[3], up[3], forward[3], tan_x, tan_y.
 * Ray `first + i` belongs to pixel x = id % width, y = id / width:  sx = (((x + 0.5) / W) * 2) - 1,
 * sy = 1 - (((y + 0.5) / H) * 2),  dir = (forward + (sx * tan_x) * right) + (sy * tan_y) * up  (separately
 * rounded f32 operations), ray = Ray::new(eye, dir) (ray_impl.rs:70-80).  `out_dev` is device memory. */
int bvhgpu_gen_primary_rays_f32(bvhgpu_ctx *ctx, const float cam[14], uint32_t width, uint32_t height, uint64_t first,
                                size_t n, bvhgpu_ray_f32 *out_dev);
int bvhgpu_gen_primary_rays_f64(bvhgpu_ctx *ctx, const float cam[14], uint32_t width, uint32_t height, uint64_t first,
                                size_t n, bvhgpu_ray_f64 *out_dev);

/* ---- traverse: replaces <FlatBvh as BoundingHierarchy>::traverse (flat_bvh.rs:396-431) and, by the
 * equivalence of bvh_node.rs:288-319, Bvh::traverse (bvh_impl.rs:104-119), for a BATCH of rays.
 * Result = CSR: offsets[n_rays+1], indices[total]; ray i's shapes are indices[offsets[i]..offsets[i+1])
 * in the reference's order (flat-array / DFS left-first order).
 * *hits may point to NULL (a result object is allocated) or to a previous result (buffers reused). ---- */
int bvhgpu_traverse_f32(bvhgpu_tree *tree, const bvhgpu_ray_f32 *rays, size_t n_rays, int mem, unsigned flags,
                        bvhgpu_hits **hits);
int bvhgpu_traverse_f64(bvhgpu_tree *tree, const bvhgpu_ray_f64 *rays, size_t n_rays, int mem, unsigned flags,
                        bvhgpu_hits **hits);

/* ---- the same for a caller whose rays live in HOST memory and who wants the hit lists back in host memory (ABI 7): what
 * GpuBvh::traverse_batch of the Rust shim does, in one call.  Replaces `for ray in rays { flat.traverse(&Ray::new(o, d), shapes) }`
 * (ray_impl.rs:70-80, flat_bvh.rs:396-431).
 *   origins, directions   n_rays x 3 T each: Ray::new runs on the device (normalised direction and 1/d correctly rounded: the bits
 *                         Ray::new gives) — 24 bytes per ray cross the link instead of the 36 of a Ray struct.
 *                         directions == NULL: `origins` points to n_rays Ray structs (bvhgpu_ray_f32 / _f64), used as they are.
 *   offsets               n_rays + 1 entries, always written.
 *   indices, indices_cap  written when the batch's hit total fits (total <= indices_cap); otherwise the call still succeeds,
 *                         *total says what is needed and bvhgpu_traverse_host_indices fetches them (no second traversal).
 *   flags                 0, BVHGPU_TRAVERSE_COHERENT, BVHGPU_TRAVERSE_RAYS_OD6 (origins = n_rays x [o xyz, d xyz], directions ignored).
 * The tree may still be building (bvhgpu_rebuild_flat_async_* with BVHGPU_HOST shapes): the ray upload does not wait for the build.
 * The batch is walked in chunks (BVHGPU_TUNE_HOST_CHUNKS: by default three, the last one an eighth of the batch) on three streams — upload of
 * chunk k+1, Ray::new + walk of chunk k, download of the offsets of chunk k-1 — with one host wait at the end; with pinned buffers (bvhgpu_host_alloc / _register) the copies are DMA at link
 * speed.  Results are those of bvhgpu_traverse_* on the same rays, byte for byte.  Returns when everything is in the caller's buffers. */
int bvhgpu_traverse_host_f32(bvhgpu_tree *tree, const float *origins, const float *directions, size_t n_rays, unsigned flags,
                             uint32_t *offsets, uint32_t *indices, size_t indices_cap, uint64_t *total);
int bvhgpu_traverse_host_f64(bvhgpu_tree *tree, const double *origins, const double *directions, size_t n_rays, unsigned flags,
                             uint32_t *offsets, uint32_t *indices, size_t indices_cap, uint64_t *total);
int bvhgpu_traverse_host_indices(bvhgpu_ctx *ctx, uint32_t *indices, size_t indices_cap);
/* GpuBvh::build + traverse_batch of a frame in ONE call: bvhgpu_rebuild_flat_async_*(aabbs, BVHGPU_HOST) + bvhgpu_traverse_host_*, with the
 * ray upload enqueued FIRST — it is the long pole (24 MB against the build's 3) and depends on nothing — so that the build (Bvh::build_par +
 * flatten, bvh_impl.rs:40-96, flat_bvh.rs:240-319) runs underneath it.  Same results, same errors (NaN / inf shapes: BVHGPU_INVALID_ARG,
 * nothing usable built). */
int bvhgpu_build_traverse_host_f32(bvhgpu_tree *tree, const float *aabbs, size_t n, const float *origins, const float *directions, size_t n_rays,
                                   unsigned flags, uint32_t *offsets, uint32_t *indices, size_t indices_cap, uint64_t *total);
int bvhgpu_build_traverse_host_f64(bvhgpu_tree *tree, const double *aabbs, size_t n, const double *origins, const double *directions, size_t n_rays,
                                   unsigned flags, uint32_t *offsets, uint32_t *indices, size_t indices_cap, uint64_t *total);
int bvhgpu_traverse_async_f32(bvhgpu_tree *tree, const bvhgpu_ray_f32 *rays, size_t n_rays, int mem, unsigned flags,
                              bvhgpu_hits **hits);
int bvhgpu_traverse_async_f64(bvhgpu_tree *tree, const bvhgpu_ray_f64 *rays, size_t n_rays, int mem, unsigned flags,
                              bvhgpu_hits **hits);
int bvhgpu_hits_wait(bvhgpu_hits *hits);
/* Triangle vertices of the shapes (n x [a xyz, b xyz, c xyz], the fields of testbase.rs Triangle :316-323) for the
 * TRIANGLES / CLOSEST flags; n must equal the tree's shape count.  The tree keeps its own HBM copy. */
int bvhgpu_tree_set_triangles_f32(bvhgpu_tree *tree, const float *verts, size_t n, int mem);
int bvhgpu_tree_set_triangles_f64(bvhgpu_tree *tree, const double *verts, size_t n, int mem);
int bvhgpu_hits_info(const bvhgpu_hits *hits, size_t *n_rays, uint64_t *total, bvhgpu_traverse_stats *stats);
/* Which form of the walk produced the batch the result object holds (diagnostic; the lists never depend on it): */
#define BVHGPU_WALK_WIDE 1u       /* the 4-wide walk (batches of BVHGPU_TUNE_TRAVERSE_LDS_MIN_RAYS rays and more) */
#define BVHGPU_WALK_STAGED 2u     /* ... with a ray's first hits handed over through its own slot (BVHGPU_TUNE_WIDE_STAGE_SHIFT) */
#define BVHGPU_WALK_REC8 4u       /* ... with pool records of 8 bytes per hit (BVHGPU_TUNE_WIDE_REC8) */
#define BVHGPU_WALK_F64_GUIDE 8u  /* ... over the f32 guide boxes of an f64 tree, leaf candidates confirmed in f64 (BVHGPU_TUNE_WIDE_F64_GUIDE) */
int bvhgpu_hits_walk_info(const bvhgpu_hits *hits, unsigned *flags);
/* ... and the name of the walk kernel it was handed to, NUL-terminated, spelled the way rocprofv3 prints kernel names (e.g.
 * "bvhgpu::k_traverse_wide<float, 0, 2, 1024, 8, 0>"): what a profile of the same call must be looked up under (diagnostic, ABI 6) */
int bvhgpu_hits_walk_kernel(const bvhgpu_hits *hits, char *name, size_t cap);
/* copy out; indices / tslice may be NULL.  tslice: 2 scalars of the tree's dtype per hit (flag T_SLICE). */
int bvhgpu_hits_fetch(bvhgpu_hits *hits, uint32_t *offsets, uint32_t *indices, void *tslice, int mem);
/* TRIANGLES: 3 scalars {distance,u,v} per hit, CSR order (distance = +inf: no intersection, ray_impl.rs:150-151). */
int bvhgpu_hits_fetch_triangles(bvhgpu_hits *hits, void *isect, int mem);
/* CLOSEST: per ray {distance,u,v} (+inf,0,0 when nothing is hit) and the shape index (BVHGPU_NONE when nothing is hit). */
int bvhgpu_hits_fetch_closest(bvhgpu_hits *hits, void *isect, uint32_t *shape, int mem);
/* borrow the device arrays (valid until the next traverse into / destroy of this result). */
int bvhgpu_hits_device(const bvhgpu_hits *hits, const uint32_t **offsets, const uint32_t **indices, const void **tslice);
void bvhgpu_hits_destroy(bvhgpu_hits *hits);

/* ---- AABB / point / ball queries: <FlatBvh as BoundingHierarchy>::traverse (flat_bvh.rs:396-431) with the crate's other three
 * IntersectsAabb queries (aabb/intersection.rs:35-45, ball.rs:102-106), for a BATCH.  Query i's list is the list
 * FlatBvh::traverse(&q_i, shapes) returns, in its order (flat-array / DFS left-first order): inner entries test the node box, leaf
 * entries the shape's own AABB, with the predicate of the kind (restated operation by operation, no contraction):
 *   BVHGPU_QUERY_AABB   6 T per query (min xyz, max xyz)  Aabb::intersects_aabb (aabb_impl.rs:240-248): a hit unless, on some axis,
 *                                                          q.max < lo or hi < q.min (touching counts; a NaN component hits every box)
 *   BVHGPU_QUERY_POINT  3 T per query                      Aabb::contains (aabb_impl.rs:175-177): lo <= p <= hi on all axes (NaN: no hit)
 *   BVHGPU_QUERY_BALL   4 T per query (centre xyz, radius) Ball::intersects_aabb (ball.rs:85-99): ((0 + d0*d0) + d1*d1) + d2*d2 <= r*r
 *                                                          with d = clamp(c, lo, hi) - c, clamp as num_traits (c < lo ? lo : c > hi ? hi : c)
 * `queries` lives in `mem` (HOST queries are staged into the result object).  queries == NULL with BVHGPU_QUERY_AABB and n equal to
 * the tree's shape count: query i is shape i's own AABB (broad phase, no upload; row i contains i).  `flags` is reserved (0).
 * The result is an ordinary result object: bvhgpu_hits_info / _fetch (tslice NULL) / _device / _walk_info / _walk_kernel / _wait
 * apply; _fetch_triangles / _fetch_closest return BVHGPU_INVALID_ARG.  Synchronises like bvhgpu_traverse_*.  Errors: queries of
 * another dtype than the tree's → BVHGPU_DTYPE_MISMATCH; an unknown kind → BVHGPU_INVALID_ARG; a tree that is not flattened →
 * BVHGPU_NOT_FLATTENED; more than 2^32-1 hits → BVHGPU_OVERFLOW.  A tree imported (scene blob, broadcast) from a build that had a
 * split without SAH winner is refused (BVHGPU_INVALID_ARG): its leaves' navigator boxes were folded away. */
#define BVHGPU_QUERY_AABB 1
#define BVHGPU_QUERY_POINT 2
#define BVHGPU_QUERY_BALL 3
int bvhgpu_query_f32(bvhgpu_tree *tree, int kind, const float *queries, size_t n, int mem, unsigned flags, bvhgpu_hits **hits);
int bvhgpu_query_f64(bvhgpu_tree *tree, int kind, const double *queries, size_t n, int mem, unsigned flags, bvhgpu_hits **hits);

/* ---- any-hit (occlusion) queries for ray segments: "does the segment from o to o + tmax·d hit any triangle?" (shadow / visibility rays).
 * Ray i comes with tmax[i] in the tree's dtype (tmax == NULL: +inf for every ray).  Let L_i be the list FlatBvh::traverse(&ray_i, shapes)
 * returns (flat_bvh.rs:396-431), in its order, and isect_s = Ray::intersects_triangle (ray_impl.rs:154-213) on shape s's triangle, the same
 * IEEE sequence as the TRIANGLES output.  The result for ray i is the FIRST s in L_i with isect_s.distance < tmax[i] (strict, in T) and its
 * Intersection {distance, u, v}; if there is none, BVHGPU_NONE and {+inf, 0, 0}.  So a miss (distance +inf) never occludes, not even with
 * tmax = +inf, and a NaN tmax or tmax <= epsilon never occludes.  The answer is the first candidate in reference order, not the nearest one:
 * it is deterministic, and every walk stops at it.  Needs bvhgpu_tree_set_triangles.
 * `rays` and `tmax` live in `mem` (HOST tmax is staged into the result object).  `flags`: 0 or BVHGPU_TRAVERSE_COHERENT (a hint); every other
 * bit → BVHGPU_INVALID_ARG.  No triangles → BVHGPU_INVALID_ARG; tree not flattened → BVHGPU_NOT_FLATTENED; another dtype than the tree's →
 * BVHGPU_DTYPE_MISMATCH; n_rays = 0 is fine.  Synchronises like bvhgpu_traverse_*.  bvhgpu_hits_info's `total` is the number of occluded
 * rays; _fetch / _fetch_triangles / _fetch_closest / _device return BVHGPU_INVALID_ARG on such a result, and bvhgpu_hits_fetch_any on any
 * other.  bvhgpu_hits_fetch_any: per ray {distance, u, v} (n x 3 T) and the shape (n u32); either may be NULL. */
int bvhgpu_traverse_any_f32(bvhgpu_tree *tree, const bvhgpu_ray_f32 *rays, const float *tmax, size_t n_rays, int mem, unsigned flags,
                            bvhgpu_hits **hits);
int bvhgpu_traverse_any_f64(bvhgpu_tree *tree, const bvhgpu_ray_f64 *rays, const double *tmax, size_t n_rays, int mem, unsigned flags,
                            bvhgpu_hits **hits);
int bvhgpu_hits_fetch_any(bvhgpu_hits *hits, void *isect, uint32_t *shape, int mem);

/* ---- closest-hit and any-hit ray queries against the shapes' own boxes: "which shape's box does the ray enter first?" / "is anything in the
 * way before tmax?" for trees without triangles (voxel worlds, box scenes, picking / visibility over sphere bounds).
 * Ray i comes with tmax[i] in the tree's dtype.  A NULL tmax means +inf for every ray.
 *  - L_i is the list FlatBvh::traverse(&ray_i, shapes) returns (flat_bvh.rs:396-431), in its order.  This is the engine's CSR row.
 *  - For s in L_i, (enter_s, exit_s) is Ray::intersection_slice_for_aabb (ray_impl.rs:118-145) on shape s's AABB as the tree holds it.  These
 *    are the same values BVHGPU_TRAVERSE_T_SLICE returns for that hit.
 *  - The slab test and the slice share one condition (!nan && tmx >= max(tmn, 0)).  So the slice is Some for every member of L_i.
 *  - enter_s is never NaN, never negative and never -0.  max(tmn, 0) returns +0.
 * A shape s is a candidate iff enter_s < tmax[i].  The comparison is strict and done in T.  So a NaN, zero or negative tmax admits nothing,
 * and tmax == enter_s does not admit s.
 *  - closest (default): the candidate with the smallest enter_s.  On equal enter_s the first one in L_i order wins.
 *  - first (BVHGPU_TRAVERSE_FIRST, any-hit): the first candidate in L_i order.  Every walk may stop at it.
 * Per ray the result is {enter, exit} (2 T) and the shape index.  With no candidate it is {+inf, 0} and BVHGPU_NONE.  bvhgpu_hits_info's
 * `total` is the number of rays with a candidate.  No triangles are needed or read.  The definition holds for every tree the CSR walks
 * accept: built here, refitted, imported / broadcast, an uploaded FlatBvh whose shapes moved (leaf tests use the shape AABBs), trees with
 * empty child bounds (a split without SAH winner).
 * `rays` and `tmax` live in `mem` (HOST tmax is staged into the result object).  `flags`: BVHGPU_TRAVERSE_COHERENT (a hint) and
 * BVHGPU_TRAVERSE_FIRST; every other bit → BVHGPU_INVALID_ARG.  Tree not flattened → BVHGPU_NOT_FLATTENED; another dtype than the tree's →
 * BVHGPU_DTYPE_MISMATCH; n_rays = 0 and an empty tree are fine.  Synchronises like bvhgpu_traverse_any_*.  _fetch / _fetch_triangles /
 * _fetch_closest / _fetch_any / _device return BVHGPU_INVALID_ARG on such a result, and bvhgpu_hits_fetch_box on any other.
 * bvhgpu_hits_fetch_box: per ray {enter, exit} (n x 2 T) and the shape (n u32); either may be NULL. */
int bvhgpu_traverse_box_f32(bvhgpu_tree *tree, const bvhgpu_ray_f32 *rays, const float *tmax, size_t n_rays, int mem, unsigned flags,
                            bvhgpu_hits **hits);
int bvhgpu_traverse_box_f64(bvhgpu_tree *tree, const bvhgpu_ray_f64 *rays, const double *tmax, size_t n_rays, int mem, unsigned flags,
                            bvhgpu_hits **hits);
int bvhgpu_hits_fetch_box(bvhgpu_hits *hits, void *slice, uint32_t *shape, int mem);

/* ---- closest-hit and any-hit ray queries against sphere shapes: "which sphere does this ray hit first?" / "is anything in the way before
 * tmax?" for particles, atoms, splats, bounding spheres — the fused form of the reference's first example (examples/simple.rs: build from the
 * spheres' AABBs, traverse, then a ray-sphere test over the returned list on the host).
 * Shape s has a sphere {c[3], r} in the tree's dtype T, set with bvhgpu_tree_set_spheres_*.  The sphere is independent of the AABB the tree
 * was built from.  The caller normally builds from c -/+ r, as simple.rs does.
 * Ray i has tmax[i] in T.  A NULL tmax means +inf for every ray.  L_i is the list FlatBvh::traverse(&ray_i, shapes) returns, in its order.
 * That is the engine's CSR row.
 * For s in L_i, with the ray's o and d as the Ray record holds them, the leaf stage is the following.  Every operation is rounded once in T,
 * with no contraction.  dot3 is (a0*b0 + a1*b1) + a2*b2.
 *     f[k] = o[k] - c[k]
 *     a    = dot3(d, d)
 *     tc   = (-dot3(f, d)) / a              parameter of the ray's point nearest the centre
 *     l[k] = f[k] + tc * d[k]               centre -> that point
 *     disc = r*r - dot3(l, l)
 *     if !(disc >= 0): miss
 *     h  = sqrt(disc / a)
 *     t0 = tc - h ;  t1 = tc + h
 *     t  = (t0 > eps) ? t0 : t1             eps = T::epsilon(), the triangle stage's bound
 *     hit iff t > eps  ->  {distance = t, exit = t1};   miss -> {+inf, 0}
 *  - Why the geometric form.  It is chosen over b*b - a*c because that form loses r*r against |f|^2 in f32 for distant origins.
 *  - What follows from the arithmetic.  Nothing else is special-cased.  A NaN centre, radius or direction misses.  r < 0 acts like |r|.  A
 *    zero direction misses.  An origin inside the sphere hits at t1.  A distance of +inf is never below any tmax.
 *  - Overflow.  Where r*r or disc / a overflows to +inf while dot3(l, l) stays finite (a huge radius or scene, a subnormal a), the stage hits
 *    with h = +inf, t0 = -inf and t1 = +inf: the record is {+inf, +inf}, a hit that no tmax admits.  Such a shape is never a candidate.  The
 *    ray's result is {+inf, 0} and BVHGPU_NONE if it has no other, and a multi-hit row never lists it.  Where both overflow, disc is NaN: a miss.
 *  - Candidate.  s is a candidate iff it hits and distance < tmax[i], strict and in T.  A NaN, zero or negative tmax admits nothing.
 *  - closest (default): the candidate with the smallest distance, and the first of L_i on equal distances.
 *  - first (BVHGPU_TRAVERSE_FIRST): the first candidate of L_i.  Every walk may stop there.
 *  - Result per ray.  {distance, exit} and the shape.  Without a candidate, {+inf, 0} and BVHGPU_NONE.  bvhgpu_hits_info's `total` is the
 *    number of rays with a candidate.
 *  - Sphere data is never validated.  NaN, infinite and negative radii follow the arithmetic.
 *  - Trees.  It holds for every tree the CSR walks accept: built here, refitted, an uploaded FlatBvh, imported, or with empty child bounds.
 *    Scene export and broadcast do not carry spheres.  A receiving tree has none until they are set.
 * bvhgpu_tree_set_spheres_*: `spheres` is n x 4 T {cx, cy, cz, r} in `mem`; the tree keeps its own HBM copy, beside any triangles.  n must
 * equal the tree's shape count (BVHGPU_INVALID_ARG); another dtype than the tree's is BVHGPU_DTYPE_MISMATCH.  A rebuild with a different
 * shape count drops the spheres, as it drops the triangles; refit does not touch them.
 * bvhgpu_traverse_sphere_*: `rays`, `tmax`, `flags` (BVHGPU_TRAVERSE_COHERENT, BVHGPU_TRAVERSE_FIRST) and the statuses are those of
 * bvhgpu_traverse_box_*; without spheres set, BVHGPU_INVALID_ARG ("... need bvhgpu_tree_set_spheres first").  _fetch / _fetch_triangles /
 * _fetch_closest / _fetch_any / _fetch_box / _device return BVHGPU_INVALID_ARG on such a result, and bvhgpu_hits_fetch_sphere on any other.
 * bvhgpu_hits_fetch_sphere: per ray {distance, exit} (n x 2 T) and the shape (n u32); either may be NULL. */
int bvhgpu_tree_set_spheres_f32(bvhgpu_tree *tree, const float *spheres /* n x 4: cx, cy, cz, r */, size_t n, int mem);
int bvhgpu_tree_set_spheres_f64(bvhgpu_tree *tree, const double *spheres /* n x 4: cx, cy, cz, r */, size_t n, int mem);
int bvhgpu_traverse_sphere_f32(bvhgpu_tree *tree, const bvhgpu_ray_f32 *rays, const float *tmax, size_t n_rays, int mem, unsigned flags,
                               bvhgpu_hits **hits);
int bvhgpu_traverse_sphere_f64(bvhgpu_tree *tree, const bvhgpu_ray_f64 *rays, const double *tmax, size_t n_rays, int mem, unsigned flags,
                               bvhgpu_hits **hits);
int bvhgpu_hits_fetch_sphere(bvhgpu_hits *hits, void *slice, uint32_t *shape, int mem);

/* ---- multi-hit ray queries: the k nearest hits of every ray, in order — transparency and depth peeling, absorption through particles or
 * splats, LiDAR multi-return, picking through a front surface, inside/outside parity — without fetching the whole CSR and reducing it on
 * the host.  The ray counterpart of bvhgpu_knearest_*.
 * Ray i has tmax[i] in the tree's dtype T.  A NULL tmax means +inf for every ray.  L_i is the list FlatBvh::traverse(&ray_i, shapes)
 * returns, in its order.  That is the engine's CSR row.
 * For s in L_i the leaf stage `leaf` gives a record of W scalars.  Its first scalar is the DISTANCE.
 *     BVHGPU_LEAF_BOX       {enter, exit}       W = 2   Ray::intersection_slice_for_aabb on s's AABB as the tree holds it: the bits
 *                                                       BVHGPU_TRAVERSE_T_SLICE returns.  Needs nothing.
 *     BVHGPU_LEAF_TRIANGLE  {distance, u, v}    W = 3   Ray::intersects_triangle's Intersection: the bits BVHGPU_TRAVERSE_TRIANGLES returns.
 *                                                       Needs bvhgpu_tree_set_triangles_*.
 *     BVHGPU_LEAF_SPHERE    {distance, exit}    W = 2   the sphere leaf stage of bvhgpu_traverse_sphere_* above.  Needs bvhgpu_tree_set_spheres_*.
 *  - Candidate.  s is a candidate iff distance < tmax[i], strict and in T.  A miss (+inf) is never a candidate.  A NaN, zero or negative
 *    tmax admits nothing.
 *  - Row i.  The candidates of L_i in a stable ascending sort by distance, cut to the first k.  Equal distances stay in the order of L_i.
 *    That order is not shape-index order.
 *  - Padding.  Slots beyond the number of candidates hold BVHGPU_NONE and {+inf, 0} / {+inf, 0, 0}, the existing no-candidate records.
 *  - Incremental form, which the kernel runs: bvhgpu_knearest_*'s list with the strict < of T.  While the list is not full every candidate
 *    enters.  A full list accepts d iff d < L[k-1] and drops L[k-1].  An accepted d goes in front of the first element e with d < e, else
 *    to the end.  A candidate's distance is never NaN (enter is max(tmin, 0); the triangle and sphere stages return +inf or a value > eps),
 *    so rows are always sorted.
 *  - Limits.  1 <= k <= BVHGPU_KHITS_MAX_K, else BVHGPU_INVALID_ARG.
 *  - Trees.  It holds for every tree the binary CSR walks accept: built here, refitted, an uploaded FlatBvh, scene-imported, trees with
 *    empty child bounds, one shape, and no shapes (every slot is padding).
 *  - No pruning.  The walk visits all of L_i, as BVHGPU_TRAVERSE_CLOSEST does.
 * out_shape[i*k + j] and out_vals[(i*k + j)*W ..] are slot j of row i.  `rays`, `tmax` and both outputs live in `mem`.  The call is
 * synchronous: the rows are complete when it returns.  Refused, touching no buffer: a NULL tree; a tree of another dtype
 * (BVHGPU_DTYPE_MISMATCH); a tree that is not flattened (BVHGPU_NOT_FLATTENED); k out of range, a NULL pointer with n_rays > 0, a `mem`
 * that is neither BVHGPU_HOST nor BVHGPU_DEVICE, an unknown `leaf`, triangles or spheres that were not set (BVHGPU_INVALID_ARG);
 * n_rays >= 2^32-1 or n_rays * k >= 2^32 (BVHGPU_OVERFLOW). */
#define BVHGPU_KHITS_MAX_K 64u /* the lists of a 64-lane workgroup live in LDS: 64 x 64 x (8 + 4) bytes = 48 KB in f64 */
#define BVHGPU_LEAF_BOX 0
#define BVHGPU_LEAF_TRIANGLE 1
#define BVHGPU_LEAF_SPHERE 2
int bvhgpu_traverse_khits_f32(bvhgpu_tree *tree, const bvhgpu_ray_f32 *rays, const float *tmax, size_t n_rays, int mem, int leaf, uint32_t k,
                              uint32_t *out_shape /* n x k */, float *out_vals /* n x k x W */);
int bvhgpu_traverse_khits_f64(bvhgpu_tree *tree, const bvhgpu_ray_f64 *rays, const double *tmax, size_t n_rays, int mem, int leaf, uint32_t k,
                              uint32_t *out_shape /* n x k */, double *out_vals /* n x k x W */);

/* ---- all-hits ray queries: EVERY hit of every ray, in order, as a CSR — absorption or transmittance through all particles along a ray,
 * order-independent transparency with an unknown layer count, inside/outside parity, LiDAR full-waveform returns, "exactly the triangles
 * this segment crosses" — without fetching the candidate CSR of bvhgpu_traverse_* and filtering and sorting it on the host.  The unbounded
 * form of bvhgpu_traverse_khits_* above.
 * Ray i has tmax[i] in the tree's dtype T.  A NULL tmax means +inf for every ray.  L_i is the list FlatBvh::traverse(&ray_i, shapes)
 * returns, in its order.  That is the engine's CSR row.
 * For s in L_i the leaf stage `leaf` gives a record of W scalars whose first scalar is the DISTANCE.  The leaf stage is exactly that of
 * bvhgpu_traverse_khits_*: BVHGPU_LEAF_BOX, BVHGPU_LEAF_TRIANGLE or BVHGPU_LEAF_SPHERE, the same device functions on the same operands,
 * so the bits are the same.
 *  - Candidate.  s is a candidate iff distance < tmax[i], strict and in T.  A miss (+inf) is never a candidate.  A NaN, zero or negative
 *    tmax admits nothing.
 *  - Row i, default.  All candidates of L_i in a stable ascending sort by distance.  Equal distances stay in the order of L_i.  A
 *    candidate's distance is never NaN, so the order is the total order on (distance, position in L_i): it is unique whatever algorithm
 *    produces it.
 *  - Row i with BVHGPU_ALLHITS_LIST_ORDER.  The candidates in the order of L_i, with no sort pass.
 *  - Output.  offsets[n_rays + 1] holds the exclusive prefix sums of the row lengths, as u32; offsets[n_rays] == total.  shape[total] holds
 *    the shape indices, as u32.  vals[total x W] holds the records.  There is no padding anywhere.
 *  - Consequence.  For every k, the first min(k, len) entries of a default row are row i of bvhgpu_traverse_khits_* in front of its padding.
 *  - Trees.  Every tree bvhgpu_traverse_khits_* accepts: built here, refitted, an uploaded FlatBvh, scene-imported, trees with empty
 *    child bounds, with one shape, and with no shapes (all offsets 0).
 *  - No pruning.  The walk visits all of L_i.
 *  - Limits.  n_rays < 2^32-1, else BVHGPU_OVERFLOW.  total <= 2^32-1, else BVHGPU_OVERFLOW: the total is summed in 64 bits and the
 *    status is returned after the count pass, before anything is sized by it; the result object then holds an empty all-hits result.
 * `rays` and `tmax` live in `mem`.  The call is synchronous: the result object is complete on return.  *hits may be NULL or an earlier
 * result object of any kind, whose buffers are then reused.  bvhgpu_hits_info gives n_rays and total, the number of candidates;
 * stats.hits == total and the other stats are 0.  bvhgpu_hits_wait returns BVHGPU_OK, bvhgpu_hits_walk_info gives 0,
 * bvhgpu_hits_walk_kernel names the fill kernel.  _fetch / _fetch_triangles / _fetch_closest / _fetch_any / _fetch_box / _fetch_sphere /
 * _fetch_within / _device return BVHGPU_INVALID_ARG on such a result, and bvhgpu_hits_fetch_allhits on any other.
 * Refused, touching no buffer and leaving *hits as it was, in this order: a NULL tree or a NULL `hits`; what the settle of the tree's
 * asynchronous build returns; a result object that still holds an asynchronous batch; a tree of another dtype (BVHGPU_DTYPE_MISMATCH);
 * a tree that is not flattened (BVHGPU_NOT_FLATTENED); a NULL `rays` with n_rays > 0, a `mem` that is neither BVHGPU_HOST nor
 * BVHGPU_DEVICE, an unknown `leaf`, a flag bit other than BVHGPU_ALLHITS_LIST_ORDER, triangles or spheres that were not set
 * (BVHGPU_INVALID_ARG); n_rays >= 2^32-1 (BVHGPU_OVERFLOW).
 * bvhgpu_hits_fetch_allhits: offsets (n_rays + 1 u32), shape (total u32) and vals (total x W T) copied to `mem`; each may be NULL. */
#define BVHGPU_ALLHITS_LIST_ORDER 1u /* rows in the order of FlatBvh::traverse's list instead of ascending distance */
int bvhgpu_traverse_allhits_f32(bvhgpu_tree *tree, const bvhgpu_ray_f32 *rays, const float *tmax, size_t n_rays, int mem, int leaf, unsigned flags,
                                bvhgpu_hits **hits);
int bvhgpu_traverse_allhits_f64(bvhgpu_tree *tree, const bvhgpu_ray_f64 *rays, const double *tmax, size_t n_rays, int mem, int leaf, unsigned flags,
                                bvhgpu_hits **hits);
int bvhgpu_hits_fetch_allhits(bvhgpu_hits *hits, uint32_t *offsets, uint32_t *shape, void *vals, int mem);

/* ---- radius search: EVERY shape within max_dist of every query point, in order, as a CSR — normals and density estimation on point
 * clouds, DBSCAN, contact candidates with real triangle distances, "everything within r of this probe" — without cutting rows at
 * BVHGPU_KNN_MAX_K and without fetching the ball query's CSR and computing, filtering and sorting distances on the host.  The unbounded
 * form of bvhgpu_knearest_tree_*'s max_dist.
 * Definition: the loop of nearest_to over the FlatNode array (flat_bvh.rs:524-558) with the moving `best_dist` replaced by a fixed limit.
 * Point p_i has m = max_dist[i] in the tree's dtype T; r2 = m * m is one multiplication in T.  A negative or NaN m gives an empty row
 * without a walk.
 *   i = 0
 *   while i < len(flat):
 *     non-leaf entry: md = aabb.min_distance_squared(p);  i = (md <= r2) ? entry_index : exit_index
 *     leaf entry:     d  = shape.distance_squared(p);     if d <= r2: candidate (d, shape);  i = exit_index
 *  - shape.distance_squared is `kind` 0, the shape's own Aabb::min_distance_squared, or `kind` 1, the triangle (needs
 *    bvhgpu_tree_set_triangles): the device functions of bvhgpu_knearest_*, so the bits are the same.  Every comparison is T's <= as
 *    written, so the limit itself is inside.  m = 0 keeps the shapes at distance 0.  m = +inf keeps every shape whose distance is not NaN.
 *    A NaN d is never a candidate, so a candidate's key is never NaN and the sorted order below is a total order.
 *  - NaN and infinite point coordinates.  Aabb::min_distance_squared ends every axis with max(0), which turns NaN into 0: a NaN
 *    coordinate adds 0 on its axis to every box distance (an all-NaN point is at distance 0 of every box).  An infinite coordinate gives
 *    +inf against a finite box, which only m = +inf admits.  The triangle distance has no such guard: such points give it NaN or +inf.
 *  - Row i, default.  All candidates in a stable ascending sort by d.  Equal d stay in the order the loop met them (leaf pre-order).  The
 *    output distance is sqrt(d), as in the k-nearest rows.
 *  - Row i with BVHGPU_WITHIN_LIST_ORDER.  The candidates in the order the loop met them, with no sort pass.  Where every operation is
 *    exact, kind 0 gives exactly the shapes and order of bvhgpu_query_*'s BVHGPU_QUERY_BALL row.
 *  - BVHGPU_WITHIN_COUNT_ONLY.  Only `offsets` is produced (neighbour counts); `total` is still reported; shape and dist are empty.
 *  - Walk-independence.  The threshold never moves, so the candidate set is "every box on the shape's path passes md <= r2 and the shape
 *    passes d <= r2", whatever order a walk visits nodes in.  The boxes of the non-leaf entries are the child boxes of the BvhNode array,
 *    so for a row no longer than k, bvhgpu_knearest_tree_*(k, max_dist) holds the same candidates with bit-equal distances; only the order
 *    inside a group of equal distances may differ.
 *  - Output.  offsets[n + 1] holds the exclusive prefix sums of the row lengths, as u32; offsets[n] == total.  shape[total] holds the
 *    shape indices, as u32.  dist[total] holds the distances, as T.  There is no padding anywhere.
 *  - Trees.  Every tree bvhgpu_knearest_* accepts: built here, refitted, an uploaded FlatBvh, scene-imported, trees with empty child
 *    bounds, one shape, and no shapes (all offsets 0).  One caveat: a tree whose build had a split without SAH winner (empty child
 *    bounds) and that arrived by scene import or broadcast carries the folded traversal array only, in which a leaf's navigator box —
 *    empty below such a split, at distance 0 of every point — is replaced by the shape's own box.  With kind 0 the rows are the
 *    definition's all the same.  With kind 1 a row can lack a triangle whose distance is within the limit while its box's distance,
 *    by rounding, is not (a query on a triangle vertex with max_dist 0).  Trees built, rebuilt or refitted here and uploaded FlatBvhs
 *    have no such case.
 *  - Limits.  n < 2^32 - 1 and total <= 2^32 - 1, else BVHGPU_OVERFLOW.  The total is summed in 64 bits and checked before anything is
 *    sized by it.
 * The call is synchronous: the result object is complete on return, for BVHGPU_HOST and BVHGPU_DEVICE points alike (`mem` applies to
 * `points` and `max_dist`).  *hits may be NULL or a result object of any kind, whose buffers are then reused.  bvhgpu_hits_info gives n
 * and total; stats.hits == total and the other stats are 0.  bvhgpu_hits_wait returns BVHGPU_OK, bvhgpu_hits_walk_info gives 0,
 * bvhgpu_hits_walk_kernel names the fill kernel (the count kernel of a COUNT_ONLY batch).  _fetch / _fetch_triangles / _fetch_closest /
 * _fetch_any / _fetch_box / _fetch_sphere / _fetch_allhits / _device return BVHGPU_INVALID_ARG on such a result, and
 * bvhgpu_hits_fetch_within on any other.
 * Refused, touching no buffer and leaving *hits as it was, in this order: a NULL tree or a NULL `hits`; what the settle of the tree's
 * asynchronous build returns; a result object that still holds an asynchronous batch; a tree of another dtype (BVHGPU_DTYPE_MISMATCH);
 * a tree that is not flattened (BVHGPU_NOT_FLATTENED); a NULL `points` or a NULL `max_dist` with n > 0, a `mem` that is neither
 * BVHGPU_HOST nor BVHGPU_DEVICE, a `kind` other than 0 / 1, a flag bit other than the two below, triangles that were not set for kind 1
 * (BVHGPU_INVALID_ARG); n >= 2^32-1 (BVHGPU_OVERFLOW).
 * bvhgpu_hits_fetch_within: offsets (n + 1 u32), shape (total u32) and dist (total T) copied to `mem`; each may be NULL. */
#define BVHGPU_WITHIN_LIST_ORDER 1u /* rows in the order the loop met the candidates instead of ascending distance */
#define BVHGPU_WITHIN_COUNT_ONLY 2u /* offsets (neighbour counts) and the total only */
int bvhgpu_within_f32(bvhgpu_tree *tree, const float *points, const float *max_dist, size_t n, int mem, int kind, unsigned flags,
                      bvhgpu_hits **hits);
int bvhgpu_within_f64(bvhgpu_tree *tree, const double *points, const double *max_dist, size_t n, int mem, int kind, unsigned flags,
                      bvhgpu_hits **hits);
int bvhgpu_hits_fetch_within(bvhgpu_hits *hits, uint32_t *offsets, uint32_t *shape, void *dist, int mem);

/* ---- the point families against sphere shapes (ABI 7): the k nearest spheres of a point, and every sphere within max_dist of it.  A
 * tree can carry one sphere {cx, cy, cz, r} per shape (bvhgpu_tree_set_spheres_*); these six entries are bvhgpu_knearest_*,
 * bvhgpu_knearest_tree_* and bvhgpu_within_* word for word — the loop, the list, the strict comparisons, the NaN rules, the rows, the
 * padding (BVHGPU_NONE, +inf), max_dist, the flags, the result object (of the within kind: bvhgpu_hits_fetch_within fetches it), the
 * trees each accepts, the argument rules and their order — with one change: shape.distance_squared(p) at a leaf is the squared
 * distance from p to the SOLID BALL, and there is no `kind` argument.
 *   f[k] = p[k] - c[k]           k = 0, 1, 2
 *   s2   = f[0]*f[0] + f[1]*f[1];  s2 = s2 + f[2]*f[2]       (three products, two sums, in this order)
 *   len  = sqrt(s2)              correctly rounded
 *   g    = len - r
 *   q    = (g < 0) ? 0 : g       a point inside or on the ball is at distance 0; NaN stays NaN
 *   d    = q * q
 * Every operation is rounded once in T, in the order written, no contraction.  Lists and thresholds hold d; output distances are
 * sqrt(d), as for kinds 0 and 1.  Deliberate consequences:
 *  - A NaN in the sphere or the point gives d = NaN — not 0, unlike the box distance, whose max(0) turns NaN into 0.  The families' NaN
 *    rules apply: never a candidate of within; accepted by the k-nearest forms only while the list is not full.
 *  - r is taken literally and never validated, as bvhgpu_tree_set_spheres_* says: a negative r adds |r| to the distance; r = +inf gives
 *    0 unless len is +inf too, which gives NaN.  An s2 that overflows gives d = +inf.
 *  - Nodes are still pruned by their BOXES, exactly as the reference prunes any PointDistance shape by its Aabb: a subtree is entered
 *    by the box rule of the unsuffixed entry.  A sphere that reaches outside its shape's box can therefore be pruned, as the ray entries
 *    can miss it.  Rows are "the k nearest spheres" / "all spheres within max_dist" in the geometric sense where every sphere lies inside
 *    its shape's box (boxes {c - r, c + r}, as the Python layer's spheres_aabbs makes them); in every case they are what the loop above produces.
 *  - The sphere distance is not the box distance, so the array that is walked is chosen by kind 1's rule (bvhgpu_within_*, "Trees"):
 *    the caveat about scene-imported trees with empty child bounds applies as for kind 1.
 * Refused with BVHGPU_INVALID_ARG at the place the unsuffixed entry checks its kind's array: a tree without spheres (before the first
 * bvhgpu_tree_set_spheres_*, or after a rebuild to another shape count dropped them).  The unsuffixed entries keep refusing kind 2. */
int bvhgpu_knearest_sphere_f32(bvhgpu_tree *tree, const float *points, size_t n, int mem, uint32_t k,
                               uint32_t *out_shape /* n x k */, float *out_dist /* n x k */);
int bvhgpu_knearest_sphere_f64(bvhgpu_tree *tree, const double *points, size_t n, int mem, uint32_t k,
                               uint32_t *out_shape /* n x k */, double *out_dist /* n x k */);
int bvhgpu_knearest_tree_sphere_f32(bvhgpu_tree *tree, const float *points, size_t n, int mem, uint32_t k,
                                    const float *max_dist /* NULL, or n values in the points' memory space */,
                                    uint32_t *out_shape /* n x k */, float *out_dist /* n x k */);
int bvhgpu_knearest_tree_sphere_f64(bvhgpu_tree *tree, const double *points, size_t n, int mem, uint32_t k,
                                    const double *max_dist /* NULL, or n values in the points' memory space */,
                                    uint32_t *out_shape /* n x k */, double *out_dist /* n x k */);
int bvhgpu_within_sphere_f32(bvhgpu_tree *tree, const float *points, const float *max_dist, size_t n, int mem, unsigned flags,
                             bvhgpu_hits **hits);
int bvhgpu_within_sphere_f64(bvhgpu_tree *tree, const double *points, const double *max_dist, size_t n, int mem, unsigned flags,
                             bvhgpu_hits **hits);

/* ---- convex regions (plane sets): EVERY shape whose box passes a set of planes, per region, in list order, as a CSR — view-frustum
 * culling, shadow-cascade slabs, a light's froxel, portals, selection prisms: "which shapes can this camera see".  Every operation below
 * is rounded once in the tree's dtype T, in the order written, with no contraction.
 *  - Batch.  n regions of m planes each, 0 <= m <= BVHGPU_REGION_MAX_PLANES, m uniform per batch.  `planes` is n x m x 4 T: (nx, ny, nz, d).
 *    A point x is inside a plane when n.x + d >= 0: normals point inward and need not be normalised.  Nothing is validated.
 *  - Test of a region against a box [lo, hi], for each plane in order:
 *        p[k] = (n[k] >= 0) ? hi[k] : lo[k]      the corner farthest along the normal; -0 takes hi, a NaN component takes lo
 *        s    = ((n0*p0 + n1*p1) + n2*p2) + d
 *    The box passes iff s >= 0 holds for every plane; a NaN s is a miss.  m = 0 passes every box.  A padding plane (0, 0, 0, 0) passes
 *    every box that has no infinite or NaN coordinate: that is how a caller mixes plane counts in one batch.  The test is the
 *    conservative corner test of every culling system: it never loses a shape that touches the region, and it may keep one near an
 *    edge of the region that does not; the caller refines where that matters.
 *  - Row q is FlatBvh::traverse (flat_bvh.rs:396-431) with that test in place of intersects_aabb: an inner entry tests its box and goes
 *    to entry_index on a pass and to exit_index otherwise; a leaf entry tests the shape's own AABB and reports the shape on a pass.
 *    Rows are in that (pre-order) order, as a CSR without padding.
 *  - BVHGPU_REGION_COUNT_ONLY: `offsets` and the total only.
 *  - BVHGPU_REGION_CLASSIFY: also one byte per reported shape, 1 iff the shape's AABB lies wholly inside — the same sums with the
 *    opposite corner, p'[k] = (n[k] >= 0) ? lo[k] : hi[k], give s' >= 0 for every plane — else 0.  A renderer skips finer tests for the 1s.
 *    (Ignored together with COUNT_ONLY.)
 *  - Fact 1.  On a tree whose inner boxes are exact joins (built or refitted here, no empty child bounds) the test is monotone in
 *    floating point: p of a child is <= (for a negative normal component >=) p of its parent, and products and sums round
 *    monotonically.  So the row equals "every shape whose own box passes, in leaf pre-order" — for inverted shape boxes too.
 *  - Fact 2.  On a tree with empty child bounds (a split without SAH winner) the empty box gives -inf or NaN and is never entered (for
 *    m > 0): the walk defines the row, not the brute-force set.
 *  - Output.  offsets[n + 1]: exclusive prefix sums of the row lengths, u32, offsets[n] == total.  shape[total]: u32.  inside[total]:
 *    bytes (CLASSIFY).
 *  - Trees.  Built here, rebuilt, refitted, uploaded FlatBvhs, one shape, no shapes (all offsets 0), built trees with empty child
 *    bounds.  A tree with empty child bounds that arrived by scene import or broadcast carries the folded array only, which would report
 *    leaves the reference never reaches: BVHGPU_INVALID_ARG, as bvhgpu_query_* answers.
 *    An uploaded array must be a pre-order array whose subtrees nest: an inner entry i owns the range [i, exit_i), and the exit of every
 *    entry inside that range is at most exit_i.  bvhgpu_tree_from_flat checks entry == i + 1, exit > i and "at most two children", not the
 *    nesting: the other walks follow the pointers one entry at a time and give FlatBvh::traverse's row on any array, whereas this one
 *    skips to the largest exit of the entries that failed, which is the same row only where subtrees nest (every array FlatBvh::flatten
 *    writes does).  On an array that does not, the call still ends (a step never goes backwards) and its rows are unspecified.
 *  - Limits.  n < 2^32 - 1 and total <= 2^32 - 1, else BVHGPU_OVERFLOW (the total is summed in 64 bits before anything is sized by it).
 *  - Working memory, in the result object: one u32 per (region, chunk) unit twice over (counts and their scan), n x n_chunks < n + 8192
 *    units whatever the tree's size — about 8 (n + 8192) bytes, which grows with n and is not capped — and 260 bytes per chunk.
 * The call is synchronous: the result object is complete on return.  HOST planes are staged into the result object.  *hits may be NULL
 * or a result object of any kind, whose buffers are then reused.  bvhgpu_hits_info gives n and total; stats.hits == total.  The result is
 * a kind of its own: _fetch / _fetch_triangles / _fetch_closest / _fetch_any / _fetch_box / _fetch_sphere / _fetch_allhits / _fetch_within /
 * _device return BVHGPU_INVALID_ARG on it, and bvhgpu_hits_fetch_region on any other.
 * Refused, touching no buffer and leaving *hits as it was, in this order: a NULL tree or a NULL `hits`; what the settle of the tree's
 * asynchronous build returns; a result object that still holds an asynchronous batch; a tree of another dtype (BVHGPU_DTYPE_MISMATCH); a
 * tree that is not flattened (BVHGPU_NOT_FLATTENED); m > BVHGPU_REGION_MAX_PLANES, a NULL `planes` with n * m > 0, a `mem` that is
 * neither BVHGPU_HOST nor BVHGPU_DEVICE, a flag bit other than the two below, the imported tree above (BVHGPU_INVALID_ARG);
 * n >= 2^32 - 1 (BVHGPU_OVERFLOW).
 * bvhgpu_hits_fetch_region: offsets (n + 1 u32), shape (total u32) and inside (total bytes; NULL, or a CLASSIFY batch) copied to `mem`;
 * each may be NULL.  A COUNT_ONLY batch has offsets only.
 * bvhgpu_hits_region_info: how the batch was cut — a region is walked as n_chunks ranges of chunk_entries entries of the pre-order
 * array, one wavefront each (both 0 for a batch without regions or a tree without shapes).  The rows do not depend on it. */
#define BVHGPU_REGION_MAX_PLANES 32
#define BVHGPU_REGION_COUNT_ONLY 1u /* offsets and the total only */
#define BVHGPU_REGION_CLASSIFY 2u   /* one byte per reported shape: 1 = its AABB lies wholly inside the region */
int bvhgpu_region_f32(bvhgpu_tree *tree, const float *planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits **hits);
int bvhgpu_region_f64(bvhgpu_tree *tree, const double *planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits **hits);
int bvhgpu_hits_fetch_region(bvhgpu_hits *hits, uint32_t *offsets, uint32_t *shape, void *inside, int mem);
int bvhgpu_hits_region_info(const bvhgpu_hits *hits, uint32_t *n_chunks, uint32_t *chunk_entries);

/* ---- instanced scenes: closest-hit and first-hit ray queries over transformed copies of trees — many copies of one mesh (a forest, a
 * crowd) with the mesh built once, and rigid motion at the cost of rebuilding a tree over a few dozen object boxes while every object's own
 * tree stays untouched.  Every operation below is rounded once in the set's dtype T, in the order written, with no contraction (the
 * discipline of the triangle stage).
 *  - Instance set.  n_trees member trees and n instances.  A member is a bvhgpu_tree of the set's context and dtype, flattened, with
 *    triangles set.  Instance i is (tree_of[i], X_i).  X_i is 12 scalars, row-major 3x4 (m[k][j] = x[4k + j]), object -> world:
 *        w[k] = ((m[k][0]*p[0] + m[k][1]*p[1]) + m[k][2]*p[2]) + m[k][3]
 *  - Inverse Y_i (world -> object), computed on the device once per pose.  The nine cofactors are each a*b - c*d, two rounded products and
 *    one subtraction:
 *        C00 = m11*m22 - m12*m21    C01 = m12*m20 - m10*m22    C02 = m10*m21 - m11*m20
 *        C10 = m02*m21 - m01*m22    C11 = m00*m22 - m02*m20    C12 = m01*m20 - m00*m21
 *        C20 = m01*m12 - m02*m11    C21 = m02*m10 - m00*m12    C22 = m00*m11 - m01*m10
 *        det = (m00*C00 + m01*C01) + m02*C02        r = 1/det        y[k][j] = C[j][k] * r   (j, k < 3)
 *        y[k][3] = -(((y[k][0]*m03) + (y[k][1]*m13)) + y[k][2]*m23)
 *    Nothing is validated: a singular matrix follows the arithmetic.
 *  - Tree bounds B_t.  The component-wise min of the mins and max of the maxes over the member's shape AABBs as the tree holds them, with
 *    -0 below +0.  The reduction is exact and order-free for NaN-free boxes; a tree built here cannot hold a NaN box.  For an uploaded tree
 *    with a NaN box B_t is unspecified.
 *  - World box W_i.  The min and max (again -0 below +0) over the 8 corners of B_tree_of[i], each mapped by the forward formula; bit k of
 *    the corner number picks the max on axis k.
 *  - Top level.  The tree bvhgpu_build_flat_* builds over W_0 .. W_{n-1}.  The builder's input check therefore refuses a NaN or infinite
 *    world box with BVHGPU_INVALID_ARG (a NaN in a transform, a member without shapes).  n == 1 and n == 0 behave as they do for any tree.
 *  - Ray j with tmax[j] (NULL: +inf).  I_j = FlatBvh::traverse(ray_j, W) over the top level, in its order.  For each instance i in I_j the
 *    object-space ray r' is
 *        o'[k] = ((y[k][0]*o[0] + y[k][1]*o[1]) + y[k][2]*o[2]) + y[k][3]
 *        d'[k] = (y[k][0]*d[0] + y[k][1]*d[1]) + y[k][2]*d[2]                inv'[k] = 1/d'[k]
 *    d' is NOT renormalised, so the parameter of an object-space hit is the world ray's parameter and distances compare across instances.
 *    L' = FlatBvh::traverse(r', shapes of the member), in its order; for each s in L': isect = Ray::intersects_triangle(r', triangle s).
 *  - Closest (flags 0).  Among all (i, s) in that double order the candidates are those with isect.distance < tmax[j], strict and in T.  The
 *    winner is chosen by the rule BVHGPU_TRAVERSE_CLOSEST uses within one tree, carried across instances: strict <, the earlier candidate
 *    keeps a tie.
 *  - First (BVHGPU_TRAVERSE_FIRST).  The first (i, s) in that order with isect.distance < tmax[j].
 *  - Output per ray: {distance, u, v}, the instance index and the shape index within that instance's tree.  A miss is {+inf, 0, 0},
 *    BVHGPU_NONE, BVHGPU_NONE.
 *  - No pruning.  No inner node and no instance is skipped because of tmax or of the best distance so far.
 *  - Trees.  Every tree the binary walks accept as a member: built here, refitted, an uploaded FlatBvh, scene-imported, trees with empty
 *    child bounds, with one shape.
 * Memory.  `trees` is always a host array of handles.  In create / update `mem` covers `xforms` and `tree_of`; in trace it covers `rays`,
 * `tmax` and the three outputs.  Every call is synchronous.
 * Commit.  create and update both commit a pose: they read every member's arrays (completing a lazy flatten), counts and generation,
 * compute B_t, Y_i and W_i and rebuild the top level.  update is the re-pose AND the re-sync: call it after moving instances and after any
 * rebuild, refit or bvhgpu_tree_set_triangles of a member.  A commit that fails (a NaN or infinite world box) leaves the set uncommitted:
 * trace and boxes return BVHGPU_INVALID_ARG until an update succeeds; a failed create returns no set.  A refused update (the rules below)
 * changes nothing: the set keeps the pose it had.
 * Stale sets.  trace compares every member's current arrays, counts and generation with the committed ones and refuses with
 * BVHGPU_INVALID_ARG, "instances are stale: call bvhgpu_instances_update", when any differ — before anything is launched.  The check
 * cannot see a refit, which keeps both the arrays and the generation: after a refit without an update, trace answers over the new member
 * boxes inside the old world boxes.  The member trees must outlive every call on the set except bvhgpu_instances_destroy, which frees what
 * the set owns and never looks at a member.
 * Refused, touching no buffer, the first broken rule in this order: NULL arguments (ctx, out, the set, a needed array, a member);
 * a `mem` that is neither BVHGPU_HOST nor BVHGPU_DEVICE; a member, or the call, of another dtype than the set's (BVHGPU_DTYPE_MISMATCH);
 * a member of another context; what the settle of a member's asynchronous build returns; a member that is not flattened
 * (BVHGPU_NOT_FLATTENED); a member without triangles; n > (2^32-2)/3 (BVHGPU_OVERFLOW); tree_of[i] >= n_trees; in update, n other than the
 * set's n; in trace, a flag bit other than BVHGPU_TRAVERSE_FIRST, an uncommitted set, a stale set, n_rays >= 2^32-1 (BVHGPU_OVERFLOW).
 * Everything not marked is BVHGPU_INVALID_ARG.  n_rays == 0 is fine.  n == 0 is fine: every ray misses.
 * bvhgpu_instances_boxes: W_i of the committed pose, n x 6 T {min xyz, max xyz}, copied to `mem`. */
typedef struct bvhgpu_instances bvhgpu_instances;
int bvhgpu_instances_create_f32(bvhgpu_ctx *ctx, bvhgpu_tree *const *trees, size_t n_trees, const uint32_t *tree_of, const float *xforms, size_t n,
                                int mem, bvhgpu_instances **out);
int bvhgpu_instances_create_f64(bvhgpu_ctx *ctx, bvhgpu_tree *const *trees, size_t n_trees, const uint32_t *tree_of, const double *xforms, size_t n,
                                int mem, bvhgpu_instances **out);
int bvhgpu_instances_update_f32(bvhgpu_instances *s, const float *xforms, size_t n, int mem);
int bvhgpu_instances_update_f64(bvhgpu_instances *s, const double *xforms, size_t n, int mem);
int bvhgpu_instances_trace_f32(bvhgpu_instances *s, const bvhgpu_ray_f32 *rays, const float *tmax, size_t n_rays, int mem, unsigned flags,
                               float *out_vals /* n x 3 */, uint32_t *out_instance, uint32_t *out_shape);
int bvhgpu_instances_trace_f64(bvhgpu_instances *s, const bvhgpu_ray_f64 *rays, const double *tmax, size_t n_rays, int mem, unsigned flags,
                               double *out_vals /* n x 3 */, uint32_t *out_instance, uint32_t *out_shape);
int bvhgpu_instances_boxes(bvhgpu_instances *s, void *out, int mem);
int bvhgpu_instances_info(const bvhgpu_instances *s, int *dtype, size_t *n_trees, size_t *n_instances);
void bvhgpu_instances_destroy(bvhgpu_instances *s);

/* ---- instanced scenes of box and sphere shapes: a set has a LEAF KIND, fixed at creation, one of BVHGPU_LEAF_BOX, BVHGPU_LEAF_TRIANGLE
 * and BVHGPU_LEAF_SPHERE.  Every ray family of the set — bvhgpu_instances_trace_*, _khits_*, _allhits_* and their _masked_* forms — answers
 * with that kind's leaf stage.  bvhgpu_instances_create_* is bvhgpu_instances_create_leaf_* with BVHGPU_LEAF_TRIANGLE: for such a set every
 * byte is what it was.  Every operation below is rounded once in the set's dtype T, in the order written, with no contraction.
 *  - Everything up to and including the object-space ray r' = {Y o + y3, Y d, 1/(Y d)} is the block above, unchanged; so are the list
 *    L' = FlatBvh::traverse(r', shapes of the member) and the double order of the candidates (i, s).
 *  - The record of candidate (i, s), W scalars (3 for TRIANGLE, 2 otherwise), its first scalar the DISTANCE:
 *      BVHGPU_LEAF_BOX       {enter, exit} of Ray::intersection_slice_for_aabb for r' on shape s's own AABB as the member holds it (its shape
 *                            array — not the node box of the walked array, which a folded array or a tree with empty child bounds does not
 *                            keep at the leaf); {+inf, 0} on a miss.
 *      BVHGPU_LEAF_SPHERE    the sphere stage of bvhgpu_traverse_sphere_* on r' and the member's sphere s: {distance, exit}.  It divides by
 *                            dot(d', d'), so it is exact for the direction that is not renormalised.
 *      BVHGPU_LEAF_TRIANGLE  {distance, u, v} of Ray::intersects_triangle(r', triangle s), as above.
 *    Because d' is not renormalised the two scalars of a BOX or SPHERE record are parameters of the WORLD ray.
 *  - Closest / first / tmax, the k nearest hits and all hits apply to the distance by the rules of the blocks that define them for
 *    triangles, word for word: strict <, the earlier candidate keeps a tie, tmax strict and in T.  A miss or a padding slot is
 *    {+inf, 0[, 0]}, BVHGPU_NONE, BVHGPU_NONE.  No pruning.
 *  - What is hit.  A sphere under an affine X_i is the ELLIPSOID X_i maps it to; a box is the PARALLELEPIPED X_i maps it to.  W_i stays the
 *    image of the join of the member's shape AABBs: a sphere that reaches outside its shape's box is not covered there, exactly as
 *    bvhgpu_traverse_sphere_* does not cover it on one tree.
 *  - Output widths.  out_vals of trace is n x W, of khits n x k x W; bvhgpu_hits_fetch_instances_allhits copies total x W.
 *  - Members.  TRIANGLE needs bvhgpu_tree_set_triangles_* on every member, SPHERE bvhgpu_tree_set_spheres_*, BOX neither.  An unknown `leaf`
 *    is BVHGPU_INVALID_ARG, tested before the member rules.  update applies the set's own kind's rule.
 *  - Stale sets.  The check watches the array the set's kind reads: a bvhgpu_tree_set_spheres_* that moves the buffer of a SPHERE set's
 *    member makes the set stale until an update, and so does a rebuild to another shape count (which drops the spheres: update is refused
 *    until they are set again).  A BOX set watches the boxes alone.
 *  - bvhgpu_instances_region_* reads boxes only and serves every set.  The point families (within, knearest, knearest_tree and their masked
 *    forms) measure triangle distance and refuse a BOX or SPHERE set with BVHGPU_INVALID_ARG, directly after the dtype rule.
 * bvhgpu_instances_leaf: the set's kind. */
int bvhgpu_instances_create_leaf_f32(bvhgpu_ctx *ctx, bvhgpu_tree *const *trees, size_t n_trees, const uint32_t *tree_of, const float *xforms,
                                     size_t n, int mem, int leaf, bvhgpu_instances **out);
int bvhgpu_instances_create_leaf_f64(bvhgpu_ctx *ctx, bvhgpu_tree *const *trees, size_t n_trees, const uint32_t *tree_of, const double *xforms,
                                     size_t n, int mem, int leaf, bvhgpu_instances **out);
int bvhgpu_instances_leaf(const bvhgpu_instances *s, int *leaf);

/* ---- convex regions over an instanced scene: per region every (instance, shape) whose box passes, as a CSR — "which instances, and which
 * shapes inside them, can this camera see", without flattening the scene.  Every operation below is rounded once in the set's dtype T, in
 * the order written, with no contraction.
 *  - Batch.  bvhgpu_region_*'s: n regions of m <= BVHGPU_REGION_MAX_PLANES WORLD-space planes (nx, ny, nz, d), `planes` is n x m x 4 T, with
 *    that entry's box test and its CLASSIFY test, unchanged.  The set is a committed bvhgpu_instances (X_i, W_i, the top level over W).
 *  - Candidates.  I_q is row q of bvhgpu_region_* over the top level with the world planes: the instances whose W_i passes, in the top
 *    level's list order.
 *  - Object-space planes of region q in instance i, per plane, from the FORWARD transform X_i = m[k][j] (a plane transforms by the
 *    transpose of the forward map, n.(M p + t) + d = (M^T n).p + (n.t + d): no inverse enters):
 *        n'[j] = ((m[0][j]*n[0] + m[1][j]*n[1]) + m[2][j]*n[2])          j = 0, 1, 2
 *        d'    = (((n[0]*m[0][3] + n[1]*m[1][3]) + n[2]*m[2][3]) + d)
 *    A padding plane (0, 0, 0, 0) stays a padding plane for a finite X_i.  Nothing is validated.
 *  - Row q.  For each i in I_q, in order: L' = row of bvhgpu_region_* over member tree_of[i] with the planes (n', d').  The row is the
 *    concatenation of (i, s) for s in L'.  An instance that passes at the top and reports no shape contributes nothing.  The box test is
 *    applied to the member's boxes in their own frame: conservative there, and tighter than a world-space box around a rotated shape.  The
 *    world-box test and the object-space tests are separate roundings; neither is asserted to imply the other: the composition is the
 *    definition.
 *  - BVHGPU_REGION_COUNT_ONLY, BVHGPU_REGION_CLASSIFY: as for bvhgpu_region_*; the byte of (i, s) is 1 iff the opposite corner of s's box
 *    passes every (n', d').
 *  - BVHGPU_REGION_INSTANCES_ONLY: the row is I_q itself — instance indices, no shapes ("which objects do I draw").  With CLASSIFY the byte
 *    is 1 iff W_i lies wholly inside the world planes.  bvhgpu_region_* refuses this bit.
 *  - No pruning and no shortcut.  An instance whose W_i lies wholly inside is still walked and tested shape by shape.
 *  - Members.  Served exactly where bvhgpu_region_* serves that tree: built, rebuilt and refitted trees, uploaded FlatBvhs, one-shape
 *    trees, built trees with empty child bounds.  A member with empty child bounds that arrived by scene import or broadcast:
 *    BVHGPU_INVALID_ARG from this call (not from create), unless BVHGPU_REGION_INSTANCES_ONLY is set, which reads no member.
 *  - n == 0 instances, n == 0 regions and m == 0 (every instance, every shape) behave as bvhgpu_region_* does; so do a set of one instance
 *    and a top level with empty child bounds (coincident world boxes).
 *  - Staleness and commits.  bvhgpu_instances_trace_*'s rules: an uncommitted or a stale set is refused before anything is launched; a
 *    refit of a member is invisible until bvhgpu_instances_update.
 *  - Limits.  n < 2^32 - 1, the number of (region, instance) pairs P <= 2^32 - 1, total <= 2^32 - 1, else BVHGPU_OVERFLOW; each is summed
 *    in 64 bits before anything is sized by it.
 *  - Output.  offsets[n + 1] u32, instance[total] u32, shape[total] u32 (absent with INSTANCES_ONLY), inside[total] bytes (CLASSIFY).
 *  - Working memory.  Stage 1 (the top level) runs into a result object the set owns.  Stage 2 walks (pair, chunk) units, one wavefront
 *    each: member t is cut into nc_t <= ceil(8192 / P) chunks, the units are P x max_t nc_t < P + 8192 whatever the members' sizes —
 *    one u32 per unit twice over, one u32 per pair, 260 bytes per chunk of every member, in the caller's result object.
 * The call is synchronous: the result object is complete on return.  HOST planes are staged into the result object.  *hits may be NULL
 * or a result object of any kind, whose buffers are then reused.  bvhgpu_hits_info gives n and total; stats.hits == total.  The result is
 * a kind of its own: every _fetch_* above and _device return BVHGPU_INVALID_ARG on it, bvhgpu_hits_fetch_region included, and
 * bvhgpu_hits_fetch_instances_region on any other, a bvhgpu_region_* result included.  bvhgpu_hits_region_info gives the chunks per pair
 * (the uniform stride max_t nc_t) and the largest member's chunk_entries; with INSTANCES_ONLY, the top level's.
 * Refused, touching no buffer and leaving *hits as it was, in this order: a NULL set or a NULL `hits`; a result object that still holds
 * an asynchronous batch; m > BVHGPU_REGION_MAX_PLANES; a NULL `planes` with n * m > 0; a `mem` that is neither BVHGPU_HOST nor
 * BVHGPU_DEVICE; a set of another dtype (BVHGPU_DTYPE_MISMATCH); a flag bit other than the three; an uncommitted set; a stale set; the
 * imported member above; n >= 2^32 - 1 (BVHGPU_OVERFLOW).  Everything not marked is BVHGPU_INVALID_ARG.
 * bvhgpu_hits_fetch_instances_region: offsets (n + 1 u32), instance and shape (total u32 each) and inside (total bytes; NULL, or a
 * CLASSIFY batch) copied to `mem`; each may be NULL; `shape` must be NULL for an INSTANCES_ONLY batch.  A COUNT_ONLY batch has offsets only. */
#define BVHGPU_REGION_INSTANCES_ONLY 4u /* bvhgpu_instances_region_*: rows of instances, no shapes */
int bvhgpu_instances_region_f32(bvhgpu_instances *s, const float *planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits **hits);
int bvhgpu_instances_region_f64(bvhgpu_instances *s, const double *planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits **hits);
int bvhgpu_hits_fetch_instances_region(bvhgpu_hits *hits, uint32_t *offsets, uint32_t *instance, uint32_t *shape, void *inside, int mem);

/* ---- all hits over an instanced scene: per ray every (instance, shape) its segment crosses, in order, as a CSR — transmittance through
 * all surfaces, order-independent transparency, inside/outside parity, full-waveform returns, without flattening the scene.
 * Everything of bvhgpu_instances_trace_* stands unchanged: the committed set, Y_i, the object-space ray {Y o + y3, Y d, 1/(Y d)} (not
 * renormalised), the double order — the instances in the order of FlatBvh::traverse(ray, W) over the top level, within each instance the
 * shapes in the order of FlatBvh::traverse(r', member) — and isect = Ray::intersects_triangle(r', triangle s) per member of that list.
 * Every operation is rounded once in the set's dtype T, in the order written, with no contraction.
 *  - Candidate.  (i, s) is a candidate of ray j iff isect.distance < tmax[j], strict and in T.  A NULL tmax means +inf.  A miss (+inf) is
 *    never a candidate; a NaN distance fails the strict comparison, so it is never a candidate; a NaN, zero or negative tmax admits
 *    nothing.  So no key is ever NaN, and the sorted order below is a total order on (distance, position in the double order): it is
 *    unique whatever algorithm produces it.
 *  - Row j, default.  All candidates in a stable ascending sort by distance: equal distances stay in the double order.
 *  - Row j with BVHGPU_INSTANCES_ALLHITS_LIST_ORDER.  The candidates in the double order, with no sort pass.
 *  - BVHGPU_INSTANCES_ALLHITS_COUNT_ONLY.  `offsets` only (the hit counts per ray); `total` is still reported.  Nothing else is produced
 *    and the second walk does not run.
 *  - Output.  offsets[n_rays + 1] u32 exclusive prefix sums, offsets[n_rays] == total; instance[total] u32; shape[total] u32, the shape
 *    index within that instance's tree; vals[total x 3] T = {distance, u, v}, the distance in the world ray's parameter.  No padding.
 *  - Consequences.  A non-empty default row starts with exactly what bvhgpu_instances_trace_* (flags 0) returns for that ray: closest is
 *    strict < with the earlier candidate keeping a tie, which is the head of a stable sort.  A non-empty LIST_ORDER row starts with what
 *    BVHGPU_TRAVERSE_FIRST returns.  A row is empty iff bvhgpu_instances_trace_* reports a miss for the ray (it is not occluded).
 *  - No pruning.  Both walks visit the whole double order.
 *  - Members, n == 0 instances (every row is empty), one instance, a top level with empty child bounds (coincident world boxes): served
 *    exactly where bvhgpu_instances_trace_* serves them.  Staleness and commits: that entry's rules.
 *  - Limits.  n_rays < 2^32 - 1 and total <= 2^32 - 1, else BVHGPU_OVERFLOW; the total is summed in 64 bits and checked before anything is
 *    sized by it.  After such a refusal the result object holds an empty result of this kind.
 * The call is synchronous: the result object is complete on return.  `mem` covers `rays` and `tmax`; HOST rays are staged.  *hits may be
 * NULL or a result object of any kind, whose buffers are then reused.  bvhgpu_hits_info gives n_rays and total; stats.hits == total;
 * bvhgpu_hits_wait returns BVHGPU_OK; bvhgpu_hits_walk_kernel names the fill kernel, or the count kernel of a COUNT_ONLY batch.  The
 * result is a kind of its own: every _fetch_* above and _device return BVHGPU_INVALID_ARG on it, and
 * bvhgpu_hits_fetch_instances_allhits on any other.
 * Refused, touching no buffer and leaving *hits as it was, the first broken rule in this order: a NULL set or a NULL `hits`; a result
 * object that still holds an asynchronous batch; a NULL `rays` with n_rays > 0; a `mem` that is neither BVHGPU_HOST nor BVHGPU_DEVICE; a
 * set of another dtype (BVHGPU_DTYPE_MISMATCH); a flag bit other than the two; an uncommitted set; a stale set (the check and the message
 * of bvhgpu_instances_trace_*); n_rays >= 2^32 - 1 (BVHGPU_OVERFLOW).  Everything not marked is BVHGPU_INVALID_ARG.
 * bvhgpu_hits_fetch_instances_allhits: offsets (n_rays + 1 u32), instance and shape (total u32 each) and vals (total x 3 T) copied to
 * `mem`; each may be NULL.  A COUNT_ONLY batch has offsets only: a non-NULL instance, shape or vals is BVHGPU_INVALID_ARG. */
#define BVHGPU_INSTANCES_ALLHITS_LIST_ORDER 1u /* rows in the double order (top-level list, then member list) instead of sorted by distance */
#define BVHGPU_INSTANCES_ALLHITS_COUNT_ONLY 2u /* offsets (the hit counts) only: no instances, shapes or records */
int bvhgpu_instances_allhits_f32(bvhgpu_instances *s, const bvhgpu_ray_f32 *rays, const float *tmax, size_t n_rays, int mem, unsigned flags,
                                 bvhgpu_hits **hits);
int bvhgpu_instances_allhits_f64(bvhgpu_instances *s, const bvhgpu_ray_f64 *rays, const double *tmax, size_t n_rays, int mem, unsigned flags,
                                 bvhgpu_hits **hits);
int bvhgpu_hits_fetch_instances_allhits(bvhgpu_hits *hits, uint32_t *offsets, uint32_t *instance, uint32_t *shape, void *vals, int mem);

/* ---- radius search over an instanced scene: per query point every (instance, shape) whose WORLD-space triangle lies within max_dist of
 * it, in order, as a CSR — contact candidates, proximity and clearance checks, density estimation, snapping, without flattening the scene.
 * The set is the committed one of bvhgpu_instances_trace_*: X_i as uploaded, Y_i, the world boxes W_i and the top-level tree over W.
 * All arithmetic is in the set's dtype T; every operation is rounded once, in the order written, with no contraction.
 * Point p_j comes with m = max_dist[j]; r2 = m * m.  A negative or NaN m gives an empty row without a walk; -0.0 is the limit 0.
 *   top level: <FlatBvh as BoundingHierarchy>::nearest_to's loop with a fixed limit (bvhgpu_within_* above) over the top level's FlatNode
 *   array, with the world point:
 *     non-leaf entry: md = aabb.min_distance_squared(p);  entry_index iff md <= r2, else exit_index
 *     leaf entry (instance i): walk instance i, then exit_index
 *   instance i (member t = tree_of[i]):
 *     q[k] = ((Y_i[k][0]*p[0] + Y_i[k][1]*p[1]) + Y_i[k][2]*p[2]) + Y_i[k][3]                     the point in the object's frame
 *     f[k] = (Y_i[k][0]*Y_i[k][0] + Y_i[k][1]*Y_i[k][1]) + Y_i[k][2]*Y_i[k][2];  F = (f[0] + f[1]) + f[2]    ||Y_i's 3x3 part||_F squared
 *     r2o  = r2 * F                                                                                  the limit in the object's frame
 *     the same loop over member t's FlatNode array with q and r2o:
 *       non-leaf entry: md = aabb.min_distance_squared(q);  entry_index iff md <= r2o, else exit_index
 *       leaf entry (shape s): w[v][k] = ((X_i[k][0]*tri_s[v][0] + X_i[k][1]*tri_s[v][1]) + X_i[k][2]*tri_s[v][2]) + X_i[k][3], v = a, b, c:
 *                             the triangle in WORLD space;  d = <Triangle as PointDistance>::distance_squared(w, p);
 *                             (i, s) is a candidate with key d iff d <= r2;  then exit_index
 *  - The distance is the true world-space distance to the transformed triangle, meaningful under any affine X_i (distances do not
 *    survive a non-uniform scale, so nothing is measured in the object's frame).  There is no box kind: a box under an affine map is not
 *    a box, and the distance is a triangle's: a set created with BVHGPU_LEAF_BOX or BVHGPU_LEAF_SPHERE (bvhgpu_instances_create_leaf_*)
 *    is refused with BVHGPU_INVALID_ARG, directly after the dtype rule.
 *  - The prune is conservative.  |p - (X v + x3)| = |X (q - v)| >= |q - v| / ||Y||_F, so every point of a world triangle within m of p
 *    lies within m * ||Y||_F of q in the object's frame, and so does every box that contains it; W_i contains the world triangles.  In
 *    exact arithmetic row j is therefore exactly {(i, s) : d(i, s) <= r2}.  In floating point the row is what the loop above yields: a
 *    pair whose d lies within rounding of r2 may be decided by a box test, as for bvhgpu_within_*.  The threshold never moves, so the
 *    candidate set does not depend on the order of the walk.
 *  - Row j, default.  All candidates in a stable ascending sort by d; equal d stay in the order the loop met them: the double order, the
 *    instances in the top level's list order, within each the shapes in the member's.  No key is NaN (a NaN d fails <=), so the order
 *    is total and unique.
 *  - Row j with BVHGPU_INSTANCES_WITHIN_LIST_ORDER.  The candidates in the double order, with no sort pass.
 *  - BVHGPU_INSTANCES_WITHIN_COUNT_ONLY.  `offsets` only; `total` is still reported.  The second walk does not run.
 *  - Output.  offsets[n + 1] u32 exclusive prefix sums, offsets[n] == total; instance[total] u32; shape[total] u32, the shape index
 *    within that instance's tree; dist[total] T = sqrt(d).  No padding.
 *  - Edge cases.  m = +inf keeps every pair whose distance is not NaN.  A NaN r2o (0 * inf) passes no box test of that instance.  NaN
 *    and infinite points behave as bvhgpu_within_* describes for the box and the triangle distance.  Every walk terminates whatever
 *    the values: the index only moves forward.
 *  - Consequences.  An instance whose X is exactly the identity has Y = I and y3 = -0, so q = p and w = tri bit for bit, and F = 3: its
 *    entries of a LIST_ORDER row hold the distances of bvhgpu_within_* (kind 1, LIST_ORDER) on the member itself, bit-equal, and its
 *    shapes — identical wherever the single-tree prune (md <= r2) and this one (md <= 3 * r2) keep the same leaves.  A row is empty
 *    iff no pair passes.
 *  - Which arrays are walked: bvhgpu_instances_region_*'s rule, member by member, and the same rule for the top level (its build over
 *    the world boxes can meet a split without SAH winner too: its empty child boxes are at distance 0 of every point, as in the
 *    FlatNode array).  An imported member tree whose build had such a split is refused as there.
 *  - Limits.  n < 2^32 - 1 and total <= 2^32 - 1, else BVHGPU_OVERFLOW; the total is summed in 64 bits and checked before anything is
 *    sized by it.  After such a refusal the result object holds an empty result of this kind.
 * The call is synchronous: the result object is complete on return.  `mem` covers `points` and `max_dist`; HOST input is staged.  *hits
 * may be NULL or a result object of any kind, whose buffers are then reused.  bvhgpu_hits_info gives n and total; stats.hits == total;
 * bvhgpu_hits_wait returns BVHGPU_OK; bvhgpu_hits_walk_kernel names the fill kernel, or the count kernel of a COUNT_ONLY batch.  The
 * result is a kind of its own: every _fetch_* above and _device return BVHGPU_INVALID_ARG on it, and
 * bvhgpu_hits_fetch_instances_within on any other.
 * Refused, touching no buffer and leaving *hits as it was, the first broken rule in this order: a NULL set or a NULL `hits`; a result
 * object that still holds an asynchronous batch; a NULL `points` with n > 0; a NULL `max_dist` with n > 0; a `mem` that is neither
 * BVHGPU_HOST nor BVHGPU_DEVICE; a set of another dtype (BVHGPU_DTYPE_MISMATCH); a flag bit other than the two; an uncommitted set; a
 * stale set (the check and the message of bvhgpu_instances_trace_*); the imported member above; n >= 2^32 - 1 (BVHGPU_OVERFLOW).
 * Everything not marked is BVHGPU_INVALID_ARG.
 * bvhgpu_hits_fetch_instances_within: offsets (n + 1 u32), instance and shape (total u32 each) and dist (total T) copied to `mem`; each
 * may be NULL.  A COUNT_ONLY batch has offsets only: a non-NULL instance, shape or dist is BVHGPU_INVALID_ARG. */
#define BVHGPU_INSTANCES_WITHIN_LIST_ORDER 1u /* rows in the double order (top-level list, then member list) instead of sorted by distance */
#define BVHGPU_INSTANCES_WITHIN_COUNT_ONLY 2u /* offsets (the counts) only: no instances, shapes or distances */
int bvhgpu_instances_within_f32(bvhgpu_instances *s, const float *points, const float *max_dist, size_t n, int mem, unsigned flags, bvhgpu_hits **hits);
int bvhgpu_instances_within_f64(bvhgpu_instances *s, const double *points, const double *max_dist, size_t n, int mem, unsigned flags, bvhgpu_hits **hits);
int bvhgpu_hits_fetch_instances_within(bvhgpu_hits *hits, uint32_t *offsets, uint32_t *instance, uint32_t *shape, void *dist, int mem);

/* ---- k-nearest over an instanced scene: per query point the k (instance, shape) pairs whose WORLD-space triangles are nearest, ascending
 * — distance fields, proximity and contact, snapping, without flattening the scene and without guessing a radius for
 * bvhgpu_instances_within_*.  k = 1 is the reference's `nearest_to` over the scene.  The set is the committed one of
 * bvhgpu_instances_trace_*.  All arithmetic is in the set's dtype T; every operation is rounded once, in the order written.
 * Per point p a list L of at most k triples (d, instance, shape), ascending in d, the squared world distance in T.  full = len(L) == k,
 * bound = L[last].d.  Every comparison is the strict < of T.  Insertion is bvhgpu_knearest_*'s: a full list drops its last element, and
 * the new one goes in front of the first element e with d < e.d, else to the end.
 *   top level (the FlatNode array over the world boxes, with p):
 *     non-leaf entry: md = aabb.min_distance_squared(p);  entry_index iff !full || md < bound, else exit_index
 *     leaf entry (instance i): walk instance i, then exit_index
 *   instance i (member t = tree_of[i]), q[k] and F as for bvhgpu_instances_within_*:
 *     member t's FlatNode array with q:
 *       non-leaf entry: md = aabb.min_distance_squared(q);  entry_index iff !full || md < bound * F, else exit_index.  bound * F is ONE
 *                       multiplication in T, made again whenever `bound` changes and on entry to the instance
 *       leaf entry (shape s): w = the triangle in WORLD space and d = distance_squared(w, p) as for bvhgpu_instances_within_*;
 *                             accepted iff !full || d < bound;  then exit_index
 *  - Output row j, padded to k: out_instance[j*k + m], out_shape[j*k + m] and out_dist[j*k + m] = sqrt(L[m].d) for m < len(L); the other
 *    slots hold BVHGPU_NONE, BVHGPU_NONE and +inf.
 *  - The prune is conservative: |p - X v| >= |q - v| / ||Y||_F, so a member box with md >= bound * F holds no triangle with d < bound, and
 *    a world box with md >= bound holds none either.  Acceptance is strict, so what a prune skips could not have been accepted (in exact
 *    arithmetic; F exceeds the squared largest singular value of Y by the sum of the other two, which is the room rounding has for every
 *    non-singular transform).  A row therefore equals the list built by offering EVERY (instance, shape) pair in the double order — the
 *    instances in the top level's list order, within each the shapes in the member's — with no tree at all.
 *  - Order and ties.  Equal distances stay in the double order.  A candidate equal to `bound` of a full list is refused, so a tie at the
 *    k-th distance keeps the pairs met first.
 *  - NaN behaves as in bvhgpu_knearest_*: a NaN d is accepted only while the list is not full, as `bound` of a full list it is never
 *    replaced, and a NaN bound * F passes no box test.
 *  - A set without instances gives all padding.  n = 0 is fine (NULL buffers too).
 *  - Which arrays are walked: bvhgpu_instances_within_*'s rule; an imported member tree whose build had a split without SAH winner is
 *    refused as there.  The table of arrays and the mirrors belong to the set and are freed by bvhgpu_instances_destroy.
 *  - An identity instance of one tree gives that tree's own bvhgpu_knearest_* rows (kind 1): shapes and distances bit for bit.
 * `mem` covers all four buffers.  The call runs on the context's stream and returns when the rows are complete; there is no result object.
 * 1 <= k <= BVHGPU_INSTANCES_KNN_MAX_K: the lists of a workgroup live in LDS, k x (sizeof(T) + 8) bytes a lane — 64 lanes, k = 64 and f64 are
 * exactly the 64 KB a launch gets.
 * Refused, touching no buffer and leaving the set as it was, the first broken rule in this order: a NULL set; k = 0 or k >
 * BVHGPU_INSTANCES_KNN_MAX_K; a NULL buffer with n > 0; a `mem` that is neither BVHGPU_HOST nor BVHGPU_DEVICE; a set of another dtype
 * (BVHGPU_DTYPE_MISMATCH); an uncommitted set (the last update failed); a stale set (the check and the message of
 * bvhgpu_instances_trace_*: "instances are stale" — a member that lost its triangles is stale); the imported member above; n >= 2^32 - 1
 * or n * k >= 2^32 (BVHGPU_OVERFLOW).  Everything not marked is BVHGPU_INVALID_ARG. */
#define BVHGPU_INSTANCES_KNN_MAX_K 64u /* 64 lanes x 64 slots x (8 + 4 + 4) bytes = 64 KB of LDS in f64 */
int bvhgpu_instances_knearest_f32(bvhgpu_instances *s, const float *points, size_t n, int mem, uint32_t k,
                                  uint32_t *out_instance, uint32_t *out_shape, float *out_dist);
int bvhgpu_instances_knearest_f64(bvhgpu_instances *s, const double *points, size_t n, int mem, uint32_t k,
                                  uint32_t *out_instance, uint32_t *out_shape, double *out_dist);

/* ---- k-nearest point queries over an instanced scene, nearest child first and with a search radius: the "tree form" of
 * bvhgpu_instances_knearest_* (the "flat form"), as bvhgpu_knearest_tree_* is the tree form of bvhgpu_knearest_*.  The flat form walks
 * both levels in list order and prunes nothing until a list is full; this one descends the BvhNode arrays of the top level and of the
 * members nearest child first, so the first candidates a point meets are near ones, and it takes an optional limit per point.  The set is
 * the committed one of bvhgpu_instances_trace_*.  All arithmetic is in the set's dtype T; every operation is rounded once, in the order
 * written.
 * For one query point p, L is a list of at most k triples (d, instance, shape); d is the squared WORLD distance in T.  full = len(L) == k,
 * bound = L[last].d.  With a limit m = max_dist[j], r2 = m * m is one multiplication in T.  Insertion is bvhgpu_knearest_*'s: a full list
 * drops its last element; the new one goes in front of the first e with d < e.d, else at the end.  Every comparison is T's <, > or <= as
 * written; NaN behaves as in bvhgpu_knearest_* and bvhgpu_knearest_tree_*: a row that holds a NaN need not be sorted.
 *   cmd(box, x)   = 0 if box.min[0] > box.max[0]      (a child of a split without SAH winner carries Aabb::empty(): nothing is known below it)
 *                   else box.min_distance_squared(x)
 *   admit_w(x)    = (max_dist == NULL || (m >= 0 && x <= r2))     && (!full || x < bound)       a leaf's d, world frame
 *   admit_b(x, F) = (max_dist == NULL || (m >= 0 && x <= r2 * F)) && (!full || x < bound * F || bound * F == +inf)
 *                   a child box: F = 1 at the top level (world frame: the products are r2 and bound themselves), F of the instance the walk
 *                   is in below it (object frame).  A bound or a product that is +inf — a list that holds an infinite distance, or
 *                   bound * F overflowing — says nothing about a box whose own distance overflowed as well, so it prunes nothing
 *   top(node) over the BvhNode array of the top-level tree (the tree over the world boxes W), root = node 0, with p:
 *     Leaf{shape = i}:  enter instance i
 *     Node{l, l_aabb, r, r_aabb}:  c = [(l, cmd(l_aabb, p)), (r, cmd(r_aabb, p))];  if c[0].1 > c[1].1: swap   (strict >: ties and NaN keep left first)
 *                                  for (idx, cd) in c: if admit_b(cd, 1): top(idx)  (the second test sees the list as the first subtree left it)
 *   instance i (member t = tree_of[i]), bvhgpu_instances_knearest_*'s operation order:
 *     q[c] = row4(Y_i[c], p);   F = (row3(Y_i[0],Y_i[0]) + row3(Y_i[1],Y_i[1])) + row3(Y_i[2],Y_i[2])
 *     member(node) over member t's BvhNode array, root = node 0, with q:
 *       Leaf{shape = s}:  w[v][c] = row4(X_i[c], tri_s[v]);  d = triangle_dist2(w, p)   (world triangle, world point: the flat form's leaf)
 *                         if admit_w(d): insert (d, i, s)
 *       Node{...}:        as above with cmd(., q) and admit_b(., F)
 *  - r2 * F is ONE multiplication in T, made on entry to the instance.  bound * F is ONE multiplication in T, made on entry and whenever
 *    `bound` changes.
 *  - Output row j is the flat form's layout: out_instance[j*k + m], out_shape[j*k + m] and out_dist[j*k + m] = sqrt(L[m].d) for
 *    m < len(L); the other slots hold BVHGPU_NONE, BVHGPU_NONE and +inf.
 *  - A negative or NaN max_dist[j] gives a row of padding.  So do a set without instances and a member without shapes.  A limit of 0 keeps
 *    only distance 0.  max_dist is NULL (no limit) or n values in the points' memory space.  n = 0 is fine (NULL buffers too).
 *  - The prune is conservative by the flat form's argument, with <= for the radius: |p - X v| >= |q - v| / ||Y||_F, so a world triangle
 *    with d <= r2 lies within sqrt(r2 * F) of q, and one with d < bound within sqrt(bound * F).  Acceptance into a full list is strict, so
 *    what a prune skips could not have been accepted (in exact arithmetic).  Where bound * F overflows, admit_b's last clause switches the
 *    box test off instead of comparing inf < inf: at coordinates near sqrt(max of T) the rows are still the nearest-first lists.
 *  - Order and ties.  The order of a node's two children depends on the distances alone, never on the list.  Without prunes the walk
 *    therefore visits all (instance, shape) pairs in one fixed order per point, the NEAREST-FIRST ORDER, and a row is the list built by
 *    offering every pair in that order with no prune at all.  Ties stay in that order.  It is neither the flat form's double order nor
 *    leaf pre-order: the flat and the tree form may name different pairs at tied distances.  Their distances agree.
 *  - Members.  The descent reads the BvhNode array of every member, so every member must have been built here: an uploaded FlatBvh, an
 *    imported or a broadcast member is refused (bvhgpu_instances_knearest_* takes such members).  The per-member table belongs to the set
 *    and is freed by bvhgpu_instances_destroy.
 *  - An identity instance of one tree gives that tree's own bvhgpu_knearest_tree_* distances (kind 1) bit for bit, and its shapes wherever a
 *    row has no repeated distance (F = 3 there: the member's boxes are tested against wider limits, which may change the order ties are met in).
 * `mem` covers all five buffers.  The call runs on the context's stream and returns when the rows are complete; there is no result object.
 * 1 <= k <= BVHGPU_INSTANCES_KNN_MAX_K, the flat form's lists in LDS.
 * Refused, touching no buffer and leaving the set as it was, the first broken rule in this order: a NULL set; k = 0 or k >
 * BVHGPU_INSTANCES_KNN_MAX_K; a NULL points or output buffer with n > 0; a `mem` that is neither BVHGPU_HOST nor BVHGPU_DEVICE; a set of
 * another dtype (BVHGPU_DTYPE_MISMATCH); an uncommitted set; a stale set (the check and the message of bvhgpu_instances_trace_*:
 * "instances are stale"); a member that was not built here; n >= 2^32 - 1 or n * k >= 2^32 (BVHGPU_OVERFLOW).  Everything not marked is
 * BVHGPU_INVALID_ARG. */
int bvhgpu_instances_knearest_tree_f32(bvhgpu_instances *s, const float *points, size_t n, int mem, uint32_t k, const float *max_dist,
                                       uint32_t *out_instance, uint32_t *out_shape, float *out_dist);
int bvhgpu_instances_knearest_tree_f64(bvhgpu_instances *s, const double *points, size_t n, int mem, uint32_t k, const double *max_dist,
                                       uint32_t *out_instance, uint32_t *out_shape, double *out_dist);

/* ---- multi-hit ray queries over an instanced scene: the k nearest hits of every ray, in order, in fixed-width padded rows — depth
 * peeling, transparency with a known layer budget, LiDAR multi-return, picking through a front surface — without flattening the scene
 * and without fetching bvhgpu_instances_allhits_*'s whole CSR and cutting every row on the host.  bvhgpu_traverse_khits_* over the
 * committed set of bvhgpu_instances_trace_*.  All arithmetic is in the set's dtype T; every operation is rounded once, in the order written.
 *  - Candidates.  Ray j meets the pairs (instance, shape) in the double order of bvhgpu_instances_trace_*: the instances in the top level's
 *    list order, within each the shapes in the member's list order.  The record {distance, u, v} of a pair comes from the object-frame
 *    ray against the member's triangle, exactly as bvhgpu_instances_trace_* and bvhgpu_instances_allhits_* compute it.  A pair is a
 *    candidate iff distance < tmax[j], strict, in T.  A NULL tmax means +inf for every ray.  A miss (+inf), or a NaN, zero or negative
 *    tmax, admits nothing.
 *  - Row j.  The candidates in a stable ascending sort by distance, cut to the first k.  Equal distances stay in the double order; a tie
 *    at the k-th distance keeps the pairs met first.
 *  - Padding.  Slots beyond the number of candidates hold BVHGPU_NONE, BVHGPU_NONE and {+inf, 0, 0}.
 *  - Consequences.  Row j in front of its padding is the first min(k, len) entries of row j of bvhgpu_instances_allhits_* in its default
 *    (sorted) order, byte for byte.  At k = 1 the row is bvhgpu_instances_trace_*'s closest hit.  Over one identity instance the shape
 *    and vals columns equal bvhgpu_traverse_khits_* with BVHGPU_LEAF_TRIANGLE on the member.
 *  - Incremental form, which the kernel runs: bvhgpu_traverse_khits_*'s list with the strict < of T.  While the list is not full every
 *    candidate enters.  A full list accepts d iff d < L[k-1] and drops L[k-1].  An accepted d goes in front of the first element e with
 *    d < e, else to the end.  A candidate's distance is never NaN (it passed a strict <), so rows are always sorted.
 *  - No pruning.  The walk visits the whole double order, as trace and all-hits do.
 *  - A set without instances, or whose top level is empty, gives rows that are all padding.  n_rays = 0 is fine (NULL buffers too).
 * out_instance[j*k + m], out_shape[j*k + m] and out_vals[(j*k + m)*3 ..] are slot m of row j.  `mem` covers `rays`, `tmax` and the three
 * outputs; HOST input is staged.  The call runs on the context's stream and returns when the rows are complete; there is no result object.
 * 1 <= k <= BVHGPU_INSTANCES_KHITS_MAX_K: the lists of a workgroup live in LDS, k x (sizeof(T) + 8) bytes a lane.
 * Refused on the host before anything is launched, touching no buffer and leaving the set as it was, the first broken rule in this
 * order: a NULL set; k = 0 or k > BVHGPU_INSTANCES_KHITS_MAX_K; a NULL `rays` or output with n_rays > 0; a `mem` that is neither
 * BVHGPU_HOST nor BVHGPU_DEVICE; a set of another dtype (BVHGPU_DTYPE_MISMATCH); an uncommitted set; a stale set (the check and the
 * message of bvhgpu_instances_trace_*: "instances are stale"); n_rays >= 2^32 - 1 or n_rays * k >= 2^32 (BVHGPU_OVERFLOW).  Everything
 * not marked is BVHGPU_INVALID_ARG. */
#define BVHGPU_INSTANCES_KHITS_MAX_K 64u /* 64 lanes x 64 slots x (8 + 4 + 4) bytes = 64 KB of LDS in f64 */
int bvhgpu_instances_khits_f32(bvhgpu_instances *s, const bvhgpu_ray_f32 *rays, const float *tmax, size_t n_rays, int mem, uint32_t k,
                               uint32_t *out_instance /* n x k */, uint32_t *out_shape /* n x k */, float *out_vals /* n x k x 3 */);
int bvhgpu_instances_khits_f64(bvhgpu_instances *s, const bvhgpu_ray_f64 *rays, const double *tmax, size_t n_rays, int mem, uint32_t k,
                               uint32_t *out_instance /* n x k */, uint32_t *out_shape /* n x k */, double *out_vals /* n x k x 3 */);

/* ---- per-instance visibility masks for the ray queries over an instanced scene: shadow rays that must not see the emitter, picking rays
 * that see only selectable objects, one set serving several layers or LODs — without a set (a top level, an update per frame, an order of
 * ties) per ray type and without filtering an all-hits CSR after the member walks of every hidden instance have been paid for.
 *  - Every instance i of a set carries a 32-bit mask M[i].  A new set has M[i] = 0xFFFFFFFF for all i.
 *  - A masked ray batch carries one 32-bit mask R[j] per ray.  A NULL `ray_mask` means 0xFFFFFFFF for every ray.
 *  - Instance i is VISIBLE to ray j iff (M[i] & R[j]) != 0.
 *  - The answer of a masked entry is the answer of the same unmasked entry computed over bvhgpu_instances_trace_*'s candidate table with
 *    the rows of invisible instances removed.  That table is the double order: instances in the top level's list order, shapes in the
 *    member's list order.
 *  - Nothing else changes: the strict < against tmax; closest's strict < with the earlier candidate keeping a tie; first is the first
 *    surviving candidate; a k-hits row is the stable ascending sort of the survivors cut to k, padded with BVHGPU_NONE and {+inf, 0, 0};
 *    all-hits is sorted, list order or count only.
 *  - A surviving candidate's bits are unchanged.  Its object-space ray is computed from the world ray and Y_i alone.
 *  - The kernel skips an invisible instance at its top-level leaf.  It loads no record, re-expresses no ray and visits no member node.  The
 *    lane stays in the top level and goes on at i + 1.  A hidden instance costs one 4-byte load.
 *  - Still no pruning by distance.
 *  - Masks are not part of the pose: bvhgpu_instances_update_* keeps them; setting them needs no commit and leaves the top level untouched;
 *    setting them is allowed on a set whose last commit failed.
 *  - The existing entries keep ignoring masks, so every instance is visible to them: bvhgpu_instances_trace_*, _khits_*, _allhits_*, and
 *    the point and region families (_within_*, _knearest_*, _knearest_tree_*, _region_*).
 * bvhgpu_instances_set_masks: `masks` is n u32 in `mem`, or NULL for all ones again; n must equal the set's number of instances.
 * Synchronous: the masks are in place when it returns.  Refused with BVHGPU_INVALID_ARG, the set unchanged: a NULL set; a `mem` that is
 * neither BVHGPU_HOST nor BVHGPU_DEVICE; an n that differs from the set's.
 * bvhgpu_instances_masks: M, n u32, copied to `mem` (like bvhgpu_instances_boxes, but a set whose last commit failed answers too).
 * The masked entries: `ray_mask` is n_rays u32 in the rays' memory, or NULL; every other argument, the flags and the range of k are the
 * unmasked counterpart's.  Each makes the refusals of its counterpart, in the same order and with the same messages; a refused call
 * touches no buffer.  An all-hits-masked result has the kind bvhgpu_instances_allhits_* produces and is read by
 * bvhgpu_hits_fetch_instances_allhits. */
int bvhgpu_instances_set_masks(bvhgpu_instances *s, const uint32_t *masks, size_t n, int mem);
int bvhgpu_instances_masks(bvhgpu_instances *s, uint32_t *out, int mem);
int bvhgpu_instances_trace_masked_f32(bvhgpu_instances *s, const bvhgpu_ray_f32 *rays, const float *tmax, const uint32_t *ray_mask, size_t n_rays,
                                      int mem, unsigned flags, float *out_vals, uint32_t *out_instance, uint32_t *out_shape);
int bvhgpu_instances_trace_masked_f64(bvhgpu_instances *s, const bvhgpu_ray_f64 *rays, const double *tmax, const uint32_t *ray_mask, size_t n_rays,
                                      int mem, unsigned flags, double *out_vals, uint32_t *out_instance, uint32_t *out_shape);
int bvhgpu_instances_khits_masked_f32(bvhgpu_instances *s, const bvhgpu_ray_f32 *rays, const float *tmax, const uint32_t *ray_mask, size_t n_rays,
                                      int mem, uint32_t k, uint32_t *out_instance, uint32_t *out_shape, float *out_vals);
int bvhgpu_instances_khits_masked_f64(bvhgpu_instances *s, const bvhgpu_ray_f64 *rays, const double *tmax, const uint32_t *ray_mask, size_t n_rays,
                                      int mem, uint32_t k, uint32_t *out_instance, uint32_t *out_shape, double *out_vals);
int bvhgpu_instances_allhits_masked_f32(bvhgpu_instances *s, const bvhgpu_ray_f32 *rays, const float *tmax, const uint32_t *ray_mask, size_t n_rays,
                                        int mem, unsigned flags, bvhgpu_hits **hits);
int bvhgpu_instances_allhits_masked_f64(bvhgpu_instances *s, const bvhgpu_ray_f64 *rays, const double *tmax, const uint32_t *ray_mask, size_t n_rays,
                                        int mem, unsigned flags, bvhgpu_hits **hits);

/* ---- the same masks for the point and region queries over an instanced scene: the nearest selectable object, a proximity
 * query that must not see the querying object's own instance, collision layers, frustum culling with a camera's layer mask.
 *  - M[i] is the instance mask above: no new state; bvhgpu_instances_set_masks, _masks and _update_* are untouched.
 *  - A masked point batch carries one u32 P[j] per point, a masked region batch one u32 P[q] per region.  A NULL `point_mask` /
 *    `region_mask` means 0xFFFFFFFF for every row.  Instance i is VISIBLE to row j iff (M[i] & P[j]) != 0.
 *  - within: row j is bvhgpu_instances_within_*'s row with the pairs of invisible instances removed (the candidate set does not depend on the
 *    walk's order).  Sorted, LIST_ORDER and COUNT_ONLY as there; distances and the order of ties unchanged.
 *  - knearest: bvhgpu_instances_knearest_*'s incremental list (strict <, the earlier pair keeps a tie) over the double order with the rows of
 *    invisible instances removed; the bound that prunes comes from visible pairs only.  Row j is the first k of the stable ascending sort
 *    of all VISIBLE pairs, padded with BVHGPU_NONE / +inf.  (Filtering an unmasked row afterwards is not this: its k slots may be spent on
 *    hidden pairs.)
 *  - knearest_tree: bvhgpu_instances_knearest_tree_*'s descent over the SAME top-level BvhNode array — the top level of the whole set.  A
 *    top-level leaf whose instance is invisible contributes nothing and is left as a leaf whose member has no shapes is left.  Ties stay
 *    in this walk's order; max_dist and its special values as there.
 *  - region: I_q is the VISIBLE instances among those whose world box passes, in the top level's order; the object-space planes, the member
 *    rows and the CLASSIFY bytes of the survivors are unchanged.  With BVHGPU_REGION_INSTANCES_ONLY the row is that I_q, with CLASSIFY the
 *    surviving bytes.
 *  - A surviving pair's bits are unchanged: every operand of its test comes from the point or region and from X_i / Y_i alone.  No pruning
 *    beyond what each family already does.  A hidden instance costs one 4-byte load at its top-level leaf (region: per unit of its pair).
 *  - The unmasked entries keep ignoring masks.
 * `point_mask` is n u32 in the points' memory and `region_mask` n u32 in the planes' memory, or NULL; every other argument, the flags and
 * the range of k are the unmasked counterpart's.  Each entry makes the refusals of its counterpart, in the same order and with the same
 * messages; a refused call touches no buffer and leaves *hits as it was.  A result is of the counterpart's kind and is read by the
 * counterpart's fetch entries (bvhgpu_hits_fetch_instances_within, bvhgpu_hits_fetch_instances_region).  bvhgpu_hits_walk_kernel on a
 * masked within result names the masked fill (or count) kernel; on a masked region result it names the launch that looks at the masks —
 * the count walk k_instances_region_walk<T, false, false, true>, or k_instances_region_visible with BVHGPU_REGION_INSTANCES_ONLY — not the
 * kernel that writes the rows, which is the unmasked fill walk. */
int bvhgpu_instances_within_masked_f32(bvhgpu_instances *s, const float *points, const float *max_dist, const uint32_t *point_mask, size_t n, int mem,
                                       unsigned flags, bvhgpu_hits **hits);
int bvhgpu_instances_within_masked_f64(bvhgpu_instances *s, const double *points, const double *max_dist, const uint32_t *point_mask, size_t n, int mem,
                                       unsigned flags, bvhgpu_hits **hits);
int bvhgpu_instances_knearest_masked_f32(bvhgpu_instances *s, const float *points, const uint32_t *point_mask, size_t n, int mem, uint32_t k,
                                         uint32_t *out_instance /* n x k */, uint32_t *out_shape /* n x k */, float *out_dist /* n x k */);
int bvhgpu_instances_knearest_masked_f64(bvhgpu_instances *s, const double *points, const uint32_t *point_mask, size_t n, int mem, uint32_t k,
                                         uint32_t *out_instance /* n x k */, uint32_t *out_shape /* n x k */, double *out_dist /* n x k */);
int bvhgpu_instances_knearest_tree_masked_f32(bvhgpu_instances *s, const float *points, const uint32_t *point_mask, size_t n, int mem, uint32_t k,
                                              const float *max_dist, uint32_t *out_instance, uint32_t *out_shape, float *out_dist);
int bvhgpu_instances_knearest_tree_masked_f64(bvhgpu_instances *s, const double *points, const uint32_t *point_mask, size_t n, int mem, uint32_t k,
                                              const double *max_dist, uint32_t *out_instance, uint32_t *out_shape, double *out_dist);
int bvhgpu_instances_region_masked_f32(bvhgpu_instances *s, const float *planes, const uint32_t *region_mask, size_t n, uint32_t m, int mem,
                                       unsigned flags, bvhgpu_hits **hits);
int bvhgpu_instances_region_masked_f64(bvhgpu_instances *s, const double *planes, const uint32_t *region_mask, size_t n, uint32_t m, int mem,
                                       unsigned flags, bvhgpu_hits **hits);

/* ---- timing hook used by bench.py: HIP-event time (ms) of the kernels of the last call of each
 * phase on this ctx's stream (build / flatten / traverse main kernel / traverse total). ---- */
typedef struct { float build_ms, flatten_ms, traverse_kernel_ms, traverse_total_ms; } bvhgpu_timings;
int bvhgpu_enable_timing(bvhgpu_ctx *ctx, int on);
int bvhgpu_last_timings(bvhgpu_ctx *ctx, bvhgpu_timings *out);

/* ---- scene ingest (host code): Wavefront OBJ → triangles, as `obj::load_obj::<Triangle>` + `FromRawVertex::process`
 * do for the reference's Sponza benches (testbase.rs:445-487, 619-634): every polygon (P / PT / PN / PTN) becomes a
 * triangle fan over its positions.  *tris_out: malloc'ed n x 9 floats [a xyz, b xyz, c xyz] (release with
 * bvhgpu_obj_free); bounds_out (nullable): join of the triangle AABBs.  Errors: BVHGPU_INVALID_ARG + bvhgpu_obj_last_error(). */
int bvhgpu_obj_parse(const char *text, size_t len, float **tris_out, size_t *n_tris_out, float bounds_out[6]);
void bvhgpu_obj_free(float *tris);
const char *bvhgpu_obj_last_error(void);
/* Triangle::new's cached aabb = empty.grow(a).grow(b).grow(c) (testbase.rs:325-333): n x [min xyz, max xyz] */
int bvhgpu_triangles_aabbs_f32(const float *tris, size_t n, float *aabbs_out);

/* ---- tuning knobs (performance only; results never change).  Not part of the reference surface. ---- */
typedef enum {
    BVHGPU_TUNE_TRAVERSE_VARIANT = 0,      /* 0 one ray per lane per launch; 2 persistent workgroups over the binary traversal
                                              array with ray refill and the top of the tree resident in LDS; 3 (default) wide
                                              walk (four grandchild boxes per step) where its preconditions hold, else 2 */
    BVHGPU_TUNE_WIDE_ITEMS_LOG4 = 1,       /* variant 3, CSR outputs: cut every ray into up to 4^v items (v = 0, 1, 2); default -1 = by batch size */
    BVHGPU_TUNE_WIDE_STACK_LDS = 2,        /* variant 3: stack entries per lane kept in LDS (default -1 = 6 for rays cut into items, 8 for whole rays, 10 for whole rays of a COHERENT batch; deeper entries live in HBM) */
    BVHGPU_TUNE_TRAVERSE_LDS_MIN_RAYS = 3, /* variant 2 is used for batches of at least this many rays (default 16384) */
    BVHGPU_TUNE_TRAVERSE_LDS_SLOTS = 4,    /* variant 2: top-of-tree entries kept in LDS per workgroup (default 0 = as many as let two workgroups share a CU: f32 2559, f64 1462) */
    BVHGPU_TUNE_TRAVERSE_LDS_THREADS = 5,  /* variant 2: workgroup size (default 0 = per type: f32 1024, f64 512) */
    BVHGPU_TUNE_TRAVERSE_SPLIT = 6,        /* variant 2, CSR outputs: walk every ray as two items (left / right subtree of the
                                              root); default 1 */
    BVHGPU_TUNE_WIDE_WG_PER_CU = 7,        /* variant 3: workgroups sharing a CU's LDS (default 0 = 2) */
    BVHGPU_TUNE_WIDE_THREADS = 8,          /* variant 3: workgroup size (default 0 = per type: f32 1024, f64 512) */
    BVHGPU_TUNE_WIDE_SLOTS = 9,            /* variant 3: cap on the top-of-tree wide nodes kept in LDS (default 0 = what fits) */
    BVHGPU_TUNE_BUILD_LEVEL_LAUNCHES = 10, /* builder, level tier: 1 = one launch per tree level (k_level: split of level L-1 and binning of level L fused,
                                              the selection recomputed per tile: the shorter chain, more work per shape); 2 = two launches per level
                                              (k_bin, k_split); 0 (default) = by scene size: 1 up to 250 000 shapes, 2 above */
    BVHGPU_TUNE_WIDE_EARLY_ITEMS = 11,     /* variant 3 with BVHGPU_TRAVERSE_RAYS_READY on a tree that is being rebuilt: 1 = cut the rays into items on a
                                              side stream as soon as the build has split tree level 3; 0 (default) = in the walk's prologue.  Measured on
                                              configs[1]: the walk shrinks by 10 µs, the two stream dependencies and the guest kernel cost the build as
                                              much — kept selectable, off by default */
    BVHGPU_TUNE_WIDE_STAGE_SHIFT = 12,     /* variant 3, whole rays (large batches), indices only: the first 2^v shapes of every ray are written straight to a
                                              per-ray slot (4 bytes per hit) and gathered into the CSR; only later hits of a ray go through 12-byte pool
                                              records.  -1 (default) = 3 for batches flagged BVHGPU_TRAVERSE_COHERENT, off otherwise; 0 = off (every hit
                                              through the pool); 2 .. 5 = on for every such batch */
    BVHGPU_TUNE_WIDE_REC8 = 13,            /* variant 3, whole rays, indices only: pool records of 8 bytes per hit (16-byte records {ray, k, shape, shape} for two
                                              consecutive hits of a ray) instead of 12; 1 (default) on, 0 off */
    BVHGPU_TUNE_WIDE_F64_GUIDE = 14,       /* variant 3, f64 trees, indices only: 1 (default) = walk the tree's f32 guide boxes (the f64 boxes grown by 2^-18 of the
                                              scene's largest |coordinate| and rounded outward) with the rays converted to f32 where the walk loads them, and test only the leaf
                                              candidates in f64 — the hit lists are the same, the walk runs at the f32 rate; a batch with a ray outside
                                              the range the argument covers (|origin| > 3 x scene, |1/d| x scene outside 2^+-100, non-finite) is replayed
                                              with the f64 walk and the result object skips the guide for 1, 2, 4 … 64 batches on consecutive failures before it tries again; 0 = always the f64 walk */
    BVHGPU_TUNE_FLATTEN_LAZY = 15,         /* bvhgpu_rebuild_flat_async / bvhgpu_build_flat_*: 1 (default) = the flatten behind a build writes what the wide walk
                                              reads (wide nodes, their LDS slot table, an f64 tree's guide nodes); the reference-layout FlatNode array and the
                                              folded binary array are written by a second pass the first time something asks for them (bvhgpu_flat_nodes,
                                              a binary / STATS / t-slice / ordered walk, nearest_to, scene export, a broadcast) — same arrays, byte for byte;
                                              0 = every flatten writes everything at once; 2 = every flatten writes everything, the second pass on the ctx's side
                                              stream BESIDE the walk that follows (the walk reads none of it); the batch's wait covers it; 3 = every flatten writes
                                              the reference-layout FlatNode array (what Bvh::flatten returns) and the wide walk's arrays; only the engine's own folded
                                              binary array waits for its first reader */
    BVHGPU_TUNE_BUILD_LEVEL_PERSIST = 16,  /* builder, level tier with one launch per level, scenes of 32 x 769 shapes and more: != 0 = the tier's passes from tree level 4 on run as
                                              ONE persistent launch, a workgroup group per level-3 subtree that synchronises with itself after every pass (1 = 32 workgroups
                                              per group, 8 .. 64 = that many); 0 (default) = a launch per level throughout.  Measured on configs[1]: 64 per group builds in
                                              0.1886 - 0.1891 ms against 0.1876 - 0.1895 ms (the pass is a chain of dependent loads, not its launch boundary), 32 per group is
                                              slower (two tiles per workgroup) — kept selectable and parity-tested, off by default (profiles/r5_persist_ab.log) */
    BVHGPU_TUNE_HOST_CHUNKS = 17,          /* bvhgpu_traverse_host_*: the batch is walked as this many chunks, so that the upload of one overlaps the walk of the
                                              previous one and the download of the offsets of the one before (1 .. 16); 0 (default) = by batch size: 3 from 512 K
                                              rays, 2 from 256 K, else 1.  The last chunk is an eighth of the batch (what is left to do when the upload ends) */
    BVHGPU_TUNE_WIDE_MIN_RAYS_PER_WG = 18, /* variant 3, rays cut into 16 items, batches that fill at most a quarter of the chip's workgroup slots at one ray per lane
                                              (up to 128 K rays): the rays are spread over all slots, down to this many rays per workgroup (multiple of 64; default
                                              256); 0 = one ray per lane always */
    BVHGPU_TUNE_HOST_ZERO_COPY = 19,       /* bvhgpu_traverse_host_* / bvhgpu_build_traverse_host_* on PINNED buffers (bvhgpu_host_alloc / _register): bit 1 = the device
                                              writes offsets / indices straight into the caller's arrays (no download, no hop to a third stream); bit 0 = the device
                                              reads the caller's ray arrays itself (Ray::new straight out of host memory, no staging copy).  Default 2: bit 0 moves the
                                              bytes at link speed (56 GB/s) but the build running beside it slows down four-fold while a kernel streams host memory
                                              (k_level 12 -> 50 µs: profiles/r6_host_zero_copy.log), so the copy engines keep the upload.  0 = copy engines both
                                              ways.  Pageable buffers always go through the copy engines */
    BVHGPU_TUNE_BUILD_LEVEL_TILE = 20,     /* builder, level tier, two launches per level (scenes above 250 K shapes): positions per workgroup tile, a multiple of 256
                                              (0, default: 512, from 600 K shapes 1024, from 2 M 2048, from 6 M 4096).  A scheduling unit only: the tree is the same whatever the tile */
    BVHGPU_TUNE_FLATTEN_INLINE = 21,       /* f32 trees, the flatten enqueued with a build: the builder's wave tier writes the FlatNode / wide-node entries of the
                                              subtrees it builds (<= 64 shapes: 97 % of the nodes) itself and the flatten kernel behind it only the nodes above:
                                              1 (default), or 0: the flatten kernel writes everything.  Same arrays either way */
    BVHGPU_TUNE_QUERY_VARIANT = 22,        /* bvhgpu_query_*: 0 = the binary walk (one query per lane over the folded array); 1 = the wide walk (four grandchild
                                              boxes per step, per-lane stack in LDS) wherever its preconditions hold; -1 (default) = by kind, dtype and batch size where the
                                              wide walk measured ahead on configs[1]'s scene: points (f32 below 262 144 queries, f64 always), f64
                                              boxes, f64 balls from 262 144 queries; the binary walk otherwise (profiles/r7_query_bench.json).
                                              Results never change */
    BVHGPU_TUNE_COUNT = 23
} bvhgpu_tune;
int bvhgpu_set_tuning(bvhgpu_ctx *ctx, int knob, int value);
int bvhgpu_get_tuning(const bvhgpu_ctx *ctx, int knob, int *value);

#ifdef __cplusplus
}
#endif
#endif /* BVH_MI355X_H */

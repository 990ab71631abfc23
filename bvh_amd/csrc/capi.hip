// capi.hip — the extern "C" boundary declared in include/bvh_mi355x.h.
// Every entry point catches everything, records a message on the ctx and returns a status code.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>

#include "engine.hpp"

using namespace bvhgpu;

namespace {

thread_local std::string g_noctx_err;

int fail(bvhgpu_ctx* ctx, int status, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_noctx_err = msg;
    return status;
}

template <typename F> int guarded(bvhgpu_ctx* ctx, F&& f) {
    try {
        return f();
    } catch (const HipFail& e) {
        switch (e.kind) {
            case Fail::None: break;
            case Fail::Overflow: return fail(ctx, BVHGPU_OVERFLOW, "more than 2^32-1 hits in one batch");
            case Fail::NonFinite:
                return fail(ctx, BVHGPU_INVALID_ARG, "shape AABBs contain NaN or infinity (or their centroid extent overflows): the reference panics on "
                                                     "such input (bvh_node.rs:214-217, to_usize().unwrap()); nothing was built");
            case Fail::Rebroadcast:
                return fail(ctx, BVHGPU_REBROADCAST, "the tree was broadcast before its build was finalized and the build then needed the slow path (unbalanced tree): "
                                                     "this rank's tree and results are complete, the peers' are not — every rank calls bvhgpu_bcast_known again");
            case Fail::RecvRebroadcast:
                return fail(ctx, BVHGPU_REBROADCAST, "the root broadcast its tree before the build was finalized and the build was not complete: nothing usable was "
                                                     "received — every rank calls bvhgpu_bcast_known again");
            case Fail::RecvInvalid:
                return fail(ctx, BVHGPU_INVALID_ARG, "the broadcast's root reported that it had no valid tree to send (its own call returned the reason); nothing was received");
            case Fail::RecvGarbled: return fail(ctx, BVHGPU_RCCL_ERROR, "the broadcast header did not arrive intact");
            case Fail::StaleTree: return fail(ctx, BVHGPU_INVALID_ARG, "the tree changed before the asynchronous batch was completed");
            case Fail::OrderedDepth: return fail(ctx, BVHGPU_OVERFLOW, "tree deeper than the ordered iterator's 32-entry stack (child_distance_traverse.rs:36)");
        }
        char buf[512];
        snprintf(buf, sizeof buf, "%s failed: %s (line %d)", e.what, hipGetErrorString(e.err), e.line);
        return fail(ctx, e.err == hipErrorOutOfMemory ? BVHGPU_OOM : BVHGPU_HIP_ERROR, buf);
    } catch (const std::bad_alloc&) {
        return fail(ctx, BVHGPU_OOM, "host allocation failed");
    } catch (...) {
        return fail(ctx, BVHGPU_HIP_ERROR, "unknown exception");
    }
}

void use_device(bvhgpu_ctx* ctx) { BVH_HIP(hipSetDevice(ctx->device)); }

// ---- named rules ------------------------------------------------------------------------------------------------------------------------
// Each refusal that more than one family gives, worded once: BVHGPU_OK (0) or the status, with the message recorded.  A front end is a
// flat list of `if (const int rc = rule_...) return rc;` lines in ITS OWN order — which refusal wins when two apply is interface and
// differs between the families on purpose; what is shared is what a rule says.  A new family lists the rules it needs and adds none.
static_assert(BVHGPU_OK == 0, "a rule's status is tested as a truth value");
int rule_mem(bvhgpu_ctx* ctx, int mem) {
    return mem == BVHGPU_HOST || mem == BVHGPU_DEVICE ? (int)BVHGPU_OK : fail(ctx, BVHGPU_INVALID_ARG, "mem must be BVHGPU_HOST or BVHGPU_DEVICE");
}
int rule_hits_arg(bvhgpu_ctx* ctx, bvhgpu_hits* const* hits) { return hits ? (int)BVHGPU_OK : fail(ctx, BVHGPU_INVALID_ARG, "hits is NULL"); }
int rule_hits_idle(bvhgpu_ctx* ctx, bvhgpu_hits* const* hits) {   // the result object a batch is about to fill
    return *hits && (*hits)->pend_async ? fail(ctx, BVHGPU_INVALID_ARG, "the result object still holds an asynchronous batch: call bvhgpu_hits_wait first") : (int)BVHGPU_OK;
}
int rule_hits_complete(const bvhgpu_hits* h) {                    // the result object an accessor is about to read
    return h->pend_async ? fail(h->ctx, BVHGPU_INVALID_ARG, "the result object holds an asynchronous batch that has not been completed: call bvhgpu_hits_wait first") : (int)BVHGPU_OK;
}
int rule_batch_size(bvhgpu_ctx* ctx, size_t n, const char* plural) {   // offsets and NONE are u32
    return n >= 0xFFFFFFFFull ? fail(ctx, BVHGPU_OVERFLOW, std::string("more than 2^32-2 ") + plural + " in one batch") : (int)BVHGPU_OK;
}
int rule_rows_size(bvhgpu_ctx* ctx, size_t n, uint32_t k, const char* msg) {   // n padded rows of k slots
    return n >= 0xFFFFFFFFull || n * (size_t)k >= 0x100000000ull ? fail(ctx, BVHGPU_OVERFLOW, msg) : (int)BVHGPU_OK;
}
int rule_k(bvhgpu_ctx* ctx, uint32_t k, uint32_t max_k, const char* max_name) {
    return k == 0 || k > max_k ? fail(ctx, BVHGPU_INVALID_ARG, std::string("k must be between 1 and ") + max_name) : (int)BVHGPU_OK;
}
int rule_flattened(const bvhgpu_tree* t) { return t->flattened ? (int)BVHGPU_OK : fail(t->ctx, BVHGPU_NOT_FLATTENED, "call bvhgpu_flatten first"); }
int rule_leaf(bvhgpu_ctx* ctx, int leaf) {
    return leaf == BVHGPU_LEAF_BOX || leaf == BVHGPU_LEAF_TRIANGLE || leaf == BVHGPU_LEAF_SPHERE
               ? (int)BVHGPU_OK : fail(ctx, BVHGPU_INVALID_ARG, "leaf must be BVHGPU_LEAF_BOX, BVHGPU_LEAF_TRIANGLE or BVHGPU_LEAF_SPHERE");
}
int rule_leaf_array(const bvhgpu_tree* t, int leaf) {   // the per-shape array the leaf kind reads
    if (leaf == BVHGPU_LEAF_TRIANGLE && !t->has_tris) return fail(t->ctx, BVHGPU_INVALID_ARG, "triangle hits need bvhgpu_tree_set_triangles first");
    if (leaf == BVHGPU_LEAF_SPHERE && !t->has_spheres) return fail(t->ctx, BVHGPU_INVALID_ARG, "sphere hits need bvhgpu_tree_set_spheres first");
    return BVHGPU_OK;
}
int rule_shape_kind(bvhgpu_ctx* ctx, int kind) {
    return kind == 0 || kind == 1 ? (int)BVHGPU_OK : fail(ctx, BVHGPU_INVALID_ARG, "shape kind must be 0 (AABB) or 1 (triangle)");
}
int rule_kind_array(const bvhgpu_tree* t, int kind) {
    return kind == 1 && !t->has_tris ? fail(t->ctx, BVHGPU_INVALID_ARG, "triangle distance needs bvhgpu_tree_set_triangles first") : (int)BVHGPU_OK;
}
int rule_sphere_array(const bvhgpu_tree* t) {   // the *_sphere_* point entries: rule_kind_array's place
    return !t->has_spheres ? fail(t->ctx, BVHGPU_INVALID_ARG, "sphere distance needs bvhgpu_tree_set_spheres first") : (int)BVHGPU_OK;
}
// a walk that tests the leaves' navigator boxes cannot run on an imported tree that lost them — nor on a set with such a member
bool folded_away(const bvhgpu_tree* t) { return t->exact_only && !t->built && !t->unfolded; }
int rule_unfolded(const bvhgpu_tree* t) {
    return folded_away(t) ? fail(t->ctx, BVHGPU_INVALID_ARG, "an imported tree whose build had a split without SAH winner: its leaves' navigator boxes were folded away") : (int)BVHGPU_OK;
}
int rule_members_unfolded(const bvhgpu_instances* s) {
    for (const bvhgpu_tree* t : s->trees)
        if (folded_away(t)) return fail(s->ctx, BVHGPU_INVALID_ARG, "an imported member tree whose build had a split without SAH winner: its leaves' navigator boxes were folded away");
    return BVHGPU_OK;
}
int rule_planes(bvhgpu_ctx* ctx, const void* planes, size_t n, uint32_t m) {   // n regions of m planes
    if (m > BVHGPU_REGION_MAX_PLANES) return fail(ctx, BVHGPU_INVALID_ARG, "more than BVHGPU_REGION_MAX_PLANES planes per region");
    return n && m && !planes ? fail(ctx, BVHGPU_INVALID_ARG, "planes is NULL") : (int)BVHGPU_OK;
}
int no_tree() { return fail(nullptr, BVHGPU_INVALID_ARG, "NULL tree"); }
int no_set() { return fail(nullptr, BVHGPU_INVALID_ARG, "NULL instance set"); }
template <typename T> int rule_tree_dtype(const bvhgpu_tree* t, const char* noun) {
    return t->dtype != Traits<T>::dtype ? fail(t->ctx, BVHGPU_DTYPE_MISMATCH, std::string("tree dtype differs from ") + noun + " dtype") : (int)BVHGPU_OK;
}
template <typename T> int rule_set_dtype(const bvhgpu_instances* s, const char* noun) {
    return s->dtype != Traits<T>::dtype ? fail(s->ctx, BVHGPU_DTYPE_MISMATCH, std::string("instance set dtype differs from ") + noun + " dtype") : (int)BVHGPU_OK;
}

// bring a caller buffer to HBM: returns a device pointer (either the caller's or the ctx staging copy)
const void* to_device(bvhgpu_ctx* ctx, const void* p, size_t bytes, int mem, DevBuf& stage) {
    if (mem == BVHGPU_DEVICE || bytes == 0) return p;
    stage.reserve(bytes);
    BVH_HIP(hipMemcpyAsync(stage.p, p, bytes, hipMemcpyHostToDevice, ctx->stream));
    return stage.p;
}

void copy_out(bvhgpu_ctx* ctx, void* dst, const void* src_dev, size_t bytes, int mem) {
    if (!bytes) return;
    BVH_HIP(hipMemcpyAsync(dst, src_dev, bytes, mem == BVHGPU_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           ctx->stream));
    BVH_HIP(hipStreamSynchronize(ctx->stream));
}

// ---- the row stage: inputs and outputs of a synchronous padded-row call (bvhgpu_nearest_* / _knearest* / _traverse_khits_* and the
// bvhgpu_instances_trace / _knearest / _khits entries) -----------------------------------------------------------------------------------
// The caller lists its input and output columns as (pointer, bytes); at<U>(i) is column i's device pointer, inputs first.  DEVICE: the
// caller's own pointers.  HOST: every column gets a 16-byte-aligned place in ctx->upload (so each is aligned to its element, whatever the
// order) and the inputs are copied in; a NULL column (no tmax, no max_dist) stays NULL.  finish() copies each HOST output out with its own
// wait, or — DEVICE, where the family promises complete rows on return — waits for the stream.  A new padded-row family is a column list.
struct Span { const void* p; size_t bytes; };
class RowStage {
    static constexpr size_t MAX_COLS = 6;
    bvhgpu_ctx* ctx_; bool host_; size_t n_in_, n_ = 0;
    Span col_[MAX_COLS]; void* dev_[MAX_COLS];
  public:
    RowStage(bvhgpu_ctx* ctx, int mem, std::initializer_list<Span> in, std::initializer_list<Span> out) : ctx_(ctx), host_(mem == BVHGPU_HOST), n_in_(in.size()) {
        for (const Span& s : in) col_[n_++] = s;
        for (const Span& s : out) col_[n_++] = s;
        size_t off[MAX_COLS], need = 0;
        for (size_t i = 0; i < n_; i++) { off[i] = need; need += (col_[i].bytes + 15) & ~(size_t)15; }
        if (host_) ctx->upload.reserve(need + 64);
        for (size_t i = 0; i < n_; i++) dev_[i] = !host_ ? const_cast<void*>(col_[i].p) : col_[i].p ? ctx->upload.as<char>() + off[i] : nullptr;
        for (size_t i = 0; host_ && i < n_in_; i++)
            if (col_[i].p && col_[i].bytes) BVH_HIP(hipMemcpyAsync(dev_[i], col_[i].p, col_[i].bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    template <typename U> U* at(size_t i) const { return static_cast<U*>(dev_[i]); }
    void finish(bool sync_device) {
        for (size_t i = n_in_; host_ && i < n_; i++) copy_out(ctx_, const_cast<void*>(col_[i].p), dev_[i], col_[i].bytes, BVHGPU_HOST);
        if (!host_ && sync_device) BVH_HIP(hipStreamSynchronize(ctx_->stream));
    }
};

// an asynchronous build may still be in flight: wait for it and finish / validate it (build.hip build_finalize); likewise a
// broadcast that was received on the stream (comm.hip recv_finalize: its status header tells whether the root's tree was good)
void ensure_built(bvhgpu_tree* t) {
    if (t->pending_recv) recv_finalize(t);
    if (!t->pending_build) return;
    const bool sent_early = t->bcast_gen == t->gen;   // bvhgpu_bcast_known went out before this finalize (optimistic)
    if (t->dtype == BVHGPU_F32) build_finalize<float>(t); else build_finalize<double>(t);
    if (sent_early && t->redone_gen == t->gen) throw HipFail{hipErrorNotReady, nullptr, __LINE__, Fail::Rebroadcast};
}
// ... for a caller that replaces the tree's contents: what the previous build or receive came to no longer matters (a failed HIP call does)
void ensure_built_ignoring_outcome(bvhgpu_tree* t) {
    try { ensure_built(t); }
    catch (const HipFail& e) {
        switch (e.kind) {
            case Fail::Rebroadcast: case Fail::NonFinite: case Fail::RecvRebroadcast: case Fail::RecvInvalid: case Fail::RecvGarbled: break;
            default: throw;
        }
    }
}
int settle(bvhgpu_tree* t) {   // entry points that look at a tree's state first complete its asynchronous build
    if (!t->pending_build && !t->pending_recv) return BVHGPU_OK;
    return guarded(t->ctx, [&] { use_device(t->ctx); ensure_built(t); return (int)BVHGPU_OK; });
}

void detach_waiter(bvhgpu_hits* h) {
    bvhgpu_tree* t = h->wait_tree;
    h->wait_tree = nullptr;
    if (!t) return;
    for (size_t i = 0; i < t->waiters.size(); i++)
        if (t->waiters[i] == h) { t->waiters[i] = t->waiters.back(); t->waiters.pop_back(); break; }
}

// Completes an asynchronous batch (the body of bvhgpu_hits_wait; throws).  Whether the optimistic walk is still good is
// decided from what THIS result object recorded when it was enqueued — the tree's generation and whether that generation was
// still unfinalized — not from the tree's state now: the build may have been finalized since by bvhgpu_tree_wait, by another
// result object's wait, by a flatten / nearest / rebuild call, and a slow-path finalize (`redone_gen`) or a tree that must not be
// walked wide (`exact_only`) invalidates every batch of that generation, whoever notices first.
void finish_hits(bvhgpu_hits* h) {
    if (!h->pend_async) return;
    bvhgpu_ctx* ctx = h->ctx;
    h->pend_async = false;
    detach_waiter(h);
    bvhgpu_tree* t = h->pend_tree;
    BVH_HIP(hipStreamSynchronize(ctx->stream));
    if (!t) return;   // empty batch
    bool rebroadcast = false;
    try { ensure_built(t); }
    catch (const HipFail& e) { if (e.kind == Fail::Rebroadcast) rebroadcast = true; else throw; }
    // the generation this batch walked turned out to hold nothing (NaN / inf input, a broadcast whose root had no valid tree) and the
    // error may have been consumed elsewhere — bvhgpu_tree_wait, a rebuild that replaces the tree, another result object's wait: the
    // wait of THIS batch still returns what the synchronous call would have returned, never lists from an unbuilt tree
    if (t->failed_gen != 0 && t->failed_gen == h->pend_gen) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, t->failed_what != Fail::None ? t->failed_what : Fail::NonFinite};
    bool replay = h->pend_on_pending && h->pend_gen == t->gen && (t->redone_gen == h->pend_gen || (h->pend_wide && t->exact_only));
    if (h->pend_gen != t->gen) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::StaleTree};   // (rebuild / import settle the waiters first: unreachable)
    const void* rays = h->pend_rays;
    for (;;) {
        if (!replay && traverse_check(h)) break;
        replay = false;
        h->replays++;
        if (h->dtype == BVHGPU_F32) traverse_enqueue<float>(t, static_cast<const bvhgpu_ray_f32*>(rays), h->n_rays, h->flags, h);
        else traverse_enqueue<double>(t, static_cast<const bvhgpu_ray_f64*>(rays), h->n_rays, h->flags, h);
        BVH_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (rebroadcast) throw HipFail{hipErrorNotReady, nullptr, __LINE__, Fail::Rebroadcast};   // this rank's result is complete; the peers' trees are not
}
// Before a tree's arrays are overwritten or freed (rebuild, refit, import, broadcast receive, destroy): the asynchronous batches
// that were enqueued on it are completed first, so that a replay never runs on the wrong tree and no result object keeps a
// dangling pointer.  A failure is kept in the result object and returned by its own bvhgpu_hits_wait.
void settle_waiters_impl(bvhgpu_tree* t) {
    while (!t->waiters.empty()) {
        bvhgpu_hits* h = t->waiters.back();
        bvhgpu_ctx* hc = h->ctx;
        const std::string keep = hc ? hc->err : std::string();
        const int rc = guarded(hc, [&] { use_device(hc); finish_hits(h); return (int)BVHGPU_OK; });
        if (rc != BVHGPU_OK) { h->deferred_rc = rc; h->deferred_err = hc ? hc->err : std::string(); if (hc) hc->err = keep; }
        if (!t->waiters.empty() && t->waiters.back() == h) { h->wait_tree = nullptr; t->waiters.pop_back(); }   // (defensive: always detached by now)
    }
}

constexpr size_t MAX_SHAPES = (0xFFFFFFFFull - 1) / 3;  // flat indices are u32 (flat_bvh.rs:136)

template <typename T> int do_build(bvhgpu_tree* t, const T* aabbs, size_t n, int mem, bool flat = false, bool async = false) {
    bvhgpu_ctx* ctx = t->ctx;
    if (n && !aabbs) return fail(ctx, BVHGPU_INVALID_ARG, "aabbs is NULL");
    if (n > MAX_SHAPES) return fail(ctx, BVHGPU_OVERFLOW, "too many shapes for u32 flat indices");
    if (mem != BVHGPU_HOST && mem != BVHGPU_DEVICE) return fail(ctx, BVHGPU_INVALID_ARG, "bad mem kind");
    use_device(ctx);
    ensure_built_ignoring_outcome(t);   // a previous asynchronous build of this tree (its outcome no longer matters: everything is rebuilt)
    settle_waiters_impl(t);
    if (ctx->timing) BVH_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    const T* dev = aabbs;
    if (n && mem == BVHGPU_HOST) {  // upload straight into the tree's own copy
        t->aabbs.reserve(n * 6 * sizeof(T));
        BVH_HIP(hipMemcpyAsync(t->aabbs.p, aabbs, n * 6 * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        dev = t->aabbs.as<T>();
    }
    if (async) build_enqueue<T>(t, dev, n, flat);
    else build_tree<T>(t, dev, n, flat);
    if (flat && n == 0) t->flattened = true;
    if (ctx->timing) { BVH_HIP(hipEventRecord(ctx->ev[1], ctx->stream)); ctx->ev_set |= 1u; }
    return BVHGPU_OK;
}

// the shapes moved: same topology, boxes recomputed (refit.hip)
template <typename T> int do_refit(bvhgpu_tree* t, const T* aabbs, size_t n, int mem) {
    bvhgpu_ctx* ctx = t->ctx;
    use_device(ctx);
    ensure_built(t);
    settle_waiters_impl(t);
    if (!t->built) return fail(ctx, BVHGPU_INVALID_ARG, "refit needs a tree that was built here (imported scenes carry no BvhNode array)");
    join_flat(t);
    if (n != t->n) return fail(ctx, BVHGPU_INVALID_ARG, "refit: the number of shapes differs from the tree's (build again)");
    if (n && !aabbs) return fail(ctx, BVHGPU_INVALID_ARG, "aabbs is NULL");
    if (mem != BVHGPU_HOST && mem != BVHGPU_DEVICE) return fail(ctx, BVHGPU_INVALID_ARG, "bad mem kind");
    use_device(ctx);
    // HOST input is staged in the ctx (one shape: straight into the tree's own copy, nothing is validated), so that the tree's arrays are
    // first written after the input has passed the builders' contract; k_refit_leaves then copies it into the tree's own copy
    const T* dev = aabbs;
    if (n == 1 && mem == BVHGPU_HOST) {
        BVH_HIP(hipMemcpyAsync(t->aabbs.p, aabbs, 6 * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        dev = t->aabbs.as<T>();
    } else if (n) {
        dev = static_cast<const T*>(to_device(ctx, aabbs, n * 6 * sizeof(T), mem, ctx->upload));
    }
    if (!refit_input_ok<T>(t, dev))
        return fail(ctx, BVHGPU_INVALID_ARG, "refit: shape AABBs contain NaN or infinity (the builders' input contract); the tree is unchanged");
    refit_tree<T>(t, dev);
    return BVHGPU_OK;
}

// bvhgpu_rebuild*_f32 / _f64 and bvhgpu_refit_f32 / _f64: the tree must be of the entry point's dtype
template <typename T> int tree_is(bvhgpu_tree* t) {
    if (!t) return BVHGPU_INVALID_ARG;
    if (t->dtype != Traits<T>::dtype) return fail(t->ctx, BVHGPU_DTYPE_MISMATCH, t->dtype == BVHGPU_F64 ? "tree is f64" : "tree is f32");
    return BVHGPU_OK;
}
template <typename T> int rebuild(bvhgpu_tree* t, const T* aabbs, size_t n, int mem, bool flat, bool async) {
    const int rc = tree_is<T>(t);
    return rc != BVHGPU_OK ? rc : guarded(t->ctx, [&] { return do_build<T>(t, aabbs, n, mem, flat, async); });
}
template <typename T> int refit(bvhgpu_tree* t, const T* aabbs, size_t n, int mem) {
    const int rc = tree_is<T>(t);
    return rc != BVHGPU_OK ? rc : guarded(t->ctx, [&] { return do_refit<T>(t, aabbs, n, mem); });
}

template <typename T> int new_build(bvhgpu_ctx* ctx, const T* aabbs, size_t n, int mem, bvhgpu_tree** out, bool flat = false) {
    if (!ctx || !out) return fail(ctx, BVHGPU_INVALID_ARG, "ctx/out is NULL");
    *out = nullptr;
    bvhgpu_tree* t = new bvhgpu_tree();
    t->ctx = ctx;
    t->dtype = Traits<T>::dtype;
    int rc = guarded(ctx, [&] { return do_build<T>(t, aabbs, n, mem, flat); });
    if (rc != BVHGPU_OK) { delete t; return rc; }
    *out = t;
    return BVHGPU_OK;
}

// ---- what kind of result a bvhgpu_hits holds ---------------------------------------------------------------------------------------------
// One row per kind, in the enum's order: how the header spells the batches that make it, the accessor that reads it, and the internal
// bits of bvhgpu_hits::flags that mark it (traverse_batch's walk-mode selectors and rows_reset's kinds; 0: the caller's flags alone).
// A new family adds a row here and nothing to the accessors of the others.
enum class HitsKind { Csr, Closest, Any, Box, Sphere, Allhits, Within, Region, InstRegion, InstAllhits, InstWithin };
struct HitsKindRow { HitsKind kind; const char* entry; const char* reader; unsigned bits; };
static constexpr HitsKindRow HITS_KINDS[] = {
    {HitsKind::Csr, "bvhgpu_traverse_* / bvhgpu_query_* CSR", "bvhgpu_hits_fetch", 0},   // (options: T_SLICE, and TRIANGLES for bvhgpu_hits_fetch_triangles)
    {HitsKind::Closest, "BVHGPU_TRAVERSE_CLOSEST", "bvhgpu_hits_fetch_closest", 0},
    {HitsKind::Any, "bvhgpu_traverse_any_*", "bvhgpu_hits_fetch_any", TRAVERSE_ANY_HIT},
    {HitsKind::Box, "bvhgpu_traverse_box_*", "bvhgpu_hits_fetch_box", TRAVERSE_BOX_HIT},
    {HitsKind::Sphere, "bvhgpu_traverse_sphere_*", "bvhgpu_hits_fetch_sphere", TRAVERSE_SPHERE_HIT},
    {HitsKind::Allhits, "bvhgpu_traverse_allhits_*", "bvhgpu_hits_fetch_allhits", TRAVERSE_ALLHITS},
    {HitsKind::Within, "bvhgpu_within_*", "bvhgpu_hits_fetch_within", TRAVERSE_WITHIN},
    {HitsKind::Region, "bvhgpu_region_*", "bvhgpu_hits_fetch_region", TRAVERSE_REGION},
    // (its refusals name both region accessors: a caller who mixed the two region kinds up is told which one reads what)
    {HitsKind::InstRegion, "bvhgpu_instances_region_*", "bvhgpu_hits_fetch_instances_region, not bvhgpu_hits_fetch_region", TRAVERSE_REGION},   // (options: shapes / INSTANCES_ONLY)
    {HitsKind::InstAllhits, "bvhgpu_instances_allhits_*", "bvhgpu_hits_fetch_instances_allhits", TRAVERSE_INST_ALLHITS},
    {HitsKind::InstWithin, "bvhgpu_instances_within_*", "bvhgpu_hits_fetch_instances_within", TRAVERSE_INST_WITHIN},
};
static constexpr unsigned hits_kind_bits() {
    unsigned m = 0;
    for (const HitsKindRow& r : HITS_KINDS) m |= r.bits;
    return m;
}
static const HitsKindRow& hits_row(HitsKind k) { return HITS_KINDS[(int)k]; }
static_assert(HITS_KINDS[(int)HitsKind::InstWithin].kind == HitsKind::InstWithin && sizeof(HITS_KINDS) / sizeof(HITS_KINDS[0]) == 11, "rows in the enum's order");

// from what the object already stores: the internal bit, rg_inst within the region bit, else the caller's CLOSEST
static HitsKind hits_kind(const bvhgpu_hits* h) {
    for (const HitsKindRow& r : HITS_KINDS)
        if (h->flags & r.bits) return r.bits != TRAVERSE_REGION ? r.kind : h->rg_inst == REGION_INST_NONE ? HitsKind::Region : HitsKind::InstRegion;
    return (h->flags & BVHGPU_TRAVERSE_CLOSEST) ? HitsKind::Closest : HitsKind::Csr;
}

// What every accessor of a result object does first.  BVHGPU_OK: h holds a completed batch of the kind `want` (or `also`); every other
// kind is refused with one message, which names the accessor that does read it.  copies: the accessor copies out of HBM, so it needs the ctx.
static int hits_expect(const bvhgpu_hits* h, bool copies, HitsKind want, HitsKind also) {
    if (!h || (copies && !h->ctx)) return BVHGPU_INVALID_ARG;
    if (const int rc = rule_hits_complete(h)) return rc;
    const HitsKindRow& have = hits_row(hits_kind(h));
    if (have.kind == want || have.kind == also) return BVHGPU_OK;
    const std::string none = want == HitsKind::Closest ? std::string("traverse was run without BVHGPU_TRAVERSE_CLOSEST")
                                                       : std::string("the result object holds no ") + hits_row(want).entry + " batch";
    return fail(h->ctx, BVHGPU_INVALID_ARG, none + ": it holds a " + have.entry + " batch, use " + have.reader);
}
static int hits_expect(const bvhgpu_hits* h, bool copies, HitsKind want) { return hits_expect(h, copies, want, want); }

// ---- result-object batches: bvhgpu_traverse_* / _traverse_async_* / _traverse_any_* / _traverse_box_* / _query_* ----------------------
// What a family tests between batch_open and batch_refusal — its flags, `mem`, the wait for the tree's build — stays in the family:
// the families differ there on purpose (an any-hit batch refuses bad flags before it settles the tree, a ray batch does not), and
// which refusal a caller gets when two apply is part of the interface.
int batch_open(bvhgpu_tree* tree, bvhgpu_hits** hits) {
    if (!tree) return BVHGPU_INVALID_ARG;
    return rule_hits_arg(tree->ctx, hits);
}
// the refusals every family shares, in the order every family reports them (input_missing: the family's own test of its input pointer)
template <typename T>
int batch_refusal(bvhgpu_tree* tree, bvhgpu_hits* const* hits, const char* noun, const char* plural, bool input_missing, const char* missing_msg, size_t n) {
    bvhgpu_ctx* ctx = tree->ctx;
    if (const int rc = rule_hits_idle(ctx, hits)) return rc;
    if (const int rc = rule_tree_dtype<T>(tree, noun)) return rc;
    if (const int rc = rule_flattened(tree)) return rc;
    if (input_missing) return fail(ctx, BVHGPU_INVALID_ARG, missing_msg);
    return rule_batch_size(ctx, n, plural);
}
// the caller's result object, made if there is none yet
bvhgpu_hits* batch_hits(bvhgpu_hits** hits) {
    bvhgpu_hits* h = *hits;
    if (!h) h = new bvhgpu_hits();
    *hits = h;
    h->pend_kind = 0; h->pend_queries = nullptr; h->pend_qwide = false;   // (the object may have held a query batch)
    return h;
}
// ---- what a result-object family stages in the result object ----------------------------------------------------------------------------
// The per-row side array (tmax of rays, max_dist of points) → its device pointer.  NULL stays NULL (+inf for every ray), DEVICE is used in
// place, HOST values go into h->tmaxbuf.  The rows families (all-hits, within and their instanced forms) pass the pointer on and keep none.
template <typename T> const T* stage_side(bvhgpu_ctx* ctx, bvhgpu_hits* h, const T* v, size_t n, int mem) {
    if (!v || !n || mem != BVHGPU_HOST) return v;
    h->tmaxbuf.reserve(n * sizeof(T));
    BVH_HIP(hipMemcpyAsync(h->tmaxbuf.p, v, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return h->tmaxbuf.as<T>();
}
// ... of an any-hit / box / sphere batch: kept in the result object, so that a replay (wide-walk stack overflow) reads it again
template <typename T> void stage_tmax(bvhgpu_ctx* ctx, bvhgpu_hits* h, const T* tmax, size_t n_rays, int mem) {
    h->pend_tmax = stage_side<T>(ctx, h, tmax, n_rays, mem);
}
// The main input of the families whose input is not rays or points (queries, planes) → its device pointer; HOST values go into h->qbuf
// (a replay of a query batch reads them again).
template <typename T> const T* stage_queries(bvhgpu_ctx* ctx, bvhgpu_hits* h, const T* q, size_t bytes, int mem) {
    if (mem != BVHGPU_HOST || !bytes) return q;
    h->qbuf.reserve(bytes);
    BVH_HIP(hipMemcpyAsync(h->qbuf.p, q, bytes, hipMemcpyHostToDevice, ctx->stream));
    return h->qbuf.as<T>();
}

template <typename T>
int do_traverse(bvhgpu_tree* tree, const typename Traits<T>::Ray* rays, size_t n_rays, int mem, unsigned flags,
                bvhgpu_hits** hits, bool async = false) {
    if (const int rc = batch_open(tree, hits)) return rc;
    bvhgpu_ctx* ctx = tree->ctx;
    if (!async) { if (const int rc = settle(tree)) return rc; }
    else if (mem != BVHGPU_DEVICE) return fail(ctx, BVHGPU_INVALID_ARG, "asynchronous traversal takes rays that are resident in HBM");
    if (const int rc = batch_refusal<T>(tree, hits, "ray", "rays", n_rays && !rays, "rays is NULL", n_rays)) return rc;
    if ((flags & (BVHGPU_TRAVERSE_TRIANGLES | BVHGPU_TRAVERSE_CLOSEST)) && !tree->has_tris)
        return fail(ctx, BVHGPU_INVALID_ARG, "TRIANGLES / CLOSEST need bvhgpu_tree_set_triangles first");
    if ((flags & BVHGPU_TRAVERSE_T_SLICE) && (flags & (BVHGPU_TRAVERSE_TRIANGLES | BVHGPU_TRAVERSE_CLOSEST)))
        return fail(ctx, BVHGPU_INVALID_ARG, "T_SLICE cannot be combined with TRIANGLES / CLOSEST");
    if (flags & (BVHGPU_TRAVERSE_NEAREST_FIRST | BVHGPU_TRAVERSE_FARTHEST_FIRST)) {
        if (!tree->built && !tree->pending_build) return fail(ctx, BVHGPU_INVALID_ARG, "ordered traversal walks the BvhNode array: the tree must have been built here");
        if ((flags & BVHGPU_TRAVERSE_NEAREST_FIRST) && (flags & BVHGPU_TRAVERSE_FARTHEST_FIRST))
            return fail(ctx, BVHGPU_INVALID_ARG, "NEAREST_FIRST and FARTHEST_FIRST are alternatives");
        if (flags & (BVHGPU_TRAVERSE_T_SLICE | BVHGPU_TRAVERSE_STATS))
            return fail(ctx, BVHGPU_INVALID_ARG, "ordered traversal supports the INDICES, TRIANGLES and CLOSEST outputs only");
    } else if (flags & BVHGPU_TRAVERSE_BEST_FIRST) {
        return fail(ctx, BVHGPU_INVALID_ARG, "BEST_FIRST needs NEAREST_FIRST or FARTHEST_FIRST");
    }
    if ((flags & BVHGPU_TRAVERSE_TRIANGLES) && (flags & BVHGPU_TRAVERSE_CLOSEST))
        return fail(ctx, BVHGPU_INVALID_ARG, "TRIANGLES and CLOSEST are alternatives");
    flags &= ~hits_kind_bits();   // (internal: only the entries of the other kinds set them)
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        const auto* dev = static_cast<const typename Traits<T>::Ray*>(
            to_device(ctx, rays, n_rays * sizeof(typename Traits<T>::Ray), mem, ctx->upload));
        if (async) {
            h->force_binary = false; h->pend_attempts = 0; h->deferred_rc = 0; h->replays = 0;
            h->pend_gen = tree->gen; h->pend_on_pending = tree->pending_build || tree->pending_recv;
            traverse_enqueue<T>(tree, dev, n_rays, flags, h);
            h->pend_async = true;
            h->wait_tree = tree; tree->waiters.push_back(h);
        } else {
            traverse_batch<T>(tree, dev, n_rays, flags, h);
        }
        return (int)BVHGPU_OK;
    });
}

// bvhgpu_traverse_any_*, bvhgpu_traverse_box_* and bvhgpu_traverse_sphere_*: one result per ray among the candidates of FlatBvh::traverse's list below tmax[i].
//   any-hit (kind_bit TRAVERSE_ANY_HIT, traverse.hip MODE_ANY): the first candidate whose triangle distance is < tmax[i]; needs triangles.
//   box hit (kind_bit TRAVERSE_BOX_HIT, MODE_BOX_CLOSEST / MODE_BOX_FIRST): the shape whose own AABB the ray enters first — or, with
//   BVHGPU_TRAVERSE_FIRST, the first one of the list — among those with enter < tmax[i].  No triangles are needed or read.
//   sphere hit (kind_bit TRAVERSE_SPHERE_HIT, MODE_SPHERE_CLOSEST / MODE_SPHERE_FIRST): the same two choices among the shapes whose sphere
//   (bvhgpu_tree_set_spheres_*) the ray hits with distance < tmax[i] (walk.hpp ray_sphere); needs the spheres, no triangles.
template <typename T>
int do_traverse_tmax(bvhgpu_tree* tree, const typename Traits<T>::Ray* rays, const T* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits,
                     unsigned allowed_flags, const char* flags_msg, unsigned kind_bit, const char* needs_msg) {   // needs_msg: the refusal when the kind's per-shape array (sphere hit: the spheres, else the triangles) is not set; NULL: none needed
    if (const int rc = batch_open(tree, hits)) return rc;
    bvhgpu_ctx* ctx = tree->ctx;
    if (flags & ~allowed_flags) return fail(ctx, BVHGPU_INVALID_ARG, flags_msg);
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = settle(tree)) return rc;
    if (const int rc = batch_refusal<T>(tree, hits, "ray", "rays", n_rays && !rays, "rays is NULL", n_rays)) return rc;
    if (needs_msg && !(kind_bit == TRAVERSE_SPHERE_HIT ? tree->has_spheres : tree->has_tris)) return fail(ctx, BVHGPU_INVALID_ARG, needs_msg);
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        const auto* dev = static_cast<const typename Traits<T>::Ray*>(
            to_device(ctx, rays, n_rays * sizeof(typename Traits<T>::Ray), mem, ctx->upload));
        stage_tmax<T>(ctx, h, tmax, n_rays, mem);
        traverse_batch<T>(tree, dev, n_rays, flags | kind_bit, h);
        return (int)BVHGPU_OK;
    });
}
template <typename T>
int do_traverse_any(bvhgpu_tree* tree, const typename Traits<T>::Ray* rays, const T* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_tmax<T>(tree, rays, tmax, n_rays, mem, flags, hits, BVHGPU_TRAVERSE_COHERENT, "any-hit flags: 0 or BVHGPU_TRAVERSE_COHERENT",
                               TRAVERSE_ANY_HIT, "any-hit queries need bvhgpu_tree_set_triangles first");
}
template <typename T>
int do_traverse_box(bvhgpu_tree* tree, const typename Traits<T>::Ray* rays, const T* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_tmax<T>(tree, rays, tmax, n_rays, mem, flags, hits, BVHGPU_TRAVERSE_COHERENT | BVHGPU_TRAVERSE_FIRST,
                               "box-hit flags: BVHGPU_TRAVERSE_COHERENT and BVHGPU_TRAVERSE_FIRST only", TRAVERSE_BOX_HIT, nullptr);
}
template <typename T>
int do_traverse_sphere(bvhgpu_tree* tree, const typename Traits<T>::Ray* rays, const T* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_tmax<T>(tree, rays, tmax, n_rays, mem, flags, hits, BVHGPU_TRAVERSE_COHERENT | BVHGPU_TRAVERSE_FIRST,
                               "sphere-hit flags: BVHGPU_TRAVERSE_COHERENT and BVHGPU_TRAVERSE_FIRST only", TRAVERSE_SPHERE_HIT,
                               "sphere queries need bvhgpu_tree_set_spheres first");
}

// bvhgpu_query_*: an AABB / point / ball batch (query.hip).  queries == NULL: the tree's own shape AABBs (self-overlap).
template <typename T>
int do_query(bvhgpu_tree* tree, int kind, const T* queries, size_t n, int mem, unsigned flags, bvhgpu_hits** hits) {
    if (const int rc = batch_open(tree, hits)) return rc;
    bvhgpu_ctx* ctx = tree->ctx;
    if (kind != BVHGPU_QUERY_AABB && kind != BVHGPU_QUERY_POINT && kind != BVHGPU_QUERY_BALL) return fail(ctx, BVHGPU_INVALID_ARG, "unknown query kind");
    if (flags != 0) return fail(ctx, BVHGPU_INVALID_ARG, "query flags are reserved (0)");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = settle(tree)) return rc;
    const bool self = queries == nullptr;
    { const int rc = batch_refusal<T>(tree, hits, "query", "queries", self && !(kind == BVHGPU_QUERY_AABB && n == tree->n),
                                      "queries is NULL: only BVHGPU_QUERY_AABB with n = the tree's shape count (self-overlap)", n); if (rc != BVHGPU_OK) return rc; }
    if (const int rc = rule_unfolded(tree)) return rc;
    const size_t per = kind == BVHGPU_QUERY_AABB ? 6 : (kind == BVHGPU_QUERY_POINT ? 3 : 4);
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        const T* dev = self ? tree->aabbs.as<T>() : stage_queries<T>(ctx, h, queries, n * per * sizeof(T), mem);
        query_batch<T>(tree, kind, dev, n, h);
        return (int)BVHGPU_OK;
    });
}

template <typename T>
int do_rays_new(bvhgpu_ctx* ctx, const T* origins, const T* dirs, size_t n, int mem_in, typename Traits<T>::Ray* out,
                int mem_out) {
    if (!ctx) return BVHGPU_INVALID_ARG;
    if (n && (!origins || !dirs || !out)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    return guarded(ctx, [&] {
        use_device(ctx);
        using Ray = typename Traits<T>::Ray;
        const size_t vb = n * 3 * sizeof(T);
        const T* o = origins; const T* d = dirs;
        Ray* outd = out;
        size_t need = (mem_in == BVHGPU_HOST ? 2 * vb : 0) + (mem_out == BVHGPU_HOST ? n * sizeof(Ray) : 0);
        ctx->upload.reserve(need + 64);
        char* base = ctx->upload.as<char>();
        if (mem_in == BVHGPU_HOST) {
            BVH_HIP(hipMemcpyAsync(base, origins, vb, hipMemcpyHostToDevice, ctx->stream));
            BVH_HIP(hipMemcpyAsync(base + vb, dirs, vb, hipMemcpyHostToDevice, ctx->stream));
            o = reinterpret_cast<const T*>(base); d = reinterpret_cast<const T*>(base + vb);
            base += 2 * vb;
        }
        if (mem_out == BVHGPU_HOST) outd = reinterpret_cast<Ray*>(base);
        rays_new<T>(ctx, o, d, n, outd);
        if (mem_out == BVHGPU_HOST) copy_out(ctx, out, outd, n * sizeof(Ray), BVHGPU_HOST);
        return (int)BVHGPU_OK;
    });
}

// bvhgpu_gen_rays_* / bvhgpu_gen_primary_rays_*: rays written straight into HBM
void gen_rays(bvhgpu_ctx* ctx, uint64_t first, size_t n, const float bounds[6], bvhgpu_ray_f32* out_dev) { gen_rays_f32(ctx, first, n, bounds, out_dev); }
void gen_rays(bvhgpu_ctx* ctx, uint64_t first, size_t n, const float bounds[6], bvhgpu_ray_f64* out_dev) { gen_rays_f64(ctx, first, n, bounds, out_dev); }
template <typename Ray> int do_gen_rays(bvhgpu_ctx* ctx, uint64_t first, size_t n, const float bounds[6], Ray* out_dev) {
    if (!ctx || !bounds || (n && !out_dev)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (n >= 0xFFFFFFFFull) return fail(ctx, BVHGPU_OVERFLOW, "too many rays in one call");
    return guarded(ctx, [&] { use_device(ctx); gen_rays(ctx, first, n, bounds, out_dev); return (int)BVHGPU_OK; });
}
template <typename T>
int do_gen_primary(bvhgpu_ctx* ctx, const float cam[14], uint32_t width, uint32_t height, uint64_t first, size_t n, typename Traits<T>::Ray* out_dev) {
    if (!ctx || !cam || (n && !out_dev) || !width || !height) return fail(ctx, BVHGPU_INVALID_ARG, "bad argument");
    if (n >= 0xFFFFFFFFull) return fail(ctx, BVHGPU_OVERFLOW, "too many rays in one call");
    return guarded(ctx, [&] { use_device(ctx); gen_primary<T>(ctx, cam, width, height, first, n, out_dev); return (int)BVHGPU_OK; });
}

// ---- FlatBvh upload: convert the reference layout to the engine layout on the host (a marshalling
// step, like the AABB gather), keeping nav+leaf pairs un-folded unless their boxes are bit-identical.
template <typename T>
int tree_from_flat(bvhgpu_ctx* ctx, const typename Traits<T>::Flat* flat, size_t n_flat, const T* shape_aabbs,
                          size_t n, bvhgpu_tree** out) {
    if (!ctx || !out) return fail(ctx, BVHGPU_INVALID_ARG, "ctx/out is NULL");
    *out = nullptr;
    if ((n_flat && !flat) || (n && !shape_aabbs)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (n_flat >= 0xFFFFFFFFull) return fail(ctx, BVHGPU_OVERFLOW, "flat array too long");
    // validate indices; every entry maps 1:1 to a traversal entry (no folding: the uploaded shapes
    // may have moved since the build, flat_bvh.rs:411-418 re-tests shape.aabb())
    std::vector<TravNode<T>> trav(n_flat);
    for (size_t i = 0; i < n_flat; i++) {
        const auto& f = flat[i];
        TravNode<T> tn;
        std::memset(&tn, 0, sizeof tn);
        if (f.entry == NONE) {  // leaf entry
            if (f.shape >= n) return fail(ctx, BVHGPU_INVALID_ARG, "flat leaf refers to a shape out of range");
            if (f.exit != i + 1) return fail(ctx, BVHGPU_INVALID_ARG, "flat leaf exit_index must be index+1");
            const T* sb = shape_aabbs + 6 * (size_t)f.shape;
            for (int k = 0; k < 3; k++) { tn.mn[k] = sb[k]; tn.mx[k] = sb[3 + k]; }
            tn.exit = (uint32_t)(i + 1);
            tn.shape = f.shape;
        } else {
            if (f.entry != i + 1 || f.exit <= i || f.exit > n_flat)
                return fail(ctx, BVHGPU_INVALID_ARG, "flat navigator entry/exit out of range");
            for (int k = 0; k < 3; k++) { tn.mn[k] = f.min[k]; tn.mx[k] = f.max[k]; }
            tn.exit = f.exit;
            tn.shape = TRAV_INNER | SLOT_NONE;
        }
        trav[i] = tn;
    }
    // top-of-tree slots (heap numbers, flatten.hip k_top_slots) for the LDS-resident part of traversal:
    // an entry's first child follows it directly, its second child sits at the first child's exit.
    constexpr uint32_t SLOTS = TopCfg<T>::SLOTS;
    std::vector<uint32_t> slot_entry(SLOTS, NONE);
    {
        struct Frame { size_t index; uint32_t exit, heap, kids; };
        std::vector<Frame> stack;
        std::vector<uint32_t> heap(n_flat, SLOT_NONE);
        stack.push_back(Frame{(size_t)-1, (uint32_t)n_flat, 1u, 0u});
        bool binary = true;
        for (size_t i = 0; i < n_flat && binary; i++) {
            while (stack.size() > 1 && stack.back().exit <= i) stack.pop_back();
            Frame& par = stack.back();
            if (++par.kids > 2) { binary = false; break; }
            const uint32_t h = std::min<uint32_t>(2u * par.heap + (par.kids - 1u), SLOT_NONE);
            heap[i] = h;
            if (flat[i].entry != NONE) stack.push_back(Frame{i, flat[i].exit, h, 0u});
        }
        // FlatBvh::flatten only ever emits binary trees; an array that passes the index checks above but is not
        // binary would leave the LDS slot table empty while traversal still starts at slot 2
        if (!binary) return fail(ctx, BVHGPU_INVALID_ARG, "flat array is not a flattened binary tree (an entry has more than two children)");
        if (binary) {
            for (size_t i = 0; i < n_flat; i++) {
                if (heap[i] < SLOTS) slot_entry[heap[i]] = (uint32_t)i;
                if (flat[i].entry != NONE) {
                    const uint32_t ex = flat[i].exit;
                    const uint32_t es = (ex < n_flat && heap[ex] < SLOTS) ? heap[ex] : SLOT_NONE;
                    trav[i].shape = TRAV_INNER | es;
                }
            }
        }
    }
    bvhgpu_tree* t = new bvhgpu_tree();
    t->ctx = ctx; t->dtype = Traits<T>::dtype; t->n = n; t->n_nodes = 0; t->n_flat = n_flat; t->n_trav = n_flat;
    int rc = guarded(ctx, [&] {
        use_device(ctx);
        t->aabbs.reserve(n * 6 * sizeof(T) + 16);
        t->trav.reserve(n_flat * sizeof(TravNode<T>) + 16);
        t->flat.reserve(n_flat * sizeof(typename Traits<T>::Flat) + 16);
        t->slot_entry.reserve(SLOTS * 4);
        BVH_HIP(hipMemcpyAsync(t->slot_entry.p, slot_entry.data(), SLOTS * 4, hipMemcpyHostToDevice, ctx->stream));
        if (n) BVH_HIP(hipMemcpyAsync(t->aabbs.p, shape_aabbs, n * 6 * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        if (n_flat) {
            BVH_HIP(hipMemcpyAsync(t->trav.p, trav.data(), n_flat * sizeof(TravNode<T>), hipMemcpyHostToDevice, ctx->stream));
            BVH_HIP(hipMemcpyAsync(t->flat.p, flat, n_flat * sizeof(typename Traits<T>::Flat), hipMemcpyHostToDevice, ctx->stream));
        }
        BVH_HIP(hipStreamSynchronize(ctx->stream));
        return (int)BVHGPU_OK;
    });
    if (rc != BVHGPU_OK) { delete t; return rc; }
    t->built = false; t->flattened = true; t->unfolded = true; t->lazy_flat = false;
    *out = t;
    return BVHGPU_OK;
}

template <typename T>
int do_pairs(bvhgpu_ctx* ctx, const typename Traits<T>::Ray* rays, const T* tris, size_t n, int mem, T* out) {
    if (!ctx) return BVHGPU_INVALID_ARG;
    if (n && (!rays || !tris || !out)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (n >= 0xFFFFFFFFull) return fail(ctx, BVHGPU_OVERFLOW, "too many pairs in one call");
    return guarded(ctx, [&] {
        use_device(ctx);
        using Ray = typename Traits<T>::Ray;
        const Ray* rd = rays; const T* td = tris; T* od = out;
        if (mem == BVHGPU_HOST) {
            const size_t rb = n * sizeof(Ray), tb = n * 9 * sizeof(T), ob = n * 3 * sizeof(T);
            ctx->upload.reserve(rb + tb + ob + 64);
            char* base = ctx->upload.as<char>();
            BVH_HIP(hipMemcpyAsync(base, rays, rb, hipMemcpyHostToDevice, ctx->stream));
            BVH_HIP(hipMemcpyAsync(base + rb, tris, tb, hipMemcpyHostToDevice, ctx->stream));
            rd = reinterpret_cast<const Ray*>(base); td = reinterpret_cast<const T*>(base + rb); od = reinterpret_cast<T*>(base + rb + tb);
        }
        ray_triangle_pairs<T>(ctx, rd, td, n, od);
        if (mem == BVHGPU_HOST) copy_out(ctx, out, od, n * 3 * sizeof(T), BVHGPU_HOST);
        return (int)BVHGPU_OK;
    });
}

// ---- point batches: bvhgpu_nearest_* / bvhgpu_knearest_* / bvhgpu_knearest_tree_* --------------------------------------------------
// One set of rules and one row stage (points, max_dist → dist, shape); bvhgpu_nearest_* is k = 1 without limits, and only the
// nearest-first descent takes max_dist.  That descent reads the BvhNode array (a tree built here, flattened or not); the other two walks
// read the flattened arrays.  (A NULL tree is refused without a message here and with one by the later families: kept as it is.)
// sphere (bvhgpu_knearest_sphere_* / _knearest_tree_sphere_*): the shape distance is the sphere's, `kind` is not looked at, and the two kind
// rules are replaced by rule_sphere_array.
enum class PointWalk { Nearest, KNearest, KNearestTree };
template <typename T>
int do_points(bvhgpu_tree* t, PointWalk walk, const T* points, size_t n, int mem, int kind, uint32_t k, const T* max_dist, uint32_t* out_shape, T* out_dist,
              bool sphere = false) {
    if (!t) return BVHGPU_INVALID_ARG;
    bvhgpu_ctx* ctx = t->ctx;
    if (const int rc = settle(t)) return rc;
    if (const int rc = rule_tree_dtype<T>(t, "point")) return rc;
    if (walk == PointWalk::KNearestTree) {
        if (!t->built) return fail(ctx, BVHGPU_INVALID_ARG, "the nearest-first descent needs a tree that was built here (uploaded and imported trees carry no BvhNode array)");
    } else if (const int rc = rule_flattened(t)) {
        return rc;
    }
    if (const int rc = rule_k(ctx, k, BVHGPU_KNN_MAX_K, "BVHGPU_KNN_MAX_K")) return rc;
    if (n && (!points || !out_shape || !out_dist)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (sphere) {
        if (const int rc = rule_sphere_array(t)) return rc;
        kind = POINT_KIND_SPHERE;
    } else {
        if (const int rc = rule_shape_kind(ctx, kind)) return rc;
        if (const int rc = rule_kind_array(t, kind)) return rc;
    }
    if (const int rc = rule_rows_size(ctx, n, k, walk == PointWalk::Nearest ? "too many points in one call" : "too many results (points x k) in one call")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        RowStage st(ctx, mem, {{points, n * 3 * sizeof(T)}, {max_dist, n * sizeof(T)}}, {{out_dist, n * k * sizeof(T)}, {out_shape, n * k * 4}});
        const T* pd = st.at<const T>(0); T* dd = st.at<T>(2); uint32_t* sd = st.at<uint32_t>(3);
        if (walk == PointWalk::KNearestTree) knearest_tree_batch<T>(t, pd, n, kind, k, st.at<const T>(1), sd, dd);
        else if (walk == PointWalk::KNearest) knearest_batch<T>(t, pd, n, kind, k, sd, dd);
        else if (t->n == 0) {   // empty hierarchy → None for every query (flat_bvh.rs:518-520)
            if (n) { BVH_HIP(hipMemsetAsync(sd, 0xFF, n * 4, ctx->stream)); BVH_HIP(hipMemsetAsync(dd, 0, n * sizeof(T), ctx->stream)); }
        } else {
            nearest_batch<T>(t, pd, n, kind, sd, dd);
        }
        st.finish(walk != PointWalk::Nearest);   // k-nearest in HBM: the rows are complete when the call returns, whichever stream reads them next
        return (int)BVHGPU_OK;
    });
}

// ---- multi-hit ray batches: bvhgpu_traverse_khits_* ----------------------------------------------------------------------------------
// do_points' rules and order for rays, on the row stage (rays, tmax → vals, shape); synchronous, and a refused call touches no buffer.
template <typename T>
int do_khits(bvhgpu_tree* t, const typename Traits<T>::Ray* rays, const T* tmax, size_t n, int mem, int leaf, uint32_t k, uint32_t* out_shape, T* out_vals) {
    using Ray = typename Traits<T>::Ray;
    if (!t) return no_tree();
    bvhgpu_ctx* ctx = t->ctx;
    if (const int rc = settle(t)) return rc;
    if (const int rc = rule_tree_dtype<T>(t, "ray")) return rc;
    if (const int rc = rule_flattened(t)) return rc;
    if (const int rc = rule_k(ctx, k, BVHGPU_KHITS_MAX_K, "BVHGPU_KHITS_MAX_K")) return rc;
    if (n && (!rays || !out_shape || !out_vals)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_leaf(ctx, leaf)) return rc;
    if (const int rc = rule_leaf_array(t, leaf)) return rc;
    if (const int rc = rule_rows_size(ctx, n, k, "too many results (rays x k) in one call")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        const size_t w = leaf == BVHGPU_LEAF_TRIANGLE ? 3 : 2;
        RowStage st(ctx, mem, {{rays, n * sizeof(Ray)}, {tmax, n * sizeof(T)}}, {{out_vals, n * k * w * sizeof(T)}, {out_shape, n * k * 4}});
        khits_batch<T>(t, st.at<const Ray>(0), n ? st.at<const T>(1) : nullptr, n, leaf, k, st.at<uint32_t>(3), st.at<T>(2));
        st.finish(true);   // in HBM too the rows are complete when the call returns, whichever stream reads them next
        return (int)BVHGPU_OK;
    });
}

// ---- the rows families on a tree: bvhgpu_traverse_allhits_* / bvhgpu_within_* / bvhgpu_region_* -------------------------------------------
// Each is its own rule list (the later ones were written in the earlier one's order, with their own inputs and flags), then: the main
// input to HBM, the side array or the planes staged in the result object (stage_side / stage_queries), the family's batch (allhits.hip,
// within.hip, region.hip).  The result goes to a result object, whose buffers a later batch of any kind reuses.  A refused call touches no
// buffer and leaves *hits as it was.  (batch_open / batch_refusal do not fit: these families name a NULL tree, and they size the batch last.)
template <typename T>
int do_allhits(bvhgpu_tree* t, const typename Traits<T>::Ray* rays, const T* tmax, size_t n, int mem, int leaf, unsigned flags, bvhgpu_hits** hits) {
    using Ray = typename Traits<T>::Ray;
    if (!t) return no_tree();
    bvhgpu_ctx* ctx = t->ctx;
    if (const int rc = rule_hits_arg(ctx, hits)) return rc;
    if (const int rc = settle(t)) return rc;
    if (const int rc = rule_hits_idle(ctx, hits)) return rc;
    if (const int rc = rule_tree_dtype<T>(t, "ray")) return rc;
    if (const int rc = rule_flattened(t)) return rc;
    if (n && !rays) return fail(ctx, BVHGPU_INVALID_ARG, "rays is NULL");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_leaf(ctx, leaf)) return rc;
    if (flags & ~BVHGPU_ALLHITS_LIST_ORDER) return fail(ctx, BVHGPU_INVALID_ARG, "all-hits flags: 0 or BVHGPU_ALLHITS_LIST_ORDER");
    if (const int rc = rule_leaf_array(t, leaf)) return rc;
    if (const int rc = rule_batch_size(ctx, n, "rays")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        const auto* dev = static_cast<const Ray*>(to_device(ctx, rays, n * sizeof(Ray), mem, ctx->upload));
        const T* td = n ? stage_side<T>(ctx, h, tmax, n, mem) : nullptr;
        allhits_batch<T>(t, dev, td, n, leaf, flags, h);
        return (int)BVHGPU_OK;
    });
}

template <typename T>
int do_within(bvhgpu_tree* t, const T* points, const T* max_dist, size_t n, int mem, int kind, unsigned flags, bvhgpu_hits** hits, bool sphere = false) {
    if (!t) return no_tree();
    bvhgpu_ctx* ctx = t->ctx;
    if (const int rc = rule_hits_arg(ctx, hits)) return rc;
    if (const int rc = settle(t)) return rc;
    if (const int rc = rule_hits_idle(ctx, hits)) return rc;
    if (const int rc = rule_tree_dtype<T>(t, "point")) return rc;
    if (const int rc = rule_flattened(t)) return rc;
    if (n && !points) return fail(ctx, BVHGPU_INVALID_ARG, "points is NULL");
    if (n && !max_dist) return fail(ctx, BVHGPU_INVALID_ARG, "max_dist is NULL");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (!sphere) { if (const int rc = rule_shape_kind(ctx, kind)) return rc; }   // (bvhgpu_within_sphere_*: no kind argument)
    if (flags & ~(BVHGPU_WITHIN_LIST_ORDER | BVHGPU_WITHIN_COUNT_ONLY))
        return fail(ctx, BVHGPU_INVALID_ARG, "within flags: BVHGPU_WITHIN_LIST_ORDER and BVHGPU_WITHIN_COUNT_ONLY only");
    if (const int rc = sphere ? rule_sphere_array(t) : rule_kind_array(t, kind)) return rc;
    if (sphere) kind = POINT_KIND_SPHERE;
    if (const int rc = rule_batch_size(ctx, n, "points")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        const auto* dev = static_cast<const T*>(to_device(ctx, points, n * 3 * sizeof(T), mem, ctx->upload));
        const T* md = n ? stage_side<T>(ctx, h, max_dist, n, mem) : nullptr;
        within_batch<T>(t, dev, md, n, kind, flags, h);
        return (int)BVHGPU_OK;
    });
}

template <typename T>
int do_region(bvhgpu_tree* t, const T* planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits** hits) {
    if (!t) return no_tree();
    bvhgpu_ctx* ctx = t->ctx;
    if (const int rc = rule_hits_arg(ctx, hits)) return rc;
    if (const int rc = settle(t)) return rc;
    if (const int rc = rule_hits_idle(ctx, hits)) return rc;
    if (const int rc = rule_tree_dtype<T>(t, "plane")) return rc;
    if (const int rc = rule_flattened(t)) return rc;
    if (const int rc = rule_planes(ctx, planes, n, m)) return rc;
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (flags & ~(BVHGPU_REGION_COUNT_ONLY | BVHGPU_REGION_CLASSIFY))
        return fail(ctx, BVHGPU_INVALID_ARG, "region flags: BVHGPU_REGION_COUNT_ONLY and BVHGPU_REGION_CLASSIFY only");
    if (const int rc = rule_unfolded(t)) return rc;
    if (const int rc = rule_batch_size(ctx, n, "regions")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        region_batch<T>(t, stage_queries<T>(ctx, h, planes, n * m * 4 * sizeof(T), mem), n, m, flags, h);
        return (int)BVHGPU_OK;
    });
}

// ---- host-resident batches (ABI 7): bvhgpu_traverse_host_* / bvhgpu_build_traverse_host_* -------------------------------------------
// What GpuBvh::traverse_batch of the Rust shim costs a caller whose rays live in host memory and who wants the hit lists back there is a
// PCIe problem, not a kernel problem: 1 M rays are 36 MB as Ray structs and 24 MB as origins + directions, the CSR offsets 4 MB.  The
// batch is cut into chunks (host_batch_upload says how), each an ordinary asynchronous batch on a result object of its own:
//   upload stream  chunk k+1: origins + directions H2D (the copy engines; one transfer per chunk in the OD6 layout)
//   main stream    [the tree's build, if one is in flight: the uploads do not wait for it]  chunk k: Ray::new (k_rays_new: the correctly
//                  rounded divide and square root give the bits Ray::new gives, ray_impl.rs:70-80), the walk + CSR assembly, then the
//                  chunk's index list appended to the batch's and its offsets rebased into the batch's array — through their host
//                  addresses straight into the caller's arrays when those are pinned (BVHGPU_TUNE_HOST_ZERO_COPY bit 1)
//   download stream (result arrays that are NOT pinned) chunk k-1: offsets D2H; behind the last chunk the index lists, as many entries as
//                  the previous batch had hits
// and ONE host wait at the end.  A chunk that had to be replayed (hit pool too small on a first batch, a build that finished on the
// slow path) sends its results again, in one piece.
// the address under which the device sees a host range (pinned: bvhgpu_host_alloc / _register), or NULL for pageable memory
template <typename U> U* dev_visible(U* p) {
    void* d = nullptr;
    if (!p) return nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void*>(static_cast<const void*>(p)), 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return static_cast<U*>(d);
}
constexpr unsigned HOST_READ_BLOCKS = 48;   // workgroups of a kernel that reads pinned host memory: 12 K lanes x 24 B in flight cover the link's latency

void host_batch_init(bvhgpu_ctx* ctx) {
    if (!ctx->host) ctx->host = new HostBatch();
    HostBatch& hb = *ctx->host;
    if (!hb.up) BVH_HIP(hipStreamCreateWithFlags(&hb.up, hipStreamNonBlocking));
    if (!hb.up2) BVH_HIP(hipStreamCreateWithFlags(&hb.up2, hipStreamNonBlocking));
    if (!hb.down) BVH_HIP(hipStreamCreateWithFlags(&hb.down, hipStreamNonBlocking));
    if (!hb.ev_main) BVH_HIP(hipEventCreateWithFlags(&hb.ev_main, hipEventDisableTiming));
    if (!hb.ev_aabbs) BVH_HIP(hipEventCreateWithFlags(&hb.ev_aabbs, hipEventDisableTiming));
    // (the upload streams do NOT wait for the main stream: the previous host batch ended with a wait for everything it had enqueued, and
    //  a build that bvhgpu_rebuild_flat_async_* has just put on the main stream is exactly what the ray upload is meant to run beside)
}

// phase A: the batch's chunks and their uploads (up stream).  Nothing here depends on the tree, so the fused entry
// (bvhgpu_build_traverse_host_*) enqueues it right behind the shapes' upload and BEFORE the build's launches: the ray upload — 24 MB
// against the build's 3 — is the long pole.
template <typename T>
void host_batch_upload(bvhgpu_ctx* ctx, const T* origins, const T* directions, size_t n_rays, bool od6) {
    using Ray = typename Traits<T>::Ray;
    HostBatch& hb = *ctx->host;
    if (od6) directions = origins + 3;
    hb.total = 0; hb.fetched = false; hb.n_rays = n_rays; hb.chunks = 0; hb.with_od = directions != nullptr; hb.od6 = od6;
    if (n_rays == 0) return;
    // Chunks: the walks of all chunks run one after the other on the main stream, each as soon as its rays have arrived; what is
    // left when the last upload ends is the LAST chunk's conversion + walk + offsets download, so the last chunk is the small one
    // (an eighth of the batch, at least 64 K rays: below that the walk's persistent workgroups run half empty) and the others share
    // the rest evenly.  Fewer, larger chunks walk faster in total (1 M rays: 123 µs in one walk, 4 x 47 µs in four).
    const int knob = ctx->tune[BVHGPU_TUNE_HOST_CHUNKS];
    const int want = knob & 0xFF;
    const bool two_up = (knob & 0x100) != 0;   // (experiment: origins and directions on two upload streams)
    int K = want > 0 ? std::min(want, (int)HostBatch::MAX_CHUNKS) : (n_rays >= 524288 ? 3 : (n_rays >= 262144 ? 2 : 1));
    K = (int)std::min<size_t>((size_t)K, std::max<size_t>(n_rays / 32768, 1));
    const size_t last = K > 1 ? std::min(std::max<size_t>(n_rays / 8, 65536), n_rays / (size_t)K) : 0;
    const size_t body = n_rays - last;
    for (int k = 0; k <= K; k++) {
        size_t r = k == K ? n_rays : (k == K - 1 && K > 1 ? body : body * (size_t)k / (size_t)std::max(K - 1, 1));
        if (k != K) r = std::min(n_rays, (r + 1023) & ~(size_t)1023);
        hb.r0[k] = r;
    }
    for (int k = 1; k <= K; k++) hb.r0[k] = std::max(hb.r0[k], hb.r0[k - 1]);
    hb.chunks = K;
    hb.rays.reserve(n_rays * sizeof(Ray));
    hb.offsets.reserve((n_rays + 1) * 4);
    Ray* rays_dev = hb.rays.as<Ray>();
    // pinned ray arrays: the device reads them itself — Ray::new (or a plain copy of the caller's Ray structs) straight out of host memory on
    // the upload stream, one small launch per chunk: no staging buffer, no conversion pass on the main stream, none of the copy engines'
    // 10 - 20 µs between two transfers (seven of them per batch)
    const T* o_vis = (ctx->tune[BVHGPU_TUNE_HOST_ZERO_COPY] & 1) ? dev_visible(origins) : nullptr;
    const T* d_vis = (o_vis && directions) ? (od6 ? o_vis + 3 : dev_visible(directions)) : nullptr;
    hb.zero_copy_in = o_vis && (!directions || d_vis);
    if (directions && !hb.zero_copy_in) hb.od.reserve(2 * n_rays * 3 * sizeof(T));
    for (int k = 0; k < K; k++) {
        const size_t a = hb.r0[k], nk = hb.r0[k + 1] - a;
        if (!hb.ev_up[k]) BVH_HIP(hipEventCreateWithFlags(&hb.ev_up[k], hipEventDisableTiming));
        if (!hb.ev_up2[k]) BVH_HIP(hipEventCreateWithFlags(&hb.ev_up2[k], hipEventDisableTiming));
        if (!hb.ev_done[k]) BVH_HIP(hipEventCreateWithFlags(&hb.ev_done[k], hipEventDisableTiming));
        if (nk && hb.zero_copy_in) {
            if (directions) rays_new<T>(ctx, o_vis + (od6 ? 6 : 3) * a, d_vis + (od6 ? 6 : 3) * a, nk, rays_dev + a, hb.up, HOST_READ_BLOCKS, od6 ? 6u : 3u);
            else copy16(hb.up, reinterpret_cast<const Ray*>(o_vis) + a, rays_dev + a, nk * sizeof(Ray));
        } else if (nk) {
            if (od6) {   // origin and direction of a ray side by side: ONE transfer per chunk
                BVH_HIP(hipMemcpyAsync(hb.od.as<T>() + 6 * a, origins + 6 * a, nk * 6 * sizeof(T), hipMemcpyHostToDevice, hb.up));
            } else if (directions) {
                BVH_HIP(hipMemcpyAsync(hb.od.as<T>() + 3 * a, origins + 3 * a, nk * 3 * sizeof(T), hipMemcpyHostToDevice, hb.up));
                BVH_HIP(hipMemcpyAsync(hb.od.as<T>() + 3 * n_rays + 3 * a, directions + 3 * a, nk * 3 * sizeof(T), hipMemcpyHostToDevice, two_up ? hb.up2 : hb.up));
                if (two_up) { BVH_HIP(hipEventRecord(hb.ev_up2[k], hb.up2)); BVH_HIP(hipStreamWaitEvent(hb.up, hb.ev_up2[k], 0)); }
            } else {   // the caller's own Ray structs (36 / 72 bytes per ray), used as they are
                BVH_HIP(hipMemcpyAsync(rays_dev + a, reinterpret_cast<const Ray*>(origins) + a, nk * sizeof(Ray), hipMemcpyHostToDevice, hb.up));
            }
        }
        BVH_HIP(hipEventRecord(hb.ev_up[k], hb.up));
    }
}

// phase B: per chunk, on the main stream (behind the tree's build if one is in flight): Ray::new, the walk + CSR assembly as an ordinary
// asynchronous batch, the offsets rebased into the batch's array and the index list appended to the batch's; the offsets' download on the
// down stream, the index lists' behind the last chunk — as many entries as the PREVIOUS batch had hits (a frame loop's totals change
// little: the rest, if any, follows after the wait); then ONE host wait
template <typename T>
int host_batch_walk(bvhgpu_tree* tree, unsigned flags, uint32_t* offsets, uint32_t* indices, size_t indices_cap, uint64_t* total) {
    using Ray = typename Traits<T>::Ray;
    bvhgpu_ctx* ctx = tree->ctx;
    HostBatch& hb = *ctx->host;
    const size_t n_rays = hb.n_rays;
    const int K = hb.chunks;
    if (n_rays == 0) {   // (the tree's build, if one is in flight, is completed by whoever looks at the tree next)
        offsets[0] = 0;
        return BVHGPU_OK;
    }
    Ray* rays_dev = hb.rays.as<Ray>();
    uint32_t* offs_all = hb.offsets.as<uint32_t>();
    hipStream_t st = ctx->stream;
    // pinned result arrays: the device writes them itself (k_offsets_rebase / k_indices_append store through the host addresses): no download
    const bool zc_out = (ctx->tune[BVHGPU_TUNE_HOST_ZERO_COPY] & 2) != 0;
    hb.offsets_host = zc_out ? dev_visible(offsets) : nullptr;
    hb.indices_host = (hb.offsets_host && indices && indices_cap) ? dev_visible(indices) : nullptr;
    hb.idx_stage = hb.indices_host ? indices_cap : (indices ? std::min(indices_cap, HostBatch::IDX_STAGE_MAX) : 0);
    if (hb.idx_stage && !hb.indices_host) hb.indices.reserve(hb.idx_stage * 4);
    int enq = 0;
    auto finish_all = [&](bool swallow) {   // every chunk that was enqueued is completed, whatever the first failure was
        bool replayed = false;
        for (int k = 0; k < enq; k++) {
            bvhgpu_hits* h = hb.hits[k];
            if (!swallow) { finish_hits(h); replayed = replayed || h->replays != 0; continue; }
            try { finish_hits(h); } catch (...) { h->pend_async = false; detach_waiter(h); }
        }
        return replayed;
    };
    auto rebase_chunk = [&](int k) {
        const size_t a = hb.r0[k], nk = hb.r0[k + 1] - a;
        offsets_rebase(st, hb.hits[k]->offsets.template as<uint32_t>(), nk, offs_all + a, hb.offsets_host ? hb.offsets_host + a : nullptr,
                       hb.hits[k]->indices.template as<uint32_t>(), hb.indices_host ? hb.indices_host : (hb.idx_stage ? hb.indices.as<uint32_t>() : nullptr),
                       hb.idx_stage, k == 0);
    };
    try {
        for (int k = 0; k < K; k++) {
            const size_t a = hb.r0[k], nk = hb.r0[k + 1] - a;
            BVH_HIP(hipStreamWaitEvent(st, hb.ev_up[k], 0));
            if (hb.with_od && !hb.zero_copy_in) {
                if (hb.od6) rays_new<T>(ctx, hb.od.as<T>() + 6 * a, hb.od.as<T>() + 6 * a + 3, nk, rays_dev + a, st, 0, 6);
                else rays_new<T>(ctx, hb.od.as<T>() + 3 * a, hb.od.as<T>() + 3 * n_rays + 3 * a, nk, rays_dev + a, st);
            }
            const int rc = do_traverse<T>(tree, rays_dev + a, nk, BVHGPU_DEVICE, flags, &hb.hits[k], true);
            if (rc != BVHGPU_OK) { const std::string keep = ctx->err; (void)finish_all(true); (void)hipStreamSynchronize(hb.up); ctx->err = keep; return rc; }
            enq = k + 1;
            rebase_chunk(k);
            if (hb.offsets_host) continue;
            BVH_HIP(hipEventRecord(hb.ev_done[k], st));
            BVH_HIP(hipStreamWaitEvent(hb.down, hb.ev_done[k], 0));
            const size_t skip = k ? 1 : 0;   // (offsets[a] of a later chunk is the previous chunk's last entry)
            if (nk + 1 > skip) BVH_HIP(hipMemcpyAsync(offsets + a + skip, offs_all + a + skip, (nk + 1 - skip) * 4, hipMemcpyDeviceToHost, hb.down));
        }
        uint64_t sent = hb.indices_host ? hb.idx_stage : std::min<uint64_t>(hb.guess, hb.idx_stage);
        if (sent && !hb.indices_host) {
            // (behind the last chunk's append on the main stream — also when the offsets went straight to a pinned array and no chunk
            //  has tied the download stream to the main stream yet)
            BVH_HIP(hipEventRecord(hb.ev_done[K - 1], st));
            BVH_HIP(hipStreamWaitEvent(hb.down, hb.ev_done[K - 1], 0));
            BVH_HIP(hipMemcpyAsync(indices, hb.indices.p, sent * 4, hipMemcpyDeviceToHost, hb.down));
        }
        const bool replayed = finish_all(false);
        BVH_HIP(hipStreamSynchronize(hb.down));
        uint64_t tot = 0;
        for (int k = 0; k < K; k++) tot += hb.hits[k]->total;
        if (tot > 0xFFFFFFFFull) throw HipFail{hipErrorInvalidValue, nullptr, __LINE__, Fail::Overflow};
        if (replayed) {   // what went down came from an incomplete walk: rebase again, one copy
            for (int k = 0; k < K; k++) rebase_chunk(k);
            if (!hb.offsets_host) BVH_HIP(hipMemcpyAsync(offsets, offs_all, (n_rays + 1) * 4, hipMemcpyDeviceToHost, st));
            BVH_HIP(hipStreamSynchronize(st));
            if (!hb.indices_host) sent = 0;
        }
        hb.total = tot;
        hb.guess = tot;
        *total = tot;
        if (indices && tot <= indices_cap) {
            if (hb.indices_host) {
                // (written by the device, all of them: idx_stage == indices_cap >= tot)
            } else if (tot <= hb.idx_stage) {   // the batch's lists are in one piece: whatever the optimistic download did not cover
                if (tot > sent) { BVH_HIP(hipMemcpyAsync(indices + sent, hb.indices.as<uint32_t>() + sent, (tot - sent) * 4, hipMemcpyDeviceToHost, st)); BVH_HIP(hipStreamSynchronize(st)); }
            } else {
                uint64_t base = 0;
                for (int k = 0; k < K; k++) {
                    const uint64_t tk = hb.hits[k]->total;
                    if (tk) BVH_HIP(hipMemcpyAsync(indices + base, hb.hits[k]->indices.p, tk * 4, hipMemcpyDeviceToHost, st));
                    base += tk;
                }
                BVH_HIP(hipStreamSynchronize(st));
            }
            hb.fetched = true;
        }
    } catch (...) {
        (void)finish_all(true);
        (void)hipStreamSynchronize(hb.up); (void)hipStreamSynchronize(hb.up2); (void)hipStreamSynchronize(hb.down);
        throw;
    }
    return BVHGPU_OK;
}

// rebuild == false: the tree as it is (bvhgpu_traverse_host_*).  rebuild: the shapes' AABBs go up first on the upload stream — the
// link is one resource: a second copy beside the rays' would slow both — the rays right behind them, and the main stream builds
// (bvhgpu_rebuild_flat_async_*) as soon as the shapes are there
template <typename T>
int do_traverse_host(bvhgpu_tree* tree, const T* aabbs, size_t n_shapes, bool rebuild, const T* origins, const T* directions, size_t n_rays,
                     unsigned flags, uint32_t* offsets, uint32_t* indices, size_t indices_cap, uint64_t* total) {
    if (!tree) return BVHGPU_INVALID_ARG;
    bvhgpu_ctx* ctx = tree->ctx;
    if (!offsets || !total) return fail(ctx, BVHGPU_INVALID_ARG, "offsets / total is NULL");
    if (n_rays && !origins) return fail(ctx, BVHGPU_INVALID_ARG, "origins is NULL");
    if (flags & ~(BVHGPU_TRAVERSE_COHERENT | BVHGPU_TRAVERSE_RAYS_OD6))
        return fail(ctx, BVHGPU_INVALID_ARG, "bvhgpu_traverse_host_* returns index lists: only BVHGPU_TRAVERSE_COHERENT and BVHGPU_TRAVERSE_RAYS_OD6 may be set");
    const bool od6 = (flags & BVHGPU_TRAVERSE_RAYS_OD6) != 0;
    flags &= ~BVHGPU_TRAVERSE_RAYS_OD6;
    if (tree->dtype != Traits<T>::dtype) return fail(ctx, BVHGPU_DTYPE_MISMATCH, "tree dtype differs from ray / shape dtype");
    if (n_rays >= 0xFFFFFFFFull) return fail(ctx, BVHGPU_OVERFLOW, "more than 2^32-2 rays in one batch");
    if (rebuild && n_shapes && !aabbs) return fail(ctx, BVHGPU_INVALID_ARG, "aabbs is NULL");
    if (rebuild && n_shapes > MAX_SHAPES) return fail(ctx, BVHGPU_OVERFLOW, "too many shapes for u32 flat indices");
    *total = 0;
    return guarded(ctx, [&] {
        use_device(ctx);
        if (rebuild) {   // whatever is in flight on the tree is completed before its shape array is overwritten (as bvhgpu_rebuild_* does)
            ensure_built_ignoring_outcome(tree);
            settle_waiters_impl(tree);
        }
        host_batch_init(ctx);
        HostBatch& hb = *ctx->host;
        if (rebuild && n_shapes) {
            tree->aabbs.reserve(n_shapes * 6 * sizeof(T));
            const T* a_vis = (ctx->tune[BVHGPU_TUNE_HOST_ZERO_COPY] & 1) ? dev_visible(aabbs) : nullptr;
            if (a_vis) copy16(hb.up, a_vis, tree->aabbs.p, n_shapes * 6 * sizeof(T));
            else BVH_HIP(hipMemcpyAsync(tree->aabbs.p, aabbs, n_shapes * 6 * sizeof(T), hipMemcpyHostToDevice, hb.up));
            BVH_HIP(hipEventRecord(hb.ev_aabbs, hb.up));
        }
        host_batch_upload<T>(ctx, origins, directions, n_rays, od6);
        if (rebuild) {
            if (n_shapes) BVH_HIP(hipStreamWaitEvent(ctx->stream, hb.ev_aabbs, 0));
            const int rc = do_build<T>(tree, tree->aabbs.as<T>(), n_shapes, BVHGPU_DEVICE, true, true);
            if (rc != BVHGPU_OK) { (void)hipStreamSynchronize(hb.up); (void)hipStreamSynchronize(hb.up2); return rc; }
        }
        return host_batch_walk<T>(tree, flags, offsets, indices, indices_cap, total);
    });
}

// ---- instanced scenes: bvhgpu_instances_* (instances.hip) ------------------------------------------------------------------------------
// The rules every member tree must pass, rule by rule over all members (the first broken rule wins); create and update share them.
// leaf: the set's kind — the per-shape array every member must hold (BVHGPU_LEAF_BOX: none besides its boxes)
template <typename T> int instances_members_ok(bvhgpu_ctx* ctx, bvhgpu_tree* const* trees, size_t n_trees, int leaf) {
    for (size_t k = 0; k < n_trees; k++) if (!trees[k]) return fail(ctx, BVHGPU_INVALID_ARG, "NULL member tree");
    for (size_t k = 0; k < n_trees; k++)
        if (trees[k]->dtype != Traits<T>::dtype) return fail(ctx, BVHGPU_DTYPE_MISMATCH, "member tree dtype differs from the instance set's");
    for (size_t k = 0; k < n_trees; k++)
        if (trees[k]->ctx != ctx) return fail(ctx, BVHGPU_INVALID_ARG, "member tree belongs to another context");
    for (size_t k = 0; k < n_trees; k++) if (const int rc = settle(trees[k])) return rc;
    for (size_t k = 0; k < n_trees; k++)
        if (!trees[k]->flattened) return fail(ctx, BVHGPU_NOT_FLATTENED, "member tree is not flattened: call bvhgpu_flatten first");
    for (size_t k = 0; k < n_trees; k++) {
        if (leaf == BVHGPU_LEAF_TRIANGLE && !trees[k]->has_tris)
            return fail(ctx, BVHGPU_INVALID_ARG, "instances need bvhgpu_tree_set_triangles on every member tree first");
        if (leaf == BVHGPU_LEAF_SPHERE && !trees[k]->has_spheres)
            return fail(ctx, BVHGPU_INVALID_ARG, "instances of sphere leaves need bvhgpu_tree_set_spheres on every member tree first");
    }
    return BVHGPU_OK;
}
// the pose in the caller's memory becomes the set's own copy and is committed (throws)
template <typename T> void instances_pose(bvhgpu_instances* s, const T* xforms, int mem) {
    bvhgpu_ctx* ctx = s->ctx;
    s->committed = false;
    const size_t bytes = s->n * 12 * sizeof(T);
    if (bytes) {
        s->xforms.reserve(bytes);
        BVH_HIP(hipMemcpyAsync(s->xforms.p, xforms, bytes, mem == BVHGPU_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    }
    instances_commit<T>(s);
}
template <typename T>
int do_instances_create(bvhgpu_ctx* ctx, bvhgpu_tree* const* trees, size_t n_trees, const uint32_t* tree_of, const T* xforms, size_t n, int mem,
                        int leaf, bvhgpu_instances** out) {
    if (!ctx || !out) return fail(ctx, BVHGPU_INVALID_ARG, "ctx/out is NULL");
    *out = nullptr;
    if ((n_trees && !trees) || (n && (!tree_of || !xforms))) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_leaf(ctx, leaf)) return rc;
    if (const int rc = instances_members_ok<T>(ctx, trees, n_trees, leaf)) return rc;
    if (n > MAX_SHAPES || n_trees >= 0xFFFFFFFFull) return fail(ctx, BVHGPU_OVERFLOW, "too many instances for u32 flat indices");
    bvhgpu_instances* s = nullptr;
    const int rc = guarded(ctx, [&] {
        use_device(ctx);
        s = new bvhgpu_instances();
        s->ctx = ctx; s->dtype = Traits<T>::dtype; s->leaf = leaf; s->n = n;
        s->trees.assign(trees, trees + n_trees);
        s->top = new bvhgpu_tree();
        s->top->ctx = ctx; s->top->dtype = Traits<T>::dtype;
        if (n) {   // every instance visible to every ray (bvhgpu_instances_set_masks)
            s->masks.reserve(n * 4);
            BVH_HIP(hipMemsetAsync(s->masks.p, 0xFF, n * 4, ctx->stream));
        }
        if (n) {   // the set's own copy of tree_of, and a look at it on the host
            std::vector<uint32_t> of(n);
            s->tree_of.reserve(n * 4);
            BVH_HIP(hipMemcpyAsync(s->tree_of.p, tree_of, n * 4, mem == BVHGPU_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
            if (mem == BVHGPU_DEVICE) BVH_HIP(hipMemcpyAsync(of.data(), tree_of, n * 4, hipMemcpyDeviceToHost, ctx->stream));
            else std::memcpy(of.data(), tree_of, n * 4);
            BVH_HIP(hipStreamSynchronize(ctx->stream));
            for (size_t i = 0; i < n; i++)
                if (of[i] >= n_trees) return fail(ctx, BVHGPU_INVALID_ARG, "tree_of[i] is not below n_trees");
        }
        instances_pose<T>(s, xforms, mem);
        return (int)BVHGPU_OK;
    });
    if (rc != BVHGPU_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        if (s) { if (s->top) bvhgpu_tree_destroy(s->top); delete s; }
        return rc;
    }
    *out = s;
    return BVHGPU_OK;
}
template <typename T> int do_instances_update(bvhgpu_instances* s, const T* xforms, size_t n, int mem) {
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (n && !xforms) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_set_dtype<T>(s, "transform")) return rc;
    if (const int rc = instances_members_ok<T>(ctx, s->trees.data(), s->trees.size(), s->leaf)) return rc;
    if (n != s->n) return fail(ctx, BVHGPU_INVALID_ARG, "update: the number of instances differs from the set's");
    const int rc = guarded(ctx, [&] { use_device(ctx); instances_pose<T>(s, xforms, mem); return (int)BVHGPU_OK; });
    if (rc != BVHGPU_OK) (void)hipStreamSynchronize(ctx->stream);   // (the set stays uncommitted: instances_pose cleared the mark first)
    return rc;
}
// what every batch over a set asks before anything is launched: a committed pose, and members that are still what the commit read
size_t set_width(const bvhgpu_instances* s) { return s->leaf == BVHGPU_LEAF_TRIANGLE ? 3 : 2; }   // scalars per record of the set's ray families
// the point families measure the distance to a member's triangles: a BOX or SPHERE set has none to measure
int rule_set_triangles(const bvhgpu_instances* s) {
    return s->leaf == BVHGPU_LEAF_TRIANGLE ? (int)BVHGPU_OK
                                           : fail(s->ctx, BVHGPU_INVALID_ARG, "point queries measure triangle distance: the instance set was created with BVHGPU_LEAF_BOX or BVHGPU_LEAF_SPHERE");
}
int rule_committed(const bvhgpu_instances* s) {
    return s->committed ? (int)BVHGPU_OK : fail(s->ctx, BVHGPU_INVALID_ARG, "instances are not committed (the last commit failed): call bvhgpu_instances_update");
}
int instances_current(bvhgpu_instances* s) {
    if (const int rc = rule_committed(s)) return rc;
    for (size_t k = 0; k < s->trees.size(); k++) {   // what the commit read of every member must still be what the member holds
        const bvhgpu_tree* t = s->trees[k];
        const bvhgpu_instances::Seen& c = s->seen[k];
        // the array of the set's kind: where it lives and whether the member still has it (a BOX set reads the boxes alone)
        const void* prims = s->leaf == BVHGPU_LEAF_TRIANGLE ? t->tris.p : (s->leaf == BVHGPU_LEAF_SPHERE ? t->spheres.p : nullptr);
        const bool has = s->leaf == BVHGPU_LEAF_TRIANGLE ? t->has_tris : (s->leaf == BVHGPU_LEAF_SPHERE ? t->has_spheres : true);
        if (t->trav.p != c.trav || t->aabbs.p != c.aabbs || prims != c.prims || t->n != c.n || t->n_trav != c.n_trav || t->gen != c.gen ||
            !t->flattened || !has || t->pending_build || t->pending_recv)
            return fail(s->ctx, BVHGPU_INVALID_ARG, "instances are stale: call bvhgpu_instances_update");
    }
    return BVHGPU_OK;
}
// ---- batches over an instance set ---------------------------------------------------------------------------------------------------------
// The padded-row entries (trace, knearest, khits: the row stage, no result object, synchronous) and the rows entries (region, allhits,
// within: a result object, staged as their tree forms stage).  Every rule list ends with the commit and staleness rules, the refusal of an
// imported member whose navigator boxes were folded away where the walk tests them, and the batch size; the k entries test k first.  A
// refused call touches no buffer and leaves *hits and the set as they were.
// The *_masked_* entries of trace, khits and allhits are the same functions with `masked`: the same rules in the same order, and ray_mask
// (NULL: all ones) staged where the family stages tmax — a column of the row stage, or the result object's side buffer for all-hits.
// Likewise the *_masked_* entries of within, knearest, knearest_tree and region with point_mask / region_mask: a column of the
// row stage for the two padded-row families, the result object's mask buffer (stage_mask) for within and region.
// a HOST mask array of a result-object family → its device pointer in h->maskbuf (every walk of the batch reads it); NULL and DEVICE as they are
const uint32_t* stage_mask(bvhgpu_ctx* ctx, bvhgpu_hits* h, const uint32_t* mask, size_t n, int mem) {
    if (!mask || !n || mem != BVHGPU_HOST) return n ? mask : nullptr;
    h->maskbuf.reserve(n * 4);
    BVH_HIP(hipMemcpyAsync(h->maskbuf.p, mask, n * 4, hipMemcpyHostToDevice, ctx->stream));
    return h->maskbuf.as<uint32_t>();
}
template <typename T>
int do_instances_trace(bvhgpu_instances* s, const typename Traits<T>::Ray* rays, const T* tmax, size_t n, int mem, unsigned flags, T* out_vals,
                       uint32_t* out_instance, uint32_t* out_shape, bool masked = false, const uint32_t* ray_mask = nullptr) {
    using Ray = typename Traits<T>::Ray;
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (n && (!rays || !out_vals || !out_instance || !out_shape)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_set_dtype<T>(s, "ray")) return rc;
    if (flags & ~BVHGPU_TRAVERSE_FIRST) return fail(ctx, BVHGPU_INVALID_ARG, "instance trace flags: 0 or BVHGPU_TRAVERSE_FIRST");
    if (const int rc = instances_current(s)) return rc;
    if (const int rc = rule_batch_size(ctx, n, "rays")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        RowStage st(ctx, mem, {{rays, n * sizeof(Ray)}, {tmax, n * sizeof(T)}, {masked ? ray_mask : nullptr, masked ? n * 4 : 0}},
                    {{out_vals, n * set_width(s) * sizeof(T)}, {out_instance, n * 4}, {out_shape, n * 4}});
        instances_trace<T>(s, st.at<const Ray>(0), n ? st.at<const T>(1) : nullptr, n, (flags & BVHGPU_TRAVERSE_FIRST) != 0, st.at<T>(3), st.at<uint32_t>(4),
                           st.at<uint32_t>(5), masked, n ? st.at<const uint32_t>(2) : nullptr);
        st.finish(true);   // in HBM too the rows are complete when the call returns, whichever stream reads them next
        return (int)BVHGPU_OK;
    });
}
template <typename T>
int do_instances_region(bvhgpu_instances* s, const T* planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits** hits, bool masked = false,
                        const uint32_t* region_mask = nullptr) {
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (const int rc = rule_hits_arg(ctx, hits)) return rc;
    if (const int rc = rule_hits_idle(ctx, hits)) return rc;
    if (const int rc = rule_planes(ctx, planes, n, m)) return rc;
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_set_dtype<T>(s, "plane")) return rc;
    if (flags & ~(BVHGPU_REGION_COUNT_ONLY | BVHGPU_REGION_CLASSIFY | BVHGPU_REGION_INSTANCES_ONLY))
        return fail(ctx, BVHGPU_INVALID_ARG, "instance region flags: BVHGPU_REGION_COUNT_ONLY, BVHGPU_REGION_CLASSIFY and BVHGPU_REGION_INSTANCES_ONLY only");
    if (const int rc = instances_current(s)) return rc;
    if (!(flags & BVHGPU_REGION_INSTANCES_ONLY))   // (the instances' world boxes alone: no member is walked)
        if (const int rc = rule_members_unfolded(s)) return rc;
    if (const int rc = rule_batch_size(ctx, n, "regions")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        const T* dev = stage_queries<T>(ctx, h, planes, n * m * 4 * sizeof(T), mem);
        instances_region_batch<T>(s, dev, n, m, flags, h, masked, masked ? stage_mask(ctx, h, region_mask, n, mem) : nullptr);
        return (int)BVHGPU_OK;
    });
}
template <typename T>
int do_instances_allhits(bvhgpu_instances* s, const typename Traits<T>::Ray* rays, const T* tmax, size_t n, int mem, unsigned flags, bvhgpu_hits** hits,
                         bool masked = false, const uint32_t* ray_mask = nullptr) {
    using Ray = typename Traits<T>::Ray;
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (const int rc = rule_hits_arg(ctx, hits)) return rc;
    if (const int rc = rule_hits_idle(ctx, hits)) return rc;
    if (n && !rays) return fail(ctx, BVHGPU_INVALID_ARG, "rays is NULL");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_set_dtype<T>(s, "ray")) return rc;
    if (flags & ~(BVHGPU_INSTANCES_ALLHITS_LIST_ORDER | BVHGPU_INSTANCES_ALLHITS_COUNT_ONLY))
        return fail(ctx, BVHGPU_INVALID_ARG, "instance all-hits flags: BVHGPU_INSTANCES_ALLHITS_LIST_ORDER and BVHGPU_INSTANCES_ALLHITS_COUNT_ONLY only");
    if (const int rc = instances_current(s)) return rc;
    if (const int rc = rule_batch_size(ctx, n, "rays")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        const auto* dev = static_cast<const Ray*>(to_device(ctx, rays, n * sizeof(Ray), mem, ctx->upload));
        const T* td = n ? stage_side<T>(ctx, h, tmax, n, mem) : nullptr;
        const uint32_t* rm = masked && n ? ray_mask : nullptr;
        if (rm && mem == BVHGPU_HOST) {   // (both walks of the batch read it: it stays in the result object like tmax)
            h->maskbuf.reserve(n * 4);
            BVH_HIP(hipMemcpyAsync(h->maskbuf.p, ray_mask, n * 4, hipMemcpyHostToDevice, ctx->stream));
            rm = h->maskbuf.as<uint32_t>();
        }
        instances_allhits_batch<T>(s, dev, td, n, flags, h, masked, rm);
        return (int)BVHGPU_OK;
    });
}
template <typename T>
int do_instances_within(bvhgpu_instances* s, const T* points, const T* max_dist, size_t n, int mem, unsigned flags, bvhgpu_hits** hits, bool masked = false,
                        const uint32_t* point_mask = nullptr) {
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (const int rc = rule_hits_arg(ctx, hits)) return rc;
    if (const int rc = rule_hits_idle(ctx, hits)) return rc;
    if (n && !points) return fail(ctx, BVHGPU_INVALID_ARG, "points is NULL");
    if (n && !max_dist) return fail(ctx, BVHGPU_INVALID_ARG, "max_dist is NULL");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_set_dtype<T>(s, "point")) return rc;
    if (const int rc = rule_set_triangles(s)) return rc;
    if (flags & ~(BVHGPU_INSTANCES_WITHIN_LIST_ORDER | BVHGPU_INSTANCES_WITHIN_COUNT_ONLY))
        return fail(ctx, BVHGPU_INVALID_ARG, "instance within flags: BVHGPU_INSTANCES_WITHIN_LIST_ORDER and BVHGPU_INSTANCES_WITHIN_COUNT_ONLY only");
    if (const int rc = instances_current(s)) return rc;
    if (const int rc = rule_members_unfolded(s)) return rc;
    if (const int rc = rule_batch_size(ctx, n, "points")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        bvhgpu_hits* h = batch_hits(hits);
        const auto* dev = static_cast<const T*>(to_device(ctx, points, n * 3 * sizeof(T), mem, ctx->upload));
        const T* md = n ? stage_side<T>(ctx, h, max_dist, n, mem) : nullptr;
        instances_within_batch<T>(s, dev, md, n, flags, h, masked, masked ? stage_mask(ctx, h, point_mask, n, mem) : nullptr);
        return (int)BVHGPU_OK;
    });
}
template <typename T>
int do_instances_knearest(bvhgpu_instances* s, const T* points, size_t n, int mem, uint32_t k, uint32_t* out_instance, uint32_t* out_shape, T* out_dist,
                          bool masked = false, const uint32_t* point_mask = nullptr) {
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (const int rc = rule_k(ctx, k, BVHGPU_INSTANCES_KNN_MAX_K, "BVHGPU_INSTANCES_KNN_MAX_K")) return rc;
    if (n && (!points || !out_instance || !out_shape || !out_dist)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_set_dtype<T>(s, "point")) return rc;
    if (const int rc = rule_set_triangles(s)) return rc;
    if (const int rc = instances_current(s)) return rc;   // (a member that lost its triangles is stale)
    if (const int rc = rule_members_unfolded(s)) return rc;
    if (const int rc = rule_rows_size(ctx, n, k, "too many results (points x k) in one call")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        RowStage st(ctx, mem, {{points, n * 3 * sizeof(T)}, {masked ? point_mask : nullptr, masked ? n * 4 : 0}},
                    {{out_dist, n * k * sizeof(T)}, {out_instance, n * k * 4}, {out_shape, n * k * 4}});
        instances_knearest_batch<T>(s, st.at<const T>(0), n, k, st.at<uint32_t>(3), st.at<uint32_t>(4), st.at<T>(2), masked, n ? st.at<const uint32_t>(1) : nullptr);
        st.finish(true);   // in HBM too the rows are complete when the call returns, whichever stream reads them next
        return (int)BVHGPU_OK;
    });
}
// the nearest-first descent reads every member's BvhNode array: rule_members_unfolded's place in the order, another rule
int rule_members_built(const bvhgpu_instances* s) {
    for (const bvhgpu_tree* t : s->trees)
        if (!t->built)
            return fail(s->ctx, BVHGPU_INVALID_ARG, "the nearest-first descent needs the BvhNode array of every member tree: an uploaded, imported or broadcast member carries none (bvhgpu_instances_knearest_* takes such members)");
    return BVHGPU_OK;
}
template <typename T>
int do_instances_knearest_tree(bvhgpu_instances* s, const T* points, size_t n, int mem, uint32_t k, const T* max_dist, uint32_t* out_instance,
                               uint32_t* out_shape, T* out_dist, bool masked = false, const uint32_t* point_mask = nullptr) {
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (const int rc = rule_k(ctx, k, BVHGPU_INSTANCES_KNN_MAX_K, "BVHGPU_INSTANCES_KNN_MAX_K")) return rc;
    if (n && (!points || !out_instance || !out_shape || !out_dist)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_set_dtype<T>(s, "point")) return rc;
    if (const int rc = rule_set_triangles(s)) return rc;
    if (const int rc = instances_current(s)) return rc;   // (a member that lost its triangles is stale)
    if (const int rc = rule_members_built(s)) return rc;
    if (const int rc = rule_rows_size(ctx, n, k, "too many results (points x k) in one call")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        RowStage st(ctx, mem, {{points, n * 3 * sizeof(T)}, {max_dist, n * sizeof(T)}, {masked ? point_mask : nullptr, masked ? n * 4 : 0}},
                    {{out_dist, n * k * sizeof(T)}, {out_instance, n * k * 4}, {out_shape, n * k * 4}});
        instances_knearest_tree_batch<T>(s, st.at<const T>(0), n, k, st.at<const T>(1), st.at<uint32_t>(4), st.at<uint32_t>(5), st.at<T>(3), masked,
                                         n ? st.at<const uint32_t>(2) : nullptr);
        st.finish(true);   // in HBM too the rows are complete when the call returns, whichever stream reads them next
        return (int)BVHGPU_OK;
    });
}
template <typename T>
int do_instances_khits(bvhgpu_instances* s, const typename Traits<T>::Ray* rays, const T* tmax, size_t n, int mem, uint32_t k, uint32_t* out_instance,
                       uint32_t* out_shape, T* out_vals, bool masked = false, const uint32_t* ray_mask = nullptr) {
    using Ray = typename Traits<T>::Ray;
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (const int rc = rule_k(ctx, k, BVHGPU_INSTANCES_KHITS_MAX_K, "BVHGPU_INSTANCES_KHITS_MAX_K")) return rc;
    if (n && (!rays || !out_instance || !out_shape || !out_vals)) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_set_dtype<T>(s, "ray")) return rc;
    if (const int rc = instances_current(s)) return rc;
    if (const int rc = rule_rows_size(ctx, n, k, "too many results (rays x k) in one call")) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        RowStage st(ctx, mem, {{rays, n * sizeof(Ray)}, {tmax, n * sizeof(T)}, {masked ? ray_mask : nullptr, masked ? n * 4 : 0}},
                    {{out_vals, n * k * set_width(s) * sizeof(T)}, {out_instance, n * k * 4}, {out_shape, n * k * 4}});
        instances_khits_batch<T>(s, st.at<const Ray>(0), n ? st.at<const T>(1) : nullptr, n, k, st.at<uint32_t>(4), st.at<uint32_t>(5), st.at<T>(3), masked,
                                 n ? st.at<const uint32_t>(2) : nullptr);
        st.finish(true);   // in HBM too the rows are complete when the call returns, whichever stream reads them next
        return (int)BVHGPU_OK;
    });
}

}  // namespace

namespace bvhgpu {
void settle_waiters(bvhgpu_tree* t) { settle_waiters_impl(t); }   // (comm.hip: a peer's tree is about to be overwritten by a broadcast)
}

#ifdef BVH_PROFILE_MID
namespace bvhgpu { void debug_mid_prof(unsigned long long* out, bool reset); }
#endif
#ifdef BVH_LEVEL_PROFILE
namespace bvhgpu { void debug_level_prof(unsigned long long* out, size_t n); }
#endif
#ifdef BVH_SMALL_PROFILE
namespace bvhgpu { void debug_small_prof(unsigned long long* out, size_t n); }
#endif
#ifdef BVH_WIDE_PROFILE
namespace bvhgpu { void debug_wide_prof(unsigned long long* out, size_t n); void debug_wide_util(unsigned long long* out, size_t n); }
#endif

extern "C" {

int bvhgpu_abi_version(void) { return BVHGPU_ABI_VERSION; }

int bvhgpu_device_count(int* out) {
    if (!out) return BVHGPU_INVALID_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out = 0; (void)hipGetLastError(); return BVHGPU_OK; }
    *out = n;
    return BVHGPU_OK;
}

const char* bvhgpu_status_string(int s) {
    switch (s) {
        case BVHGPU_OK: return "ok";
        case BVHGPU_INVALID_ARG: return "invalid argument";
        case BVHGPU_HIP_ERROR: return "HIP error";
        case BVHGPU_OOM: return "out of memory";
        case BVHGPU_OVERFLOW: return "index overflow";
        case BVHGPU_NO_DEVICE: return "no MI355X / HIP device available";
        case BVHGPU_DTYPE_MISMATCH: return "dtype mismatch";
        case BVHGPU_NOT_FLATTENED: return "tree not flattened";
        case BVHGPU_RCCL_ERROR: return "RCCL error";
        case BVHGPU_REBROADCAST: return "broadcast again";
        default: return "unknown status";
    }
}

int bvhgpu_create(int device, void* stream, bvhgpu_ctx** out) {
    if (!out) return BVHGPU_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(nullptr, BVHGPU_NO_DEVICE, "no HIP device"); }
    if (device < 0 || device >= n) return fail(nullptr, BVHGPU_INVALID_ARG, "device index out of range");
    bvhgpu_ctx* ctx = new bvhgpu_ctx();
    ctx->device = device;
    int rc = guarded(ctx, [&] {
        BVH_HIP(hipSetDevice(device));
        if (stream) { ctx->stream = static_cast<hipStream_t>(stream); ctx->own_stream = false; }
        else { BVH_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
        hipDeviceProp_t prop;
        BVH_HIP(hipGetDeviceProperties(&prop, device));
        ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        for (auto& e : ctx->ev) BVH_HIP(hipEventCreate(&e));
        BVH_HIP(hipHostMalloc(&ctx->pinned, 4096, hipHostMallocDefault));
        return (int)BVHGPU_OK;
    });
    if (rc != BVHGPU_OK) { g_noctx_err = ctx->err; delete ctx; return rc; }
    *out = ctx;
    return BVHGPU_OK;
}

void bvhgpu_destroy(bvhgpu_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
}

const char* bvhgpu_last_error(const bvhgpu_ctx* ctx) { return ctx ? ctx->err.c_str() : g_noctx_err.c_str(); }

int bvhgpu_synchronize(bvhgpu_ctx* ctx) {
    if (!ctx) return BVHGPU_INVALID_ARG;
    return guarded(ctx, [&] { BVH_HIP(hipStreamSynchronize(ctx->stream)); return (int)BVHGPU_OK; });
}

void* bvhgpu_stream(bvhgpu_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int bvhgpu_device_alloc(bvhgpu_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    *out = nullptr;
    return guarded(ctx, [&] { use_device(ctx); BVH_HIP(hipMalloc(out, bytes ? bytes : 1)); return (int)BVHGPU_OK; });
}
int bvhgpu_device_free(bvhgpu_ctx* ctx, void* p) {
    if (!ctx) return BVHGPU_INVALID_ARG;
    if (!p) return BVHGPU_OK;
    return guarded(ctx, [&] { use_device(ctx); BVH_HIP(hipStreamSynchronize(ctx->stream)); BVH_HIP(hipFree(p)); return (int)BVHGPU_OK; });
}
int bvhgpu_device_copy(bvhgpu_ctx* ctx, void* dst, int dst_mem, const void* src, int src_mem, size_t bytes) {
    if (!ctx || (bytes && (!dst || !src))) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if ((dst_mem != BVHGPU_HOST && dst_mem != BVHGPU_DEVICE) || (src_mem != BVHGPU_HOST && src_mem != BVHGPU_DEVICE))
        return fail(ctx, BVHGPU_INVALID_ARG, "bad mem kind");
    return guarded(ctx, [&] {
        use_device(ctx);
        if (bytes) {
            BVH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, ctx->stream));   // (ordered behind the ctx's earlier work)
            BVH_HIP(hipStreamSynchronize(ctx->stream));
        }
        return (int)BVHGPU_OK;
    });
}

// ---- pinned host memory (ABI 7): buffers the DMA engines read and write directly ----
int bvhgpu_host_alloc(bvhgpu_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    *out = nullptr;
    return guarded(ctx, [&] { use_device(ctx); BVH_HIP(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault)); return (int)BVHGPU_OK; });
}
int bvhgpu_host_free(bvhgpu_ctx* ctx, void* p) {
    if (!ctx) return BVHGPU_INVALID_ARG;
    if (!p) return BVHGPU_OK;
    return guarded(ctx, [&] { use_device(ctx); BVH_HIP(hipStreamSynchronize(ctx->stream)); BVH_HIP(hipHostFree(p)); return (int)BVHGPU_OK; });
}
int bvhgpu_host_register(bvhgpu_ctx* ctx, void* p, size_t bytes) {
    if (!ctx || !p || !bytes) return fail(ctx, BVHGPU_INVALID_ARG, "NULL / empty range");
    return guarded(ctx, [&] { use_device(ctx); BVH_HIP(hipHostRegister(p, bytes, hipHostRegisterDefault)); return (int)BVHGPU_OK; });
}
int bvhgpu_host_unregister(bvhgpu_ctx* ctx, void* p) {
    if (!ctx || !p) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    return guarded(ctx, [&] { use_device(ctx); BVH_HIP(hipStreamSynchronize(ctx->stream)); BVH_HIP(hipHostUnregister(p)); return (int)BVHGPU_OK; });
}

int bvhgpu_build_f32(bvhgpu_ctx* ctx, const float* aabbs, size_t n, int mem, bvhgpu_tree** out) {
    return new_build<float>(ctx, aabbs, n, mem, out);
}
int bvhgpu_build_f64(bvhgpu_ctx* ctx, const double* aabbs, size_t n, int mem, bvhgpu_tree** out) {
    return new_build<double>(ctx, aabbs, n, mem, out);
}
int bvhgpu_rebuild_f32(bvhgpu_tree* t, const float* aabbs, size_t n, int mem) { return rebuild<float>(t, aabbs, n, mem, false, false); }
int bvhgpu_rebuild_f64(bvhgpu_tree* t, const double* aabbs, size_t n, int mem) { return rebuild<double>(t, aabbs, n, mem, false, false); }

int bvhgpu_refit_f32(bvhgpu_tree* t, const float* aabbs, size_t n, int mem) { return refit<float>(t, aabbs, n, mem); }
int bvhgpu_refit_f64(bvhgpu_tree* t, const double* aabbs, size_t n, int mem) { return refit<double>(t, aabbs, n, mem); }

// FlatBvh::build (flat_bvh.rs:328-331) = Bvh::build + flatten in one call: one host round trip instead of two
int bvhgpu_build_flat_f32(bvhgpu_ctx* ctx, const float* aabbs, size_t n, int mem, bvhgpu_tree** out) {
    return new_build<float>(ctx, aabbs, n, mem, out, true);
}
int bvhgpu_build_flat_f64(bvhgpu_ctx* ctx, const double* aabbs, size_t n, int mem, bvhgpu_tree** out) {
    return new_build<double>(ctx, aabbs, n, mem, out, true);
}
int bvhgpu_rebuild_flat_f32(bvhgpu_tree* t, const float* aabbs, size_t n, int mem) { return rebuild<float>(t, aabbs, n, mem, true, false); }
int bvhgpu_rebuild_flat_f64(bvhgpu_tree* t, const double* aabbs, size_t n, int mem) { return rebuild<double>(t, aabbs, n, mem, true, false); }

// ---- asynchronous step ----
int bvhgpu_rebuild_flat_async_f32(bvhgpu_tree* t, const float* aabbs, size_t n, int mem) { return rebuild<float>(t, aabbs, n, mem, true, true); }
int bvhgpu_rebuild_flat_async_f64(bvhgpu_tree* t, const double* aabbs, size_t n, int mem) { return rebuild<double>(t, aabbs, n, mem, true, true); }
int bvhgpu_tree_wait(bvhgpu_tree* t) {
    if (!t) return BVHGPU_INVALID_ARG;
    return settle(t);
}
int bvhgpu_traverse_async_f32(bvhgpu_tree* tree, const bvhgpu_ray_f32* rays, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse<float>(tree, rays, n_rays, mem, flags, hits, true);
}
int bvhgpu_traverse_async_f64(bvhgpu_tree* tree, const bvhgpu_ray_f64* rays, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse<double>(tree, rays, n_rays, mem, flags, hits, true);
}
// Completes an asynchronous batch: waits for the stream, completes the tree's asynchronous build if there is one (input
// validation, unbalanced trees) and replays the batch where the optimistic launch was not enough — a tree that was not
// finished when the walk ran, a tree the wide walk must not be used on, a hit pool / stack / heap that was too small.
int bvhgpu_hits_wait(bvhgpu_hits* h) {
    if (!h || !h->ctx) return BVHGPU_INVALID_ARG;
    bvhgpu_ctx* ctx = h->ctx;
    if (!h->pend_async) {   // nothing in flight — or completed meanwhile on behalf of a rebuild / destroy of its tree
        const int rc = h->deferred_rc;
        if (rc != BVHGPU_OK) { ctx->err = h->deferred_err; h->deferred_rc = 0; }
        return rc;
    }
    return guarded(ctx, [&] { use_device(ctx); finish_hits(h); return (int)BVHGPU_OK; });
}

void bvhgpu_tree_destroy(bvhgpu_tree* t) {
    if (!t) return;
    if (t->ctx) { (void)hipSetDevice(t->ctx->device); (void)hipStreamSynchronize(t->ctx->stream); }
    if (!t->waiters.empty()) {   // asynchronous batches still refer to this tree: complete them while it exists
        (void)settle(t);
        settle_waiters_impl(t);
    }
    delete t;
}

int bvhgpu_tree_info(const bvhgpu_tree* t, int* dtype, size_t* n_shapes, size_t* n_nodes, size_t* n_flat) {
    if (!t) return BVHGPU_INVALID_ARG;
    if (dtype) *dtype = t->dtype;
    if (n_shapes) *n_shapes = t->n;
    if (n_nodes) *n_nodes = t->n_nodes;
    if (n_flat) *n_flat = t->n_flat;
    return BVHGPU_OK;
}

int bvhgpu_tree_nodes(bvhgpu_tree* t, void* out, int mem) {
    if (!t) return BVHGPU_INVALID_ARG;
    if (const int rc = settle(t)) return rc;
    if (!t->built) return fail(t->ctx, BVHGPU_INVALID_ARG, "tree has no node array (imported scene)");
    if (t->n_nodes && !out) return fail(t->ctx, BVHGPU_INVALID_ARG, "out is NULL");
    return guarded(t->ctx, [&] {
        use_device(t->ctx);
        size_t sz = t->dtype == BVHGPU_F32 ? sizeof(bvhgpu_node_f32) : sizeof(bvhgpu_node_f64);
        copy_out(t->ctx, out, t->nodes.p, t->n_nodes * sz, mem);
        return (int)BVHGPU_OK;
    });
}

int bvhgpu_tree_shape_nodes(bvhgpu_tree* t, uint32_t* out, int mem) {
    if (!t) return BVHGPU_INVALID_ARG;
    if (const int rc = settle(t)) return rc;
    if (!t->built) return fail(t->ctx, BVHGPU_INVALID_ARG, "tree has no node array (imported scene)");
    if (t->n && !out) return fail(t->ctx, BVHGPU_INVALID_ARG, "out is NULL");
    return guarded(t->ctx, [&] {
        use_device(t->ctx);
        copy_out(t->ctx, out, t->shape_node.p, t->n * 4, mem);
        return (int)BVHGPU_OK;
    });
}

int bvhgpu_tree_build_levels(const bvhgpu_tree* t, int* levels) {
    if (!t || !levels) return BVHGPU_INVALID_ARG;
    if (t->pending_build) if (const int rc = settle(const_cast<bvhgpu_tree*>(t))) return rc;
    *levels = t->levels;
    return BVHGPU_OK;
}

int bvhgpu_flatten(bvhgpu_tree* t) {
    if (!t) return BVHGPU_INVALID_ARG;
    if (const int rc = settle(t)) return rc;
    if (!t->built) return fail(t->ctx, BVHGPU_INVALID_ARG, "tree has no node array (imported scene)");
    bvhgpu_ctx* ctx = t->ctx;
    return guarded(ctx, [&] {
        use_device(ctx);
        if (ctx->timing) BVH_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
        const bool lazy = ctx->tune[BVHGPU_TUNE_FLATTEN_LAZY] != 0;   // (the FlatNode array then follows on first use: bvhgpu_flat_nodes, a binary walk …)
        if (t->dtype == BVHGPU_F32) flatten_tree<float>(t, nullptr, nullptr, 0, nullptr, 0, 0, lazy); else flatten_tree<double>(t, nullptr, nullptr, 0, nullptr, 0, 0, lazy);
        if (ctx->timing) { BVH_HIP(hipEventRecord(ctx->ev[3], ctx->stream)); ctx->ev_set |= 2u; }
        return (int)BVHGPU_OK;
    });
}

int bvhgpu_flat_nodes(bvhgpu_tree* t, void* out, int mem) {
    if (!t) return BVHGPU_INVALID_ARG;
    if (const int rc = settle(t)) return rc;
    if (!t->flattened || !t->built) return fail(t->ctx, BVHGPU_NOT_FLATTENED, "call bvhgpu_flatten first");
    if (t->n_flat && !out) return fail(t->ctx, BVHGPU_INVALID_ARG, "out is NULL");
    return guarded(t->ctx, [&] {
        use_device(t->ctx);
        size_t sz = t->dtype == BVHGPU_F32 ? sizeof(bvhgpu_flat_f32) : sizeof(bvhgpu_flat_f64);
        ensure_flat_arrays(t);
        copy_out(t->ctx, out, t->flat.p, t->n_flat * sz, mem);
        return (int)BVHGPU_OK;
    });
}

int bvhgpu_tree_from_flat_f32(bvhgpu_ctx* ctx, const bvhgpu_flat_f32* flat, size_t n_flat, const float* shape_aabbs, size_t n,
                              bvhgpu_tree** out) {
    return tree_from_flat<float>(ctx, flat, n_flat, shape_aabbs, n, out);
}
int bvhgpu_tree_from_flat_f64(bvhgpu_ctx* ctx, const bvhgpu_flat_f64* flat, size_t n_flat, const double* shape_aabbs, size_t n,
                              bvhgpu_tree** out) {
    return tree_from_flat<double>(ctx, flat, n_flat, shape_aabbs, n, out);
}

// ---- scene blob: header | traversal array | shape AABBs | top-of-tree slot table ----
// exact_only: some split of the tree had no SAH winner (empty child bounds, bvh_node.rs:225-230), so a child box is not the join of its
// grandchildren and the importer must not walk it wide (traverse.hip) — it travels with the tree
struct SceneHeader { uint32_t magic, dtype; uint64_t n, n_trav; uint32_t unfolded, exact_only; uint64_t trav_bytes, aabb_bytes, slot_bytes, tri_bytes; };
static constexpr uint32_t SCENE_MAGIC = 0x42564836u;  // "BVH6" (BVH5 + exact_only)
static size_t slot_table_bytes(int dtype) { return (dtype == BVHGPU_F32 ? TopCfg<float>::SLOTS : TopCfg<double>::SLOTS) * 4; }
static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int bvhgpu_scene_nbytes(const bvhgpu_tree* t, size_t* nbytes) {
    if (!t || !nbytes) return BVHGPU_INVALID_ARG;
    if (!t->flattened) return BVHGPU_NOT_FLATTENED;
    size_t tsz = t->dtype == BVHGPU_F32 ? sizeof(TravNode<float>) : sizeof(TravNode<double>);
    size_t ssz = t->dtype == BVHGPU_F32 ? 4 : 8;
    *nbytes = 256 + align256(t->n_trav * tsz) + align256(t->n * 6 * ssz) + align256(t->slot_entry.p ? slot_table_bytes(t->dtype) : 0) +
              align256(t->has_tris ? t->n * 9 * ssz : 0);
    return BVHGPU_OK;
}

int bvhgpu_scene_export(bvhgpu_tree* t, void* dst, int mem) {
    if (!t || !dst) return BVHGPU_INVALID_ARG;
    if (const int rc = settle(t)) return rc;
    if (!t->flattened) return fail(t->ctx, BVHGPU_NOT_FLATTENED, "call bvhgpu_flatten first");
    bvhgpu_ctx* ctx = t->ctx;
    return guarded(ctx, [&] {
        use_device(ctx);
        ensure_flat_arrays(t);
        size_t tsz = t->dtype == BVHGPU_F32 ? sizeof(TravNode<float>) : sizeof(TravNode<double>);
        size_t ssz = t->dtype == BVHGPU_F32 ? 4 : 8;
        SceneHeader* h = reinterpret_cast<SceneHeader*>(ctx->pinned);
        std::memset(h, 0, 256);
        h->magic = SCENE_MAGIC; h->dtype = (uint32_t)t->dtype; h->n = t->n; h->n_trav = t->n_trav;
        h->unfolded = t->unfolded ? 1u : 0u;
        h->exact_only = t->exact_only ? 1u : 0u;
        h->trav_bytes = t->n_trav * tsz; h->aabb_bytes = t->n * 6 * ssz;
        h->slot_bytes = t->slot_entry.p ? slot_table_bytes(t->dtype) : 0;
        h->tri_bytes = t->has_tris ? t->n * 9 * ssz : 0;
        char* d = static_cast<char*>(dst);
        const hipMemcpyKind kd = mem == BVHGPU_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        BVH_HIP(hipMemcpyAsync(d, h, 256, mem == BVHGPU_DEVICE ? hipMemcpyHostToDevice : hipMemcpyHostToHost, ctx->stream));
        if (h->trav_bytes) BVH_HIP(hipMemcpyAsync(d + 256, t->trav.p, h->trav_bytes, kd, ctx->stream));
        if (h->aabb_bytes) BVH_HIP(hipMemcpyAsync(d + 256 + align256(h->trav_bytes), t->aabbs.p, h->aabb_bytes, kd, ctx->stream));
        if (h->slot_bytes) BVH_HIP(hipMemcpyAsync(d + 256 + align256(h->trav_bytes) + align256(h->aabb_bytes), t->slot_entry.p, h->slot_bytes, kd, ctx->stream));
        if (h->tri_bytes) BVH_HIP(hipMemcpyAsync(d + 256 + align256(h->trav_bytes) + align256(h->aabb_bytes) + align256(h->slot_bytes), t->tris.p, h->tri_bytes, kd, ctx->stream));
        BVH_HIP(hipStreamSynchronize(ctx->stream));  // the pinned header page is reused by the next call
        return (int)BVHGPU_OK;
    });
}

int bvhgpu_scene_import(bvhgpu_ctx* ctx, const void* src, size_t nbytes, int mem, bvhgpu_tree** out) {
    if (!ctx || !out || !src) return fail(ctx, BVHGPU_INVALID_ARG, "NULL argument");
    if (nbytes < 256) return fail(ctx, BVHGPU_INVALID_ARG, "scene blob too small");
    bvhgpu_tree* given = *out;
    if (given && given->ctx == ctx && (given->pending_build || given->pending_recv)) (void)settle(given);   // whatever was in flight is replaced
    if (given && (given->built || given->pending_build || given->ctx != ctx))
        return fail(ctx, BVHGPU_INVALID_ARG, "*out must be NULL or a tree from bvhgpu_scene_import on this ctx");
    if (given) settle_waiters_impl(given);
    bvhgpu_tree* t = given ? given : new bvhgpu_tree();
    t->ctx = ctx;
    int rc = guarded(ctx, [&] {
        use_device(ctx);
        SceneHeader* h = reinterpret_cast<SceneHeader*>(ctx->pinned);
        const char* s = static_cast<const char*>(src);
        BVH_HIP(hipMemcpyAsync(h, s, 256, mem == BVHGPU_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost, ctx->stream));
        BVH_HIP(hipStreamSynchronize(ctx->stream));
        if (h->magic != SCENE_MAGIC || h->dtype > 1 || h->exact_only > 1 || h->unfolded > 1) return fail(ctx, BVHGPU_INVALID_ARG, "not a bvhgpu scene blob (or one of another ABI version)");
        // the header is untrusted: every section size must be what (n, n_trav, dtype) imply, and the sum must fit the blob
        const SceneHeader hd = *h;   // (the pinned page is reused below)
        const uint64_t tsz = hd.dtype == BVHGPU_F32 ? sizeof(TravNode<float>) : sizeof(TravNode<double>);
        const uint64_t ssz = hd.dtype == BVHGPU_F32 ? 4 : 8;
        if (hd.n > MAX_SHAPES || hd.n_trav > 3 * (uint64_t)MAX_SHAPES) return fail(ctx, BVHGPU_INVALID_ARG, "scene blob: shape / entry count out of range");
        if (hd.trav_bytes != hd.n_trav * tsz || hd.aabb_bytes != hd.n * 6 * ssz || (hd.tri_bytes != 0 && hd.tri_bytes != hd.n * 9 * ssz))
            return fail(ctx, BVHGPU_INVALID_ARG, "scene blob: section sizes do not match the shape / entry counts");
        if (hd.slot_bytes && hd.slot_bytes != slot_table_bytes((int)hd.dtype)) return fail(ctx, BVHGPU_INVALID_ARG, "scene blob slot table size");
        if (!hd.unfolded && hd.n_trav != (hd.n >= 2 ? 2 * hd.n - 2 : hd.n)) return fail(ctx, BVHGPU_INVALID_ARG, "scene blob: entry count does not match the shape count");
        {
            uint64_t need = 256;   // sizes are < 2^40 after the checks above: the sum cannot wrap
            for (uint64_t part : {hd.trav_bytes, hd.aabb_bytes, hd.slot_bytes, hd.tri_bytes}) need += align256((size_t)part);
            if (need > nbytes) return fail(ctx, BVHGPU_INVALID_ARG, "scene blob truncated");
        }
        const size_t tb = hd.trav_bytes, ab = hd.aabb_bytes, sb = hd.slot_bytes, gb = hd.tri_bytes;
        t->flattened = false; t->lazy_flat = false;   // until the new arrays are in place
        t->trav.reserve(tb + 16);
        t->aabbs.reserve(ab + 16);
        const hipMemcpyKind kd = mem == BVHGPU_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (tb) BVH_HIP(hipMemcpyAsync(t->trav.p, s + 256, tb, kd, ctx->stream));
        if (ab) BVH_HIP(hipMemcpyAsync(t->aabbs.p, s + 256 + align256(tb), ab, kd, ctx->stream));
        if (sb) { t->slot_entry.reserve(sb); BVH_HIP(hipMemcpyAsync(t->slot_entry.p, s + 256 + align256(tb) + align256(ab), sb, kd, ctx->stream)); }
        else t->slot_entry.release();
        if (gb) { t->tris.reserve(gb); BVH_HIP(hipMemcpyAsync(t->tris.p, s + 256 + align256(tb) + align256(ab) + align256(sb), gb, kd, ctx->stream)); }
        // every copy is enqueued: only now does the tree take the new identity (a failure above leaves a reused tree as it was,
        // apart from buffers that may have grown)
        t->dtype = (int)hd.dtype; t->n = hd.n; t->n_trav = hd.n_trav; t->n_nodes = 0; t->n_flat = 0;
        t->unfolded = hd.unfolded != 0;
        t->has_tris = gb != 0;
        t->has_spheres = false;   // (spheres do not travel in a scene blob: none until bvhgpu_tree_set_spheres_*)
        t->built = false; t->flattened = true; t->exact_only = hd.exact_only != 0;
        t->pending_build = false; t->pending_recv = false; t->gen++;
        if (t->exact_only) t->has_wide = false;   // (never walked wide: no wide nodes needed)
        else if (t->dtype == BVHGPU_F32) wide_from_trav<float>(t); else wide_from_trav<double>(t);
        if (mem != BVHGPU_DEVICE) BVH_HIP(hipStreamSynchronize(ctx->stream));
        return (int)BVHGPU_OK;
    });
    if (rc != BVHGPU_OK) { if (!given) delete t; return rc; }
    *out = t;
    return BVHGPU_OK;
}

// ---- rays ----
int bvhgpu_rays_new_f32(bvhgpu_ctx* ctx, const float* o, const float* d, size_t n, int mem_in, bvhgpu_ray_f32* out, int mem_out) {
    return do_rays_new<float>(ctx, o, d, n, mem_in, out, mem_out);
}
int bvhgpu_rays_new_f64(bvhgpu_ctx* ctx, const double* o, const double* d, size_t n, int mem_in, bvhgpu_ray_f64* out, int mem_out) {
    return do_rays_new<double>(ctx, o, d, n, mem_in, out, mem_out);
}
int bvhgpu_gen_rays_f32(bvhgpu_ctx* ctx, uint64_t first, size_t n, const float bounds[6], bvhgpu_ray_f32* out_dev) { return do_gen_rays(ctx, first, n, bounds, out_dev); }
int bvhgpu_gen_rays_f64(bvhgpu_ctx* ctx, uint64_t first, size_t n, const float bounds[6], bvhgpu_ray_f64* out_dev) { return do_gen_rays(ctx, first, n, bounds, out_dev); }

int bvhgpu_gen_primary_rays_f32(bvhgpu_ctx* ctx, const float cam[14], uint32_t width, uint32_t height, uint64_t first, size_t n,
                                bvhgpu_ray_f32* out_dev) {
    return do_gen_primary<float>(ctx, cam, width, height, first, n, out_dev);
}
int bvhgpu_gen_primary_rays_f64(bvhgpu_ctx* ctx, const float cam[14], uint32_t width, uint32_t height, uint64_t first, size_t n,
                                bvhgpu_ray_f64* out_dev) {
    return do_gen_primary<double>(ctx, cam, width, height, first, n, out_dev);
}
int bvhgpu_nearest_f32(bvhgpu_tree* t, const float* points, size_t n, int mem, int kind, uint32_t* out_shape, float* out_dist) {
    return do_points<float>(t, PointWalk::Nearest, points, n, mem, kind, 1, nullptr, out_shape, out_dist);
}
int bvhgpu_nearest_f64(bvhgpu_tree* t, const double* points, size_t n, int mem, int kind, uint32_t* out_shape, double* out_dist) {
    return do_points<double>(t, PointWalk::Nearest, points, n, mem, kind, 1, nullptr, out_shape, out_dist);
}
int bvhgpu_knearest_f32(bvhgpu_tree* t, const float* points, size_t n, int mem, int kind, uint32_t k, uint32_t* out_shape, float* out_dist) {
    return do_points<float>(t, PointWalk::KNearest, points, n, mem, kind, k, nullptr, out_shape, out_dist);
}
int bvhgpu_knearest_f64(bvhgpu_tree* t, const double* points, size_t n, int mem, int kind, uint32_t k, uint32_t* out_shape, double* out_dist) {
    return do_points<double>(t, PointWalk::KNearest, points, n, mem, kind, k, nullptr, out_shape, out_dist);
}
int bvhgpu_knearest_tree_f32(bvhgpu_tree* t, const float* points, size_t n, int mem, int kind, uint32_t k, const float* max_dist,
                             uint32_t* out_shape, float* out_dist) {
    return do_points<float>(t, PointWalk::KNearestTree, points, n, mem, kind, k, max_dist, out_shape, out_dist);
}
int bvhgpu_knearest_tree_f64(bvhgpu_tree* t, const double* points, size_t n, int mem, int kind, uint32_t k, const double* max_dist,
                             uint32_t* out_shape, double* out_dist) {
    return do_points<double>(t, PointWalk::KNearestTree, points, n, mem, kind, k, max_dist, out_shape, out_dist);
}
int bvhgpu_knearest_sphere_f32(bvhgpu_tree* t, const float* points, size_t n, int mem, uint32_t k, uint32_t* out_shape, float* out_dist) {
    return do_points<float>(t, PointWalk::KNearest, points, n, mem, 0, k, nullptr, out_shape, out_dist, true);
}
int bvhgpu_knearest_sphere_f64(bvhgpu_tree* t, const double* points, size_t n, int mem, uint32_t k, uint32_t* out_shape, double* out_dist) {
    return do_points<double>(t, PointWalk::KNearest, points, n, mem, 0, k, nullptr, out_shape, out_dist, true);
}
int bvhgpu_knearest_tree_sphere_f32(bvhgpu_tree* t, const float* points, size_t n, int mem, uint32_t k, const float* max_dist, uint32_t* out_shape,
                                    float* out_dist) {
    return do_points<float>(t, PointWalk::KNearestTree, points, n, mem, 0, k, max_dist, out_shape, out_dist, true);
}
int bvhgpu_knearest_tree_sphere_f64(bvhgpu_tree* t, const double* points, size_t n, int mem, uint32_t k, const double* max_dist, uint32_t* out_shape,
                                    double* out_dist) {
    return do_points<double>(t, PointWalk::KNearestTree, points, n, mem, 0, k, max_dist, out_shape, out_dist, true);
}
int bvhgpu_traverse_khits_f32(bvhgpu_tree* t, const bvhgpu_ray_f32* rays, const float* tmax, size_t n_rays, int mem, int leaf, uint32_t k,
                              uint32_t* out_shape, float* out_vals) {
    return do_khits<float>(t, rays, tmax, n_rays, mem, leaf, k, out_shape, out_vals);
}
int bvhgpu_traverse_khits_f64(bvhgpu_tree* t, const bvhgpu_ray_f64* rays, const double* tmax, size_t n_rays, int mem, int leaf, uint32_t k,
                              uint32_t* out_shape, double* out_vals) {
    return do_khits<double>(t, rays, tmax, n_rays, mem, leaf, k, out_shape, out_vals);
}
int bvhgpu_traverse_allhits_f32(bvhgpu_tree* t, const bvhgpu_ray_f32* rays, const float* tmax, size_t n_rays, int mem, int leaf, unsigned flags,
                                bvhgpu_hits** hits) {
    return do_allhits<float>(t, rays, tmax, n_rays, mem, leaf, flags, hits);
}
int bvhgpu_traverse_allhits_f64(bvhgpu_tree* t, const bvhgpu_ray_f64* rays, const double* tmax, size_t n_rays, int mem, int leaf, unsigned flags,
                                bvhgpu_hits** hits) {
    return do_allhits<double>(t, rays, tmax, n_rays, mem, leaf, flags, hits);
}
int bvhgpu_within_f32(bvhgpu_tree* t, const float* points, const float* max_dist, size_t n, int mem, int kind, unsigned flags, bvhgpu_hits** hits) {
    return do_within<float>(t, points, max_dist, n, mem, kind, flags, hits);
}
int bvhgpu_within_f64(bvhgpu_tree* t, const double* points, const double* max_dist, size_t n, int mem, int kind, unsigned flags, bvhgpu_hits** hits) {
    return do_within<double>(t, points, max_dist, n, mem, kind, flags, hits);
}
int bvhgpu_within_sphere_f32(bvhgpu_tree* t, const float* points, const float* max_dist, size_t n, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_within<float>(t, points, max_dist, n, mem, 0, flags, hits, true);
}
int bvhgpu_within_sphere_f64(bvhgpu_tree* t, const double* points, const double* max_dist, size_t n, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_within<double>(t, points, max_dist, n, mem, 0, flags, hits, true);
}
int bvhgpu_region_f32(bvhgpu_tree* t, const float* planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_region<float>(t, planes, n, m, mem, flags, hits);
}
int bvhgpu_region_f64(bvhgpu_tree* t, const double* planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_region<double>(t, planes, n, m, mem, flags, hits);
}
int bvhgpu_ray_triangle_pairs_f32(bvhgpu_ctx* ctx, const bvhgpu_ray_f32* rays, const float* tris, size_t n, int mem, float* out) {
    return do_pairs<float>(ctx, rays, tris, n, mem, out);
}
int bvhgpu_ray_triangle_pairs_f64(bvhgpu_ctx* ctx, const bvhgpu_ray_f64* rays, const double* tris, size_t n, int mem, double* out) {
    return do_pairs<double>(ctx, rays, tris, n, mem, out);
}

// ---- traverse ----
int bvhgpu_traverse_f32(bvhgpu_tree* tree, const bvhgpu_ray_f32* rays, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse<float>(tree, rays, n_rays, mem, flags, hits);
}
int bvhgpu_traverse_f64(bvhgpu_tree* tree, const bvhgpu_ray_f64* rays, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse<double>(tree, rays, n_rays, mem, flags, hits);
}

int bvhgpu_traverse_any_f32(bvhgpu_tree* tree, const bvhgpu_ray_f32* rays, const float* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_any<float>(tree, rays, tmax, n_rays, mem, flags, hits);
}
int bvhgpu_traverse_any_f64(bvhgpu_tree* tree, const bvhgpu_ray_f64* rays, const double* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_any<double>(tree, rays, tmax, n_rays, mem, flags, hits);
}

int bvhgpu_traverse_box_f32(bvhgpu_tree* tree, const bvhgpu_ray_f32* rays, const float* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_box<float>(tree, rays, tmax, n_rays, mem, flags, hits);
}
int bvhgpu_traverse_box_f64(bvhgpu_tree* tree, const bvhgpu_ray_f64* rays, const double* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_box<double>(tree, rays, tmax, n_rays, mem, flags, hits);
}

int bvhgpu_traverse_sphere_f32(bvhgpu_tree* tree, const bvhgpu_ray_f32* rays, const float* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_sphere<float>(tree, rays, tmax, n_rays, mem, flags, hits);
}
int bvhgpu_traverse_sphere_f64(bvhgpu_tree* tree, const bvhgpu_ray_f64* rays, const double* tmax, size_t n_rays, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_traverse_sphere<double>(tree, rays, tmax, n_rays, mem, flags, hits);
}

int bvhgpu_query_f32(bvhgpu_tree* tree, int kind, const float* queries, size_t n, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_query<float>(tree, kind, queries, n, mem, flags, hits);
}
int bvhgpu_query_f64(bvhgpu_tree* tree, int kind, const double* queries, size_t n, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_query<double>(tree, kind, queries, n, mem, flags, hits);
}

int bvhgpu_traverse_host_f32(bvhgpu_tree* tree, const float* origins, const float* directions, size_t n_rays, unsigned flags, uint32_t* offsets,
                             uint32_t* indices, size_t indices_cap, uint64_t* total) {
    return do_traverse_host<float>(tree, nullptr, 0, false, origins, directions, n_rays, flags, offsets, indices, indices_cap, total);
}
int bvhgpu_traverse_host_f64(bvhgpu_tree* tree, const double* origins, const double* directions, size_t n_rays, unsigned flags, uint32_t* offsets,
                             uint32_t* indices, size_t indices_cap, uint64_t* total) {
    return do_traverse_host<double>(tree, nullptr, 0, false, origins, directions, n_rays, flags, offsets, indices, indices_cap, total);
}
int bvhgpu_build_traverse_host_f32(bvhgpu_tree* tree, const float* aabbs, size_t n, const float* origins, const float* directions, size_t n_rays,
                                   unsigned flags, uint32_t* offsets, uint32_t* indices, size_t indices_cap, uint64_t* total) {
    return do_traverse_host<float>(tree, aabbs, n, true, origins, directions, n_rays, flags, offsets, indices, indices_cap, total);
}
int bvhgpu_build_traverse_host_f64(bvhgpu_tree* tree, const double* aabbs, size_t n, const double* origins, const double* directions, size_t n_rays,
                                   unsigned flags, uint32_t* offsets, uint32_t* indices, size_t indices_cap, uint64_t* total) {
    return do_traverse_host<double>(tree, aabbs, n, true, origins, directions, n_rays, flags, offsets, indices, indices_cap, total);
}
int bvhgpu_traverse_host_indices(bvhgpu_ctx* ctx, uint32_t* indices, size_t indices_cap) {
    if (!ctx) return BVHGPU_INVALID_ARG;
    HostBatch* hb = ctx->host;
    if (!hb || (hb->n_rays && hb->chunks == 0)) return fail(ctx, BVHGPU_INVALID_ARG, "no completed bvhgpu_traverse_host_* batch on this ctx");
    if (hb->total > indices_cap) return fail(ctx, BVHGPU_INVALID_ARG, "indices_cap is smaller than the batch's hit total");
    if (hb->total && !indices) return fail(ctx, BVHGPU_INVALID_ARG, "indices is NULL");
    return guarded(ctx, [&] {
        use_device(ctx);
        uint64_t base = 0;
        for (int k = 0; k < hb->chunks; k++) {
            const uint64_t tk = hb->hits[k]->total;
            if (tk) BVH_HIP(hipMemcpyAsync(indices + base, hb->hits[k]->indices.p, tk * 4, hipMemcpyDeviceToHost, ctx->stream));
            base += tk;
        }
        BVH_HIP(hipStreamSynchronize(ctx->stream));
        hb->fetched = true;
        return (int)BVHGPU_OK;
    });
}

// bvhgpu_tree_set_triangles_* / bvhgpu_tree_set_spheres_*: one record of `per` scalars per shape (3 vertices; {cx, cy, cz, r}) into a buffer
// of the tree's own — a tree may hold triangles and spheres at once; nothing is validated.  Only the sphere setter tests `mem` (the
// triangle setter, the older one, takes anything but BVHGPU_DEVICE for host memory: kept as it is).
static int set_shape_array(bvhgpu_tree* t, const void* src, size_t n, int mem, int dtype, size_t per, DevBuf bvhgpu_tree::*buf, bool bvhgpu_tree::*has,
                           const char* noun, const char* arg, bool test_mem) {
    if (!t) return BVHGPU_INVALID_ARG;
    bvhgpu_ctx* ctx = t->ctx;
    if (t->dtype != dtype) return fail(ctx, BVHGPU_DTYPE_MISMATCH, std::string(noun) + " dtype differs from tree dtype");
    if (n != t->n) return fail(ctx, BVHGPU_INVALID_ARG, std::string("one ") + noun + " per shape is required");
    if (n && !src) return fail(ctx, BVHGPU_INVALID_ARG, std::string(arg) + " is NULL");
    if (test_mem) if (const int rc = rule_mem(ctx, mem)) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        const size_t bytes = n * per * (dtype == BVHGPU_F32 ? 4 : 8);
        settle_waiters_impl(t);   // (a replay of a batch in flight must see the array it was enqueued with)
        (t->*buf).reserve(bytes + 16);
        if (bytes) {
            BVH_HIP(hipMemcpyAsync((t->*buf).p, src, bytes, mem == BVHGPU_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
            if (mem != BVHGPU_DEVICE) BVH_HIP(hipStreamSynchronize(ctx->stream));
        }
        t->*has = true;
        return (int)BVHGPU_OK;
    });
}
static int set_triangles(bvhgpu_tree* t, const void* verts, size_t n, int mem, int dtype) {
    return set_shape_array(t, verts, n, mem, dtype, 9, &bvhgpu_tree::tris, &bvhgpu_tree::has_tris, "triangle", "verts", false);
}
static int set_spheres(bvhgpu_tree* t, const void* spheres, size_t n, int mem, int dtype) {
    return set_shape_array(t, spheres, n, mem, dtype, 4, &bvhgpu_tree::spheres, &bvhgpu_tree::has_spheres, "sphere", "spheres", true);
}
int bvhgpu_tree_set_triangles_f32(bvhgpu_tree* t, const float* verts, size_t n, int mem) { return set_triangles(t, verts, n, mem, BVHGPU_F32); }
int bvhgpu_tree_set_triangles_f64(bvhgpu_tree* t, const double* verts, size_t n, int mem) { return set_triangles(t, verts, n, mem, BVHGPU_F64); }
int bvhgpu_tree_set_spheres_f32(bvhgpu_tree* t, const float* spheres, size_t n, int mem) { return set_spheres(t, spheres, n, mem, BVHGPU_F32); }
int bvhgpu_tree_set_spheres_f64(bvhgpu_tree* t, const double* spheres, size_t n, int mem) { return set_spheres(t, spheres, n, mem, BVHGPU_F64); }

int bvhgpu_hits_fetch_triangles(bvhgpu_hits* h, void* isect, int mem) {
    if (const int rc = hits_expect(h, true, HitsKind::Csr)) return rc;
    bvhgpu_ctx* ctx = h->ctx;
    if (!(h->flags & BVHGPU_TRAVERSE_TRIANGLES)) return fail(ctx, BVHGPU_INVALID_ARG, "traverse was run without BVHGPU_TRAVERSE_TRIANGLES");
    return guarded(ctx, [&] {
        use_device(ctx);
        if (isect && h->total) copy_out(ctx, isect, h->isect.p, h->total * 3 * (h->dtype == BVHGPU_F32 ? 4 : 8), mem);
        return (int)BVHGPU_OK;
    });
}
// one record per ray (`per_ray` scalars in h->closest, the shape in h->closest_prim) of a batch of the kind `kind`
static int fetch_per_ray(bvhgpu_hits* h, void* values, uint32_t* shape, int mem, HitsKind kind, size_t per_ray) {
    if (const int rc = hits_expect(h, true, kind)) return rc;
    bvhgpu_ctx* ctx = h->ctx;
    return guarded(ctx, [&] {
        use_device(ctx);
        if (values && h->n_rays) copy_out(ctx, values, h->closest.p, h->n_rays * per_ray * (h->dtype == BVHGPU_F32 ? 4 : 8), mem);
        if (shape && h->n_rays) copy_out(ctx, shape, h->closest_prim.p, h->n_rays * 4, mem);
        return (int)BVHGPU_OK;
    });
}
int bvhgpu_hits_fetch_closest(bvhgpu_hits* h, void* isect, uint32_t* shape, int mem) {
    return fetch_per_ray(h, isect, shape, mem, HitsKind::Closest, 3);
}
int bvhgpu_hits_fetch_any(bvhgpu_hits* h, void* isect, uint32_t* shape, int mem) {
    return fetch_per_ray(h, isect, shape, mem, HitsKind::Any, 3);
}
int bvhgpu_hits_fetch_box(bvhgpu_hits* h, void* slice, uint32_t* shape, int mem) {
    return fetch_per_ray(h, slice, shape, mem, HitsKind::Box, 2);
}
int bvhgpu_hits_fetch_sphere(bvhgpu_hits* h, void* slice, uint32_t* shape, int mem) {
    return fetch_per_ray(h, slice, shape, mem, HitsKind::Sphere, 2);
}

int bvhgpu_hits_info(const bvhgpu_hits* h, size_t* n_rays, uint64_t* total, bvhgpu_traverse_stats* stats) {
    if (!h) return BVHGPU_INVALID_ARG;
    if (const int rc = rule_hits_complete(h)) return rc;
    if (n_rays) *n_rays = h->n_rays;
    if (total) *total = h->total;
    if (stats) *stats = h->stats;
    return BVHGPU_OK;
}

int bvhgpu_hits_walk_info(const bvhgpu_hits* h, unsigned* flags) {
    if (!h || !flags) return BVHGPU_INVALID_ARG;
    if (const int rc = rule_hits_complete(h)) return rc;
    *flags = (h->pend_wide || h->pend_qwide ? BVHGPU_WALK_WIDE : 0u) | (h->pend_wide && h->pend_staged ? BVHGPU_WALK_STAGED : 0u) |
             (h->pend_wide && h->pend_rec8 ? BVHGPU_WALK_REC8 : 0u) | (h->pend_wide && h->pend_guide ? BVHGPU_WALK_F64_GUIDE : 0u);
    return BVHGPU_OK;
}

int bvhgpu_hits_walk_kernel(const bvhgpu_hits* h, char* name, size_t cap) {
    if (!h || !name || cap == 0) return BVHGPU_INVALID_ARG;
    std::snprintf(name, cap, "%s", h->walk_kernel.c_str());
    return BVHGPU_OK;
}

// ---- the CSR accessors: bvhgpu_hits_fetch and one per rows kind ------------------------------------------------------------------------------
// An accessor is: the kind its result object must hold (csr_open: hits_expect, then `mem` — which bvhgpu_hits_fetch, the oldest, never
// tested: kept), the kind's own refusals, and ONE csr_copy: the offsets buffer (n_rays + 1 u32) and up to four columns (destination,
// source buffer, bytes per row) of `rows` rows — the batch's total, or none where a COUNT_ONLY batch hands out offsets alone.  Every
// destination may be NULL.  A new rows kind adds a row to HITS_KINDS and an accessor of this shape.
struct CsrCol { void* dst; const DevBuf* src; size_t row_bytes; };
static int csr_open(const bvhgpu_hits* h, HitsKind kind, int mem) {
    if (const int rc = hits_expect(h, true, kind)) return rc;
    return rule_mem(h->ctx, mem);
}
static int csr_copy(bvhgpu_hits* h, int mem, uint32_t* offsets, const DevBuf& offsets_src, size_t rows, std::initializer_list<CsrCol> cols) {
    bvhgpu_ctx* ctx = h->ctx;
    return guarded(ctx, [&] {
        use_device(ctx);
        if (offsets) copy_out(ctx, offsets, offsets_src.p, (h->n_rays + 1) * 4, mem);
        for (const CsrCol& c : cols)
            if (c.dst && rows) copy_out(ctx, c.dst, c.src->p, rows * c.row_bytes, mem);
        return (int)BVHGPU_OK;
    });
}
static size_t scalar_bytes(const bvhgpu_hits* h) { return h->dtype == BVHGPU_F32 ? 4 : 8; }
static size_t rows_unless_count_only(const bvhgpu_hits* h) { return h->count_only ? 0 : (size_t)h->total; }   // (whatever `total` says)

int bvhgpu_hits_fetch(bvhgpu_hits* h, uint32_t* offsets, uint32_t* indices, void* tslice, int mem) {
    if (const int rc = hits_expect(h, true, HitsKind::Csr)) return rc;
    if (tslice && !(h->flags & BVHGPU_TRAVERSE_T_SLICE)) return fail(h->ctx, BVHGPU_INVALID_ARG, "traverse was run without BVHGPU_TRAVERSE_T_SLICE");
    return csr_copy(h, mem, offsets, h->offsets, h->total, {{indices, &h->indices, 4}, {tslice, &h->tslice, 2 * scalar_bytes(h)}});
}
// all-hits: the shapes (u32), the records (W x T)
int bvhgpu_hits_fetch_allhits(bvhgpu_hits* h, uint32_t* offsets, uint32_t* shape, void* vals, int mem) {
    if (const int rc = csr_open(h, HitsKind::Allhits, mem)) return rc;
    const size_t w = h->row_leaf == BVHGPU_LEAF_TRIANGLE ? 3 : 2;
    return csr_copy(h, mem, offsets, h->offsets, h->total, {{shape, &h->indices, 4}, {vals, &h->row_vals, w * scalar_bytes(h)}});
}
// within: the shapes (u32), the distances (T); none of a COUNT_ONLY batch
int bvhgpu_hits_fetch_within(bvhgpu_hits* h, uint32_t* offsets, uint32_t* shape, void* dist, int mem) {
    if (const int rc = csr_open(h, HitsKind::Within, mem)) return rc;
    return csr_copy(h, mem, offsets, h->offsets, rows_unless_count_only(h), {{shape, &h->indices, 4}, {dist, &h->row_vals, scalar_bytes(h)}});
}
// region: offsets of its own, the shapes (u32), the inside bytes (CLASSIFY batches); none of a COUNT_ONLY batch
int bvhgpu_hits_fetch_region(bvhgpu_hits* h, uint32_t* offsets, uint32_t* shape, void* inside, int mem) {
    if (const int rc = csr_open(h, HitsKind::Region, mem)) return rc;
    if (inside && !h->rg_classify) return fail(h->ctx, BVHGPU_INVALID_ARG, "the region batch was run without BVHGPU_REGION_CLASSIFY");
    return csr_copy(h, mem, offsets, h->rg_offsets, rows_unless_count_only(h), {{shape, &h->indices, 4}, {inside, &h->rg_inside, 1}});
}
// region over an instance set (a bvhgpu_region_* result is another kind): the instances and the shapes (u32 each), the inside bytes.  A
// batch with BVHGPU_REGION_INSTANCES_ONLY has no shapes, and its instances are stage 1's rows: where a region result keeps its shapes.
int bvhgpu_hits_fetch_instances_region(bvhgpu_hits* h, uint32_t* offsets, uint32_t* instance, uint32_t* shape, void* inside, int mem) {
    if (const int rc = csr_open(h, HitsKind::InstRegion, mem)) return rc;
    const bool only = h->rg_inst == REGION_INST_ONLY;
    if (inside && !h->rg_classify) return fail(h->ctx, BVHGPU_INVALID_ARG, "the region batch was run without BVHGPU_REGION_CLASSIFY");
    if (shape && only) return fail(h->ctx, BVHGPU_INVALID_ARG, "the region batch was run with BVHGPU_REGION_INSTANCES_ONLY: it has no shapes");
    return csr_copy(h, mem, offsets, h->rg_offsets, rows_unless_count_only(h),
                    {{instance, only ? &h->indices : &h->row_instance, 4}, {shape, &h->indices, 4}, {inside, &h->rg_inside, 1}});
}
// all-hits over an instance set: the instances and the shapes (u32 each), the records (W x T by the set's leaf kind).  A COUNT_ONLY batch refuses every column.
int bvhgpu_hits_fetch_instances_allhits(bvhgpu_hits* h, uint32_t* offsets, uint32_t* instance, uint32_t* shape, void* vals, int mem) {
    if (const int rc = csr_open(h, HitsKind::InstAllhits, mem)) return rc;
    if ((instance || shape || vals) && h->count_only)
        return fail(h->ctx, BVHGPU_INVALID_ARG, "the batch was run with BVHGPU_INSTANCES_ALLHITS_COUNT_ONLY: it has offsets only");
    return csr_copy(h, mem, offsets, h->offsets, h->total, {{instance, &h->row_instance, 4}, {shape, &h->indices, 4}, {vals, &h->row_vals, (h->row_leaf == BVHGPU_LEAF_TRIANGLE ? 3 : 2) * scalar_bytes(h)}});
}
// within over an instance set: the instances and the shapes (u32 each), the distances (T).  A COUNT_ONLY batch refuses every column.
int bvhgpu_hits_fetch_instances_within(bvhgpu_hits* h, uint32_t* offsets, uint32_t* instance, uint32_t* shape, void* dist, int mem) {
    if (const int rc = csr_open(h, HitsKind::InstWithin, mem)) return rc;
    if ((instance || shape || dist) && h->count_only)
        return fail(h->ctx, BVHGPU_INVALID_ARG, "the batch was run with BVHGPU_INSTANCES_WITHIN_COUNT_ONLY: it has offsets only");
    return csr_copy(h, mem, offsets, h->offsets, h->total, {{instance, &h->row_instance, 4}, {shape, &h->indices, 4}, {dist, &h->row_vals, scalar_bytes(h)}});
}

int bvhgpu_hits_region_info(const bvhgpu_hits* h, uint32_t* n_chunks, uint32_t* chunk_entries) {
    if (const int rc = hits_expect(h, false, HitsKind::Region, HitsKind::InstRegion)) return rc;
    if (n_chunks) *n_chunks = h->rg_chunks;
    if (chunk_entries) *chunk_entries = h->rg_chunk_entries;
    return BVHGPU_OK;
}

int bvhgpu_hits_device(const bvhgpu_hits* h, const uint32_t** offsets, const uint32_t** indices, const void** tslice) {
    if (const int rc = hits_expect(h, false, HitsKind::Csr)) return rc;
    if (offsets) *offsets = h->offsets.as<uint32_t>();
    if (indices) *indices = h->indices.as<uint32_t>();
    if (tslice) *tslice = (h->flags & BVHGPU_TRAVERSE_T_SLICE) ? h->tslice.p : nullptr;
    return BVHGPU_OK;
}

void bvhgpu_hits_destroy(bvhgpu_hits* h) {
    if (!h) return;
    if (h->ctx) { (void)hipSetDevice(h->ctx->device); (void)hipStreamSynchronize(h->ctx->stream); }
    detach_waiter(h);   // an asynchronous batch that is never waited for: its tree forgets it
    delete h;
}

int bvhgpu_instances_create_f32(bvhgpu_ctx* ctx, bvhgpu_tree* const* trees, size_t n_trees, const uint32_t* tree_of, const float* xforms, size_t n,
                                int mem, bvhgpu_instances** out) {
    return do_instances_create<float>(ctx, trees, n_trees, tree_of, xforms, n, mem, BVHGPU_LEAF_TRIANGLE, out);
}
int bvhgpu_instances_create_f64(bvhgpu_ctx* ctx, bvhgpu_tree* const* trees, size_t n_trees, const uint32_t* tree_of, const double* xforms, size_t n,
                                int mem, bvhgpu_instances** out) {
    return do_instances_create<double>(ctx, trees, n_trees, tree_of, xforms, n, mem, BVHGPU_LEAF_TRIANGLE, out);
}
int bvhgpu_instances_create_leaf_f32(bvhgpu_ctx* ctx, bvhgpu_tree* const* trees, size_t n_trees, const uint32_t* tree_of, const float* xforms, size_t n,
                                     int mem, int leaf, bvhgpu_instances** out) {
    return do_instances_create<float>(ctx, trees, n_trees, tree_of, xforms, n, mem, leaf, out);
}
int bvhgpu_instances_create_leaf_f64(bvhgpu_ctx* ctx, bvhgpu_tree* const* trees, size_t n_trees, const uint32_t* tree_of, const double* xforms, size_t n,
                                     int mem, int leaf, bvhgpu_instances** out) {
    return do_instances_create<double>(ctx, trees, n_trees, tree_of, xforms, n, mem, leaf, out);
}
int bvhgpu_instances_leaf(const bvhgpu_instances* s, int* leaf) {
    if (!s) return no_set();
    if (leaf) *leaf = s->leaf;
    return BVHGPU_OK;
}
int bvhgpu_instances_update_f32(bvhgpu_instances* s, const float* xforms, size_t n, int mem) { return do_instances_update<float>(s, xforms, n, mem); }
int bvhgpu_instances_update_f64(bvhgpu_instances* s, const double* xforms, size_t n, int mem) { return do_instances_update<double>(s, xforms, n, mem); }
int bvhgpu_instances_trace_f32(bvhgpu_instances* s, const bvhgpu_ray_f32* rays, const float* tmax, size_t n_rays, int mem, unsigned flags,
                               float* out_vals, uint32_t* out_instance, uint32_t* out_shape) {
    return do_instances_trace<float>(s, rays, tmax, n_rays, mem, flags, out_vals, out_instance, out_shape);
}
int bvhgpu_instances_trace_f64(bvhgpu_instances* s, const bvhgpu_ray_f64* rays, const double* tmax, size_t n_rays, int mem, unsigned flags,
                               double* out_vals, uint32_t* out_instance, uint32_t* out_shape) {
    return do_instances_trace<double>(s, rays, tmax, n_rays, mem, flags, out_vals, out_instance, out_shape);
}
int bvhgpu_instances_region_f32(bvhgpu_instances* s, const float* planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_instances_region<float>(s, planes, n, m, mem, flags, hits);
}
int bvhgpu_instances_region_f64(bvhgpu_instances* s, const double* planes, size_t n, uint32_t m, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_instances_region<double>(s, planes, n, m, mem, flags, hits);
}
int bvhgpu_instances_allhits_f32(bvhgpu_instances* s, const bvhgpu_ray_f32* rays, const float* tmax, size_t n_rays, int mem, unsigned flags,
                                 bvhgpu_hits** hits) {
    return do_instances_allhits<float>(s, rays, tmax, n_rays, mem, flags, hits);
}
int bvhgpu_instances_allhits_f64(bvhgpu_instances* s, const bvhgpu_ray_f64* rays, const double* tmax, size_t n_rays, int mem, unsigned flags,
                                 bvhgpu_hits** hits) {
    return do_instances_allhits<double>(s, rays, tmax, n_rays, mem, flags, hits);
}
int bvhgpu_instances_within_f32(bvhgpu_instances* s, const float* points, const float* max_dist, size_t n, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_instances_within<float>(s, points, max_dist, n, mem, flags, hits);
}
int bvhgpu_instances_within_f64(bvhgpu_instances* s, const double* points, const double* max_dist, size_t n, int mem, unsigned flags, bvhgpu_hits** hits) {
    return do_instances_within<double>(s, points, max_dist, n, mem, flags, hits);
}
int bvhgpu_instances_knearest_f32(bvhgpu_instances* s, const float* points, size_t n, int mem, uint32_t k, uint32_t* out_instance, uint32_t* out_shape,
                                  float* out_dist) {
    return do_instances_knearest<float>(s, points, n, mem, k, out_instance, out_shape, out_dist);
}
int bvhgpu_instances_knearest_f64(bvhgpu_instances* s, const double* points, size_t n, int mem, uint32_t k, uint32_t* out_instance, uint32_t* out_shape,
                                  double* out_dist) {
    return do_instances_knearest<double>(s, points, n, mem, k, out_instance, out_shape, out_dist);
}
int bvhgpu_instances_knearest_tree_f32(bvhgpu_instances* s, const float* points, size_t n, int mem, uint32_t k, const float* max_dist,
                                       uint32_t* out_instance, uint32_t* out_shape, float* out_dist) {
    return do_instances_knearest_tree<float>(s, points, n, mem, k, max_dist, out_instance, out_shape, out_dist);
}
int bvhgpu_instances_knearest_tree_f64(bvhgpu_instances* s, const double* points, size_t n, int mem, uint32_t k, const double* max_dist,
                                       uint32_t* out_instance, uint32_t* out_shape, double* out_dist) {
    return do_instances_knearest_tree<double>(s, points, n, mem, k, max_dist, out_instance, out_shape, out_dist);
}
int bvhgpu_instances_khits_f32(bvhgpu_instances* s, const bvhgpu_ray_f32* rays, const float* tmax, size_t n_rays, int mem, uint32_t k,
                               uint32_t* out_instance, uint32_t* out_shape, float* out_vals) {
    return do_instances_khits<float>(s, rays, tmax, n_rays, mem, k, out_instance, out_shape, out_vals);
}
int bvhgpu_instances_khits_f64(bvhgpu_instances* s, const bvhgpu_ray_f64* rays, const double* tmax, size_t n_rays, int mem, uint32_t k,
                               uint32_t* out_instance, uint32_t* out_shape, double* out_vals) {
    return do_instances_khits<double>(s, rays, tmax, n_rays, mem, k, out_instance, out_shape, out_vals);
}
// ---- visibility masks: the set's n u32 and the three ray families that look at them ------------------------------------------
// Not part of the pose: no commit, no look at `committed`, the top level untouched.  Synchronous: the masks are in place on return.
int bvhgpu_instances_set_masks(bvhgpu_instances* s, const uint32_t* masks, size_t n, int mem) {
    if (!s) return fail(nullptr, BVHGPU_INVALID_ARG, "set_masks: NULL instance set");
    bvhgpu_ctx* ctx = s->ctx;
    if (mem != BVHGPU_HOST && mem != BVHGPU_DEVICE) return fail(ctx, BVHGPU_INVALID_ARG, "set_masks: mem must be BVHGPU_HOST or BVHGPU_DEVICE");
    if (n != s->n) return fail(ctx, BVHGPU_INVALID_ARG, "set_masks: the number of masks differs from the set's number of instances");
    return guarded(ctx, [&] {
        use_device(ctx);
        if (n) {
            s->masks.reserve(n * 4);   // (create made it: never a new allocation)
            if (masks) BVH_HIP(hipMemcpyAsync(s->masks.p, masks, n * 4, mem == BVHGPU_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
            else BVH_HIP(hipMemsetAsync(s->masks.p, 0xFF, n * 4, ctx->stream));
        }
        BVH_HIP(hipStreamSynchronize(ctx->stream));
        return (int)BVHGPU_OK;
    });
}
int bvhgpu_instances_masks(bvhgpu_instances* s, uint32_t* out, int mem) {
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (s->n && !out) return fail(ctx, BVHGPU_INVALID_ARG, "out is NULL");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        copy_out(ctx, out, s->masks.p, s->n * 4, mem);
        return (int)BVHGPU_OK;
    });
}
int bvhgpu_instances_trace_masked_f32(bvhgpu_instances* s, const bvhgpu_ray_f32* rays, const float* tmax, const uint32_t* ray_mask, size_t n_rays, int mem,
                                      unsigned flags, float* out_vals, uint32_t* out_instance, uint32_t* out_shape) {
    return do_instances_trace<float>(s, rays, tmax, n_rays, mem, flags, out_vals, out_instance, out_shape, true, ray_mask);
}
int bvhgpu_instances_trace_masked_f64(bvhgpu_instances* s, const bvhgpu_ray_f64* rays, const double* tmax, const uint32_t* ray_mask, size_t n_rays, int mem,
                                      unsigned flags, double* out_vals, uint32_t* out_instance, uint32_t* out_shape) {
    return do_instances_trace<double>(s, rays, tmax, n_rays, mem, flags, out_vals, out_instance, out_shape, true, ray_mask);
}
int bvhgpu_instances_khits_masked_f32(bvhgpu_instances* s, const bvhgpu_ray_f32* rays, const float* tmax, const uint32_t* ray_mask, size_t n_rays, int mem,
                                      uint32_t k, uint32_t* out_instance, uint32_t* out_shape, float* out_vals) {
    return do_instances_khits<float>(s, rays, tmax, n_rays, mem, k, out_instance, out_shape, out_vals, true, ray_mask);
}
int bvhgpu_instances_khits_masked_f64(bvhgpu_instances* s, const bvhgpu_ray_f64* rays, const double* tmax, const uint32_t* ray_mask, size_t n_rays, int mem,
                                      uint32_t k, uint32_t* out_instance, uint32_t* out_shape, double* out_vals) {
    return do_instances_khits<double>(s, rays, tmax, n_rays, mem, k, out_instance, out_shape, out_vals, true, ray_mask);
}
int bvhgpu_instances_allhits_masked_f32(bvhgpu_instances* s, const bvhgpu_ray_f32* rays, const float* tmax, const uint32_t* ray_mask, size_t n_rays, int mem,
                                        unsigned flags, bvhgpu_hits** hits) {
    return do_instances_allhits<float>(s, rays, tmax, n_rays, mem, flags, hits, true, ray_mask);
}
int bvhgpu_instances_allhits_masked_f64(bvhgpu_instances* s, const bvhgpu_ray_f64* rays, const double* tmax, const uint32_t* ray_mask, size_t n_rays, int mem,
                                        unsigned flags, bvhgpu_hits** hits) {
    return do_instances_allhits<double>(s, rays, tmax, n_rays, mem, flags, hits, true, ray_mask);
}
int bvhgpu_instances_within_masked_f32(bvhgpu_instances* s, const float* points, const float* max_dist, const uint32_t* point_mask, size_t n, int mem,
                                       unsigned flags, bvhgpu_hits** hits) {
    return do_instances_within<float>(s, points, max_dist, n, mem, flags, hits, true, point_mask);
}
int bvhgpu_instances_within_masked_f64(bvhgpu_instances* s, const double* points, const double* max_dist, const uint32_t* point_mask, size_t n, int mem,
                                       unsigned flags, bvhgpu_hits** hits) {
    return do_instances_within<double>(s, points, max_dist, n, mem, flags, hits, true, point_mask);
}
int bvhgpu_instances_knearest_masked_f32(bvhgpu_instances* s, const float* points, const uint32_t* point_mask, size_t n, int mem, uint32_t k,
                                         uint32_t* out_instance, uint32_t* out_shape, float* out_dist) {
    return do_instances_knearest<float>(s, points, n, mem, k, out_instance, out_shape, out_dist, true, point_mask);
}
int bvhgpu_instances_knearest_masked_f64(bvhgpu_instances* s, const double* points, const uint32_t* point_mask, size_t n, int mem, uint32_t k,
                                         uint32_t* out_instance, uint32_t* out_shape, double* out_dist) {
    return do_instances_knearest<double>(s, points, n, mem, k, out_instance, out_shape, out_dist, true, point_mask);
}
int bvhgpu_instances_knearest_tree_masked_f32(bvhgpu_instances* s, const float* points, const uint32_t* point_mask, size_t n, int mem, uint32_t k,
                                              const float* max_dist, uint32_t* out_instance, uint32_t* out_shape, float* out_dist) {
    return do_instances_knearest_tree<float>(s, points, n, mem, k, max_dist, out_instance, out_shape, out_dist, true, point_mask);
}
int bvhgpu_instances_knearest_tree_masked_f64(bvhgpu_instances* s, const double* points, const uint32_t* point_mask, size_t n, int mem, uint32_t k,
                                              const double* max_dist, uint32_t* out_instance, uint32_t* out_shape, double* out_dist) {
    return do_instances_knearest_tree<double>(s, points, n, mem, k, max_dist, out_instance, out_shape, out_dist, true, point_mask);
}
int bvhgpu_instances_region_masked_f32(bvhgpu_instances* s, const float* planes, const uint32_t* region_mask, size_t n, uint32_t m, int mem, unsigned flags,
                                       bvhgpu_hits** hits) {
    return do_instances_region<float>(s, planes, n, m, mem, flags, hits, true, region_mask);
}
int bvhgpu_instances_region_masked_f64(bvhgpu_instances* s, const double* planes, const uint32_t* region_mask, size_t n, uint32_t m, int mem, unsigned flags,
                                       bvhgpu_hits** hits) {
    return do_instances_region<double>(s, planes, n, m, mem, flags, hits, true, region_mask);
}
int bvhgpu_instances_boxes(bvhgpu_instances* s, void* out, int mem) {
    if (!s) return no_set();
    bvhgpu_ctx* ctx = s->ctx;
    if (s->n && !out) return fail(ctx, BVHGPU_INVALID_ARG, "out is NULL");
    if (const int rc = rule_mem(ctx, mem)) return rc;
    if (const int rc = rule_committed(s)) return rc;
    return guarded(ctx, [&] {
        use_device(ctx);
        copy_out(ctx, out, s->wboxes.p, s->n * 6 * (s->dtype == BVHGPU_F32 ? 4 : 8), mem);
        return (int)BVHGPU_OK;
    });
}
int bvhgpu_instances_info(const bvhgpu_instances* s, int* dtype, size_t* n_trees, size_t* n_instances) {
    if (!s) return BVHGPU_INVALID_ARG;
    if (dtype) *dtype = s->dtype;
    if (n_trees) *n_trees = s->trees.size();
    if (n_instances) *n_instances = s->n;
    return BVHGPU_OK;
}
// frees what the set owns; the member trees are the caller's and may be gone already: they are not looked at
void bvhgpu_instances_destroy(bvhgpu_instances* s) {
    if (!s) return;
    if (s->ctx) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    if (s->top) bvhgpu_tree_destroy(s->top);
    delete s;
}

int bvhgpu_enable_timing(bvhgpu_ctx* ctx, int on) {
    if (!ctx) return BVHGPU_INVALID_ARG;
    ctx->timing = on != 0;
    return BVHGPU_OK;
}
int bvhgpu_last_timings(bvhgpu_ctx* ctx, bvhgpu_timings* out) {
    if (!ctx || !out) return BVHGPU_INVALID_ARG;
    return guarded(ctx, [&] {
        use_device(ctx);
        BVH_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->ev_set & 1u) (void)hipEventElapsedTime(&ctx->last.build_ms, ctx->ev[0], ctx->ev[1]);
        if (ctx->ev_set & 2u) (void)hipEventElapsedTime(&ctx->last.flatten_ms, ctx->ev[2], ctx->ev[3]);
        if (ctx->ev_set & 4u) {
            (void)hipEventElapsedTime(&ctx->last.traverse_kernel_ms, ctx->ev[4], ctx->ev[5]);
            (void)hipEventElapsedTime(&ctx->last.traverse_total_ms, ctx->ev[4], ctx->ev[6]);
        }
        *out = ctx->last;
        return (int)BVHGPU_OK;
    });
}

int bvhgpu_set_tuning(bvhgpu_ctx* ctx, int knob, int value) {
    if (!ctx || knob < 0 || knob >= BVHGPU_TUNE_COUNT) return BVHGPU_INVALID_ARG;
    ctx->tune[knob] = value;
    return BVHGPU_OK;
}
int bvhgpu_get_tuning(const bvhgpu_ctx* ctx, int knob, int* value) {
    if (!ctx || !value || knob < 0 || knob >= BVHGPU_TUNE_COUNT) return BVHGPU_INVALID_ARG;
    *value = ctx->tune[knob];
    return BVHGPU_OK;
}

#ifdef BVH_LEVEL_PROFILE
void bvhgpu_debug_level_prof(unsigned long long* out, size_t n) { bvhgpu::debug_level_prof(out, n); }
#endif
#ifdef BVH_WIDE_PROFILE
void bvhgpu_debug_wide_prof(unsigned long long* out, size_t n) { bvhgpu::debug_wide_prof(out, n); }
void bvhgpu_debug_wide_util(unsigned long long* out, size_t n) { bvhgpu::debug_wide_util(out, n); }
#endif
#ifdef BVH_SMALL_PROFILE
void bvhgpu_debug_small_prof(unsigned long long* out, size_t n) { bvhgpu::debug_small_prof(out, n); }
#endif
#ifdef BVH_PROFILE_MID
void bvhgpu_debug_mid_prof(unsigned long long* out, int reset) { bvhgpu::debug_mid_prof(out, reset != 0); }
#endif

}  // extern "C"

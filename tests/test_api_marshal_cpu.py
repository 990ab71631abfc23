"""bvh_amd/api.py only marshals: what it hands to the C ABI is the whole of its behaviour.  This module replaces `_lib.load` with a fake
library that records every call, runs every public method of Context, RayBatch, _Hits, _TreeBase, FlatBvh and Bvh (f32 and f64, 4 rays or
points on 7 shapes, host inputs and duck-typed device tensors where no torch output is allocated) and compares, per scenario,
  * the call log: (entry point, normalised arguments) — integers as they are, pointers as NULL / PTR, byref outputs as OUT, and for host
    inputs whose length follows from the other arguments (points, max_dist, tmax, AABBs, queries, triangles, spheres) the values read
    back through the pointer, so that a wrong reshape or scalar broadcast shows,
  * the shapes and dtypes of what is returned,
  * the error raised (type, status, message),
with tests/golden/api_calls.json.  Needs no GPU and no libbvh_mi355x.so.  In the log an entry point of the tree's dtype reads `_T` for its
suffix and that dtype reads `T`, so the file holds an f64 record only where it differs from the f32 one.

The recording is made by this file's __main__ and only ever from the api.py that precedes a change of the marshalling code:
    python tests/test_api_marshal_cpu.py [path/to/api_calls.json]
run in a checkout of that earlier commit (this file copied into its tests/); the changed api.py must reproduce the file unedited."""
from __future__ import annotations

import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bvh_amd import _lib, api  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "api_calls.json")
N, NSHAPES = 4, 7
_BYREF = type(C.byref(C.c_int()))

# host inputs whose length follows from the other arguments: entry stem → [(pointer arg, count arg, mem arg or None, scalars per row)]
_INPUTS = {
    "build": [(1, 2, 3, 6)], "rebuild": [(1, 2, 3, 6)], "rebuild_flat": [(1, 2, 3, 6)], "rebuild_flat_async": [(1, 2, 3, 6)],
    "refit": [(1, 2, 3, 6)], "rays_new": [(1, 3, 4, 3), (2, 3, 4, 3)], "nearest": [(1, 2, 3, 3)], "knearest": [(1, 2, 3, 3)],
    "knearest_tree": [(1, 2, 3, 3), (6, 2, 3, 1)], "within": [(1, 3, 4, 3), (2, 3, 4, 1)], "traverse_any": [(2, 3, 4, 1)],
    "traverse_box": [(2, 3, 4, 1)], "traverse_sphere": [(2, 3, 4, 1)], "traverse_khits": [(2, 3, 4, 1)], "traverse_allhits": [(2, 3, 4, 1)],
    "tree_set_triangles": [(1, 2, 3, 9)], "tree_set_spheres": [(1, 2, 3, 4)], "tree_from_flat": [(3, 4, None, 6)],
    "ray_triangle_pairs": [(2, 3, 4, 9)], "build_traverse_host": [(1, 2, None, 6)],
}


class FakeLib:
    """every bvhgpu_* symbol: log (name, normalised args), fill the outputs a caller reads, answer BVHGPU_OK"""

    def __init__(self):
        self.log = []
        self.sfx, self.dtype_code, self.devices = "f32", _lib.F32, 1
        self._mem = []          # what bvhgpu_host_alloc handed out

    def __getattr__(self, name):
        if not name.startswith("bvhgpu_"):
            raise AttributeError(name)

        def fn(*args):
            shown = name[7:-3] + "T" if name.endswith("_" + self.sfx) else name[7:]     # (an entry of the other dtype keeps its suffix)
            self.log.append(f"{shown}({','.join(str(self._norm(a)) for a in args)})" + "".join(self._values(name[7:], args)))
            return self._answer(name[7:], args)
        return fn

    @staticmethod
    def _norm(a):
        if a is None:
            return "NULL"
        if isinstance(a, (bool, int, np.integer)):
            return int(a)
        if isinstance(a, C.c_void_p):      # (D: a stand-in tensor's own memory, Dc: that of its contiguous() copy)
            return {None: "NULL", 0: "NULL", FakeTensor.PTR: "D", FakeTensor.PTR_CONTIGUOUS: "Dc"}.get(a.value, "P")
        if isinstance(a, _BYREF):
            return "OUT"
        if isinstance(a, C.Array):
            return "BUF"
        if isinstance(a, C._SimpleCData):
            return f"{type(a).__name__}:{a.value}"
        return repr(type(a))

    @staticmethod
    def _values(name, args):
        stem, _, sfx = name.rpartition("_")
        if sfx not in ("f32", "f64"):
            return []
        dt = np.float32 if sfx == "f32" else np.float64
        specs = list(_INPUTS.get(stem, []))
        if stem == "query":
            specs = [(2, 3, 4, _lib.QUERY_WIDTH.get(args[1], 1))]
        if stem in ("traverse_host", "build_traverse_host"):      # origins [, directions] or [o, d] rows; Ray structs are not read back
            o = 1 if stem == "traverse_host" else 3
            od6 = args[o + 3] & _lib.TRAVERSE_RAYS_OD6
            specs += [(o, o + 2, None, 6)] if od6 else [(o, o + 2, None, 3), (o + 1, o + 2, None, 3)] if args[o + 1] is not None else []
        out = []
        for p, n, mem, w in specs:
            a = args[p]
            if not isinstance(a, C.c_void_p) or not a.value or (mem is not None and args[mem] != _lib.HOST) or not 0 < int(args[n]) * w <= 256:
                continue
            raw = (C.c_char * (int(args[n]) * w * np.dtype(dt).itemsize)).from_address(a.value)
            out.append(" [" + " ".join(f"{x:g}" for x in np.frombuffer(raw, dtype=dt).tolist()) + "]")
        return out

    def _answer(self, name, args):
        def put(i, v):
            if i < len(args) and isinstance(args[i], _BYREF):
                args[i]._obj.value = v
        if name == "device_count":
            put(0, self.devices)
        elif name == "create":
            put(2, 0x1000)
        elif name.startswith(("build_f", "build_flat_f", "tree_from_flat_", "scene_import")):
            put(len(args) - 1, 0x2000)
        elif name == "tree_info":
            put(1, self.dtype_code), put(2, NSHAPES), put(3, 13), put(4, 19)
        elif name == "hits_info":
            put(2, 5)
            if isinstance(args[3], _BYREF):
                st = args[3]._obj
                st.hits, st.visited, st.leaf_visits, st.device_steps, st.wave_steps = 11, 12, 13, 14, 15
        elif name == "hits_walk_info":
            put(1, 3)
        elif name == "hits_walk_kernel":
            args[1].value = b"k_fake"
        elif name == "host_alloc":
            self._mem.append((C.c_char * args[1])())
            put(2, C.addressof(self._mem[-1]))
        elif name in ("scene_nbytes", "get_tuning", "tree_build_levels"):
            put(len(args) - 1, 42)
        elif name.startswith(("traverse_host_f", "build_traverse_host_f")):
            put(len(args) - 1, 5)
        elif name.startswith(("traverse_", "query_", "within_")):
            if isinstance(args[-1]._obj if isinstance(args[-1], _BYREF) else None, C.c_void_p):
                put(len(args) - 1, 0x3000)      # the result object's handle
        elif name in ("last_error", "status_string"):
            return b""
        elif name == "abi_version":
            return _lib.ABI_VERSION
        return _lib.OK


class FakeDtype:
    def __init__(self, name):
        self.name = name

    def __str__(self):
        return "torch." + self.name

    def __eq__(self, o):
        return str(self) == str(o)

    def __ne__(self, o):
        return str(self) != str(o)

    __hash__ = None


class FakeTensor:
    """what api.py reads of a torch GPU tensor: data_ptr, is_cuda, dtype, contiguous, numel, device.  It stands for a strided tensor:
    contiguous() answers a copy at another address, so the log tells whether a call site took the tensor as it was"""
    is_cuda = True
    device = "cuda:0"
    PTR, PTR_CONTIGUOUS = 0xD000, 0xC000

    def __init__(self, name, numel, ptr=PTR):
        self.dtype, self._n, self._ptr = FakeDtype(name), numel, ptr

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n

    def contiguous(self):
        return FakeTensor(self.dtype.name, self._n, self.PTR_CONTIGUOUS)


class Shape(api.BHShape):
    def __init__(self, i):
        self.i, self.node = i, None

    def aabb(self):
        return api.Aabb([self.i, 0, 0], [self.i + 0.5, 1, 1])

    def set_bh_node_index(self, index):
        self.node = index

    def bh_node_index(self):
        return self.node

    def __repr__(self):
        return f"Shape{self.i}"


TREE_DTYPE = "float32"      # (run_all sets it: the tree's dtype reads "T" in a description, so that most f64 records equal the f32 ones)


def describe(v):
    """shapes and dtypes of a return value"""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, np.ndarray):
        return f"{v.dtype if v.dtype.names is None else 'struct%d' % v.dtype.itemsize}{list(v.shape)}".replace(TREE_DTYPE, "T")
    if isinstance(v, np.generic):
        return f"{v.dtype}:{v.item()}".replace(TREE_DTYPE, "T")
    if isinstance(v, dict):
        return " ".join(f"{k}={describe(v[k])}" for k in v)
    if isinstance(v, (tuple, list)):
        return [describe(x) for x in v]
    if isinstance(v, (api._TreeBase, api.RayBatch)):
        return f"{type(v).__name__}:{v.sfx}"
    return type(v).__name__ if not isinstance(v, Shape) else repr(v)


class Env:
    def __init__(self, lib, sfx):
        self.lib, self.sfx = lib, sfx
        self.ft = ft = np.float32 if sfx == "f32" else np.float64
        self.other = np.float64 if sfx == "f32" else np.float32
        self.tname, self.oname = ("float32", "float64") if sfx == "f32" else ("float64", "float32")
        lib.sfx, lib.dtype_code = sfx, _lib.F32 if sfx == "f32" else _lib.F64
        self.ctx = api.Context(0)
        api._default_ctx = self.ctx
        self.aabbs = (np.arange(NSHAPES * 6) * 0.25).astype(ft).reshape(NSHAPES, 6)
        self.bvh = api.Bvh.from_aabbs(self.aabbs, self.ctx)
        self.flat = self.bvh.flatten()
        self.up = api.FlatBvh.from_flat_nodes(np.zeros(19, dtype=_lib.FLAT_F32 if sfx == "f32" else _lib.FLAT_F64), self.aabbs, self.ctx)
        self.o = (np.arange(N * 3) * 0.5).astype(ft).reshape(N, 3)
        self.d = (1 + np.arange(N * 3) * 0.25).astype(ft).reshape(N, 3)
        self.rays = api.RayBatch.new(self.o, self.d, ft, self.ctx)
        self.orays = api.RayBatch(N, self.other, host=np.zeros(N, dtype=api._ray_dtype("f64" if sfx == "f32" else "f32")))
        self.drays = api.RayBatch.from_device(self.dev(N * 9), N, ft)
        self.ray = api.Ray([0, 0.5, 1], [1, 0, 0], ft, self.ctx)
        self.pts = (np.arange(N * 3) * 0.25 - 1).astype(ft).reshape(N, 3)
        self.tmax = (1 + np.arange(N) * 0.5).astype(ft)
        self.md = (2 + np.arange(N) * 0.25).astype(ft)
        self.tris = (np.arange(NSHAPES * 9) * 0.125).astype(ft).reshape(NSHAPES, 3, 3)
        self.sph = (np.arange(NSHAPES * 4) * 0.5).astype(ft).reshape(NSHAPES, 4)
        self.shapes = [Shape(i) for i in range(NSHAPES)]

    def dev(self, numel, wrong=False):
        return FakeTensor(self.oname if wrong else self.tname, numel)

    def trees(self):
        return [("bvh", self.bvh), ("flat", self.flat)]


def scenarios(E):
    """[(name, callable)] in the order they run; every callable takes no argument"""
    S = []

    def add(name, fn):
        S.append((name, fn))
    ft, other, ctx = E.ft, E.other, E.ctx
    # ---- Context ---------------------------------------------------------------------------------------------------------------
    add("ctx.new_stream", lambda: api.Context(1, stream=0x77).close())
    add("ctx.synchronize", ctx.synchronize)
    add("ctx.enable_timing", lambda: (ctx.enable_timing(), ctx.enable_timing(False)))
    add("ctx.last_timings", ctx.last_timings)
    add("ctx.set_tuning", lambda: ctx.set_tuning(3, 9))
    add("ctx.get_tuning", lambda: ctx.get_tuning(3))
    add("ctx.close.deferred", lambda: _deferred_close())

    def no_device():
        E.lib.devices = 0
        try:
            return api.Context(0)
        finally:
            E.lib.devices = 1
    add("ctx.new_no_device", no_device)

    def _deferred_close():
        c = api.Context(0)
        t = api.Bvh.from_aabbs(E.aabbs, c)
        c.close()
        t.close()
    add("default_context", lambda: api.default_context() is ctx)
    # ---- RayBatch, Ray, free functions -------------------------------------------------------------------------------------------
    add("rays.new", lambda: (lambda r: (r, r.mem, r.n, describe(r.host)))(api.RayBatch.new(E.o.tolist(), E.d, ft, ctx)))
    add("rays.new_other_dtype_in", lambda: api.RayBatch.new(E.o.astype(other), E.d.astype(other), ft, ctx))
    add("rays.new_length", lambda: api.RayBatch.new(E.o, E.d[:3], ft, ctx))
    add("rays.from_device", lambda: (lambda r: (r, r.mem, r.n, r.device_ptr))(api.RayBatch.from_device(E.dev(N * 9), N, ft)))
    add("rays.generate", lambda: api.RayBatch.generate(5, N, [0, 0, 0, 1, 2, 3], E.dev(N * 9), ft, ctx))
    add("rays.primary", lambda: api.RayBatch.primary(api.camera([0, 0, 0], [0, 0, 1]), 2, 2, 0, N, E.dev(N * 9), ft, ctx))
    add("rays.mem", lambda: (E.rays.mem, E.drays.mem))
    add("rays.bad_dtype", lambda: api.RayBatch(N, np.int32))
    add("rays._ptr", lambda: (E.rays._ptr() is not None, E.drays._ptr().value))
    add("ray.new", lambda: (lambda r: (r.origin, r.direction, r.inv_direction, str(r.dtype)))(api.Ray.new([0, 0, 0], [0, 0, 1], ft)))
    add("ray.intersects_aabb", lambda: E.ray.intersects_aabb(api.Aabb([0, 0, 0], [1, 1, 1])))
    add("ray.intersection_slice_for_aabb", lambda: E.ray.intersection_slice_for_aabb(api.Aabb([0, 0, 0], [1, 1, 1])))
    add("ray.intersects_triangle", lambda: E.ray.intersects_triangle([0, 0, 0], [1, 0, 0], [0, 1, 0]))
    add("intersect_triangle_pairs", lambda: api.intersect_triangle_pairs(E.rays, E.tris[:N], ctx))
    add("intersect_triangle_pairs_length", lambda: api.intersect_triangle_pairs(E.rays, E.tris[:3], ctx))
    add("intersect_triangle_pairs_device", lambda: api.intersect_triangle_pairs(E.drays, E.tris[:N], ctx))
    add("pinned_array", lambda: api.pinned_array(ctx, (3, 6), ft))
    for od6 in (False, True):
        for fused in (True, False):
            def host_step(od6=od6, fused=fused):
                hs = api.HostStep(E.bvh, NSHAPES, N, ft, index_cap=2 if od6 else None, od6=od6)
                hs.aabbs[:] = E.aabbs
                hs.origins[:] = E.o
                hs.directions[:] = E.d
                r = hs.run(coherent=od6, fused=fused)
                hs.close()
                return r
            add(f"host_step.od6={od6}.fused={fused}", host_step)
    # ---- _Hits ---------------------------------------------------------------------------------------------------------------------
    h = E.flat._hits
    add("hits.wait", h.wait)
    add("hits.info", h.info)
    add("hits.walk_kernel", h.walk_kernel)
    add("hits.walk_flags", h.walk_flags)
    for f in ("fetch_closest", "fetch_any", "fetch_box", "fetch_sphere"):
        add(f"hits.{f}", lambda f=f: getattr(h, f)(N, ft))
        add(f"hits.{f}.default_dtype", lambda f=f: getattr(h, f)(N))
    add("hits.fetch_triangles", lambda: h.fetch_triangles(ft))
    add("hits.fetch", lambda: h.fetch(N))
    for leaf in ("box", "triangle", "sphere"):
        add(f"hits.fetch_allhits.{leaf}", lambda leaf=leaf: h.fetch_allhits(N, leaf, ft))
    add("hits.fetch_allhits.default", lambda: h.fetch_allhits(N))
    add("hits.fetch_allhits.bad_leaf", lambda: h.fetch_allhits(N, "cone", ft))
    for co in (False, True):
        add(f"hits.fetch_within.count_only={co}", lambda co=co: h.fetch_within(N, ft, None, co))
    add("hits.fetch_within.default", lambda: h.fetch_within(N))
    add("hits.close", lambda: (lambda x: (x.close(), x.close(), x.h))(api._Hits(ctx)))
    # ---- every tree method, on a Bvh (flattens first where the flat walk needs it) and on its flat view -----------------------------
    for tn, t in E.trees():
        def T(name, fn, both=False, tn=tn):
            if both or tn == "flat":      # the Bvh inherits every method: it runs the plain form, the refusals and what flattens first
                add(f"{tn}.{name}", fn)
        T("info", t.info)
        for kw in ({}, {"want_t": True}, {"stats": True}, {"fetch": False}, {"coherent": True}, {"order": "nearest"}, {"order": "farthest"},
                   {"order": "nearest_heap"}, {"order": "farthest_heap"}, {"order": "sideways"},
                   {"want_t": True, "stats": True, "coherent": True, "order": "nearest"}):
            tag = ",".join(f"{k}={v}" for k, v in kw.items())
            T(f"traverse_batch({tag})", lambda t=t, kw=kw: t.traverse_batch(E.rays, **kw), both=not kw)
            if "want_t" not in kw and kw.get("order") in (None, "farthest_heap", "sideways"):
                if "fetch" not in kw:
                    T(f"intersect_triangles({tag})", lambda t=t, kw=kw: t.intersect_triangles(E.rays, **kw))
                T(f"closest_hits({tag})", lambda t=t, kw=kw: t.closest_hits(E.rays, **kw), both=not kw)
        T("traverse_batch.device_rays", lambda t=t: t.traverse_batch(E.drays))
        T("traverse_batch.ray_dtype", lambda t=t: t.traverse_batch(E.orays))
        T("traverse_async", lambda t=t: t.traverse_async(E.drays) is t._hits)
        T("traverse_async.flags_hits", lambda t=t: (lambda own: t.traverse_async(E.drays, own, 17) is own)(api._Hits(ctx)))
        T("traverse_async.ray_dtype", lambda t=t: t.traverse_async(E.orays))
        T("set_triangles", lambda t=t: t.set_triangles(E.tris), both=True)
        T("set_triangles.n9_list", lambda t=t: t.set_triangles(E.tris.reshape(-1, 9).tolist()))
        T("set_triangles.other_dtype", lambda t=t: t.set_triangles(E.tris.astype(other)))
        T("set_triangles.device", lambda t=t: t.set_triangles(E.dev(NSHAPES * 9)))
        T("set_triangles.device_other_dtype", lambda t=t: t.set_triangles(E.dev(NSHAPES * 9, wrong=True)))
        T("set_spheres", lambda t=t: t.set_spheres(E.sph))
        T("set_spheres.list", lambda t=t: t.set_spheres(E.sph.tolist()))
        T("set_spheres.other_dtype", lambda t=t: t.set_spheres(E.sph.astype(other)))
        T("set_spheres.device", lambda t=t: t.set_spheres(E.dev(NSHAPES * 4)))
        T("set_spheres.device_other_dtype", lambda t=t: t.set_spheres(E.dev(NSHAPES * 4, wrong=True)))
        tmaxes = {"none": (E.rays, None), "array": (E.rays, E.tmax), "list": (E.rays, E.tmax.tolist()), "scalar": (E.rays, 2.0),
                  "other_dtype": (E.rays, E.tmax.astype(other)), "length": (E.rays, E.tmax[:3]), "2d": (E.rays, E.tmax.reshape(2, 2)),
                  "device_on_host_rays": (E.rays, E.dev(N)), "host_on_device_rays": (E.drays, E.tmax), "device": (E.drays, E.dev(N)),
                  "device_other_dtype": (E.drays, E.dev(N, wrong=True)), "device_length": (E.drays, E.dev(N + 1)),
                  "none_device_rays": (E.drays, None), "ray_dtype": (E.orays, None)}
        for m in ("any_hits", "closest_box_hits", "first_box_hits", "closest_sphere_hits", "first_sphere_hits"):
            for tag, (rays, tm) in tmaxes.items():
                if m == "any_hits" or tag in ("array", "ray_dtype") or (tag in ("none", "length", "device") and m.startswith("closest")):     # (one _tmax_arg: its cases run once)
                    T(f"{m}.tmax={tag}", lambda t=t, m=m, rays=rays, tm=tm: getattr(t, m)(rays, tm), both=m == "any_hits" and tag == "array")
            T(f"{m}.fetch=False", lambda t=t, m=m: getattr(t, m)(E.rays, E.tmax, fetch=False))
            T(f"{m}.device.fetch=False.coherent", lambda t=t, m=m: getattr(t, m)(E.drays, E.dev(N), False, True))
        for m in ("occluded", "box_occluded", "sphere_occluded"):
            T(m, lambda t=t, m=m: getattr(t, m)(E.rays), both=m == "occluded")
            T(f"{m}.tmax", lambda t=t, m=m: getattr(t, m)(E.rays, E.tmax))
        for k in (1, 3, 0, 65):
            T(f"khits_batch.k={k}", lambda t=t, k=k: t.khits_batch(E.rays, k), both=k == 3)
            T(f"knearest_batch.k={k}", lambda t=t, k=k: t.knearest_batch(E.pts, k), both=k == 3)
            T(f"knearest_tree_batch.k={k}", lambda t=t, k=k: t.knearest_tree_batch(E.pts, k), both=k == 3)
        for leaf in ("box", "triangle", "sphere", "cone"):
            T(f"khits_batch.leaf={leaf}", lambda t=t, leaf=leaf: t.khits_batch(E.rays, 3, leaf, E.tmax), both=leaf == "cone")
            T(f"allhits_batch.leaf={leaf}", lambda t=t, leaf=leaf: t.allhits_batch(E.rays, leaf), both=leaf in ("box", "cone"))
        for tag in ("list", "other_dtype", "length", "device_on_host_rays", "ray_dtype"):
            T(f"khits_batch.tmax={tag}", lambda t=t, a=tmaxes[tag]: t.khits_batch(a[0], 2, "box", a[1]), both=tag == "ray_dtype")
            T(f"allhits_batch.tmax={tag}", lambda t=t, a=tmaxes[tag]: t.allhits_batch(a[0], "box", a[1]))
        T("allhits_batch.tmax.sort=False", lambda t=t: t.allhits_batch(E.rays, "triangle", E.tmax, False))
        T("nearest_batch", lambda t=t: t.nearest_batch(E.pts), both=True)
        T("nearest_batch.triangles.list", lambda t=t: t.nearest_batch(E.pts.tolist(), True))
        T("nearest_batch.other_dtype", lambda t=t: t.nearest_batch(E.pts.astype(other)))
        T("nearest_batch.flat_input", lambda t=t: t.nearest_batch(E.pts.reshape(-1)))
        T("knearest_batch.triangles.list", lambda t=t: t.knearest_batch(E.pts.tolist(), 2, True))
        T("knearest_batch.other_dtype", lambda t=t: t.knearest_batch(E.pts.astype(other), 2), both=True)
        T("knearest_batch.noncontiguous", lambda t=t: t.knearest_batch(np.asfortranarray(E.pts), 2))
        limits = {"none": None, "scalar": 1.5, "int_scalar": 2, "np_scalar": ft(0.75), "array": E.md, "list": E.md.tolist(),
                  "other_dtype": E.md.astype(other), "length": E.md[:3], "2d": E.md.reshape(2, 2), "device": E.dev(N)}
        for tag, md in limits.items():
            T(f"knearest_tree_batch.max_dist={tag}", lambda t=t, md=md: t.knearest_tree_batch(E.pts, 2, False, md))
            T(f"within_batch.max_dist={tag}", lambda t=t, md=md: t.within_batch(E.pts, md), both=tag in ("none", "scalar", "length"))
        T("knearest_tree_batch.triangles.list", lambda t=t: t.knearest_tree_batch(E.pts.tolist(), 2, True, 1.0))
        T("knearest_tree_batch.other_dtype", lambda t=t: t.knearest_tree_batch(E.pts.astype(other), 2))
        T("within_batch.other_dtype", lambda t=t: t.within_batch(E.pts.astype(other), 1.0), both=True)
        T("within_batch.list.triangles", lambda t=t: t.within_batch(E.pts.tolist(), 1.0, True))
        T("within_batch.sort=False", lambda t=t: t.within_batch(E.pts, E.md, sort=False))
        T("within_batch.count_only", lambda t=t: t.within_batch(E.pts, E.md, count_only=True))
        T("within_batch.all_flags", lambda t=t: t.within_batch(E.pts, 0.5, True, False, True))
        # points in HBM: every refusal comes before an output is allocated, so the stand-in tensor reaches it
        dpts = {"host_max_dist": (E.dev(N * 3), E.md), "point_dtype": (E.dev(N * 3, wrong=True), E.dev(N)),
                "max_dist_dtype": (E.dev(N * 3), E.dev(N, wrong=True)), "max_dist_length": (E.dev(N * 3), E.dev(N + 1)),
                "host_list_max_dist": (E.dev(N * 3), E.md.tolist())}
        for tag, (dp, md) in dpts.items():
            T(f"within_batch.device_points.{tag}", lambda t=t, dp=dp, md=md: t.within_batch(dp, md), both=tag == "host_max_dist")
            T(f"knearest_tree_batch.device_points.{tag}", lambda t=t, dp=dp, md=md: t.knearest_tree_batch(dp, 2, False, md))
        T("within_batch.device_points.no_max_dist", lambda t=t: t.within_batch(E.dev(N * 3), None))
        T("knearest_batch.device_points.point_dtype", lambda t=t: t.knearest_batch(E.dev(N * 3, wrong=True), 2), both=True)
        T("nearest_to", lambda t=t: t.nearest_to([0.5, 0.25, 0], E.shapes), both=True)
        T("nearest_to.triangles", lambda t=t: t.nearest_to([0.5, 0.25, 0], E.shapes, True))
        for m in ("nearest_traverse", "farthest_traverse", "nearest_child_traverse", "farthest_child_traverse"):
            T(m, lambda t=t, m=m: getattr(t, m)(E.ray, E.shapes), both=m == "nearest_traverse")
        T("hits_device", t.hits_device)
        queries = {"ray": E.ray, "aabb": api.Aabb([0, 0, 0], [1, 2, 3]), "ball": api.Ball([1, 2, 3], 0.5), "point": [0.5, 1, 1.5],
                   "point_array": np.array([1, 2, 3], dtype=other), "bad": [1, 2]}
        for tag, q in queries.items():
            T(f"traverse.{tag}", lambda t=t, q=q: t.traverse(q, E.shapes), both=tag in ("ray", "point", "bad"))
        q6 = (np.arange(N * 6) * 0.5).astype(ft).reshape(N, 6)
        for kind, code, w in (("aabb", _lib.QUERY_AABB, 6), ("point", _lib.QUERY_POINT, 3), ("ball", _lib.QUERY_BALL, 4), ("sphere", 3, 4)):
            qs = np.ascontiguousarray(q6[:, :w])
            T(f"query_batch.{kind}", lambda t=t, kind=kind, qs=qs: t.query_batch(kind, qs), both=kind == "ball")
            if kind != "sphere":
                T(f"query_batch.{kind}.code.list", lambda t=t, code=code, qs=qs: t.query_batch(code, qs.tolist()))
                T(f"query_batch.{kind}.device.fetch=False", lambda t=t, kind=kind, w=w: t.query_batch(kind, E.dev(N * w), fetch=False))
        T("query_batch.none", lambda t=t: t.query_batch("aabb", None))
        T("query_batch.fetch=False", lambda t=t: t.query_batch("point", E.pts, False))
        T("query_batch.other_dtype", lambda t=t: t.query_batch("point", E.pts.astype(other)), both=True)
        T("query_batch.device_other_dtype", lambda t=t: t.query_batch("point", E.dev(N * 3, wrong=True)))
        T("query_batch.unknown_kind", lambda t=t: t.query_batch(9, E.pts))
        ragged = np.arange(7).astype(ft)        # no whole number of rows
        T("query_batch.ragged", lambda t=t: t.query_batch("point", ragged))
        T("query_batch.ragged.device", lambda t=t: t.query_batch("point", E.dev(7), fetch=False))
        T("knearest_batch.ragged", lambda t=t: _raises(ValueError, lambda: t.knearest_batch(ragged, 2)))
        T("nearest_batch.ragged", lambda t=t: _raises(ValueError, lambda: t.nearest_batch(ragged)))
        T("within_batch.ragged", lambda t=t: _raises(ValueError, lambda: t.within_batch(ragged, 1.0)))
        T("set_spheres.ragged", lambda t=t: _raises(ValueError, lambda: t.set_spheres(ragged)))
        T("set_triangles.ragged", lambda t=t: _raises(ValueError, lambda: t.set_triangles(ragged)))
        T("set_triangles.ragged.device", lambda t=t: t.set_triangles(E.dev(20)))
        T("self_overlaps", t.self_overlaps, both=True)
        T("self_overlaps.fetch=False", lambda t=t: t.self_overlaps(False))
        T("query_kernel", t.query_kernel)
        T("scene_nbytes", t.scene_nbytes)
        T("scene_export.host", lambda t=t: t.scene_export(np.zeros(42, dtype=np.uint8)))
        T("scene_export.device", lambda t=t: t.scene_export(E.dev(42)))
    # ---- FlatBvh ---------------------------------------------------------------------------------------------------------------------
    add("flat.build", lambda: (lambda f: (f, type(f).__name__, [s.node for s in E.shapes]))(api.FlatBvh.build(E.shapes, ft, ctx)))
    add("flat.build_par", lambda: api.FlatBvh.build_par(E.shapes, ft, ctx))
    add("flat.nodes", lambda: E.flat.nodes)
    add("flat.len", lambda: len(E.flat))
    add("flat.from_flat_nodes", lambda: (lambda f: (f, type(f).__name__))(
        api.FlatBvh.from_flat_nodes(np.zeros(19, dtype=_lib.FLAT_F32 if E.sfx == "f32" else _lib.FLAT_F64), E.aabbs.astype(other).tolist(), ctx)))
    add("flat.scene_import.host", lambda: api.FlatBvh.scene_import(np.zeros(42, dtype=np.uint8), 42, ctx))
    add("flat.scene_import.device", lambda: api.FlatBvh.scene_import(E.dev(42), 42, ctx))
    add("flat.scene_import.reuse", lambda: (lambda r: api.FlatBvh.scene_import(E.dev(42), 42, ctx, reuse=r) is r)(E.up))
    add("flat.uploaded.within_batch", lambda: E.up.within_batch(E.pts, 1.0))
    add("flat.uploaded.khits_batch", lambda: E.up.khits_batch(E.rays, 2))
    add("flat.close", lambda: (lambda f: (f.close(), f._t))(E.bvh.flatten()))
    # ---- Bvh -------------------------------------------------------------------------------------------------------------------------
    for tag, a in (("same", E.aabbs), ("other", E.aabbs.astype(other)), ("int", np.arange(12).reshape(2, 6)), ("list", E.aabbs[:2].tolist()),
                   ("flat_input", E.aabbs.reshape(-1)), ("empty", np.zeros((0, 6), dtype=ft))):
        add(f"bvh.from_aabbs.{tag}", lambda a=a: api.Bvh.from_aabbs(a, ctx))
    add("bvh.from_aabbs.default_ctx", lambda: api.Bvh.from_aabbs(E.aabbs))
    for fl in (False, True):
        add(f"bvh.rebuild.flatten={fl}", lambda fl=fl: E.bvh.rebuild(E.aabbs, fl) is E.bvh)
        add(f"bvh.rebuild.flatten={fl}.other_dtype.list", lambda fl=fl: (E.bvh.rebuild(E.aabbs.astype(other), fl), E.bvh.rebuild(E.aabbs.tolist(), fl)))
        add(f"bvh.rebuild.flatten={fl}.device", lambda fl=fl: E.bvh.rebuild(E.dev(NSHAPES * 6), flatten=fl))
    add("bvh.rebuild.device_other_dtype", lambda: E.bvh.rebuild(E.dev(NSHAPES * 6, wrong=True)))
    add("bvh.rebuild.ragged", lambda: _raises(ValueError, lambda: E.bvh.rebuild(E.aabbs.reshape(-1)[:7])))
    add("bvh.refit.ragged", lambda: _raises(ValueError, lambda: E.bvh.refit(E.aabbs.reshape(-1)[:7])))
    add("bvh.from_aabbs.ragged", lambda: _raises(ValueError, lambda: api.Bvh.from_aabbs(E.aabbs.reshape(-1)[:7], ctx)))
    add("bvh.refit", lambda: E.bvh.refit(E.aabbs) is E.bvh)
    add("bvh.refit.other_dtype.list", lambda: (E.bvh.refit(E.aabbs.astype(other)), E.bvh.refit(E.aabbs.tolist())))
    add("bvh.refit.device", lambda: E.bvh.refit(E.dev(NSHAPES * 6)))
    add("bvh.refit.device_other_dtype", lambda: E.bvh.refit(E.dev(NSHAPES * 6, wrong=True)))

    def pinned():
        a = api.pinned_array(ctx, (NSHAPES, 6), ft)
        a[:] = E.aabbs
        return a
    add("bvh.rebuild_async.pinned", lambda: E.bvh.rebuild_async(pinned()) is E.bvh)
    add("bvh.rebuild_async.device", lambda: E.bvh.rebuild_async(E.dev(NSHAPES * 6)) is E.bvh)
    add("bvh.rebuild_async.pageable", lambda: E.bvh.rebuild_async(E.aabbs))
    add("bvh.rebuild_async.list", lambda: E.bvh.rebuild_async(E.aabbs.tolist()))
    off, idx = np.zeros(N + 1, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    od = np.ascontiguousarray(np.concatenate([E.o, E.d], axis=1))
    add("bvh.traverse_host", lambda: E.bvh.traverse_host(E.o, E.d, off, idx))
    add("bvh.traverse_host.coherent.aabbs", lambda: E.bvh.traverse_host(E.o, E.d, off, idx, coherent=True, aabbs=E.aabbs))
    add("bvh.traverse_host.ray_structs", lambda: E.bvh.traverse_host(E.rays.host, None, off, idx))
    add("bvh.traverse_host.od6", lambda: E.bvh.traverse_host(od, None, off, idx, od6=True))
    add("bvh.traverse_host.od6.aabbs", lambda: E.bvh.traverse_host(od, None, off, idx, False, E.aabbs, True))
    add("bvh.traverse_host.other_dtype", lambda: E.bvh.traverse_host(E.o.astype(other), E.d.astype(other), off, idx))
    add("bvh.traverse_host.small_offsets", lambda: E.bvh.traverse_host(E.o, E.d, off[:N], idx))
    add("bvh.traverse_host.aabbs_other_dtype", lambda: E.bvh.traverse_host(E.o, E.d, off, idx, aabbs=E.aabbs.astype(other)))
    add("bvh.traverse_host_indices", lambda: E.bvh.traverse_host_indices(idx))
    add("bvh.wait", lambda: E.bvh.wait() is E.bvh)
    for m in ("build", "build_par"):
        add(f"bvh.{m}", lambda m=m: (lambda b: (b, [s.node for s in E.shapes]))(getattr(api.Bvh, m)(E.shapes, ft, ctx)))
    add("bvh.build.empty", lambda: api.Bvh.build([], ft, ctx))
    add("bvh.build_with_executor", lambda: api.Bvh.build_with_executor(E.shapes, object(), ft, ctx))
    add("bvh.nodes", lambda: E.bvh.nodes)
    add("bvh.shape_nodes", lambda: E.bvh.shape_nodes)
    add("bvh.build_levels", lambda: E.bvh.build_levels)
    add("bvh.flatten", lambda: (lambda f: (f, type(f).__name__, f._owner is E.bvh, f._hits is E.bvh._hits))(E.bvh.flatten()))
    add("bvh.flatten_in_place", E.bvh.flatten_in_place)
    add("bvh.close", lambda: (lambda b: (b.close(), b.close(), b._t))(api.Bvh.from_aabbs(E.aabbs, ctx)))
    return S


def _raises(exc, fn):
    """(numpy's own messages are not part of the record)"""
    try:
        fn()
    except exc:
        return exc.__name__
    return "no error"


def _close_all(before):
    for kind in ("_Hits", "tree", "Context"):
        for obj in list(api._live):
            k = type(obj).__name__
            if id(obj) not in before and ((kind == "tree" and k not in ("_Hits", "Context")) or k == kind):
                try:
                    obj.close()
                except Exception:
                    pass


def run_all():
    """{sfx: {scenario: {"calls": [...], "ret": ..., "err": ...}}} against the api module that is importable now"""
    global TREE_DTYPE
    real_load, real_ctx = _lib.load, api._default_ctx
    before = {id(o) for o in api._live}
    out = {}
    try:
        for sfx in ("f32", "f64"):
            lib = FakeLib()
            TREE_DTYPE = "float32" if sfx == "f32" else "float64"
            _lib.load = lambda lib=lib: lib
            E = Env(lib, sfx)
            out[sfx] = {"setup": {"calls": lib.log}}
            for name, fn in scenarios(E):
                assert name not in out[sfx], name
                lib.log = []
                rec = out[sfx][name] = {}
                try:
                    rec["ret"] = describe(fn())
                except Exception as e:  # noqa: BLE001 — the error is the result
                    rec["err"] = f"{type(e).__name__} status={getattr(e, 'status', None)}: {e}"
                rec["calls"] = lib.log
            lib.log = []
            E = None
            _close_all(before)      # (under the fake: nothing made here may reach the real library's destroy calls)
    finally:
        _lib.load, api._default_ctx = real_load, real_ctx
    return json.loads(json.dumps(out))      # (tuples → lists, as the recorded file has them)


_GOT = None


def got():
    global _GOT
    if _GOT is None:
        _GOT = run_all()
    return _GOT


def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["f64"] = {k: g["f64"].get(k, v) for k, v in g["f32"].items()}      # (the file holds an f64 record only where it differs from the f32 one)
    return g


def _names():
    try:
        g = _golden()
    except OSError:
        return []
    return [(sfx, name) for sfx in sorted(g) for name in g[sfx]]


def test_the_scenario_list_is_the_recorded_one():
    g = _golden()
    assert sorted(g) == ["f32", "f64"] and os.path.getsize(GOLDEN) < 100_000
    for sfx in g:
        assert list(got()[sfx]) == list(g[sfx])
    assert len(g["f32"]) > 250


@pytest.mark.parametrize("sfx,name", _names(), ids=lambda v: v)
def test_calls_returns_and_errors(sfx, name):
    want, have = _golden()[sfx][name], got()[sfx][name]
    assert have.get("err") == want.get("err")
    assert have["calls"] == want["calls"]
    assert have.get("ret") == want.get("ret") and ("ret" in have) == ("ret" in want)


def test_every_public_method_has_a_scenario():
    """a scenario is named <object>.<method>[.<variant> | (<arguments>)]: every public method, property and static method of the six
    classes is the <method> of a recorded scenario on an object of that class"""
    have = {m.groups() for m in (re.match(r"(\w+)\.(\w+)", name) for name in _golden()["f32"]) if m}
    objects = {api.Context: ("ctx",), api.RayBatch: ("rays",), api._Hits: ("hits",), api._TreeBase: ("flat", "bvh"), api.FlatBvh: ("flat",),
               api.Bvh: ("bvh",)}
    for cls, prefixes in objects.items():
        for name, member in vars(cls).items():
            if name.startswith("_") or not (callable(member) or isinstance(member, (property, staticmethod))):
                continue
            assert any((p, name) in have for p in prefixes), f"{cls.__name__}.{name} has no scenario"


def test_every_python_side_refusal_is_recorded():
    """each status / message api.py raises itself (every `raise BvhGpuError` of the file, with what its call sites put into the message)
    appears in the recording, so none can change unnoticed"""
    g = _golden()
    seen = {e for sfx in g for r in g[sfx].values() for e in [r.get("err")] if e}
    I, D = _lib.INVALID_ARG, _lib.DTYPE_MISMATCH
    for want in [(D, "ray dtype differs from tree dtype"), (D, "tmax dtype differs from tree dtype"), (D, "sphere dtype differs from tree dtype"),
                 (D, "point dtype differs from tree dtype"), (D, "max_dist dtype differs from tree dtype"), (D, "query dtype differs from tree dtype"),
                 (I, "tmax is a GPU tensor but the rays are in host memory"), (I, "tmax is in host memory but the rays are in HBM"),
                 (I, "tmax has 3 values for 4 rays"), (I, "tmax has 5 values for 4 rays"), (I, "max_dist has 3 values for 4 points"),
                 (I, "max_dist is a GPU tensor but the points are in host memory"), (I, "max_dist is in host memory but the points are in HBM"),
                 (I, "max_dist has 5 values for 4 points"), (_lib.NO_DEVICE, "no MI355X / HIP device visible: the engine has no CPU fallback"),
                 (I, "leaf must be one of ['box', 'sphere', 'triangle']"), (I, "within_batch needs max_dist (a scalar or one value per point)"),
                 (I, "rebuild_async takes shape AABBs that are resident in HBM (or in pinned host memory: pinned_array)")]:
        assert f"BvhGpuError status={want[0]}: bvhgpu status {want[0]}: {want[1]}" in seen, want


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = run_all()
    assert list(rec["f32"]) == list(rec["f64"])
    rec["f64"] = {k: v for k, v in rec["f64"].items() if v != rec["f32"][k]}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(
            json.dumps(sfx) + ": {\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in rec[sfx].items()) + "\n}"
            for sfx in rec) + "\n}\n")
    print(f"{path}: {sum(len(v) for v in rec.values())} scenarios, {os.path.getsize(path)} bytes")

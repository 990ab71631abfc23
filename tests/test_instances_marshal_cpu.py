"""bvh_amd/instances.py only marshals, like api.py and region.py: what it hands to the C ABI is the whole of its behaviour.  This module is
tests/test_api_marshal_cpu.py's counterpart for the Instances class, on the same fake library, inputs and file format (see that file and the
"call traces" part of tests/test_module_entries_cpu.py): every public method of Instances is run against the recording library — f32 and
f64, host inputs, 4 rays / points / regions, 2 instances of one 7-shape tree, every flag combination a method can produce, k at 1, 3, 0 and
MAX + 1, the Python-side refusals (through the duck-typed GPU tensor where the refusal comes before an output is allocated) — and the call
log, the returned shapes and dtypes and the errors are compared with tests/golden/instances_calls.json.  Needs no GPU and no .so.

The recording is made by this file's __main__ and only ever from the instances.py that precedes a change of the marshalling code:
    python tests/test_instances_marshal_cpu.py [path/to/instances_calls.json]
The changed code must reproduce the file unedited."""
from __future__ import annotations

import ctypes as C
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_api_marshal_cpu as tam  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "instances_calls.json")
N, NI, NM = tam.N, 2, 2                             # rays / points / regions, instances, planes per region
KS = (1, 3, 0, 65)

# host float inputs of the instance entries: stem → [(pointer arg, [count args, multiplied], mem arg, scalars per row)]
_INPUTS = {
    "instances_create": [(4, [5], 6, 12)], "instances_update": [(1, [2], 3, 12)], "instances_trace": [(2, [3], 4, 1)],
    "instances_region": [(1, [2, 3], 4, 4)], "instances_allhits": [(2, [3], 4, 1)], "instances_khits": [(2, [3], 4, 1)],
    "instances_within": [(1, [3], 4, 3), (2, [3], 4, 1)], "instances_knearest": [(1, [2], 3, 3)],
}


class Lib(tam.FakeLib):
    """test_api_marshal_cpu's recording library, with what the instance calls read: the set's handle and figures, the result object's
    handle, a total, and the values of the host inputs (tree_of as integers)"""
    total = 5

    def _values(self, name, args):
        stem, _, sfx = name.rpartition("_")
        if stem not in _INPUTS or sfx not in ("f32", "f64"):
            return tam.FakeLib._values(name, args)
        dt = np.float32 if sfx == "f32" else np.float64
        specs = [(p, int(np.prod([int(args[c]) for c in cs])) * w, mem, dt) for p, cs, mem, w in _INPUTS[stem]]
        if stem == "instances_create":
            specs.insert(0, (3, int(args[5]), 6, np.uint32))
        out = []
        for p, count, mem, t in specs:
            a = args[p]
            if not isinstance(a, C.c_void_p) or not a.value or args[mem] != tam._lib.HOST or not 0 < count <= 256:
                continue
            raw = (C.c_char * (count * np.dtype(t).itemsize)).from_address(a.value)
            out.append(" [" + " ".join(f"{x:g}" for x in np.frombuffer(raw, dtype=t).tolist()) + "]")
        return out

    def _answer(self, name, args):
        rc = tam.FakeLib._answer(self, name, args)
        if name.startswith("instances_create_"):
            args[-1]._obj.value = 0x4000
        elif name == "instances_info":
            args[1]._obj.value, args[2]._obj.value, args[3]._obj.value = self.dtype_code, 1, NI
        elif name.startswith(("instances_region_", "instances_allhits_", "instances_within_")) and isinstance(args[-1], tam._BYREF):
            args[-1]._obj.value = 0x3000            # the result object's handle
        elif name == "hits_info" and isinstance(args[2], tam._BYREF):
            args[2]._obj.value = self.total
        return rc


def scenarios(E):
    from bvh_amd.instances import Instances
    S = []
    ft, other = E.ft, E.other
    xf = (np.arange(NI * 12) * 0.25 - 1).astype(ft).reshape(NI, 12)
    pl = (np.arange(N * NM * 4) * 0.5 - 2).astype(ft).reshape(N, NM, 4)
    s = E.inst

    def add(name, fn):
        S.append((f"inst.{name}", fn))

    def empty(fn):
        def run():
            E.lib.total = 0
            try:
                return fn()
            finally:
                E.lib.total = 5
        return run

    def made(*a, **kw):
        i = Instances(*a, **kw)
        return i, i.sfx, i.n, i.ctx is E.ctx
    # ---- the constructor, update, the set's own figures ------------------------------------------------------------------------------
    add("new", lambda: made([E.flat], [0, 0], xf))
    add("new.bvh.3x4.array_tree_of.ctx", lambda: made([E.bvh], np.array([0, 0], dtype=np.int64), xf.reshape(NI, 3, 4), E.ctx))
    add("new.two_trees.list", lambda: made([E.flat, E.up], [1, 0], xf.tolist()))
    add("new.no_trees", lambda: made([], [], np.zeros((0, 12), dtype=ft)))
    add("new.other_dtype", lambda: made([E.flat], [0, 0], xf.astype(other)))
    add("new.tree_of_length", lambda: made([E.flat], [0, 0, 0], xf))
    add("new.tree_of_device", lambda: made([E.flat], E.dev(NI), xf))
    add("new.ragged", lambda: tam._raises(ValueError, lambda: made([E.flat], [0], xf.reshape(-1)[:13])))
    add("new.device_other_dtype", lambda: made([E.flat], [0, 0], E.dev(NI * 12, wrong=True)))
    add("update", lambda: s.update(xf) is s)
    add("update.3x4.list", lambda: s.update(xf.reshape(NI, 3, 4).tolist()) is s)
    add("update.other_dtype", lambda: s.update(xf.astype(other)))
    add("update.device_other_dtype", lambda: s.update(E.dev(NI * 12, wrong=True)))
    add("world_boxes", lambda: s.world_boxes)
    add("info", s.info)
    # ---- the padded-row ray calls ----------------------------------------------------------------------------------------------------
    tmaxes = {"none": (E.rays, None), "array": (E.rays, E.tmax), "list": (E.rays, E.tmax.tolist()), "scalar": (E.rays, 2.0),
              "other_dtype": (E.rays, E.tmax.astype(other)), "length": (E.rays, E.tmax[:3]), "device_on_host_rays": (E.rays, E.dev(N)),
              "host_on_device_rays": (E.drays, E.tmax), "device_other_dtype": (E.drays, E.dev(N, wrong=True)),
              "device_length": (E.drays, E.dev(N + 1)), "ray_dtype": (E.orays, None)}
    for m in ("closest_hits", "any_hits", "occluded"):
        for tag, (rays, tm) in tmaxes.items():
            if m == "closest_hits" or tag in ("none", "array", "ray_dtype"):        # (one _side_in: its cases run once per call shape)
                add(f"{m}.tmax={tag}", lambda m=m, rays=rays, tm=tm: getattr(s, m)(rays, tm))
        add(f"{m}.default", lambda m=m: getattr(s, m)(E.rays))
    for k in KS:
        add(f"khits_batch.k={k}", lambda k=k: s.khits_batch(E.rays, k))
        add(f"khits_batch.k={k}.tmax", lambda k=k: s.khits_batch(E.rays, k, E.tmax))
        add(f"knearest_batch.k={k}", lambda k=k: s.knearest_batch(E.pts, k))
    for tag in ("list", "other_dtype", "length", "device_on_host_rays", "host_on_device_rays", "ray_dtype"):
        add(f"khits_batch.tmax={tag}", lambda a=tmaxes[tag]: s.khits_batch(a[0], 2, a[1]))
        add(f"allhits_batch.tmax={tag}", lambda a=tmaxes[tag]: s.allhits_batch(a[0], a[1]))
    add("khits_batch.k=float", lambda: s.khits_batch(E.rays, 2.0))
    add("knearest_batch.list", lambda: s.knearest_batch(E.pts.tolist(), 2))
    add("knearest_batch.noncontiguous", lambda: s.knearest_batch(np.asfortranarray(E.pts), 2))
    add("knearest_batch.other_dtype", lambda: s.knearest_batch(E.pts.astype(other), 2))
    add("knearest_batch.device_other_dtype", lambda: s.knearest_batch(E.dev(N * 3, wrong=True), 2))
    add("knearest_batch.ragged", lambda: tam._raises(ValueError, lambda: s.knearest_batch(np.arange(7).astype(ft), 2)))
    add("nearest_batch", lambda: s.nearest_batch(E.pts))
    add("nearest_batch.list", lambda: s.nearest_batch(E.pts.tolist()))
    add("nearest_batch.other_dtype", lambda: s.nearest_batch(E.pts.astype(other)))
    # ---- the CSR calls ---------------------------------------------------------------------------------------------------------------
    for cl in (False, True):
        for co in (False, True):
            for io in (False, True):
                kw = dict(classify=cl, count_only=co, instances_only=io)
                tag = ",".join(f"{k}={v}" for k, v in kw.items())
                add(f"region_batch({tag})", lambda kw=kw: s.region_batch(pl, **kw))
                if not co:
                    add(f"region_batch({tag}).empty_result", empty(lambda kw=kw: s.region_batch(pl, **kw)))
    add("region_batch.default", lambda: s.region_batch(pl))
    add("region_batch.positional", lambda: s.region_batch(pl, True, False, True))
    add("region_batch.one_region", lambda: s.region_batch(pl[0], classify=True))
    add("region_batch.list", lambda: s.region_batch(pl.tolist()))
    add("region_batch.noncontiguous", lambda: s.region_batch(np.asfortranarray(pl)))
    add("region_batch.m=0", lambda: s.region_batch(np.zeros((N, 0, 4), dtype=ft), classify=True))
    add("region_batch.no_regions", empty(lambda: s.region_batch(np.zeros((0, NM, 4), dtype=ft), classify=True)))
    add("region_batch.m=33", lambda: s.region_batch(np.zeros((1, 33, 4), dtype=ft)))                   # (the library refuses it, not Python)
    add("region_batch.other_dtype", lambda: s.region_batch(pl.astype(other)))
    add("region_batch.shape_n_m_3", lambda: s.region_batch(np.zeros((N, NM, 3), dtype=ft)))
    add("region_batch.shape_1d", lambda: s.region_batch(np.zeros(8, dtype=ft)))
    add("region_batch.device_other_dtype", lambda: s.region_batch(_shaped(E.oname, (N, NM, 4))))
    add("region_batch.device_shape", lambda: s.region_batch(_shaped(E.tname, (N, NM * 4))))
    for so in (True, False):
        for co in (False, True):
            tag = f"sort={so},count_only={co}"
            add(f"allhits_batch({tag})", lambda so=so, co=co: s.allhits_batch(E.rays, None, so, co))
            add(f"allhits_batch({tag}).tmax", lambda so=so, co=co: s.allhits_batch(E.rays, E.tmax, sort=so, count_only=co))
            add(f"within_batch({tag})", lambda so=so, co=co: s.within_batch(E.pts, E.md, so, co))
            add(f"within_batch({tag}).scalar", lambda so=so, co=co: s.within_batch(E.pts, 1.5, sort=so, count_only=co))
    add("allhits_batch.default", lambda: s.allhits_batch(E.rays))
    add("allhits_batch.empty_result", empty(lambda: s.allhits_batch(E.rays, E.tmax)))
    add("within_batch.default", lambda: s.within_batch(E.pts, E.md))
    add("within_batch.empty_result", empty(lambda: s.within_batch(E.pts, E.md)))
    limits = {"none": None, "int_scalar": 2, "np_scalar": ft(0.75), "list": E.md.tolist(), "other_dtype": E.md.astype(other),
              "length": E.md[:3], "2d": E.md.reshape(2, 2), "device": E.dev(N)}
    for tag, md in limits.items():
        add(f"within_batch.max_dist={tag}", lambda md=md: s.within_batch(E.pts, md))
    add("within_batch.list", lambda: s.within_batch(E.pts.tolist(), 1.0))
    add("within_batch.other_dtype", lambda: s.within_batch(E.pts.astype(other), 1.0))
    add("within_batch.ragged", lambda: tam._raises(ValueError, lambda: s.within_batch(np.arange(7).astype(ft), 1.0)))
    # points in HBM: every refusal comes before an output is allocated, so the stand-in tensor reaches it
    dpts = {"host_max_dist": (E.dev(N * 3), E.md), "point_dtype": (E.dev(N * 3, wrong=True), E.dev(N)),
            "max_dist_dtype": (E.dev(N * 3), E.dev(N, wrong=True)), "max_dist_length": (E.dev(N * 3), E.dev(N + 1)),
            "host_list_max_dist": (E.dev(N * 3), E.md.tolist()), "no_max_dist": (E.dev(N * 3), None)}
    for tag, (dp, md) in dpts.items():
        add(f"within_batch.device_points.{tag}", lambda dp=dp, md=md: s.within_batch(dp, md))
    # ---- close: the result object made by the CSR calls goes first, a second close is nothing ------------------------------------------

    def closing(batch):
        i = Instances([E.flat], [0, 0], xf)
        if batch:
            i.allhits_batch(E.rays)
        with i as j:
            assert j is i
        i.close()
        return i._s, getattr(i, "_hits", None)
    add("close", lambda: closing(False))
    add("close.after_a_csr_batch", lambda: closing(True))
    return S


def _shaped(name, shape):
    """a stand-in GPU tensor with the shape region_batch reads n and m from"""
    t = tam.FakeTensor(name, int(np.prod(shape)))
    t.shape = tuple(shape)
    return t


def run_all():
    """{sfx: {scenario: {"calls": [...], "ret": ..., "err": ...}}}: test_api_marshal_cpu.run_all's loop over this module's scenarios"""
    from bvh_amd.instances import Instances
    _lib, api = tam._lib, tam.api
    real_load, real_ctx, real_name = _lib.load, api._default_ctx, tam.TREE_DTYPE
    before = {id(o) for o in api._live}
    out = {}
    try:
        for sfx in ("f32", "f64"):
            lib = Lib()
            tam.TREE_DTYPE = "float32" if sfx == "f32" else "float64"
            _lib.load = lambda lib=lib: lib
            E = tam.Env(lib, sfx)
            lib.log = []
            E.inst = Instances([E.flat], [0, 0], (np.arange(NI * 12) * 0.5).astype(E.ft).reshape(NI, 12))
            out[sfx] = {"setup": {"calls": lib.log}}
            for name, fn in scenarios(E):
                assert name not in out[sfx], name
                lib.log = []
                rec = out[sfx][name] = {}
                try:
                    rec["ret"] = tam.describe(fn())
                except Exception as e:  # noqa: BLE001 — the error is the result
                    rec["err"] = f"{type(e).__name__} status={getattr(e, 'status', None)}: {e}"
                rec["calls"] = lib.log
            lib.log = []
            E = None
            tam._close_all(before)
    finally:
        _lib.load, api._default_ctx, tam.TREE_DTYPE = real_load, real_ctx, real_name
    return json.loads(json.dumps(out))


@functools.lru_cache(maxsize=None)
def got():
    return run_all()


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
    assert sorted(g) == ["f32", "f64"] and os.path.getsize(GOLDEN) < 60_000
    for sfx in g:
        assert list(got()[sfx]) == list(g[sfx])
    assert len(g["f32"]) >= 130


@pytest.mark.parametrize("sfx,name", _names(), ids=lambda v: v)
def test_calls_returns_and_errors(sfx, name):
    want, have = _golden()[sfx][name], got()[sfx][name]
    assert have.get("err") == want.get("err")
    assert have["calls"] == want["calls"]
    assert have.get("ret") == want.get("ret") and ("ret" in have) == ("ret" in want)


def test_the_recording_says_what_the_methods_hand_over():
    """read off the file, so that a recording made from a wrong instances.py cannot pass for a right one"""
    g = _golden()["f32"]
    L = tam._lib
    H = L.HOST

    def vals(a):
        return " [" + " ".join(f"{x:g}" for x in np.asarray(a, dtype=np.float64).reshape(-1).tolist()) + "]"

    def calls(name, stem):
        return [c for c in g[f"inst.{name}"]["calls"] if c.startswith(stem + "(")]
    xf = np.arange(NI * 12) * 0.25 - 1
    tmax, md, pts = 1 + np.arange(N) * 0.5, 2 + np.arange(N) * 0.25, np.arange(N * 3) * 0.25 - 1
    pl = np.arange(N * NM * 4) * 0.5 - 2
    assert calls("new", "instances_create_T") == [f"instances_create_T(P,BUF,1,P,P,{NI},{H},OUT) [0 0]" + vals(xf)]
    assert calls("new.two_trees.list", "instances_create_T") == [f"instances_create_T(P,BUF,2,P,P,{NI},{H},OUT) [1 0]" + vals(xf)]
    assert g["inst.new.bvh.3x4.array_tree_of.ctx"]["calls"][0].startswith("flatten")           # a Bvh member is flattened first
    assert g["inst.new"]["ret"] == ["Instances", "f32", NI, True]
    assert calls("update", "instances_update_T") == calls("update.3x4.list", "instances_update_T") == [f"instances_update_T(P,P,{NI},{H})" + vals(xf)]
    for m, flags in (("closest_hits", 0), ("any_hits", L.TRAVERSE_FIRST), ("occluded", L.TRAVERSE_FIRST)):
        assert g[f"inst.{m}.tmax=none"]["calls"] == g[f"inst.{m}.default"]["calls"] == [f"instances_trace_T(P,P,NULL,{N},{H},{flags},P,P,P)"]
        assert g[f"inst.{m}.tmax=array"]["calls"] == [f"instances_trace_T(P,P,P,{N},{H},{flags},P,P,P)" + vals(tmax)]
    assert g["inst.closest_hits.tmax=array"]["ret"] == [f"T[{N}, 3]", f"uint32[{N}]", f"uint32[{N}]"] and g["inst.occluded.default"]["ret"] == f"bool[{N}]"
    for k in KS:
        rows = k if 1 <= k <= 64 else 0
        assert g[f"inst.khits_batch.k={k}"]["calls"] == [f"instances_khits_T(P,P,NULL,{N},{H},{k},P,P,P)"]
        assert g[f"inst.khits_batch.k={k}.tmax"]["calls"] == [f"instances_khits_T(P,P,P,{N},{H},{k},P,P,P)" + vals(tmax)]
        assert g[f"inst.khits_batch.k={k}"]["ret"] == [f"uint32[{N}, {rows}]", f"uint32[{N}, {rows}]", f"T[{N}, {rows}, 3]"]
        assert g[f"inst.knearest_batch.k={k}"]["calls"] == [f"instances_knearest_T(P,P,{N},{H},{k},P,P,P)" + vals(pts)]
        assert g[f"inst.knearest_batch.k={k}"]["ret"] == [f"uint32[{N}, {rows}]", f"uint32[{N}, {rows}]", f"T[{N}, {rows}]"]
    assert g["inst.nearest_batch"]["calls"] == g["inst.knearest_batch.k=1"]["calls"]
    assert g["inst.nearest_batch"]["ret"] == [f"uint32[{N}]", f"uint32[{N}]", f"T[{N}]"]
    CO, CL, IO = L.REGION_COUNT_ONLY, L.REGION_CLASSIFY, L.REGION_INSTANCES_ONLY
    for cl in (False, True):
        for co in (False, True):
            for io in (False, True):
                name = f"region_batch(classify={cl},count_only={co},instances_only={io})"
                flags = (CO if co else 0) | (CL if cl and not co else 0) | (IO if io else 0)
                rows, P = (0, "NULL") if co else (5, "P")
                shape, inside = P if not io else "NULL", P if cl and not co else "NULL"
                assert g[f"inst.{name}"]["calls"] == [f"instances_region_T(P,P,{N},{NM},{H},{flags},OUT)" + vals(pl)] + \
                    ([] if co else ["hits_info(P,NULL,OUT,NULL)"]) + [f"hits_fetch_instances_region(P,P,{P},{shape},{inside},{H})"]
                ret = f"offsets=uint32[{N + 1}] instance=uint32[{rows}]" + ("" if io else f" shape=uint32[{rows}]") + \
                    (f" inside=uint8[{rows}]" if cl and not co else "")
                assert g[f"inst.{name}"]["ret"] == ret
                if not co:
                    assert calls(f"{name}.empty_result", "hits_fetch_instances_region") == [f"hits_fetch_instances_region(P,P,NULL,NULL,NULL,{H})"]
    assert g["inst.region_batch.default"] == g["inst.region_batch(classify=False,count_only=False,instances_only=False)"]
    assert g["inst.region_batch.list"] == g["inst.region_batch.noncontiguous"] == g["inst.region_batch.default"]
    assert calls("region_batch.one_region", "instances_region_T")[0].startswith(f"instances_region_T(P,P,1,{NM},{H},{CL},OUT)")
    for so in (True, False):
        for co in (False, True):
            tag = f"(sort={so},count_only={co})"
            af = (0 if so else L.INSTANCES_ALLHITS_LIST_ORDER) | (L.INSTANCES_ALLHITS_COUNT_ONLY if co else 0)
            wf = (0 if so else L.INSTANCES_WITHIN_LIST_ORDER) | (L.INSTANCES_WITHIN_COUNT_ONLY if co else 0)
            P = "NULL" if co else "P"
            tail = ([] if co else ["hits_info(P,NULL,OUT,NULL)"])
            assert g[f"inst.allhits_batch{tag}"]["calls"] == [f"instances_allhits_T(P,P,NULL,{N},{H},{af},OUT)"] + tail + \
                [f"hits_fetch_instances_allhits(P,P,{P},{P},{P},{H})"]
            assert g[f"inst.allhits_batch{tag}.tmax"]["calls"][0] == f"instances_allhits_T(P,P,P,{N},{H},{af},OUT)" + vals(tmax)
            assert g[f"inst.within_batch{tag}"]["calls"] == [f"instances_within_T(P,P,P,{N},{H},{wf},OUT)" + vals(pts) + vals(md)] + tail + \
                [f"hits_fetch_instances_within(P,P,{P},{P},{P},{H})"]
            assert g[f"inst.within_batch{tag}.scalar"]["calls"][0].endswith(vals(pts) + vals([1.5] * N))
            csr = f"offsets=uint32[{N + 1}]"
            assert g[f"inst.allhits_batch{tag}"]["ret"] == csr + ("" if co else " instance=uint32[5] shape=uint32[5] vals=T[5, 3]")
            assert g[f"inst.within_batch{tag}"]["ret"] == csr + ("" if co else " instance=uint32[5] shape=uint32[5] dist=T[5]")
    for m in ("allhits", "within"):
        assert calls(f"{m}_batch.empty_result", f"hits_fetch_instances_{m}") == [f"hits_fetch_instances_{m}(P,P,NULL,NULL,NULL,{H})"]
    assert g["inst.close"]["calls"][-1] == "instances_destroy(P)" and g["inst.close"]["calls"].count("instances_destroy(P)") == 1
    assert g["inst.close.after_a_csr_batch"]["calls"][-2:] == ["hits_destroy(P)", "instances_destroy(P)"]
    assert g["inst.close"]["ret"] == g["inst.close.after_a_csr_batch"]["ret"] == [None, None]


def test_every_public_method_has_a_scenario():
    from bvh_amd.instances import Instances
    have = {m.group(1) for m in (re.match(r"inst\.(\w+)", name) for name in _golden()["f32"]) if m}
    public = {k for k, v in vars(Instances).items() if not k.startswith("_") and (callable(v) or isinstance(v, (property, staticmethod)))}
    assert public == {"update", "closest_hits", "any_hits", "occluded", "region_batch", "allhits_batch", "khits_batch", "within_batch",
                      "knearest_batch", "nearest_batch", "world_boxes", "info", "close"}
    assert public | {"new"} <= have, sorted(public - have)


def test_every_python_side_refusal_is_recorded():
    """each status / message bvh_amd/instances.py raises itself — read off its source, so that a new one fails here until it has a
    scenario — and the ones api._rows_in, api._side_in and region._plane_dims raise for it are in the recording"""
    g = _golden()
    seen = {e for sfx in g for r in g[sfx].values() for e in [r.get("err")] if e}
    L = tam._lib
    I, D = L.INVALID_ARG, L.DTYPE_MISMATCH
    for w in [(D, "ray dtype differs from the instance set's dtype"), (I, "tree_of is a GPU tensor but the transforms are in host memory"),
              (I, "tree_of has 3 values for 2 transforms"), (I, "within_batch needs max_dist (a scalar or one value per point)"),
              (D, "transform dtype differs from tree dtype"), (D, "tmax dtype differs from tree dtype"), (D, "point dtype differs from tree dtype"),
              (D, "max_dist dtype differs from tree dtype"), (D, "plane dtype differs from tree dtype"),
              (I, "tmax is a GPU tensor but the rays are in host memory"), (I, "tmax is in host memory but the rays are in HBM"),
              (I, "tmax has 3 values for 4 rays"), (I, "tmax has 1 values for 4 rays"), (I, "tmax has 5 values for 4 rays"),
              (I, "max_dist is a GPU tensor but the points are in host memory"), (I, "max_dist is in host memory but the points are in HBM"),
              (I, "max_dist has 3 values for 4 points"), (I, "max_dist has 5 values for 4 points"),
              (I, "planes must be (n, m, 4) or (m, 4), not (4, 2, 3)"), (I, "planes must be (n, m, 4) or (m, 4), not (8,)"),
              (I, "planes must be (n, m, 4) or (m, 4), not (1, 4, 8)")]:
        assert f"BvhGpuError status={w[0]}: bvhgpu status {w[0]}: {w[1]}" in seen, w
    src = open(os.path.join(ROOT, "bvh_amd", "instances.py")).read()
    raised = re.findall(r'raise BvhGpuError\(_lib\.(\w+),\s*f?"([^"]*)"', src)
    assert len(raised) == len(re.findall(r"raise BvhGpuError\(", src)) >= 4
    for status, msg in raised:
        pat = re.compile(re.escape(f"status={getattr(L, status)}: bvhgpu status {getattr(L, status)}: ") +
                         re.sub(r"\\\{[^}]*\\\}", r"\\d+", re.escape(msg)) + "$")
        assert any(pat.search(e) for e in seen), (status, msg)


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

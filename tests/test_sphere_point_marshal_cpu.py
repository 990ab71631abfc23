"""What the four sphere point methods (bvh_amd/api.py, class _SpherePointQueries: knearest_sphere_batch, nearest_sphere_batch,
knearest_tree_sphere_batch, within_sphere_batch) hand to the C ABI: tests/test_api_marshal_cpu.py's recording library, trees and inputs,
with the calls, returns and errors of every scenario below compared with tests/golden/sphere_point_calls.json, and the principal calls
written out by hand as well.  Needs no GPU and no .so.

The recording is made by this file's __main__ (python tests/test_sphere_point_marshal_cpu.py) and only ever from the api.py that
precedes a change of the marshalling code."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import test_api_marshal_cpu as tam

GOLDEN = os.path.join(tam.ROOT, "tests", "golden", "sphere_point_calls.json")
N = tam.N
METHODS = {"knearest_sphere_batch", "nearest_sphere_batch", "knearest_tree_sphere_batch", "within_sphere_batch"}
# host inputs of the new entries: stem -> [(pointer arg, count arg, mem arg, scalars per row)]
INPUTS = {"knearest_sphere": [(1, 2, 3, 3)], "knearest_tree_sphere": [(1, 2, 3, 3), (5, 2, 3, 1)], "within_sphere": [(1, 3, 4, 3), (2, 3, 4, 1)]}


class Lib(tam.FakeLib):
    """... which also shows the host values of the new entries' points and limits"""

    def _values(self, name, args):
        stem, _, sfx = name.rpartition("_")
        if stem not in INPUTS:
            return tam.FakeLib._values(name, args)
        dt = np.float32 if sfx == "f32" else np.float64
        out = []
        for p, n, mem, w in INPUTS[stem]:
            a = args[p]
            if not isinstance(a, tam.C.c_void_p) or not a.value or args[mem] != tam._lib.HOST or not 0 < int(args[n]) * w <= 256:
                continue
            raw = (tam.C.c_char * (int(args[n]) * w * np.dtype(dt).itemsize)).from_address(a.value)
            out.append(" [" + " ".join(f"{x:g}" for x in np.frombuffer(raw, dtype=dt).tolist()) + "]")
        return out


def vals(a):
    return " [" + " ".join(f"{x:g}" for x in np.asarray(a, dtype=np.float64).reshape(-1).tolist()) + "]"


def scenarios(E):
    S = []
    for tn, t in (("bvh", E.bvh), ("flat", E.flat), ("up", E.up)):
        for k in (1, 3, 64, 0, 65, 2.0):
            S.append((f"{tn}.knearest_sphere_batch({k})", lambda t=t, k=k: t.knearest_sphere_batch(E.pts, k)))
            S.append((f"{tn}.knearest_tree_sphere_batch({k})", lambda t=t, k=k: t.knearest_tree_sphere_batch(E.pts, k)))
        S.append((f"{tn}.nearest_sphere_batch", lambda t=t: t.nearest_sphere_batch(E.pts)))
        S.append((f"{tn}.nearest_sphere_batch.list", lambda t=t: t.nearest_sphere_batch(E.pts.tolist())))
        S.append((f"{tn}.knearest_sphere_batch.fortran", lambda t=t: t.knearest_sphere_batch(np.asfortranarray(E.pts), 2)))
        for mn, m in (("array", E.md), ("list", E.md.tolist()), ("2x2", E.md.reshape(2, 2)), ("scalar", 1.5), ("int", 2), ("none", None)):
            S.append((f"{tn}.knearest_tree_sphere_batch.limit.{mn}", lambda t=t, m=m: t.knearest_tree_sphere_batch(E.pts, 2, m)))
            if m is not None:
                S.append((f"{tn}.within_sphere_batch.limit.{mn}", lambda t=t, m=m: t.within_sphere_batch(E.pts, m)))
        S.append((f"{tn}.within_sphere_batch.none", lambda t=t: t.within_sphere_batch(E.pts, None)))
        S.append((f"{tn}.within_sphere_batch.list_order", lambda t=t: t.within_sphere_batch(E.pts, E.md, sort=False)))
        S.append((f"{tn}.within_sphere_batch.count_only", lambda t=t: t.within_sphere_batch(E.pts, E.md, count_only=True)))
        S.append((f"{tn}.within_sphere_batch.both", lambda t=t: t.within_sphere_batch(E.pts, E.md, False, True)))
        for en, fn in (("points_dtype", lambda t=t: t.knearest_sphere_batch(E.pts.astype(E.other), 2)),
                       ("tree_points_dtype", lambda t=t: t.knearest_tree_sphere_batch(E.pts.astype(E.other), 2)),
                       ("within_points_dtype", lambda t=t: t.within_sphere_batch(E.pts.astype(E.other), 1.0)),
                       ("limit_dtype", lambda t=t: t.knearest_tree_sphere_batch(E.pts, 2, E.md.astype(E.other))),
                       ("limit_short", lambda t=t: t.within_sphere_batch(E.pts, E.md[:3])),
                       ("limit_device", lambda t=t: t.within_sphere_batch(E.pts, E.dev(N))),
                       ("points_device_limit_host", lambda t=t: t.knearest_tree_sphere_batch(E.dev(N * 3), 2, E.md)),
                       ("device_limit_long", lambda t=t: t.within_sphere_batch(E.dev(N * 3), E.dev(N + 1))),
                       ("device_wrong_dtype", lambda t=t: t.within_sphere_batch(E.dev(N * 3, wrong=True), E.dev(N)))):
            S.append((f"{tn}.refusal.{en}", fn))
    return S


def run_all():
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
            out[sfx] = {}
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


def test_the_methods_are_a_mixin_that_shadows_nothing():
    api = tam.api
    mixin = api._SpherePointQueries
    assert issubclass(api._TreeBase, mixin) and issubclass(api.Bvh, mixin) and issubclass(api.FlatBvh, mixin)
    assert {k for k in vars(mixin) if not k.startswith("_")} == METHODS
    for cls in (api._TreeBase, api.FlatBvh, api.Bvh, api._FlatView, api._Typed):
        assert not (set(vars(cls)) & set(vars(mixin)) - {"__module__", "__doc__", "__dict__", "__weakref__"}), cls
    for name in METHODS:
        assert getattr(api.Bvh, name) is vars(mixin)[name] and getattr(api.FlatBvh, name) is vars(mixin)[name]
    import bvh_amd
    assert not any("sphere_batch" in n for n in dir(bvh_amd))                # no new module-level entry


def test_the_scenario_list_is_the_recorded_one():
    g = _golden()
    assert sorted(g) == ["f32", "f64"] and os.path.getsize(GOLDEN) < 100_000
    for sfx in g:
        assert list(got()[sfx]) == list(g[sfx])
    assert len(g["f32"]) > 100
    assert {name.split(".")[1].split("(")[0] for name in g["f32"]} >= METHODS


@pytest.mark.parametrize("sfx,name", _names(), ids=lambda v: v)
def test_calls_returns_and_errors(sfx, name):
    want, have = _golden()[sfx][name], got()[sfx][name]
    assert have.get("err") == want.get("err")
    assert have["calls"] == want["calls"]
    assert have.get("ret") == want.get("ret") and ("ret" in have) == ("ret" in want)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_principal_calls_by_hand(sfx):
    """independent of the recording: the argument lists of the six entries as include/bvh_mi355x.h declares them"""
    g, H = got()[sfx], tam._lib.HOST
    pts, md = np.arange(N * 3) * 0.25 - 1, 2 + np.arange(N) * 0.25
    flatten = ["flatten(P)"]                                  # a Bvh flattens before the two flat forms, and only then
    for tn, pre in (("bvh", flatten), ("flat", []), ("up", [])):
        for k in (1, 3, 64, 0, 65):
            rows = k if 1 <= k <= 64 else 0                   # (out of range: the engine refuses, the binding allocates nothing)
            r = g[f"{tn}.knearest_sphere_batch({k})"]
            assert r["calls"][-1] == f"knearest_sphere_T(P,P,{N},{H},{k},P,P)" + vals(pts) and r["ret"] == [f"uint32[{N}, {rows}]", f"T[{N}, {rows}]"]
            assert r["calls"][:-1] in ([], pre)
            r = g[f"{tn}.knearest_tree_sphere_batch({k})"]
            assert r["calls"] == [f"knearest_tree_sphere_T(P,P,{N},{H},{k},NULL,P,P)" + vals(pts)]
            assert r["ret"] == [f"uint32[{N}, {rows}]", f"T[{N}, {rows}]"]
        r = g[f"{tn}.nearest_sphere_batch"]
        assert r["calls"][-1] == f"knearest_sphere_T(P,P,{N},{H},1,P,P)" + vals(pts) and r["ret"] == [f"uint32[{N}]", f"T[{N}]"]
        assert g[f"{tn}.knearest_tree_sphere_batch.limit.array"]["calls"] == [f"knearest_tree_sphere_T(P,P,{N},{H},2,P,P,P)" + vals(pts) + vals(md)]
        assert g[f"{tn}.knearest_tree_sphere_batch.limit.scalar"]["calls"] == [f"knearest_tree_sphere_T(P,P,{N},{H},2,P,P,P)" + vals(pts) + vals([1.5] * N)]
        for variant, flags in (("limit.array", 0), ("list_order", tam._lib.WITHIN_LIST_ORDER), ("count_only", tam._lib.WITHIN_COUNT_ONLY),
                               ("both", tam._lib.WITHIN_LIST_ORDER | tam._lib.WITHIN_COUNT_ONLY)):
            r = g[f"{tn}.within_sphere_batch.{variant}"]
            call = [c for c in r["calls"] if c.startswith("within_sphere_T")]
            assert call == [f"within_sphere_T(P,P,P,{N},{H},{flags},OUT)" + vals(pts) + vals(md)]
            assert any(c.startswith("hits_fetch_within(") for c in r["calls"])
            assert r["ret"][0] == f"uint32[{N + 1}]" and len(r["ret"]) == 3
        r = g[f"{tn}.within_sphere_batch.none"]
        assert r["err"] == f"BvhGpuError status={tam._lib.INVALID_ARG}: bvhgpu status {tam._lib.INVALID_ARG}: within_sphere_batch needs max_dist (a scalar or one value per point)"
        assert not any(c.startswith("within_sphere") for c in r["calls"])
        for en in ("points_dtype", "tree_points_dtype", "within_points_dtype", "limit_dtype", "limit_short", "limit_device", "points_device_limit_host",
                   "device_limit_long", "device_wrong_dtype"):
            r = g[f"{tn}.refusal.{en}"]
            assert r["err"].startswith("BvhGpuError status=") and not any("sphere" in c for c in r["calls"]), (tn, en, r)


if __name__ == "__main__":
    rec = run_all()
    rec["f64"] = {k: v for k, v in rec["f64"].items() if v != rec["f32"][k]}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=False)
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN))

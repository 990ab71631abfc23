"""What `Instances(..., leaf=)` hands to the C ABI and what the ray methods of such a set return: tests/test_instances_marshal_cpu.py's
recording library and inputs (through tests/test_instances_masks_marshal_cpu.py's Lib, which also shows masks), compared with this
module's own recording tests/golden/instances_leaf_calls.json — the constructor per kind, the ValueError of an unknown kind, and the shapes
of closest_hits, any_hits, occluded, khits_batch, allhits_batch and their masked forms, whose value columns are _lib.LEAF_WIDTH wide.  The
default constructor and every existing method stay held by tests/golden/instances_calls.json.  Needs no GPU and no .so.

The recording is made by this file's __main__:
    python tests/test_instances_leaf_marshal_cpu.py [path/to/instances_leaf_calls.json]"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_api_marshal_cpu as tam  # noqa: E402
import test_instances_marshal_cpu as tim  # noqa: E402
import test_instances_masks_marshal_cpu as tmm  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "instances_leaf_calls.json")
N, NI = tim.N, tim.NI
KINDS = ("box", "triangle", "sphere")


def scenarios(E):
    from bvh_amd.instances import Instances
    xf = (np.arange(NI * 12) * 0.5).astype(E.ft).reshape(NI, 12)
    S = []

    def made(*a, **kw):
        i = Instances(*a, **kw)
        return i, i.n, i.leaf

    for leaf in KINDS:
        S.append((f"new.leaf={leaf}", lambda leaf=leaf: made([E.flat], [0, 0], xf, leaf=leaf)))
        S.append((f"new.leaf={leaf}.positional", lambda leaf=leaf: made([E.flat, E.up], [1, 0], xf.tolist(), E.ctx, leaf)))
    S.append(("new.default", lambda: made([E.flat], [0, 0], xf)))
    for bad in ("cube", "Triangle", "", 1, None):
        S.append((f"new.leaf={bad!r}", lambda bad=bad: made([E.flat], [0, 0], xf, leaf=bad)))
    for leaf in KINDS:
        s = E.sets[leaf]
        for m in ("closest_hits", "any_hits", "occluded"):
            S.append((f"{leaf}.{m}", lambda s=s, m=m: getattr(s, m)(E.rays, E.tmax)))
            S.append((f"{leaf}.{m}_masked", lambda s=s, m=m: getattr(s, m + "_masked")(E.rays, E.mask, E.tmax)))
        for k in (1, 3, 0, 65):
            S.append((f"{leaf}.khits_batch.k={k}", lambda s=s, k=k: s.khits_batch(E.rays, k)))
            S.append((f"{leaf}.khits_masked_batch.k={k}", lambda s=s, k=k: s.khits_masked_batch(E.rays, k, E.mask)))
        for so in (True, False):
            for co in (False, True):
                S.append((f"{leaf}.allhits_batch(sort={so},count_only={co})", lambda s=s, so=so, co=co: s.allhits_batch(E.rays, None, so, co)))
                S.append((f"{leaf}.allhits_masked_batch(sort={so},count_only={co})",
                          lambda s=s, so=so, co=co: s.allhits_masked_batch(E.rays, E.mask, None, so, co)))
        S.append((f"{leaf}.closest_hits.device", lambda s=s: s.closest_hits(E.drays)))
        S.append((f"{leaf}.region_batch", lambda s=s: s.region_batch((np.arange(N * 2 * 4) * 0.5 - 2).astype(E.ft).reshape(N, 2, 4))))
    return S


def run_sfx(sfx):
    from bvh_amd.instances import Instances
    _lib, api = tam._lib, tam.api
    real_load, real_ctx, real_name, real_out, real_sync = _lib.load, api._default_ctx, tam.TREE_DTYPE, api._out_cols, api._torch_sync
    before = {id(o) for o in api._live}
    lib = tmm.Lib()
    tam.TREE_DTYPE = "float32" if sfx == "f32" else "float64"
    _lib.load = lambda: lib
    api._torch_sync = lambda device: None                                              # (no torch stream to wait for)
    api._out_cols = lambda device, ft, *cols: real_out(None, ft, *cols)                # (outputs of HBM rays are made on the host)
    rec = {}
    try:
        E = tam.Env(lib, sfx)
        xf = (np.arange(NI * 12) * 0.5).astype(E.ft).reshape(NI, 12)
        E.sets = {leaf: Instances([E.flat], [0, 0], xf, leaf=leaf) for leaf in KINDS}
        E.mask = np.array([1, 0x80000000, 0, 0xFFFFFFFF], dtype=np.uint32)
        for name, fn in scenarios(E):
            lib.log = []
            try:
                ret = fn()
                r = {"ret": tam.describe(ret)}
                if isinstance(ret, tuple) and ret and hasattr(ret[0], "close"):
                    ret[0].close()
            except Exception as e:  # noqa: BLE001 — the error is the result
                r = {"err": f"{type(e).__name__} status={getattr(e, 'status', None)}: {e}"}
            r["calls"] = [c.replace(f"_{sfx}(", "_T(") for c in lib.log]
            if "ret" in r:
                r["ret"] = json.loads(json.dumps(r["ret"]).replace("float32" if sfx == "f32" else "float64", "T"))
            rec[name] = r
        E = None
        tam._close_all(before)
    finally:
        _lib.load, api._default_ctx, tam.TREE_DTYPE, api._out_cols, api._torch_sync = real_load, real_ctx, real_name, real_out, real_sync
    return rec


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_recording_is_reproduced(golden, sfx):
    rec = run_sfx(sfx)
    want = golden["both"]
    assert list(rec) == list(want)
    for name in want:
        assert rec[name] == want[name], (name, rec[name], want[name])


def test_what_the_recording_says(golden):
    """the recording itself, against the calls and shapes written out"""
    g, L = golden["both"], tam._lib
    H = L.HOST
    xf = " [0 0] [" + " ".join(f"{x:g}" for x in (np.arange(NI * 12) * 0.5).tolist()) + "]"
    # "triangle" is the existing entry, handed what the default constructor hands it; the other kinds go to create_leaf with the kind's code
    assert g["new.leaf=triangle"]["calls"][0] == g["new.default"]["calls"][0] == f"instances_create_T(P,BUF,1,P,P,{NI},{H},OUT)" + xf
    for leaf in ("box", "sphere"):
        assert g[f"new.leaf={leaf}"]["calls"][0].startswith(f"instances_create_leaf_T(P,BUF,1,P,P,{NI},{H},{L.LEAF_KINDS[leaf]},OUT)")
        assert g[f"new.leaf={leaf}.positional"]["calls"][0].startswith(f"instances_create_leaf_T(P,BUF,2,P,P,{NI},{H},{L.LEAF_KINDS[leaf]},OUT)")
    for leaf in KINDS:
        assert g[f"new.leaf={leaf}"]["ret"] == g[f"new.leaf={leaf}.positional"]["ret"] == ["Instances", NI, leaf]
    assert g["new.default"]["ret"] == ["Instances", NI, "triangle"]
    for bad in ("cube", "Triangle", "", 1, None):
        r = g[f"new.leaf={bad!r}"]
        assert r["calls"] == [] and r["err"].startswith("ValueError status=None: leaf must be one of ['box', 'sphere', 'triangle']"), r
    for leaf in KINDS:
        w = L.LEAF_WIDTH[L.LEAF_KINDS[leaf]]
        assert w == (3 if leaf == "triangle" else 2)
        rows = [f"T[{N}, {w}]", f"uint32[{N}]", f"uint32[{N}]"]
        for m in ("closest_hits", "any_hits"):
            assert g[f"{leaf}.{m}"]["ret"] == g[f"{leaf}.{m}_masked"]["ret"] == rows
        assert g[f"{leaf}.closest_hits.device"]["ret"] == rows
        assert g[f"{leaf}.occluded"]["ret"] == g[f"{leaf}.occluded_masked"]["ret"] == f"bool[{N}]"
        for k in (1, 3, 0, 65):
            r = k if 1 <= k <= 64 else 0
            want = [f"uint32[{N}, {r}]", f"uint32[{N}, {r}]", f"T[{N}, {r}, {w}]"]
            assert g[f"{leaf}.khits_batch.k={k}"]["ret"] == g[f"{leaf}.khits_masked_batch.k={k}"]["ret"] == want
        for so in (True, False):
            tag = f"(sort={so},count_only=False)"
            want = f"offsets=uint32[{N + 1}] instance=uint32[5] shape=uint32[5] vals=T[5, {w}]"
            assert g[f"{leaf}.allhits_batch{tag}"]["ret"] == g[f"{leaf}.allhits_masked_batch{tag}"]["ret"] == want
            assert g[f"{leaf}.allhits_batch(sort={so},count_only=True)"]["ret"] == f"offsets=uint32[{N + 1}]"
        # the calls themselves do not depend on the kind: the set knows it
        for name in (k for k in g if k.startswith("triangle.")):
            assert g[leaf + name[len("triangle"):]]["calls"] == g[name]["calls"], (leaf, name)


def test_the_class_gains_no_public_name():
    from bvh_amd.instances import Instances
    public = {k for k, v in vars(Instances).items() if not k.startswith("_")}
    assert public == {"update", "closest_hits", "any_hits", "occluded", "region_batch", "allhits_batch", "khits_batch", "within_batch",
                      "knearest_batch", "nearest_batch", "world_boxes", "info", "close"}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    a, b = run_sfx("f32"), run_sfx("f64")
    assert a == b, [k for k in a if a[k] != b[k]]
    with open(path, "w") as f:
        f.write('{\n"both": {\n' + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in a.items()) + "\n}\n}\n")
    print(f"{path}: {len(a)} scenarios, {os.path.getsize(path)} bytes")

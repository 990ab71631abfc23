"""The batch entries of the Python API that are module-level functions (bvh_amd.region_batch) under the two completeness checks the
methods of the tree classes are under, which enumerate classes and so cannot see a function:

  tests/test_tree_generations_cpu.py   every batch entry has a row in a reader table, and tests/test_gpu_tree_generations.py makes every row
                                       the first reader of each new tree generation under every flatten mode
  tests/test_api_marshal_cpu.py        every public method has a recorded call trace, and every Python-side refusal is recorded

This module is their counterpart for functions, on the same scenes, inputs, fake library and file format:

  MODULE_READERS  name -> (exported function, the call, the reference) over test_tree_generations_cpu's generations A, B, A', C, D.  The
                  reference of a region row is region_ref.walk over the ORACLE's tree of that generation (for A' the oracle's refit of A's
                  tree: same topology, re-joined boxes), never an array the engine produced.  tests/test_gpu_module_entries.py runs them.
  completeness    every function exported from bvh_amd has a row, or a reason in NO_TREE why it reads no tree — and a function with a
                  reason takes no tree.  A batch entry added as a function fails here until it has a row.
  sensitivity     the expectations tell the generations apart, the stale-array model (the previous generation's flat array over the new
                  boxes) is not the new answer, every expectation is non-trivial and crosses a chunk border of the kernel's schedule
  call traces     every public function of bvh_amd/region.py run against test_api_marshal_cpu's recording library, compared with
                  tests/golden/region_calls.json: flags, n and m, the plane values read back through the pointer, NULL pointers for empty
                  results, the (m, 4) form, the dtype and shape refusals.  Recorded by this file's __main__:
                      python tests/test_module_entries_cpu.py [path/to/region_calls.json]
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
import json
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import region_ref as rr  # noqa: E402
import test_api_marshal_cpu as tam  # noqa: E402
from test_tree_generations_cpu import DTYPES, Reader, gen, same_all  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "region_calls.json")
N_REGIONS, REGION_SEED = 40, 31
CHUNK_MIN = 1024                                    # region.hip REGION_CHUNK_MIN (tests/test_region_cpu.py pins it against the source)


# ---- the reader table -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planes(dtype):
    """ONE batch per dtype, the same for every generation: 40 regions of 1 - 6 planes through the middle of scene A, padded to 6"""
    p = rr.random_regions(gen("A", dtype).aabbs, N_REGIONS, REGION_SEED)
    p.setflags(write=False)
    return p


def _rows(G):
    return G.memo("region", lambda: rr.walk(G.flat, G.aabbs, planes(G.dtype)))


def _numpy(r, keys):
    """a region_batch result as the reference's arrays, whichever memory it is in"""
    out = []
    for k in keys:
        v = r[k]
        if not isinstance(v, np.ndarray):           # a torch tensor in HBM: offsets int64, indices int32, inside uint8
            v = v.cpu().numpy()
            v = v.astype(np.uint32) if k == "offsets" else v.view(np.uint32) if k == "indices" else v
        out.append(v)
    return tuple(out)


def _region(tree, keys, device=False, **kw):
    def call(T, I):
        import bvh_amd
        return _numpy(bvh_amd.region_batch(getattr(T, tree), I.planes_dev if device else I.planes, **kw), keys)
    return call


ALL3, CSR = ("offsets", "indices", "inside"), ("offsets", "indices")
MODULE_READERS = [
    Reader("region_classify", "region_batch", _region("flat", ALL3, classify=True), lambda G, I: _rows(G), kind="rows"),
    Reader("region_plain_bvh", "region_batch", _region("bvh", CSR), lambda G, I: _rows(G)[:2], kind="rows"),
    Reader("region_count_only", "region_batch", _region("flat", CSR, count_only=True), lambda G, I: (_rows(G)[0], _rows(G)[1][:0]), kind="counts"),
    Reader("region_device_planes", "region_batch", _region("flat", ALL3, device=True, classify=True), lambda G, I: _rows(G), kind="rows"),
]
MODULE_READER_IDS = [r.name for r in MODULE_READERS]

# exported functions that read no tree: the only kind this list may hold
NO_TREE = {
    "device_count": "bvhgpu_device_count: no context, no tree",
    "default_context": "makes or returns a Context",
    "pinned_array": "allocates host memory in a Context",
    "spheres_aabbs": "numpy on the host: the boxes of spheres",
    "aabb_planes": "numpy on the host: six planes of a box",
    "frustum_planes": "numpy on the host: six planes of a camera",
}


def want(reader, name, dtype):
    return tuple(np.ascontiguousarray(x) for x in reader.want(gen(name, dtype), None))


def exported_functions():
    import bvh_amd
    return {k: v for k, v in vars(bvh_amd).items() if not k.startswith("_") and isinstance(v, (types.FunctionType, types.BuiltinFunctionType))}


def test_every_exported_function_has_a_row_or_reads_no_tree():
    import bvh_amd
    fns = exported_functions()
    assert set(fns) <= set(bvh_amd.__all__), sorted(set(fns) - set(bvh_amd.__all__))
    rows = {r.method for r in MODULE_READERS}
    assert rows <= set(fns), sorted(rows - set(fns))
    assert not rows & set(NO_TREE) and set(NO_TREE) <= set(fns), sorted(set(NO_TREE) - set(fns))
    missing = set(fns) - rows - set(NO_TREE)
    assert not missing, f"no row in MODULE_READERS and no reason in NO_TREE for {sorted(missing)}"
    for name in NO_TREE:                            # a reason does not excuse a function that is handed a tree
        params = set(inspect.signature(fns[name]).parameters)
        assert not params & {"tree", "bvh", "flat", "hits"}, (name, params)
    for name in rows:
        assert "tree" in inspect.signature(fns[name]).parameters, name
    # every module of the package that defines an exported function handed a tree is read by the call-trace part below
    assert {fns[name].__module__ for name in rows} == {"bvh_amd.region"}
    assert len(set(MODULE_READER_IDS)) == len(MODULE_READER_IDS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reader", MODULE_READERS, ids=MODULE_READER_IDS)
def test_expectations_tell_the_generations_apart(reader, dtype):
    wa = want(reader, "A", dtype)
    for other in ("B", "A1", "C", "D"):
        assert not same_all(wa, want(reader, other, dtype)), other
    assert not same_all(want(reader, "C", dtype), want(reader, "D", dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stale_arrays_over_new_boxes_are_not_the_new_answer(dtype):
    """a region_batch that skipped ensure_flat_arrays walks the previous generation's array over the new shape boxes"""
    a = gen("A", dtype)
    for new in ("B", "A1"):
        g = gen(new, dtype)
        stale = rr.walk(a.flat, g.aabbs, planes(dtype))
        assert not same_all(stale[:2], _rows(g)[:2]), new
        assert stale[0].tobytes() != _rows(g)[0].tobytes(), new      # (the count-only row sees it too)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["B", "A1", "D"])
def test_expectations_are_not_trivial(name, dtype):
    """rows of two and more shapes, both `inside` values, and — on the folded array the engine walks, at the kernel's smallest chunk —
    rows that continue over a chunk border, so that a stale ancestor table or unit count would show"""
    g = gen(name, dtype)
    off, idx, ins = _rows(g)
    n = np.diff(off.astype(np.int64))
    assert off[-1] > 0 and len(idx) == off[-1] == len(ins) and (n >= 2).sum() >= 10
    assert (ins == 0).any() and (ins == 1).any()
    ent = rr.entries(g.flat, g.aabbs, True)
    assert len(ent["exit"]) == 2 * len(g.aabbs) - 2 > CHUNK_MIN
    spanning = 0
    for q in range(0, N_REGIONS, 5):
        units = []
        assert rr.scan(ent, planes(dtype)[q], 64, CHUNK_MIN, units=units) == idx[off[q]:off[q + 1]].tolist(), q
        spanning += sum(u["count"] > 0 for u in units) >= 2
    assert spanning >= 3, spanning


# ---- call traces ------------------------------------------------------------------------------------------------------------------------
NR, NM = 3, 2                                       # regions and planes per region of the recorded batches


class Lib(tam.FakeLib):
    """test_api_marshal_cpu's recording library, with what the region calls read: a total, the chunk figures, the plane values"""
    total = 5

    def _values(self, name, args):
        stem, _, sfx = name.rpartition("_")
        if stem != "region" or sfx not in ("f32", "f64"):
            return tam.FakeLib._values(name, args)
        count = int(args[2]) * int(args[3]) * 4
        a = args[1]
        if not isinstance(a, C.c_void_p) or not a.value or args[4] != tam._lib.HOST or not 0 < count <= 256:
            return []
        dt = np.float32 if sfx == "f32" else np.float64
        raw = (C.c_char * (count * np.dtype(dt).itemsize)).from_address(a.value)
        return [" [" + " ".join(f"{x:g}" for x in np.frombuffer(raw, dtype=dt).tolist()) + "]"]

    def _answer(self, name, args):
        rc = tam.FakeLib._answer(self, name, args)
        if name.startswith("region_f") and isinstance(args[-1], tam._BYREF):
            args[-1]._obj.value = 0x3000            # the result object's handle
        elif name == "hits_region_info":
            args[1]._obj.value, args[2]._obj.value = 3, 1024
        elif name == "hits_info" and isinstance(args[2], tam._BYREF):
            args[2]._obj.value = self.total
        return rc


class ShapedTensor(tam.FakeTensor):
    """a stand-in GPU tensor with the shape region_batch reads n and m from"""

    def __init__(self, name, shape):
        tam.FakeTensor.__init__(self, name, int(np.prod(shape)))
        self.shape = tuple(shape)


def scenarios(E):
    from bvh_amd import region
    S = []
    ft, other = E.ft, E.other
    pl = (np.arange(NR * NM * 4) * 0.5 - 2).astype(ft).reshape(NR, NM, 4)

    def add(name, fn):
        S.append((f"region.{name}", fn))

    def empty(fn):
        def run():
            E.lib.total = 0
            try:
                return fn()
            finally:
                E.lib.total = 5
        return run
    add("region_batch", lambda: region.region_batch(E.flat, pl))
    add("region_batch.bvh", lambda: region.region_batch(E.bvh, pl))
    add("region_batch.uploaded", lambda: region.region_batch(E.up, pl))
    add("region_batch.classify", lambda: region.region_batch(E.flat, pl, classify=True))
    add("region_batch.count_only", lambda: region.region_batch(E.flat, pl, count_only=True))
    add("region_batch.classify.count_only", lambda: region.region_batch(E.flat, pl, True, True))
    add("region_batch.one_region", lambda: region.region_batch(E.flat, pl[0], classify=True))
    add("region_batch.list", lambda: region.region_batch(E.flat, pl.tolist()))
    add("region_batch.noncontiguous", lambda: region.region_batch(E.flat, np.asfortranarray(pl)))
    add("region_batch.m=0", lambda: region.region_batch(E.flat, np.zeros((NR, 0, 4), dtype=ft), classify=True))
    add("region_batch.no_regions", empty(lambda: region.region_batch(E.flat, np.zeros((0, NM, 4), dtype=ft), classify=True)))
    add("region_batch.empty_result", empty(lambda: region.region_batch(E.flat, pl, classify=True)))
    add("region_batch.m=33", lambda: region.region_batch(E.flat, np.zeros((1, 33, 4), dtype=ft)))      # (the library refuses it, not Python)
    add("region_batch.other_dtype", lambda: region.region_batch(E.flat, pl.astype(other)))
    add("region_batch.int_dtype", lambda: region.region_batch(E.flat, np.ones((NR, NM, 4), dtype=np.int32)))
    add("region_batch.shape_n_m_3", lambda: region.region_batch(E.flat, np.zeros((NR, NM, 3), dtype=ft)))
    add("region_batch.shape_1d", lambda: region.region_batch(E.flat, np.zeros(8, dtype=ft)))
    add("region_batch.shape_4d", lambda: region.region_batch(E.flat, np.zeros((1, NR, NM, 4), dtype=ft)))
    add("region_batch.device_other_dtype", lambda: region.region_batch(E.flat, ShapedTensor(E.oname, (NR, NM, 4))))
    add("region_batch.device_shape", lambda: region.region_batch(E.flat, ShapedTensor(E.tname, (NR, NM * 4))))
    add("frustum_planes", lambda: region.frustum_planes([0, 0, 0], [0, 0, 1], dtype=ft))
    add("frustum_planes.all_arguments", lambda: region.frustum_planes([1, 2, 3], [4, 5, 9], [0, 0, 1], 45.0, 2.0, 0.5, 50.0, ft))
    add("frustum_planes.default_dtype", lambda: str(region.frustum_planes([0, 0, 0], [0, 0, 1]).dtype))
    add("aabb_planes", lambda: region.aabb_planes([0, 1, 2], [3, 4, 5], ft))
    add("aabb_planes.values", lambda: region.aabb_planes([0, 1, 2], [3, 4, 5], ft).tolist())
    add("aabb_planes.default_dtype", lambda: str(region.aabb_planes(np.zeros(3), np.ones((1, 3))).dtype))
    return S


def run_all():
    """{sfx: {scenario: {"calls": [...], "ret": ..., "err": ...}}}: test_api_marshal_cpu.run_all's loop over this module's scenarios"""
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
    assert sorted(g) == ["f32", "f64"] and os.path.getsize(GOLDEN) < 20_000
    for sfx in g:
        assert list(got()[sfx]) == list(g[sfx])
    assert len(g["f32"]) >= 25


@pytest.mark.parametrize("sfx,name", _names(), ids=lambda v: v)
def test_calls_returns_and_errors(sfx, name):
    want_, have = _golden()[sfx][name], got()[sfx][name]
    assert have.get("err") == want_.get("err")
    assert have["calls"] == want_["calls"]
    assert have.get("ret") == want_.get("ret") and ("ret" in have) == ("ret" in want_)


def test_the_recording_says_what_the_entry_hands_over():
    """read off the file, so that a recording made from a wrong region.py cannot pass for a right one"""
    g = _golden()["f32"]
    vals = " [" + " ".join(f"{x:g}" for x in (np.arange(NR * NM * 4) * 0.5 - 2).tolist()) + "]"
    HOST, CO, CL = tam._lib.HOST, tam._lib.REGION_COUNT_ONLY, tam._lib.REGION_CLASSIFY

    def region_call(name):
        calls = [c for c in g[f"region.region_batch{name}"]["calls"] if c.startswith("region_T(")]
        assert len(calls) == 1, (name, g[f"region.region_batch{name}"])
        return calls[0]

    def fetch(name):
        return [c for c in g[f"region.region_batch{name}"]["calls"] if c.startswith("hits_fetch_region(")]
    assert region_call("") == f"region_T(P,P,{NR},{NM},{HOST},0,OUT)" + vals
    assert region_call(".classify") == f"region_T(P,P,{NR},{NM},{HOST},{CL},OUT)" + vals
    assert region_call(".count_only") == region_call(".classify.count_only") == f"region_T(P,P,{NR},{NM},{HOST},{CO},OUT)" + vals
    assert region_call(".one_region") == f"region_T(P,P,1,{NM},{HOST},{CL},OUT)" + " [" + " ".join(f"{x:g}" for x in (np.arange(NM * 4) * 0.5 - 2).tolist()) + "]"
    assert region_call(".list") == region_call(".noncontiguous") == region_call(".bvh") == region_call(".uploaded") == region_call("")
    assert region_call(".m=0").startswith(f"region_T(P,P,{NR},0,{HOST},{CL},OUT)")
    assert region_call(".no_regions").startswith(f"region_T(P,P,0,{NM},{HOST},{CL},OUT)")
    assert fetch("") == [f"hits_fetch_region(P,P,P,NULL,{HOST})"] and fetch(".classify") == [f"hits_fetch_region(P,P,P,P,{HOST})"]
    assert fetch(".count_only") == fetch(".classify.count_only") == [f"hits_fetch_region(P,P,NULL,NULL,{HOST})"]
    assert fetch(".empty_result") == fetch(".no_regions") == [f"hits_fetch_region(P,P,NULL,NULL,{HOST})"]
    assert g["region.region_batch.classify"]["ret"] == "offsets=uint32[4] indices=uint32[5] chunks=3 chunk_entries=1024 inside=uint8[5]"
    assert g["region.region_batch.count_only"]["ret"] == "offsets=uint32[4] indices=uint32[0] chunks=3 chunk_entries=1024"
    assert g["region.region_batch.bvh"]["calls"][0].startswith("flatten")     # a Bvh is flattened first, a FlatBvh is not
    assert not g["region.region_batch"]["calls"][0].startswith("flatten")


def test_every_public_function_has_a_scenario():
    from bvh_amd import region
    have = {m.group(1) for m in (re.match(r"region\.(\w+)", name) for name in _golden()["f32"]) if m}
    public = {k for k, v in vars(region).items() if not k.startswith("_") and isinstance(v, types.FunctionType) and v.__module__ == region.__name__}
    assert public == {"region_batch", "frustum_planes", "aabb_planes"} and public <= have, sorted(public - have)


def test_every_python_side_refusal_is_recorded():
    """each status / message bvh_amd/region.py raises itself, and the one api._rows_in raises for it, is in the recording — and the file
    has no `raise BvhGpuError` beyond those"""
    g = _golden()
    seen = {e for sfx in g for r in g[sfx].values() for e in [r.get("err")] if e}
    I, D = tam._lib.INVALID_ARG, tam._lib.DTYPE_MISMATCH
    own = [(I, "planes must be (n, m, 4) or (m, 4), not (3, 2, 3)"), (I, "planes must be (n, m, 4) or (m, 4), not (8,)"),
           (I, "planes must be (n, m, 4) or (m, 4), not (1, 3, 2, 4)"), (I, "planes must be (n, m, 4) or (m, 4), not (1, 3, 8)")]
    for w in own + [(D, "plane dtype differs from tree dtype")]:
        assert f"BvhGpuError status={w[0]}: bvhgpu status {w[0]}: {w[1]}" in seen, w
    src = open(os.path.join(ROOT, "bvh_amd", "region.py")).read()
    assert len(re.findall(r"raise BvhGpuError\(", src)) == 1 and 'f"planes must be (n, m, 4) or (m, 4), not {shp}"' in src


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

"""What Instances.knearest_tree_batch / nearest_tree_batch (bvh_amd/instances.py, class InstancesTreeForm) hand to the C ABI:
tests/test_instances_marshal_cpu.py's recording library and inputs, with the expected calls, returns and refusals written out here
(no recorded file: two methods, one entry point).  Needs no GPU and no .so."""
from __future__ import annotations

import numpy as np
import pytest

import test_api_marshal_cpu as tam
import test_instances_marshal_cpu as tim

N, NI = tim.N, tim.NI
INPUTS = [(1, 2, 3, 3), (5, 2, 3, 1)]          # (pointer arg, count arg, mem arg, scalars per row): the points, then max_dist


class Lib(tim.Lib):
    """... which also shows the host values of the new entry's points and limits"""

    def _values(self, name, args):
        stem, _, sfx = name.rpartition("_")
        if stem != "instances_knearest_tree":
            return tim.Lib._values(self, name, args)
        dt = np.float32 if sfx == "f32" else np.float64
        out = []
        for p, n, mem, w in INPUTS:
            a = args[p]
            if not isinstance(a, tam.C.c_void_p) or not a.value or args[mem] != tam._lib.HOST or not 0 < int(args[n]) * w <= 256:
                continue
            raw = (tam.C.c_char * (int(args[n]) * w * np.dtype(dt).itemsize)).from_address(a.value)
            out.append(" [" + " ".join(f"{x:g}" for x in np.frombuffer(raw, dtype=dt).tolist()) + "]")
        return out


def vals(a):
    return " [" + " ".join(f"{x:g}" for x in np.asarray(a, dtype=np.float64).reshape(-1).tolist()) + "]"


@pytest.fixture(params=["f32", "f64"])
def env(request):
    """(E, run): run(fn) → (described return or None, error text or None, the calls fn made)"""
    from bvh_amd.instances import Instances
    _lib, api = tam._lib, tam.api
    real_load, real_ctx, real_name = _lib.load, api._default_ctx, tam.TREE_DTYPE
    before = {id(o) for o in api._live}
    sfx = request.param
    lib = Lib()
    tam.TREE_DTYPE = "float32" if sfx == "f32" else "float64"
    _lib.load = lambda: lib
    try:
        E = tam.Env(lib, sfx)
        E.inst = Instances([E.flat], [0, 0], (np.arange(NI * 12) * 0.5).astype(E.ft).reshape(NI, 12))

        def run(fn):
            lib.log = []
            try:
                return tam.describe(fn()), None, lib.log
            except Exception as e:  # noqa: BLE001 — the error is the result
                return None, f"{type(e).__name__} status={getattr(e, 'status', None)}: {e}", lib.log
        yield E, run
        E = None
        tam._close_all(before)
    finally:
        _lib.load, api._default_ctx, tam.TREE_DTYPE = real_load, real_ctx, real_name


def test_the_methods_belong_to_the_set():
    from bvh_amd.instances import Instances, InstancesTreeForm
    assert issubclass(Instances, InstancesTreeForm)
    assert {k for k in vars(InstancesTreeForm) if not k.startswith("_")} == {"knearest_tree_batch", "nearest_tree_batch"}


def test_calls_and_returns(env):
    E, run = env
    s, H = E.inst, tam._lib.HOST
    pts, md = np.arange(N * 3) * 0.25 - 1, 2 + np.arange(N) * 0.25
    for k in (1, 3, 0, 65):
        rows = k if 1 <= k <= 64 else 0                       # (out of range: the engine refuses, the binding allocates nothing)
        ret, err, calls = run(lambda: s.knearest_tree_batch(E.pts, k))
        assert err is None and calls == [f"instances_knearest_tree_T(P,P,{N},{H},{k},NULL,P,P,P)" + vals(pts)]
        assert ret == [f"uint32[{N}, {rows}]", f"uint32[{N}, {rows}]", f"T[{N}, {rows}]"]
    want = [f"instances_knearest_tree_T(P,P,{N},{H},2,P,P,P,P)" + vals(pts) + vals(md)]
    for m in (E.md, E.md.tolist(), E.md.reshape(2, 2)):
        assert run(lambda: s.knearest_tree_batch(E.pts, 2, m))[1:] == (None, want)
    assert run(lambda: s.knearest_tree_batch(E.pts.tolist(), 2, max_dist=E.md))[2] == want
    assert run(lambda: s.knearest_tree_batch(np.asfortranarray(E.pts), 2, E.md))[2] == want
    for m, shown in ((1.5, [1.5] * N), (2, [2] * N), (E.ft(0.75), [0.75] * N)):          # a scalar is every point's limit
        assert run(lambda: s.knearest_tree_batch(E.pts, 2, m))[2] == [want[0][:want[0].rindex(" [")] + vals(shown)]
    assert run(lambda: s.knearest_tree_batch(E.pts, 2.0))[2] == [f"instances_knearest_tree_T(P,P,{N},{H},2,NULL,P,P,P)" + vals(pts)]
    ret, err, calls = run(lambda: s.nearest_tree_batch(E.pts))
    assert err is None and calls == [f"instances_knearest_tree_T(P,P,{N},{H},1,NULL,P,P,P)" + vals(pts)]
    assert ret == [f"uint32[{N}]", f"uint32[{N}]", f"T[{N}]"]
    assert run(lambda: s.nearest_tree_batch(E.pts, E.md))[2] == [f"instances_knearest_tree_T(P,P,{N},{H},1,P,P,P,P)" + vals(pts) + vals(md)]


def test_python_side_refusals(env):
    """api._rows_in's and api._side_in's refusals come before anything is handed over"""
    E, run = env
    s = E.inst
    I, D = tam._lib.INVALID_ARG, tam._lib.DTYPE_MISMATCH
    for fn, status, text in (
            (lambda: s.knearest_tree_batch(E.pts.astype(E.other), 2), D, "point dtype differs from tree dtype"),
            (lambda: s.knearest_tree_batch(E.pts, 2, E.md.astype(E.other)), D, "max_dist dtype differs from tree dtype"),
            (lambda: s.knearest_tree_batch(E.pts, 2, E.md[:3]), I, "max_dist has 3 values for 4 points"),
            (lambda: s.knearest_tree_batch(E.pts, 2, E.dev(N)), I, "max_dist is a GPU tensor but the points are in host memory"),
            (lambda: s.knearest_tree_batch(E.dev(N * 3), 2, E.md), I, "max_dist is in host memory but the points are in HBM"),
            (lambda: s.knearest_tree_batch(E.dev(N * 3), 2, E.md.tolist()), I, "max_dist is in host memory but the points are in HBM"),
            (lambda: s.knearest_tree_batch(E.dev(N * 3, wrong=True), 2, E.dev(N)), D, "point dtype differs from tree dtype"),
            (lambda: s.knearest_tree_batch(E.dev(N * 3), 2, E.dev(N, wrong=True)), D, "max_dist dtype differs from tree dtype"),
            (lambda: s.knearest_tree_batch(E.dev(N * 3), 2, E.dev(N + 1)), I, "max_dist has 5 values for 4 points"),
            (lambda: s.nearest_tree_batch(E.pts.astype(E.other)), D, "point dtype differs from tree dtype")):
        ret, err, calls = run(fn)
        assert err == f"BvhGpuError status={status}: bvhgpu status {status}: {text}" and calls == [], (err, calls)
    with pytest.raises(ValueError):
        s.knearest_tree_batch(np.arange(7).astype(E.ft), 2)

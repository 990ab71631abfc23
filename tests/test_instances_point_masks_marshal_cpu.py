"""What the masked point and region methods of an instance set (bvh_amd/instances.py, class InstancesMaskedQueries: within_masked_batch,
knearest_masked_batch, nearest_masked_batch, knearest_tree_masked_batch, nearest_tree_masked_batch, region_masked_batch) hand to the C ABI:
tests/test_instances_masks_marshal_cpu.py's recording library and inputs, with the expected calls, returns and refusals written out here
(no recorded file).  Inputs in HBM are the duck-typed GPU tensor of tests/test_api_marshal_cpu.py; where a call on them gets as far as
allocating outputs, the outputs are made on the host instead (the pointers handed over for the inputs are what is looked at).  Needs no
GPU and no .so."""
from __future__ import annotations

import numpy as np
import pytest

import test_api_marshal_cpu as tam
import test_instances_marshal_cpu as tim
import test_instances_masks_marshal_cpu as tmm

N, NI, NM = tim.N, tim.NI, tim.NM
C = tam.C
# entry stem → [(pointer arg, count arg, mem arg, kind)]: the side arrays whose host values the log shows (limits as floats, masks in hex)
SIDE = {"instances_within_masked": [(2, 4, 5, "f"), (3, 4, 5, "m")], "instances_knearest_masked": [(2, 3, 4, "m")],
        "instances_knearest_tree_masked": [(6, 3, 4, "f"), (2, 3, 4, "m")], "instances_region_masked": [(2, 3, 5, "m")]}
fl, hx = tmm.fl, tmm.hx
NAMES = {"within_masked_batch", "knearest_masked_batch", "nearest_masked_batch", "knearest_tree_masked_batch", "nearest_tree_masked_batch",
         "region_masked_batch"}


class Lib(tmm.Lib):
    def _values(self, name, args):
        stem, _, sfx = name.rpartition("_")
        if stem not in SIDE:
            return tmm.Lib._values(self, name, args)
        out = []
        for p, n, mem, kind in SIDE[stem]:
            dt = np.uint32 if kind == "m" else np.float32 if sfx == "f32" else np.float64
            a = args[p]
            if not isinstance(a, C.c_void_p) or not a.value or args[mem] != tam._lib.HOST or not 0 < int(args[n]) <= 256:
                continue
            raw = (C.c_char * (int(args[n]) * np.dtype(dt).itemsize)).from_address(a.value)
            v = np.frombuffer(raw, dtype=dt).tolist()
            out.append(" [" + " ".join(f"{x:#x}" if kind == "m" else f"{x:g}" for x in v) + "]")
        return out


@pytest.fixture(params=["f32", "f64"])
def env(request, monkeypatch):
    """(E, run): run(fn) → (described return or None, error text or None, the calls fn made)"""
    from bvh_amd.instances import Instances
    _lib, api = tam._lib, tam.api
    real_load, real_ctx, real_name = _lib.load, api._default_ctx, tam.TREE_DTYPE
    before = {id(o) for o in api._live}
    sfx = request.param
    lib = Lib()
    tam.TREE_DTYPE = "float32" if sfx == "f32" else "float64"
    _lib.load = lambda: lib
    real_out = api._out_cols
    monkeypatch.setattr(api, "_torch_sync", lambda device: None)                       # (no torch stream to wait for)
    monkeypatch.setattr(api, "_out_cols", lambda device, ft, *cols: real_out(None, ft, *cols))
    try:
        E = tam.Env(lib, sfx)
        E.inst = Instances([E.flat], [0, 0], (np.arange(NI * 12) * 0.5).astype(E.ft).reshape(NI, 12))
        E.mask = np.array([1, 0x80000000, 0, 0xFFFFFFFF], dtype=np.uint32)
        E.dmask = lambda numel=N, name="int32": tam.FakeTensor(name, numel)
        E.pl = (np.arange(N * NM * 4) * 0.5 - 2).astype(E.ft).reshape(N, NM, 4)
        E.dpl = lambda name=None: tim._shaped(name or E.tname, (N, NM, 4))

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
    from bvh_amd.instances import Instances, InstancesMaskedQueries, InstancesMasks, InstancesTreeForm
    assert issubclass(Instances, InstancesMaskedQueries)
    assert {k for k in vars(InstancesMaskedQueries) if not k.startswith("_")} == NAMES
    for name in vars(InstancesMaskedQueries):                # none of them shadows or is shadowed by a name of the set's other classes
        for other in (Instances, InstancesMasks, InstancesTreeForm, tam.api._Typed):
            assert name.startswith("__") or name not in vars(other), (name, other)
    names = {s[0] for s in tam._lib.SYMBOLS}
    for e in ("within_masked", "knearest_masked", "knearest_tree_masked", "region_masked"):
        assert {f"bvhgpu_instances_{e}_f32", f"bvhgpu_instances_{e}_f64"} <= names, e
    import os
    src = open(os.path.join(tim.ROOT, "bvh_amd", "instances.py")).read()
    body = src[src.index("class InstancesMaskedQueries"):src.index("class Instances(")]
    assert "raise" not in body                               # its refusals are api.py's


def test_within_calls_and_returns(env):
    E, run = env
    s, H, D, L = E.inst, tam._lib.HOST, tam._lib.DEVICE, tam._lib
    md = 2 + np.arange(N) * 0.25
    for so in (True, False):
        for co in (False, True):
            flags = (0 if so else L.INSTANCES_WITHIN_LIST_ORDER) | (L.INSTANCES_WITHIN_COUNT_ONLY if co else 0)
            P = "NULL" if co else "P"
            tail = ([] if co else ["hits_info(P,NULL,OUT,NULL)"]) + [f"hits_fetch_instances_within(P,P,{P},{P},{P},{H})"]
            ret = f"offsets=uint32[{N + 1}]" + ("" if co else " instance=uint32[5] shape=uint32[5] dist=T[5]")
            assert run(lambda: s.within_masked_batch(E.pts, E.md, E.mask, so, co)) == \
                (ret, None, [f"instances_within_masked_T(P,P,P,P,{N},{H},{flags},OUT)" + fl(md) + hx(E.mask)] + tail)
            assert run(lambda: s.within_masked_batch(E.pts, E.md, None, sort=so, count_only=co)) == \
                (ret, None, [f"instances_within_masked_T(P,P,P,NULL,{N},{H},{flags},OUT)" + fl(md)] + tail)
            assert run(lambda: s.within_masked_batch(E.pts, 1.5, 0x80000000, sort=so, count_only=co))[2][0] == \
                f"instances_within_masked_T(P,P,P,P,{N},{H},{flags},OUT)" + fl([1.5] * N) + hx([0x80000000] * N)
    want = [f"instances_within_masked_T(P,P,P,P,{N},{H},0,OUT)" + fl(md) + hx(E.mask)]
    for mk in (E.mask.tolist(), E.mask.astype(np.int64), E.mask.view(np.int32), E.mask.reshape(2, 2)):
        assert run(lambda: s.within_masked_batch(E.pts.tolist(), E.md, mk))[2][:1] == want, mk
    assert run(lambda: s.within_masked_batch(E.pts, max_dist=E.md.tolist(), point_mask=E.mask))[2][:1] == want
    # points in HBM: the tensors' own memory is handed over (the side arrays made contiguous)
    assert run(lambda: s.within_masked_batch(E.dev(N * 3), E.dev(N), E.dmask()))[2][0] == f"instances_within_masked_T(P,Dc,Dc,Dc,{N},{D},0,OUT)"
    assert run(lambda: s.within_masked_batch(E.dev(N * 3), E.dev(N), None))[2][0] == f"instances_within_masked_T(P,Dc,Dc,NULL,{N},{D},0,OUT)"
    E.lib.total = 0                                           # an empty result: every column NULL in the fetch
    try:
        assert run(lambda: s.within_masked_batch(E.pts, E.md, E.mask))[2][-1] == f"hits_fetch_instances_within(P,P,NULL,NULL,NULL,{H})"
    finally:
        E.lib.total = 5


def test_knearest_calls_and_returns(env):
    E, run = env
    s, H, D = E.inst, tam._lib.HOST, tam._lib.DEVICE
    md = 2 + np.arange(N) * 0.25
    for k in (1, 3, 64, 0, 65, -1):
        rows = k if 1 <= k <= 64 else 0                       # (out of range: the engine refuses, the binding allocates nothing)
        shapes = [f"uint32[{N}, {rows}]", f"uint32[{N}, {rows}]", f"T[{N}, {rows}]"]
        ret, err, calls = run(lambda: s.knearest_masked_batch(E.pts, k, E.mask))
        assert err is None and calls == [f"instances_knearest_masked_T(P,P,P,{N},{H},{k & 0xFFFFFFFF},P,P,P)" + hx(E.mask)] and ret == shapes
        ret, err, calls = run(lambda: s.knearest_tree_masked_batch(E.pts, k, E.mask))
        assert err is None and calls == [f"instances_knearest_tree_masked_T(P,P,P,{N},{H},{k & 0xFFFFFFFF},NULL,P,P,P)" + hx(E.mask)] and ret == shapes
    assert run(lambda: s.knearest_masked_batch(E.pts, 2, None))[2] == [f"instances_knearest_masked_T(P,P,NULL,{N},{H},2,P,P,P)"]
    assert run(lambda: s.knearest_masked_batch(E.pts.tolist(), 2.0, 9))[2] == [f"instances_knearest_masked_T(P,P,P,{N},{H},2,P,P,P)" + hx([9] * N)]
    assert run(lambda: s.knearest_masked_batch(E.dev(N * 3), 2, E.dmask()))[1:] == (None, [f"instances_knearest_masked_T(P,Dc,Dc,{N},{D},2,P,P,P)"])
    assert run(lambda: s.knearest_masked_batch(E.dev(N * 3), 2, None))[1:] == (None, [f"instances_knearest_masked_T(P,Dc,NULL,{N},{D},2,P,P,P)"])
    ret, err, calls = run(lambda: s.nearest_masked_batch(E.pts, E.mask.view(np.int32)))
    assert err is None and calls == [f"instances_knearest_masked_T(P,P,P,{N},{H},1,P,P,P)" + hx(E.mask)]
    assert ret == [f"uint32[{N}]", f"uint32[{N}]", f"T[{N}]"]
    # the tree form: max_dist after k, the mask beside the points
    want = [f"instances_knearest_tree_masked_T(P,P,P,{N},{H},2,P,P,P,P)" + fl(md) + hx(E.mask)]
    for m in (E.md, E.md.tolist(), E.md.reshape(2, 2)):
        assert run(lambda: s.knearest_tree_masked_batch(E.pts, 2, E.mask, m))[1:] == (None, want)
    assert run(lambda: s.knearest_tree_masked_batch(E.pts, 2, point_mask=E.mask.tolist(), max_dist=E.md))[2] == want
    assert run(lambda: s.knearest_tree_masked_batch(E.pts, 2, None, 1.5))[2] == [f"instances_knearest_tree_masked_T(P,P,NULL,{N},{H},2,P,P,P,P)" + fl([1.5] * N)]
    assert run(lambda: s.knearest_tree_masked_batch(E.pts, 2, 5, 1.5))[2] == \
        [f"instances_knearest_tree_masked_T(P,P,P,{N},{H},2,P,P,P,P)" + fl([1.5] * N) + hx([5] * N)]
    assert run(lambda: s.knearest_tree_masked_batch(E.dev(N * 3), 2, E.dmask(), E.dev(N)))[1:] == \
        (None, [f"instances_knearest_tree_masked_T(P,Dc,Dc,{N},{D},2,Dc,P,P,P)"])
    ret, err, calls = run(lambda: s.nearest_tree_masked_batch(E.pts, E.mask, E.md))
    assert err is None and calls == [f"instances_knearest_tree_masked_T(P,P,P,{N},{H},1,P,P,P,P)" + fl(md) + hx(E.mask)]
    assert ret == [f"uint32[{N}]", f"uint32[{N}]", f"T[{N}]"]
    assert run(lambda: s.nearest_tree_masked_batch(E.pts, None))[2] == [f"instances_knearest_tree_masked_T(P,P,NULL,{N},{H},1,NULL,P,P,P)"]


def test_region_calls_and_returns(env):
    E, run = env
    s, H, D, L = E.inst, tam._lib.HOST, tam._lib.DEVICE, tam._lib
    for cl in (False, True):
        for co in (False, True):
            for io in (False, True):
                classify = cl and not co
                flags = (L.REGION_COUNT_ONLY if co else 0) | (L.REGION_CLASSIFY if classify else 0) | (L.REGION_INSTANCES_ONLY if io else 0)
                cols = ["NULL" if co else "P", "NULL" if co or io else "P", "P" if classify else "NULL"]
                tail = ([] if co else ["hits_info(P,NULL,OUT,NULL)"]) + [f"hits_fetch_instances_region(P,P,{cols[0]},{cols[1]},{cols[2]},{H})"]
                ret, err, calls = run(lambda: s.region_masked_batch(E.pl, E.mask, classify=cl, count_only=co, instances_only=io))
                assert err is None and calls == [f"instances_region_masked_T(P,P,P,{N},{NM},{H},{flags},OUT)" + hx(E.mask)] + tail, (cl, co, io, calls)
                keys = ["offsets", "instance"] + ([] if io else ["shape"]) + (["inside"] if classify else [])
                assert [p.split("=")[0] for p in ret.split(" ")] == keys, (ret, keys)
    assert run(lambda: s.region_masked_batch(E.pl, None))[2][0] == f"instances_region_masked_T(P,P,NULL,{N},{NM},{H},0,OUT)"
    assert run(lambda: s.region_masked_batch(E.pl.tolist(), 7, True, False, True))[2][0] == \
        f"instances_region_masked_T(P,P,P,{N},{NM},{H},{L.REGION_CLASSIFY | L.REGION_INSTANCES_ONLY},OUT)" + hx([7] * N)
    # one region given as (m, 4): one mask
    assert run(lambda: s.region_masked_batch(E.pl[0], [3]))[2][0] == f"instances_region_masked_T(P,P,P,1,{NM},{H},0,OUT)" + hx([3])
    assert run(lambda: s.region_masked_batch(E.pl[0], 0xC))[2][0] == f"instances_region_masked_T(P,P,P,1,{NM},{H},0,OUT)" + hx([0xC])
    assert run(lambda: s.region_masked_batch(E.dpl(), E.dmask()))[2][0] == f"instances_region_masked_T(P,Dc,Dc,{N},{NM},{D},0,OUT)"
    assert run(lambda: s.region_masked_batch(E.dpl(), None, classify=True))[2][0] == f"instances_region_masked_T(P,Dc,NULL,{N},{NM},{D},{L.REGION_CLASSIFY},OUT)"


def test_python_side_refusals(env):
    """api._needs', api._rows_in's, api._side_in's, region._plane_dims' and api._mask_in's refusals come before anything is handed over"""
    E, run = env
    s = E.inst
    I, Dm = tam._lib.INVALID_ARG, tam._lib.DTYPE_MISMATCH
    calls_of = {
        "within_masked_batch": (lambda m, p=None: s.within_masked_batch(E.pts if p is None else p, 1.0 if p is None else E.dev(N), m), "point", "points", lambda: E.dev(N * 3)),
        "knearest_masked_batch": (lambda m, p=None: s.knearest_masked_batch(E.pts if p is None else p, 2, m), "point", "points", lambda: E.dev(N * 3)),
        "nearest_masked_batch": (lambda m, p=None: s.nearest_masked_batch(E.pts if p is None else p, m), "point", "points", lambda: E.dev(N * 3)),
        "knearest_tree_masked_batch": (lambda m, p=None: s.knearest_tree_masked_batch(E.pts if p is None else p, 2, m), "point", "points", lambda: E.dev(N * 3)),
        "nearest_tree_masked_batch": (lambda m, p=None: s.nearest_tree_masked_batch(E.pts if p is None else p, m), "point", "points", lambda: E.dev(N * 3)),
        "region_masked_batch": (lambda m, p=None: s.region_masked_batch(E.pl if p is None else p, m), "region", "regions", lambda: E.dpl())}
    assert set(calls_of) == NAMES
    for name, (f, one, of, dev) in calls_of.items():
        what = f"{one}_mask"
        for fn, status, text in (
                (lambda: f(E.mask[:3]), I, f"{what} has 3 values for 4 {of}"),
                (lambda: f(np.zeros(N + 1, np.uint32)), I, f"{what} has 5 values for 4 {of}"),
                (lambda: f(E.dmask()), I, f"{what} is a GPU tensor but the {of} are in host memory"),
                (lambda: f(E.mask, dev()), I, f"{what} is in host memory but the {of} are in HBM"),
                (lambda: f(E.mask.tolist(), dev()), I, f"{what} is in host memory but the {of} are in HBM"),
                (lambda: f(E.dmask(N + 1), dev()), I, f"{what} has 5 values for 4 {of}"),
                (lambda: f(E.dmask(N, "int64"), dev()), Dm, f"{what} must be a torch.int32 tensor (its bits are the masks)"),
                (lambda: f(E.dmask(N, E.tname), dev()), Dm, f"{what} must be a torch.int32 tensor (its bits are the masks)"),
                (lambda: f(E.mask.astype(E.ft)), Dm, f"{what} must be integers"),
                (lambda: f([0.5] * N), Dm, f"{what} must be integers"),
                (lambda: f(np.array([0, 1, 2, -1], dtype=np.int64)), I, f"{what} values must be in [0, 2^32)"),
                (lambda: f([0, 1, 2, 1 << 32]), I, f"{what} values must be in [0, 2^32)"),
                (lambda: f(-1), I, f"{what} must be in [0, 2^32), not -1"),
                (lambda: f(1 << 32), I, f"{what} must be in [0, 2^32), not 4294967296")):
            ret, err, calls = run(fn)
            assert err == f"BvhGpuError status={status}: bvhgpu status {status}: {text}" and calls == [], (name, err, calls)
    for fn, status, text in (
            (lambda: s.within_masked_batch(E.pts, None, E.mask), I, "within_masked_batch needs max_dist (a scalar or one value per point)"),
            (lambda: s.within_masked_batch(E.pts.astype(E.other), 1.0, E.mask), Dm, "point dtype differs from tree dtype"),
            (lambda: s.within_masked_batch(E.pts, E.md[:3], E.mask), I, "max_dist has 3 values for 4 points"),
            (lambda: s.within_masked_batch(E.pts, E.md.astype(E.other), E.mask), Dm, "max_dist dtype differs from tree dtype"),
            (lambda: s.within_masked_batch(E.dev(N * 3), E.md, E.dmask()), I, "max_dist is in host memory but the points are in HBM"),
            (lambda: s.knearest_masked_batch(E.pts.astype(E.other), 2, E.mask), Dm, "point dtype differs from tree dtype"),
            (lambda: s.knearest_masked_batch(E.dev(N * 3, wrong=True), 2, E.dmask()), Dm, "point dtype differs from tree dtype"),
            (lambda: s.knearest_tree_masked_batch(E.pts, 2, E.mask, E.md[:3]), I, "max_dist has 3 values for 4 points"),
            (lambda: s.knearest_tree_masked_batch(E.pts, 2, E.mask, E.dev(N)), I, "max_dist is a GPU tensor but the points are in host memory"),
            (lambda: s.nearest_tree_masked_batch(E.pts.astype(E.other), E.mask), Dm, "point dtype differs from tree dtype"),
            (lambda: s.region_masked_batch(E.pl.astype(E.other), E.mask), Dm, "plane dtype differs from tree dtype"),
            (lambda: s.region_masked_batch(np.zeros((N, NM, 3), dtype=E.ft), E.mask), I, "planes must be (n, m, 4) or (m, 4), not (4, 2, 3)"),
            (lambda: s.region_masked_batch(E.pl[0], E.mask), I, "region_mask has 4 values for 1 regions")):
        ret, err, calls = run(fn)
        assert err == f"BvhGpuError status={status}: bvhgpu status {status}: {text}" and calls == [], (err, calls)
    with pytest.raises(ValueError):
        s.knearest_masked_batch(np.arange(7).astype(E.ft), 2, None)

"""What the masked methods of an instance set (bvh_amd/instances.py, class InstancesMasks: set_masks, masks, closest_hits_masked,
any_hits_masked, occluded_masked, khits_masked_batch, allhits_masked_batch) hand to the C ABI: tests/test_instances_marshal_cpu.py's recording
library and inputs, with the expected calls, returns and refusals written out here (no recorded file).  Rays in HBM are the duck-typed GPU
tensor of tests/test_api_marshal_cpu.py; where a call on them gets as far as allocating outputs, the outputs are made on the host instead
(the pointers handed over for the inputs are what is looked at).  Needs no GPU and no .so."""
from __future__ import annotations

import numpy as np
import pytest

import test_api_marshal_cpu as tam
import test_instances_marshal_cpu as tim

N, NI = tim.N, tim.NI
C = tam.C
# entry stem → (tmax arg, ray_mask arg, count arg, mem arg)
RAY_ENTRIES = {"instances_trace_masked": (2, 3, 4, 5), "instances_khits_masked": (2, 3, 4, 5), "instances_allhits_masked": (2, 3, 4, 5)}


class Lib(tim.Lib):
    """... which also shows the host values of the masked entries' tmax (floats) and masks (hexadecimal)"""
    masks = [0x11, 0x80000002]

    def _values(self, name, args):
        stem, _, sfx = name.rpartition("_")
        if name == "instances_set_masks":
            cols = [(1, 2, 3, np.uint32)]
        elif stem in RAY_ENTRIES:
            t, m, n, mem = RAY_ENTRIES[stem]
            cols = [(t, n, mem, np.float32 if sfx == "f32" else np.float64), (m, n, mem, np.uint32)]
        else:
            return tim.Lib._values(self, name, args)
        out = []
        for p, n, mem, dt in cols:
            a = args[p]
            if not isinstance(a, C.c_void_p) or not a.value or args[mem] != tam._lib.HOST or not 0 < int(args[n]) <= 256:
                continue
            raw = (C.c_char * (int(args[n]) * np.dtype(dt).itemsize)).from_address(a.value)
            v = np.frombuffer(raw, dtype=dt).tolist()
            out.append(" [" + " ".join(f"{x:#x}" if dt is np.uint32 else f"{x:g}" for x in v) + "]")
        return out

    def _answer(self, name, args):
        rc = tim.Lib._answer(self, name, args)
        if name == "instances_masks":
            (C.c_uint32 * NI).from_address(args[1].value)[:] = self.masks
        return rc


def fl(a):
    return " [" + " ".join(f"{x:g}" for x in np.asarray(a, dtype=np.float64).reshape(-1).tolist()) + "]"


def hx(a):
    return " [" + " ".join(f"{int(x):#x}" for x in np.asarray(a).reshape(-1).tolist()) + "]"


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
    from bvh_amd.instances import Instances, InstancesMasks
    assert issubclass(Instances, InstancesMasks)
    assert {k for k in vars(InstancesMasks) if not k.startswith("_")} == {
        "set_masks", "masks", "closest_hits_masked", "any_hits_masked", "occluded_masked", "khits_masked_batch", "allhits_masked_batch"}
    for name in vars(InstancesMasks):                        # none of them shadows or is shadowed by one of Instances' own
        assert name.startswith("__") or name not in vars(Instances), name
    names = {s[0] for s in tam._lib.SYMBOLS}
    for e in ("set_masks", "masks", "trace_masked_f32", "trace_masked_f64", "khits_masked_f32", "khits_masked_f64", "allhits_masked_f32",
              "allhits_masked_f64"):
        assert "bvhgpu_instances_" + e in names, e


def test_set_masks_and_masks(env):
    E, run = env
    s, H, D = E.inst, tam._lib.HOST, tam._lib.DEVICE
    m = np.array([0x11, 0x80000002], dtype=np.uint32)
    want = [f"instances_set_masks(P,P,{NI},{H})" + hx(m)]
    for v in (m, m.tolist(), m.astype(np.int64), m.astype(np.uint64), m.view(np.int32), m.reshape(2, 1)):
        ret, err, calls = run(lambda: s.set_masks(v) is s)
        assert (ret, err, calls) == (True, None, want), (v, err, calls)
    assert run(lambda: s.set_masks(None) is s) == (True, None, [f"instances_set_masks(P,NULL,{NI},{H})"])
    assert run(lambda: s.set_masks(E.dmask(NI)) is s) == (True, None, [f"instances_set_masks(P,Dc,{NI},{D})"])
    assert run(lambda: s.masks) == ("uint32[2]", None, [f"instances_masks(P,P,{H})"])
    assert s.masks.tolist() == Lib.masks


def test_trace_calls_and_returns(env):
    E, run = env
    s, H, D, F = E.inst, tam._lib.HOST, tam._lib.DEVICE, tam._lib.TRAVERSE_FIRST
    tmax = 1 + np.arange(N) * 0.5
    rows = [f"T[{N}, 3]", f"uint32[{N}]", f"uint32[{N}]"]
    for m, flags, ret_want in (("closest_hits_masked", 0, rows), ("any_hits_masked", F, rows), ("occluded_masked", F, f"bool[{N}]")):
        fn = getattr(s, m)
        assert run(lambda: fn(E.rays, None)) == (ret_want, None, [f"instances_trace_masked_T(P,P,NULL,NULL,{N},{H},{flags},P,P,P)"])
        assert run(lambda: fn(E.rays, E.mask)) == (ret_want, None, [f"instances_trace_masked_T(P,P,NULL,P,{N},{H},{flags},P,P,P)" + hx(E.mask)])
        want = [f"instances_trace_masked_T(P,P,P,P,{N},{H},{flags},P,P,P)" + fl(tmax) + hx(E.mask)]
        for mk in (E.mask, E.mask.tolist(), E.mask.astype(np.int64), E.mask.view(np.int32), E.mask.reshape(2, 2)):
            assert run(lambda: fn(E.rays, mk, E.tmax))[1:] == (None, want), mk
        assert run(lambda: fn(E.rays, ray_mask=E.mask, tmax=E.tmax.tolist()))[2] == want
        for v in (0, 5, 0x80000000, 0xFFFFFFFF, np.uint32(12), np.int64(3)):             # a scalar is every ray's mask
            assert run(lambda: fn(E.rays, v))[2] == [f"instances_trace_masked_T(P,P,NULL,P,{N},{H},{flags},P,P,P)" + hx([int(v)] * N)]
        # rays in HBM: the tensors' own memory is handed over (the mask made contiguous)
        assert run(lambda: fn(E.drays, None))[1:] == (None, [f"instances_trace_masked_T(P,D,NULL,NULL,{N},{D},{flags},P,P,P)"])
        assert run(lambda: fn(E.drays, E.dmask()))[1:] == (None, [f"instances_trace_masked_T(P,D,NULL,Dc,{N},{D},{flags},P,P,P)"])
        assert run(lambda: fn(E.drays, E.dmask(), E.dev(N)))[1:] == (None, [f"instances_trace_masked_T(P,D,Dc,Dc,{N},{D},{flags},P,P,P)"])


def test_khits_calls_and_returns(env):
    E, run = env
    s, H, D = E.inst, tam._lib.HOST, tam._lib.DEVICE
    tmax = 1 + np.arange(N) * 0.5
    for k in (1, 3, 64, 0, 65, -1):
        rows = k if 1 <= k <= 64 else 0                       # (out of range: the engine refuses, the binding allocates nothing)
        ret, err, calls = run(lambda: s.khits_masked_batch(E.rays, k, E.mask))
        assert err is None and calls == [f"instances_khits_masked_T(P,P,NULL,P,{N},{H},{k & 0xFFFFFFFF},P,P,P)" + hx(E.mask)]
        assert ret == [f"uint32[{N}, {rows}]", f"uint32[{N}, {rows}]", f"T[{N}, {rows}, 3]"]
    assert run(lambda: s.khits_masked_batch(E.rays, 2, None))[2] == [f"instances_khits_masked_T(P,P,NULL,NULL,{N},{H},2,P,P,P)"]
    assert run(lambda: s.khits_masked_batch(E.rays, 2.0, 9, E.tmax))[2] == [f"instances_khits_masked_T(P,P,P,P,{N},{H},2,P,P,P)" + fl(tmax) + hx([9] * N)]
    assert run(lambda: s.khits_masked_batch(E.drays, 2, E.dmask(), E.dev(N)))[1:] == (None, [f"instances_khits_masked_T(P,D,Dc,Dc,{N},{D},2,P,P,P)"])


def test_allhits_calls_and_returns(env):
    E, run = env
    s, H, L = E.inst, tam._lib.HOST, tam._lib
    tmax = 1 + np.arange(N) * 0.5
    for so in (True, False):
        for co in (False, True):
            flags = (0 if so else L.INSTANCES_ALLHITS_LIST_ORDER) | (L.INSTANCES_ALLHITS_COUNT_ONLY if co else 0)
            P = "NULL" if co else "P"
            tail = ([] if co else ["hits_info(P,NULL,OUT,NULL)"]) + [f"hits_fetch_instances_allhits(P,P,{P},{P},{P},{H})"]
            ret = f"offsets=uint32[{N + 1}]" + ("" if co else " instance=uint32[5] shape=uint32[5] vals=T[5, 3]")
            assert run(lambda: s.allhits_masked_batch(E.rays, E.mask, None, so, co)) == \
                (ret, None, [f"instances_allhits_masked_T(P,P,NULL,P,{N},{H},{flags},OUT)" + hx(E.mask)] + tail)
            assert run(lambda: s.allhits_masked_batch(E.rays, None, E.tmax, sort=so, count_only=co)) == \
                (ret, None, [f"instances_allhits_masked_T(P,P,P,NULL,{N},{H},{flags},OUT)" + fl(tmax)] + tail)
            assert run(lambda: s.allhits_masked_batch(E.rays, 0x80000000, E.tmax, sort=so, count_only=co))[2][0] == \
                f"instances_allhits_masked_T(P,P,P,P,{N},{H},{flags},OUT)" + fl(tmax) + hx([0x80000000] * N)
    E.lib.total = 0                                           # an empty result: every column NULL in the fetch
    try:
        assert run(lambda: s.allhits_masked_batch(E.rays, E.mask))[2][-1] == f"hits_fetch_instances_allhits(P,P,NULL,NULL,NULL,{H})"
    finally:
        E.lib.total = 5


def test_python_side_refusals(env):
    """the ray dtype, api._side_in's and api._mask_in's refusals come before anything is handed over"""
    E, run = env
    s = E.inst
    I, Dm = tam._lib.INVALID_ARG, tam._lib.DTYPE_MISMATCH
    calls_of = {
        "closest_hits_masked": lambda r, m, t=None: s.closest_hits_masked(r, m, t), "any_hits_masked": lambda r, m, t=None: s.any_hits_masked(r, m, t),
        "occluded_masked": lambda r, m, t=None: s.occluded_masked(r, m, t), "khits_masked_batch": lambda r, m, t=None: s.khits_masked_batch(r, 2, m, t),
        "allhits_masked_batch": lambda r, m, t=None: s.allhits_masked_batch(r, m, t)}
    for name, f in calls_of.items():
        for fn, status, text in (
                (lambda: f(E.orays, E.mask), Dm, "ray dtype differs from the instance set's dtype"),
                (lambda: f(E.rays, E.mask, E.tmax.astype(E.other)), Dm, "tmax dtype differs from tree dtype"),
                (lambda: f(E.rays, E.mask, E.tmax[:3]), I, "tmax has 3 values for 4 rays"),
                (lambda: f(E.rays, E.mask[:3]), I, "ray_mask has 3 values for 4 rays"),
                (lambda: f(E.rays, np.zeros(N + 1, np.uint32)), I, "ray_mask has 5 values for 4 rays"),
                (lambda: f(E.rays, E.dmask()), I, "ray_mask is a GPU tensor but the rays are in host memory"),
                (lambda: f(E.drays, E.mask), I, "ray_mask is in host memory but the rays are in HBM"),
                (lambda: f(E.drays, E.mask.tolist()), I, "ray_mask is in host memory but the rays are in HBM"),
                (lambda: f(E.drays, E.dmask(N + 1)), I, "ray_mask has 5 values for 4 rays"),
                (lambda: f(E.drays, E.dmask(N, "int64")), Dm, "ray_mask must be a torch.int32 tensor (its bits are the masks)"),
                (lambda: f(E.drays, E.dmask(N, E.tname)), Dm, "ray_mask must be a torch.int32 tensor (its bits are the masks)"),
                (lambda: f(E.rays, E.mask.astype(E.ft)), Dm, "ray_mask must be integers"),
                (lambda: f(E.rays, [0.5] * N), Dm, "ray_mask must be integers"),
                (lambda: f(E.rays, np.array([0, 1, 2, -1], dtype=np.int64)), I, "ray_mask values must be in [0, 2^32)"),
                (lambda: f(E.rays, [0, 1, 2, 1 << 32]), I, "ray_mask values must be in [0, 2^32)"),
                (lambda: f(E.rays, -1), I, "ray_mask must be in [0, 2^32), not -1"),
                (lambda: f(E.rays, 1 << 32), I, "ray_mask must be in [0, 2^32), not 4294967296")):
            ret, err, calls = run(fn)
            assert err == f"BvhGpuError status={status}: bvhgpu status {status}: {text}" and calls == [], (name, err, calls)
    for fn, status, text in (
            (lambda: s.set_masks([1, 2, 3]), I, "masks has 3 values for 2 instances"),
            (lambda: s.set_masks(7), I, "masks has 1 values for 2 instances"),
            (lambda: s.set_masks(E.dmask(NI + 1)), I, "masks has 3 values for 2 instances"),
            (lambda: s.set_masks(E.dmask(NI, "int64")), Dm, "masks must be a torch.int32 tensor (its bits are the masks)"),
            (lambda: s.set_masks([0.5, 1.0]), Dm, "masks must be integers"),
            (lambda: s.set_masks([-1, 0]), I, "masks values must be in [0, 2^32)")):
        ret, err, calls = run(fn)
        assert err == f"BvhGpuError status={status}: bvhgpu status {status}: {text}" and calls == [], (err, calls)

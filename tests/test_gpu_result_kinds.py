"""Which accessor reads which kind of result: one result object is handed through every batch family in turn, and after each batch all
fourteen accessors of a bvhgpu_hits are called on it.  The table below is written from include/bvh_mi355x.h: per (held batch, accessor)
the status, and where the header promises it, that the refusal names the accessor which does read the held kind.  A refused call leaves
the caller's arrays untouched, and the held kind's own accessor returns the same bytes before and after the thirteen other calls.
Nothing here provokes a fault: every refusal is made on the host before anything is copied."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID_ARG = 0, 1
HOST = 0
LEAF_TRIANGLE = 1
N = 4
FILL_U, FILL_F, FILL_P = 0xABABABAB, 7.0, 0xABAB

# the fourteen accessors, in the table's column order
ACCESSORS = ["fetch", "fetch_triangles", "fetch_closest", "fetch_any", "fetch_box", "fetch_sphere", "fetch_allhits", "fetch_within",
             "fetch_region", "fetch_instances_region", "fetch_instances_allhits", "fetch_instances_within", "region_info", "device"]
# per held batch: the accessor that reads its kind, and one cell per accessor —
#   K  BVHGPU_OK
#   n  BVHGPU_INVALID_ARG, and the message names the reader of the held kind
#   -  BVHGPU_INVALID_ARG (the message is the accessor's own "holds no ..." / "was run without ...")
#   o  BVHGPU_INVALID_ARG from the kind's own accessor: an output was asked for that the batch's flags did not request (OPTION has the text)
TABLE = {
    #                                                          f t c a b s A W R I X Y i d
    "csr":               ("bvhgpu_hits_fetch",                   "K o - - - - - - n n - - - K"),
    "csr_t_slice":       ("bvhgpu_hits_fetch",                   "K o - - - - - - n n - - - K"),
    "csr_triangles":     ("bvhgpu_hits_fetch",                   "K K - - - - - - n n - - - K"),
    "closest":           ("bvhgpu_hits_fetch_closest",           "n - K - - - - - n n - - - -"),
    "any":               ("bvhgpu_hits_fetch_any",               "n - - K - - - - n n - - - -"),
    "box":               ("bvhgpu_hits_fetch_box",               "n - - - K - - - n n - - - -"),
    "sphere":            ("bvhgpu_hits_fetch_sphere",            "n n n n n K - - n n - - - n"),
    "query":             ("bvhgpu_hits_fetch",                   "K o - - - - - - n n - - - K"),
    "allhits":           ("bvhgpu_hits_fetch_allhits",           "n n n n n n K - n n - - - n"),
    "within":            ("bvhgpu_hits_fetch_within",            "n n n n n n n K n n - - - n"),
    "within_count":      ("bvhgpu_hits_fetch_within",            "n n n n n n n K n n - - - n"),
    "region":            ("bvhgpu_hits_fetch_region",            "n n n n n n n n K n - - K n"),
    "inst_region":       ("bvhgpu_hits_fetch_instances_region",  "- - - - - - - - n K - - K -"),
    "inst_region_only":  ("bvhgpu_hits_fetch_instances_region",  "- - - - - - - - n o - - K -"),
    "inst_allhits":      ("bvhgpu_hits_fetch_instances_allhits", "n n n n n n n n n n K - - n"),
    "inst_within":       ("bvhgpu_hits_fetch_instances_within",  "n n n n n n n n n n n K - n"),
    "inst_within_count": ("bvhgpu_hits_fetch_instances_within",  "n n n n n n n n n n n o - n"),
}
OPTION = {("csr", "fetch_triangles"): "BVHGPU_TRAVERSE_TRIANGLES", ("csr_t_slice", "fetch_triangles"): "BVHGPU_TRAVERSE_TRIANGLES",
          ("query", "fetch_triangles"): "BVHGPU_TRAVERSE_TRIANGLES", ("inst_region_only", "fetch_instances_region"): "BVHGPU_REGION_INSTANCES_ONLY",
          ("inst_within_count", "fetch_instances_within"): "COUNT_ONLY"}
# message parts that callers already rely on (tests/test_gpu_capi_refusals.py and the families' own suites)
PINNED = {("csr", "fetch_closest"): "traverse was run without BVHGPU_TRAVERSE_CLOSEST",
          ("csr", "fetch_any"): "the result object holds no bvhgpu_traverse_any_* batch",
          ("within", "fetch_instances_within"): "no bvhgpu_instances_within_",
          ("closest", "fetch_instances_allhits"): "no bvhgpu_instances_allhits_",
          ("inst_within", "fetch_instances_allhits"): "use bvhgpu_hits_fetch_instances_within",
          ("inst_allhits", "fetch_within"): "use bvhgpu_hits_fetch_instances_allhits",
          ("inst_region", "fetch"): "bvhgpu_hits_fetch_region", ("inst_region", "fetch_region"): "bvhgpu_hits_fetch_instances_region"}


class Scene:
    """8 cubes (96 triangles, their spheres set), 2 instances of that tree, 4 rays, 4 points and 4 regions, f32"""

    def __init__(self, eng):
        from bvh_amd import _lib, testbase as tb
        assert (_lib.LEAF_TRIANGLE, _lib.QUERY_AABB) == (LEAF_TRIANGLE, 1)
        self.lib, self.ptr = _lib.load(), _lib.ptr
        self.ctx = eng.Context(0)
        tris, aabbs = tb.create_n_cubes(8)
        assert tris.shape == (96, 3, 3) and aabbs.shape == (96, 6)
        self.aabbs, self.tris = np.ascontiguousarray(aabbs, np.float32), np.ascontiguousarray(tris, np.float32)
        centres = tris.reshape(8, 36, 3).astype(np.float64).mean(axis=1)[:N]
        self.tree = eng.Bvh.from_aabbs(self.aabbs, self.ctx).flatten()
        self.tree.set_triangles(self.tris)
        c = (self.aabbs[:, :3] + self.aabbs[:, 3:]) / 2
        r = np.linalg.norm(self.aabbs[:, 3:] - self.aabbs[:, :3], axis=1, keepdims=True) / 2
        self.tree.set_spheres(np.ascontiguousarray(np.concatenate([c, r], axis=1), np.float32))
        # a ray through every one of the first four cubes (off the diagonal of its faces), a point in its middle, a box region around it
        self.rays = eng.RayBatch.new(centres + [0.11, 0.07, -1000.0], np.tile([0.0, 0.0, 1.0], (N, 1)), np.float32, self.ctx).host
        self.points = np.ascontiguousarray(centres, np.float32)
        self.limits = np.full(N, 1.5, np.float32)
        self.boxes = np.ascontiguousarray(np.concatenate([centres - 1.0, centres + 1.0], axis=1), np.float32)   # (BVHGPU_QUERY_AABB)
        self.planes = np.ascontiguousarray(np.stack([eng.aabb_planes(p - 1.0, p + 1.0) for p in centres]), np.float32)
        x = np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (2, 1))
        x[1, 3] = 0.25                                      # the second instance: the same tree moved along x
        self.inst = eng.Instances([self.tree], np.zeros(2, np.uint32), x, self.ctx)
        self.h = C.c_void_p()                               # ONE result object for every batch below
        self.so, self.si, self.ss = (np.full(n, FILL_U, np.uint32) for n in (64, 4096, 4096))
        self.sv = np.full((4096, 3), FILL_F, np.float32)
        self.info = [C.c_uint32(FILL_P), C.c_uint32(FILL_P)]
        self.dev = [C.c_void_p(FILL_P), C.c_void_p(FILL_P), C.c_void_p(FILL_P)]

    def close(self):
        self.lib.bvhgpu_hits_destroy(self.h)
        self.inst.close()

    def error(self):
        return self.lib.bvhgpu_last_error(self.ctx._h).decode()

    def untouched(self):
        return ((self.so == FILL_U).all() and (self.si == FILL_U).all() and (self.ss == FILL_U).all() and (self.sv == FILL_F).all()
                and all(v.value == FILL_P for v in self.info + self.dev))

    def reset(self):
        self.so[:], self.si[:], self.ss[:], self.sv[:] = FILL_U, FILL_U, FILL_U, FILL_F
        for v in self.info + self.dev:
            v.value = FILL_P

    def run(self, held):
        lib, p, t, s, h = self.lib, self.ptr, self.tree._t, self.inst._s, C.byref(self.h)
        rays, pts, lim, planes = p(self.rays), p(self.points), p(self.limits), p(self.planes)
        calls = {
            "csr": lambda: lib.bvhgpu_traverse_f32(t, rays, N, HOST, 0, h),
            "csr_t_slice": lambda: lib.bvhgpu_traverse_f32(t, rays, N, HOST, 1, h),
            "csr_triangles": lambda: lib.bvhgpu_traverse_f32(t, rays, N, HOST, 4, h),
            "closest": lambda: lib.bvhgpu_traverse_f32(t, rays, N, HOST, 8, h),
            "any": lambda: lib.bvhgpu_traverse_any_f32(t, rays, None, N, HOST, 0, h),
            "box": lambda: lib.bvhgpu_traverse_box_f32(t, rays, None, N, HOST, 0, h),
            "sphere": lambda: lib.bvhgpu_traverse_sphere_f32(t, rays, None, N, HOST, 0, h),
            "query": lambda: lib.bvhgpu_query_f32(t, 1, p(self.boxes), N, HOST, 0, h),
            "allhits": lambda: lib.bvhgpu_traverse_allhits_f32(t, rays, None, N, HOST, LEAF_TRIANGLE, 0, h),
            "within": lambda: lib.bvhgpu_within_f32(t, pts, lim, N, HOST, 1, 0, h),
            "within_count": lambda: lib.bvhgpu_within_f32(t, pts, lim, N, HOST, 1, 2, h),
            "region": lambda: lib.bvhgpu_region_f32(t, planes, N, 6, HOST, 0, h),
            "inst_region": lambda: lib.bvhgpu_instances_region_f32(s, planes, N, 6, HOST, 0, h),
            "inst_region_only": lambda: lib.bvhgpu_instances_region_f32(s, planes, N, 6, HOST, 4, h),
            "inst_allhits": lambda: lib.bvhgpu_instances_allhits_f32(s, rays, None, N, HOST, 0, h),
            "inst_within": lambda: lib.bvhgpu_instances_within_f32(s, pts, lim, N, HOST, 0, h),
            "inst_within_count": lambda: lib.bvhgpu_instances_within_f32(s, pts, lim, N, HOST, 2, h),
        }
        keep = self.h.value
        assert calls[held]() == OK, (held, self.error())
        assert keep is None or self.h.value == keep                      # the same object, whatever it held before
        total = C.c_uint64()
        assert lib.bvhgpu_hits_info(self.h, None, C.byref(total), None) == OK
        return int(total.value)

    def call(self, accessor):
        """the accessor with every output pointing into the sentinel arrays"""
        lib, p, h = self.lib, self.ptr, self.h
        so, si, ss, sv = p(self.so), p(self.si), p(self.ss), p(self.sv)
        if accessor == "fetch":
            return lib.bvhgpu_hits_fetch(h, so, ss, None, HOST)
        if accessor == "fetch_triangles":
            return lib.bvhgpu_hits_fetch_triangles(h, sv, HOST)
        if accessor in ("fetch_closest", "fetch_any", "fetch_box", "fetch_sphere"):
            return getattr(lib, "bvhgpu_hits_" + accessor)(h, sv, ss, HOST)
        if accessor in ("fetch_allhits", "fetch_within"):
            return getattr(lib, "bvhgpu_hits_" + accessor)(h, so, ss, sv, HOST)
        if accessor == "fetch_region":
            return lib.bvhgpu_hits_fetch_region(h, so, ss, None, HOST)
        if accessor == "fetch_instances_region":
            return lib.bvhgpu_hits_fetch_instances_region(h, so, si, ss, None, HOST)
        if accessor in ("fetch_instances_allhits", "fetch_instances_within"):
            return getattr(lib, "bvhgpu_hits_" + accessor)(h, so, si, ss, sv, HOST)
        if accessor == "region_info":
            return lib.bvhgpu_hits_region_info(h, C.byref(self.info[0]), C.byref(self.info[1]))
        return lib.bvhgpu_hits_device(h, *(C.byref(v) for v in self.dev))

    def own(self, held, total):
        """everything the held kind's own accessor gives, as bytes (arrays of the batch's own size, not the sentinels)"""
        lib, p, h = self.lib, self.ptr, self.h
        off, a, b = np.zeros(N + 1, np.uint32), np.zeros(max(total, 1), np.uint32), np.zeros(max(total, 1), np.uint32)
        v = np.zeros((max(total, N), 3), np.float32)
        if held in ("csr", "query"):
            rc = lib.bvhgpu_hits_fetch(h, p(off), p(a), None, HOST)
        elif held == "csr_t_slice":
            rc = lib.bvhgpu_hits_fetch(h, p(off), p(a), p(v), HOST)
        elif held == "csr_triangles":
            rc = lib.bvhgpu_hits_fetch(h, p(off), p(a), None, HOST) or lib.bvhgpu_hits_fetch_triangles(h, p(v), HOST)
        elif held in ("closest", "any", "box", "sphere"):
            rc = getattr(lib, "bvhgpu_hits_fetch_" + held)(h, p(v), p(a), HOST)
        elif held == "allhits":
            rc = lib.bvhgpu_hits_fetch_allhits(h, p(off), p(a), p(v), HOST)
        elif held in ("within", "within_count"):
            rc = lib.bvhgpu_hits_fetch_within(h, p(off), p(a), p(v), HOST)
        elif held == "region":
            rc = lib.bvhgpu_hits_fetch_region(h, p(off), p(a), None, HOST)
        elif held == "inst_region":
            rc = lib.bvhgpu_hits_fetch_instances_region(h, p(off), p(a), p(b), None, HOST)
        elif held == "inst_region_only":
            rc = lib.bvhgpu_hits_fetch_instances_region(h, p(off), p(a), None, None, HOST)
        elif held == "inst_allhits":
            rc = lib.bvhgpu_hits_fetch_instances_allhits(h, p(off), p(a), p(b), p(v), HOST)
        elif held == "inst_within":
            rc = lib.bvhgpu_hits_fetch_instances_within(h, p(off), p(a), p(b), p(v), HOST)
        else:   # inst_within_count: offsets alone
            rc = lib.bvhgpu_hits_fetch_instances_within(h, p(off), None, None, None, HOST)
        assert rc == OK, (held, self.error())
        return off.tobytes() + a.tobytes() + b.tobytes() + v.tobytes()


@pytest.fixture(scope="module")
def scene():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    s = Scene(bvh_amd)
    yield s
    s.close()


def test_the_table_is_complete():
    assert all(len(row.split()) == len(ACCESSORS) for _, row in TABLE.values())
    assert all(k in TABLE and a in ACCESSORS for k, a in list(OPTION) + list(PINNED))
    assert {(k, a) for k, (_, row) in TABLE.items() for a, cell in zip(ACCESSORS, row.split()) if cell == "o"} == set(OPTION)


def test_every_accessor_on_every_kind_of_result(scene):
    """the batches in TABLE's order into one result object; after each, the fourteen accessors"""
    for held, (reader, row) in TABLE.items():
        total = scene.run(held)
        if held not in ("closest", "any", "box", "sphere"):   # (a per-ray result has no total)
            assert total > 0, held
        before = scene.own(held, total)
        scene.reset()
        for accessor, cell in zip(ACCESSORS, row.split()):
            rc = scene.call(accessor)
            msg = scene.error()
            print(f"{held:18s} {accessor:24s} status {rc}  {msg!r}" if rc != OK else f"{held:18s} {accessor:24s} status {rc}")
            assert rc == (OK if cell == "K" else INVALID_ARG), (held, accessor, rc, msg)
            if cell == "K":
                scene.reset()
                continue
            assert scene.untouched(), (held, accessor)
            if cell == "n":   # the reader's name, not a longer accessor name that begins with it
                assert re.search(re.escape(reader) + r"(?![_a-z])", msg), (held, accessor, msg)
            if cell == "o":
                assert OPTION[held, accessor] in msg, (held, accessor, msg)
            if (held, accessor) in PINNED:
                assert PINNED[held, accessor] in msg, (held, accessor, msg)
        assert scene.own(held, total) == before, held


def test_outputs_a_batch_did_not_request_are_refused_by_its_own_accessor(scene):
    """T_SLICE, CLASSIFY, INSTANCES_ONLY and COUNT_ONLY: the kind's own accessor, asked for what the batch's flags left out"""
    lib, p, h = scene.lib, scene.ptr, scene.h
    so, si, ss, sv = p(scene.so), p(scene.si), p(scene.ss), p(scene.sv)
    cases = [
        ("csr", lambda: lib.bvhgpu_hits_fetch(h, so, ss, sv, HOST), "traverse was run without BVHGPU_TRAVERSE_T_SLICE"),
        ("region", lambda: lib.bvhgpu_hits_fetch_region(h, so, ss, sv, HOST), "without BVHGPU_REGION_CLASSIFY"),
        ("inst_region", lambda: lib.bvhgpu_hits_fetch_instances_region(h, so, si, ss, sv, HOST), "without BVHGPU_REGION_CLASSIFY"),
        ("inst_region_only", lambda: lib.bvhgpu_hits_fetch_instances_region(h, so, None, ss, None, HOST), "BVHGPU_REGION_INSTANCES_ONLY"),
        ("inst_allhits", lambda: lib.bvhgpu_hits_fetch_instances_allhits(h, so, si, ss, sv, 9), "mem must be"),
        ("inst_within_count", lambda: lib.bvhgpu_hits_fetch_instances_within(h, so, None, ss, None, HOST), "COUNT_ONLY"),
    ]
    for held, call, text in cases:
        total = scene.run(held)
        before = scene.own(held, total)
        scene.reset()
        assert call() == INVALID_ARG and text in scene.error(), (held, scene.error())
        assert scene.untouched(), held
        assert scene.own(held, total) == before, held

"""AABB / point / ball queries on the CPU: the checker (tests/query_ref.py) against the reference's own known answers
(tests/golden/query_known_answers.json, transcribed by hand) and its lockstep walk against a scalar per-query walk."""
import json
import os

import numpy as np
import pytest

from bvh_amd import testbase as tb
from oracle import orc

import query_ref as qr

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "query_known_answers.json")))
KINDS = {"aabb": qr.AABB, "point": qr.POINT, "ball": qr.BALL}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_checker_reproduces_traverse_some_built_bh(dtype):
    g = GOLD["aligned_boxes"]
    boxes = tb.generate_aligned_boxes_aabbs().astype(dtype)
    ids = g["ids"]
    for case in g["queries"]:
        off, idx, _ = qr.reference_lists(boxes, KINDS[case["kind"]], [case["query"]])
        got = sorted(ids[i] for i in idx.tolist())
        assert got == sorted(case["hit_ids"]), case


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_checker_reproduces_the_doc_tests(dtype):
    for case in GOLD["doc_tests"]:
        box = np.asarray([case["box"]], dtype=dtype)
        off, idx, _ = qr.reference_lists(box, KINDS[case["kind"]], [case["query"]])
        assert (idx.tolist() == [0]) == case["hit"], case


def _random_queries(rng, kind, n, lo, hi, dtype):
    c = rng.uniform(lo, hi, size=(n, 3))
    if kind == qr.POINT:
        return c.astype(dtype)
    e = rng.uniform(0.0, (hi - lo) * 0.2, size=(n, 3))
    if kind == qr.AABB:
        return np.concatenate([c - e, c + e], axis=1).astype(dtype)
    return np.concatenate([c, e[:, :1]], axis=1).astype(dtype)


def _edge_rows(kind, dtype):
    nan, inf = np.nan, np.inf
    if kind == qr.AABB:
        rows = [[nan, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, nan], [5, 5, 5, -5, -5, -5], [-inf, -inf, -inf, inf, inf, inf],
                [0.5, 0, 0, 0.5, 0, 0], [-0.0, -0.0, -0.0, 0.0, 0.0, 0.0]]
    elif kind == qr.POINT:
        rows = [[nan, 0, 0], [0, nan, 0], [0.5, 0.5, 0.5], [-0.0, 0.0, -0.0], [inf, 0, 0]]
    else:
        rows = [[0, 0, 0, nan], [nan, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, -2], [0, 0, 0, 1e30], [0.5, 0, 0, 0.0], [0, 0, 0, inf]]
    return np.asarray(rows, dtype=dtype)


def _no_winner_scene(dtype, n=40, seed=5):
    """boxes so far apart that surface areas overflow: SAH costs are NaN, splits have no winner and their child boxes stay
    Aabb::empty() (bvh_node.rs:225-230)"""
    rng = np.random.default_rng(seed)
    big = dtype(1e19 if dtype == np.float32 else 1e154)
    lo = (rng.uniform(-1, 1, size=(n, 3)) * big).astype(dtype)
    return np.concatenate([lo, lo + big * dtype(0.01)], axis=1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", [qr.AABB, qr.POINT, qr.BALL])
def test_lockstep_walk_equals_scalar_walk(dtype, kind):
    rng = np.random.default_rng(7 + kind)
    scenes = [tb.create_n_cubes(3)[1].astype(dtype), tb.generate_aligned_boxes_aabbs().astype(dtype),
              np.zeros((0, 6), dtype=dtype), tb.generate_aligned_boxes_aabbs()[:1].astype(dtype), _no_winner_scene(dtype),
              np.repeat(np.asarray([[0, 0, 0, 1, 1, 1]], dtype=dtype), 5, axis=0)]
    for boxes in scenes:
        lo, hi = (float(boxes[:, :3].min()), float(boxes[:, 3:].max())) if len(boxes) else (0.0, 1.0)
        lo, hi = max(lo, -1e6), min(hi, 1e6)
        q = np.concatenate([_random_queries(rng, kind, 40, lo, hi, dtype), _edge_rows(kind, dtype)])
        off, idx, flat = qr.reference_lists(boxes, kind, q)
        for i in range(len(q)):
            assert idx[off[i]:off[i + 1]].tolist() == qr.walk_one(flat, boxes, kind, q[i]), (i, q[i])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_empty_bounds_tree_differs_from_brute_force(dtype):
    """why the checker walks: on a tree with empty child bounds a finite box query reaches no leaf, a NaN query reaches all"""
    boxes = _no_winner_scene(dtype)
    tree = orc.build(boxes)
    flat = orc.flatten(tree.nodes)
    nav = flat[flat["entry"] != qr.NONE]
    empty = np.isposinf(nav["min"]).all(axis=1)
    assert empty.any(), "expected empty navigator boxes"
    whole = np.asarray([[-np.inf] * 3 + [np.inf] * 3], dtype=dtype)
    lo, hi = boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)
    q = np.concatenate([np.concatenate([lo, hi])[None, :], [[np.nan] * 6], whole]).astype(dtype)
    off, idx = qr.walk(flat, boxes, qr.AABB, q)
    assert len(idx[off[0]:off[1]]) < len(boxes)          # a box around the scene: brute force would list every shape
    assert sorted(idx[off[1]:off[2]].tolist()) == list(range(len(boxes)))   # all-NaN box: every comparison is false, every entry passes
    assert sorted(idx[off[2]:off[3]].tolist()) == list(range(len(boxes)))   # (-inf, +inf) touches the empty boxes too

"""The world-query limit cases (tests/query_limit_cases.py) without a GPU: the launch caps read from the sources
(voxelengine_amd/csrc, include/vxrt.h), every case past the cap it targets, a copy of the sources with any one cap raised
64-fold leaving some case short of its path (so raising a cap fails here instead of quietly emptying
tests/test_gpu_query_limits.py), and the closed-form references of the GPU cases held against the restatements
(tests/ref_nav.py, tests/ref_islands.py) at small sizes."""
import os
import re

import numpy as np
import pytest

from tests import query_limit_cases as Q
from tests import ref_islands, ref_nav


def _short(caps):
    return [(case.name, what, value, bound) for case in Q.LAUNCH_CASES for what, value, bound in case.reach(caps)
            if not value > bound]


def test_caps_are_read_from_the_sources():
    c = Q.read_caps()
    assert c["edit_max_ops"] == c["edit_max_ops_h"]
    assert all(v > 0 for v in c.values())


@pytest.mark.parametrize("case", Q.LAUNCH_CASES, ids=[c.name for c in Q.LAUNCH_CASES])
def test_case_exceeds_the_cap_it_targets(case):
    caps = Q.read_caps()
    for what, value, bound in case.reach(caps):
        assert value > bound, (case.name, what, value, bound)


@pytest.mark.parametrize("name", [n for n in Q.CAP_SOURCES if n != "edit_max_ops_h"])
def test_a_raised_cap_leaves_a_case_short(tmp_path, name):
    """each cap multiplied by 64 in a copy of its source: some case no longer exceeds it"""
    for path, _ in Q.CAP_SOURCES.values():
        dst = tmp_path / path
        dst.parent.mkdir(parents=True, exist_ok=True)
        with open(os.path.join(Q.ROOT, path)) as f:
            dst.write_text(f.read())
    path, rx = Q.CAP_SOURCES[name]
    text = (tmp_path / path).read_text()
    m = re.search(rx, text)
    raised = m.group(0).replace(m.group(1), str(int(m.group(1)) * 64))
    (tmp_path / path).write_text(text.replace(m.group(0), raised))
    caps = Q.read_caps(str(tmp_path))
    assert caps[name] == 64 * Q.read_caps()[name]
    assert _short(caps), name
    assert not _short(Q.read_caps())


def _nav_both(world, origin, dims, agent, goals):
    a = ref_nav.nav_field(world, origin, dims, agent, goals)
    if ref_nav.have_scipy():
        b = ref_nav.nav_field_scipy(world, origin, dims, agent, goals)
        assert all(np.array_equal(a[k], b[k]) for k in ("walkable", "dist", "next")) and a["summary"] == b["summary"]
    return a


@pytest.mark.parametrize("X,Z", [(16, 10), (9, 7), (12, 1), (5, 2), (33, 12)])
def test_snake_closed_form_equals_the_restatements(X, Z):
    snake = ref_nav.snake_world(X, Z)
    vox = np.zeros((X, 16, Z), bool)
    vox[:, :snake.shape[1]] = snake
    for agent in [(1, 2, 1, 3), (1, 3, 0, 0), (1, 1, 3, 3)]:
        want = _nav_both(vox, (0, 0, 0), snake.shape, agent, [(0, 1, 0)])
        dist, nxt, path = Q.snake_field(X, Z, snake.shape[1], agent)
        assert np.array_equal(want["dist"], dist) and np.array_equal(want["next"], nxt), agent
        assert want["summary"][3:] == (len(path), len(path) - 1, len(path))
    assert len(Q.snake_path(512, 512)) == 256 * 512 + 256


@pytest.mark.parametrize("dims,origin", [((7, 6, 5), (0, 0, 0)), ((9, 4, 33), (-3, -2, 5)), ((1, 8, 8), (2, 0, 1)),
                                         ((40, 3, 2), (1, 1, 1))])
def test_checkerboard_closed_form_equals_the_restatements(dims, origin):
    vox = Q.checkerboard(dims, origin)
    for anchors in (0, ref_islands.FACES, ref_islands.FLOOR | ref_islands.X_LO, ref_islands.Y_HI | ref_islands.Z_LO):
        want = ref_islands.find_islands(vox, origin, anchors)
        if ref_islands.have_scipy():
            s = ref_islands.find_islands_scipy(vox, origin, anchors)
            assert s["summary"] == want["summary"] and np.array_equal(s["table"], want["table"])
        summary, floating, ids, lo = Q.checker_islands(dims, origin, anchors)
        rows = want["table"]
        assert summary == want["summary"] and np.array_equal(floating, want["floating"]), anchors
        assert np.array_equal(rows[:, 0], ids) and (rows[:, 1] == 1).all()
        assert np.array_equal(rows[:, 2:5], lo) and np.array_equal(rows[:, 5:8], lo + 1)


@pytest.mark.parametrize("seed", range(4))
def test_vectorised_decoding_equals_decode_paths(seed):
    rng = np.random.default_rng(seed)
    vox = rng.random((40, 24, 40)) < 0.08
    vox[:, 0, :] = True
    o, d, agent = (3, -1, 2), (36, 16, 37), [(1, 2, 1, 3), (2, 3, 0, 1), (1, 1, 2, 8), (3, 2, 1, 2)][seed]
    probe = ref_nav.nav_field(vox, o, d, agent, [])
    nodes = np.argwhere(probe["walkable"]) + o
    goals = [tuple(nodes[i]) for i in rng.choice(len(nodes), 3, replace=False)]
    nxt = ref_nav.nav_field(vox, o, d, agent, goals)["next"].copy()
    # codes no field writes there: one that leaves B and one that names no move
    edge = np.argwhere(nxt[0] != ref_nav.NONE)[:3]
    nxt[0, edge[:, 0], edge[:, 1]] = 1 + (1 + agent[2] + agent[3])          # -x out of B
    nxt[5, 5, 5] = 200
    starts = np.concatenate([nodes[rng.integers(0, len(nodes), 400)],
                             np.stack([rng.integers(o[k] - 3, o[k] + d[k] + 3, 200) for k in range(3)], 1)])
    seen = set()
    for max_steps in (0, 1, 5, 60):
        c, l, s = ref_nav.decode_paths(nxt, o, agent, starts, max_steps)
        seen |= set(s.tolist())
        vc, vl, vs = Q.decode_paths_np(nxt, o, agent, starts, max_steps)
        assert np.array_equal(c, vc) and np.array_equal(l, vl) and np.array_equal(s, vs), max_steps
        _, nl, ns = Q.decode_paths_np(nxt, o, agent, starts, max_steps, cells=False)
        assert np.array_equal(nl, vl) and np.array_equal(ns, vs)
    assert seen == {ref_nav.AT_GOAL, ref_nav.NO_PATH, ref_nav.TRUNCATED, ref_nav.OUTSIDE}

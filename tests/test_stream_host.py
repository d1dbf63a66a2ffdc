"""CPU checks of the chunk-streaming policy (include/vxrt.h, vxrt_stream_focus): the two restatements of
tests/ref_stream.py on hand-derived cases and against each other on random focus sequences, and the library's policy
(csrc/vxrt_stream.hpp) compiled for the host (tests/tools/stream_check.cpp) against them -- every call's status, the
eight stats, every chunk's base slot and, after each sequence, which file brick every pool brick holds."""
import numpy as np
import pytest

from tests import ref_stream as R
from tests.helpers import build_harness, run_harness_files

F32 = np.float32
INF = float("inf")
NAN = float("nan")
RC = {R.OK: 0, R.INVALID: 1, R.READ_FAILED: 2}


def tables(cdims, bricks, factor=8, seed=0):
    """a chunk table with bricks[ch] occupied cells in chunk ch (at random cells of its tile)"""
    ncells = int(np.prod(cdims))
    occ = np.zeros(ncells, bool)
    rng = np.random.default_rng(seed)
    for ch, n in enumerate(bricks):
        occ[ch * 512 + rng.choice(512, int(n), replace=False)] = True
    bits = np.packbits(occ, bitorder="little").view("<u4").astype(np.uint32)
    return R.Tables(factor, cdims, bits)


def both(t, capacity):
    return R.StreamModelA(t, capacity), R.StreamModelB(t, capacity)


def call(models, focus, radius, unreadable=()):
    """one call on both models, asserted equal; returns model A's result"""
    a, b = (m.focus(focus, radius, unreadable) for m in models)
    assert a["rc"] == b["rc"] and a["stats"] == b["stats"]
    assert np.array_equal(a["base"], b["base"]) and np.array_equal(models[0].src, models[1].src)
    return a


def stats(res):
    return dict(zip(R.STAT_FIELDS, res["stats"]))


# ---- hand-derived cases (factor 8: a chunk is 64 voxels on a side) ----------------------------------------------------
def test_a_focus_at_exactly_the_radius_from_a_face():
    t = tables((24, 8, 8), [1, 1, 1])            # chunks along x: [0, 64], [64, 128], [128, 192]
    m = both(t, 3)
    # (32, 32, 20): gap 32 to chunk 1's face x = 64, 96 to chunk 2 (a box with x and z swapped would be 44 away)
    r = call(m, (32.0, 32.0, 20.0), float(np.nextafter(F32(32.0), F32(0.0))))
    assert list(r["flags"]) == [1, 0, 0]
    r = call(m, (32.0, 32.0, 20.0), 32.0)        # d^2 = 1024 <= r^2 = 1024
    assert list(r["flags"]) == [1, 1, 0] and stats(r)["chunks_loaded"] == 1 and stats(r)["bytes_read"] == 64
    r = call(m, (32.0, 32.0, 20.0), 96.0)
    assert list(r["flags"]) == [1, 1, 1] and stats(r)["chunks_loaded"] == 1


def test_a_focus_at_exactly_the_radius_from_an_edge():
    t = tables((16, 8, 16), [2, 1, 1, 3])       # 2 x 1 x 2 chunks; chunk 0's nearest point to the focus is on an edge
    m = both(t, 7)
    r = call(m, (-3.0, 32.0, -4.0), float(np.nextafter(F32(5.0), F32(0.0))))   # d^2 = 9 + 16 = 25
    assert r["stats"][2] == 0 and list(r["flags"]) == [0, 0, 0, 0]
    r = call(m, (-3.0, 32.0, -4.0), 5.0)
    assert list(r["flags"]) == [1, 0, 0, 0] and r["stats"][3] == 2
    # chunk 1 (tx 1, tz 0) is 67 away along x and 4 along z; chunk 2 (tx 0, tz 1) 3 along x and 68 along z
    r = call(m, (-3.0, 32.0, -4.0), float(np.sqrt(67 * 67 + 16)) + 0.001)
    assert list(r["flags"]) == [1, 1, 0, 0]
    assert float(F32(3 * 3) + F32(68 * 68)) == 4633.0 and float(F32(67 * 67) + F32(16)) == 4505.0


def test_ties_go_to_the_lower_chunk_index():
    t = tables((24, 8, 8), [1, 1, 1])
    m = both(t, 2)
    r = call(m, (96.0, 10.0, 10.0), 32.0)       # chunk 1 holds the focus; 0 and 2 both 32 away, room for one of them
    assert list(r["flags"]) == [1, 1, 0] and stats(r)["chunks_missing"] == 1 and list(r["base"]) == [1, 0, -1]


def test_radius_zero_inside_a_chunk_and_on_a_shared_face():
    t = tables((24, 8, 8), [4, 5, 6])
    m = both(t, 15)
    r = call(m, (100.0, 1.0, 63.5), 0.0)
    assert list(r["flags"]) == [0, 1, 0] and r["stats"][3] == 5
    r = call(m, (128.0, 64.0, 0.0), 0.0)        # a corner of chunks 1 and 2: both boxes are closed
    assert list(r["flags"]) == [0, 1, 1] and stats(r)["chunks_loaded"] == 1
    r = call(m, (1e30, -1e30, 1e30), INF)       # +inf takes every chunk, even at an infinite d^2
    assert list(r["flags"]) == [1, 1, 1] and r["stats"][3] == 15


def test_a_focus_outside_the_world():
    t = tables((16, 8, 8), [3, 3])
    m = both(t, 6)
    r = call(m, (-30.0, 100.0, 32.0), 47.0)     # d^2: chunk 0 900 + 1296 = 2196, chunk 1 8836 + 1296 = 10132
    assert list(r["flags"]) == [1, 0]
    r = call(m, (-30.0, 100.0, 32.0), 100.0)
    assert list(r["flags"]) == [1, 0] and stats(r)["chunks_loaded"] == 0
    r = call(m, (-30.0, 100.0, 32.0), 101.0)
    assert list(r["flags"]) == [1, 1] and list(r["base"]) == [0, 3]


def test_a_chunk_larger_than_the_whole_pool_evicts_what_is_outside_and_is_missing():
    t = tables((24, 8, 8), [2, 10, 1])
    m = both(t, 5)
    call(m, (32.0, 32.0, 32.0), 0.0)
    r = call(m, (160.0, 32.0, 32.0), 0.0)
    assert list(r["base"]) == [0, -1, 2]
    r = call(m, (96.0, 32.0, 32.0), 0.0)        # chunk 1 can never fit, and both others are 32 away: they go first
    assert stats(r) == dict(chunks_total=3, chunks_occupied=3, chunks_resident=0, bricks_resident=0, chunks_loaded=0,
                            chunks_evicted=2, chunks_missing=1, bytes_read=0)
    assert list(m[0].free) == [[0, 5]]


def test_only_merging_the_free_ranges_makes_room():
    t = tables((32, 8, 8), [2, 2, 2, 4])        # chunk centres at x = 32, 96, 160, 224
    m = both(t, 6)
    r = call(m, (96.0, 32.0, 32.0), 32.0)       # order 1, 0, 2: bases 0, 2, 4 -- the pool is full
    assert list(r["base"]) == [2, 0, 4, -1]
    # chunk 3 needs 4: chunk 0 (farthest) goes, [2, 4) alone is too short; chunk 1 goes, [0, 2) + [2, 4) is one range
    r = call(m, (224.0, 32.0, 32.0), 0.0)
    assert list(r["base"]) == [-1, -1, 4, 0] and stats(r)["chunks_evicted"] == 2
    assert list(m[1].src) == [6, 6 + 1, 6 + 2, 6 + 3, 4, 5]   # the file slots of chunk 3, then those of chunk 2


def test_evicting_everything_outside_the_radius_still_does_not_make_room():
    t = tables((24, 8, 8), [3, 4, 2])
    m = both(t, 6)
    call(m, (32.0, 32.0, 32.0), 0.0)
    r = call(m, (160.0, 32.0, 32.0), 0.0)
    assert list(r["base"]) == [0, -1, 3]
    r = call(m, (64.0, 32.0, 32.0), 0.0)        # chunks 0 and 1 in reach; 0 stays, 2 goes, 1 still needs 4 of 3
    assert stats(r)["chunks_evicted"] == 1 and stats(r)["chunks_missing"] == 1 and list(r["flags"]) == [1, 0, 0]
    assert list(m[0].free) == [[3, 3]]


def test_an_empty_world():
    t = tables((16, 16, 8), [0, 0, 0, 0])
    m = both(t, 1)
    for focus, radius in (((0.0, 0.0, 0.0), INF), ((64.0, 64.0, 32.0), 0.0)):
        assert call(m, focus, radius)["stats"] == (4, 0, 0, 0, 0, 0, 0, 0)


def test_a_refused_focus_changes_nothing():
    t = tables((24, 8, 8), [1, 2, 3])
    m = both(t, 6)
    call(m, (32.0, 32.0, 32.0), 40.0)
    before = m[0].base.copy()
    for focus, radius in (((NAN, 0.0, 0.0), 10.0), ((0.0, INF, 0.0), 10.0), ((0.0, 0.0, -INF), INF), ((0.0, 0.0, 0.0), -1.0),
                          ((0.0, 0.0, 0.0), NAN), ((0.0, 0.0, 0.0), -INF)):
        r = call(m, focus, radius)
        assert r["rc"] == R.INVALID and np.array_equal(r["base"], before)
    assert call(m, (0.0, 0.0, 0.0), -0.0)["rc"] == R.OK


def test_a_failed_read_stops_the_call_and_keeps_what_was_done():
    t = tables((32, 8, 8), [2, 2, 2, 2])
    m = both(t, 4)
    call(m, (32.0, 32.0, 32.0), 32.0)           # chunks 0, 1
    r = call(m, (224.0, 32.0, 32.0), 64.0, unreadable={2})   # order 3, 2: chunk 3 evicts 0, chunk 2 evicts 1 and fails
    assert r["rc"] == R.READ_FAILED and r["stats"] is None and list(r["base"]) == [-1, -1, -1, 0]
    assert list(m[0].free) == [[2, 2]]
    r = call(m, (224.0, 32.0, 32.0), 64.0)
    assert list(r["base"]) == [-1, -1, 2, 0] and stats(r)["chunks_loaded"] == 1 and stats(r)["chunks_evicted"] == 0


# ---- random sequences: A against B, and the library's policy against A -----------------------------------------------
GRIDS = [(16, 8, 24), (24, 16, 8), (32, 8, 8), (16, 16, 16), (40, 8, 24), (8, 8, 8), (24, 8, 32)]


def random_tables(rng, k):
    cdims = GRIDS[k % len(GRIDS)]
    nch = int(np.prod(cdims)) // 512
    kind = rng.random(nch)
    bricks = np.where(kind < 0.25, 0, np.where(kind < 0.85, rng.integers(1, 9, nch), rng.integers(1, 513, nch)))
    return tables(cdims, bricks, factor=int(rng.choice([8, 16, 32])), seed=k)


def random_sequences(rng, t, nseq):
    """[(capacity, [(focus, radius, unreadable)])]: capacities from one brick to everything, foci in and around the world
    (some on chunk boundaries), radii from 0 to past the world (some exact distances, some +inf), a few failing reads"""
    total = max(t.nslots, 1)
    ext = np.array(t.cdims, np.float64) * t.factor
    e = 8.0 * t.factor
    occupied = np.flatnonzero(t.nbricks > 0)
    seqs = []
    for _ in range(nseq):
        u = rng.random()
        cap = int(total if u < 0.15 else (1 if u < 0.2 else rng.integers(1, total + 1)))
        calls = []
        for _ in range(int(rng.integers(1, 12))):
            if rng.random() < 0.3:
                focus = np.round(rng.uniform(-0.5, 1.5, 3) * ext / (e / 2)) * (e / 2)   # on chunk faces and centres
            else:
                focus = rng.uniform(-0.3, 1.3, 3) * ext
            focus = [float(F32(v)) for v in focus]
            v = rng.random()
            if v < 0.1:
                radius = 0.0
            elif v < 0.15:
                radius = INF
            elif v < 0.35 and occupied.size:
                radius = float(np.sqrt(np.float64(t.d2(focus)[rng.choice(occupied)])))   # at (about) a chunk's distance
            else:
                radius = float(rng.uniform(0, 0.8 * ext.max()))
            fails = set()
            if rng.random() < 0.08 and occupied.size:
                fails = set(int(c) for c in rng.choice(occupied, size=min(3, occupied.size), replace=False))
            calls.append((focus, radius, fails))
        seqs.append((cap, calls))
    return seqs


def run_models(t, seqs, cls):
    out = []
    for cap, calls in seqs:
        m = cls(t, cap)
        out.append(([m.focus(f, r, u) for f, r, u in calls], m.src.copy()))
    return out


@pytest.mark.parametrize("part", range(4))
def test_the_two_restatements_agree_on_random_sequences(part):
    rng = np.random.default_rng(100 + part)
    nseq = nfail = nmissing = nevicted = 0
    for k in range(part * 14, part * 14 + 14):
        t = random_tables(rng, k)
        seqs = random_sequences(rng, t, 40)
        a, b = run_models(t, seqs, R.StreamModelA), run_models(t, seqs, R.StreamModelB)
        for (ra, sa), (rb, sb) in zip(a, b):
            assert np.array_equal(sa, sb)
            for x, y in zip(ra, rb):
                assert x["rc"] == y["rc"] and x["stats"] == y["stats"] and np.array_equal(x["base"], y["base"])
                nfail += x["rc"] == R.READ_FAILED
                if x["stats"]:
                    nmissing += x["stats"][6] > 0
                    nevicted += x["stats"][5] > 0
        nseq += len(seqs)
    assert nseq >= 500 and nfail > 0 and nmissing > 20 and nevicted > 20


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "stream_check")


def run_check(harness, tmp_path, t, seqs):
    """the library's policy on `seqs`: per sequence ([(rc, stats, base)], src)"""
    ncells = int(np.prod(t.cdims))
    bits = np.packbits(t.occupied, bitorder="little").view("<u4")
    meta = np.zeros((ncells, 2), np.uint32)
    meta[:, 0] = R.EMPTY
    meta[t.occupied, 0] = np.arange(t.nslots)
    body = []
    for cap, calls in seqs:
        body.append(np.array([cap & 0xFFFFFFFF, cap >> 32, len(calls)], np.uint32))
        for focus, radius, fails in calls:
            body.append(np.array(list(focus) + [radius], F32).view(np.uint32))
            body.append(np.array([len(fails)] + sorted(fails), np.uint32))
    raw, _ = run_harness_files(harness, tmp_path, [t.factor, *t.cdims, t.nslots, len(seqs)], bits, meta, *body)
    words = raw.view(np.int64)
    out, at = [], 0
    for cap, calls in seqs:
        res = []
        for _ in calls:
            rc, st, base = int(words[at]), tuple(int(v) for v in words[at + 1:at + 9]), words[at + 9:at + 9 + t.nchunks]
            res.append((rc, st, base))
            at += 9 + t.nchunks
        out.append((res, words[at:at + cap]))
        at += cap
    assert at == words.size
    return out


def assert_check_equals_model(harness, tmp_path, t, seqs):
    got = run_check(harness, tmp_path, t, seqs)
    for (res, src), (want, wsrc) in zip(got, run_models(t, seqs, R.StreamModelA)):
        for j, ((rc, st, base), w) in enumerate(zip(res, want)):
            assert rc == RC[w["rc"]], j
            assert st == (w["stats"] or (0,) * 8), j
            assert np.array_equal(base, w["base"]), j
        assert np.array_equal(src, wsrc)


def test_the_library_policy_equals_the_model_on_the_hand_cases(harness, tmp_path):
    cases = [
        (tables((24, 8, 8), [1, 1, 1]), [(3, [((32.0, 32.0, 20.0), float(np.nextafter(F32(32.0), F32(0.0))), set()),
                                              ((32.0, 32.0, 20.0), 32.0, set())]),
                                         (2, [((96.0, 10.0, 10.0), 32.0, set())])]),
        (tables((16, 8, 16), [2, 1, 1, 3]), [(7, [((-3.0, 32.0, -4.0), v, set()) for v in (4.999999, 5.0, 67.2)])]),
        (tables((24, 8, 8), [2, 10, 1]), [(5, [((32.0, 32.0, 32.0), 0.0, set()), ((160.0, 32.0, 32.0), 0.0, set()),
                                               ((96.0, 32.0, 32.0), 0.0, set())])]),
        (tables((32, 8, 8), [2, 2, 2, 4]), [(6, [((96.0, 32.0, 32.0), 32.0, set()), ((224.0, 32.0, 32.0), 0.0, set())])]),
        (tables((24, 8, 8), [3, 4, 2]), [(6, [((32.0, 32.0, 32.0), 0.0, set()), ((160.0, 32.0, 32.0), 0.0, set()),
                                              ((64.0, 32.0, 32.0), 0.0, set())])]),
        (tables((32, 8, 8), [2, 2, 2, 2]), [(4, [((32.0, 32.0, 32.0), 32.0, set()), ((224.0, 32.0, 32.0), 64.0, {2}),
                                                 ((NAN, 0.0, 0.0), 1.0, set()), ((0.0, 0.0, 0.0), NAN, set()),
                                                 ((224.0, 32.0, 32.0), 64.0, set())])]),
        (tables((16, 16, 8), [0, 0, 0, 0]), [(1, [((0.0, 0.0, 0.0), INF, set())])]),
    ]
    for t, seqs in cases:
        assert_check_equals_model(harness, tmp_path, t, seqs)


@pytest.mark.parametrize("part", range(2))
def test_the_library_policy_equals_the_model_on_random_sequences(harness, tmp_path, part):
    rng = np.random.default_rng(200 + part)
    for k in range(part * 10, part * 10 + 10):
        t = random_tables(rng, k)
        assert_check_equals_model(harness, tmp_path, t, random_sequences(rng, t, 30))

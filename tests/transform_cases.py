"""Hand-derived cases of the stamp orientations (include/vxrt.h, vxrt_transform_stamp), source and expected words written
out.  Each case: the source dims and region words (padding bits set where the case says so), an orientation (axis, flip), and
the destination dims and words worked out by hand from q[k] = sd[axis[k]] - 1 - p[axis[k]] if flip bit k else p[axis[k]].

The quarter turns, from the header's "one turn about a takes axis a + 1 onto a + 2":
  about x   n = 1: q = (p0, sd2-1-p2, p1)   n = 2: q = (p0, sd1-1-p1, sd2-1-p2)   n = 3: q = (p0, p2, sd1-1-p1)
  about y   n = 1: q = (p2, p1, sd0-1-p0)   n = 2: q = (sd0-1-p0, p1, sd2-1-p2)   n = 3: q = (sd2-1-p2, p1, p0)
  about z   n = 1: q = (sd1-1-p1, p0, p2)   n = 2: q = (sd0-1-p0, sd1-1-p1, p2)   n = 3: q = (p1, sd0-1-p0, p2)
"""
import numpy as np

from tests import ref_transform as R

# (rotation axis, turns) -> (axis, flip), from the table above
TURNS = {
    (0, 1): ((0, 2, 1), 0b010), (0, 2): ((0, 1, 2), 0b110), (0, 3): ((0, 2, 1), 0b100),
    (1, 1): ((2, 1, 0), 0b100), (1, 2): ((0, 1, 2), 0b101), (1, 3): ((2, 1, 0), 0b001),
    (2, 1): ((1, 0, 2), 0b001), (2, 2): ((0, 1, 2), 0b011), (2, 3): ((1, 0, 2), 0b010),
}

# a stick with its voxel (0, 0, 0) set and its other voxel clear, under every quarter turn: (dims, words) afterwards
STICK_X = {"dims": (2, 1, 1), "words": [0b01], "turned": {
    (0, 1): ((2, 1, 1), [0b01]), (0, 2): ((2, 1, 1), [0b01]), (0, 3): ((2, 1, 1), [0b01]),
    (1, 1): ((1, 1, 2), [0, 1]), (1, 2): ((2, 1, 1), [0b10]), (1, 3): ((1, 1, 2), [1, 0]),
    (2, 1): ((1, 2, 1), [1, 0]), (2, 2): ((2, 1, 1), [0b10]), (2, 3): ((1, 2, 1), [0, 1]),
}}
STICK_Y = {"dims": (1, 2, 1), "words": [1, 0], "turned": {
    (0, 1): ((1, 1, 2), [1, 0]), (0, 2): ((1, 2, 1), [0, 1]), (0, 3): ((1, 1, 2), [0, 1]),
    (1, 1): ((1, 2, 1), [1, 0]), (1, 2): ((1, 2, 1), [1, 0]), (1, 3): ((1, 2, 1), [1, 0]),
    (2, 1): ((2, 1, 1), [0b10]), (2, 2): ((1, 2, 1), [0, 1]), (2, 3): ((2, 1, 1), [0b01]),
}}


def _grid(dims, voxels):
    g = np.zeros(dims, bool)
    for v in voxels:
        g[v] = True
    return g


# the L-tromino in a 2 x 2 x 1 box: rows y = 0 (x = 0, 1 set) and y = 1 (x = 0 set)
TROMINO = _grid((2, 2, 1), [(0, 0, 0), (1, 0, 0), (0, 1, 0)])
TROMINO_WORDS = [0b11, 0b01]
# It lies in a plane and has the mirror plane x = y, so the half turn about the diagonal (1, 1, 0) maps it onto itself: its
# 24 rotations are 12 different shapes, each met twice, and its mirror images are among them.
TROMINO_DISTINCT = 12
# A piece without any symmetry: a path of two steps along x, one along y and one along z.  A symmetry would have to map the
# path onto itself, and its ends differ (one ends a segment of two steps), so it fixes every segment's direction: the
# identity alone.  Its 24 rotations are pairwise different after cropping and its mirror images equal none of them.
CHIRAL = _grid((3, 2, 2), [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (2, 1, 1)])
CHIRAL_WORDS = [0b111, 0b100, 0b000, 0b100]  # rows (y, z) = (0, 0), (1, 0), (0, 1), (1, 1)


def written_out():
    """the cases with both sides written out: dicts of name, dims, words (source), o, want_dims, want_words"""
    cases = []
    for name, stick in (("stick x", STICK_X), ("stick y", STICK_Y)):
        for turn, (dd, words) in stick["turned"].items():
            cases.append(dict(name="%s turn %s" % (name, turn), dims=stick["dims"], words=stick["words"], o=TURNS[turn], want_dims=dd,
                              want_words=words))
    # the tromino a quarter turn about z: q = (1 - p1, p0, 0): (0,0,0) -> (1,0,0), (1,0,0) -> (1,1,0), (0,1,0) -> (0,0,0)
    cases.append(dict(name="tromino turn z", dims=(2, 2, 1), words=TROMINO_WORDS, o=TURNS[(2, 1)], want_dims=(2, 2, 1),
                      want_words=[0b11, 0b10]))
    # mirrored along x: q = (1 - p0, p1, 0): rows y = 0: both, y = 1: x = 1
    cases.append(dict(name="tromino mirror x", dims=(2, 2, 1), words=TROMINO_WORDS, o=((0, 1, 2), 0b001), want_dims=(2, 2, 1),
                      want_words=[0b11, 0b10]))
    # the chiral piece a quarter turn about y: q = (p2, p1, 2 - p0), dims (2, 2, 3): (0,0,0) -> (0,0,2), (1,0,0) -> (0,0,1),
    # (2,0,0) -> (0,0,0), (2,1,0) -> (0,1,0), (2,1,1) -> (1,1,0); rows (y, z) in order (0,0), (1,0), (0,1), (1,1), (0,2), (1,2)
    cases.append(dict(name="chiral turn y", dims=(3, 2, 2), words=CHIRAL_WORDS, o=TURNS[(1, 1)], want_dims=(2, 2, 3),
                      want_words=[0b01, 0b11, 0b01, 0b00, 0b01, 0b00]))
    # a row of 33 voxels, 0, 31 and 32 set, the 31 padding bits of its second word set as well
    row = [0x80000001, 0xFFFFFFFF]
    cases.append(dict(name="row33 identity", dims=(33, 1, 1), words=row, o=R.IDENTITY, want_dims=(33, 1, 1), want_words=[0x80000001, 1]))
    # mirrored along x: q0 = 32 - p0: voxels 32, 1 and 0
    cases.append(dict(name="row33 mirror x", dims=(33, 1, 1), words=row, o=((0, 1, 2), 0b001), want_dims=(33, 1, 1), want_words=[0b11, 1]))
    # a quarter turn about z: 33 rows of one voxel, q1 = p0
    cases.append(dict(name="row33 turn z", dims=(33, 1, 1), words=row, o=TURNS[(2, 1)], want_dims=(1, 33, 1),
                      want_words=[1] + [0] * 30 + [1, 1]))
    # three quarter turns about z: q1 = 32 - p0
    cases.append(dict(name="row33 turn z3", dims=(33, 1, 1), words=row, o=TURNS[(2, 3)], want_dims=(1, 33, 1),
                      want_words=[1, 1] + [0] * 30 + [1]))
    # one voxel at each corner of a 3 x 4 x 5 box (one word a row, word y + 4 z), a quarter turn about z: dims (4, 3, 5), one
    # word a row, q = (3 - p1, p0, p2): the voxel is bit 3 - p1 of word p0 + 3 p2
    for p in [(x, y, z) for x in (0, 2) for y in (0, 3) for z in (0, 4)]:
        src, dst = [0] * 20, [0] * 15
        src[p[1] + 4 * p[2]] = 1 << p[0]
        dst[p[0] + 3 * p[2]] = 1 << (3 - p[1])
        cases.append(dict(name="corner %s turn z" % (p,), dims=(3, 4, 5), words=src, o=TURNS[(2, 1)], want_dims=(4, 3, 5), want_words=dst))
    return cases


def check(case, dims, words):
    """the destination `dims` and `words` of a transform against a written-out case"""
    assert tuple(dims) == tuple(case["want_dims"]), case["name"]
    assert [int(w) for w in np.asarray(words).view(np.uint32)] == list(case["want_words"]), case["name"]


def source_grid(case):
    """the case's source as a bool grid (its padding bits dropped)"""
    return R.unpack(np.asarray(case["words"], np.uint32), case["dims"])[0]

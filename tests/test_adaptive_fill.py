"""The adaptive fill (mvpath_multi.h:79-115) on the CPU oracle: what tests/test_gpu_adaptive_fill.py relies on.

That module holds the device's fill to the oracle's fixed-point film bit for bit, on masks far denser than any
stock shape gives.  Two things about it can be checked without a device: that the bar notices a fill sample in the
wrong place of the pass's compressed array (a prefix or a total off by one moves the seed or the index of every
repeat of the range), and that the scene edits behind the dense cases still give the masks those cases assert.

The scene edits, the dense shapes and the oracle's count phase are defined here and imported by the GPU module.
"""
import os

import numpy as np

from conftest import SCENES

CBOX = os.path.join(SCENES, "cbox_grid.xml")

# views 0.8 apart looking through a 4 degree lens see disjoint patches of the room: no other view of the group
# sees a lane's hit point, which is what flags the lane (adapt_mask: at most one view valid)
DENSE_EDITS = (('<float name="cam_dist" value="0.4"/>', '<float name="cam_dist" value="0.8"/>'),
               ('<float name="fov" value="39.3077"/>', '<float name="fov" value="4"/>'))

DENSE_ALL = dict(gx=2, gy=1, reuse=2, adaptive=1, res=32, spp=16)          # 32768 lanes, 8 compaction tiles
DENSE_MANY_TILES = dict(DENSE_ALL, res=96)                                 # 294912 lanes, 72 tiles
DENSE_MULTICHUNK = dict(gx=2, gy=2, reuse=4, adaptive=3, res=24, spp=16)   # 36864 lanes, 9 tiles, n_adapt = 3


def edit_once(xml, old, new):
    assert xml.count(old) == 1, old
    return xml.replace(old, new)


def dense_xml():
    xml = open(CBOX).read()
    for old, new in DENSE_EDITS:
        xml = edit_once(xml, old, new)
    return xml


def bit_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def oracle_range_counts(oracle, sd, vd, p, ranges):
    """Count phase on the oracle: per lane range, its flagged lanes in every pass (the fill's output of these
    renders is of no use: each range is given prefix 0 and its own count as the total)."""
    counts = []
    try:
        for b, e in ranges:
            got = []
            oracle.set_exchange(lambda local, got=got: (got.append(local), (0, local))[1])
            oracle.render(sd, vd, p, lane_begin=b, lane_end=e, threads=16)
            counts.append(got)
    finally:
        oracle.set_exchange(None)
    return counts


def test_dense_edits_flag_most_lanes(oracle, amvpt_mod):
    """The three dense shapes of the GPU module: every lane flagged at G = 2 (one tile of compaction output is the
    identity), and at G = 4 more than half of them, with a fill wavefront of more than twice the pass."""
    xml = dense_xml()
    for kw in (DENSE_ALL, DENSE_MANY_TILES):
        s = amvpt_mod.load_string(xml, **kw)   # the descriptors live as long as the scene
        sd, vd, p = s.describe(0, 0, 0)
        lanes = oracle.plan(p)["lanes"]
        assert lanes == 2 * kw["res"] ** 2 * 16 and lanes % 4096 == 0
        _, _, st = oracle.render(sd, vd, p, threads=16)
        print("res %d: %d of %d lanes flagged, oracle %.2f s" % (kw["res"], st["adaptive_lanes"], lanes, st["seconds"]))
        assert st["adaptive_lanes"] == lanes
    s = amvpt_mod.load_string(xml, **DENSE_MULTICHUNK)
    sd, vd, p = s.describe(0, 0, 0)
    lanes = oracle.plan(p)["lanes"]
    assert lanes == 36864
    _, _, st = oracle.render(sd, vd, p, threads=16)
    flagged = st["adaptive_lanes"] // 3
    print("G = 4: %d of %d lanes flagged (%.3f)" % (flagged, lanes, flagged / lanes))
    assert st["adaptive_lanes"] == 3 * flagged and flagged > 0.5 * lanes
    assert 2 * lanes < st["adaptive_lanes"] <= 3 * lanes   # three fill chunks of at most a pass each


def test_fixed_film_notices_a_shifted_prefix_or_total(oracle, amvpt_mod):
    """The second of two lane ranges (cut inside a compaction tile, off the 16-lane groups) rendered into the
    fixed-point film: the same film twice with the right (prefix, total); another film with the prefix one too
    small (every repeat takes its neighbour's index) and with the total one too large (every repeat another seed)."""
    s = amvpt_mod.load_file(CBOX, res=24, spp=16, gx=4, gy=2, reuse=8, adaptive=3)
    sd, vd, p = s.describe(0, 0, 0)
    plan = oracle.plan(p)
    assert plan["passes"] == 1 and plan["lanes"] == 73728
    cut = 2 * 4096 + 7
    (below,), (local,) = oracle_range_counts(oracle, sd, vd, p, [(0, cut), (cut, plan["lanes"])])
    print("flagged lanes below and above lane %d: %d, %d" % (cut, below, local))
    assert below > 0 and local > 0

    def second_range(prefix, total):
        def fn(n):
            assert n == local
            return prefix, total
        oracle.set_exchange(fn)
        try:
            film, _, st = oracle.render(sd, vd, p, lane_begin=cut, lane_end=plan["lanes"], threads=16, fixed_film=True)
        finally:
            oracle.set_exchange(None)
        assert st["adaptive_lanes"] == 3 * local and st["range_drops"] == 0
        return film
    right = second_range(below, below + local)
    assert bit_equal(right, second_range(below, below + local)).all()
    for what, film in (("prefix - 1", second_range(below - 1, below + local)),
                       ("total + 1", second_range(below, below + local + 1))):
        differ = int((~bit_equal(right, film)).sum())
        print("%s: %d of %d floats differ" % (what, differ, right.size))
        assert differ > 0

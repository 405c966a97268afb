"""The shapes of tests/test_gpu_group_sizes.py on the CPU oracle alone: that they can fail for the right reason.

k_mv_primary, k_vis, k_prim_hit_req and k_splat_multi are compiled once per view-group size G (2..16, a run-time
instance for 17..256 views and one for 257..1024), and the instances of one G differ in where a view's state lives, in
the bits of the packed view masks they reach and in the LDS they take ("Every group-size
instance").  The GPU module renders one small frame per G and compares every per-lane, per-view record with the
oracle's.  Such a comparison is worth something only if the frame really has a record in every view slot, if the slot
of a record is tied to a view, and if a glossy frame really holds both kinds of wave.  This module asserts that on the
oracle's own output, and holds the shapes, the shared oracle frames (computed once per shape) and the host-side regime
checks that the GPU module imports.
"""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from conftest import SCENES

CBOX = os.path.join(SCENES, "cbox_grid.xml")
VEACH = os.path.join(SCENES, "veach_grid.xml")
MESH = os.path.join(SCENES, "cbox_mesh.xml")

# one group of G views as gx x gy tiles; 17 is the first run-time group
GRID = {2: (2, 1), 3: (3, 1), 4: (2, 2), 5: (5, 1), 6: (3, 2), 7: (7, 1), 8: (4, 2), 9: (3, 3), 10: (5, 2), 11: (11, 1),
        12: (4, 3), 13: (13, 1), 14: (7, 2), 15: (5, 3), 16: (4, 4), 17: (17, 1)}
COMPILE_TIME = list(range(2, 17))
MIS_VARIANT_G = (8, 9, 16)   # both sides of pdf_in_regs' bound, and view bit 15


def shape(G, **extra):
    """res 8, 16 spp in one pass, one group of G views: 1024 x G lanes, a quilt width that is a multiple of 4."""
    gx, gy = GRID[G]
    kw = dict(res=8, spp=16, gx=gx, gy=gy, reuse=G)
    kw.update(extra)
    return kw


# scenes with several groups per frame: (scene, defines, G, views)
TWO_GROUPS = {
    "cbox_7x2_g7": (CBOX, dict(res=8, spp=16, gx=7, gy=2, reuse=7), 7, 14),
    "veach_6x5_g15": (VEACH, dict(res=8, spp=16, gx=6, gy=5, reuse=15), 15, 30),
    "veach_4x4_g16": (VEACH, dict(res=8, spp=16, gx=4, gy=4, reuse=16), 16, 16),
    "veach_8x4_g16": (VEACH, dict(res=8, spp=16, gx=8, gy=4, reuse=16), 16, 32),
    "cbox_8x4_g16": (CBOX, dict(res=8, spp=16, gx=8, gy=4, reuse=16), 16, 32),
}
# ragged frames under an odd G: (scene, defines, G, lanes)
RAGGED = {
    "cbox_7x1_res5": (CBOX, dict(res=5, spp=16, gx=7, gy=1, reuse=7), 7, 2800),
    "cbox_13x1_res5": (CBOX, dict(res=5, spp=16, gx=13, gy=1, reuse=13), 13, 5200),
    "mesh_7x1_res8": (MESH, dict(res=8, spp=16, gx=7, gy=1, reuse=7), 7, 7168),
    "mesh_13x1_res8": (MESH, dict(res=8, spp=16, gx=13, gy=1, reuse=13), 13, 13312),
}
# run-time group sizes at their boundaries: (scene, defines, G, lane ranges or None for the whole frame)
RUNTIME = {
    "cbox_g17": (CBOX, shape(17), 17, None),
    "veach_g17": (VEACH, shape(17), 17, None),
    "cbox_g257": (CBOX, dict(res=2, spp=16, gx=257, gy=1, reuse=257), 257, None),
    # the largest legal group, 65536 lanes: the first 2048 and 2048 from the middle of the frame, starting 37 lanes
    # past a wave (and 5 samples into a pixel)
    "cbox_g1024": (CBOX, dict(res=2, spp=16, gx=32, gy=32, reuse=1024), 1024, ((0, 2048), (32805, 34853))),
}


class Frame:
    """One single-pass scene and the oracle's frames of it, computed once per (scene, defines, lane range) and never
    modified: .oracle() -> (float film, records of pass 0), .oracle_fixed() -> the fixed-point film."""
    _cache = {}

    def __init__(self, amvpt_mod, oracle, scene_file, defines, lanes=None):
        self.mod, self.O = amvpt_mod, oracle
        self.scene = amvpt_mod.load_file(scene_file, **defines)
        self.sd, self.vd, self.p = self.scene.describe(0, 0, 0)
        self.plan = oracle.plan(self.p)
        assert self.plan["passes"] == 1 and self.plan["spp_per_pass"] == 16
        self.G = self.plan["group"]
        self.lanes = (0, self.plan["lanes"]) if lanes is None else tuple(lanes)
        assert 0 <= self.lanes[0] < self.lanes[1] <= self.plan["lanes"]
        self.key = (os.path.basename(scene_file), tuple(sorted(defines.items())), self.lanes)

    def _get(self, fixed):
        k = self.key + (fixed,)
        if k not in Frame._cache:
            film, rec, _ = self.O.render(self.sd, self.vd, self.p, self.lanes[0], self.lanes[1], threads=16,
                                         record_pass=None if fixed else 0, fixed_film=fixed)
            film.setflags(write=False)
            if rec is not None:
                rec.setflags(write=False)
            Frame._cache[k] = (film, rec)
        return Frame._cache[k]

    def oracle(self):
        return self._get(False)

    def oracle_fixed(self):
        return self._get(True)[0]

    def primary_view(self):
        """View index of every lane of the range (sample_ray_idx, grid.cpp:269-297: the quilt tile of the lane's
        pixel, mirrored along a reversed axis; no crop here)."""
        pix = np.arange(self.lanes[0], self.lanes[1]) // 16
        return self.tile_view(pix % self.p.film_width, pix // self.p.film_width)

    def tile_view(self, x, y):
        """View index of the quilt tile that holds integer quilt position (x, y)."""
        p = self.p
        tx, ty = x // (p.film_width // p.grid_x), y // (p.film_height // p.grid_y)
        if p.reverse_x:
            tx = p.grid_x - 1 - tx
        if p.reverse_y:
            ty = p.grid_y - 1 - ty
        return ty * p.grid_x + tx

    def view_tile(self, view):
        """(x0, y0, width, height) of the quilt tile of `view`: tile_view's inverse."""
        p = self.p
        rx, ry = p.film_width // p.grid_x, p.film_height // p.grid_y
        ty, tx = view // p.grid_x, view % p.grid_x
        if p.reverse_x:
            tx = p.grid_x - 1 - tx
        if p.reverse_y:
            ty = p.grid_y - 1 - ty
        return tx * rx, ty * ry, rx, ry

    def slot_view(self):
        """(lanes, G): the view of group slot k of every lane (mvpath_multi.h:31-38: p_idx + k, wrapped inside the
        lane's own group of G consecutive views)."""
        p_idx = self.primary_view()[:, None]
        ids = p_idx + np.arange(self.G)[None, :]
        return np.where(ids < self.G * (p_idx // self.G + 1), ids, ids - self.G)


def valid_share(rec):
    """Share of lanes with a valid record, per view slot."""
    return (rec[:, :, 7] != 0).mean(axis=0)


def check_slots(frame, rec, min_share=0.5):
    """Every reprojected slot is valid on at least half of the lanes, and every valid record lies in the quilt tile of
    the view that the slot stands for -- equal records therefore tie the device to those slots and views."""
    share = valid_share(rec)
    k = int(np.argmin(share[1:])) + 1
    print("smallest valid share over slots: %.3f (slot %d of %d)" % (share[k], k, frame.G))
    assert share[1:].min() >= min_share, share
    valid = rec[:, :, 7] != 0
    x0, y0, rx, ry = frame.view_tile(frame.slot_view())
    x, y = rec[:, :, 0], rec[:, :, 1]
    # closed on the far side: the f32 sum of a view position just under the tile size and the tile's offset may round up
    inside = (x >= x0) & (x <= x0 + rx) & (y >= y0) & (y <= y0 + ry)
    assert inside[valid].all(), "%d valid records outside their slot's view tile" % (~inside)[valid].sum()
    return share


def glossy_shapes(scene_file):
    """Indices (the scene file's shape order, which the scene description keeps) of the shapes that carry a BSDF other
    than a plain `diffuse` one."""
    root = ET.parse(scene_file).getroot()
    named = {b.get("id"): b for b in root.findall("bsdf")}

    def plain(b):
        return b.get("type") == "diffuse"
    out = set()
    for i, s in enumerate(root.findall("shape")):
        bsdfs = list(s.iter("bsdf")) + [named[r.get("id")] for r in s.findall("ref") if r.get("id") in named]
        if any(not plain(b) for b in bsdfs):
            out.add(i)
    return out


def wave_tiles(hits, glossy):
    """Of the frame's 4-pixel wave tiles (64 consecutive lanes: 4 pixels of a quilt row x 16 samples; the quilt width
    is a multiple of 4, so no tile wraps), (tiles whose pixel-centre hits are all diffuse or misses, with the same true
    of every neighbouring pixel: the jittered samples stay inside the pixels; tiles with a glossy centre hit)."""
    H, W = hits.shape[:2]
    assert W % 4 == 0
    g = np.isin(hits[..., 0].astype(np.int64), sorted(glossy))
    near = np.zeros_like(g)
    pad = np.pad(g, 1)
    for dy in range(3):
        for dx in range(3):
            near |= pad[dy:dy + H, dx:dx + W]
    return int((~near.reshape(H, W // 4, 4).any(axis=2)).sum()), int(g.reshape(H, W // 4, 4).any(axis=2).sum())


def check_mixed_waves(frame):
    """A glossy frame holds waves for both launches of the generic k_mv_primary: the all-diffuse one (kDW) and the
    generic one."""
    hits = frame.O.primary_hits(frame.sd, frame.vd, frame.p)
    glossy = glossy_shapes(VEACH)
    assert glossy == {0, 1, 2, 3}   # the four rough-conductor plates
    diffuse_tiles, glossy_tiles = wave_tiles(hits, glossy)
    print("wave tiles: %d all diffuse, %d with a glossy hit, of %d" % (diffuse_tiles, glossy_tiles, hits.shape[0] * hits.shape[1] // 4))
    assert diffuse_tiles >= 1 and glossy_tiles >= 1
    return diffuse_tiles, glossy_tiles


def _check_frame(frame, G, min_share=0.5):
    assert frame.G == G
    film, rec = frame.oracle()
    assert rec.shape == (frame.lanes[1] - frame.lanes[0], G, 8)
    assert np.isfinite(film).all() and np.abs(film).max() > 0
    assert np.isfinite(frame.oracle_fixed()).all()
    return check_slots(frame, rec, min_share)


@pytest.mark.parametrize("G", list(GRID))
def test_cornell_shapes(amvpt_mod, oracle, G):
    _check_frame(Frame(amvpt_mod, oracle, CBOX, shape(G)), G)


@pytest.mark.parametrize("G", COMPILE_TIME + [17])
def test_veach_shapes(amvpt_mod, oracle, G):
    f = Frame(amvpt_mod, oracle, VEACH, shape(G))
    _check_frame(f, G)
    check_mixed_waves(f)


@pytest.mark.parametrize("G", MIS_VARIANT_G)
@pytest.mark.parametrize("mis", [dict(fast_mis="true"), dict(sa_mis="false")], ids=["fast_mis", "no_mis"])
def test_veach_mis_variants(amvpt_mod, oracle, G, mis):
    """The other two weightings are different frames: their records differ from the sa_mis frame's."""
    f = Frame(amvpt_mod, oracle, VEACH, shape(G, **mis))
    _check_frame(f, G)
    base = Frame(amvpt_mod, oracle, VEACH, shape(G)).oracle()[1]
    assert not np.array_equal(f.oracle()[1], base)


def test_veach_shape_order(amvpt_mod, oracle):
    """primary_hits' shape index is the scene file's shape order: hits on shape 8 lie on the floor (y = -3.5), on
    shape 9 on the back wall (z = -6), on the glossy shapes 0..3 on neither."""
    f = Frame(amvpt_mod, oracle, VEACH, shape(8, res=16))
    hits = oracle.primary_hits(f.sd, f.vd, f.p)
    ids = hits[..., 0].astype(int)
    assert (ids == 8).any() and (ids == 9).any() and np.isin(ids, [0, 1, 2, 3]).any()
    assert np.abs(hits[ids == 8][:, 5] + 3.5).max() < 1e-3 and np.abs(hits[ids == 9][:, 6] + 6.0).max() < 1e-3
    plates = hits[np.isin(ids, [0, 1, 2, 3])]
    assert (plates[:, 5] > -3.4).all() and (plates[:, 6] > -5.9).all()
    assert glossy_shapes(CBOX) == set() and glossy_shapes(MESH) != set()


@pytest.mark.parametrize("case", list(TWO_GROUPS))
def test_two_group_shapes(amvpt_mod, oracle, case):
    scene, defines, G, views = TWO_GROUPS[case]
    f = Frame(amvpt_mod, oracle, scene, defines)
    assert f.p.n_views == views
    _check_frame(f, G)
    if views > G:
        assert set(np.unique(f.primary_view() // G)) == set(range(views // G))
    if scene == VEACH:
        check_mixed_waves(f)


@pytest.mark.parametrize("case", list(RAGGED))
def test_ragged_shapes(amvpt_mod, oracle, case):
    scene, defines, G, lanes = RAGGED[case]
    f = Frame(amvpt_mod, oracle, scene, defines)
    assert f.plan["lanes"] == lanes
    if defines["res"] == 5:
        assert lanes % 128 != 0 and lanes % 64 != 0 and f.p.film_width % 4 != 0   # partial block and wave, no tiles
    _check_frame(f, G)


@pytest.mark.parametrize("case", list(RUNTIME))
def test_runtime_boundary_shapes(amvpt_mod, oracle, case):
    scene, defines, G, ranges = RUNTIME[case]
    for lanes in ranges or (None,):
        f = Frame(amvpt_mod, oracle, scene, defines, lanes)
        if lanes is not None:
            assert f.plan["lanes"] == 65536 and (lanes[0] % 64 == 0) == (lanes[0] == 0)
        _check_frame(f, G)
    if scene == VEACH:
        check_mixed_waves(f)


def _differs(a, b):
    return ~(((a == b) | (np.isnan(a) & np.isnan(b))).all(axis=(1, 2)))


def test_swapped_slots_change_the_records(amvpt_mod, oracle):
    """View slots 14 and 15 of the G = 16 frames swapped: a device that mixed up view bit 15's slot with its
    neighbour's could not produce the oracle's records."""
    for scene in (CBOX, VEACH):
        rec = Frame(amvpt_mod, oracle, scene, shape(16)).oracle()[1]
        swapped = rec.copy()
        swapped[:, [14, 15]] = rec[:, [15, 14]]
        share = _differs(rec, swapped).mean()
        print("%s: %.3f of the lanes differ" % (os.path.basename(scene), share))
        assert share > 0.9


def test_shifted_second_group_changes_the_records(amvpt_mod, oracle):
    """The two-group frame with the second group's view index taken one further (slot k showing view k + 1 of the
    group, the last slot wrapping to the first reprojected one): every record comparison of the second group's lanes
    would see it; the first group's lanes are untouched."""
    scene, defines, G, _ = TWO_GROUPS["cbox_7x2_g7"]
    f = Frame(amvpt_mod, oracle, scene, defines)
    rec = f.oracle()[1]
    second = f.primary_view() >= G
    assert 0.4 < second.mean() < 0.6
    shifted = rec.copy()
    shifted[second, 1:] = np.roll(rec[second, 1:], -1, axis=1)
    d = _differs(rec, shifted)
    print("second group: %.3f of its lanes differ" % d[second].mean())
    assert d[second].mean() > 0.9 and not d[~second].any()

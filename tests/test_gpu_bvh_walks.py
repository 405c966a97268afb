"""GPU parity of the BVH walk instances and tree shapes the stock scenes do not reach.

The bar is test_gpu_parity.py's: every per-lane, per-view record of pass 0 bit-identical to the oracle's and
the film within 1e-5 of its largest magnitude.  What changes from case to case is WHICH walk runs and which
memory it reads -- spheres or rectangles in a BVH read from device memory (the whole-record leaves of the
two-box walks, WALK_LANE / WALK_LANE_NS), rectangles in BVH leaves at all (more than kOuterMax = 8 of them),
two-box trees exactly at and one past the kStack2 = 16 stack bound, leaves of up to 15 primitives, a float16
node frame thousands of times wider than the geometry, and the LDS-staged tier on both sides of its 48 KiB
limit.  Every case asserts the evidence that it reached its tier (node counts, the two-box tree's size and
depth, kernel launch counters): a scene that slips into another tier fails instead of passing there.

Scenes are string edits of scenes/cbox_mesh.xml and scenes/cbox_grid.xml; meshes are OBJ files written at
test time (a sine heightfield, single triangles): scene_gen.py, shared with the CPU scene-image tests.
"""
import os

import numpy as np
import pytest

from conftest import SCENES
from scene_gen import (_add, _extra_rects, _grid_with_heightfield_xml, _heightfield_obj, _heightfield_room_xml,  # noqa: F401
                       _obj_shape, _triangle_obj, _xml)

pytestmark = pytest.mark.gpu

G8 = dict(res=16, spp=16, gx=4, gy=2, reuse=8)   # 32768 lanes, one group of 8 views
G1 = dict(res=16, spp=16, reuse=1)               # render_sample / sample_single
SIZES = pytest.mark.parametrize("kw", [G8, G1], ids=["g8", "path_g1"])


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module", autouse=True)
def _device_started(gpu_ready, amvpt_mod):
    """The process's one-time costs (importing torch, creating the HIP context, loading the library's code objects
    at its first launch: about 12 s) are paid here when this module is the first to use the device, so that
    `--durations` shows each case's own time."""
    torch = _torch()
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_mesh.xml"), res=4, spp=16)
    sd, vd, p = s.describe(0, 0, 0)
    film = torch.zeros((p.film_height, p.film_width, 4), dtype=torch.float32, device="cuda")
    amvpt_mod.DeviceScene(sd).render_ex(vd, p, film.data_ptr())
    torch.cuda.synchronize()


def _bit_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _render(amvpt_mod, dev, vd, p, plan, flags=0):
    """(film, records of pass 0) of one frame."""
    torch = _torch()
    film = torch.zeros((p.film_height, p.film_width, 4), dtype=torch.float32, device="cuda")
    rec = torch.zeros((plan["lanes"], plan["group"], 8), dtype=torch.float32, device="cuda")
    dev.render_ex(vd, p, film.data_ptr(), flags=flags, records_ptr=rec.data_ptr())
    torch.cuda.synchronize()
    return film.cpu().numpy(), rec.cpu().numpy()


def _launches(amvpt_mod, dev, vd, p, flags=0):
    torch = _torch()
    film = torch.zeros((p.film_height, p.film_width, 4), dtype=torch.float32, device="cuda")
    cnt = amvpt_mod.Counters()
    dev.render_ex(vd, p, film.data_ptr(), counters=cnt, flags=flags)
    torch.cuda.synchronize()
    return cnt.as_dict()["kernel_launches"]


def _oracle(oracle, sd, vd, p, bvh=False):
    """The oracle's (film, records).  bvh: its BVH mode, for meshes too large to brute-force in seconds
    (test_oracle_bvh_mode_matches_brute_force pins that mode to the brute-force scan)."""
    if not bvh:
        return oracle.render(sd, vd, p, threads=16, record_pass=0)[:2]
    oracle.set_bvh(True)
    try:
        return oracle.render(sd, vd, p, threads=16, record_pass=0)[:2]
    finally:
        oracle.set_bvh(False)


def _assert_parity(gfilm, grec, ofilm, orec):
    # the comparison is of something: most lanes carry light (record floats 2..4 are the RGB value)
    assert (orec[..., 2:5] != 0).any(axis=(1, 2)).mean() > 0.5
    eq = _bit_equal(grec, orec).all(axis=(1, 2))
    if not eq.all():
        for lane in np.argwhere(~eq)[:5, 0]:
            print("lane", lane, "\ngpu", grec[lane], "\noracle", orec[lane])
    assert eq.all(), "lane records: %.6f bit-identical" % eq.mean()
    err = np.abs(gfilm - ofilm).max() / np.abs(ofilm).max()
    assert err < 1e-5, "film max relative difference %.3e" % err


FLAG_SETS = ("OPT_NO_BINNING", "OPT_THREADED_BVH", "OPT_NO_BINNING|OPT_THREADED_BVH")


def _check(amvpt_mod, oracle, scene, dev=None, flag_sets=(), oracle_bvh=False):
    """The oracle bar and the film bar on `scene`; flag_sets: records equal to the default's under each.
    Returns the default records, the launch counters and the device scene."""
    sd, vd, p = scene.describe(0, 0, 0)
    plan = oracle.plan(p)
    dev = dev or amvpt_mod.DeviceScene(sd)
    gfilm, grec = _render(amvpt_mod, dev, vd, p, plan)
    ofilm, orec = _oracle(oracle, sd, vd, p, oracle_bvh)
    _assert_parity(gfilm, grec, ofilm, orec)
    for names in flag_sets:
        flags = 0
        for n in names.split("|"):
            flags |= getattr(amvpt_mod, n)
        _, r = _render(amvpt_mod, dev, vd, p, plan, flags)
        eq = _bit_equal(grec, r).all(axis=(1, 2))
        assert eq.all(), "%s: %d of %d lanes differ from the default walk" % (names, (~eq).sum(), eq.size)
    return grec, _launches(amvpt_mod, dev, vd, p), dev


def _device_bvh(amvpt_mod, scene):
    dev = amvpt_mod.DeviceScene(scene.describe(0, 0, 0)[0])
    (n_nodes, n_prims), (n2, depth) = dev.stats(), dev.bvh2()
    print("BVH: %d nodes, %d primitives; two-box: %d nodes, depth %d" % (n_nodes, n_prims, n2, depth))
    return dev, n_nodes, n_prims, n2, depth


# ---- spheres in a BVH read from device memory --------------------------------------------------------------------

# the shapes of test_gpu_parity._cbox_spheres (two diffuse spheres, one small sphere light), clear of the mesh box's
# ball (centre 0.4, -0.7, 0.3, radius 0.3) and ring (around -0.35, -0.45, -0.2)
THREE_SPHERES = (
    '<shape type="sphere"><point name="center" x="-0.55" y="-0.7" z="0.6"/><float name="radius" value="0.3"/>'
    '<ref id="white"/></shape>'
    '<shape type="sphere"><point name="center" x="0.45" y="0.1" z="-0.55"/><float name="radius" value="0.25"/>'
    '<ref id="white"/></shape>'
    '<shape type="sphere"><point name="center" x="0.0" y="0.55" z="0.2"/><float name="radius" value="0.08"/>'
    '<emitter type="area"><rgb name="radiance" value="20, 20, 20"/></emitter></shape>')


def _sphere_field(n_spheres):
    """test_gpu_parity.test_many_spheres' field of small spheres."""
    balls = []
    for i in range(n_spheres):
        x, y, z = -0.8 + 0.2 * (i % 9), -0.9 + 0.22 * ((i // 9) % 9), -0.6 + 0.45 * (i // 81)
        balls.append('<shape type="sphere"><point name="center" x="%.3f" y="%.3f" z="%.3f"/>'
                     '<float name="radius" value="0.07"/><ref id="white"/></shape>' % (x, y, z))
    return "\n".join(balls)


@SIZES
@pytest.mark.parametrize("case", ["spheres_deferred", "spheres_in_place"])
def test_spheres_in_device_memory_bvh(gpu_ready, amvpt_mod, oracle, case, kw):
    """Spheres next to the 3.6 k-triangle meshes: the suffix walks are the WALK_LANE instances on the two-box tree
    (whole-record leaves, sphere tests behind float16 boxes, binned rays); the coherent primary and visibility rays
    walk the 8-copy threaded tree wave-uniformly with the float64 sphere tests deferred (3 spheres: at most 64) or
    in place (70 spheres)."""
    n_sph = 3 if case == "spheres_deferred" else 70
    s = amvpt_mod.load_string(_add(_xml("cbox_mesh.xml"), THREE_SPHERES if n_sph == 3 else _sphere_field(70)), **kw)
    dev, n_nodes, n_prims, n2, depth = _device_bvh(amvpt_mod, s)
    assert n_nodes > 255 and n_prims == 6 + 1280 + 2304 + n_sph
    assert n2 > 0 and 0 < depth <= 16
    _, k, _ = _check(amvpt_mod, oracle, s, dev, FLAG_SETS)
    assert k["k_bin"] > 0 and k["k_extend"] > 0 and k["k_suffix"] == 0


# ---- rectangles in BVH leaves ------------------------------------------------------------------------------------

def _rects_entered_the_tree(amvpt_mod, base_xml, kw):
    """9 rectangles exceed kOuterMax, so all of them become BVH primitives; with 8 they all stay outside."""
    s9 = amvpt_mod.load_string(_add(base_xml, _extra_rects(3)), **kw)
    s8 = amvpt_mod.load_string(_add(base_xml, _extra_rects(2)), **kw)
    dev, n9, p9, n2, depth = _device_bvh(amvpt_mod, s9)
    _, n8, p8, _, _ = _device_bvh(amvpt_mod, s8)
    assert p9 == p8 + 1
    assert n9 > n8 + 8, (n9, n8)
    return s9, dev, n2, depth


@SIZES
def test_rects_in_bvh(gpu_ready, amvpt_mod, oracle, kw):
    """More than 8 rectangles: the walls, the light and three small rectangles (one an area light) are leaves of the
    device-memory BVH next to the meshes' triangles -- WALK_LANE_NS on the two-box tree with whole-record leaves and
    the rectangle branch of the leaf test, NEE towards a rectangle light that is a BVH leaf."""
    s, dev, n2, depth = _rects_entered_the_tree(amvpt_mod, _xml("cbox_mesh.xml"), kw)
    assert n2 > 0 and 0 < depth <= 16
    _, k, _ = _check(amvpt_mod, oracle, s, dev, FLAG_SETS)
    assert k["k_bin"] > 0 and k["k_extend"] > 0 and k["k_suffix"] == 0


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["auto_brute_suffix", "wave_uniform", "per_lane_staged"])
def test_rects_in_small_bvh(gpu_ready, amvpt_mod, oracle, mode):
    """The Cornell box with 9 rectangles (33 primitives, all in the BVH): rectangle leaves under the coherent
    wave-uniform walks with the brute-force fused suffix (auto), the wave-uniform suffix (1) and the LDS-staged
    per-lane suffix (2)."""
    amvpt_mod.set_traversal(mode)
    try:
        s, dev, n2, _ = _rects_entered_the_tree(amvpt_mod, _xml("cbox_grid.xml"), G8)
        assert n2 == 0
        _, k, _ = _check(amvpt_mod, oracle, s, dev)
        assert k["k_bin"] == 0
        if mode == 0:
            assert k["k_suffix"] > 0 and k["k_extend"] == 0
        else:
            assert k["k_suffix"] == 0 and k["k_extend"] > 0
    finally:
        amvpt_mod.set_traversal(0)


# ---- the two-box stack bound -------------------------------------------------------------------------------------

def _heightfield_room(amvpt_mod, tmp_path, n, kw):
    """scene_gen._heightfield_room_xml, loaded."""
    xml, n_tri = _heightfield_room_xml(tmp_path, n)
    return amvpt_mod.load_string(xml, **kw), n_tri


@SIZES
def test_two_box_tree_at_the_stack_bound(gpu_ready, amvpt_mod, oracle, tmp_path, kw):
    """depth_16: a two-box tree exactly kStack2 = 16 inner nodes deep (a 128 x 128 heightfield, 32768 triangles):
    the deepest path pushes into the last stack entry of its thread; one more would land in the next thread's."""
    s, n_tri = _heightfield_room(amvpt_mod, tmp_path, 128, kw)
    dev, n_nodes, n_prims, n2, depth = _device_bvh(amvpt_mod, s)
    assert n_prims == 6 + n_tri == 6 + 32768
    assert depth == 16 and n2 > 0
    _, k, _ = _check(amvpt_mod, oracle, s, dev, FLAG_SETS, oracle_bvh=True)
    assert k["k_bin"] > 0 and k["k_extend"] > 0


@SIZES
def test_tree_past_the_stack_bound_stays_threaded(gpu_ready, amvpt_mod, oracle, tmp_path, kw):
    """depth_17: a tree one inner node deeper than the stack (a 200 x 200 heightfield, 80000 triangles) gets no
    two-box form; the suffix walks fall back to the threaded walks over the 8 octant copies, still binned, and
    AMVPT_OPT_THREADED_BVH changes nothing."""
    s, n_tri = _heightfield_room(amvpt_mod, tmp_path, 200, kw)
    dev, n_nodes, n_prims, n2, depth = _device_bvh(amvpt_mod, s)
    assert n_prims == 6 + n_tri == 6 + 80000
    assert depth == 17 and n2 == 0
    _, k, _ = _check(amvpt_mod, oracle, s, dev, FLAG_SETS, oracle_bvh=True)
    assert k["k_bin"] > 0 and k["k_extend"] > 0


# ---- leaves of more than 2 primitives ----------------------------------------------------------------------------

@pytest.mark.parametrize("scene,mode,kw", [("cbox_mesh.xml", 0, G8), ("cbox_mesh.xml", 0, G1),
                                           ("cbox_grid.xml", 1, G8), ("cbox_grid.xml", 2, G8)],
                         ids=["mesh_g8", "mesh_path_g1", "grid_wave_uniform", "grid_per_lane_staged"])
def test_wide_leaves(gpu_ready, amvpt_mod, oracle, scene, mode, kw):
    """amvpt_set_bvh_build(15, 8.0): a traversal cost that keeps leaves of up to 15 primitives (the 4-bit count
    fields, the leaf loops) -- the same records as the default build's and the oracle's, from a tree of less than
    half the nodes."""
    s = amvpt_mod.load_string(_xml(scene), **kw)
    sd, vd, p = s.describe(0, 0, 0)
    amvpt_mod.set_traversal(mode)
    try:
        narrow, n_narrow, prims_narrow, _, _ = _device_bvh(amvpt_mod, s)
        amvpt_mod.set_bvh_build(15, 8.0)
        try:
            wide, n_wide, prims_wide, n2, depth = _device_bvh(amvpt_mod, s)
        finally:
            amvpt_mod.set_bvh_build(4, 0.0)
        assert prims_wide == prims_narrow and 2 * n_wide < n_narrow, (n_wide, n_narrow)
        if mode == 0:
            assert n_wide > 255 and n2 > 0 and 0 < depth <= 16
        rec, k, _ = _check(amvpt_mod, oracle, s, wide, FLAG_SETS if mode == 0 else ())
        assert k["k_extend"] > 0 and (k["k_bin"] > 0) == (mode == 0)
        _, ref = _render(amvpt_mod, narrow, vd, p, oracle.plan(p))
        assert _bit_equal(rec, ref).all()
    finally:
        amvpt_mod.set_traversal(0)


# ---- the float16 node frame --------------------------------------------------------------------------------------

@SIZES
@pytest.mark.parametrize("case", ["wide_frame_edge", "wide_frame_centre"])
def test_wide_float16_frame(gpu_ready, amvpt_mod, oracle, tmp_path, case, kw):
    """A root box 2000 times wider than the room sets the two-box nodes' float16 frame: with one far triangle at
    x = +2000 the room sits near -1 of the frame (float16 steps of 2^-11, half a unit of the scene), with one at
    each of x = -2000 and +2000 near 0 (denormal halves).  Every child plane must round outwards: the records equal
    the threaded walks' (float boxes) and the oracle's."""
    obj = str(tmp_path / "triangle.obj")
    _triangle_obj(obj)
    far = _obj_shape(obj, '<translate x="2000" y="0.3"/>')
    if case == "wide_frame_centre":
        far += _obj_shape(obj, '<translate x="-2000" y="-0.3"/>')
    s = amvpt_mod.load_string(_add(_xml("cbox_mesh.xml"), far), **kw)
    dev, n_nodes, n_prims, n2, depth = _device_bvh(amvpt_mod, s)
    assert n_prims == 6 + 1280 + 2304 + (2 if case == "wide_frame_centre" else 1)
    assert n2 > 0 and 0 < depth <= 16
    _, k, _ = _check(amvpt_mod, oracle, s, dev, FLAG_SETS)
    assert k["k_bin"] > 0 and k["k_extend"] > 0


# ---- the LDS-staged tier in automatic mode -----------------------------------------------------------------------

def _grid_with_heightfield(amvpt_mod, tmp_path, n, kw, loose=0):
    """scene_gen._grid_with_heightfield_xml, loaded."""
    xml, n_tri = _grid_with_heightfield_xml(tmp_path, n, loose)
    return amvpt_mod.load_string(xml, **kw), n_tri


@SIZES
def test_staged_auto(gpu_ready, amvpt_mod, oracle, tmp_path, kw):
    """The Cornell box plus a 12 x 12 heightfield: more than 255 nodes in less than 48 KiB, so automatic mode stages
    the BVH in LDS (several blocks' worth of the cooperative copy) and walks it per lane, unbinned."""
    s, n_tri = _grid_with_heightfield(amvpt_mod, tmp_path, 12, kw)
    dev, n_nodes, n_prims, n2, depth = _device_bvh(amvpt_mod, s)
    assert n_prims == 6 + 24 + n_tri == 6 + 24 + 288
    assert n_nodes > 255 and n_nodes * 32 + n_prims * 64 <= 48 * 1024
    assert n2 == 0
    _, k, _ = _check(amvpt_mod, oracle, s, dev)
    assert k["k_bin"] == 0 and k["k_extend"] > 0 and k["k_suffix"] == 0


@SIZES
def test_just_past_staged(gpu_ready, amvpt_mod, oracle, tmp_path, kw):
    """A 16 x 16 heightfield instead: past 48 KiB, the BVH stays in device memory (two-box tree, binned rays)."""
    s, n_tri = _grid_with_heightfield(amvpt_mod, tmp_path, 16, kw)
    dev, n_nodes, n_prims, n2, depth = _device_bvh(amvpt_mod, s)
    assert n_prims == 6 + 24 + n_tri == 6 + 24 + 512
    assert n_nodes * 32 + (n_prims - 6) * 64 > 48 * 1024
    assert n2 > 0 and 0 < depth <= 16
    _, k, _ = _check(amvpt_mod, oracle, s, dev, FLAG_SETS)
    assert k["k_bin"] > 0 and k["k_extend"] > 0


@pytest.mark.parametrize("loose,staged", [(31, True), (32, False), (35, False)],
                         ids=["96_bytes_under", "32_bytes_over", "352_bytes_over"])
def test_staging_threshold(gpu_ready, amvpt_mod, oracle, tmp_path, loose, staged):
    """Either side of the 48 KiB limit, to the record: a 15 x 15 heightfield and 31 / 32 single triangles make
    49056 / 49184 bytes of nodes and primitives.  The bytes are those the staged tier copies -- BVH nodes, BVH
    primitives AND the rectangles kept outside the BVH -- in the renderer's choice of the tier and in the scene
    build's choice of what to build for it (octant copies, two-box tree): a BVH within 6 x 64 bytes under the limit
    without the rectangles (35 triangles: 49120 bytes without, 49504 with) once got neither tier."""
    s, n_tri = _grid_with_heightfield(amvpt_mod, tmp_path, 15, G8, loose=loose)
    dev, n_nodes, n_prims, n2, depth = _device_bvh(amvpt_mod, s)
    assert n_prims == 6 + 24 + n_tri == 6 + 24 + 450 + loose
    size = n_nodes * 32 + n_prims * 64
    assert n_nodes > 255 and (size <= 48 * 1024) == staged and abs(size - 48 * 1024) < 512, size
    _, k, _ = _check(amvpt_mod, oracle, s, dev, () if staged else FLAG_SETS)
    assert k["k_extend"] > 0 and k["k_suffix"] == 0
    if staged:
        assert n2 == 0 and k["k_bin"] == 0
    else:
        assert n2 > 0 and 0 < depth <= 16 and k["k_bin"] > 0

"""Guide buffers on the device (include/amvpt_guides.h) against the oracle's primary-hit hook.

The bar: DeviceScene.guides equals oracle.primary_hits on every float of every pixel (the bit patterns), and
guide_depth on the device equals guide_depth_host.  What changes from case to case is which instance of k_guides
runs (wave-uniform or per-lane), where the BVH lies (scalar loads from device memory, LDS-staged, per-lane loads from
device memory), which sensor layout maps pixels to views, and whether pixels miss.  Every case asserts the evidence
of its regime -- node counts, the staged size, the traversal mode it set, hit and miss pixels -- in the style of
test_gpu_bvh_walks.py, whose generated meshes it borrows.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENES
from test_gpu_bvh_walks import _grid_with_heightfield, _heightfield_obj, _heightfield_room, _torch
from test_guides import bits, open_scene_xml

pytestmark = pytest.mark.gpu

F = np.float32
Q8 = dict(res=32, gx=4, gy=2)       # 8 views of 32 x 32: a 128 x 64 quilt, 32 blocks of 256 pixels
GUARD = 256                         # floats after every output buffer that must stay as they were
SENTINEL = -12345.0
LDS_SCENE_BYTES = 48 * 1024
UNIFORM_NODES = 255                 # the automatic mode's wave-uniform tier: BVHs of at most this many nodes


@pytest.fixture(scope="module", autouse=True)
def _device_started(gpu_ready, amvpt_mod):
    """The process's one-time costs (importing torch, creating the HIP context, loading the code objects) are paid
    here when this module is the first to use the device, so that `--durations` shows each case's own time."""
    torch = _torch()
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=4, gx=2, gy=2)
    sd, vd, p = s.describe(0, 0, 0)
    out = torch.zeros((p.film_height * p.film_width * 8,), dtype=torch.float32, device="cuda")
    amvpt_mod.DeviceScene(sd).guides(vd, p, out.data_ptr())
    torch.cuda.synchronize()


def _guides(dev, vd, p, rect=None):
    """The records of `rect` (None: the whole quilt crop) as (h, w, 8); the guard after them must be untouched."""
    torch = _torch()
    w, h = (rect[2], rect[3]) if rect is not None else (p.film_width, p.film_height)
    buf = torch.full((h * w * 8 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    dev.guides(vd, p, buf.data_ptr(), rect=rect)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[h * w * 8:] == F(SENTINEL)).all(), "the guard region after the output was written"
    return host[:h * w * 8].reshape(h, w, 8), buf


def _assert_records(got, ref):
    assert got.shape == ref.shape
    eq = (bits(got) == bits(ref)).all(axis=-1)
    if not eq.all():
        for y, x in np.argwhere(~eq)[:5]:
            print("pixel", (x, y), "\ngpu   ", got[y, x], "\noracle", ref[y, x])
    assert eq.all(), "guide records: %d of %d pixels differ from the oracle" % ((~eq).sum(), eq.size)


def _device_depth(amvpt_mod, buf, vd, p, n):
    torch = _torch()
    z = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    amvpt_mod.guide_depth(buf.data_ptr(), vd, p.n_views, n, z.data_ptr())
    torch.cuda.synchronize()
    host = z.cpu().numpy()
    assert (host[n:] == F(SENTINEL)).all()
    return host[:n], z


def _check(amvpt_mod, oracle, scene, dev=None, oracle_bvh=False):
    """The two bars on `scene`; returns (records, oracle records, device scene)."""
    sd, vd, p = scene.describe(0, 0, 0)
    oracle.set_bvh(bool(oracle_bvh))
    try:
        ref = oracle.primary_hits(sd, vd, p)
    finally:
        oracle.set_bvh(False)
    dev = dev or amvpt_mod.DeviceScene(sd)
    got, buf = _guides(dev, vd, p)
    _assert_records(got, ref)
    z, _ = _device_depth(amvpt_mod, buf, vd, p, got.shape[0] * got.shape[1])
    assert np.array_equal(bits(z), bits(amvpt_mod.guide_depth_host(ref, vd, p.n_views).ravel()))
    return got, ref, dev


def _mesh_shape(scene, n_faces):
    """Index of the one mesh of n_faces triangles in the scene's shape table: what record[0] holds for it."""
    sd = scene.describe(0, 0, 0)[0].contents
    found = [i for i in range(sd.shape_count) if sd.shapes[i].type == 1 and sd.shapes[i].face_count == n_faces]
    assert len(found) == 1
    return found[0]


def _hit_and_miss(rec):
    hit = rec[..., 0] >= 0
    return hit.any() and (~hit).any()


def _views_cover(rec, p):
    """Every view index appears, and tile (tx, ty) holds one view only."""
    view = rec[..., 7].astype(int)
    assert sorted(np.unique(view)) == list(range(p.n_views))
    return view


# ---- the sensor layouts, on a BVH small enough for the wave-uniform instance ----------------------------------------

@pytest.mark.parametrize("defines", [dict(), dict(cam="thinlens")], ids=["perspective", "thinlens"])
def test_grid_of_views(gpu_ready, amvpt_mod, oracle, defines):
    """cbox_grid.xml, 4 x 2 views: the automatic mode's wave-uniform instance on a brute-force-sized scene; with
    thin-lens cameras the ray leaves the centre of the lens (aperture sample (.5, .5))."""
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), **Q8, **defines)
    _, vd, p = s.describe(0, 0, 0)
    assert (p.film_width, p.film_height, p.n_views, p.multisensor, p.batch) == (128, 64, 8, 1, 0)
    assert vd[0].type == (1 if defines else 0) and (not defines or vd[0].aperture_radius > 0)
    got, _, dev = _check(amvpt_mod, oracle, s)
    n_nodes, n_prims = dev.stats()
    assert n_nodes <= UNIFORM_NODES and n_prims <= 48
    view = _views_cover(got, p)
    assert all(len(np.unique(view[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32])) == 1 for ty in range(2) for tx in range(4))
    assert _hit_and_miss(got)   # the outer views look past the edges of the box's open front


@pytest.mark.parametrize("defines", [dict(), dict(revx="true", offx="0.1")], ids=["defaults", "revx_offx"])
def test_cone_layout(gpu_ready, amvpt_mod, oracle, defines):
    """cbox_cone.xml: lens-shifted views on a cone, reverse_y by default and reverse_x on request -- the view index
    and the tile order of the record."""
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_cone.xml"), res=32, **defines)
    _, vd, p = s.describe(0, 0, 0)
    assert (p.reverse_x, p.reverse_y) == (1 if defines else 0, 1) and (p.grid_x, p.grid_y) == (4, 2)
    got, _, dev = _check(amvpt_mod, oracle, s)
    assert dev.stats()[0] <= UNIFORM_NODES
    view = _views_cover(got, p)
    for ty in range(2):
        for tx in range(4):
            want = (3 - tx if defines else tx) + 4 * (1 - ty)
            assert (view[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32] == want).all()


def test_batch_layout_with_a_crop(gpu_ready, amvpt_mod, oracle):
    """cbox_batch.xml, four views side by side, cropped off the 32-pixel tile boundaries on every side (a width the
    four views divide, as every render of a MultiSensor needs)."""
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_batch.xml"), res=32, width=128, crop_x=13, crop_w=68, crop_y=3,
                            crop_h=21)
    _, vd, p = s.describe(0, 0, 0)
    assert (p.batch, p.multisensor, p.n_views) == (1, 1, 4)
    assert (p.film_width, p.film_height, p.crop_offset_x, p.crop_offset_y, p.full_width) == (68, 21, 13, 3, 128)
    got, _, _ = _check(amvpt_mod, oracle, s)
    view = _views_cover(got, p)
    assert (np.diff(view, axis=1) >= 0).all()


def test_single_camera_with_a_crop(gpu_ready, amvpt_mod, oracle):
    """cbox_path.xml: one perspective camera (multisensor = 0), a crop window off every edge."""
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_path.xml"), res=64, crop_x=7, crop_y=5, crop_w=41, crop_h=23)
    _, vd, p = s.describe(0, 0, 0)
    assert (p.multisensor, p.n_views, p.film_width, p.film_height, p.crop_offset_x, p.crop_offset_y) == (0, 1, 41, 23, 7, 5)
    got, _, _ = _check(amvpt_mod, oracle, s)
    assert (got[..., 7] == 0).all() and (got[..., 0] >= 0).any()


def test_spheres(gpu_ready, amvpt_mod, oracle):
    """veach_grid.xml: spheres, whose intersection is float64 on both sides."""
    s = amvpt_mod.load_file(os.path.join(SCENES, "veach_grid.xml"), res=32)
    sd, vd, p = s.describe(0, 0, 0)
    sphere_shapes = [i for i in range(sd.contents.shape_count) if sd.contents.shapes[i].type == 2]
    assert sphere_shapes and p.n_views == 8
    got, _, dev = _check(amvpt_mod, oracle, s)
    assert dev.stats()[0] <= UNIFORM_NODES
    assert np.isin(got[..., 0], sphere_shapes).any(), "no pixel sees a sphere"


def test_thirty_two_views(gpu_ready, amvpt_mod, oracle):
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=16, gx=8, gy=4)
    _, vd, p = s.describe(0, 0, 0)
    assert p.n_views == 32 and (p.film_width, p.film_height) == (128, 64)
    got, _, _ = _check(amvpt_mod, oracle, s)
    _views_cover(got, p)


# ---- the per-lane instance and the BVH tiers -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", [2, 0], ids=["per_lane_device_memory", "auto_wave_uniform"])
def test_mesh(gpu_ready, amvpt_mod, oracle, mode):
    """cbox_mesh.xml (3.6 k triangles, a BVH past the 48 KiB that LDS stages): amvpt_set_traversal(2) takes the
    per-lane instance with per-lane loads from device memory; the automatic mode walks the same BVH wave-uniformly
    (its direction-octant copies)."""
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_mesh.xml"), **Q8)
    amvpt_mod.set_traversal(mode)
    try:
        dev = amvpt_mod.DeviceScene(s.describe(0, 0, 0)[0])
        n_nodes, n_prims = dev.stats()
        assert n_prims == 6 + 1280 + 2304
        assert n_nodes > UNIFORM_NODES and n_nodes * 32 + n_prims * 64 > LDS_SCENE_BYTES
        got, _, _ = _check(amvpt_mod, oracle, s, dev)
    finally:
        amvpt_mod.set_traversal(0)
    assert len(np.unique(got[..., 0])) >= 6   # walls, light, ball and ring


@pytest.mark.parametrize("mode", [2, 0], ids=["per_lane_staged", "auto_wave_uniform"])
def test_staged_heightfield(gpu_ready, amvpt_mod, oracle, tmp_path, mode):
    """The Cornell box plus a 12 x 12 heightfield: more than 255 nodes in less than 48 KiB.  Per-lane mode stages
    the BVH in LDS (32 blocks make the cooperative copy); the automatic mode reads it with scalar loads."""
    amvpt_mod.set_traversal(mode)
    try:
        s, n_tri = _grid_with_heightfield(amvpt_mod, tmp_path, 12, Q8)
        dev = amvpt_mod.DeviceScene(s.describe(0, 0, 0)[0])
        n_nodes, n_prims = dev.stats()
        assert n_prims == 6 + 24 + n_tri == 6 + 24 + 288
        assert n_nodes > UNIFORM_NODES and n_nodes * 32 + n_prims * 64 <= LDS_SCENE_BYTES
        got, _, _ = _check(amvpt_mod, oracle, s, dev)
    finally:
        amvpt_mod.set_traversal(0)
    assert (got[..., 0] == _mesh_shape(s, n_tri)).sum() > 50, "the heightfield (seen nearly edge-on) is missing"


@pytest.mark.parametrize("mode", [0, 2], ids=["auto_wave_uniform", "per_lane_device_memory"])
def test_deep_tree(gpu_ready, amvpt_mod, oracle, tmp_path, mode):
    """A 200 x 200 heightfield (80000 triangles, a tree 17 inner nodes deep, the oracle in its BVH mode), 16 x 16
    pixels per view."""
    amvpt_mod.set_traversal(mode)
    try:
        s, n_tri = _heightfield_room(amvpt_mod, tmp_path, 200, dict(res=16, gx=4, gy=2))
        dev = amvpt_mod.DeviceScene(s.describe(0, 0, 0)[0])
        n_nodes, n_prims = dev.stats()
        assert n_prims == 6 + n_tri == 6 + 80000 and n_nodes > 20000
        if mode == 0:
            assert dev.bvh2() == (0, 17)
        got, _, _ = _check(amvpt_mod, oracle, s, dev, oracle_bvh=True)
    finally:
        amvpt_mod.set_traversal(0)
    assert (got[..., 0] == _mesh_shape(s, n_tri)).sum() > 100   # the heightfield lies on the floor


# ---- misses --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def open_scene(amvpt_mod, tmp_path_factory):
    """A heightfield, a sphere and the light rectangle in empty space."""
    obj = str(tmp_path_factory.mktemp("guides") / "heightfield_12.obj")
    _heightfield_obj(obj, 12)
    return amvpt_mod.load_string(open_scene_xml(obj), **Q8)


@pytest.mark.parametrize("mode", [0, 2], ids=["auto_wave_uniform", "per_lane_staged"])
def test_misses(gpu_ready, amvpt_mod, oracle, open_scene, mode):
    """No walls: every view tile holds hit and miss pixels.  A miss is shape -1, a zero normal and point, and still
    the pixel's view index."""
    amvpt_mod.set_traversal(mode)
    try:
        got, ref, dev = _check(amvpt_mod, oracle, open_scene)
    finally:
        amvpt_mod.set_traversal(0)
    n_nodes, n_prims = dev.stats()
    print("BVH: %d nodes, %d primitives" % (n_nodes, n_prims))
    # small enough for LDS: the per-lane mode stages it; the automatic mode walks it wave-uniformly whatever its size
    assert n_prims == 1 + 1 + 288 and n_nodes * 32 + n_prims * 64 <= LDS_SCENE_BYTES
    for ty in range(2):
        for tx in range(4):
            tile = got[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32]
            assert _hit_and_miss(tile), "view tile (%d, %d)" % (tx, ty)
            assert len(np.unique(tile[..., 7])) == 1
    miss = got[..., 0] < 0
    assert (got[miss][:, 0] == -1).all() and (got[miss][:, 1:7] == 0).all()
    assert len(np.unique(got[~miss][:, 0])) == 3   # the light, the sphere and the heightfield are all seen


# ---- rectangles, independence, depth planes, refusals, the host layer ---------------------------------------------

@pytest.fixture(scope="module")
def grid_case(amvpt_mod):
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), **Q8)
    sd, vd, p = s.describe(0, 0, 0)
    dev = amvpt_mod.DeviceScene(sd)
    whole, _ = _guides(dev, vd, p)
    return s, dev, vd, p, whole


@pytest.mark.parametrize("rect", [(5, 3, 41, 27), (17, 9, 1, 1), (0, 63, 128, 1), (127, 0, 1, 64)],
                         ids=["41x27", "one_pixel", "last_row", "last_column"])
def test_rectangles(gpu_ready, amvpt_mod, grid_case, rect):
    """A rectangle equals the same window of the whole-quilt result: pixel counts that are no multiple of 64 or 256,
    rows that start anywhere, and nothing written past the last record."""
    _, dev, vd, p, whole = grid_case
    x0, y0, w, h = rect
    got, _ = _guides(dev, vd, p, rect=rect)
    assert np.array_equal(bits(got), bits(whole[y0:y0 + h, x0:x0 + w]))


def test_independent_of_the_sampling(gpu_ready, amvpt_mod, grid_case):
    """No sampler, no filter: spp, seed, group size, adaptive passes and the integrator do not change a bit."""
    _, dev, vd, p, whole = grid_case
    assert (p.integrator, p.reuse_count, p.adaptive) == (amvpt_mod.INTEGRATOR_MVPATH, 4, 0)
    for field, values in (("spp", (1, 64)), ("seed", (0, 7)), ("reuse_count", (1, 8)), ("adaptive", (0, 3)),
                          ("integrator", (amvpt_mod.INTEGRATOR_PATH, amvpt_mod.INTEGRATOR_MVPATH)),
                          ("hide_emitters", (0, 1)), ("rfilter", (amvpt_mod.RFILTER_BOX, amvpt_mod.RFILTER_TENT))):
        for v in values:
            q = amvpt_mod.Params.from_buffer_copy(p)
            setattr(q, field, v)
            got, _ = _guides(dev, vd, q)
            assert np.array_equal(bits(got), bits(whole)), "%s = %d changed the guide records" % (field, v)


def test_depth_range_and_depth8(gpu_ready, amvpt_mod, open_scene):
    """The device's range and 8-bit codes equal the host forms: a plane with misses, a 41 x 27 window of it (3 w no
    multiple of 4, a pixel count no multiple of 4: the byte tail) and an output that is not dword-aligned."""
    torch = _torch()
    sd, vd, p = open_scene.describe(0, 0, 0)
    dev = amvpt_mod.DeviceScene(sd)
    for rect in (None, (5, 3, 41, 27)):
        got, buf = _guides(dev, vd, p, rect=rect)
        h, w = got.shape[:2]
        z_host = amvpt_mod.guide_depth_host(got, vd, p.n_views)
        assert np.isinf(z_host).any() and np.isfinite(z_host).any()
        z, zbuf = _device_depth(amvpt_mod, buf, vd, p, h * w)
        assert np.array_equal(bits(z), bits(z_host.ravel()))
        lo, hi = amvpt_mod.guide_depth_range(zbuf.data_ptr(), h * w)
        hlo, hhi = amvpt_mod.guide_depth_range_host(z_host)
        assert (bits(lo), bits(hi)) == (bits(hlo), bits(hhi)) and 0 < lo < hi
        assert (lo, hi) == (z_host[np.isfinite(z_host)].min(), z_host[np.isfinite(z_host)].max())
        for near, far in ((lo, hi), (F(3.5), F(4.0)), (F(4.0), F(4.0))):
            want = amvpt_mod.depth8_host(z_host, near, far)
            for shift in (0, 1):
                out = torch.full((h * w * 3 + 64,), 77, dtype=torch.uint8, device="cuda")
                amvpt_mod.depth8(zbuf.data_ptr(), w, h, near, far, out.data_ptr() + shift)
                torch.cuda.synchronize()
                o = out.cpu().numpy()
                assert np.array_equal(o[shift:shift + h * w * 3].reshape(h, w, 3), want)
                assert (o[:shift] == 77).all() and (o[shift + h * w * 3:] == 77).all()
    empty = torch.full((300,), float("inf"), dtype=torch.float32, device="cuda")
    assert amvpt_mod.guide_depth_range(empty.data_ptr(), 300) == (0.0, 0.0)


def test_out_of_range_views_are_misses_on_the_device(gpu_ready, amvpt_mod, grid_case):
    """A record whose view index is outside the table: the device entry writes +inf, the host entry refuses."""
    torch = _torch()
    _, dev, vd, p, whole = grid_case
    rec = whole.reshape(-1, 8).copy()
    hits = np.flatnonzero(rec[:, 0] >= 0)[:4]
    rec[hits, 7] = [8.0, -1.0, np.nan, 1e30]
    buf = torch.from_numpy(rec).cuda()
    z, _ = _device_depth(amvpt_mod, buf, vd, p, len(rec))
    assert np.isposinf(z[hits]).all()
    rec[hits, 7] = 0.0
    ok = amvpt_mod.guide_depth_host(rec, vd, p.n_views)
    keep = np.ones(len(rec), bool)
    keep[hits] = False
    assert np.array_equal(bits(z[keep]), bits(ok[keep]))


def test_refusals(gpu_ready, amvpt_mod, grid_case):
    _, dev, vd, p, _ = grid_case
    torch = _torch()
    out = torch.zeros((128 * 64 * 8,), dtype=torch.float32, device="cuda")
    L = dev._lib

    def status(rect, ptr):
        r = ctypes.byref((ctypes.c_uint32 * 4)(*rect)) if rect else None
        return L.amvpt_guides(dev.h, vd, ctypes.byref(p), r, ctypes.c_void_p(ptr), None), L.amvpt_last_error().decode()

    for rect in ((100, 0, 29, 10), (0, 60, 10, 5), (128, 0, 1, 1), (0xffffffff, 0, 2, 1)):
        rc, msg = status(rect, out.data_ptr())
        assert rc == 1 and "amvpt_guides: rect" in msg and "outside the quilt crop" in msg, (rect, msg)
    for rect in ((0, 0, 0, 5), (0, 0, 5, 0)):
        rc, msg = status(rect, out.data_ptr())
        assert rc == 1 and "amvpt_guides: rect has zero area" in msg
    rc, msg = status(None, 0)
    assert rc == 1 and "amvpt_guides: null out_device" in msg
    rc, msg = status(None, out.data_ptr() + 4)
    assert rc == 1 and "out_device must be 16-byte aligned" in msg
    bad = amvpt_mod.Params.from_buffer_copy(p)
    bad.n_views = 7   # as amvpt_render_ex refuses it
    with pytest.raises(RuntimeError, match="n_views == grid_x \\* grid_y"):
        dev.guides(vd, bad, out.data_ptr())
    torch.cuda.synchronize()
    assert (out == 0).all()


def test_host_layer(gpu_ready, amvpt_mod, grid_case):
    """amvpt.guides after amvpt.render runs on the device scene the render cached, and equals the C-ABI's records;
    amvpt.depth and display.depth_quilt are the composition of the pieces."""
    import amvpt.display as D
    _, _, vd, p, whole = grid_case
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), spp=4, **Q8)
    img = amvpt_mod.render(s)
    before = amvpt_mod.render_stats(s)
    assert (before["scene_creates"], before["renders"]) == (1, 1)
    g = amvpt_mod.guides(s)
    z = amvpt_mod.depth(s)
    assert amvpt_mod.render_stats(s) == before   # no second device scene, no cached buffer touched
    assert g.shape == (64, 128, 8) and np.array_equal(bits(g), bits(whole))
    assert np.array_equal(bits(z), bits(amvpt_mod.guide_depth_host(whole, vd, p.n_views)))
    lo, hi = amvpt_mod.guide_depth_range_host(z)
    assert np.array_equal(D.depth_quilt(s), amvpt_mod.depth8_host(z, lo, hi))
    assert np.array_equal(D.depth_quilt(s, near=3.0, far=5.0), amvpt_mod.depth8_host(z, 3.0, 5.0))
    assert img.shape == (64, 128, 3)
    # a scene that has not rendered yet creates its device scene for the guides, once
    fresh = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), **Q8)
    assert np.array_equal(bits(amvpt_mod.guides(fresh)), bits(whole))
    assert np.array_equal(bits(amvpt_mod.depth(fresh)), bits(z))
    assert amvpt_mod.render_stats(fresh)["scene_creates"] == 1

"""Guide buffers on the CPU (include/amvpt_guides.h, the EXR channel writer): the host entries against numpy float32
restatements of their definitions, bit for bit.  The records come from the oracle's primary-hit hook, which is what
amvpt_guides reproduces on the device (tests/test_gpu_guides.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import SCENES

F = np.float32


def xml_of(name):
    """A stock scene's text with its mesh paths made absolute (load_string has no base directory)."""
    xml = open(os.path.join(SCENES, name)).read()
    return xml.replace('value="meshes/', 'value="%s/meshes/' % SCENES)


def obj_shape(path, transform, bsdf="white"):
    return ('<shape type="obj"><string name="filename" value="%s"/><transform name="to_world">%s</transform>'
            '<ref id="%s"/></shape>' % (path, transform, bsdf))


def open_scene_xml(heightfield_obj=None):
    """cbox_grid.xml without its walls and boxes: a sphere, the light rectangle and (given an OBJ) a heightfield that
    faces the cameras, in empty space -- every view sees them in its middle and nothing at its corners."""
    xml, n = re.subn(r'<shape type="(?:rectangle|cube)" id="(?!light")[^"]*">.*?</shape>\s*', "", xml_of("cbox_grid.xml"),
                     flags=re.S)
    assert n == 7 and 'id="light"' in xml
    shapes = ('<shape type="sphere"><point name="center" x="0.35" y="-0.1" z="0.1"/><float name="radius" value="0.4"/>'
              '<ref id="green"/></shape>')
    if heightfield_obj:
        shapes += obj_shape(heightfield_obj, '<scale value="0.9"/><translate x="-0.4" y="0.1" z="-0.2"/>')
    return xml.replace("</scene>", shapes + "\n</scene>")


def depth_restated(hits, vd, n_views):
    """The header's formula in numpy float32: every product and sum rounded on its own."""
    m = np.array([list(vd[v].to_world_inv) for v in range(n_views)], dtype=F)
    view = hits[..., 7].astype(np.int64)
    assert (view >= 0).all() and (view < n_views).all()
    r = m[view]
    px, py, pz = hits[..., 4], hits[..., 5], hits[..., 6]
    z = ((r[..., 8] * px + r[..., 9] * py).astype(F) + (r[..., 10] * pz).astype(F)).astype(F) + r[..., 11]
    return np.where(hits[..., 0] >= 0, z.astype(F), F(np.inf)).astype(F)


def depth8_restated(z, near, far):
    z = np.asarray(z, dtype=F)
    near, far = F(near), F(far)
    span = F(far - near)
    with np.errstate(all="ignore"):
        t = ((far - z).astype(F) / span).astype(F)
        t = np.where(t > 0, np.where(t < 1, t, F(1)), F(0)).astype(F)   # a NaN gives 0
        code = np.rint((F(255) * t).astype(F))                            # half to even
    code = np.where(np.isfinite(z), F(255) if span == 0 else code, F(0)).astype(np.uint8)
    return np.repeat(code[..., None], 3, axis=-1)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def grid_hits(oracle, amvpt_mod):
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=16, gx=4, gy=2)
    sd, vd, p = s.describe(0, 0, 0)
    return s, vd, p, oracle.primary_hits(sd, vd, p)


@pytest.fixture(scope="module")
def open_hits(oracle, amvpt_mod):
    s = amvpt_mod.load_string(open_scene_xml(), res=16, gx=4, gy=2)
    sd, vd, p = s.describe(0, 0, 0)
    return s, vd, p, oracle.primary_hits(sd, vd, p)


def test_versions(amvpt_mod):
    assert amvpt_mod.guides_version() == 1
    assert amvpt_mod.hip_lib().amvpt_guides_version() == 1
    assert amvpt_mod.hip_lib().amvpt_abi_version() == 12


def test_depth_of_the_closed_box(amvpt_mod, grid_hits):
    _, vd, p, hits = grid_hits
    hit = hits[..., 0] >= 0
    assert hits.shape == (32, 64, 8) and hit.mean() > 0.8   # the off-axis views look past the open front's edges
    z = amvpt_mod.guide_depth_host(hits, vd, p.n_views)
    assert z.shape == (32, 64) and z.dtype == F
    assert np.array_equal(bits(z), bits(depth_restated(hits, vd, p.n_views)))
    # planar depth in front of cameras 3.9 from the origin of a box of half-width 1: between the box's front and back
    assert 2.0 < z[hit].min() < z[hit].max() < 5.1 and np.isposinf(z[~hit]).all()
    assert len(np.unique(hits[..., 7])) == 8


def test_depth_of_a_scene_with_misses(amvpt_mod, open_hits):
    _, vd, p, hits = open_hits
    miss = hits[..., 0] < 0
    assert miss.any() and (~miss).any()
    z = amvpt_mod.guide_depth_host(hits, vd, p.n_views)
    assert np.array_equal(bits(z), bits(depth_restated(hits, vd, p.n_views)))
    assert np.isposinf(z[miss]).all() and np.isfinite(z[~miss]).all()


def test_depth_refusals(amvpt_mod, grid_hits):
    _, vd, p, hits = grid_hits
    bad = hits.copy()
    bad[3, 5, 7] = 8.0
    with pytest.raises(RuntimeError, match=r"amvpt_guide_depth_host: guides: the view index of pixel 197 "):
        amvpt_mod.guide_depth_host(bad, vd, p.n_views)
    L = amvpt_mod.hip_lib()
    out = np.zeros(4, dtype=F)
    for args, name in (((None, vd, 8, 4, out.ctypes.data), "null guides"),
                       ((hits.ctypes.data, None, 8, 4, out.ctypes.data), "null views"),
                       ((hits.ctypes.data, vd, 8, 4, None), "null depth")):
        assert L.amvpt_guide_depth_host(*args) == 1
        assert name in L.amvpt_last_error().decode()


def test_depth_range(amvpt_mod, grid_hits, open_hits):
    for _, vd, p, hits in (grid_hits, open_hits):
        z = amvpt_mod.guide_depth_host(hits, vd, p.n_views)
        lo, hi = amvpt_mod.guide_depth_range_host(z)
        fin = z[np.isfinite(z)]
        assert bits(lo) == bits(fin.min()) and bits(hi) == bits(fin.max())
    assert amvpt_mod.guide_depth_range_host(np.full((4, 5), np.inf, dtype=F)) == (0.0, 0.0)
    assert amvpt_mod.guide_depth_range_host(np.zeros((0,), dtype=F)) == (0.0, 0.0)
    mixed = np.array([np.nan, -np.inf, 3.5, -2.25, np.inf, 1e-40, 7.0], dtype=F)   # any finite value orders
    assert amvpt_mod.guide_depth_range_host(mixed) == (F(-2.25), F(7.0))


def test_depth8(amvpt_mod):
    near, far = F(1.0), F(3.0)
    # exact half codes: t = (2 k + 1) / 510 has no float32 form, but z = far - 2 t does for k / 255 + 1 / 510 ...
    # take the z whose 255 t lands exactly on k + 0.5 after the float32 operations instead
    ks = np.arange(0, 255, dtype=np.float64)
    cand = (far - (ks + 0.5) / 255.0 * 2.0).astype(F)
    with np.errstate(all="ignore"):
        t = ((far - cand).astype(F) / F(2.0)).astype(F)
        halves = cand[(F(255) * t).astype(F) == (ks + 0.5).astype(F)]
    assert halves.size > 20, "the ramp must hold exact half codes"
    ramp = np.concatenate([np.linspace(0.5, 3.5, 997, dtype=F), halves,
                           np.array([np.inf, -np.inf, np.nan, 1.0, 3.0, 2.0, -5.0, 1e30], dtype=F)])
    ramp = np.resize(ramp, (7, (ramp.size + 6) // 7)).astype(F)
    got = amvpt_mod.depth8_host(ramp, near, far)
    want = depth8_restated(ramp, near, far)
    assert got.shape == ramp.shape + (3,) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() == 255 and len(np.unique(got)) == 256
    # half to even on the exact halves: k + 0.5 -> the even one of k, k + 1
    h8 = amvpt_mod.depth8_host(halves.reshape(1, -1), near, far)[0, :, 0]
    assert (h8 % 2 == 0).all()
    # near == far: 255 for every hit, 0 for what is not finite
    same = amvpt_mod.depth8_host(ramp, 2.0, 2.0)
    assert np.array_equal(same, depth8_restated(ramp, 2.0, 2.0))
    assert (same[np.isfinite(ramp)] == 255).all() and (same[~np.isfinite(ramp)] == 0).all()
    for near_, far_, name in ((np.nan, 1.0, "near is not finite"), (0.0, np.inf, "far is not finite"),
                              (-np.inf, 1.0, "near is not finite"), (2.0, 1.0, "far is below near")):
        with pytest.raises(RuntimeError, match="amvpt_depth8_host: " + name):
            amvpt_mod.depth8_host(ramp, near_, far_)


def test_exr_channels_round_trip(amvpt_mod, tmp_path):
    names = ["view", "R", "N.Z", "G", "id", "B", "Z", "P.Y", "N.X", "A", "P.X", "N.Y", "P.Z"]
    assert len(names) == 13 and names != sorted(names)
    rng = np.random.default_rng(5)
    data = rng.standard_normal((5, 7, 13)).astype(F)
    data[0, 0, 6] = np.inf
    path = str(tmp_path / "g.exr")
    amvpt_mod.write_exr_channels(path, data, names)
    back = amvpt_mod.read_exr_channels(path, 7, 5, names)
    assert np.array_equal(bits(back), bits(data))
    # another order of the same names: the same planes, permuted
    perm = [3, 0, 12, 7, 1, 2, 4, 5, 6, 8, 9, 10, 11]
    back2 = amvpt_mod.read_exr_channels(path, 7, 5, [names[i] for i in perm])
    assert np.array_equal(bits(back2), bits(data[..., perm]))
    # the channel list is stored in the byte order of the names
    raw = open(path, "rb").read()
    at = [raw.index(b"\0" + n.encode() + b"\0\x02\0\0\0") for n in sorted(names)]
    assert at == sorted(at)
    with pytest.raises(RuntimeError, match='"depth" is not among|not among the names'):
        amvpt_mod.read_exr_channels(path, 7, 5, names[:-1] + ["depth"])


def test_write_exr_is_the_channel_writer(amvpt_mod, tmp_path):
    rng = np.random.default_rng(6)
    for c, names in ((3, ["R", "G", "B"]), (4, ["R", "G", "B", "A"])):
        img = rng.random((6, 9, c)).astype(F)
        a, b = str(tmp_path / ("a%d.exr" % c)), str(tmp_path / ("b%d.exr" % c))
        amvpt_mod.write_exr(a, img)
        amvpt_mod.write_exr_channels(b, img, names)
        assert open(a, "rb").read() == open(b, "rb").read()
        assert np.array_equal(amvpt_mod.read_exr(a, 9, 6, c), img)


def test_exr_channel_names_are_checked(amvpt_mod, tmp_path):
    data = np.zeros((2, 2, 3), dtype=F)
    path = str(tmp_path / "n.exr")
    with pytest.raises(RuntimeError, match=r'channel 2 repeats the name "Z" of channel 0'):
        amvpt_mod.write_exr_channels(path, data, ["Z", "id", "Z"])
    with pytest.raises(RuntimeError, match=r"channel 1 has an empty name"):
        amvpt_mod.write_exr_channels(path, data, ["Z", "", "id"])
    long = "n" * 32
    with pytest.raises(RuntimeError, match=r'channel 0 \("%s"\) has a name longer than 31 bytes' % long):
        amvpt_mod.write_exr_channels(path, data, [long, "a", "b"])
    assert not os.path.exists(path)
    amvpt_mod.write_exr_channels(path, data, ["n" * 31, "a", "b"])


def test_write_guides_exr(amvpt_mod, grid_hits, tmp_path):
    _, vd, p, hits = grid_hits
    z = amvpt_mod.guide_depth_host(hits, vd, p.n_views)
    img = np.random.default_rng(7).random(hits.shape[:2] + (3,)).astype(F)
    path = str(tmp_path / "frame.exr")
    amvpt_mod.write_guides_exr(path, img, hits, z)
    names = ["R", "G", "B"] + list(amvpt_mod.GUIDE_CHANNELS)
    assert names[3:] == ["Z", "N.X", "N.Y", "N.Z", "P.X", "P.Y", "P.Z", "id", "view"]
    back = amvpt_mod.read_exr_channels(path, hits.shape[1], hits.shape[0], names)
    assert np.array_equal(back[..., :3], img) and np.array_equal(back[..., 3], z)
    assert np.array_equal(back[..., 4:10], hits[..., 1:7])
    assert np.array_equal(back[..., 10], hits[..., 0] + 1) and back[..., 10].min() == 0   # 0 is the background
    assert np.array_equal(back[..., 11], hits[..., 7])

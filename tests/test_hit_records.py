"""The hit-record table of the scene image (dscene.h DHitRec, csrc/scene_image.cpp) on the CPU.

tests/hit_records_driver.cpp builds a scene's image and prints the records beside the tables they are made from,
every float as its bit pattern.  The records are what compute_si reads of a hit, so each must agree with the tables
it replaces: positions and vertex normals equal vpos / vnrm at the face's indices bit for bit, the ids and flags are
the shape's, the geometric normal is unit and orthogonal to both edges, the stored tangent is the UV form or the
coordinate_system fallback.  The exact bits of the computed fields are pinned on the device against the oracle
(test_gpu_hit_records.py); here the bound is 1e-6 relative, a few f32 ulps.  The driver also runs under
AddressSanitizer + UBSan (a stand-alone program, nothing preloaded) and must print the same text.  No test here touches
a device.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, SCENES
from scene_gen import _add, _grid_with_heightfield_xml, _obj_shape, _xml

PKG = os.path.join(REPO, "mitsuba3-amvpt_amd")
DRIVER = os.path.join(PKG, "build", "hit_records_driver")
RECT, TRI, SPHERE = 0, 1, 2
FLIP, NORMALS = 0x100, 0x200
TOL = 1e-6

# two triangles of a tilted quad, written with every combination of vt / vn the loader distinguishes
QUAD = [(-0.3, -0.2, 0.1), (0.4, -0.25, 0.0), (0.35, 0.3, 0.2), (-0.25, 0.35, 0.15)]
QUAD_VN = [(0.1, 0.2, 1.0), (-0.2, 0.1, 0.9), (0.0, -0.1, 1.0), (0.15, 0.0, 0.8)]
QUAD_VT = [(0.0, 0.0), (1.0, 0.1), (0.9, 1.0), (0.05, 0.8)]
DEGENERATE_VT = [(0.0, 0.0), (0.5, 0.5), (1.0, 1.0), (0.25, 0.25)]   # collinear: det == 0 for both triangles


def quad_obj(path, vt=None, vn=None):
    """The quad as OBJ text: f v, f v/vt, f v//vn or f v/vt/vn."""
    with open(path, "w") as out:
        out.write("".join("v %.9g %.9g %.9g\n" % p for p in QUAD))
        if vt:
            out.write("".join("vt %.9g %.9g\n" % t for t in vt))
        if vn:
            out.write("".join("vn %.9g %.9g %.9g\n" % n for n in vn))
        ref = (lambda i: "%d/%d/%d" % (i, i, i)) if vt and vn else (lambda i: "%d/%d" % (i, i)) if vt else \
              (lambda i: "%d//%d" % (i, i)) if vn else (lambda i: "%d" % i)
        for f in ((1, 2, 3), (1, 3, 4)):
            out.write("f %s %s %s\n" % tuple(ref(i) for i in f))
    return path


QUAD_XF = '<rotate x="1" angle="-25"/><rotate y="1" angle="20"/><translate x="0.05" y="-0.1" z="0.3"/>'


def quad_shape(path, face_normals=False, flip=False):
    s = _obj_shape(path, QUAD_XF)
    extra = ('<boolean name="face_normals" value="true"/>' if face_normals else "") + \
            ('<boolean name="flip_normals" value="true"/>' if flip else "")
    return s.replace("<transform", extra + "<transform", 1)


SPHERE_SHAPE = ('<shape type="sphere"><point name="center" x="0.1" y="-0.2" z="0.2"/><float name="radius" value="0.25"/>'
                '<transform name="to_world"><rotate y="1" angle="30"/><translate x="-0.3" y="-0.3" z="0.3"/></transform>'
                '<ref id="green"/></shape>')
FLIPPED_SPHERE = SPHERE_SHAPE.replace('<ref id="green"/>', '<boolean name="flip_normals" value="true"/><ref id="red"/>') \
                             .replace('x="-0.3" y="-0.3" z="0.3"', 'x="0.45" y="0.2" z="0.1"')


def scene_texts(tmp):
    """name -> XML of the generated scenes (shared with the device test): the Cornell box's rectangles and cubes
    plus the shapes under test."""
    grid = _xml("cbox_grid.xml")
    q = lambda name, **kw: quad_obj(str(tmp / (name + ".obj")), **kw)
    return {
        "cube": grid,
        "bare_pair": _add(grid, quad_shape(q("bare"), face_normals=True)),
        "vn_only": _add(grid, quad_shape(q("vn", vn=QUAD_VN))),
        "degenerate_uv": _add(grid, quad_shape(q("deg", vt=DEGENERATE_VT, vn=QUAD_VN))),
        "uv_and_vn": _add(grid, quad_shape(q("full", vt=QUAD_VT, vn=QUAD_VN))),
        "flipped": _add(grid, quad_shape(q("flip", vt=QUAD_VT, vn=QUAD_VN), flip=True) +
                        quad_shape(q("flipbare"), face_normals=True, flip=True).replace('x="0.05"', 'x="-0.5"')),
        "mixed": _add(grid, quad_shape(q("mix", vt=QUAD_VT)) + SPHERE_SHAPE + FLIPPED_SPHERE),
        "heightfield": _grid_with_heightfield_xml(tmp, 8)[0],
    }


def f32(words):
    return np.asarray(words, dtype=np.uint32).view(np.float32)


def run_driver(driver, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([driver, path], capture_output=True, text=True, env=env, timeout=120)


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-s", "-C", PKG, "hit_records_driver", "hit_records_driver_asan"])
    syms = subprocess.run(["nm", DRIVER + "_asan"], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan" in syms, "the sanitized driver is not instrumented"
    return DRIVER, DRIVER + "_asan"


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hit_records")
    paths = {}
    for name, xml in scene_texts(tmp).items():
        paths[name] = str(tmp / (name + ".xml"))
        with open(paths[name], "w") as out:
            out.write(xml)
    paths["veach_grid"] = os.path.join(SCENES, "veach_grid.xml")
    paths["cbox_mesh"] = os.path.join(SCENES, "cbox_mesh.xml")
    return paths


NAMES = ["cube", "bare_pair", "vn_only", "degenerate_uv", "uv_and_vn", "flipped", "mixed", "heightfield", "veach_grid",
         "cbox_mesh"]


@pytest.fixture(scope="module")
def output(drivers, scenes):
    """output(name): the plain driver's text for a scene, run once."""
    cache = {}

    def get(name):
        if name not in cache:
            r = run_driver(drivers[0], scenes[name])
            assert r.returncode == 0, r.stderr
            cache[name] = r.stdout
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_same_text_under_sanitizers(drivers, scenes, output, name):
    r = run_driver(drivers[1], scenes[name])
    assert r.returncode == 0, r.stderr
    assert r.stdout == output(name)


def _unit(v):
    return v / np.sqrt((v.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))


def _coord_s(n):
    """coordinate_system's first vector (vector.h:116-136), in float64."""
    n = n.astype(np.float64)
    sg = np.copysign(1.0, n[2])
    a = -1.0 / (sg + n[2])
    b = n[0] * n[1] * a
    return np.array([np.copysign(1.0, n[2]) * (n[0] * n[0] * a) + 1.0, np.copysign(1.0, n[2]) * b,
                     -np.copysign(1.0, n[2]) * n[0]])


@pytest.mark.parametrize("name", NAMES)
def test_records_agree_with_the_tables(output, name):
    m = json.loads(output(name))
    assert m["hrec_bytes"] == 112 and m["n_hrec"] == max(1, m["n_prims"]) == max(1, len(m["prims"]))
    rec = np.asarray(m["hrec"], dtype=np.int64)
    assert rec.shape == (m["n_prims"], 4 + 24)
    rows = rec[:, 4:].astype(np.uint32).reshape(-1, 6, 4)
    vpos = np.asarray(m["vpos"], dtype=np.uint32).reshape(-1, 3)
    vnrm = np.asarray(m["vnrm"], dtype=np.uint32).reshape(-1, 3)
    vuv = f32(m["vuv"]).reshape(-1, 2)
    seen = set()
    for i, (ptype, shape, i0, i1, i2) in enumerate(m["prims"]):
        s = m["shapes"][shape]
        kind, rshape, bsdf, emitter = (int(v) for v in rec[i, :4])
        assert kind & 0xff == ptype and rshape == shape
        assert (bsdf, emitter) == (s["bsdf"], s["emitter"])
        assert bool(kind & FLIP) == bool(s["flip"]) and kind & ~(0xff | FLIP | NORMALS) == 0
        r = rows[i]
        fr = r.view(np.float32)
        if ptype == RECT:
            assert kind & NORMALS == 0
            assert r[0, :3].tolist() == [s["to_world"][3], s["to_world"][7], s["to_world"][11]]
            assert r[1, :3].tolist() == s["frame_n"] and r[2, :3].tolist() == s["frame_s"]
            assert not r[3:].any() and not r[:3, 3].any()
            n = fr[1, :3].astype(np.float64)
            assert abs(np.dot(n, n) - 1.0) <= 2 * TOL
            # the stored frame: frame_n is orthogonal to frame_s (the shading frame's s is frame_s made orthonormal)
            fs = fr[2, :3].astype(np.float64)
            assert abs(np.dot(n, fs)) <= TOL * np.linalg.norm(fs)
        elif ptype == TRI:
            idx = [i0, i1, i2]
            assert bool(kind & NORMALS) == bool(s["has_normals"])
            for v in range(3):
                assert r[v, :3].tolist() == vpos[idx[v]].tolist()
                want = vnrm[idx[v]].tolist() if s["has_normals"] else [0, 0, 0]
                assert r[3 + v, :3].tolist() == want
            p = fr[:3, :3].astype(np.float64)
            e1, e2 = p[1] - p[0], p[2] - p[0]
            n = fr[:3, 3].astype(np.float64)
            assert abs(np.dot(n, n) - 1.0) <= 2 * TOL
            assert abs(np.dot(n, e1)) <= TOL * np.linalg.norm(e1) and abs(np.dot(n, e2)) <= TOL * np.linalg.norm(e2)
            geo = _unit(np.cross(e1, e2))
            assert np.abs(n - (-geo if s["flip"] else geo)).max() <= 4 * TOL   # the side the winding gives, flipped or not
            dp_du = fr[3:, 3].astype(np.float64)
            unflipped = -n if s["flip"] else n
            det = 0.0
            if s["has_uv"]:
                # the f32 determinant as the build forms it: fma(d0x, d1y, -(d0y * d1x)) of f32 differences
                d0, d1 = (vuv[i1] - vuv[i0]).astype(np.float64), (vuv[i2] - vuv[i0]).astype(np.float64)
                det = float(np.float32(d0[0] * d1[1] - float(np.float32(d0[1] * d1[0]))))
            if s["has_uv"] and det != 0.0:
                want = (d1[1] * e1 - d0[1] * e2) / det
                scale = (abs(d1[1]) * np.abs(e1) + abs(d0[1]) * np.abs(e2)).max() / abs(det)
                assert np.abs(dp_du - want).max() <= 4 * TOL * scale
                seen.add("uv")
            else:
                want = _coord_s(fr[:3, 3] * (-1 if s["flip"] else 1))
                assert np.abs(dp_du - want).max() <= 4 * TOL
                assert abs(np.dot(dp_du, dp_du) - 1.0) <= 4 * TOL and abs(np.dot(dp_du, unflipped)) <= 4 * TOL
                seen.add("fallback_uv" if s["has_uv"] else "fallback")
            seen.add("normals" if s["has_normals"] else "flat")
            if s["flip"]:
                seen.add("flip")
        else:
            assert ptype == SPHERE and kind & NORMALS == 0
            assert r[0].tolist() == s["center"] + s["radius"]
            assert r[1].tolist() == s["to_object"][0:4] and r[2].tolist() == s["to_object"][4:8]
            for k in range(3):
                assert r[3 + k, :3].tolist() == s["to_world"][4 * k:4 * k + 3] and r[3 + k, 3] == 0
            seen.add("sphere_flip" if s["flip"] else "sphere")
    want_seen = {"cube": {"uv", "normals"}, "bare_pair": {"fallback", "flat"}, "vn_only": {"fallback", "normals"},
                 "degenerate_uv": {"fallback_uv"}, "uv_and_vn": {"uv"}, "flipped": {"flip", "flat", "normals"},
                 "mixed": {"sphere", "sphere_flip", "uv"}, "heightfield": {"fallback"}, "veach_grid": {"sphere"},
                 "cbox_mesh": {"normals"}}[name]
    assert want_seen <= seen, "the scene does not reach %s" % sorted(want_seen - seen)

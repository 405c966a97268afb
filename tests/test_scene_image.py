"""The scene image build (csrc/scene_image.cpp) on the CPU: byte identity with the recorded images, the structural
facts in words, and a clean run under AddressSanitizer + UBSan.

tests/scene_image_driver.cpp loads a scene with the host framework, calls build_scene_image and prints, per uploaded
table, its element count and the FNV-1a digest of its bytes, then every scalar of the image.  The expectation,
tests/golden/scene_image.json, was recorded from the commit before the build moved out of amvpt_scene_create (DESIGN.md
section 4 says how), so a case that fails here means that the tables a device would receive have changed.  There is no
tolerance.  No test here touches a device.
"""
import json
import os
import re
import subprocess

import pytest

from conftest import REPO, SCENES
from scene_gen import (_add, _extra_rects, _grid_with_heightfield_xml, _heightfield_obj, _heightfield_room_xml,
                       _obj_shape, _triangle_obj, _xml)

PKG = os.path.join(REPO, "mitsuba3-amvpt_amd")
DRIVER = os.path.join(PKG, "build", "scene_image_driver")
GOLDEN = os.path.join(REPO, "tests", "golden", "scene_image.json")
STOCK = ["cbox_batch", "cbox_cone", "cbox_cubelight_rects", "cbox_env", "cbox_grid", "cbox_meshlight", "cbox_mesh",
         "cbox_path", "veach_grid"]
UNIFORM_NODES, LDS_SCENE_BYTES, STACK2, OUTER_MAX, BRUTE_PRIMS = 255, 48 * 1024, 16, 8, 48


def _file(tmp, name, xml):
    path = str(tmp / (name + ".xml"))
    with open(path, "w") as out:
        out.write(xml)
    return path


def _plain_heightfield(tmp, n):
    """The Cornell box's rectangles (kept outside the BVH) and an n x n heightfield: the BVH is the heightfield's."""
    xml = re.sub(r'<shape type="cube".*?</shape>', "", _xml("cbox_grid.xml"), flags=re.S)
    obj = str(tmp / ("heightfield_%d.obj" % n))
    _heightfield_obj(obj, n)
    return _add(xml, _obj_shape(obj, '<scale value="1.6"/><rotate x="1" angle="-90"/><translate y="-0.8"/>'))


def _one_cube_on_ground(width):
    """cbox_grid.xml without its large box, plus a ground rectangle `width` units wide."""
    xml, k = re.subn(r'<shape type="cube" id="large-box">.*?</shape>', "", _xml("cbox_grid.xml"), flags=re.S)
    assert k == 1
    return _add(xml, '<shape type="rectangle"><transform name="to_world"><scale value="%g"/><rotate x="1" angle="-90"/>'
                     '<translate y="-1.01"/></transform><ref id="white"/></shape>' % (0.5 * width))


def _bare_mesh_first(tmp):
    """cbox_mesh.xml with a triangle that has neither vertex normals nor uvs in front of its two meshes."""
    tri = str(tmp / "triangle.obj")
    _triangle_obj(tri)
    bare = _obj_shape(tri, '<translate x="-0.5" y="0.2"/>').replace(
        "<transform", '<boolean name="face_normals" value="true"/><transform', 1)
    marker = '<shape type="obj" id="ball">'
    xml = _xml("cbox_mesh.xml")
    assert marker in xml
    return xml.replace(marker, bare + marker)


NODES_N, NODES_COST, NODES_COST_ABOVE = 20, 4.75, 4.5

# name -> builder(tmp directory) -> the driver's arguments
CASES = {name: (lambda tmp, name=name: [os.path.join(SCENES, name + ".xml")]) for name in STOCK}
CASES.update({
    "empty": lambda tmp: ["empty"],
    "grid_8_rects": lambda tmp: [_file(tmp, "r8", _add(_xml("cbox_grid.xml"), _extra_rects(2)))],
    "grid_9_rects": lambda tmp: [_file(tmp, "r9", _add(_xml("cbox_grid.xml"), _extra_rects(3)))],
    # 48 KiB either side, to the record (test_gpu_bvh_walks.test_staging_threshold): 49056 / 49184 bytes
    "lds_below": lambda tmp: [_file(tmp, "l31", _grid_with_heightfield_xml(tmp, 15, loose=31)[0])],
    "lds_above": lambda tmp: [_file(tmp, "l32", _grid_with_heightfield_xml(tmp, 15, loose=32)[0])],
    # kUniformNodeLimit either side with more than 48 KiB on both: one heightfield, leaves of up to 15 primitives, and
    # a traversal cost that gives exactly 255 nodes against one that gives 267
    "nodes_below": lambda tmp: [_file(tmp, "nb", _plain_heightfield(tmp, NODES_N)), "leaf=15", "cost=%g" % NODES_COST],
    "nodes_above": lambda tmp: [_file(tmp, "na", _plain_heightfield(tmp, NODES_N)), "leaf=15", "cost=%g" % NODES_COST_ABOVE],
    "depth_16": lambda tmp: [_file(tmp, "d16", _heightfield_room_xml(tmp, 128)[0])],
    "depth_17": lambda tmp: [_file(tmp, "d17", _heightfield_room_xml(tmp, 200)[0])],
    "leaf_15": lambda tmp: [os.path.join(SCENES, "cbox_mesh.xml"), "leaf=15", "cost=8"],
    "cube_narrow_ground": lambda tmp: [_file(tmp, "g2", _one_cube_on_ground(4.0))],
    "cube_wide_ground": lambda tmp: [_file(tmp, "g1000", _one_cube_on_ground(1000.0))],
    "bare_mesh_first": lambda tmp: [_file(tmp, "bare", _bare_mesh_first(tmp))],
})


def run_driver(driver, args):
    """One driver run: (exit status, parsed JSON or None, stderr)."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver] + args, capture_output=True, text=True, env=env, timeout=120)
    return r.returncode, json.loads(r.stdout) if r.returncode == 0 else None, r.stderr


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-s", "-C", PKG, "scene_image_driver", "scene_image_driver_asan"])
    syms = subprocess.run(["nm", DRIVER + "_asan"], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan" in syms, "the sanitized driver is not instrumented"
    return DRIVER, DRIVER + "_asan"


@pytest.fixture(scope="module")
def case_args(tmp_path_factory):
    """case_args(name): the driver's arguments for a case, its scene and mesh files written once."""
    tmp, cache = tmp_path_factory.mktemp("scene_image"), {}

    def get(name):
        if name not in cache:
            cache[name] = CASES[name](tmp)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def image(drivers, case_args):
    """image(name): the plain driver's JSON of a case, built once."""
    cache = {}

    def get(name):
        if name not in cache:
            status, cache[name], err = run_driver(drivers[0], case_args(name))
            assert status == 0, err
        return cache[name]
    return get


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_image_is_the_recorded_one(image, golden, name):
    got, want = image(name), golden[name]
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, "\n".join("%s: %r, recorded %r" % (k, got[k], want[k]) for k in differ)


@pytest.mark.parametrize("name", sorted(CASES))
def test_clean_under_sanitizers(drivers, case_args, golden, name):
    status, got, err = run_driver(drivers[1], case_args(name))
    assert status == 0, err
    assert got == golden[name]


# ---- the structural facts, in words --------------------------------------------------------------------------------

def _staged_bytes(m):
    return m["n_nodes"] * 32 + m["n_prims"] * 64


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_image_is_consistent(image, name):
    m = image(name)
    assert m["dev.pointers_null"] == 1
    for key in ("n_nodes", "n_sph", "n_outer", "n_boxes", "n_nodes2"):
        assert m[key] == m["dev." + key], key
    assert m["dev.n_prims"] == max(1, m["n_prims"]) == m["prims"][0]
    assert m["dev.lds_bytes"] == m["n_nodes"] * 32 + m["dev.n_prims"] * 64
    assert m["nodes"][0] == (8 if m["dev.oct_stride"] else 1) * m["n_nodes"]
    assert m["dev.oct_stride"] in (0, m["n_nodes"])
    # a BVH is wave-uniform, staged, or has the octant copies; the two-box tree comes with the copies unless too deep
    device_memory = m["n_nodes"] > UNIFORM_NODES and _staged_bytes(m) > LDS_SCENE_BYTES
    assert (m["dev.oct_stride"] != 0) == device_memory
    assert (m["n_nodes2"] != 0) == (device_memory and m["bvh2_depth"] <= STACK2)
    assert m["nodes2"][0] == m["nodes2h"][0] == max(1, m["n_nodes2"])
    assert m["n_outer"] <= OUTER_MAX and m["outer"][0] == max(1, m["n_outer"])
    assert m["sph_prims"][0] == max(1, m["n_sph"]) and m["has_spheres"] == (m["n_sph"] > 0)
    assert m["checks"]["sphere_ordinals"] == list(range(m["n_sph"]))
    assert m["boxes"][0] == max(1, m["n_boxes"]) and m["box_prims"][0] == max(1, 12 * m["n_boxes"])
    if m["n_prims"] > BRUTE_PRIMS:
        assert m["n_boxes"] == 0 and m["dev.n_loose"] == 0
    else:
        assert m["dev.n_loose"] + 12 * m["n_boxes"] == m["dev.n_prims"]
    assert sum(m["checks"]["leaf_sizes"]) * 2 - 1 == m["n_nodes"] or m["n_prims"] == m["n_outer"]


def test_no_shapes_gives_the_empty_root(image):
    m = image("empty")
    assert (m["n_nodes"], m["n_prims"], m["n_outer"], m["n_boxes"], m["n_nodes2"]) == (1, 0, 0, 0, 0)
    assert m["root_lo"] == [1, 1, 1] and m["root_hi"] == [-1, -1, -1]      # a box no ray enters
    assert sum(m["checks"]["leaf_sizes"]) == 0 and not m["bvh_tri_only"] and not m["all_diffuse"]
    assert m["dev.tab_bytes"] == 0 and m["dev.emitter_pmf"] == [0]


def test_nine_rectangles_enter_the_tree(image):
    r8, r9 = image("grid_8_rects"), image("grid_9_rects")
    assert (r8["n_outer"], r8["checks"]["rects_in_leaves"], r8["bvh_tri_only"]) == (8, 0, 1)
    assert (r9["n_outer"], r9["checks"]["rects_in_leaves"], r9["bvh_tri_only"]) == (0, 9, 0)
    assert r9["n_prims"] == r8["n_prims"] + 1 and r9["n_nodes"] > r8["n_nodes"] + 8


def test_staging_threshold(image):
    below, above = image("lds_below"), image("lds_above")
    assert (_staged_bytes(below), _staged_bytes(above)) == (49056, 49184)
    for m in (below, above):
        assert m["n_nodes"] > UNIFORM_NODES and m["n_outer"] == 6
    assert (below["dev.oct_stride"], below["n_nodes2"], below["bvh2_depth"]) == (0, 0, 0)
    assert above["dev.oct_stride"] == above["n_nodes"] and above["nodes"][0] == 8 * above["n_nodes"]
    assert above["n_nodes2"] > 0 and 0 < above["bvh2_depth"] <= STACK2


def test_uniform_node_limit(image):
    below, above = image("nodes_below"), image("nodes_above")
    for m in (below, above):
        assert _staged_bytes(m) > LDS_SCENE_BYTES and m["n_prims"] == 6 + 2 * NODES_N * NODES_N
    assert below["n_nodes"] == UNIFORM_NODES < above["n_nodes"] < UNIFORM_NODES + 16
    assert (below["dev.oct_stride"], below["n_nodes2"]) == (0, 0)
    assert above["dev.oct_stride"] == above["n_nodes"] and above["nodes"][0] == 8 * above["n_nodes"]
    assert above["n_nodes2"] > 0


def test_two_box_depth_against_the_stack(image):
    d16, d17 = image("depth_16"), image("depth_17")
    assert d16["n_prims"] == 6 + 32768 and d17["n_prims"] == 6 + 80000
    assert d16["n_nodes2"] > 0 and d16["bvh2_depth"] == 16
    assert (d17["n_nodes2"], d17["bvh2_depth"]) == (0, 17)
    assert d17["dev.oct_stride"] == d17["n_nodes"] > 20000        # the threaded walks keep their octant copies


def test_wide_leaves(image):
    narrow, wide = image("cbox_mesh"), image("leaf_15")
    assert narrow["checks"]["leaf_sizes"][4:] == [0] * 11         # the default build: at most 4 primitives
    assert wide["checks"]["leaf_sizes"][14] > 0                   # leaves of 15: the whole 4-bit count field
    assert wide["n_prims"] == narrow["n_prims"] and 2 * wide["n_nodes"] < narrow["n_nodes"]
    assert wide["n_nodes2"] > 0 and 0 < wide["bvh2_depth"] <= STACK2


def test_boxes_found_and_refused(image):
    assert image("cbox_grid")["n_boxes"] == 2 and image("cbox_grid")["dev.n_loose"] == 6
    # eleven rectangles and two file meshes: past the brute-force limit, so the scene keeps no box list
    rects = image("cbox_cubelight_rects")
    assert rects["n_prims"] > BRUTE_PRIMS and rects["n_boxes"] == 0 and rects["checks"]["rects_in_leaves"] == 11
    narrow, wide = image("cube_narrow_ground"), image("cube_wide_ground")
    assert narrow["n_prims"] == wide["n_prims"] == 7 + 12
    assert narrow["n_boxes"] == 1 and (narrow["dev.n_loose"], narrow["dev.n_loose_rect"]) == (7, 7)
    assert wide["n_boxes"] == 0 and (wide["dev.n_loose"], wide["dev.n_loose_tri"]) == (19, 12)   # conditioning


def test_sphere_ordinals_follow_sph_prims(image):
    m = image("veach_grid")
    assert m["n_sph"] > 0 and m["checks"]["sphere_ordinals"] == list(range(m["n_sph"]))


def test_missing_streams_are_zero_padded(image):
    meshes = image("bare_mesh_first")["checks"]["meshes"]
    bare, ball, ring = meshes
    assert (bare["vertices"], bare["faces"], bare["has_normals"], bare["has_uv"]) == (3, 1, 0, 0)
    assert bare["normals_zero"] and bare["uv_zero"]
    assert ball["has_normals"] and ball["has_uv"] and not ball["normals_zero"] and not ball["uv_zero"]
    assert ring["has_normals"] and not ring["has_uv"] and ring["uv_zero"]        # padded behind the last uv, too
    m = image("bare_mesh_first")
    assert m["vnrm"][0] == m["vpos"][0] and 3 * m["vuv"][0] == 2 * m["vpos"][0]

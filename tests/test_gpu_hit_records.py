"""compute_si on the device reads the per-primitive hit records (dscene.h DHitRec): every caller against the oracle.

The oracle forms a hit's position, normals and tangent from the vertex streams, per hit; the device reads what the
host computed once per primitive.  Lane records must agree bit for bit.  Each scene renders three ways so that every
caller of compute_si runs: the default (the fused primary vertex where the scene allows it, k_suffix_fused),
AMVPT_OPT_SPLIT_PRIMARY (k_prim_hit_req and the split k_mv_primary) and AMVPT_OPT_WAVEFRONT_SUFFIX (k_bounce); one
amvpt_guides call covers k_guides.  The scenes are test_hit_records.py's: each reaches one branch of the record build
(UV tangent, the coordinate_system fallback with and without UVs, vertex normals or none, flipped shapes, spheres, the
BVH tier).  2 x 1 views of 32 x 32 pixels, 16 spp in one pass, max_depth 4: 32768 lanes a frame.
"""
import numpy as np
import pytest

from test_gpu_fused_primary import _bit_equal, _render
from test_guides import bits
from test_hit_records import scene_texts

pytestmark = pytest.mark.gpu

DEFINES = dict(res=32, gx=2, gy=1, reuse=2, spp=16, spp_pass_lim=16, max_depth=4)
SCENE_NAMES = ["cube", "bare_pair", "vn_only", "degenerate_uv", "flipped", "mixed", "heightfield"]
BRUTE_PRIMS = 48


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    return scene_texts(tmp_path_factory.mktemp("gpu_hit_records"))


@pytest.fixture(scope="module")
def case(amvpt_mod, oracle, texts):
    """case(name): (scene, the oracle's lane records of pass 0), rendered once per scene."""
    cache = {}

    def get(name):
        if name not in cache:
            s = amvpt_mod.load_string(texts[name], **DEFINES)
            sd, vd, p = s.describe(0, 0, 0)
            plan = oracle.plan(p)
            assert (p.n_views, p.film_width, p.film_height, plan["lanes"]) == (2, 64, 32, 32768)
            _, orec, _ = oracle.render(sd, vd, p, threads=16, record_pass=0)
            cache[name] = (s, orec)
        return cache[name]
    return get


def _flags(amvpt_mod, way):
    return {"default": 0, "split_primary": amvpt_mod.OPT_SPLIT_PRIMARY, "wavefront_suffix": amvpt_mod.OPT_WAVEFRONT_SUFFIX}[way]


@pytest.mark.parametrize("way", ["default", "split_primary", "wavefront_suffix"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_records_equal_the_oracle(gpu_ready, amvpt_mod, oracle, case, name, way):
    s, orec = case(name)
    _, grec, c = _render(amvpt_mod, oracle, s, _flags(amvpt_mod, way))
    launches = c["kernel_launches"]
    print(name, way, {k: v for k, v in launches.items() if v})
    if way == "split_primary":
        assert launches["k_prim_hit"] > 0 and launches["k_vis"] > 0
    eq = _bit_equal(grec, orec).all(axis=(1, 2))
    if not eq.all():
        for lane in np.flatnonzero(~eq)[:3]:
            print("lane", lane, "\ngpu   ", grec[lane], "\noracle", orec[lane])
    assert eq.all(), "%d of %d lanes differ from the oracle" % ((~eq).sum(), eq.size)
    assert c["vertices"] > c["lanes"] == 32768        # the suffix ran: vertices past the primary one


def test_the_scenes_reach_their_tiers(gpu_ready, amvpt_mod, oracle, case):
    """The brute-force tier for all but the heightfield, every shape seen by primary rays; the mixed scene's primary
    hits put a rectangle, a mesh triangle and a sphere into one wave (64 consecutive pixels of a view: two rows)."""
    for name in SCENE_NAMES:
        sd, vd, p = case(name)[0].describe(0, 0, 0)
        n_prims = amvpt_mod.DeviceScene(sd).stats()[1]
        assert (n_prims > BRUTE_PRIMS) == (name == "heightfield"), (name, n_prims)
        seen = set(np.unique(oracle.primary_hits(sd, vd, p)[..., 0]).astype(int).tolist())
        assert seen >= set(range(sd.contents.shape_count)), "%s: primary rays miss shapes %s" % (
            name, sorted(set(range(sd.contents.shape_count)) - seen))
    s, _ = case("mixed")
    sd, vd, p = s.describe(0, 0, 0)
    shape = oracle.primary_hits(sd, vd, p)[:, :32, 0].astype(int)      # view 0
    types = np.array([sd.contents.shapes[i].type for i in range(sd.contents.shape_count)])
    waves = np.where(shape >= 0, types[np.maximum(shape, 0)], -1).reshape(16, 64)
    assert any(set(w.tolist()) >= {0, 1, 2} for w in waves), "no wave of view 0 sees all three shape types"


def test_guides_on_the_cube_scene(gpu_ready, amvpt_mod, oracle, case):
    """k_guides: primary shapes, geometric normals and positions of the cube scene (UVs and vertex normals)."""
    import torch
    s, _ = case("cube")
    sd, vd, p = s.describe(0, 0, 0)
    ref = oracle.primary_hits(sd, vd, p)
    out = torch.zeros((p.film_height, p.film_width, 8), dtype=torch.float32, device="cuda")
    amvpt_mod.DeviceScene(sd).guides(vd, p, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    eq = (bits(got) == bits(ref)).all(axis=-1)
    assert eq.all(), "guide records: %d of %d pixels differ from the oracle" % ((~eq).sum(), eq.size)
    mesh = [i for i in range(sd.contents.shape_count) if sd.contents.shapes[i].type == 1]
    assert np.isin(got[..., 0], mesh).sum() > 100

"""The HIP pipeline against closed-form radiometry (tests/radiometry.py) -- the cases of tests/test_radiometry.py
through amvpt.render(scene, seed=k, raw=True) at 32^2 pixels per view, 16 frames and 512 to 1024 spp: about 1e7
samples per case, a relative standard error of the frame mean near 1e-4.  The device is pinned to the oracle bit for
bit elsewhere; here both are held to answers neither of them produced.

Gate: pooled ratio of means over the frames, |ratio - 1| < 4 SE + 2e-4 (the conductor furnace: + the measured floor
of radiometry.PLATE_MEASURED instead of 2e-4); on the floor also the per-pixel Sidak Z-gate; every gate must reject a
1 % error.  Each case prints its ratio, SE and z.

Record parity on three scenes no other GPU test reaches: the flipped emitting cube (a mesh emitter with flipped
normals), a flipped emitting sphere seen from inside (the inside branch of sphere sampling, DShape.flip) and two
lights of unequal sampling_weight with an environment.  The sphere enclosure has parity only: the reference prices
emitter hits from points ON a sphere with the cone density while it samples them by area (sphere.cpp:242-245 against
:316-319), which reads 0.2 to 1.3 % high.
"""
import pytest

import radiometry as R
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu

# the adaptive cases take one pass of 32 x 32 x 8 x 256 lanes, the size of the C5 shape's passes
SIZES = dict(K=16, res=32, spp_path=1024, spp_mvpath=512, spp_adaptive=256)


@pytest.fixture(scope="module")
def backend(gpu_ready, amvpt_mod, oracle):
    last = {}

    def scene(xml):
        if last.get("xml") != xml:
            last["xml"], last["scene"] = xml, amvpt_mod.load_string(xml)
        return last["scene"]

    def render(xml, seed):
        return amvpt_mod.render(scene(xml), seed=seed, raw=True)

    def hits(xml):
        sd, vd, p = scene(xml).describe(0, 0, 0)
        return oracle.primary_hits(sd, vd, p)   # scene geometry only
    return "hip", render, hits


@pytest.mark.parametrize("case", R.enclosure_cases(), ids=[c["id"] for c in R.enclosure_cases()])
def test_enclosure(backend, case):
    R.check_enclosure(backend, case, SIZES)


@pytest.mark.parametrize("case", R.floor_cases(), ids=[c["id"] for c in R.floor_cases()])
def test_floor(backend, case):
    R.check_floor(backend, case, SIZES)


def test_furnace_diffuse_sphere(backend):
    R.check_furnace_sphere(backend, SIZES)


@pytest.mark.parametrize("case", R.plate_cases(), ids=[c["id"] for c in R.plate_cases()])
def test_furnace_rough_conductor(backend, case):
    R.check_plate(backend, case, SIZES)


@pytest.mark.parametrize("family,case_id", R.POWER_CASES, ids=[c[1] for c in R.POWER_CASES])
def test_gate_rejects_one_percent(backend, family, case_id):
    R.check_power(backend, family, case_id, SIZES)


PARITY = {
    "flipped_cube": R.enclosure_shapes("cube"),
    "flipped_sphere_inside": R.enclosure_shapes("sphere"),
    "two_weight_lights": R.floor_shapes(sphere=0.2, rect=3.0, env=R.ENV_RADIANCE),
}


@pytest.mark.parametrize("integrator,grid", [("path", None), ("mvpath", (2, 2, 4))], ids=["path", "mvpath_g4"])
@pytest.mark.parametrize("name", list(PARITY))
def test_record_parity(gpu_ready, amvpt_mod, oracle, name, integrator, grid):
    """lane records bit-identical to the oracle's, film to float summation order (test_gpu_parity._check)"""
    camera = R.FLOOR_CAMERA if name == "two_weight_lights" else R.ENCLOSURE_CAMERA
    depth = 2 if name == "two_weight_lights" else 6
    xml = R.scene_xml(PARITY[name], integrator, depth, 5, res=16, spp=16, grid=grid, cam_dist=0.1, **camera)
    s = amvpt_mod.load_string(xml)
    sd, vd, p = s.describe(0, 0, 0)
    assert sd.contents.shape_count == (3 if name == "two_weight_lights" else 1)
    if name == "flipped_sphere_inside":
        assert sd.contents.shapes[0].flip_normals == 1 and abs(sd.contents.shapes[0].radius - 2.0) < 1e-6
    _check(amvpt_mod, oracle, s)

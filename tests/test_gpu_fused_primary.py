"""The fused primary vertex (k_mv_primary's kFuse instance) against the three-launch path.

Sphere-free all-diffuse scenes walked wave-uniformly run the whole primary vertex in one launch: the lane traces
its closest hit, the emitter sample's shadow ray and each view's visibility ray itself.  AMVPT_OPT_SPLIT_PRIMARY
keeps k_prim_hit_req -> k_vis -> k_mv_primary.  Both evaluate the same functions on the same values, so lane
records, counters and the deterministic film are bit-identical; the oracle bar is test_gpu_parity's (records 1.0
bit-identical, film 1e-5 of its scale).  Sizes are chosen so every case runs in seconds.
"""
import os

import numpy as np
import pytest

from conftest import SCENES

pytestmark = pytest.mark.gpu

CBOX = os.path.join(SCENES, "cbox_grid.xml")
COUNTERS = ("lanes", "vertices", "reuse_lanes", "visibility_rays", "view_splats", "pushed_paths")


def _bit_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _render(amvpt_mod, oracle, scene, flags=0, lane_begin=0, lane_end=None, chunk_lanes=None, traversal=None):
    """One instrumented frame through amvpt_render_ex: (film, records of pass 0, counters)."""
    import torch
    assert torch.cuda.is_available()
    sd, vd, p = scene.describe(0, 0, 0)
    plan = oracle.plan(p)
    lane_end = plan["lanes"] if lane_end is None else lane_end
    dev = amvpt_mod.DeviceScene(sd)
    film = torch.zeros((p.film_height, p.film_width, 5 if p.film_alpha else 4), dtype=torch.float32, device="cuda")
    rec = torch.zeros((lane_end - lane_begin, plan["group"], 8), dtype=torch.float32, device="cuda")
    cnt = amvpt_mod.Counters()
    dev.render_ex(vd, p, film.data_ptr(), lanes=amvpt_mod.LaneSet(lane_begin, lane_end, 0, 0, 0, 0), flags=flags,
                  records_ptr=rec.data_ptr(), counters=cnt, chunk_lanes=chunk_lanes, traversal=traversal)
    torch.cuda.synchronize()
    return film.cpu().numpy(), rec.cpu().numpy(), cnt.as_dict()


def _check_oracle(amvpt_mod, oracle, scene, grec, gfilm):
    """test_gpu_parity._check's bar on a frame already rendered."""
    sd, vd, p = scene.describe(0, 0, 0)
    ofilm, orec, _ = oracle.render(sd, vd, p, threads=16, record_pass=0)
    match = _bit_equal(grec, orec).all(axis=(1, 2)).mean()
    assert match >= 1.0, "lane records: %.6f bit-identical" % match
    err = np.abs(gfilm - ofilm).max() / np.abs(ofilm).max()
    assert err < 1e-5, "film max relative difference %.3e" % err


CASES = {
    # the bench's config-M shape (8 views, G = 8) at reduced size
    "m_shape": (dict(res=64, spp=16, gx=4, gy=2, reuse=8), dict()),
    # the same shape at a size the oracle renders in seconds
    "m_shape_small": (dict(res=24, spp=16, gx=4, gy=2, reuse=8), dict()),
    # the scene's defaults: 4 views, G = 4
    "g4": (dict(res=48, spp=16), dict()),
    "g2": (dict(res=32, spp=16, reuse=2), dict()),
    # 3 x 1 views of 5 x 5 px at 16 spp: 1200 lanes, a partial last block (128) and last wave (64)
    "ragged_1200": (dict(res=5, spp=16, gx=3, gy=1, reuse=3), dict()),
    # no MIS: the second loop over the views that reads the verdicts
    "no_mis": (dict(res=48, spp=16, sa_mis="false"), dict()),
    # thin lens: the visibility rays' targets depend on the lane's aperture draw
    "thinlens": (dict(res=24, spp=16, gx=4, gy=2, reuse=8, cam="thinlens", aperture="0.05"), dict()),
    # no walk at all / no suffix push
    "depth0": (dict(res=32, spp=16, max_depth=0), dict()),
    # max_depth 1 is not "emission only" in mvpath: the primary vertex's emitter sample is added whatever the depth
    # limit (mvpath_multi.h:248-267; :531 gates the suffix alone), while the fill's sample_single honours it.  A
    # uniform enclosure reads Le (1 + c rho / (n_adapt + 1)) with c ~ 0.34, not Le: a property of the reference,
    # which is why tests/radiometry.py has no closed form for this depth
    "depth1": (dict(res=32, spp=16, max_depth=1), dict()),
    # a lane range with neither end on a wave boundary
    "lane_range": (dict(res=48, spp=16), dict(lane_begin=1003, lane_end=20021)),
    # several chunks with a ragged last one (36864 lanes)
    "chunks_5000": (dict(res=48, spp=16), dict(chunk_lanes=5000)),
}
ORACLE_CASES = ("m_shape_small", "thinlens")


@pytest.mark.parametrize("case", list(CASES))
def test_fused_primary_equals_split(gpu_ready, amvpt_mod, oracle, case):
    defines, kw = CASES[case]
    s = amvpt_mod.load_file(CBOX, **defines)
    if case == "ragged_1200":
        assert oracle.plan(s.describe(0, 0, 0)[2])["lanes"] == 1200
    ffilm, frec, fc = _render(amvpt_mod, oracle, s, 0, **kw)
    sfilm, srec, sc = _render(amvpt_mod, oracle, s, amvpt_mod.OPT_SPLIT_PRIMARY, **kw)
    assert fc["kernel_launches"]["k_vis"] == 0 and fc["kernel_launches"]["k_prim_hit"] == 0
    assert fc["kernel_launches"]["k_mv_primary"] > 0
    assert sc["kernel_launches"]["k_vis"] > 0 and sc["kernel_launches"]["k_prim_hit"] > 0
    eq = _bit_equal(frec, srec).all(axis=(1, 2))
    assert eq.all(), "%d of %d lanes differ from the split path" % ((~eq).sum(), eq.size)
    for k in COUNTERS:
        assert fc[k] == sc[k], (k, fc[k], sc[k])
    if case in ("chunks_5000",):
        assert fc["kernel_launches"]["k_mv_primary"] > 1
    if case in ORACLE_CASES:
        _check_oracle(amvpt_mod, oracle, s, frec, ffilm)


def test_fused_primary_deterministic_film(gpu_ready, amvpt_mod, oracle):
    """AMVPT_OPT_DETERMINISTIC: the fixed-point film does not depend on the order of the adds, so the fused and the
    split frame are the same floats."""
    s = amvpt_mod.load_file(CBOX, res=32, spp=16, gx=4, gy=2, reuse=8)
    det = amvpt_mod.OPT_DETERMINISTIC
    ffilm, frec, fc = _render(amvpt_mod, oracle, s, det)
    sfilm, srec, sc = _render(amvpt_mod, oracle, s, det | amvpt_mod.OPT_SPLIT_PRIMARY)
    assert fc["kernel_launches"]["k_vis"] == 0 and sc["kernel_launches"]["k_vis"] > 0
    assert np.abs(ffilm).max() > 0
    assert _bit_equal(ffilm, sfilm).all(), "%d film floats differ" % (~_bit_equal(ffilm, sfilm)).sum()
    assert _bit_equal(frec, srec).all()


@pytest.mark.parametrize("kw", [dict(traversal=2), dict(flags=1)], ids=["per_lane_traversal", "generic_kernels"])
def test_other_paths_keep_three_launches(gpu_ready, amvpt_mod, oracle, kw):
    """Per-lane traversal and the generic kernel instances (AMVPT_OPT_GENERIC_KERNELS) do not take the fused
    vertex: k_vis still runs, and the frame meets the oracle bar."""
    assert amvpt_mod.OPT_GENERIC_KERNELS == 1
    s = amvpt_mod.load_file(CBOX, res=32, spp=16, gx=4, gy=2, reuse=8)
    film, rec, c = _render(amvpt_mod, oracle, s, **kw)
    assert c["kernel_launches"]["k_vis"] > 0 and c["kernel_launches"]["k_prim_hit"] > 0
    _check_oracle(amvpt_mod, oracle, s, rec, film)

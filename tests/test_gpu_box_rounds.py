"""The brute-force walks' pooled face rounds (dgeom.h box_rounds / box_walk): one round loop over the candidate
faces of two box meshes at a time, an odd last box alone.

The hit does not depend on the order of the face tests -- closest hit follows the (t, scene-order index) rule, any
hit is a disjunction -- so for every scene the lane records must equal, bit for bit,
  * the full scan's (AMVPT_OPT_NO_BOX_SCREEN: no box_walk at all),
  * the per-depth wavefront suffix's, with NEE inside k_bounce and in k_shadow (AMVPT_OPT_WAVEFRONT_SUFFIX,
    | AMVPT_OPT_SPLIT_NEE: the k_extend / k_bounce / k_shadow instances of the same walk; the default is
    k_suffix_fused),
  * the oracle's.
The scenes are string edits of the Cornell box: one box (the single-box loop only), the stock two at the config-M
shape, three (a pair, then a single), two stacked with a coplanar shared face plane (equal t across boxes),
two interpenetrating (candidates in both boxes, origins inside the other box's slabs), and a camera level with the
small cube's top face (grazing faces, key -inf, inside the pooled order).
"""
import os
import re

import numpy as np
import pytest

from conftest import SCENES

pytestmark = pytest.mark.gpu

CBOX = os.path.join(SCENES, "cbox_grid.xml")
CBOX_PATH = os.path.join(SCENES, "cbox_path.xml")

SMALL_BOX = re.compile(r'    <shape type="cube" id="small-box">.*?</shape>\n', re.S)
SMALL_XF = '<scale value="0.3"/>\n            <rotate y="1" angle="-17"/>\n            <translate x="0.335" y="-0.7" z="0.38"/>'
CUBE = """    <shape type="cube" id="%s">
        <transform name="to_world">
            %s
        </transform>
        <ref id="white"/>
    </shape>
"""


def _xml(case):
    """(xml or None for the stock grid scene, load defines, expected box meshes)"""
    path = open(CBOX_PATH).read()
    assert len(SMALL_BOX.findall(path)) == 1 and path.count(SMALL_XF) == 1
    kw = dict(res=48, spp=16)
    if case == "one_box":
        return SMALL_BOX.sub("", path), kw, 1
    if case == "m_shape":
        return None, dict(res=32, spp=16, gx=4, gy=2, reuse=8), 2
    if case == "three_boxes":
        third = CUBE % ("third-box", '<scale value="0.15"/>\n            <rotate y="1" angle="30"/>\n'
                        '            <translate x="0.45" y="-0.85" z="-0.4"/>')
        return path.replace("</scene>", third + "</scene>"), kw, 3
    if case == "stacked":
        # the small cube on the large one's top face (y = -0.4 + 0.61 = 0.41 - 0.2), turned as the large one is
        return path.replace(SMALL_XF, '<scale value="0.2"/>\n            <rotate y="1" angle="18.25"/>\n'
                            '            <translate x="-0.33" y="0.41" z="-0.28"/>'), kw, 2
    if case == "interpenetrating":
        # the small cube pushed half way into the large one
        return path.replace(SMALL_XF, '<scale value="0.3"/>\n            <rotate y="1" angle="-17"/>\n'
                            '            <translate x="-0.1" y="-0.7" z="-0.05"/>'), kw, 2
    assert case == "grazing_top_face"
    xml = path.replace('origin="0, 0, 3.90" target="0, 0, 0"', 'origin="0, -0.4, 3.9" target="0, -0.4, 0"')
    assert 'origin="0, -0.4, 3.9"' in xml
    return xml, kw, 2


def _bit_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _records(amvpt_mod, sd, vd, p, plan, flags):
    import torch
    assert torch.cuda.is_available()
    dev = amvpt_mod.DeviceScene(sd)
    film = torch.zeros((p.film_height, p.film_width, 5 if p.film_alpha else 4), dtype=torch.float32, device="cuda")
    rec = torch.zeros((plan["lanes"], plan["group"], 8), dtype=torch.float32, device="cuda")
    cnt = amvpt_mod.Counters()
    dev.render_ex(vd, p, film.data_ptr(), flags=flags, records_ptr=rec.data_ptr(), counters=cnt)
    torch.cuda.synchronize()
    return rec.cpu().numpy(), cnt.as_dict()["kernel_launches"]


CASES = ["one_box", "m_shape", "three_boxes", "stacked", "interpenetrating", "grazing_top_face"]


@pytest.mark.parametrize("case", CASES)
def test_pooled_rounds_keep_records(gpu_ready, amvpt_mod, oracle, case):
    xml, kw, boxes = _xml(case)
    s = amvpt_mod.load_file(CBOX, **kw) if xml is None else amvpt_mod.load_string(xml, **kw)
    assert amvpt_mod.scene_box_count(s) == boxes   # the screen really applies, to this many box meshes
    sd, vd, p = s.describe(0, 0, 0)
    plan = oracle.plan(p)
    W, N = amvpt_mod.OPT_WAVEFRONT_SUFFIX, amvpt_mod.OPT_SPLIT_NEE
    a, ka = _records(amvpt_mod, sd, vd, p, plan, 0)
    assert ka["k_suffix"] > 0 and ka["k_extend"] == 0   # the default is the fused suffix
    for name, flags in (("no box screen", amvpt_mod.OPT_NO_BOX_SCREEN), ("wavefront suffix", W),
                        ("wavefront suffix, split NEE", W | N)):
        b, kb = _records(amvpt_mod, sd, vd, p, plan, flags)
        if flags & W:
            assert kb["k_suffix"] == 0 and kb["k_extend"] > 0 and (kb["k_shadow"] > 0) == bool(flags & N)
        eq = _bit_equal(a, b).all(axis=(1, 2))
        assert eq.all(), "%s: %d of %d lanes differ from the default's" % (name, (~eq).sum(), eq.size)
    _, orec, _ = oracle.render(sd, vd, p, threads=16, record_pass=0)
    eq = _bit_equal(a, orec).all(axis=(1, 2))
    assert eq.all(), "oracle: %d of %d lanes differ" % ((~eq).sum(), eq.size)

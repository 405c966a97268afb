"""Every group-size kernel instance against the oracle.

k_prim_hit_req, k_prim_req, k_vis, k_mv_primary (launch_primary<G>) and k_splat_multi (launch_splat<G>) are compiled
once per view-group size: G = 2..16, <0> for 17..256 views, <-1> for 257..1024.  The instances of one G share their
source text but not their behaviour: pdf_in_regs<G, kDiff>() keeps a view's F_PDF in registers for generic groups of
2..8 views and in LDS for 9..16 (vs_fields: 5 or 6 fields per view), k_vis runs blocks of 64 x G threads, the 16-bit
view masks share a word with other fields (view bit 15 exists only at G = 16), the dynamic LDS of k_mv_primary grows
with G up to the 64 KiB ceiling, and the arena carves 4 B x G or 32 B x G of view records and (G + 7) / 8 ballot bytes
per lane.  This module renders one small frame per G -- res 8, 16 spp, reuse = G: one pass of 1024 x G lanes on a quilt
whose width is a multiple of 4 (tiled slots) -- under each flag set that selects another instance, plus the frames with
several groups, ragged odd groups and the run-time sizes at their boundaries.

The bar is test_gpu_parity.py's and exact: every per-lane, per-view record of pass 0 bit-identical to the oracle's,
the float film within 1e-5 of max |oracle film|, the AMVPT_OPT_DETERMINISTIC film EQUAL to the oracle's fixed-point
film with no range drops.  The oracle frames are computed once per shape (test_group_sizes.Frame) and shared by the
variants; tests/test_group_sizes.py asserts on the oracle alone that every view slot of every shape holds records and
that equal records tie the device to the slots' views.
"""
import numpy as np
import pytest

from test_group_sizes import (CBOX, COMPILE_TIME, MESH, MIS_VARIANT_G, RAGGED, RUNTIME, TWO_GROUPS, VEACH, Frame,
                              check_mixed_waves, shape)

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module", autouse=True)
def _device_started(gpu_ready, amvpt_mod):
    """The process's one-time costs (importing torch, creating the HIP context, loading the library's code objects at
    its first launch) are paid here when this module is the first to use the device, so that `--durations` shows each
    case's own time."""
    torch = _torch()
    s = amvpt_mod.load_file(CBOX, res=4, spp=16)
    sd, vd, p = s.describe(0, 0, 0)
    film = torch.zeros((p.film_height, p.film_width, 4), dtype=torch.float32, device="cuda")
    amvpt_mod.DeviceScene(sd).render_ex(vd, p, film.data_ptr())
    torch.cuda.synchronize()


def _bit_equal(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _render(f, flags=0, records=True, **kw):
    """One instrumented frame of Frame `f` (its lane range) through amvpt_render_ex: (film, records of pass 0 or None,
    counters as a dict)."""
    torch = _torch()
    if not hasattr(f, "dev"):
        f.dev = f.mod.DeviceScene(f.sd)
    film = torch.zeros((f.p.film_height, f.p.film_width, 4), dtype=torch.float32, device="cuda")
    rec = None
    if records:
        rec = torch.zeros((f.lanes[1] - f.lanes[0], f.G, 8), dtype=torch.float32, device="cuda")
    cnt = f.mod.Counters()
    f.dev.render_ex(f.vd, f.p, film.data_ptr(), lanes=f.mod.LaneSet(f.lanes[0], f.lanes[1], 0, 0, 0, 0), flags=flags,
                    records_ptr=rec.data_ptr() if records else None, counters=cnt, **kw)
    torch.cuda.synchronize()
    return film.cpu().numpy(), (rec.cpu().numpy() if records else None), cnt.as_dict()


def _assert_records(f, grec, what):
    orec = f.oracle()[1]
    eq = _bit_equal(grec, orec)
    lanes = eq.all(axis=(1, 2))
    print("%s: %.6f of %d lanes x %d views bit-identical" % (what, lanes.mean(), len(lanes), f.G))
    if not lanes.all():
        slots = ~eq.all(axis=2)
        print("differing records per view slot:", slots.sum(axis=0))
        for lane in np.argwhere(~lanes)[:3, 0]:
            k = int(np.argmax(slots[lane]))
            print("lane", lane, "slot", k, "\ngpu", grec[lane, k], "\noracle", orec[lane, k])
    assert lanes.all(), "%s: lane records %.6f bit-identical" % (what, lanes.mean())


def _assert_film_close(f, gfilm, what):
    ofilm = f.oracle()[0]
    err = np.abs(gfilm - ofilm).max() / np.abs(ofilm).max()
    print("%s: film max |diff| / max |oracle film| = %.3e" % (what, err))
    assert err < TOL, "%s: film max relative difference %.3e" % (what, err)


def _plain(f, flags=0, what="default", film=True, **kw):
    """Variant (a) and its flagged relatives: records on, every record bit-identical, the float film within 1e-5."""
    gfilm, grec, c = _render(f, flags, **kw)
    _assert_records(f, grec, what)
    if film:
        _assert_film_close(f, gfilm, what)
    return c


def _deterministic(f, what="deterministic", **kw):
    """Variant (d): AMVPT_OPT_DETERMINISTIC -- k_splat_multi<G, ..., kFx>; the film equals the oracle's fixed-point
    film and nothing left the 32.32 range."""
    gfilm, grec, c = _render(f, f.mod.OPT_DETERMINISTIC, **kw)
    _assert_records(f, grec, what)
    xfilm = f.oracle_fixed()
    diff = int((~_bit_equal(gfilm, xfilm)).sum())
    print("%s: %d of %d film floats differ, %d range drops" % (what, diff, gfilm.size, c["film_range_drops"]))
    assert diff == 0, "%s: %d film floats differ from the oracle's fixed-point film" % (what, diff)
    assert c["film_range_drops"] == 0 and np.abs(gfilm).max() > 0
    return c


def _launches(c):
    return c["kernel_launches"]


def _assert_fused(c):
    k = _launches(c)
    assert k["k_vis"] == 0 and k["k_prim_hit"] == 0 and k["k_mv_primary"] > 0, k


def _assert_split(c):
    k = _launches(c)
    assert k["k_vis"] > 0 and k["k_prim_hit"] > 0 and k["k_mv_primary"] > 0, k


@pytest.mark.parametrize("G", COMPILE_TIME)
def test_all_diffuse(gpu_ready, amvpt_mod, oracle, G):
    """cbox_grid.xml, one group of G views.  (a) default flags: the fused vertex k_mv_primary<G, true, true, false,
    true> and the row splat with records; (b) AMVPT_OPT_SPLIT_PRIMARY: k_prim_hit_req<G> -> k_vis<G> (ray pairs) ->
    k_mv_primary<G, true, true>; (c) AMVPT_OPT_GENERIC_KERNELS: the generic instances (32-byte view records, the kDW
    launch takes every wave); (d) the fixed-point film's splat; (e) a plain render: the row splat's kRec = false
    instance, the one the benchmark runs; (f, G in 7, 11, 16) per-lane traversal: k_prim_req<G> and k_vis<G, false>."""
    m = amvpt_mod
    f = Frame(m, oracle, CBOX, shape(G))
    assert f.G == G and f.plan["lanes"] == 1024 * G and f.p.film_width % 4 == 0
    a = _plain(f, what="(a) default")
    _assert_fused(a)
    _assert_split(_plain(f, m.OPT_SPLIT_PRIMARY, "(b) split primary"))
    _assert_split(_plain(f, m.OPT_GENERIC_KERNELS, "(c) generic kernels"))
    _assert_fused(_deterministic(f, "(d) deterministic"))
    efilm, _, e = _render(f, records=False)
    _assert_film_close(f, efilm, "(e) plain render")
    _assert_fused(e)
    print("view_splats: %d with records, %d plain" % (a["view_splats"], e["view_splats"]))
    assert e["view_splats"] == a["view_splats"] > 0
    if G in (7, 11, 16):
        k = _launches(_plain(f, what="(f) per-lane traversal", traversal=2))
        assert k["k_prim_req"] > 0 and k["k_prim_hit"] > 0 and k["k_vis"] > 0, k


@pytest.mark.parametrize("G", COMPILE_TIME)
def test_glossy(gpu_ready, amvpt_mod, oracle, G):
    """veach_grid.xml, one group of G views: the generic k_prim_hit_req<G>, k_vis<G> and both launches of the generic
    k_mv_primary<G> -- kDW for the waves whose primary hits are all diffuse or misses, the generic body (F_PDF in
    registers up to G = 8, in LDS from G = 9: vs_fields 5 or 6) for the others; the host check shows that the frame
    holds waves of both kinds.  (a) and (d); G = 8, 9 (the two sides of pdf_in_regs) and 16 (view bit 15, the
    1024-thread k_vis block, 49152 B of per-view state) also with fast_mis and without sa_mis."""
    variants = [dict()] + ([dict(fast_mis="true"), dict(sa_mis="false")] if G in MIS_VARIANT_G else [])
    for mis in variants:
        f = Frame(amvpt_mod, oracle, VEACH, shape(G, **mis))
        assert f.G == G and f.plan["lanes"] == 1024 * G
        check_mixed_waves(f)
        tag = " ".join("%s=%s" % kv for kv in mis.items())
        _assert_split(_plain(f, what="(a) default " + tag))
        _assert_split(_deterministic(f, "(d) deterministic " + tag))


@pytest.mark.parametrize("case", list(TWO_GROUPS))
def test_two_groups(gpu_ready, amvpt_mod, oracle, case):
    """Several groups per frame: group_view_n wraps inside the lane's own group (p_idx / Gn > 0), and the view table
    reaches and passes the staging limit.  The table is staged in LDS while n_views x sizeof(DView) = n_views x 272 B
    fits kViewTabBytes = 8192 B (dscene.h; views_lds_bytes and the static_assert on sizeof(DView) in amvpt_render.hip):
    30 views x 272 = 8160 B is the largest staged table, 32 views x 272 = 8704 B is not staged, and with it neither
    are the scene tables (tables_staged): the kTab = false instances.
      cbox_7x2_g7     two odd groups, fused vertex.
      veach_6x5_g15   two groups of 15; dynamic LDS of the generic k_mv_primary<15> = tables (<= 8192) + 8160 + 6 fields
                      x 15 views x 128 threads x 4 B = 46080 B: the most a 15-view kernel takes.
      veach_4x4_g16   6 x 16 x 128 x 4 = 49152 B of per-view state + 16 x 272 = 4352 B of views + tables.
      veach_8x4_g16   32 views: k_prim_hit_req<16, false, ...>, k_mv_primary<16, false, false, true / false>.
      cbox_8x4_g16    32 views: k_mv_primary<16, false, true> -- and no fused vertex, which exists with staged tables
                      only (launch_primary: `tab && diff`), so the three launches run; also under
                      AMVPT_OPT_GENERIC_KERNELS.
    Nothing reports the staging itself; the arithmetic above is what puts the cases on their side of it."""
    scene, defines, G, views = TWO_GROUPS[case]
    f = Frame(amvpt_mod, oracle, scene, defines)
    assert f.G == G and f.p.n_views == views and f.plan["lanes"] == 1024 * views
    staged = views * 272 <= 8192
    assert staged == (case not in ("veach_8x4_g16", "cbox_8x4_g16"))
    if scene == VEACH:
        check_mixed_waves(f)
    a = _plain(f, what="(a) default")
    d = _deterministic(f, "(d) deterministic")
    for c in (a, d):
        if scene == CBOX and staged:
            _assert_fused(c)
        else:
            _assert_split(c)
    if case == "cbox_8x4_g16":
        _assert_split(_plain(f, amvpt_mod.OPT_GENERIC_KERNELS, "(c) generic kernels"))


@pytest.mark.parametrize("case", list(RAGGED))
def test_ragged_odd_group(gpu_ready, amvpt_mod, oracle, case):
    """Odd groups on frames that fill no block: 7 x 1 and 13 x 1 views of 5 x 5 px are 2800 and 5200 lanes -- a partial
    last block and wave, a quilt width that is no multiple of 4 (no tiled slots).  Rendered whole and in chunks of 1000
    lanes: the record planes of an odd G x odd chunk sizes must be read where they were written.  The same two groups
    on cbox_mesh.xml at res 8: the per-depth wavefront suffix with ray binning under an odd G."""
    scene, defines, G, lanes = RAGGED[case]
    f = Frame(amvpt_mod, oracle, scene, defines)
    assert f.G == G and f.plan["lanes"] == lanes
    whole = _plain(f, what="whole")
    chunked = _plain(f, what="chunks of 1000", chunk_lanes=1000)
    det = _deterministic(f, "deterministic, chunks of 1000", chunk_lanes=1000)
    n_chunks = -(-lanes // 1000)
    for c in (chunked, det):
        assert c["chunk_lanes"] == 1000 and _launches(c)["k_mv_primary"] == n_chunks, (c["chunk_lanes"], _launches(c))
    for key in ("lanes", "vertices", "view_splats", "visibility_rays"):
        assert whole[key] == chunked[key] == det[key], key
    if scene == MESH:
        for c in (whole, chunked):
            k = _launches(c)
            assert k["k_bin"] > 0 and k["k_extend"] > 0 and k["k_suffix"] == 0, k
    else:
        _assert_fused(whole)
        _assert_fused(chunked)


@pytest.mark.parametrize("case", list(RUNTIME))
def test_runtime_boundaries(gpu_ready, amvpt_mod, oracle, case):
    """The run-time instances at their boundaries: 17 views (the first group of launch_primary<0>, next to the 4 x 4
    G = 16 case) all-diffuse and glossy, 257 views (the first 1024-bit group, <-1>) and 1024 views, the largest legal
    group, as two lane ranges of 2048 rendered on both sides: the frame's first lanes and a range from the middle of the
    frame that starts 37 lanes past a wave boundary.  Above 256 views the float film is not compared (a cell sums
    thousands of splats: test_groups_above_16_views); the deterministic film is, and must be equal."""
    scene, defines, G, ranges = RUNTIME[case]
    for lanes in ranges or (None,):
        f = Frame(amvpt_mod, oracle, scene, defines, lanes)
        assert f.G == G
        tag = "lanes [%d, %d)" % f.lanes
        _assert_split(_plain(f, what="(a) default " + tag, film=G <= 256))
        _assert_split(_deterministic(f, "(d) deterministic " + tag))
    if scene == VEACH:
        check_mixed_waves(f)

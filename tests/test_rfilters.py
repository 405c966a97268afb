"""The tent, Mitchell-Netravali, Catmull-Rom and Lanczos reconstruction filters on the CPU: the host loader, the
host-side filter hook (amvpt_rfilter_eval: the function the splat kernels evaluate, compiled for the host), a numpy
restatement of ImageBlock::put anchored on the oracle's film, and the multi-rank borders.

The restatement (`put_film`) is the yardstick tests/test_gpu_rfilters.py holds the device films of these filters to:
the oracle only knows the Gaussian and the box filter, but its per-lane records (the put arguments) do not depend on
the filter."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import SCENES

CBOX = os.path.join(SCENES, "cbox_grid.xml")
CBOX_PATH = os.path.join(SCENES, "cbox_path.xml")
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfilter_kats.json")

F32 = np.float32
THIRD = F32(1.0) / F32(3.0)


def filter_xml(elem, scene=CBOX):
    """The scene's XML with its <rfilter> replaced by `elem` (a filter with keys cannot come from a $define)."""
    src = open(scene).read()
    old = '<rfilter type="$rfilter"/>' if '<rfilter type="$rfilter"/>' in src else '<rfilter type="gaussian"/>'
    assert src.count(old) == 1
    return src.replace(old, elem)


def elem(kind, **keys):
    """<rfilter type=kind> with float keys (an int value becomes an <integer>)."""
    body = "".join('<%s name="%s" value="%r"/>' % ("integer" if isinstance(v, int) else "float", k, v)
                   for k, v in keys.items())
    return '<rfilter type="%s">%s</rfilter>' % (kind, body)


def params_for(amvpt_mod, kind, radius=0.0, b=THIRD, c=THIRD, stddev=0.5):
    p = amvpt_mod.Params()
    p.rfilter = kind
    p.rfilter_stddev = stddev
    p.rfilter_radius = radius
    p.rfilter_b, p.rfilter_c = b, c
    return p


# ---------------------------------------------------------------------------------------------------
# numpy restatement of section 3 of the filter definitions (f32, every operation rounded on its own;
# fmadd through float64)
# ---------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """fl32(a * b + c) with one rounding.  The f64 product of two f32 is exact; the f64 sum is rounded to odd (from
    its round-to-nearest value and the exact TwoSum residual), after which the rounding to f32 is the correct one."""
    a, b, c = np.broadcast_arrays(*[np.atleast_1d(np.asarray(v, F32)).astype(np.float64) for v in (a, b, c)])
    p = a * b
    t = p + c
    bb = t - p
    e = (p - (t - bb)) + (c - bb)
    even = (e != 0) & ((t.view(np.int64) & 1) == 0)
    t = np.where(even, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
    return t.astype(F32)


def np_tent(x, radius=1.0):
    inv = F32(1.0) / F32(radius)
    return np.maximum(F32(0), F32(1) - np.abs(x.astype(F32) * inv)).astype(F32)


def mitchell_scalars(b, c):
    b, c = F32(b), F32(c)
    n = F32
    return ((n(12) - n(9) * b) - n(6) * c, (n(-18) + n(12) * b) + n(6) * c, n(6) - n(2) * b,
            (-b) - n(6) * c, n(6) * b + n(30) * c, n(-12) * b - n(48) * c, n(8) * b + n(24) * c)


def np_mitchell(x, b=THIRD, c=THIRD):
    a3, a2, a0, b3, b2, b1, b0 = mitchell_scalars(b, c)
    x = np.abs(x.astype(F32))
    x2 = x * x
    x3 = x2 * x
    inner = fma32(a3, x3, fma32(a2, x2, a0))
    outer = fma32(b3, x3, fma32(b2, x2, fma32(b1, x, b0)))
    res = (F32(1) / F32(6)) * np.where(x < 1, inner, outer)
    return np.where(x < 2, res, F32(0)).astype(F32)


def np_catmullrom(x):
    x = np.abs(x.astype(F32))
    x2 = x * x
    x3 = x2 * x
    inner = ((F32(9) * x3) + (F32(-15) * x2)) + F32(6)
    outer = (((F32(-3) * x3) + (F32(15) * x2)) + (F32(-24) * x)) + F32(12)
    res = (F32(1) / F32(6)) * np.where(x < 1, inner, outer)
    return np.where(x < 2, res, F32(0)).astype(F32)


def f64_lanczos(x, lobes=3.0):
    x = np.abs(x.astype(F32)).astype(np.float64)
    x1 = np.pi * x
    x2 = x1 / lobes
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.sin(x1) * np.sin(x2) / (x1 * x2)
    return np.where(x < 2.0 ** -24, 1.0, np.where(x > lobes, 0.0, res))


def grid(radius, n=4000):
    """~n arguments over [-radius - 1, radius + 1], with 0, +-1, +-radius and the f32 neighbours of each."""
    pts = []
    for v in (0.0, 1.0, -1.0, radius, -radius, 2.0, -2.0):
        v = F32(v)
        pts += [v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))]
    lin = np.linspace(-radius - 1, radius + 1, n).astype(F32)
    return np.concatenate([lin, np.array(pts, dtype=F32)])


# ---------------------------------------------------------------------------------------------------
# numpy restatement of ImageBlock::put (imageblock.cpp:265-427 non-coalesced, :433-558 coalesced), the
# JIT branch with recorded loops: weight = eval(rel.x + xs) * eval(rel.y + ys), accum(value_k * weight)
# ---------------------------------------------------------------------------------------------------

def _cells(pos, size, offset, radius, coalesce):
    """Per sample: first cell (unsigned semantics kept as int64), per-axis count, last valid cell, and the filter
    argument of the first cell -- for x and y (pos: (n, 2) f32)."""
    off = np.array(offset, dtype=np.int64)
    sz = np.array(size, dtype=np.int64)
    r = F32(radius)
    if not coalesce:
        shift = F32(F32(0 - off[0]) - F32(.5)), F32(F32(0 - off[1]) - F32(.5))
        pos_f = (pos + np.array(shift, dtype=F32)).astype(F32)
        p0 = np.maximum(np.ceil((pos_f - r).astype(F32)).astype(np.int64), 0)
        p1 = np.minimum(np.floor((pos_f + r).astype(F32)).astype(np.int64), sz - 1)
        count = int(np.ceil(F32(2) * r))
        rel = (p0.astype(F32) - pos_f).astype(F32)
        active = (p0 <= p1).all(axis=1)
        return p0, p1, count, rel, active
    n = int(np.ceil(r - F32(.5)))
    count = 2 * n + 1
    pos_i = np.floor(pos).astype(np.int64) - n
    local = pos_i - off
    rel = ((pos_i.astype(F32) + F32(.5)) - pos).astype(F32)
    # UInt32(local) < size: a negative start never matches until it reaches 0
    return local, np.broadcast_to(sz - 1, local.shape), count, rel, np.ones(len(pos), dtype=bool)


def put_film(records, group, params, weight_fn, radius, coalesce_single, fixed=False):
    """The ImageBlock after putting every valid record.  records: (lanes, G, 8) [x, y, r, g, b, alpha, weight, valid]
    (one array or a list of them, one per pass); slot 0 of a group > 1 is put coalesced, the other slots not; a
    group of 1 is coalesced when coalesce_single.  weight_fn: f32 array -> f32 filter values.  Products
    value_k * (wx * wy) in f32; sums in float64, or (fixed) as integers of 2^-32 after rint, which is the
    deterministic film's definition; fixed="both" returns (float64-summed film, fixed-point film)."""
    W, H = int(params.film_width), int(params.film_height)
    C = 5 if params.film_alpha else 4
    offset = (int(params.crop_offset_x), int(params.crop_offset_y))
    want_float, want_fixed = fixed in (False, "both"), fixed in (True, "both")
    acc = np.zeros(W * H * C, dtype=np.float64)
    acc_fx = np.zeros(W * H * C, dtype=np.float64)
    recs = records if isinstance(records, (list, tuple)) else [records]
    for rec in recs:
        for slot in range(group):
            r = rec[:, slot, :]
            r = r[r[:, 7] != 0]
            if not len(r):
                continue
            coalesce = coalesce_single if group == 1 else slot == 0
            vals = r[:, [2, 3, 4, 5, 6]] if C == 5 else r[:, [2, 3, 4, 6]]
            pos = np.ascontiguousarray(r[:, 0:2], dtype=F32)
            first, last, count, rel, active = _cells(pos, (W, H), offset, radius, coalesce)
            wx = [weight_fn((rel[:, 0] + F32(t)).astype(F32)) for t in range(count)]
            wy = [weight_fn((rel[:, 1] + F32(t)).astype(F32)) for t in range(count)]
            for ys in range(count):
                cy = first[:, 1] + ys
                oky = active & (cy >= 0) & (cy <= last[:, 1])
                for xs in range(count):
                    cx = first[:, 0] + xs
                    ok = oky & (cx >= 0) & (cx <= last[:, 0])
                    if not ok.any():
                        continue
                    w = (wx[xs] * wy[ys]).astype(F32)[ok]
                    base = (cy[ok] * W + cx[ok]) * C
                    for k in range(C):
                        v = (vals[ok, k] * w).astype(F32)
                        if want_fixed:
                            d = v.astype(np.float64) * 4294967296.0
                            keep = np.abs(d) < 2147483647.0 * 4294967296.0
                            acc_fx += np.bincount(base[keep] + k, weights=np.rint(d[keep]), minlength=acc.size)
                        if want_float:
                            acc += np.bincount(base + k, weights=v.astype(np.float64), minlength=acc.size)
    # integer sums carried in float64: exact while every partial sum stays below 2^53
    assert np.abs(acc_fx).max() < 2.0 ** 52
    film = acc.astype(F32).reshape(H, W, C)
    film_fx = (acc_fx * (1.0 / 4294967296.0)).astype(F32).reshape(H, W, C)
    return (film, film_fx) if fixed == "both" else film_fx if fixed else film


def gaussian_params(p):
    """A copy of the params with the default Gaussian: what the oracle (which knows no other filter) is given; its
    records do not depend on the filter."""
    q = type(p)()
    ctypes.memmove(ctypes.addressof(q), ctypes.addressof(p), ctypes.sizeof(p))
    q.rfilter = 1
    q.rfilter_stddev = 0.5
    return q


def weight_fn_of(amvpt_mod, p):
    return lambda x: amvpt_mod.rfilter_eval(p, x)[0]


# ---------------------------------------------------------------------------------------------------
# 1. loader
# ---------------------------------------------------------------------------------------------------

LOADER_CASES = [
    (elem("tent"), 2, 1.0, THIRD, THIRD),
    (elem("tent", radius=1.7), 2, F32(1.7), THIRD, THIRD),
    (elem("mitchell"), 3, 0.0, THIRD, THIRD),
    (elem("mitchell", B=0.0, C=0.5), 3, 0.0, F32(0), F32(.5)),
    (elem("catmullrom"), 4, 0.0, THIRD, THIRD),
    (elem("lanczos"), 5, 3.0, THIRD, THIRD),
    (elem("lanczos", lobes=4), 5, 4.0, THIRD, THIRD),
]


@pytest.mark.parametrize("xml,kind,radius,b,c", LOADER_CASES, ids=["tent", "tent_r1.7", "mitchell", "mitchell_b0_c.5", "catmullrom", "lanczos", "lanczos_4"])
def test_loader_accepts_the_four_filters(amvpt_mod, xml, kind, radius, b, c):
    s = amvpt_mod.load_string(filter_xml(xml), res=8, spp=4)
    _, _, p = s.describe(0, 0, 0)
    assert p.rfilter == kind
    assert F32(p.rfilter_radius) == F32(radius)
    assert F32(p.rfilter_b) == F32(b) and F32(p.rfilter_c) == F32(c)


def test_loader_filter_from_a_define(amvpt_mod):
    """The parent refused load_file(CBOX, rfilter="tent") with "not implemented"."""
    for name, kind in (("tent", 2), ("mitchell", 3), ("catmullrom", 4), ("lanczos", 5)):
        assert amvpt_mod.load_file(CBOX, res=8, spp=4, rfilter=name).describe(0, 0, 0)[2].rfilter == kind


@pytest.mark.parametrize("kind", ["tent", "mitchell", "catmullrom", "lanczos"])
def test_loader_refuses_a_stray_key(amvpt_mod, kind):
    with pytest.raises(RuntimeError, match=r'"\["stdev"\]" in reconstructionfilter plugin of type "%s"' % kind):
        amvpt_mod.load_string(filter_xml(elem(kind, stdev=1.0)), res=8, spp=4)


def test_loader_refuses_an_unknown_filter(amvpt_mod):
    with pytest.raises(RuntimeError, match=r'rfilter "nosuch" is not implemented \(gaussian, box, tent, mitchell, '
                                           r'catmullrom, lanczos\)'):
        amvpt_mod.load_string(filter_xml('<rfilter type="nosuch"/>'), res=8, spp=4)


# ---------------------------------------------------------------------------------------------------
# 2. rfilter_eval
# ---------------------------------------------------------------------------------------------------

def test_abi_and_flag(amvpt_mod):
    assert amvpt_mod.hip_lib().amvpt_abi_version() == 12
    assert amvpt_mod.OPT_BLOCK_SPLAT == 512
    with pytest.raises(RuntimeError, match="unknown rfilter"):
        amvpt_mod.rfilter_eval(params_for(amvpt_mod, 6), np.zeros(1, dtype=F32))


def test_known_answers(amvpt_mod):
    kinds = dict(tent=2, mitchell=3, catmullrom=4, lanczos=5)
    kats = json.load(open(KATS))["kats"]
    assert len(kats) == 8
    for k in kats:
        got = amvpt_mod.rfilter_eval(params_for(amvpt_mod, kinds[k["filter"]]), np.array([k["x"]], dtype=F32))[0][0]
        if k["atol"] == 0:
            assert got == k["value"], k
        else:
            assert abs(got - k["value"]) <= k["atol"], (k, got)


@pytest.mark.parametrize("name,kw,ref", [
    ("tent", dict(), lambda x: np_tent(x)),
    ("tent", dict(radius=1.7), lambda x: np_tent(x, 1.7)),
    ("tent", dict(radius=2.6), lambda x: np_tent(x, 2.6)),
    ("tent", dict(radius=0.75), lambda x: np_tent(x, 0.75)),
    ("mitchell", dict(), lambda x: np_mitchell(x)),
    ("mitchell", dict(b=F32(0), c=F32(.5)), lambda x: np_mitchell(x, 0, .5)),
    ("catmullrom", dict(), np_catmullrom),
], ids=["tent", "tent_r1.7", "tent_r2.6", "tent_r0.75", "mitchell", "mitchell_b0_c.5", "catmullrom"])
def test_eval_is_the_stated_arithmetic_bit_for_bit(amvpt_mod, name, kw, ref):
    kind = dict(tent=2, mitchell=3, catmullrom=4)[name]
    p = params_for(amvpt_mod, kind, **kw)
    got, radius = amvpt_mod.rfilter_eval(p, np.zeros(1, dtype=F32))
    assert radius == (F32(kw.get("radius", 1.0)) if name == "tent" else 2.0)
    x = grid(float(radius))
    got, _ = amvpt_mod.rfilter_eval(p, x)
    want = ref(x)
    assert got.dtype == F32 and want.dtype == F32
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), np.argwhere(got != want)[:5]
    # the default parameters' literals in the row-splat kernels are these scalars
    if name == "mitchell" and not kw:
        assert [float(v).hex() for v in mitchell_scalars(THIRD, THIRD)] == [
            "0x1.c000000000000p+2", "-0x1.8000000000000p+3", "0x1.5555560000000p+2", "-0x1.2aaaaa0000000p+1",
            "0x1.8000000000000p+3", "-0x1.4000000000000p+4", "0x1.5555560000000p+3"]


@pytest.mark.parametrize("lobes", [3, 4, 5])
def test_lanczos_against_float64(amvpt_mod, lobes):
    """Lanczos carries no bit-exactness claim (the sine is the platform's): 1e-6 absolute of a float64 evaluation."""
    p = params_for(amvpt_mod, 5, radius=float(lobes))
    x = grid(float(lobes))
    got, radius = amvpt_mod.rfilter_eval(p, x)
    assert radius == lobes
    assert np.abs(got.astype(np.float64) - f64_lanczos(x, float(lobes))).max() <= 1e-6
    assert amvpt_mod.rfilter_eval(params_for(amvpt_mod, 5), x[:1])[1] == 3.0   # 0: the default lobes


def test_gaussian_and_box_through_the_hook_equal_the_oracle(amvpt_mod, oracle):
    """The hook's anchor: the filters the oracle knows, through the same entry."""
    L = oracle.lib()
    for stddev in (0.5, 1.5):
        x = grid(4 * stddev)
        got, radius = amvpt_mod.rfilter_eval(params_for(amvpt_mod, 1, stddev=stddev), x)
        assert radius == 4 * stddev
        want = np.array([L.oracle_gaussian_eval(stddev, float(v)) for v in x], dtype=F32)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
    got, radius = amvpt_mod.rfilter_eval(params_for(amvpt_mod, 0), grid(1.0))
    assert (got == 1).all() and radius == 0.5


# ---------------------------------------------------------------------------------------------------
# 3. the restatement of ImageBlock::put against the oracle
# ---------------------------------------------------------------------------------------------------

CBOX_BATCH = os.path.join(SCENES, "cbox_batch.xml")
ANCHORS = [
    ("g8_two_passes", CBOX, False, dict(res=12, spp=32, gx=4, gy=2, reuse=8)),
    ("g1_reuse_off", CBOX, False, dict(res=12, spp=32, gx=4, gy=2, reuse=1)),
    ("stock_path", CBOX_PATH, False, dict(res=16, spp=16)),
    ("rgba", CBOX, True, dict(res=12, spp=16, gx=4, gy=2, reuse=8)),
    ("batch_crop", CBOX_BATCH, False, dict(res=16, width=64, spp=16, crop_w=32, crop_h=8, crop_x=16, crop_y=4)),
    ("wide_gaussian", CBOX, False, dict(res=12, spp=16, gx=4, gy=2, reuse=8, stddev=1.5)),
]


@pytest.fixture(scope="module", params=ANCHORS, ids=[a[0] for a in ANCHORS])
def small_frame(request, amvpt_mod, oracle):
    """A small frame of every record layout the device tests feed the restatement: the oracle's records of every
    pass, its film and its fixed-point film (default Gaussian; one case with a 7 / 12-cell footprint)."""
    _, scene, rgba, defines = request.param
    defines = dict(defines)
    stddev = defines.pop("stddev", 0.5)
    xml = filter_xml(elem("gaussian", stddev=stddev), scene)
    if rgba:
        xml = xml.replace('name="pixel_format" value="rgb"', 'name="pixel_format" value="rgba"')
    s = amvpt_mod.load_string(xml, **defines)
    sd, vd, p = s.describe(0, 0, 0)
    plan = oracle.plan(p)
    if request.param[0] == "g8_two_passes":
        assert (plan["passes"], plan["spp_per_pass"], plan["group"], p.adaptive) == (2, 16, 8, 0)
    film = oracle.render(sd, vd, p, threads=4)[0]
    recs = [oracle.render(sd, vd, p, threads=4, record_pass=k)[1] for k in range(plan["passes"])]
    fixed = oracle.render(sd, vd, p, threads=4, fixed_film=True)[0]
    return dict(scene=s, p=p, plan=plan, film=film, fixed=fixed, recs=recs, radius=4 * stddev)


def test_put_restatement_equals_the_oracle_film(amvpt_mod, small_frame):
    f = small_frame
    got, got_fx = put_film(f["recs"], f["plan"]["group"], f["p"], weight_fn_of(amvpt_mod, f["p"]), f["radius"],
                           f["plan"]["spp_per_pass"] >= 4, fixed="both")
    assert np.abs(got - f["film"]).max() <= 1e-5 * np.abs(f["film"]).max()
    assert (got_fx.view(np.uint32) == f["fixed"].view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------------
# 4. multi-rank borders
# ---------------------------------------------------------------------------------------------------

def test_filter_borders(amvpt_mod):
    from amvpt import dist as adist
    assert adist.filter_border(params_for(amvpt_mod, 2, radius=1.0)) == 4
    assert adist.filter_border(params_for(amvpt_mod, 2)) == 4
    assert adist.filter_border(params_for(amvpt_mod, 3)) == 4
    assert adist.filter_border(params_for(amvpt_mod, 4)) == 4
    assert adist.filter_border(params_for(amvpt_mod, 5, radius=5.0)) == 6
    assert adist.filter_border(params_for(amvpt_mod, 2, radius=4.2)) == 5


def test_view_group_partition_follows_a_lanczos_filter(amvpt_mod):
    s = amvpt_mod.load_string(filter_xml(elem("lanczos", lobes=5)), res=16, spp=16, gx=8, gy=4, reuse=4)
    _, _, p = s.describe(0, 0, 0)
    assert p.rfilter == 5 and p.rfilter_radius == 5.0
    H = amvpt_mod.host_lib()
    rect, win = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)()
    inner_edges = 0
    for rank in range(2):
        assert H.amvpt_host_view_group_partition(ctypes.byref(p), rank, 2, rect, win) == 1
        x0, y0, w, h = list(rect)
        assert (w, h) in ((p.film_width, p.film_height // 2), (p.film_width // 2, p.film_height))
        assert list(win) == [max(0, x0 - 6), max(0, y0 - 6),
                             min(p.film_width, x0 + w + 6) - max(0, x0 - 6),
                             min(p.film_height, y0 + h + 6) - max(0, y0 - 6)]
        # the edge a rank shares with the other one lies inside the quilt: 6 pixels of border there
        inner_edges += (win[2] * win[3] == (w + 6) * h) + (win[2] * win[3] == w * (h + 6))
    assert inner_edges == 2

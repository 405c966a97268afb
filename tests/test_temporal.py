"""Temporal accumulation on the CPU (include/amvpt_temporal.h): amvpt_temporal_host against a numpy float32 restatement
of the header's definition, bit for bit; what the definition promises about an empty history, a static camera, pixels
that are not finite and buffers it must not touch; the refusals; and the quality gate on oracle renders.  The guide
records come from the oracle's primary-hit hook, which is what amvpt_guides reproduces on the device.
tests/test_gpu_temporal.py runs the device entry over the same cases.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO, SCENES
from test_denoise import rel_rmse
from test_guides import bits, open_scene_xml, xml_of

F = np.float32
GUARD = 64
SENTINEL = F(-12345.0)
CAMERA = 'origin="0, 0, 3.9" target="0, 0, 0"'


# ---------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """fma(a, b, c) of float32 operands rounded once to float32.  The product is exact in float64; the sum is rounded
    to odd in float64 (the sticky bit of the exact sum goes into the last place), after which the rounding to
    float32 is the rounding of the exact value (53 >= 2 * 24 + 2)."""
    a, b, c = (np.asarray(v, dtype=F).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)                      # TwoSum: p + c = s + e exactly
        inexact = np.isfinite(e) & (e != 0) & np.isfinite(s)
        toward = np.where((e > 0) == (s > 0), s, np.nextafter(s, 0.0))          # the exact sum, truncated
        away = np.nextafter(toward, np.where(s > 0, np.inf, -np.inf))
        odd = (np.ascontiguousarray(toward).view(np.int64) & 1) == 1
        return np.where(inexact, np.where(odd, toward, away), s).astype(F)


def _dot(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z, every product and sum rounded to float32."""
    return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)


def _row(m, r, q):
    return fma32(m[..., 4 * r + 2], q[..., 2], fma32(m[..., 4 * r + 1], q[..., 1], fma32(m[..., 4 * r], q[..., 0], m[..., 4 * r + 3])))


def view_table(vd, n):
    get = lambda f: np.array([list(getattr(vd[i], f)) for i in range(n)], dtype=F)   # noqa: E731
    one = lambda f: np.array([getattr(vd[i], f) for i in range(n)], dtype=F)         # noqa: E731
    return dict(type=np.array([vd[i].type for i in range(n)]), twi=get("to_world_inv"), c2s=get("camera_to_sample"),
                near=one("near_clip"), far=one("far_clip"), res=get("resolution"), pp=get("pp_offset"),
                ap=one("aperture_radius"), fd=one("focus_distance"))


def layout_of(p):
    """(n_views, tw, th, tile origin of a view index array) as the header's Layout paragraph forms them."""
    W, H = int(p.film_width), int(p.film_height)
    if not p.multisensor:
        return 1, W, H, lambda v: (np.zeros_like(v), np.zeros_like(v))
    n = int(p.n_views)
    if p.batch:
        tw = W // n
        return n, tw, H, lambda v: ((n - 1 - v if p.reverse_x else v) * tw, np.zeros_like(v))
    gx, gy = int(p.grid_x), int(p.grid_y)
    tw, th = W // gx, H // gy

    def origin(v):
        col, row = v % gx, v // gx
        return (gx - 1 - col if p.reverse_x else col) * tw, (gy - 1 - row if p.reverse_y else row) * th
    return n, tw, th, origin


def restated(img, g, hi, hg, hc, prev_views, p, tp, rect=None, stops=True, diag=None):
    """amvpt_temporal_host in numpy -> (image, count).  stops=False leaves the shape, normal and plane stops out (the
    power check's ghosting); `diag` receives what the regime assertions need."""
    img, g, hi, hg = (np.ascontiguousarray(a, dtype=F) for a in (img, g, hi, hg))
    h, w = g.shape[:2]
    hc = np.ascontiguousarray(hc, dtype=F).reshape(h, w)
    rx0, ry0 = (int(rect[0]), int(rect[1])) if rect is not None else (0, 0)
    nv, tw, th, origin = layout_of(p)
    T = view_table(prev_views, nv)
    c = img[..., :3]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        fin = np.isfinite(c).all(axis=-1)
        miss = g[..., 0] < 0
        acc_m = miss & (hg[..., 0] < 0) & (hg[..., 7] == g[..., 7]) & (hc >= 1) & np.isfinite(hi[..., :3]).all(axis=-1)
        # a hit: the projection
        g7 = g[..., 7]
        vok = (g7 >= 0) & (g7 < F(nv))
        v = np.where(vok, g7, 0).astype(np.int64)
        P = g[..., 4:7]
        twi, s = T["twi"][v], T["c2s"][v]
        ref = np.stack([_row(twi, 0, P), _row(twi, 1, P), _row(twi, 2, P)], axis=-1)
        zok = (ref[..., 2] >= T["near"][v]) & (ref[..., 2] <= T["far"][v]) & (ref[..., 2] > 0)
        d = _row(s, 3, ref)
        uv_p = [(((_row(s, k, ref) / d).astype(F) - T["pp"][v][..., k]).astype(F) * T["res"][v][..., k]).astype(F) for k in (0, 1)]
        a = np.stack([(F(0) * T["ap"][v]).astype(F)] * 2 + [np.zeros((h, w), dtype=F)], axis=-1)
        l = (ref - a).astype(F)
        dist = np.sqrt(fma32(l[..., 2], l[..., 2], fma32(l[..., 1], l[..., 1], (l[..., 0] * l[..., 0]).astype(F)))).astype(F)
        l = (l * (F(1) / dist).astype(F)[..., None]).astype(F)
        inv_f = (F(1) / T["fd"][v]).astype(F)
        f = np.stack([((a[..., k] * inv_f).astype(F) + (l[..., k] / l[..., 2]).astype(F)).astype(F) for k in range(3)], axis=-1)
        uv_t = [(_row(s, k, f) * T["res"][v][..., k]).astype(F) for k in (0, 1)]
        thin = T["type"][v] == 1
        uvx, uvy = np.where(thin, uv_t[0], uv_p[0]).astype(F), np.where(thin, uv_t[1], uv_p[1]).astype(F)
        tx0, ty0 = origin(v)
        ftx, fty = tx0.astype(F), ty0.astype(F)
        sx, sy = ((ftx + uvx).astype(F) - F(.5)).astype(F), ((fty + uvy).astype(F) - F(.5)).astype(F)
        inpos = (sx >= ftx - F(1)) & (sx < ftx + F(tw)) & (sy >= fty - F(1)) & (sy < fty + F(th))
        go = ~miss & vok & zok & inpos
        x0 = np.floor(np.where(go, sx, 0)).astype(np.int64)
        y0 = np.floor(np.where(go, sy, 0)).astype(np.int64)
        ax, ay = (sx - x0.astype(F)).astype(F), (sy - y0.astype(F)).astype(F)
        sw, sn, sc = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F), np.zeros((h, w, 3), dtype=F)
        why = {k: np.zeros((h, w), dtype=bool) for k in ("edge", "shape", "normal", "plane")}
        why["edge"] |= ~miss & vok & zok & ~inpos
        best_w, best_q = np.full((h, w), F(-1)), np.zeros((h, w, 2), dtype=np.int64)
        own_ok = np.zeros((h, w), dtype=bool)   # the tap on the pixel itself was accepted
        n_lo, n_hi = np.full((h, w), F(np.inf)), np.zeros((h, w), dtype=F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = (qx >= tx0) & (qx < tx0 + tw) & (qy >= ty0) & (qy < ty0 + th)
                inside &= (qx >= rx0) & (qx < rx0 + w) & (qy >= ry0) & (qy < ry0 + h)
                lx, ly = np.clip(qx - rx0, 0, w - 1), np.clip(qy - ry0, 0, h - 1)
                gq, cq, nq = hg[ly, lx], hi[ly, lx, :3], hc[ly, lx]
                same_view = go & inside & (gq[..., 7] == g7)
                same_shape = same_view & (gq[..., 0] == g[..., 0])
                usable = same_shape & (nq >= 1) & np.isfinite(cq).all(axis=-1)
                n_ok = usable & ~(_dot(g[..., 1:4], gq[..., 1:4]) < tp.normal_cos)
                e = (gq[..., 4:7] - P).astype(F)
                p_ok = n_ok & ~(np.abs(_dot(g[..., 1:4], e)) > tp.plane_tol)
                ok = p_ok if stops else (go & inside & (gq[..., 7] == g7) & (nq >= 1) & np.isfinite(cq).all(axis=-1))
                own_ok |= ok & (qx == xs + rx0) & (qy == ys + ry0)
                why["edge"] |= go & ~inside
                why["shape"] |= same_view & ~same_shape
                why["normal"] |= usable & ~n_ok
                why["plane"] |= n_ok & ~p_ok
                wgt = ((ax if i else (F(1) - ax).astype(F)) * (ay if j else (F(1) - ay).astype(F))).astype(F)
                better = go & (wgt > best_w)
                best_w = np.where(better, wgt, best_w)
                best_q[better] = np.stack([qx, qy], axis=-1)[better]
                sw = np.where(ok, (sw + wgt).astype(F), sw)
                sc = np.where(ok[..., None], (sc + (wgt[..., None] * cq).astype(F)).astype(F), sc)
                sn = np.where(ok, (sn + (wgt * nq).astype(F)).astype(F), sn)
                n_lo, n_hi = np.where(ok & (nq < n_lo), nq, n_lo), np.where(ok & (nq > n_hi), nq, n_hi)
        got = ~miss & (sw > 0)
        hcol = np.where(got[..., None], (sc / sw[..., None]).astype(F), np.where(acc_m[..., None], hi[..., :3], F(0)))
        mean = (sn / sw).astype(F)
        mean = np.where(mean < n_lo, n_lo, np.where(mean > n_hi, n_hi, mean)).astype(F)
        n_prev = np.where(got, mean, np.where(acc_m, hc, F(0))).astype(F)
        n = (n_prev + F(1)).astype(F)
        n = np.where(n < F(tp.max_history), n, F(tp.max_history)).astype(F)
        alpha = (F(1) / n).astype(F)
        blend = (hcol + (alpha[..., None] * (c - hcol).astype(F)).astype(F)).astype(F)
        use = fin & (n_prev > 0)
        out = img.copy()
        out[..., :3] = np.where(use[..., None], blend, c)
        count = np.where(fin, np.where(use, n, F(1)), F(0)).astype(F)
    if diag is not None:
        hit = fin & ~miss
        diag.update(hit=hit, has=hit & (n_prev > 0), own_ok=hit & own_ok, own=go & (best_q[..., 0] == xs + rx0) & (best_q[..., 1] == ys + ry0),
                    whole=go & (best_w == 1), **{k: m & hit for k, m in why.items()})
    return out, count


# ---------------------------------------------------------------------------------------------------------------
# the cases (tests/test_gpu_temporal.py runs the device over them too)
# ---------------------------------------------------------------------------------------------------------------

class Case:
    """Current and history guide records of one layout, the views of both frames and the layout's parameters."""

    def __init__(self, name, p, views, prev_views, g, hg, tile, keep=()):
        self.name, self.p, self.views, self.prev_views, self.g, self.hg, self.tile, self.keep = name, p, views, prev_views, g, hg, tile, keep

    def planes(self, channels, seed, specials=True):
        """(image, history image, history count): seeded random positive float32; the count takes 0, values below 1,
        integers and fractions; with `specials` NaN and +-inf on hit, miss and tile-border pixels of both images and
        a NaN in the count."""
        rng = np.random.default_rng(seed)
        h, w = self.g.shape[:2]
        img = (rng.random((h, w, channels)) * rng.choice([0.02, 0.5, 3.0], size=(h, w, 1))).astype(F) + F(1e-3)
        hi = (rng.random((h, w, channels)) * rng.choice([0.02, 0.5, 3.0], size=(h, w, 1))).astype(F) + F(1e-3)
        hc = rng.choice(np.array([0, 0.5, 1, 1, 2, 3.25, 7, 31, 40, 70000], dtype=F), size=(h, w)).astype(F)
        if specials:
            vals = [F(np.nan), F(np.inf), F(-np.inf)]
            for k, (plane, rec) in enumerate(((img, self.g), (hi, self.hg))):
                hit, miss = np.argwhere(rec[..., 0] >= 0), np.argwhere(rec[..., 0] < 0)
                spots = [tuple(q) for grp in (hit, miss) if len(grp) for q in grp[(len(grp) // 3 + k)::max(1, len(grp) // 7)][:3]]
                if self.tile:
                    t = self.tile
                    spots += [(min(5, h - 1), t - 1), (min(t, h - 1), min(9, w - 1)), (min(t + 3, h - 1), min(t, w - 1))]
                for i, (y, x) in enumerate(spots):
                    plane[y, x, i % 3] = vals[(i + k) % 3]
            hc[h // 2, w // 2] = F(np.nan)
        return img, hi, hc


def moved(xml, dx, dy):
    out = xml.replace(CAMERA, 'origin="%g, %g, 3.9" target="%g, %g, 0"' % (dx, dy, dx, dy))
    assert out != xml
    return out


def _hits(oracle, s):
    sd, vd, p = s.describe(0, 0, 0)
    return oracle.primary_hits(sd, vd, p), vd, p


def synthetic_case(amvpt_mod, w, h, seed):
    """multisensor = 0 at w x h: a hand-made perspective view (the camera of cbox_path.xml with its resolution set to
    the film's), history records on the plane z = 0 seen through their own pixels, current hit points scattered over
    that plane (so taps land anywhere, outside the film too) and off it (the plane stop), normals tilted up to the
    normal stop and past it, four shape ids with -1 among them in patches."""
    rng = np.random.default_rng(seed)
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_path.xml"), res=40, spp=1)
    _, vd, p0 = s.describe(0, 0, 0)
    view = amvpt_mod.ViewDesc.from_buffer_copy(vd[0])
    view.resolution[0], view.resolution[1] = w, h
    views = (amvpt_mod.ViewDesc * 1)(view)
    p = amvpt_mod.Params.from_buffer_copy(p0)
    p.film_width, p.film_height, p.multisensor, p.n_views = w, h, 0, 1
    assert p.crop_offset_x == p.crop_offset_y == 0
    p.full_width = p.full_height = 0
    s2c = np.array(list(view.sample_to_camera), dtype=np.float64).reshape(4, 4)
    c2w = np.array(list(view.to_world), dtype=np.float64).reshape(4, 4)
    ys, xs = np.mgrid[0:h, 0:w]

    def on_plane(px, py):
        q = s2c @ np.stack([px / w, py / h, np.zeros_like(px), np.ones_like(px)], axis=0).reshape(4, -1)
        dcam = q[:3] / q[3]
        o, dw = c2w[:3, 3:4], c2w[:3, :3] @ dcam
        t = -o[2] / dw[2]
        return (o + dw * t).T.reshape(px.shape + (3,))

    def patches(values, ny, nx):
        grid = rng.choice(values, size=(ny, nx))
        grid.flat[:len(values)] = values
        return grid[np.minimum(ys * ny // h, ny - 1), np.minimum(xs * nx // w, nx - 1)]

    def normals(spread):
        n = np.dstack([rng.normal(0, spread, (h, w)), rng.normal(0, spread, (h, w)), np.ones((h, w))])
        return (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)

    shapes = np.array([-1, 0, 1, 2])
    hg = np.zeros((h, w, 8), dtype=F)
    hg[..., 0] = patches(shapes, 3, 4)
    hg[..., 1:4] = normals(0.15)
    hg[..., 4:7] = (on_plane(xs + 0.5, ys + 0.5) + rng.normal(0, 0.004, (h, w, 3))).astype(F)
    g = np.zeros((h, w, 8), dtype=F)
    g[..., 0] = np.where(rng.random((h, w)) < 0.85, hg[..., 0], patches(shapes, 4, 3))
    g[..., 1:4] = normals(0.2)
    pos = on_plane(xs + 0.5 + rng.uniform(-1.5, 1.5, (h, w)), ys + 0.5 + rng.uniform(-1.5, 1.5, (h, w)))
    pos[..., 2] += rng.choice([0.0, 0.0, 0.01, -0.015, 0.05], size=(h, w))
    g[..., 4:7] = pos.astype(F)
    for rec in (g, hg):
        rec[rec[..., 0] < 0, 1:7] = 0
    return Case("synthetic_%dx%d" % (w, h), p, views, views, g, hg, None, keep=(s,))


SHIFT = (0.25, 0.15)   # of the camera between the history frame and the current one, world units


def build_cases(oracle, amvpt_mod, sizes=((37, 29), (40, 1), (1, 40))):
    """name -> Case.  Oracle records at 64 x 32 (eight views of 16 x 16, or four of 16 x 32): the closed box static and
    with a moved camera, thin-lens views, a reversed cone layout, a batch sensor, an open scene with misses; and
    synthetic single-view records."""
    grid = dict(res=16, gx=4, gy=2)
    out = {}

    def add(name, cur, prev, tile=16):
        (g, vd, p), (hg, pvd, pp) = _hits(oracle, cur), _hits(oracle, prev)
        assert g.shape == hg.shape == (32, 64, 8) and (p.film_width, p.n_views) == (pp.film_width, pp.n_views)
        out[name] = Case(name, p, vd, pvd, g, hg, tile, keep=(cur, prev))

    box = xml_of("cbox_grid.xml")
    static = amvpt_mod.load_string(box, **grid)
    add("cbox_static", static, static)
    add("cbox_moved", static, amvpt_mod.load_string(moved(box, *SHIFT), **grid))
    add("thinlens_moved", amvpt_mod.load_string(box, cam="thinlens", **grid),
        amvpt_mod.load_string(moved(box, *SHIFT), cam="thinlens", **grid))
    cone = xml_of("cbox_cone.xml")
    add("cone_reversed_moved", amvpt_mod.load_string(cone, res=16, revx="true", offx="0.1"),
        amvpt_mod.load_string(moved(cone, *SHIFT), res=16, revx="true", offx="0.1"))
    batch = xml_of("cbox_batch.xml")
    turned = batch.replace('target="0, 0, 0"', 'target="0.7, 0.3, 0"')
    assert turned != batch
    add("batch_turned", amvpt_mod.load_string(batch, res=32, width=64), amvpt_mod.load_string(turned, res=32, width=64))
    # the closed box with a sphere in it: a curved surface, where the plane tolerance is the stop that decides
    ball = box.replace("</scene>", '<shape type="sphere"><point name="center" x="0.35" y="-0.1" z="0.3"/>'
                       '<float name="radius" value="0.4"/><ref id="green"/></shape>\n</scene>')
    add("cbox_sphere_moved", amvpt_mod.load_string(ball, **grid), amvpt_mod.load_string(moved(ball, *SHIFT), **grid))
    opened = open_scene_xml()
    add("open_static", amvpt_mod.load_string(opened, **grid), amvpt_mod.load_string(opened, **grid))
    add("open_moved", amvpt_mod.load_string(opened, **grid), amvpt_mod.load_string(moved(opened, *SHIFT), **grid))
    assert (out["open_moved"].g[..., 0] < 0).any() and out["cone_reversed_moved"].p.reverse_x == 1
    assert out["cone_reversed_moved"].p.reverse_y == 1 and out["batch_turned"].p.batch == 1
    assert out["thinlens_moved"].views[0].type == 1
    for i, (w, h) in enumerate(sizes):
        c = synthetic_case(amvpt_mod, w, h, 50 + i)
        out[c.name] = c
    return out


@pytest.fixture(scope="module")
def cases(oracle, amvpt_mod):
    return build_cases(oracle, amvpt_mod)


ORACLE_CASES = ["cbox_static", "cbox_moved", "cbox_sphere_moved", "thinlens_moved", "cone_reversed_moved", "batch_turned", "open_static", "open_moved"]
CASE_NAMES = ORACLE_CASES + ["synthetic_37x29", "synthetic_40x1", "synthetic_1x40"]


def _assert_same(got, want, what):
    same = bits(got) == bits(want)
    assert same.all(), "%s: %d of %d floats differ, first at %s" % (what, (~same).sum(), same.size, np.argwhere(~same)[:3].tolist())


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------

def test_versions_and_defaults(amvpt_mod):
    assert amvpt_mod.temporal_version() == 1
    assert amvpt_mod.hip_lib().amvpt_abi_version() == 12
    d = amvpt_mod.temporal_default_params()
    assert d.values() == (32, F(0.02), F(0.9)) and d.values() == amvpt_mod.TemporalParams().values()


def test_header_is_exported(amvpt_mod):
    from test_capi import declared
    path = os.path.join(REPO, "include", "amvpt_temporal.h")
    names = declared(path)
    assert names == ["amvpt_temporal", "amvpt_temporal_default_params", "amvpt_temporal_host", "amvpt_temporal_version"]
    assert all(hasattr(amvpt_mod.hip_lib(), n) for n in names)
    assert re.search(r"#define AMVPT_TEMPORAL_VERSION 1\b", open(path).read())
    assert "amvpt_temporal" not in open(os.path.join(REPO, "include", "amvpt_host.h")).read()


def test_fma_restatement():
    """fma32 against exact rational arithmetic, on operands made to cancel and to land on rounding ties."""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = rng.standard_normal(4000).astype(F)
    b = rng.standard_normal(4000).astype(F)
    c = np.concatenate([rng.standard_normal(1000), -(a[1000:2000].astype(np.float64) * b[1000:2000]),
                        np.ldexp(rng.integers(1, 2 ** 24, 1000) * 2 + 1, -25) * 3, rng.standard_normal(1000) * 1e-6]).astype(F)
    got = fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F(float(exact))               # within one float32 step of the rounding of `exact`
        cand = [np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
        err = [abs(Fraction(float(v)) - exact) for v in cand]
        best = min(err)
        winners = [v for v, e in zip(cand, err) if e == best]
        want = winners[0] if len(winners) == 1 else [v for v in winners if (int(np.asarray(v, dtype=F).view(np.uint32)) & 1) == 0][0]
        assert bits(got[i]) == bits(want), (i, a[i], b[i], c[i])


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_equals_the_restatement(amvpt_mod, cases, name, channels):
    k = cases[name]
    img, hi, hc = k.planes(channels, 100 + channels)
    assert not np.isfinite(img).all() and not np.isfinite(hi).all()
    for tp in (amvpt_mod.TemporalParams(), amvpt_mod.TemporalParams(4, 0.005, 0.99), amvpt_mod.TemporalParams(65535, 0.3, -1.0)):
        got = amvpt_mod.temporal_host(img, k.g, hi, k.hg, hc, k.prev_views, k.p, tp)
        want = restated(img, k.g, hi, k.hg, hc, k.prev_views, k.p, tp)
        _assert_same(got[0], want[0], "%s image %r" % (name, tp))
        _assert_same(got[1], want[1], "%s count %r" % (name, tp))
        if channels == 4:
            assert np.array_equal(bits(got[0][..., 3]), bits(img[..., 3]))
    assert not np.array_equal(got[0][..., :3], img[..., :3]) and (got[1] > 1).any()


def _regime(k, tp, seed=5):
    img, hi, hc = k.planes(3, seed, specials=False)
    hc = np.maximum(hc, F(1))   # every history pixel usable: the stops alone decide
    d = {}
    restated(img, k.g, hi, k.hg, hc, k.prev_views, k.p, tp, diag=d)
    n = d["hit"].sum()
    return {key: d[key].sum() / n for key in ("has", "own", "own_ok", "edge", "shape", "normal", "plane")}


def test_regimes(amvpt_mod, cases):
    """No case passes empty.  Fractions of the hit pixels, from the restatement alone: a pixel counts for a stop when
    that stop is the one that turns down at least one of its taps (the stops before it passed), for the tile edge
    when its position or one of its taps lies outside the tile.
    Measured at SHIFT = (0.25, 0.15): see the assertion messages of a run with -s."""
    tp = amvpt_mod.TemporalParams()
    for name in CASE_NAMES:
        print(name, {k: round(float(v), 4) for k, v in _regime(cases[name], tp).items()})
    for name in ("cbox_moved", "cbox_sphere_moved", "thinlens_moved", "cone_reversed_moved", "batch_turned", "open_moved"):
        r = _regime(cases[name], tp)
        assert 0.20 <= r["has"] <= 0.95 and r["shape"] >= 0.01, (name, r)
    # the tile edge: every moved case but the open scene, whose sphere and light sit in the middle of each view with
    # background around them (measured there: edge 0.0, has 0.7975, shape 0.5092, plane 0.4847)
    for name in ("cbox_moved", "cbox_sphere_moved", "thinlens_moved", "cone_reversed_moved", "batch_turned"):
        assert _regime(cases[name], tp)["edge"] >= 0.01, name
    # the moved-camera case of all three stops: the plane tolerance decides on a curved surface
    r = _regime(cases["cbox_sphere_moved"], tp)
    assert r["edge"] >= 0.01 and r["shape"] >= 0.01 and r["plane"] >= 0.01, r
    assert _regime(cases["open_moved"], tp)["plane"] >= 0.01 and _regime(cases["synthetic_37x29"], tp)["plane"] >= 0.01
    # a static camera: every hit pixel reprojects into itself, and rounding of the hit points costs no pixel its history
    for name in ("cbox_static", "open_static"):
        r = _regime(cases[name], tp)
        assert r["own"] >= 0.99 and r["own_ok"] >= 0.99, (name, r)


# ---------------------------------------------------------------------------------------------------------------
# 2. what the definition promises
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cbox_moved", "open_moved", "synthetic_37x29"])
def test_an_empty_history_gives_the_current_image(amvpt_mod, cases, name):
    k = cases[name]
    for channels in (3, 4):
        img, hi, _ = k.planes(channels, 7, specials=False)
        out, cnt = amvpt_mod.temporal_host(img, k.g, hi, k.hg, np.zeros(k.g.shape[:2], dtype=F), k.prev_views, k.p)
        assert np.array_equal(bits(out), bits(img)) and (cnt == 1).all()


def _call_host(amvpt_mod, k, img, hi, hc, tp, rect=None):
    """The C entry on buffers with guard floats behind both outputs -> (status, image, count, both buffers)."""
    L = amvpt_mod.hip_lib()
    n, m = img.size, hc.size
    out, cnt = np.full(n + GUARD, SENTINEL, dtype=F), np.full(m + GUARD, SENTINEL, dtype=F)
    rc = L.amvpt_temporal_host(img.ctypes.data, img.shape[2], k.g.ctypes.data, hi.ctypes.data, k.hg.ctypes.data, hc.ctypes.data,
                               ctypes.cast(k.prev_views, ctypes.c_void_p), ctypes.byref(k.p), rect, ctypes.byref(tp),
                               out.ctypes.data, cnt.ctypes.data)
    return rc, out[:n].reshape(img.shape), cnt[:m].reshape(hc.shape), out, cnt


@pytest.mark.parametrize("name", ["open_moved", "synthetic_37x29"])
def test_nothing_else_is_touched(amvpt_mod, cases, name):
    k = cases[name]
    tp = amvpt_mod.TemporalParams()
    for channels in (3, 4):
        img, hi, hc = k.planes(channels, 31)
        before = [a.copy() for a in (img, hi, hc, k.g, k.hg)]
        views0 = bytes(ctypes.string_at(k.prev_views, ctypes.sizeof(amvpt_mod.ViewDesc) * (k.p.n_views if k.p.multisensor else 1)))
        bad = ~np.isfinite(img[..., :3]).all(axis=-1)
        assert 3 <= bad.sum() <= 9
        rc, res, cnt, out, cbuf = _call_host(amvpt_mod, k, img, hi, hc, tp)
        assert rc == 0
        assert np.array_equal(bits(res[bad]), bits(img[bad])) and (cnt[bad] == 0).all(), "a centre that is not finite passes through"
        assert np.isfinite(res[~bad]).all() and (cnt[~bad] >= 1).all(), "a pixel that is not finite contaminated another"
        assert (out[img.size:] == SENTINEL).all() and (cbuf[hc.size:] == SENTINEL).all()
        for a, b in zip((img, hi, hc, k.g, k.hg), before):
            assert np.array_equal(bits(a), bits(b))
        assert views0 == bytes(ctypes.string_at(k.prev_views, len(views0)))
        want = restated(img, k.g, hi, k.hg, hc, k.prev_views, k.p, tp)
        _assert_same(res, want[0], "image")
        _assert_same(cnt, want[1], "count")


def test_a_rectangle_of_whole_tiles(amvpt_mod, cases):
    """No tap crosses a view: the stage over the rectangle of some whole tiles gives that part of the whole result."""
    for name, rect in (("cbox_moved", (16, 16, 32, 16)), ("cone_reversed_moved", (48, 0, 16, 32)), ("batch_turned", (16, 0, 32, 32))):
        k = cases[name]
        img, hi, hc = k.planes(3, 9)
        whole = amvpt_mod.temporal_host(img, k.g, hi, k.hg, hc, k.prev_views, k.p)
        x0, y0, w, h = rect
        cut = (slice(y0, y0 + h), slice(x0, x0 + w))
        part = amvpt_mod.temporal_host(img[cut], k.g[cut], hi[cut], k.hg[cut], hc[cut], k.prev_views, k.p, rect=rect)
        _assert_same(part[0], whole[0][cut], name)
        _assert_same(part[1], whole[1][cut], name)
        want = restated(img[cut], k.g[cut], hi[cut], k.hg[cut], hc[cut], k.prev_views, k.p, amvpt_mod.TemporalParams(), rect=rect)
        _assert_same(part[0], want[0], name + " restated")


@pytest.fixture(scope="module")
def static_frames(oracle, amvpt_mod):
    """cbox_path.xml at 64 x 64: eight frames of 1 spp with consecutive seeds, their guide records and views."""
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_path.xml"), res=64)
    frames = []
    for seed in range(8):
        sd, vd, p = s.describe(0, seed, 1)
        film, _, _ = oracle.render(sd, vd, p, threads=min(16, os.cpu_count() or 4))
        frames.append(oracle.develop(film, bool(p.film_alpha)).astype(F))
    return s, frames, oracle.primary_hits(sd, vd, p), vd, p


def _accumulate(amvpt_mod, frames, g, vd, p, tp):
    hi, hc = np.zeros_like(frames[0]), np.zeros(g.shape[:2], dtype=F)
    for f in frames:
        hi, hc = amvpt_mod.temporal_host(f, g, hi, g, hc, vd, p, tp)
    return hi, hc


def test_static_camera_averages_the_frames(amvpt_mod, static_frames):
    _, frames, g, vd, p = static_frames
    assert (p.multisensor, p.film_width, p.film_height) == (0, 64, 64) and np.isfinite(np.array(frames)).all()
    out, cnt = _accumulate(amvpt_mod, frames, g, vd, p, amvpt_mod.TemporalParams(max_history=32))
    d = {}
    restated(frames[0], g, frames[1], g, np.ones(g.shape[:2], dtype=F), vd, p, amvpt_mod.TemporalParams(), diag=d)
    whole = d["whole"] & d["own"]
    print("static camera: %d of %d pixels put their whole weight on themselves; counts %s" % (
        whole.sum(), whole.size, np.unique(cnt).tolist()))
    assert whole.sum() > 0.05 * whole.size
    mean = np.mean(np.array(frames, dtype=np.float64), axis=0)
    assert (np.abs(out[whole] - mean[whole]) <= 1e-5 * np.abs(mean[whole])).all()
    assert (cnt == 8).all()
    _, cnt4 = _accumulate(amvpt_mod, frames, g, vd, p, amvpt_mod.TemporalParams(max_history=4))
    assert (cnt4 == 4).all()


# ---------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------

ARGS = ("image", "channels", "guides", "hist_image", "hist_guides", "hist_count", "prev_views", "params", "rect", "tp",
        "out_image", "out_count")


def refusal_rows(amvpt_mod, base, n_img, n_px):
    """(row id, changed arguments, status, what the message must name): one row per refusal of the header.  `base`
    holds the valid arguments (addresses, or ctypes objects for params, rect and tp).  Shared with the device test."""
    T = amvpt_mod.TemporalParams

    def par(**kw):
        q = amvpt_mod.Params.from_buffer_copy(base["params"])
        for key, val in kw.items():
            setattr(q, key, val)
        return q

    f4 = 4
    rows = [("null_" + a, {a: None}, 1, "null " + a) for a in ARGS if a not in ("channels", "rect")]
    rows += [("channels_2", dict(channels=2), 1, "channels"), ("channels_5", dict(channels=5), 1, "channels"),
             ("width_0", dict(params=par(film_width=0)), 1, "film_width"), ("height_0", dict(params=par(film_height=0)), 1, "film_height"),
             ("width_above_2_24", dict(params=par(film_width=(1 << 24) + 1)), 1, "above 2^24"),
             ("height_above_2_24", dict(params=par(film_height=(1 << 24) + 1)), 1, "above 2^24"),
             ("history_0", dict(tp=T(max_history=0)), 1, "max_history"), ("history_65536", dict(tp=T(max_history=65536)), 1, "max_history"),
             ("cos_above", dict(tp=T(normal_cos=1.5)), 1, "normal_cos"), ("cos_below", dict(tp=T(normal_cos=-1.5)), 1, "normal_cos"),
             ("cos_nan", dict(tp=T(normal_cos=float("nan"))), 1, "normal_cos")]
    for label, v in (("zero", 0.0), ("negative", -1.0), ("nan", float("nan")), ("inf", float("inf"))):
        rows.append(("plane_tol_" + label, dict(tp=T(plane_tol=v)), 1, "plane_tol"))
    rows += [("rect_empty", dict(rect=(amvpt_mod.u32 * 4)(0, 0, 0, 8)), 1, "rect"),
             ("rect_outside", dict(rect=(amvpt_mod.u32 * 4)(8, 0, 16, 8)), 1, "rect"),
             ("rect_part_of_a_tile", dict(rect=(amvpt_mod.u32 * 4)(0, 0, 4, 8)), 1, "rect")]
    for out, n_out in (("out_image", n_img), ("out_count", n_px)):
        for name, n_in in (("image", n_img), ("guides", 8 * n_px), ("hist_image", n_img), ("hist_guides", 8 * n_px), ("hist_count", n_px)):
            rows.append(("%s_on_%s" % (out, name), {out: base[name] + f4 * (n_in - 1)}, 1, "%s overlaps" % out))
    rows.append(("out_image_on_out_count", dict(out_count=base["out_image"] + f4), 1, "out_image overlaps out_count"))
    rows += [("crop_offset", dict(params=par(crop_offset_x=1)), 4, "crop"), ("crop_offset_y", dict(params=par(crop_offset_y=2)), 4, "crop"),
             ("full_width", dict(params=par(full_width=32)), 4, "crop"), ("full_height", dict(params=par(full_height=9)), 4, "crop"),
             ("grid_does_not_divide", dict(params=par(film_width=15, full_width=0)), 4, "multiple"),
             ("grid_rows_do_not_divide", dict(params=par(grid_y=3, n_views=6)), 4, "multiple"),
             ("views_not_the_grid", dict(params=par(n_views=3)), 4, "n_views"),
             ("batch_does_not_divide", dict(params=par(batch=1, n_views=3)), 4, "multiple")]
    return rows


def refusal_base(amvpt_mod):
    """A valid 16 x 8 call of two views side by side: (numpy planes, params, views)."""
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=8, gx=2, gy=1)
    _, vd, p = s.describe(0, 0, 0)
    assert (p.film_width, p.film_height, p.n_views) == (16, 8, 2)
    rng = np.random.default_rng(2)
    g = np.zeros((8, 16, 8), dtype=F)
    g[..., 7] = np.repeat([0, 1], 8)[None, :]
    g[..., 3] = 1
    img, hi = rng.random((8, 16, 3)).astype(F), rng.random((8, 16, 3)).astype(F)
    return s, vd, p, dict(image=img, guides=g, hist_image=hi, hist_guides=g.copy(), hist_count=np.ones((8, 16), dtype=F))


def call_with(fn, a, stream=False):
    ref = lambda v: ctypes.byref(v) if v is not None else None   # noqa: E731
    args = [a["image"], a["channels"], a["guides"], a["hist_image"], a["hist_guides"], a["hist_count"],
            ctypes.cast(a["prev_views"], ctypes.c_void_p) if a["prev_views"] is not None else None, ref(a["params"]), ref(a["rect"]),
            ref(a["tp"]), a["out_image"], a["out_count"]]
    return fn(*(args + [None] if stream else args))


def test_refusals(amvpt_mod):
    L = amvpt_mod.hip_lib()
    s, vd, p, planes = refusal_base(amvpt_mod)
    out, cnt = np.full(planes["image"].size, SENTINEL, dtype=F), np.full(128, SENTINEL, dtype=F)
    base = dict({k: v.ctypes.data for k, v in planes.items()}, channels=3, prev_views=vd, params=p, rect=None,
                tp=amvpt_mod.TemporalParams(), out_image=out.ctypes.data, out_count=cnt.ctypes.data)
    assert call_with(L.amvpt_temporal_host, base) == 0
    assert call_with(L.amvpt_temporal_host, dict(base, rect=(amvpt_mod.u32 * 4)(8, 0, 8, 8))) == 0
    out[:] = SENTINEL
    cnt[:] = SENTINEL
    rows = refusal_rows(amvpt_mod, base, planes["image"].size, 128)
    assert len(rows) == 47
    for rid, change, status, names in rows:
        rc = call_with(L.amvpt_temporal_host, dict(base, **change))
        msg = L.amvpt_last_error().decode()
        assert rc == status, (rid, rc, msg)
        assert msg.startswith("amvpt_temporal_host: ") and names in msg, (rid, msg)
    assert (out == SENTINEL).all() and (cnt == SENTINEL).all(), "a refused call wrote"
    # buffers that touch without overlapping are accepted
    both = np.full(planes["image"].size + 128, SENTINEL, dtype=F)
    assert call_with(L.amvpt_temporal_host, dict(base, out_image=both.ctypes.data, out_count=both.ctypes.data + 4 * planes["image"].size)) == 0


def test_python_layer_checks_shapes(amvpt_mod):
    s, vd, p, planes = refusal_base(amvpt_mod)
    a = dict(planes)
    with pytest.raises(ValueError, match="guide records of its size"):
        amvpt_mod.temporal_host(np.zeros((8, 15, 3), dtype=F), a["guides"], a["hist_image"], a["hist_guides"], a["hist_count"], vd, p)
    with pytest.raises(ValueError, match="history planes"):
        amvpt_mod.temporal_host(a["image"], a["guides"], a["hist_image"][:4], a["hist_guides"], a["hist_count"], vd, p)
    with pytest.raises(RuntimeError, match="amvpt_temporal_host: tp: plane_tol must be finite and above 0"):
        amvpt_mod.temporal_host(a["image"], a["guides"], a["hist_image"], a["hist_guides"], a["hist_count"], vd, p,
                                amvpt_mod.TemporalParams(plane_tol=0.0))
    acc = amvpt_mod.TemporalAccumulator()
    assert acc.params.values() == amvpt_mod.TemporalParams().values() and acc.image is None and acc.frames == 0


def test_display_default_is_unchanged(amvpt_mod):
    """temporal=None is the default and the call without the keyword (the device test compares the bytes)."""
    import amvpt.display as D
    assert inspect.signature(D.display).parameters["temporal"].default is None
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=8, spp=4)
    if amvpt_mod.device_count() <= 0:
        errors = []
        for kw in (dict(), dict(temporal=None)):
            with pytest.raises(RuntimeError) as e:
                D.display(s, size=(16, 8), **kw)
            errors.append(str(e.value))
        assert errors[0] == errors[1]


# ---------------------------------------------------------------------------------------------------------------
# 4. the quality gate, on oracle renders
# ---------------------------------------------------------------------------------------------------------------

STEP = 0.05   # the camera's move per frame along x, world units: 1/40 of the box's width, 2.3 pixels
GATE = 0.68   # halfway between the measured ratio 0.364 and 1


def test_quality_gate(amvpt_mod, oracle):
    """cbox_path.xml at 128 x 128: eight frames of 1 spp (seeds 1 .. 8) while the camera moves by STEP per frame; the
    reference is a 256-spp render (seed 0) from the last camera, the metric test_denoise's relative RMSE.  The gate
    lies halfway between the measured ratio and 1.  The power check: with the current views in place of the previous
    ones (no reprojection) the same gate fails, and without the shape, normal and plane stops (the restatement with
    stops=False: ghosting) the error is larger.
    Measured: raw 0.5220, accumulated 0.1899 (ratio 0.364, mean count 7.43); without the stops 0.2232 (0.428); without
    reprojection 0.8165 (1.564: the light's filter footprint trails over the ceiling).  At a step of 0.02 the ratios
    are 0.353, 0.351 and 1.262; at 0.1, 0.449, 0.555 and 1.788."""
    threads = min(16, os.cpu_count() or 4)
    xml = xml_of("cbox_path.xml")
    cam = 'origin="0, 0, 3.90" target="0, 0, 0"'
    assert cam in xml
    frames = []
    for i in range(8):
        x = STEP * (i - 7)
        s = amvpt_mod.load_string(xml.replace(cam, 'origin="%g, 0, 3.9" target="%g, 0, 0"' % (x, x)), res=128)
        sd, vd, p = s.describe(0, 1 + i, 1)
        film, _, _ = oracle.render(sd, vd, p, threads=threads)
        frames.append((oracle.develop(film, bool(p.film_alpha)).astype(F), oracle.primary_hits(sd, vd, p), vd, p, s))
    sd, vd, p = frames[-1][4].describe(0, 0, 256)
    film, _, _ = oracle.render(sd, vd, p, threads=threads)
    ref = oracle.develop(film, bool(p.film_alpha)).astype(F)
    tp = amvpt_mod.TemporalParams()

    def run(step_fn, views_of=lambda i: frames[i - 1][2]):
        hi, hg, hc = np.zeros_like(frames[0][0]), frames[0][1], np.zeros(frames[0][1].shape[:2], dtype=F)
        for i, (img, g, vd_i, p_i, _) in enumerate(frames):
            hi, hc = step_fn(img, g, hi, hg, hc, views_of(i) if i else vd_i, p_i, tp)
            hg = g
        return hi, hc

    out, cnt = run(amvpt_mod.temporal_host)
    raw = rel_rmse(frames[-1][0], ref)
    good = rel_rmse(out, ref)
    ghost = rel_rmse(run(lambda *a: restated(*a, stops=False))[0], ref)
    wrong = rel_rmse(run(amvpt_mod.temporal_host, views_of=lambda i: frames[i][2])[0], ref)
    print("cbox_path res=128, 8 x 1 spp, step %.3f: relative RMSE raw %.4f, accumulated %.4f (ratio %.3f, mean count %.2f); "
          "without the stops %.4f (ratio %.3f); with the current views as the previous ones %.4f (ratio %.3f)" % (
              STEP, raw, good, good / raw, cnt.mean(), ghost, ghost / raw, wrong, wrong / raw))
    assert good <= GATE * raw
    assert wrong > GATE * raw, "the power check: the gate must fail without reprojection"
    assert ghost > good, "the power check: the stops must matter"

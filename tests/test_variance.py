"""The variance-guided denoiser on the CPU (include/amvpt_variance.h): its three host entries against numpy float32
restatements of the header's definition, bit for bit; amvpt_temporal_moments_host against amvpt_temporal_host; what the
moments mean on a static camera; what the definition promises about constant regions, values that are not finite and
buffers it must not touch; the refusals; and the quality gates on oracle renders, always against the pipeline this
one stands beside (amvpt_temporal_host -> amvpt_denoise_host at its defaults).  tests/test_gpu_variance.py runs the
device entries over the same cases.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_denoise import HK, rel_rmse
from test_guides import bits, xml_of
from test_temporal import CASE_NAMES, STEP, _dot, _row, build_cases, fma32, layout_of, view_table
from test_temporal import restated as temporal_restated
from test_temporal import static_frames  # noqa: F401 -- the fixture of the static camera's eight frames

F = np.float32
GUARD = 64
SENTINEL = F(-12345.0)
GK = {-1: F(0.25), 0: F(0.5), 1: F(0.25)}
MOVED = ["cbox_moved", "cbox_sphere_moved", "thinlens_moved", "cone_reversed_moved", "batch_turned", "open_moved"]


# ---------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------

def lum(c):
    """(0.2126f*r + 0.7152f*g) + 0.0722f*b, every product and sum rounded to float32."""
    return ((F(0.2126) * c[..., 0]).astype(F) + (F(0.7152) * c[..., 1]).astype(F)).astype(F) + (F(0.0722) * c[..., 2]).astype(F)


def max0(x):
    return np.where(x > 0, x, F(0)).astype(F)


def restated_moments(img, g, hi, hg, hc, hm, prev_views, p, tp, rect=None):
    """amvpt_temporal_moments_host in numpy -> (image, count, moments): amvpt_temporal.h's definition once more, with the
    moments of stage 1 riding its accepted taps.  (Image and count are also compared with test_temporal's restatement.)"""
    img, g, hi, hg, hm = (np.ascontiguousarray(a, dtype=F) for a in (img, g, hi, hg, hm))
    h, w = g.shape[:2]
    hc = np.ascontiguousarray(hc, dtype=F).reshape(h, w)
    rx0, ry0 = (int(rect[0]), int(rect[1])) if rect is not None else (0, 0)
    nv, tw, th, origin = layout_of(p)
    T = view_table(prev_views, nv)
    c = img[..., :3]
    with np.errstate(all="ignore"):
        fin = np.isfinite(c).all(axis=-1)
        l = lum(c)
        m = np.stack([l, (l * l).astype(F)], axis=-1)
        miss = g[..., 0] < 0
        acc_m = miss & (hg[..., 0] < 0) & (hg[..., 7] == g[..., 7]) & (hc >= 1) & np.isfinite(hi[..., :3]).all(axis=-1)
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
        lv = (ref - a).astype(F)
        dist = np.sqrt(fma32(lv[..., 2], lv[..., 2], fma32(lv[..., 1], lv[..., 1], (lv[..., 0] * lv[..., 0]).astype(F)))).astype(F)
        lv = (lv * (F(1) / dist).astype(F)[..., None]).astype(F)
        inv_f = (F(1) / T["fd"][v]).astype(F)
        f = np.stack([((a[..., k] * inv_f).astype(F) + (lv[..., k] / lv[..., 2]).astype(F)).astype(F) for k in range(3)], axis=-1)
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
        sw, sn = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
        sc, sm = np.zeros((h, w, 3), dtype=F), np.zeros((h, w, 2), dtype=F)
        n_lo, n_hi = np.full((h, w), F(np.inf)), np.zeros((h, w), dtype=F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = (qx >= tx0) & (qx < tx0 + tw) & (qy >= ty0) & (qy < ty0 + th)
                inside &= (qx >= rx0) & (qx < rx0 + w) & (qy >= ry0) & (qy < ry0 + h)
                lx, ly = np.clip(qx - rx0, 0, w - 1), np.clip(qy - ry0, 0, h - 1)
                gq, cq, nq, mq = hg[ly, lx], hi[ly, lx, :3], hc[ly, lx], hm[ly, lx]
                ok = go & inside & (gq[..., 7] == g7) & (gq[..., 0] == g[..., 0]) & (nq >= 1) & np.isfinite(cq).all(axis=-1)
                ok &= ~(_dot(g[..., 1:4], gq[..., 1:4]) < tp.normal_cos)
                e = (gq[..., 4:7] - P).astype(F)
                ok &= ~(np.abs(_dot(g[..., 1:4], e)) > tp.plane_tol)
                wgt = ((ax if i else (F(1) - ax).astype(F)) * (ay if j else (F(1) - ay).astype(F))).astype(F)
                sw = np.where(ok, (sw + wgt).astype(F), sw)
                sc = np.where(ok[..., None], (sc + (wgt[..., None] * cq).astype(F)).astype(F), sc)
                sm = np.where(ok[..., None], (sm + (wgt[..., None] * mq).astype(F)).astype(F), sm)
                sn = np.where(ok, (sn + (wgt * nq).astype(F)).astype(F), sn)
                n_lo, n_hi = np.where(ok & (nq < n_lo), nq, n_lo), np.where(ok & (nq > n_hi), nq, n_hi)
        got = ~miss & (sw > 0)
        hcol = np.where(got[..., None], (sc / sw[..., None]).astype(F), np.where(acc_m[..., None], hi[..., :3], F(0)))
        hmom = np.where(got[..., None], (sm / sw[..., None]).astype(F), np.where(acc_m[..., None], hm, F(0)))
        mean = (sn / sw).astype(F)
        mean = np.where(mean < n_lo, n_lo, np.where(mean > n_hi, n_hi, mean)).astype(F)
        n_prev = np.where(got, mean, np.where(acc_m, hc, F(0))).astype(F)
        n = (n_prev + F(1)).astype(F)
        n = np.where(n < F(tp.max_history), n, F(tp.max_history)).astype(F)
        alpha = (F(1) / n).astype(F)
        blend = (hcol + (alpha[..., None] * (c - hcol).astype(F)).astype(F)).astype(F)
        mblend = (hmom + (alpha[..., None] * (m - hmom).astype(F)).astype(F)).astype(F)
        use = fin & (n_prev > 0)
        out = img.copy()
        out[..., :3] = np.where(use[..., None], blend, c)
        count = np.where(fin, np.where(use, n, F(1)), F(0)).astype(F)
        mom = np.where(fin[..., None], np.where(use[..., None], mblend, m), F(0)).astype(F)
    return out, count, mom


def _guide_weight(g, gq, inv_sp, squarings):
    """wn*wp of amvpt_denoise between every pixel's record and its tap's."""
    wn = _dot(g[..., 1:4], gq[..., 1:4]).astype(F)
    wn = np.where(wn > 0, wn, F(0)).astype(F)
    for _ in range(squarings):
        wn = (wn * wn).astype(F)
    e = (gq[..., 4:7] - g[..., 4:7]).astype(F)
    t = (np.abs(_dot(g[..., 1:4], e)).astype(F) * inv_sp).astype(F)
    wp = (F(1) / (F(1) + (t * t).astype(F)).astype(F)).astype(F)
    return (wn * wp).astype(F)


def restated_variance(mom, cnt, g, q, diag=None):
    """amvpt_variance_host in numpy.  `diag` receives the masks of the regime assertions."""
    mom, cnt, g = (np.ascontiguousarray(a, dtype=F) for a in (mom, cnt, g))
    h, w = cnt.shape
    m1, m2 = mom[..., 0], mom[..., 1]
    mh, inv_sp = F(q.min_history), F(1) / F(q.sigma_plane)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        valid = (cnt >= 1) & np.isfinite(m1) & np.isfinite(m2)
        tv = max0((m2 - (m1 * m1).astype(F)).astype(F))
        hit = g[..., 0] >= 0
        s1, s2, sw = (np.zeros((h, w), dtype=F) for _ in range(3))
        why = {k: np.zeros((h, w), dtype=bool) for k in ("edge", "view", "shape", "unusable")}
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                gq, mq, nq = g[qy, qx], mom[qy, qx], cnt[qy, qx]
                same_view = inside & (gq[..., 7] == g[..., 7])
                same_shape = same_view & (gq[..., 0] == g[..., 0])
                ok = same_shape & (nq >= 1) & np.isfinite(mq).all(axis=-1)
                why["edge"] |= ~inside
                why["view"] |= inside & ~same_view
                why["shape"] |= same_view & ~same_shape
                why["unusable"] |= same_shape & ~ok
                wgt = np.where(hit, _guide_weight(g, gq, inv_sp, q.normal_squarings), F(1)).astype(F)
                s1 = np.where(ok, (s1 + (wgt * mq[..., 0]).astype(F)).astype(F), s1)
                s2 = np.where(ok, (s2 + (wgt * mq[..., 1]).astype(F)).astype(F), s2)
                sw = np.where(ok, (sw + wgt).astype(F), sw)
        r = (mh / cnt).astype(F)
        e1, e2 = (s1 / sw).astype(F), (s2 / sw).astype(F)
        spatial = np.where(sw > 0, (max0((e2 - (e1 * e1).astype(F)).astype(F)) * r).astype(F), (tv * r).astype(F))
        long_ = cnt >= mh
        v = np.where(long_, tv, spatial).astype(F)
        var = np.where(valid, (v / cnt).astype(F), F(0)).astype(F)
    if diag is not None:
        short = valid & ~long_
        diag.update(short=short, **{k: m & short for k, m in why.items()})
    return var


def restated_filter_iteration(img, vin, g, step, sl2, var_floor, inv_sp, squarings, diag=None):
    h, w, _ = img.shape
    c = img[..., :3]
    hit = g[..., 0] >= 0
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        sg, sk = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
        taken = np.zeros((h, w), dtype=np.int64)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                gq, vq = g[qy, qx], vin[qy, qx]
                ok = inside & (gq[..., 7] == g[..., 7]) & (gq[..., 0] == g[..., 0]) & np.isfinite(vq)
                kw = F(GK[dy] * GK[dx])
                sg = np.where(ok, (sg + (kw * vq).astype(F)).astype(F), sg)
                sk = np.where(ok, (sk + kw).astype(F), sk)
                taken += ok
        gv = np.where(sk > 0, (sg / sk).astype(F), F(0)).astype(F)
        lp = lum(c)
        kl = (F(1) / ((sl2 * gv).astype(F) + var_floor).astype(F)).astype(F)
        sum_c, sum_w, sum_v = np.zeros((h, w, 3), dtype=F), np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * step, xs + dx * step
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                gq, cq, vq = g[qy, qx], c[qy, qx], vin[qy, qx]
                ok = inside & np.isfinite(cq).all(axis=-1) & (gq[..., 7] == g[..., 7]) & (gq[..., 0] == g[..., 0]) & np.isfinite(vq)
                dl = (lum(cq) - lp).astype(F)
                wl = (F(1) / (F(1) + ((dl * dl).astype(F) * kl).astype(F)).astype(F)).astype(F)
                wgt = (F(HK[dy] * HK[dx]) * wl).astype(F)
                wgt = np.where(hit, (wgt * _guide_weight(g, gq, inv_sp, squarings)).astype(F), wgt)
                sum_c = np.where(ok[..., None], (sum_c + (wgt[..., None] * cq).astype(F)).astype(F), sum_c)
                sum_w = np.where(ok, (sum_w + wgt).astype(F), sum_w)
                sum_v = np.where(ok, (sum_v + ((wgt * wgt).astype(F) * vq).astype(F)).astype(F), sum_v)
        out = img.copy()
        good = sum_w > 0
        out[..., :3] = np.where(good[..., None], (sum_c / sum_w[..., None]).astype(F), c)
        vout = np.where(good, (sum_v / (sum_w * sum_w).astype(F)).astype(F), vin).astype(F)
    if diag is not None:
        diag["alone"] = (taken == 1) & np.isfinite(vin)   # every prefilter tap but the pixel's own was stopped
    return out, vout


def restated_filter(img, var, g, q, diag=None):
    """amvpt_denoise_variance_host in numpy -> the (image, variance) after every iteration 1 .. q.iterations."""
    img, var, g = (np.ascontiguousarray(a, dtype=F) for a in (img, var, g))
    sl2 = F(F(q.sigma_lum) * F(q.sigma_lum))
    inv_sp = F(1) / F(q.sigma_plane)
    steps = []
    for i in range(q.iterations):
        img, var = restated_filter_iteration(img, var, g, 1 << i, sl2, F(q.var_floor), inv_sp, q.normal_squarings,
                                             diag if i == 0 else None)
        steps.append((img, var))
    return steps


# ---------------------------------------------------------------------------------------------------------------
# the cases (tests/test_gpu_variance.py runs the device over them too)
# ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases(oracle, amvpt_mod):
    return build_cases(oracle, amvpt_mod)


def history_moments(k, seed, specials=True):
    """A history of the luminance moments for case k: seeded, positive, M2 above M1^2; with `specials` a NaN, a +inf and
    a -inf on hit, miss and tile-border pixels of the history."""
    rng = np.random.default_rng(seed)
    h, w = k.g.shape[:2]
    m1 = (rng.random((h, w)) * rng.choice([0.02, 0.5, 3.0], size=(h, w))).astype(F) + F(1e-3)
    hm = np.stack([m1, (m1 * m1 * (1 + rng.random((h, w)))).astype(F)], axis=-1).astype(F)
    if specials:
        vals = [F(np.nan), F(np.inf), F(-np.inf)]
        hit, miss = np.argwhere(k.hg[..., 0] >= 0), np.argwhere(k.hg[..., 0] < 0)
        spots = [tuple(q) for grp in (hit, miss) if len(grp) for q in grp[(len(grp) // 4)::max(1, len(grp) // 5)][:3]]
        if k.tile:
            t = k.tile
            spots += [(min(6, h - 1), t - 1), (min(t, h - 1), min(11, w - 1)), (min(t + 2, h - 1), min(t, w - 1))]
        for i, (y, x) in enumerate(spots):
            hm[y, x, i % 2] = vals[i % 3]
    return hm


def seeded_stage2(k, s):
    """Stage 2's inputs with values stage 1 never writes: copies of its moments and count with NaN, +inf, -inf, 0 and
    0.5 in the count and NaN, +inf, -inf in the moments, on hit, miss and tile-border pixels and on the right-hand
    neighbours (same view and shape) of short-history pixels, so that window taps meet them -> (moments, count)."""
    mom, cnt = s["mom"].copy(), s["cnt"].copy()
    g = k.g
    h, w = cnt.shape
    cvals = [F(np.nan), F(np.inf), F(-np.inf), F(0), F(0.5)]
    mvals = [F(np.nan), F(np.inf), F(-np.inf)]
    hit, miss = np.argwhere(g[..., 0] >= 0), np.argwhere(g[..., 0] < 0)
    short = np.argwhere((s["cnt"] >= 1) & (s["cnt"] < 4))
    beside = [(y, x + 1) for y, x in short if x + 1 < w and g[y, x + 1, 0] == g[y, x, 0] and g[y, x + 1, 7] == g[y, x, 7]]
    border = []
    if k.tile:
        t = k.tile
        border = [(min(5, h - 1), t - 1), (min(t, h - 1), min(9, w - 1)), (min(t + 3, h - 1), min(t, w - 1)),
                  (min(t - 1, h - 1), min(t + 1, w - 1)), (min(2, h - 1), min(2 * t, w - 1))]

    def pick(grp, first, n):
        return [tuple(q) for q in grp[first::max(1, len(grp) // (n + 1))][:n]] if len(grp) else []

    for i, (y, x) in enumerate(pick(hit, 1, 5) + pick(miss, 1, 5) + border + pick(beside, 0, 5)):
        cnt[y, x] = cvals[i % 5]
    for i, (y, x) in enumerate(pick(hit, 2, 3) + pick(miss, 2, 3) + [(y, min(x + 2, w - 1)) for y, x in border[:3]] + pick(beside, 1, 3)):
        mom[y, x, i % 2] = mvals[i % 3]
    return mom, cnt


def ringed_variance(var, g, specials=True):
    """`var` with NaN, +inf and -inf on hit, miss and (with views of 16) tile-border pixels, and one pixel whose every
    neighbour is not finite: the prefilter of that pixel has its own tap alone."""
    v = np.array(var, dtype=F)
    h, w = v.shape
    if not specials:
        return v
    vals = [F(np.nan), F(np.inf), F(-np.inf)]
    hit, miss = np.argwhere(g[..., 0] >= 0), np.argwhere(g[..., 0] < 0)
    spots = [tuple(q) for grp in (hit, miss) if len(grp) for q in grp[(len(grp) // 5)::max(1, len(grp) // 6)][:3]]
    if h > 17 and w > 17:
        spots += [(3, 15), (16, 7), (17, 16)]
    for i, (y, x) in enumerate(spots):
        v[y, x] = vals[i % 3]
    cy, cx = (h * 2) // 3, (w * 2) // 3
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y, x = cy + dy, cx + dx
            if (dy or dx) and 0 <= y < h and 0 <= x < w:
                v[y, x] = vals[(dy + dx) % 3]
    v[cy, cx] = F(0.25)
    return v


def stage_inputs(amvpt_mod, k, channels, seed=100, specials=True):
    """The three stages' inputs for case k: the planes of test_temporal's Case, a history of moments, and the outputs
    of stage 1 (host entry) that stages 2 and 3 work on."""
    img, hi, hc = k.planes(channels, seed + channels, specials=specials)
    hm = history_moments(k, seed + 7, specials=specials)
    out, cnt, mom = amvpt_mod.temporal_moments_host(img, k.g, hi, k.hg, hc, hm, k.prev_views, k.p)
    return dict(img=img, hi=hi, hc=hc, hm=hm, out=out, cnt=cnt, mom=mom)


def _assert_same(got, want, what):
    same = bits(got) == bits(want)
    assert same.all(), "%s: %d of %d floats differ, first at %s" % (what, (~same).sum(), same.size, np.argwhere(~same)[:3].tolist())


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatements, bit for bit, and equality with the parent stage
# ---------------------------------------------------------------------------------------------------------------

def test_versions_and_defaults(amvpt_mod):
    assert amvpt_mod.variance_version() == 1
    assert amvpt_mod.hip_lib().amvpt_abi_version() == 12
    assert amvpt_mod.temporal_version() == 1 and amvpt_mod.denoise_version() == 1
    d = amvpt_mod.variance_default_params()
    assert d.values() == (4, 2.0, F(1e-8), F(0.05), 5, 4) and d.values() == amvpt_mod.VarianceParams().values()


def test_header_is_exported(amvpt_mod):
    from test_capi import declared
    path = os.path.join(REPO, "include", "amvpt_variance.h")
    names = declared(path)
    assert names == ["amvpt_denoise_variance", "amvpt_denoise_variance_host", "amvpt_temporal_moments",
                     "amvpt_temporal_moments_host", "amvpt_variance", "amvpt_variance_default_params", "amvpt_variance_host",
                     "amvpt_variance_version"]
    assert all(hasattr(amvpt_mod.hip_lib(), n) for n in names)
    assert re.search(r"#define AMVPT_VARIANCE_VERSION 1\b", open(path).read())
    assert "amvpt_variance" not in open(os.path.join(REPO, "include", "amvpt_host.h")).read()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_temporal_moments(amvpt_mod, cases, name, channels):
    """Stage 1 equals its restatement, and its image and count equal amvpt_temporal_host's and test_temporal's
    restatement of that, on every float."""
    k = cases[name]
    img, hi, hc = k.planes(channels, 100 + channels)
    hm = history_moments(k, 107)
    assert not np.isfinite(img).all() and not np.isfinite(hi).all() and not np.isfinite(hm).all()
    for tp in (amvpt_mod.TemporalParams(), amvpt_mod.TemporalParams(4, 0.005, 0.99), amvpt_mod.TemporalParams(65535, 0.3, -1.0)):
        got = amvpt_mod.temporal_moments_host(img, k.g, hi, k.hg, hc, hm, k.prev_views, k.p, tp)
        want = restated_moments(img, k.g, hi, k.hg, hc, hm, k.prev_views, k.p, tp)
        parent = amvpt_mod.temporal_host(img, k.g, hi, k.hg, hc, k.prev_views, k.p, tp)
        old = temporal_restated(img, k.g, hi, k.hg, hc, k.prev_views, k.p, tp)
        for i, plane in enumerate(("image", "count", "moments")):
            _assert_same(got[i], want[i], "%s %s %r" % (name, plane, tp))
        for i, plane in enumerate(("image", "count")):
            _assert_same(got[i], parent[i], "%s %s against amvpt_temporal_host %r" % (name, plane, tp))
            _assert_same(got[i], old[i], "%s %s against test_temporal's restatement %r" % (name, plane, tp))
        bad = ~np.isfinite(img[..., :3]).all(axis=-1)
        assert bad.any() and (got[2][bad] == 0).all() and (got[1][bad] == 0).all()
    blended = got[1] > 1
    assert blended.any() and (got[2][blended] != 0).any()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_variance_and_filter(amvpt_mod, cases, name, channels):
    """Stages 2 and 3 equal their restatements: min_history 1, 4 and 9; iterations 1 to 5 (the restatement runs once
    and is compared after every iteration); other parameters."""
    k = cases[name]
    s = stage_inputs(amvpt_mod, k, channels)
    variances = {}
    for mh in (1, 4, 9):
        q = amvpt_mod.VarianceParams(min_history=mh)
        got = amvpt_mod.variance_host(s["mom"], s["cnt"], k.g, q)
        _assert_same(got, restated_variance(s["mom"], s["cnt"], k.g, q), "%s variance min_history %d" % (name, mh))
        assert np.isfinite(got).all() and (got >= 0).all()
        variances[mh] = got
    if min(k.g.shape[:2]) > 1:
        assert not np.array_equal(variances[1], variances[9])
    # a count and moments stage 1 never writes: NaN, infinities, 0 and 0.5, beside short histories too
    mom2, cnt2 = seeded_stage2(k, s)
    assert np.isnan(cnt2).any() and np.isposinf(cnt2).any() and np.isneginf(cnt2).any() and (cnt2 == F(0.5)).any()
    for mh in (1, 4, 9):
        q = amvpt_mod.VarianceParams(min_history=mh)
        d = {}
        got = amvpt_mod.variance_host(mom2, cnt2, k.g, q)
        _assert_same(got, restated_variance(mom2, cnt2, k.g, q, diag=d), "%s variance of a seeded count, min_history %d" % (name, mh))
        assert np.isfinite(got).all() and (got >= 0).all(), "a count or moment that is not finite reached another pixel's variance"
        assert (got[~(cnt2 >= 1) | np.isposinf(cnt2) | ~np.isfinite(mom2).all(axis=-1)] == 0).all()
    if name in MOVED:
        assert d["unusable"].sum() >= 1, "no window met a tap with an unusable count or moment"
    q = amvpt_mod.VarianceParams(sigma_plane=0.011, normal_squarings=0, min_history=65535)
    _assert_same(amvpt_mod.variance_host(s["mom"], s["cnt"], k.g, q), restated_variance(s["mom"], s["cnt"], k.g, q), name + " other")
    var = ringed_variance(variances[4], k.g)
    assert not np.isfinite(var).all() and not np.isfinite(s["out"]).all()
    want = restated_filter(s["out"], var, k.g, amvpt_mod.VarianceParams(iterations=5))
    for it in range(1, 6):
        got = amvpt_mod.denoise_variance_host(s["out"], var, k.g, amvpt_mod.VarianceParams(iterations=it))
        _assert_same(got[0], want[it - 1][0], "%s image after %d iterations" % (name, it))
        _assert_same(got[1], want[it - 1][1], "%s variance after %d iterations" % (name, it))
        if channels == 4:
            assert np.array_equal(bits(got[0][..., 3]), bits(s["out"][..., 3]))
    assert not np.array_equal(want[0][0][..., :3], s["out"][..., :3])
    for q in (amvpt_mod.VarianceParams(8, 0.3, 0.5, 0.011, 0, 4), amvpt_mod.VarianceParams(2, 7.0, 1e-4, 3.0, 7, 4)):
        got = amvpt_mod.denoise_variance_host(s["out"], var, k.g, q)
        want_q = restated_filter(s["out"], var, k.g, q)[-1]
        _assert_same(got[0], want_q[0], "%s image %r" % (name, q))
        _assert_same(got[1], want_q[1], "%s variance %r" % (name, q))


def test_regimes(amvpt_mod, cases):
    """No case passes empty, from the restatements alone.  In the moved-camera cases some pixels have a history shorter
    than min_history and take the 7 x 7 branch, and some of those have a window tap stopped by the view, by the shape
    and by the image edge; in every case at least one pixel has every prefilter tap but its own stopped."""
    q = amvpt_mod.VarianceParams()
    for name in CASE_NAMES:
        k = cases[name]
        s = stage_inputs(amvpt_mod, k, 3)
        d, e = {}, {}
        var = restated_variance(s["mom"], s["cnt"], k.g, q, diag=d)
        restated_filter(s["out"], ringed_variance(var, k.g), k.g, amvpt_mod.VarianceParams(iterations=1), diag=e)
        print(name, {key: int(m.sum()) for key, m in d.items()}, "alone", int(e["alone"].sum()))
        assert e["alone"].sum() >= 1, name
        if name in MOVED:
            assert d["short"].sum() >= 20 and d["view"].sum() >= 1 and d["shape"].sum() >= 1 and d["edge"].sum() >= 1, (name, d)
        # the history planes are random: also a real short history, the count a first and a second frame leave
        cnt = np.where(k.g[..., 0] == k.hg[..., 0], F(2), F(1))
        d2 = {}
        restated_variance(s["mom"], cnt, k.g, q, diag=d2)
        assert d2["short"].mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------
# 2. what the moments mean
# ---------------------------------------------------------------------------------------------------------------

def test_static_camera_moments_are_the_mean_and_the_variance(amvpt_mod, static_frames):  # noqa: F811
    """Eight 1-spp frames of a static camera: on the pixels that put their whole weight on themselves M1 and M2 are the
    float64 means of l and l^2 within 1e-5 relative (the bar of test_static_camera_averages_the_frames), and 8 * var is
    the float64 population variance within 64 * 2^-24 * M2: eight blends of about four roundings each, relative to the
    larger term of a cancelling difference, doubled."""
    _, frames, g, vd, p = static_frames
    tp = amvpt_mod.TemporalParams(max_history=32)
    hi, hc, hm = np.zeros_like(frames[0]), np.zeros(g.shape[:2], dtype=F), np.zeros(g.shape[:2] + (2,), dtype=F)
    for f in frames:
        hi, hc, hm = amvpt_mod.temporal_moments_host(f, g, hi, g, hc, hm, vd, p, tp)
    assert (hc == 8).all()
    d = {}
    temporal_restated(frames[0], g, frames[1], g, np.ones(g.shape[:2], dtype=F), vd, p, amvpt_mod.TemporalParams(), diag=d)
    whole = d["whole"] & d["own"]
    assert whole.sum() > 0.05 * whole.size
    fr = np.array(frames, dtype=np.float64)[..., :3]
    l = 0.2126 * fr[..., 0] + 0.7152 * fr[..., 1] + 0.0722 * fr[..., 2]
    mean1, mean2 = l.mean(axis=0), (l * l).mean(axis=0)
    assert (np.abs(hm[..., 0] - mean1)[whole] <= 1e-5 * np.abs(mean1[whole])).all()
    assert (np.abs(hm[..., 1] - mean2)[whole] <= 1e-5 * np.abs(mean2[whole])).all()
    var = amvpt_mod.variance_host(hm, hc, g)
    pop = mean2 - mean1 * mean1
    err = np.abs(var.astype(np.float64) * 8 - pop)[whole]
    bound = 64 * 2.0 ** -24 * mean2[whole]
    print("static camera: %d pixels; largest error of 8 var %.3e at a bound of %.3e; largest share of the bound %.3f" % (
        whole.sum(), err.max(), bound[err.argmax()], (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all() and pop[whole].max() > 0


# ---------------------------------------------------------------------------------------------------------------
# 3. what the definition promises
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cbox_moved", "open_moved", "synthetic_37x29"])
def test_constant_regions_stay_put(amvpt_mod, cases, name):
    """One power of two per (view, shape) region comes out exactly equal, whatever the variance plane holds."""
    g = cases[name].g
    region = g[..., 7].astype(int) * 64 + g[..., 0].astype(int) + 1
    ids = np.unique(region)
    assert 4 <= len(ids) <= 128
    expo = np.searchsorted(ids, region) - len(ids) // 2
    img = np.repeat(np.ldexp(F(1), expo).astype(F)[..., None], 4, axis=-1)
    rng = np.random.default_rng(3)
    h, w = g.shape[:2]
    planes = [np.zeros((h, w), dtype=F), rng.random((h, w)).astype(F), np.full((h, w), F(3e37)),
              ringed_variance(rng.random((h, w)).astype(F) * F(1e-6), g)]
    for var in planes:
        for c in (3, 4):
            out, _ = amvpt_mod.denoise_variance_host(img[..., :c], var, g, amvpt_mod.VarianceParams(iterations=5))
            assert np.array_equal(out, img[..., :c])


def _call_filter(amvpt_mod, img, var, g, q, with_scratch=True, with_var_out=True):
    """amvpt_denoise_variance_host on buffers with guard floats behind all four outputs."""
    L = amvpt_mod.hip_lib()
    h, w, c = img.shape
    n, m = h * w * c, h * w
    bufs = [np.full(n + GUARD, SENTINEL, dtype=F), np.full(n + GUARD, SENTINEL, dtype=F) if with_scratch else None,
            np.full(m + GUARD, SENTINEL, dtype=F) if with_var_out else None, np.full(m + GUARD, SENTINEL, dtype=F) if with_scratch else None]
    ptr = [b.ctypes.data if b is not None else None for b in bufs]
    rc = L.amvpt_denoise_variance_host(img.ctypes.data, c, w, h, var.ctypes.data, g.ctypes.data, ctypes.byref(q), ptr[0], ptr[1],
                                       ptr[2], ptr[3])
    return rc, bufs


@pytest.mark.parametrize("name", ["open_moved", "synthetic_37x29"])
def test_nothing_else_is_touched(amvpt_mod, cases, name):
    """Guard floats behind every output of every stage, inputs compared before and after, and what is not finite stays
    where it is: a pixel whose own inputs are finite has a finite output."""
    k = cases[name]
    L = amvpt_mod.hip_lib()
    g = np.ascontiguousarray(k.g)
    h, w = g.shape[:2]
    for channels in (3, 4):
        s = stage_inputs(amvpt_mod, k, channels, seed=31)
        # stage 1
        ins = [s["img"], g, s["hi"], np.ascontiguousarray(k.hg), s["hc"], s["hm"]]
        before = [a.copy() for a in ins]
        o = [np.full(s["img"].size + GUARD, SENTINEL, dtype=F), np.full(h * w + GUARD, SENTINEL, dtype=F),
             np.full(2 * h * w + GUARD, SENTINEL, dtype=F)]
        tp = amvpt_mod.TemporalParams()
        rc = L.amvpt_temporal_moments_host(ins[0].ctypes.data, channels, ins[1].ctypes.data, ins[2].ctypes.data, ins[3].ctypes.data,
                                           ins[4].ctypes.data, ins[5].ctypes.data, ctypes.cast(k.prev_views, ctypes.c_void_p),
                                           ctypes.byref(k.p), None, ctypes.byref(tp), o[0].ctypes.data, o[1].ctypes.data, o[2].ctypes.data)
        assert rc == 0
        for buf, n, ref in zip(o, (s["img"].size, h * w, 2 * h * w), (s["out"], s["cnt"], s["mom"])):
            assert (buf[n:] == SENTINEL).all() and np.array_equal(bits(buf[:n]), bits(ref.ravel()))
        for a, b in zip(ins, before):
            assert np.array_equal(bits(a), bits(b))
        bad = ~np.isfinite(s["img"][..., :3]).all(axis=-1)
        assert bad.sum() >= 3 and np.array_equal(bits(s["out"][bad]), bits(s["img"][bad]))
        assert np.isfinite(s["out"][~bad]).all() and (s["cnt"][~bad] >= 1).all()
        # stage 2, on stage 1's own planes and on planes seeded with NaN, infinities, 0 and 0.5 in the count and NaN and
        # infinities in the moments: the variance is finite and not negative on every pixel
        assert not np.isfinite(s["mom"]).all(), "a history moment that is not finite must have reached a pixel"
        q = amvpt_mod.VarianceParams()
        for mom, cnt in ((s["mom"], s["cnt"]), seeded_stage2(k, s)):
            vbuf = np.full(h * w + GUARD, SENTINEL, dtype=F)
            mom0, cnt0 = mom.copy(), cnt.copy()
            assert L.amvpt_variance_host(mom.ctypes.data, cnt.ctypes.data, g.ctypes.data, w, h, ctypes.byref(q), vbuf.ctypes.data) == 0
            assert (vbuf[h * w:] == SENTINEL).all() and np.isfinite(vbuf[:h * w]).all() and (vbuf[:h * w] >= 0).all()
            assert np.array_equal(bits(mom), bits(mom0)) and np.array_equal(bits(cnt), bits(cnt0)) and np.array_equal(bits(g), bits(k.g))
            assert (vbuf[:h * w].reshape(h, w)[~np.isfinite(mom).all(axis=-1) | ~(cnt >= 1)] == 0).all()
        assert not np.isfinite(cnt).all() and not np.isfinite(mom).all()
        # stage 3
        var = ringed_variance(vbuf[:h * w].reshape(h, w), g)
        img = s["out"]
        img0, var0 = img.copy(), var.copy()
        bad_v = ~np.isfinite(var)
        assert bad.sum() >= 3 and bad_v.sum() >= 6
        for iterations in (1, 2, 3):
            qi = amvpt_mod.VarianceParams(iterations=iterations)
            rc, bufs = _call_filter(amvpt_mod, img, var, g, qi)
            assert rc == 0
            res, vres = bufs[0][:img.size].reshape(img.shape), bufs[2][:h * w].reshape(h, w)
            for buf, n in zip(bufs, (img.size, img.size, h * w, h * w)):
                assert (buf[n:] == SENTINEL).all()
            assert (bufs[1][:img.size] == SENTINEL).all() == (iterations == 1) and (bufs[3][:h * w] == SENTINEL).all() == (iterations == 1)
            assert np.array_equal(bits(res[bad]), bits(img[bad])), "a centre that is not finite must pass through"
            own = ~bad & ~bad_v
            assert np.isfinite(res[own]).all() and np.isfinite(vres[own]).all(), "a value that is not finite contaminated a neighbour"
            assert np.array_equal(bits(img), bits(img0)) and np.array_equal(bits(var), bits(var0)) and np.array_equal(bits(g), bits(k.g))
            want = amvpt_mod.denoise_variance_host(img, var, g, qi)
            assert np.array_equal(bits(res), bits(want[0])) and np.array_equal(bits(vres), bits(want[1]))
        # the buffers that may be absent
        rc, bufs = _call_filter(amvpt_mod, img, var, g, amvpt_mod.VarianceParams(iterations=1), with_scratch=False, with_var_out=False)
        assert rc == 0 and np.array_equal(bits(bufs[0][:img.size]), bits(amvpt_mod.denoise_variance_host(img, var, g, amvpt_mod.VarianceParams(iterations=1))[0].ravel()))
        rc, bufs = _call_filter(amvpt_mod, img, var, g, amvpt_mod.VarianceParams(iterations=2), with_var_out=False)
        assert rc == 0 and np.array_equal(bits(bufs[0][:img.size]), bits(amvpt_mod.denoise_variance_host(img, var, g, amvpt_mod.VarianceParams(iterations=2))[0].ravel()))


def test_a_rectangle_of_whole_tiles(amvpt_mod, cases):
    """No tap of any stage crosses a view: a rectangle of whole tiles, processed alone, is that part of the whole."""
    for name, rect in (("cbox_moved", (16, 16, 32, 16)), ("cone_reversed_moved", (48, 0, 16, 32)), ("batch_turned", (16, 0, 32, 32))):
        k = cases[name]
        s = stage_inputs(amvpt_mod, k, 3, seed=9)
        x0, y0, w, h = rect
        cut = (slice(y0, y0 + h), slice(x0, x0 + w))
        part = amvpt_mod.temporal_moments_host(s["img"][cut], k.g[cut], s["hi"][cut], k.hg[cut], s["hc"][cut], s["hm"][cut],
                                               k.prev_views, k.p, rect=rect)
        for got, whole in zip(part, (s["out"], s["cnt"], s["mom"])):
            _assert_same(got, whole[cut], name + " stage 1")
        want = restated_moments(s["img"][cut], k.g[cut], s["hi"][cut], k.hg[cut], s["hc"][cut], s["hm"][cut], k.prev_views, k.p,
                                amvpt_mod.TemporalParams(), rect=rect)
        _assert_same(part[2], want[2], name + " stage 1 restated")
        q = amvpt_mod.VarianceParams(iterations=5)
        var = amvpt_mod.variance_host(s["mom"], s["cnt"], k.g, q)
        _assert_same(amvpt_mod.variance_host(s["mom"][cut], s["cnt"][cut], k.g[cut], q), var[cut], name + " stage 2")
        whole = amvpt_mod.denoise_variance_host(s["out"], var, k.g, q)
        got = amvpt_mod.denoise_variance_host(s["out"][cut], var[cut], k.g[cut], q)
        _assert_same(got[0], whole[0][cut], name + " stage 3 image")
        _assert_same(got[1], whole[1][cut], name + " stage 3 variance")


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------

def moments_refusal_rows(amvpt_mod, base, n_img, n_px):
    """The rows amvpt_temporal_moments adds to test_temporal.refusal_rows (which it shares; the device test too)."""
    f4 = 4
    rows = [("null_hist_moments", dict(hist_moments=None), 1, "null hist_moments"),
            ("null_out_moments", dict(out_moments=None), 1, "null out_moments")]
    for name, n_in in (("image", n_img), ("guides", 8 * n_px), ("hist_image", n_img), ("hist_guides", 8 * n_px), ("hist_count", n_px),
                       ("hist_moments", 2 * n_px)):
        rows.append(("out_moments_on_" + name, dict(out_moments=base[name] + f4 * (n_in - 1)), 1, "out_moments overlaps"))
    rows += [("out_image_on_hist_moments", dict(out_image=base["hist_moments"] + f4), 1, "out_image overlaps hist_moments"),
             ("out_count_on_hist_moments", dict(out_count=base["hist_moments"] + f4), 1, "out_count overlaps hist_moments"),
             ("out_moments_on_out_image", dict(out_moments=base["out_image"] + f4), 1, "out_moments overlaps out_image"),
             ("out_moments_on_out_count", dict(out_moments=base["out_count"] + f4 * (n_px - 1)), 1, "out_moments overlaps out_count")]
    return rows


def call_moments(fn, a, stream=False):
    ref = lambda v: ctypes.byref(v) if v is not None else None   # noqa: E731
    args = [a["image"], a["channels"], a["guides"], a["hist_image"], a["hist_guides"], a["hist_count"], a["hist_moments"],
            ctypes.cast(a["prev_views"], ctypes.c_void_p) if a["prev_views"] is not None else None, ref(a["params"]), ref(a["rect"]),
            ref(a["tp"]), a["out_image"], a["out_count"], a["out_moments"]]
    return fn(*(args + [None] if stream else args))


def test_refusals_of_the_temporal_stage(amvpt_mod):
    from test_temporal import refusal_base, refusal_rows
    L = amvpt_mod.hip_lib()
    s, vd, p, planes = refusal_base(amvpt_mod)
    planes["hist_moments"] = np.ones((8, 16, 2), dtype=F)
    n_img = planes["image"].size
    out, cnt, mom = np.full(n_img, SENTINEL, dtype=F), np.full(128, SENTINEL, dtype=F), np.full(256, SENTINEL, dtype=F)
    base = dict({k: v.ctypes.data for k, v in planes.items()}, channels=3, prev_views=vd, params=p, rect=None,
                tp=amvpt_mod.TemporalParams(), out_image=out.ctypes.data, out_count=cnt.ctypes.data, out_moments=mom.ctypes.data)
    assert call_moments(L.amvpt_temporal_moments_host, base) == 0
    for buf in (out, cnt, mom):
        buf[:] = SENTINEL
    rows = refusal_rows(amvpt_mod, base, n_img, 128) + moments_refusal_rows(amvpt_mod, base, n_img, 128)
    assert len(rows) == 47 + 12
    for rid, change, status, names in rows:
        rc = call_moments(L.amvpt_temporal_moments_host, dict(base, **change))
        msg = L.amvpt_last_error().decode()
        assert rc == status, (rid, rc, msg)
        assert msg.startswith("amvpt_temporal_moments_host: ") and names in msg, (rid, msg)
    assert all((buf == SENTINEL).all() for buf in (out, cnt, mom)), "a refused call wrote"
    both = np.full(n_img + 128 + 256, SENTINEL, dtype=F)
    assert call_moments(L.amvpt_temporal_moments_host, dict(base, out_image=both.ctypes.data, out_count=both.ctypes.data + 4 * n_img,
                                                            out_moments=both.ctypes.data + 4 * (n_img + 128))) == 0


def parameter_rows(amvpt_mod):
    """(row id, params, what the message must name): one row per refusal of an amvpt_variance_params field."""
    P = amvpt_mod.VarianceParams
    rows = [("iterations_0", P(iterations=0), "iterations"), ("iterations_9", P(iterations=9), "iterations"),
            ("squarings_8", P(normal_squarings=8), "normal_squarings"), ("min_history_0", P(min_history=0), "min_history"),
            ("min_history_65536", P(min_history=65536), "min_history")]
    for field in ("sigma_lum", "var_floor", "sigma_plane"):
        for label, v in (("zero", 0.0), ("negative", -1.0), ("nan", float("nan")), ("inf", float("inf"))):
            rows.append(("%s_%s" % (field, label), P(**{field: v}), field))
    return rows


def variance_refusal_rows(amvpt_mod, base, n_px):
    f4 = 4
    rows = [("null_" + a, {a: None}, "null " + a) for a in ("moments", "count", "guides", "params", "out")]
    rows += [("width_0", dict(width=0), "width"), ("height_0", dict(height=0), "height"),
             ("width_above", dict(width=0x7fffff01), "above 2^31 - 256"), ("height_above", dict(height=0x7fffff01), "above 2^31 - 256"),
             ("tiles_above", dict(width=0x7fffff00, height=0x7fffff00), "above 2^31 tiles")]
    rows += [(rid, dict(params=q), names) for rid, q, names in parameter_rows(amvpt_mod)]
    rows += [("out_on_moments", dict(out=base["moments"] + f4 * (2 * n_px - 1)), "out overlaps the moments"),
             ("out_on_count", dict(out=base["count"] + f4), "out overlaps the count"),
             ("out_on_guides", dict(out=base["guides"] + 64), "out overlaps the guides")]
    return rows


def call_variance(fn, a, stream=False):
    args = [a["moments"], a["count"], a["guides"], a["width"], a["height"], ctypes.byref(a["params"]) if a["params"] is not None else None,
            a["out"]]
    return fn(*(args + [None] if stream else args))


def filter_refusal_rows(amvpt_mod, base, n_img, n_px):
    P = amvpt_mod.VarianceParams
    f4 = 4
    rows = [("null_" + a, {a: None}, "null " + a) for a in ("image", "variance", "guides", "params", "out")]
    rows += [("null_scratch", dict(scratch=None, params=P(iterations=2)), "null scratch"),
             ("null_var_scratch", dict(var_scratch=None, params=P(iterations=2)), "null var_scratch"),
             ("null_var_out", dict(var_out=None, params=P(iterations=3)), "null var_out"),
             ("channels_2", dict(channels=2), "channels"), ("channels_5", dict(channels=5), "channels"),
             ("width_0", dict(width=0), "width"), ("height_0", dict(height=0), "height"),
             ("width_above", dict(width=0x7fffff01), "above 2^31 - 256"), ("height_above", dict(height=0x7fffff01), "above 2^31 - 256"),
             ("tiles_above", dict(width=0x7fffff00, height=0x7fffff00), "above 2^31 tiles")]
    rows += [(rid, dict(params=q), names) for rid, q, names in parameter_rows(amvpt_mod)]
    sizes = dict(out=n_img, scratch=n_img, var_out=n_px, var_scratch=n_px)
    for o in ("out", "scratch", "var_out", "var_scratch"):
        rows += [("%s_on_image" % o, {o: base["image"] + f4 * (n_img - 1)}, "%s overlaps the image" % o),
                 ("%s_on_variance" % o, {o: base["variance"] + f4 * (n_px - 1)}, "%s overlaps the variance" % o),
                 ("%s_on_guides" % o, {o: base["guides"] + 64}, "%s overlaps the guides" % o)]
    for i, a in enumerate(("out", "scratch", "var_out", "var_scratch")):
        for b in ("out", "scratch", "var_out", "var_scratch")[:i]:
            rows.append(("%s_on_%s" % (a, b), {a: base[b] + f4 * (sizes[b] - 1)}, "%s overlaps %s" % (a, b)))
    return rows


def call_filter(fn, a, stream=False):
    args = [a["image"], a["channels"], a["width"], a["height"], a["variance"], a["guides"],
            ctypes.byref(a["params"]) if a["params"] is not None else None, a["out"], a["scratch"], a["var_out"], a["var_scratch"]]
    return fn(*(args + [None] if stream else args))


def refusal_planes():
    """A valid 6 x 5 call of stages 2 and 3: numpy planes, inputs and outputs, cut from one buffer with gaps wider than
    any plane between them, so that a row's overlap is the only one."""
    from test_denoise import random_image, synthetic_guides
    w, h = 6, 5
    g = synthetic_guides(w, h, 3)
    rng = np.random.default_rng(8)
    src = dict(guides=g, image=random_image(g, 3, 4, specials=False), variance=rng.random((h, w)).astype(F),
               moments=(rng.random((h, w, 2)) + 1).astype(F), count=np.full((h, w), F(2)),
               out=np.full((h, w, 3), SENTINEL), scratch=np.full((h, w, 3), SENTINEL), var_out=np.full((h, w), SENTINEL),
               var_scratch=np.full((h, w), SENTINEL), variance_out=np.full((h, w), SENTINEL))
    arena = np.zeros(512 * (len(src) + 1), dtype=F)
    planes = dict(w=w, h=h, arena=arena)
    for i, (name, a) in enumerate(src.items()):
        planes[name] = arena[512 * i + 256:512 * i + 256 + a.size].reshape(a.shape)
        planes[name][...] = a
    return planes


def test_refusals_of_the_variance_and_the_filter(amvpt_mod):
    L = amvpt_mod.hip_lib()
    pl = refusal_planes()
    w, h, n_px, n_img = pl["w"], pl["h"], pl["w"] * pl["h"], pl["image"].size
    out = pl["variance_out"].reshape(-1)
    base = dict(moments=pl["moments"].ctypes.data, count=pl["count"].ctypes.data, guides=pl["guides"].ctypes.data, width=w, height=h,
                params=amvpt_mod.VarianceParams(), out=out.ctypes.data)
    assert call_variance(L.amvpt_variance_host, base) == 0
    out[:] = SENTINEL
    rows = variance_refusal_rows(amvpt_mod, base, n_px)
    assert len(rows) == 5 + 5 + 17 + 3
    for rid, change, names in rows:
        rc = call_variance(L.amvpt_variance_host, dict(base, **change))
        msg = L.amvpt_last_error().decode()
        assert rc == 1 and msg.startswith("amvpt_variance_host: ") and names in msg, (rid, rc, msg)
    assert (out == SENTINEL).all(), "a refused call wrote"

    bufs = {k: pl[k].reshape(-1) for k in ("out", "scratch", "var_out", "var_scratch")}
    base = dict({k: v.ctypes.data for k, v in bufs.items()}, image=pl["image"].ctypes.data, channels=3, width=w, height=h,
                variance=pl["variance"].ctypes.data, guides=pl["guides"].ctypes.data, params=amvpt_mod.VarianceParams())
    assert call_filter(L.amvpt_denoise_variance_host, base) == 0
    for b in bufs.values():
        b[:] = SENTINEL
    rows = filter_refusal_rows(amvpt_mod, base, n_img, n_px)
    assert len(rows) == 5 + 10 + 17 + 12 + 6
    for rid, change, names in rows:
        rc = call_filter(L.amvpt_denoise_variance_host, dict(base, **change))
        msg = L.amvpt_last_error().decode()
        assert rc == 1 and msg.startswith("amvpt_denoise_variance_host: ") and names in msg, (rid, rc, msg)
    assert all((b == SENTINEL).all() for b in bufs.values()), "a refused call wrote"
    # buffers that touch without overlapping are accepted
    both = np.full(2 * n_img + 2 * n_px, SENTINEL, dtype=F)
    a = both.ctypes.data
    assert call_filter(L.amvpt_denoise_variance_host, dict(base, out=a, scratch=a + 4 * n_img, var_out=a + 8 * n_img,
                                                           var_scratch=a + 8 * n_img + 4 * n_px)) == 0


def test_python_layer(amvpt_mod):
    import inspect

    import amvpt.display as D
    pl = refusal_planes()
    with pytest.raises(ValueError, match="guide records are needed"):
        amvpt_mod.variance_host(pl["moments"][:4], pl["count"], pl["guides"])
    with pytest.raises(ValueError, match="of its size are needed"):
        amvpt_mod.denoise_variance_host(pl["image"], pl["variance"][:, :5], pl["guides"])
    with pytest.raises(RuntimeError, match="amvpt_variance_host: params: min_history must be 1 .. 65535, not 0"):
        amvpt_mod.variance_host(pl["moments"], pl["count"], pl["guides"], amvpt_mod.VarianceParams(min_history=0))
    with pytest.raises(RuntimeError, match="amvpt_denoise_variance_host: params: sigma_lum must be finite and above 0"):
        amvpt_mod.denoise_variance_host(pl["image"], pl["variance"], pl["guides"], amvpt_mod.VarianceParams(sigma_lum=0.0))
    acc = amvpt_mod.TemporalAccumulator(moments=True)
    assert acc.with_moments and acc.moments is None and acc.frames == 0
    plain = amvpt_mod.TemporalAccumulator()
    assert not plain.with_moments and inspect.signature(amvpt_mod.TemporalAccumulator).parameters["moments"].default is False
    with pytest.raises(ValueError, match="needs moments=True"):
        plain.variance()
    s = amvpt_mod.load_file(os.path.join(REPO, "scenes", "cbox_grid.xml"), res=8, spp=4)
    for kw in (dict(), dict(temporal=plain)):
        with pytest.raises(ValueError, match="TemporalAccumulator\\(moments=True\\)"):
            D.display(s, size=(16, 8), denoise=amvpt_mod.VarianceParams(), **kw)


# ---------------------------------------------------------------------------------------------------------------
# 5. the quality gates, on oracle renders
# ---------------------------------------------------------------------------------------------------------------

GATE_A = 0.93   # halfway between the measured ratio 0.861 and 1
GATE_B = 0.829  # halfway between the measured ratio 0.658 and 1


@pytest.fixture(scope="module")
def sequences(amvpt_mod, oracle):
    """test_temporal.test_quality_gate's sequence, cbox_path.xml at 128 x 128 with the camera moving by STEP a frame:
    eight frames (seeds 1 .. 8) at 1 spp and at 16 spp, their guide records and views, and the 256-spp reference (seed
    0) from the last camera."""
    threads = min(16, os.cpu_count() or 4)
    xml = xml_of("cbox_path.xml")
    cam = 'origin="0, 0, 3.90" target="0, 0, 0"'
    assert cam in xml
    frames = {1: [], 16: []}
    for i in range(8):
        x = STEP * (i - 7)
        s = amvpt_mod.load_string(xml.replace(cam, 'origin="%g, 0, 3.9" target="%g, 0, 0"' % (x, x)), res=128)
        for spp in frames:
            sd, vd, p = s.describe(0, 1 + i, spp)
            film, _, _ = oracle.render(sd, vd, p, threads=threads)
            frames[spp].append((oracle.develop(film, bool(p.film_alpha)).astype(F), oracle.primary_hits(sd, vd, p), vd, p, s))
    sd, vd, p = frames[1][-1][4].describe(0, 0, 256)
    film, _, _ = oracle.render(sd, vd, p, threads=threads)
    return frames, oracle.develop(film, bool(p.film_alpha)).astype(F)


def accumulate(amvpt_mod, frames):
    """Both pipelines' temporal stage over a sequence -> (image, count, moments, guides); the image and the count are
    amvpt_temporal_host's (asserted)."""
    tp = amvpt_mod.TemporalParams()
    h, w = frames[0][1].shape[:2]
    hi, hg, hc, hm = np.zeros_like(frames[0][0]), frames[0][1], np.zeros((h, w), dtype=F), np.zeros((h, w, 2), dtype=F)
    pi, pc = hi, hc
    for i, (img, g, vd, p, _) in enumerate(frames):
        prev = frames[i - 1][2] if i else vd
        pi, pc = amvpt_mod.temporal_host(img, g, pi, hg, pc, prev, p, tp)
        hi, hc, hm = amvpt_mod.temporal_moments_host(img, g, hi, hg, hc, hm, prev, p, tp)
        assert np.array_equal(bits(hi), bits(pi)) and np.array_equal(bits(hc), bits(pc))
        hg = g
    return hi, hc, hm, hg


def new_pipeline(amvpt_mod, acc, q=None, scale=None):
    img, cnt, mom, g = acc
    q = q if q is not None else amvpt_mod.VarianceParams()
    var = amvpt_mod.variance_host(mom, cnt, g, q)
    if scale is not None:
        var = (var * F(scale)).astype(F)
    return amvpt_mod.denoise_variance_host(img, var, g, q)[0]


def test_quality_gates(amvpt_mod, sequences):
    """Against the pipeline of today, amvpt_temporal_host -> amvpt_denoise_host at its defaults, on the same frames; the
    new one is amvpt_temporal_moments_host -> amvpt_variance_host -> amvpt_denoise_variance_host at its defaults.  The
    metric is test_denoise's relative RMSE against the 256-spp reference.  Gates (a) and (b) lie halfway between the
    measured ratio and 1.
    Measured, relative RMSE:
      (a) 8 x 1 spp    raw 0.5220, accumulated 0.1899, today 0.1216, variance-guided 0.1047 (ratio 0.861); the count is
                       below min_history on 0.065 of the pixels
      (b) 8 x 16 spp   raw 0.1349, accumulated 0.1134, today 0.1190 (worse than its input), variance-guided 0.0783 (ratio
                       0.658); with 64 times the variance 0.1118, above the gate's 0.0986
      (c) the 256-spp reference filtered: today moves it by 0.1061, the variance-guided filter at zero variance by 0.0068
      (power) the accumulated frame of (a) filtered at zero variance moves by 0.0119, where today's filter moves it by
              0.1621: a quarter of that is 0.0405"""
    frames, ref = sequences
    today = lambda img, g: amvpt_mod.denoise_host(img, g, amvpt_mod.DenoiseParams())   # noqa: E731
    # (a) 8 x 1 spp
    acc = accumulate(amvpt_mod, frames[1])
    e_acc, e_today, e_new = rel_rmse(acc[0], ref), rel_rmse(today(acc[0], acc[3]), ref), rel_rmse(new_pipeline(amvpt_mod, acc), ref)
    print("(a) 8 x 1 spp: raw %.4f, accumulated %.4f, today %.4f, variance-guided %.4f (ratio %.3f); count < 4 on %.3f of the pixels" % (
        rel_rmse(frames[1][-1][0], ref), e_acc, e_today, e_new, e_new / e_today, (acc[1] < 4).mean()))
    # (b) 8 x 16 spp
    acc16 = accumulate(amvpt_mod, frames[16])
    f_acc, f_today, f_new = rel_rmse(acc16[0], ref), rel_rmse(today(acc16[0], acc16[3]), ref), rel_rmse(new_pipeline(amvpt_mod, acc16), ref)
    f_loud = rel_rmse(new_pipeline(amvpt_mod, acc16, scale=64), ref)
    print("(b) 8 x 16 spp: raw %.4f, accumulated %.4f, today %.4f, variance-guided %.4f (ratio %.3f); with 64 x the variance %.4f" % (
        rel_rmse(frames[16][-1][0], ref), f_acc, f_today, f_new, f_new / f_today, f_loud))
    # (c) convergence: the reference itself, with a variance of zero
    g = frames[1][-1][1]
    zero = np.zeros(g.shape[:2], dtype=F)
    d_today = rel_rmse(today(ref, g), ref)
    d_new = rel_rmse(amvpt_mod.denoise_variance_host(ref, zero, g)[0], ref)
    print("(c) the reference filtered: today moves it by %.4f, variance-guided at zero variance by %.4f" % (d_today, d_new))
    # the power check of (a): without a variance there is no denoising
    still = rel_rmse(amvpt_mod.denoise_variance_host(acc[0], zero, acc[3])[0], acc[0])
    moved_today = rel_rmse(today(acc[0], acc[3]), acc[0])
    print("(power) the accumulated frame of (a) at zero variance moves by %.4f; today moves it by %.4f" % (still, moved_today))
    assert e_new <= GATE_A * e_today
    assert f_today > f_acc, "the defect this header answers: today's pipeline returns an image worse than its input"
    assert f_new < f_acc and f_new <= GATE_B * f_today
    assert d_new <= 0.25 * d_today
    assert not (f_loud < f_acc and f_loud <= GATE_B * f_today), "the power check: with 64 x the variance gate (b) must fail"
    assert still <= 0.25 * moved_today, "the power check: without a variance the filter must leave its input alone"

"""The a-trous denoiser on the CPU (include/amvpt_denoise.h): amvpt_denoise_host against a numpy float32 restatement
of the header's definition, bit for bit; what the definition promises about constant regions, pixels that are not
finite and buffers it must not touch; the refusals; and the quality gate on oracle renders.  The guide records come
from the oracle's primary-hit hook, which is what amvpt_guides reproduces on the device.  tests/test_gpu_denoise.py
runs the device entry over the same cases.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO, SCENES
from test_guides import bits, open_scene_xml

F = np.float32
HK = {-2: F(0.0625), -1: F(0.25), 0: F(0.375), 1: F(0.25), 2: F(0.0625)}
GUARD = 64
SENTINEL = F(-12345.0)


# ---------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------

def _dot(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z, every product and sum rounded to float32."""
    return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)


def restated_iteration(img, g, step, inv_s2, floor2, inv_sp, squarings):
    h, w, _ = img.shape
    c = img[..., :3]
    n_p, pos_p = g[..., 1:4], g[..., 4:7]
    hit = g[..., 0] >= 0
    with np.errstate(all="ignore"):
        m = (_dot(c, c) + floor2).astype(F)
        k = (inv_s2 / m).astype(F)
        sum_c = np.zeros((h, w, 3), dtype=F)
        sum_w = np.zeros((h, w), dtype=F)
        ys, xs = np.mgrid[0:h, 0:w]
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * step, xs + dx * step
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                gq, cq = g[qy, qx], c[qy, qx]
                ok = inside & np.isfinite(cq).all(axis=-1) & (gq[..., 7] == g[..., 7]) & (gq[..., 0] == g[..., 0])
                d = (cq - c).astype(F)
                wc = (F(1) / (F(1) + (_dot(d, d) * k).astype(F)).astype(F)).astype(F)
                wgt = (F(HK[dy] * HK[dx]) * wc).astype(F)
                wn = _dot(n_p, gq[..., 1:4]).astype(F)
                wn = np.where(wn > 0, wn, F(0)).astype(F)
                for _ in range(squarings):
                    wn = (wn * wn).astype(F)
                e = (gq[..., 4:7] - pos_p).astype(F)
                t = (np.abs(_dot(n_p, e)).astype(F) * inv_sp).astype(F)
                wp = (F(1) / (F(1) + (t * t).astype(F)).astype(F)).astype(F)
                wgt = np.where(hit, (wgt * (wn * wp).astype(F)).astype(F), wgt)
                sum_c = np.where(ok[..., None], (sum_c + (wgt[..., None] * cq).astype(F)).astype(F), sum_c)
                sum_w = np.where(ok, (sum_w + wgt).astype(F), sum_w)
        out = img.copy()   # alpha, and the pixels whose sum of weights is not above 0
        good = sum_w > 0
        out[..., :3] = np.where(good[..., None], (sum_c / sum_w[..., None]).astype(F), c)
    return out


def restated(img, g, q):
    """amvpt_denoise_host in numpy: the constants as the header forms them, then one pass per iteration."""
    img, g = np.ascontiguousarray(img, dtype=F), np.ascontiguousarray(g, dtype=F)
    inv_s2 = F(1) / F(F(q.sigma_color) * F(q.sigma_color))
    floor2 = F(F(q.color_floor) * F(q.color_floor))
    inv_sp = F(1) / F(q.sigma_plane)
    for i in range(q.iterations):
        img = restated_iteration(img, g, 1 << i, inv_s2, floor2, inv_sp, q.normal_squarings)
        inv_s2 = F(F(4) * inv_s2)
    return img


# ---------------------------------------------------------------------------------------------------------------
# the cases (tests/test_gpu_denoise.py runs the device over them too)
# ---------------------------------------------------------------------------------------------------------------

def synthetic_guides(w, h, seed):
    """Random unit normals and positions, 4 shape ids (-1 among them) and 3 views in irregular patches."""
    rng = np.random.default_rng(seed)
    g = np.zeros((h, w, 8), dtype=F)
    ys, xs = np.mgrid[0:h, 0:w]

    def patches(values, ny, nx):
        grid = rng.choice(values, size=(ny, nx))
        grid.flat[:len(values)] = values   # every value appears where the image is large enough
        return grid[np.minimum(ys * ny // max(h, 1), ny - 1), np.minimum(xs * nx // max(w, 1), nx - 1)]

    g[..., 0] = patches(np.array([-1, 0, 1, 2]), 5, 7)
    g[..., 7] = patches(np.array([0, 1, 2]), 4, 3)
    n = rng.standard_normal((h, w, 3))
    # normals that vary slowly along x, so that the normal weight takes values between 0 and 1
    n = n[:, :1] + 0.35 * np.cumsum(rng.standard_normal((h, w, 3)), axis=1) / np.sqrt(np.arange(1, w + 1))[None, :, None]
    g[..., 1:4] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    g[..., 4:7] = (rng.random((h, w, 3)) * 0.2 + np.dstack([xs * 0.01, ys * 0.01, np.zeros((h, w))])).astype(F)
    g[g[..., 0] < 0, 1:7] = 0
    return g


def random_image(g, channels, seed, specials=True, tile=None):
    """Seeded random positive float32; with `specials` a NaN, a +inf and a -inf each on a hit pixel, on a miss pixel
    and (given the tile size) on a pixel adjacent to a tile border."""
    rng = np.random.default_rng(seed)
    h, w = g.shape[:2]
    img = (rng.random((h, w, channels)) * rng.choice([0.02, 0.5, 3.0], size=(h, w, 1))).astype(F) + F(1e-3)
    if not specials:
        return img
    vals = [F(np.nan), F(np.inf), F(-np.inf)]
    hit = np.argwhere(g[..., 0] >= 0)
    miss = np.argwhere(g[..., 0] < 0)
    spots = []
    for group in (hit[len(hit) // 3::max(1, len(hit) // 7)][:3], miss[len(miss) // 3::max(1, len(miss) // 7)][:3]):
        spots += [tuple(p) for p in group]
    if tile:
        spots += [(min(5, h - 1), tile - 1), (min(tile, h - 1), min(9, w - 1)), (min(tile + 3, h - 1), min(tile, w - 1))]
    for i, (y, x) in enumerate(spots):
        img[y, x, i % 3] = vals[i % 3]
    return img


@pytest.fixture(scope="module")
def grid_hits(oracle, amvpt_mod):
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=16, gx=4, gy=2)
    sd, vd, p = s.describe(0, 0, 0)
    return oracle.primary_hits(sd, vd, p)


@pytest.fixture(scope="module")
def open_hits(oracle, amvpt_mod):
    s = amvpt_mod.load_string(open_scene_xml(), res=16, gx=4, gy=2)
    sd, vd, p = s.describe(0, 0, 0)
    return oracle.primary_hits(sd, vd, p)


def build_cases(grid, open_):
    """name -> (guide records, tile size or None): the oracle's records of a closed and an open scene (64 x 32, eight
    views of 16 x 16), and synthetic ones."""
    assert grid.shape == open_.shape == (32, 64, 8) and (open_[..., 0] < 0).any() and (open_[..., 0] >= 0).any()
    return {"cbox_grid": (grid, 16), "open_scene": (open_, 16), "synthetic_37x29": (synthetic_guides(37, 29, 11), None),
            "row_40x1": (synthetic_guides(40, 1, 12), None), "column_1x40": (synthetic_guides(1, 40, 13), None)}


@pytest.fixture(scope="module")
def cases(grid_hits, open_hits):
    return build_cases(grid_hits, open_hits)


CASE_NAMES = ["cbox_grid", "open_scene", "synthetic_37x29", "row_40x1", "column_1x40"]


def params_of(amvpt_mod, iterations, **kw):
    """The default parameters at `iterations` (other fields as keywords)."""
    return amvpt_mod.DenoiseParams(iterations=iterations, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------

def test_versions_and_defaults(amvpt_mod):
    assert amvpt_mod.denoise_version() == 1
    assert amvpt_mod.hip_lib().amvpt_abi_version() == 12
    d = amvpt_mod.denoise_default_params()
    assert d.values() == (3, 1.0, F(0.01), F(0.05), 5) and d.values() == amvpt_mod.DenoiseParams().values()


def test_header_is_exported(amvpt_mod):
    from test_capi import declared
    names = declared(os.path.join(REPO, "include", "amvpt_denoise.h"))
    assert names == ["amvpt_denoise", "amvpt_denoise_default_params", "amvpt_denoise_host", "amvpt_denoise_version"]
    L, H = amvpt_mod.hip_lib(), amvpt_mod.host_lib()
    assert all(hasattr(L, n) for n in names) and hasattr(H, "amvpt_host_denoise_stream")
    text = open(os.path.join(REPO, "include", "amvpt_denoise.h")).read()
    assert re.search(r"#define AMVPT_DENOISE_VERSION 1\b", text)


@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_equals_the_restatement(amvpt_mod, cases, name, channels, iterations):
    g, tile = cases[name]
    img = random_image(g, channels, 100 + channels, tile=tile)
    assert not np.isfinite(img).all()
    q = params_of(amvpt_mod, iterations)
    got = amvpt_mod.denoise_host(img, g, q)
    want = restated(img, g, q)
    same = bits(got) == bits(want)
    assert same.all(), "%d of %d floats differ from the restatement, first at %s" % (
        (~same).sum(), same.size, np.argwhere(~same)[:3].tolist())
    if channels == 4:
        assert np.array_equal(bits(got[..., 3]), bits(img[..., 3]))
    assert not np.array_equal(got[..., :3], img[..., :3])


def test_step_of_the_tile_size_stops_every_far_tap(amvpt_mod, cases):
    """Iteration 4 (step 16) on views of 16 x 16: every tap but the centre's lies in another view or outside, so the
    fifth iteration writes (w c) / w with w the centre's own weight: the fourth's result up to those two roundings
    (2^-24 each), however different the neighbouring views are."""
    g, _ = cases["cbox_grid"]
    img = random_image(g, 3, 5, specials=False)
    four = amvpt_mod.denoise_host(img, g, params_of(amvpt_mod, 4))
    five = amvpt_mod.denoise_host(img, g, params_of(amvpt_mod, 5))
    assert (np.abs(five.astype(np.float64) - four) <= 2.0 ** -22 * np.abs(four)).all()
    assert not np.array_equal(four, amvpt_mod.denoise_host(img, g, params_of(amvpt_mod, 3)))


def test_other_parameters(amvpt_mod, cases):
    """Parameters away from the defaults, 8 iterations and no squaring among them."""
    g, _ = cases["synthetic_37x29"]
    img = random_image(g, 3, 21)
    for q in (amvpt_mod.DenoiseParams(8, 0.3, 0.5, 0.011, 0), amvpt_mod.DenoiseParams(2, 7.0, 1e-4, 3.0, 7),
              amvpt_mod.DenoiseParams(3, 1.0, 0.01, 0.05, 1)):
        assert np.array_equal(bits(amvpt_mod.denoise_host(img, g, q)), bits(restated(img, g, q))), q


# ---------------------------------------------------------------------------------------------------------------
# 2. constant regions stay put
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cbox_grid", "open_scene", "synthetic_37x29"])
def test_constant_regions_stay_put(amvpt_mod, cases, name):
    g, _ = cases[name]
    region = g[..., 7].astype(int) * 64 + g[..., 0].astype(int) + 1
    ids = np.unique(region)
    assert 6 <= len(ids) <= 128
    expo = np.searchsorted(ids, region) - len(ids) // 2   # a different power of two per (view, shape) region
    img = np.repeat(np.ldexp(F(1), expo).astype(F)[..., None], 4, axis=-1)
    for c in (3, 4):
        out = amvpt_mod.denoise_host(img[..., :c], g, params_of(amvpt_mod, 5))
        assert np.array_equal(out, img[..., :c])


# ---------------------------------------------------------------------------------------------------------------
# 3. nothing else is touched
# ---------------------------------------------------------------------------------------------------------------

def _call_host(amvpt_mod, img, g, q, with_scratch=True):
    """The C entry on buffers with guard floats behind out and scratch; returns (status, out, out buffer, scratch buffer)."""
    L = amvpt_mod.hip_lib()
    h, w, c = img.shape
    n = h * w * c
    out = np.full(n + GUARD, SENTINEL, dtype=F)
    scratch = np.full(n + GUARD, SENTINEL, dtype=F) if with_scratch else None
    rc = L.amvpt_denoise_host(img.ctypes.data, c, w, h, g.ctypes.data, ctypes.byref(q), out.ctypes.data,
                              scratch.ctypes.data if scratch is not None else None)
    return rc, out[:n].reshape(h, w, c), out, scratch


@pytest.mark.parametrize("name", ["open_scene", "synthetic_37x29"])
def test_nothing_else_is_touched(amvpt_mod, cases, name):
    g, tile = cases[name]
    g = np.ascontiguousarray(g)
    for channels in (3, 4):
        img = random_image(g, channels, 31, tile=tile)
        img0, g0 = img.copy(), g.copy()
        bad = ~np.isfinite(img[..., :3]).all(axis=-1)
        assert 6 <= bad.sum() <= 9
        for iterations in (1, 2, 3):
            rc, res, out, scratch = _call_host(amvpt_mod, img, g, params_of(amvpt_mod, iterations))
            assert rc == 0
            n = img.size
            assert np.array_equal(bits(res[bad]), bits(img[bad])), "a centre that is not finite must pass through"
            assert np.isfinite(res[~bad]).all(), "a pixel that is not finite contaminated a neighbour"
            assert np.array_equal(bits(img), bits(img0)) and np.array_equal(bits(g), bits(g0))
            assert (out[n:] == SENTINEL).all() and (scratch[n:] == SENTINEL).all()
            assert (scratch[:n] == SENTINEL).all() == (iterations == 1)
            assert np.array_equal(bits(res), bits(amvpt_mod.denoise_host(img, g, params_of(amvpt_mod, iterations))))
        rc, res, out, _ = _call_host(amvpt_mod, img, g, params_of(amvpt_mod, 1), with_scratch=False)
        assert rc == 0 and (out[img.size:] == SENTINEL).all()
        assert np.array_equal(bits(res), bits(restated(img, g, params_of(amvpt_mod, 1))))


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------

def refusal_rows(amvpt_mod, base, n_img):
    """(row id, changed arguments, what the message must name): one row per refusal of the header.  `base` holds the
    valid arguments (addresses); a row replaces some of them.  Shared with the device entry's test."""
    P = amvpt_mod.DenoiseParams
    f4 = 4
    rows = [("null_image", dict(image=None), "null image"), ("null_guides", dict(guides=None), "null guides"),
            ("null_params", dict(params=None), "null params"), ("null_out", dict(out=None), "null out"),
            ("null_scratch", dict(scratch=None, params=P(iterations=2)), "null scratch"),
            ("channels_2", dict(channels=2), "channels"), ("channels_5", dict(channels=5), "channels"),
            ("width_0", dict(width=0), "width"), ("height_0", dict(height=0), "height"),
            ("iterations_0", dict(params=P(iterations=0)), "iterations"),
            ("iterations_9", dict(params=P(iterations=9)), "iterations"),
            ("squarings_8", dict(params=P(normal_squarings=8)), "normal_squarings")]
    for field in ("sigma_color", "color_floor", "sigma_plane"):
        for label, v in (("zero", 0.0), ("negative", -1.0), ("nan", float("nan")), ("inf", float("inf"))):
            rows.append(("%s_%s" % (field, label), dict(params=P(**{field: v})), field))
    rows += [("out_on_image", dict(out=base["image"] + f4 * (n_img - 1)), "out overlaps the image"),
             ("out_on_guides", dict(out=base["guides"] + f4), "out overlaps the guides"),
             ("scratch_on_image", dict(scratch=base["image"]), "scratch overlaps the image"),
             ("scratch_on_guides", dict(scratch=base["guides"] + 64), "scratch overlaps the guides"),
             ("scratch_on_out", dict(scratch=base["out"] + f4), "scratch overlaps out")]
    return rows


def test_refusals(amvpt_mod):
    L = amvpt_mod.hip_lib()
    w, h, c = 6, 5, 3
    g = synthetic_guides(w, h, 3)
    img = random_image(g, c, 4, specials=False)
    out, scratch = np.full(img.size, SENTINEL, dtype=F), np.full(img.size, SENTINEL, dtype=F)
    base = dict(image=img.ctypes.data, channels=c, width=w, height=h, guides=g.ctypes.data, params=amvpt_mod.DenoiseParams(),
                out=out.ctypes.data, scratch=scratch.ctypes.data)

    def call(a):
        return L.amvpt_denoise_host(a["image"], a["channels"], a["width"], a["height"], a["guides"],
                                    ctypes.byref(a["params"]) if a["params"] is not None else None, a["out"], a["scratch"])

    assert call(base) == 0
    out[:] = SENTINEL
    scratch[:] = SENTINEL
    rows = refusal_rows(amvpt_mod, base, img.size)
    assert len(rows) == 29
    for rid, change, names in rows:
        rc = call(dict(base, **change))
        msg = L.amvpt_last_error().decode()
        assert rc == 1, (rid, rc)
        assert msg.startswith("amvpt_denoise_host: ") and names in msg, (rid, msg)
    assert (out == SENTINEL).all() and (scratch == SENTINEL).all(), "a refused call wrote"
    # buffers that touch without overlapping are accepted
    both = np.full(2 * img.size, SENTINEL, dtype=F)
    assert call(dict(base, out=both.ctypes.data, scratch=both.ctypes.data + 4 * img.size)) == 0


def test_python_layer_checks_shapes(amvpt_mod):
    g = synthetic_guides(6, 5, 3)
    with pytest.raises(ValueError, match="guide records of its size"):
        amvpt_mod.denoise_host(np.zeros((5, 7, 3), dtype=F), g)
    with pytest.raises(RuntimeError, match="amvpt_denoise_host: channels must be 3 or 4, not 2"):
        amvpt_mod.denoise_host(np.zeros((5, 6, 2), dtype=F), g)
    with pytest.raises(RuntimeError, match="sigma_plane must be finite and above 0"):
        amvpt_mod.denoise_host(np.zeros((5, 6, 3), dtype=F), g, amvpt_mod.DenoiseParams(sigma_plane=0.0))


# ---------------------------------------------------------------------------------------------------------------
# 5. the quality gate, on oracle renders
# ---------------------------------------------------------------------------------------------------------------

def rel_rmse(a, ref):
    a, ref = a[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(((a - ref) / (ref + 0.01)) ** 2)))


def test_quality_gate(amvpt_mod, oracle):
    """cbox_path.xml at 256 x 256, seed 7, against a 256-spp render with seed 0; the metric is
    sqrt(mean(((a - ref) / (ref + 0.01))^2)) over RGB.  The default parameters with the Python default sigma_plane
    must at least halve the error of the 1-spp frame and must not make the 4-spp frame worse.
    Measured: 1 spp 0.5107 -> 0.1817 (ratio 0.356); 4 spp 0.2494 -> 0.0911 (ratio 0.365)."""
    threads = min(16, os.cpu_count() or 4)
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_path.xml"), res=256)

    def frame(seed, spp):
        sd, vd, p = s.describe(0, seed, spp)
        film, _, _ = oracle.render(sd, vd, p, threads=threads)
        return oracle.develop(film, bool(p.film_alpha)).astype(F), (sd, vd, p)

    ref, (sd, vd, p) = frame(0, 256)
    g = oracle.primary_hits(sd, vd, p)
    q = amvpt_mod.DenoiseParams(sigma_plane=amvpt_mod.denoise_sigma_plane(g))
    assert q.values()[:3] == (3, 1.0, F(0.01)) and q.normal_squarings == 5
    assert abs(q.sigma_plane - 0.05) < 0.005   # the Cornell box is 2 wide: 1/40 of it
    for spp, bound in ((1, 0.5), (4, 1.0)):
        noisy, _ = frame(7, spp)
        before, after = rel_rmse(noisy, ref), rel_rmse(amvpt_mod.denoise_host(noisy, g, q), ref)
        print("cbox_path res=256 seed=7 spp=%d: relative RMSE %.4f -> %.4f (ratio %.3f), sigma_plane %.5f" % (
            spp, before, after, after / before, q.sigma_plane))
        assert after <= bound * before


# ---------------------------------------------------------------------------------------------------------------
# 6. the display stage's default is unchanged
# ---------------------------------------------------------------------------------------------------------------

def test_display_default_is_unchanged(amvpt_mod):
    """denoise=None is the default and the call without the keyword: without a device both refuse alike (the case of
    tests/test_display.py); with one, both show the cached frame in the same bytes."""
    import amvpt.display as D
    assert inspect.signature(D.display).parameters["denoise"].default is None
    s = amvpt_mod.load_file(os.path.join(SCENES, "cbox_grid.xml"), res=8, spp=4)
    if amvpt_mod.device_count() <= 0:
        errors = []
        for kw in (dict(), dict(denoise=None), dict(rerender=False), dict(rerender=False, denoise=None)):
            with pytest.raises(RuntimeError) as e:
                D.display(s, size=(16, 8), **kw)
            errors.append(str(e.value))
        assert errors[0] == errors[1] and errors[2] == errors[3]
        with pytest.raises(RuntimeError):
            D.display(s, size=(16, 8), denoise=True)
        return
    D.display(s, size=(16, 8))
    a = D.display(s, size=(16, 8), rerender=False)
    b = D.display(s, size=(16, 8), rerender=False, denoise=None)
    assert np.array_equal(a, b)

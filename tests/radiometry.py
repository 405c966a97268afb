"""Closed-form radiometry for small scenes: XML scene builders, float64 answers and the gates.

Shared by tests/test_radiometry.py (CPU oracle) and tests/test_gpu_radiometry.py (HIP path).  Every other test
compares the device with the oracle; both restate the reference, so an error they share is invisible there.  The
scenes here have exact answers that depend on neither:

A. a closed Lambertian enclosure of uniform emission Le and albedo rho has constant radiance
   L = Le (1 - rho^D) / (1 - rho) at max_depth D >= 1 and Le / (1 - rho) at D = -1 (a geometric series: every
   bounce sees the same radiance) -- emitter sampling and its pdfs, BSDF / emitter MIS, depth bookkeeping,
   Russian roulette, flip_normals, a shape that emits and reflects;
B. direct light on a diffuse floor: L_o = rho L (r/d)^2 cos(theta) under a sphere light, rho E / pi with Lambert's
   polygon formula E = (L/2) |sum_i gamma_i (Gamma_i . n)| under a rectangle light, and under a constant
   environment pi L_env less what the lights cover -- cone, rectangle and environment sampling, sampling_weight;
C. a furnace (constant environment of radiance 1, max_depth 2): a diffuse sphere reads rho, a rough conductor
   its directional albedo int F D G1 G1 (w_i . m) / cos(theta_i) dw_m by float64 quadrature.

All scenes use the box filter, so a pixel is the plain mean of the radiance over the pixel.
"""
import functools

import numpy as np
from scipy.special import erf

RHO = (0.8, 0.5, 0.2)
LE = (1.0, 2.0, 3.0)
ETA = (0.2, 0.92, 1.1)      # the Veach plates' conductor (scenes/veach_grid.xml)
KAPPA = (3.9, 2.45, 2.14)


# ---------------------------------------------------------------------------------------------------------------
# scene builders

def _rgb(v):
    return ", ".join("%.9g" % x for x in v)


def scene_xml(shapes, integrator="path", max_depth=2, rr_depth=5, origin=(0, 0, 4), target=(0, 0, 0), up=(0, 1, 0),
              fov=40.0, res=16, spp=64, grid=None, adaptive=0, spp_pass=16, cam_dist=0.1, sampler_seed=0, extra=""):
    """A scene around `shapes` (XML text).  integrator "path": one perspective camera; "mvpath": grid = (gx, gy, G),
    a gx x gy quilt of perspective views on a line along x, groups of G, sa_reuse and sa_mis on.  `res` is the
    resolution per view, `sampler_seed` the sampler's own `seed` property (the reference's base seed)."""
    look = '<lookat origin="%s" target="%s" up="%s"/>' % (_rgb(origin), _rgb(target), _rgb(up))
    sampler = '<integer name="sample_count" value="%d"/><integer name="seed" value="%d"/>' % (spp, sampler_seed)
    if integrator == "path":
        assert grid is None
        head = """
    <integrator type="path">
        <integer name="max_depth" value="%d"/>
        <integer name="rr_depth" value="%d"/>
    </integrator>
    <sensor type="perspective">
        <string name="fov_axis" value="smaller"/>
        <float name="near_clip" value="0.001"/>
        <float name="far_clip" value="1000.0"/>
        <float name="fov" value="%.9g"/>
        <transform name="to_world">%s</transform>
        <sampler type="independent">%s</sampler>
        <film type="hdrfilm">
            <integer name="width" value="%d"/>
            <integer name="height" value="%d"/>
            <rfilter type="box"/>
            <string name="pixel_format" value="rgb"/>
        </film>
    </sensor>""" % (max_depth, rr_depth, fov, look, sampler, res, res)
    else:
        assert integrator == "mvpath"
        gx, gy, G = grid
        head = """
    <integrator type="mvpath">
        <integer name="max_depth" value="%d"/>
        <integer name="rr_depth" value="%d"/>
        <boolean name="sa_reuse" value="true"/>
        <boolean name="sa_mis" value="true"/>
        <integer name="reuse_count" value="%d"/>
        <integer name="adaptive" value="%d"/>
        <integer name="spp_pass_lim" value="%d"/>
    </integrator>
    <sensor type="grid">
        <integer name="grid_x" value="%d"/>
        <integer name="grid_y" value="%d"/>
        <vector name="cam_dir" value="1, 0, 0"/>
        <float name="cam_dist" value="%.9g"/>
        <boolean name="cam_center" value="true"/>
        <float name="focus_distance" value="4"/>
        <transform name="to_world">%s</transform>
        <wrap type="any">
            <string name="wrap_class" value="sensor"/>
            <string name="wrap_type" value="perspective"/>
            <float name="fov" value="%.9g"/>
            <string name="fov_axis" value="smaller"/>
            <float name="near_clip" value="0.001"/>
            <float name="far_clip" value="1000.0"/>
        </wrap>
        <wrap type="any">
            <string name="wrap_class" value="film"/>
            <string name="wrap_type" value="hdrfilm"/>
            <integer name="width" value="%d"/>
            <integer name="height" value="%d"/>
            <string name="pixel_format" value="rgb"/>
            <rfilter type="box"/>
        </wrap>
        <wrap type="any">
            <string name="wrap_class" value="sampler"/>
            <string name="wrap_type" value="independent"/>
            %s
        </wrap>
    </sensor>""" % (max_depth, rr_depth, G, adaptive, spp_pass, gx, gy, cam_dist, look, fov, res, res, sampler)
    return '<?xml version="1.0" encoding="utf-8"?>\n<scene version="3.0.0">%s\n%s\n%s\n</scene>\n' % (head, shapes, extra)


def _surface(rho, le):
    s = ""
    if rho is not None:
        s += '<bsdf type="diffuse"><rgb name="reflectance" value="%s"/></bsdf>' % _rgb(rho)
    if le is not None:
        s += '<emitter type="area"><rgb name="radiance" value="%s"/></emitter>' % _rgb(le)
    return s


_WALLS = ('<rotate x="1" angle="-90"/><translate y="-1"/>', '<rotate x="1" angle="90"/><translate y="1"/>',
          '<translate z="-1"/>', '<rotate y="1" angle="180"/><translate z="1"/>',
          '<rotate y="1" angle="-90"/><translate x="1"/>', '<rotate y="1" angle="90"/><translate x="-1"/>')


def enclosure_shapes(kind, rho=RHO, le=LE):
    """A closed box [-1, 1]^3 that emits `le` and reflects `rho` everywhere, seen from inside: "rects" six inward
    unit rectangles, "cube" one cube mesh with flip_normals, "sphere" a flipped sphere of radius 2."""
    if kind == "rects":
        return "\n".join('<shape type="rectangle"><transform name="to_world">%s</transform>%s</shape>' % (
            w, _surface(rho, le)) for w in _WALLS)
    if kind == "cube":
        return '<shape type="cube"><boolean name="flip_normals" value="true"/>%s</shape>' % _surface(rho, le)
    assert kind == "sphere"
    return ('<shape type="sphere"><float name="radius" value="2"/><boolean name="flip_normals" value="true"/>%s</shape>'
            % _surface(rho, le))


ENCLOSURE_CAMERA = dict(origin=(0.3, 0.1, 0.2), target=(-0.2, -0.3, -1.0), fov=70.0)


def enclosure_radiance(max_depth, rho=RHO, le=LE):
    rho, le = np.asarray(rho, np.float64), np.asarray(le, np.float64)
    if max_depth == -1:
        return le / (1.0 - rho)
    assert max_depth >= 1
    return le * (1.0 - rho ** max_depth) / (1.0 - rho)


# family B: a floor (y = 0, 40 x 40) under a sphere light and a one-sided rectangle light facing down, both outside
# the frustum of a camera that looks down at the floor, wholly above it, and neither in front of the other from any
# floor point in view
FLOOR_RHO = 0.6
SPHERE_LIGHT = dict(center=(-2.5, 2.5, -1.0), radius=0.5, radiance=(10.0, 8.0, 6.0))
RECT_LIGHT = dict(center=(2.5, 3.0, 1.0), half=(0.7, 0.5), radiance=(4.0, 6.0, 9.0))
FLOOR_CAMERA = dict(origin=(0.0, 3.0, 6.0), target=(0.0, 0.0, 0.0), fov=8.0)
ENV_RADIANCE = 0.5


def floor_shapes(sphere=None, rect=None, env=None):
    """sphere / rect: the light's sampling_weight (None: no such light); env: the environment's radiance."""
    s = ['<shape type="rectangle"><transform name="to_world"><scale value="20"/><rotate x="1" angle="-90"/></transform>'
         '<bsdf type="diffuse"><rgb name="reflectance" value="%s"/></bsdf></shape>' % _rgb((FLOOR_RHO,) * 3)]
    if sphere is not None:
        s.append('<shape type="sphere"><point name="center" x="%.9g" y="%.9g" z="%.9g"/><float name="radius" value="%.9g"/>'
                 '<emitter type="area"><rgb name="radiance" value="%s"/><float name="sampling_weight" value="%.9g"/>'
                 '</emitter></shape>' % (SPHERE_LIGHT["center"] + (SPHERE_LIGHT["radius"], _rgb(SPHERE_LIGHT["radiance"]), sphere)))
    if rect is not None:
        s.append('<shape type="rectangle"><transform name="to_world"><scale x="%.9g" y="%.9g"/><rotate x="1" angle="90"/>'
                 '<translate x="%.9g" y="%.9g" z="%.9g"/></transform>'
                 '<emitter type="area"><rgb name="radiance" value="%s"/><float name="sampling_weight" value="%.9g"/>'
                 '</emitter></shape>' % (RECT_LIGHT["half"] + RECT_LIGHT["center"] + (_rgb(RECT_LIGHT["radiance"]), rect)))
    if env is not None:
        s.append('<emitter type="constant"><rgb name="radiance" value="%s"/></emitter>' % _rgb((env,) * 3))
    return "\n".join(s)


def _sphere_factor(p):
    """projected solid angle / pi of the sphere light over floor points p (n = +y): (r/d)^2 cos(theta)"""
    v = np.asarray(SPHERE_LIGHT["center"], np.float64) - p
    d2 = (v * v).sum(-1)
    return SPHERE_LIGHT["radius"] ** 2 / d2 * v[..., 1] / np.sqrt(d2)


def _rect_factor(p):
    """projected solid angle / pi of the rectangle light over floor points p: Lambert's polygon formula,
    |sum_i gamma_i (Gamma_i . n)| / (2 pi) with gamma_i the angle the edge i subtends and Gamma_i the unit normal
    of the triangle (p, v_i, v_i+1)"""
    c, (hx, hz) = np.asarray(RECT_LIGHT["center"], np.float64), RECT_LIGHT["half"]
    corners = [c + np.array(o) for o in ((-hx, 0, -hz), (hx, 0, -hz), (hx, 0, hz), (-hx, 0, hz))]
    total = 0.0
    for a, b in zip(corners, corners[1:] + corners[:1]):
        va, vb = a - p, b - p
        va = va / np.linalg.norm(va, axis=-1, keepdims=True)
        vb = vb / np.linalg.norm(vb, axis=-1, keepdims=True)
        gamma = np.arccos(np.clip((va * vb).sum(-1), -1.0, 1.0))
        n = np.cross(va, vb)
        total = total + gamma * n[..., 1] / np.linalg.norm(n, axis=-1)
    return np.abs(total) / (2.0 * np.pi)


def floor_radiance(p, sphere=False, rect=False, env=None):
    """(..., 3) outgoing radiance of the floor at points p (..., 3) at max_depth 2"""
    p = np.asarray(p, np.float64)
    out = np.zeros(p.shape[:-1] + (3,))
    covered = 0.0
    if sphere:
        f = _sphere_factor(p)
        out += f[..., None] * np.asarray(SPHERE_LIGHT["radiance"])
        covered = covered + f
    if rect:
        f = _rect_factor(p)
        out += f[..., None] * np.asarray(RECT_LIGHT["radiance"])
        covered = covered + f
    if env is not None:
        out += ((1.0 - covered) * env)[..., None]
    return FLOOR_RHO * out


# family C
FURNACE_SPHERE_CAMERA = dict(origin=(0.0, 0.0, 5.0), target=(0.0, 0.0, 0.0), fov=10.0)
_TH, _PH, _DIST = np.radians(50.0), np.radians(30.0), 60.0
PLATE_CAMERA = dict(origin=(_DIST * np.sin(_TH) * np.cos(_PH), _DIST * np.sin(_TH) * np.sin(_PH), _DIST * np.cos(_TH)),
                    target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), fov=0.6)
FURNACE_ENV = '<emitter type="constant"><rgb name="radiance" value="1, 1, 1"/></emitter>'


def furnace_sphere_shapes(rho=RHO):
    return '<shape type="sphere"><float name="radius" value="1"/>%s</shape>' % _surface(rho, None)


def plate_shapes(distr, sample_visible, alpha):
    """a rough-conductor rectangle in the xy plane (normal +z, alpha_u along x), 6 x 6"""
    return ('<shape type="rectangle"><transform name="to_world"><scale value="3"/></transform>'
            '<bsdf type="roughconductor"><string name="distribution" value="%s"/>'
            '<boolean name="sample_visible" value="%s"/><float name="alpha_u" value="%.9g"/><float name="alpha_v" value="%.9g"/>'
            '<rgb name="eta" value="%s"/><rgb name="k" value="%s"/></bsdf></shape>' % (
                distr, "true" if sample_visible else "false", alpha[0], alpha[1], _rgb(ETA), _rgb(KAPPA)))


def fresnel_conductor(c, eta, k):
    """unpolarised Fresnel reflectance of a conductor of index eta + i k at cos(theta_i) = c (exact)"""
    c2 = c * c
    s2 = 1.0 - c2
    t = eta * eta - k * k - s2
    a2b2 = np.sqrt(t * t + 4.0 * eta * eta * k * k)
    a = np.sqrt(np.maximum(0.5 * (a2b2 + t), 0.0))
    rs = (a2b2 + c2 - 2.0 * a * c) / (a2b2 + c2 + 2.0 * a * c)
    rp = rs * (c2 * a2b2 + s2 * s2 - 2.0 * a * c * s2) / (c2 * a2b2 + s2 * s2 + 2.0 * a * c * s2)
    return 0.5 * (rs + rp)


def _g1(distr, v, m, au, av):
    """exact Smith shadowing of direction v for the microfacet normal m (Beckmann: the erf form, not a fit)"""
    cos = v[..., 2]
    sin2 = np.maximum(1.0 - cos * cos, 1e-300)
    a2 = (v[..., 0] ** 2 * au * au + v[..., 1] ** 2 * av * av) / sin2     # projected roughness^2
    tan2 = sin2 / np.maximum(cos * cos, 1e-300)
    if distr == "ggx":
        g = 2.0 / (1.0 + np.sqrt(1.0 + a2 * tan2))
    else:
        a = 1.0 / np.sqrt(np.maximum(a2 * tan2, 1e-300))
        g = 2.0 / (1.0 + erf(a) + np.exp(-a * a) / (a * np.sqrt(np.pi)))
    return np.where(((v * m).sum(-1) * cos > 0.0) & (cos > 0.0), g, 0.0)


def conductor_albedo(distr, alpha, wi, n_theta=1000, n_phi=2000):
    """(3,) directional albedo of the rough conductor for the incident direction wi (unit, local frame, z up):
    int F(wi.m) D(m) G1(wi, m) G1(wo, m) (wi.m) / cos(theta_i) dw_m, midpoint rule over the microfacet hemisphere"""
    au, av = alpha
    wi = np.asarray(wi, np.float64)
    out = np.zeros(3)
    th = (np.arange(n_theta) + 0.5) * (0.5 * np.pi / n_theta)
    rows = max(1, 2_000_000 // n_phi)
    ph = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    cp, sp = np.cos(ph), np.sin(ph)
    for r0 in range(0, n_theta, rows):
        t = th[r0:r0 + rows, None]
        st, ct = np.sin(t), np.cos(t)
        m = np.stack([st * cp, st * sp, ct + 0.0 * cp], -1)
        e = (m[..., 0] / au) ** 2 + (m[..., 1] / av) ** 2
        if distr == "ggx":
            D = 1.0 / (np.pi * au * av * (e + ct * ct) ** 2)
        else:
            D = np.exp(-e / (ct * ct)) / (np.pi * au * av * ct ** 4)
        im = (m * wi).sum(-1)
        wo = 2.0 * im[..., None] * m - wi
        w = D * _g1(distr, wi, m, au, av) * _g1(distr, wo, m, au, av) * np.maximum(im, 0.0) * st
        for c in range(3):
            out[c] += (w * fresnel_conductor(np.maximum(im, 0.0), ETA[c], KAPPA[c])).sum()
    return out * (0.5 * np.pi / n_theta) * (2.0 * np.pi / n_phi) / wi[2]


@functools.lru_cache(maxsize=None)
def plate_albedo(distr, alpha):
    """(albedo (3,), quadrature error bound (3,), spread over the frame (3,)) for the plate seen by PLATE_CAMERA.
    The bound is the change from half the resolution (the rule converges at least linearly, so the remaining error
    is below it); the spread is the mean over the frame's four corner directions less the centre, at the coarse
    resolution -- what evaluating at the centre alone leaves out."""
    o = np.asarray(PLATE_CAMERA["origin"], np.float64)
    wi = o / np.linalg.norm(o)
    fine = conductor_albedo(distr, alpha, wi)
    coarse = conductor_albedo(distr, alpha, wi, 500, 1000)
    # the frame's corners on the plate (z = 0): rays through the corners of a fov-0.6 square image
    fwd = -wi
    right = np.cross(fwd, np.asarray(PLATE_CAMERA["up"], np.float64))
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    tn = np.tan(np.radians(0.5 * PLATE_CAMERA["fov"]))
    corners = []
    for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        d = fwd + tn * (sx * right + sy * upv)
        p = o - d * (o[2] / d[2])
        w = o - p
        corners.append(conductor_albedo(distr, alpha, w / np.linalg.norm(w), 200, 400))
    centre = conductor_albedo(distr, alpha, wi, 200, 400)
    return fine, np.abs(fine - coarse), np.abs(np.mean(corners, 0) - centre)


# ---------------------------------------------------------------------------------------------------------------
# analytic images from primary hits

def block_mean(a, n):
    H, W = a.shape[0] // n, a.shape[1] // n
    return a.reshape(H, n, W, n, *a.shape[2:]).mean(axis=(1, 3))


def floor_image(hits_of, **lights):
    """Analytic (H, W, 3) image of a family-B scene: floor_radiance at the primary hits of `hits_of(scale)` (the
    oracle's primary_hits at `scale` x the resolution), 3 x 3 supersampled.  Asserts that every pixel centre at
    either scale hits the floor (shape 0, y = 0, normal +y): nothing is masked.  Returns (image, largest relative
    difference between the image means of the 1 x and the 3 x evaluation, per channel).  The n x n midpoint rule
    errs as 1 / n^2, so the 3 x image itself is an eighth of that difference from the pixel means."""
    imgs = []
    for scale in (1, 3):
        h = hits_of(scale)
        assert (h[..., 0] == 0).all(), "a pixel misses the floor"
        assert np.abs(h[..., 5]).max() < 1e-4 and (h[..., 2] > 0.999).all()
        imgs.append(block_mean(floor_radiance(h[..., 4:7], **lights), scale))
    return imgs[1], float(np.abs(imgs[0].mean(axis=(0, 1)) / imgs[1].mean(axis=(0, 1)) - 1.0).max())


# ---------------------------------------------------------------------------------------------------------------
# gates

FLOOR = 2e-4   # f32 film accumulation (tests/test_gpu_unbiased.py test_pooled_energy_c5_shape)


def pooled_ratio(raw, analytic):
    """Pooled ratio of means per channel of K raw frames (K, H, W, 4: RGB sums and W) to the analytic radiance
    ((3,) or (H, W, 3)): sum RGB / sum (W x analytic) over pixels and frames, with its jackknife standard error over
    the frames (the independent units).  Returns (ratio (3,), se (3,))."""
    raw = np.asarray(raw, np.float64)
    A = np.broadcast_to(np.asarray(analytic, np.float64), raw.shape[1:3] + (3,))
    num = raw[..., :3].sum(axis=(1, 2))
    den = (raw[..., 3:4] * A).sum(axis=(1, 2))
    n = len(raw)
    full = num.sum(0) / den.sum(0)
    loo = (num.sum(0) - num) / (den.sum(0) - den)
    return full, np.sqrt((n - 1) / n * ((loo - loo.mean(0)) ** 2).sum(0))


def exact_gate(ratio, se, floor=FLOOR):
    """|ratio - 1| < 4 SE + floor on every channel"""
    return bool((np.abs(ratio - 1.0) < 4.0 * se + floor).all())


def describe(name, ratio, se):
    z = np.where(se > 1e-12, (ratio - 1.0) / np.maximum(se, 1e-12), 0.0)
    return "%-34s ratio %s  se %s  z %s" % (name, np.array2string(ratio, precision=5, floatmode="fixed"),
                                            np.array2string(se, precision=5, floatmode="fixed"),
                                            np.array2string(z, precision=2, floatmode="fixed"))


def pixel_z_gate(raw, analytic, significance=0.01):
    """One-sample form of the Z-test of tests/test_gpu_unbiased.py `_z_gate`: z = |mean over frames of the developed
    pixel - analytic| / SE per pixel channel, two-sided p-value, Sidak-corrected level over the channels.  Returns
    (fraction of channels passing, smallest p, level)."""
    raw = np.asarray(raw, np.float64)
    assert (raw[..., 3] > 0).all(), "a pixel received no sample"
    dev = raw[..., :3] / raw[..., 3:4]
    diff = np.abs(dev.mean(0) - analytic)
    se = dev.std(0, ddof=1) / np.sqrt(len(dev))
    z = np.where(diff == 0.0, 0.0, diff / np.maximum(se, 1e-12))
    p = 2.0 * (1.0 - 0.5 * (1.0 + erf(z / np.sqrt(2.0))))
    alpha = 1.0 - (1.0 - significance) ** (1.0 / z.size)
    return float((p > alpha).mean()), float(p.min()), alpha


# ---------------------------------------------------------------------------------------------------------------
# cases (shared by the CPU and the GPU file; `render(xml, seed)` returns one raw frame (H, W, 4), `hits(xml)` the
# oracle's primary hits)

DEPTHS = ((1, 5), (2, 5), (3, 5), (6, 5), (-1, 5), (12, 2))   # (max_depth, rr_depth)
GRIDS = ((2, 2, 4), (4, 2, 8))                                # (grid_x, grid_y, views per group)


def enclosure_cases():
    """Family A.  `path` at every depth; `mvpath` without max_depth 1 (there the reference adds the primary vertex's
    emitter sample whatever the depth limit, mvpath_multi.h:248-267 against :531, so the answer is no closed form);
    the adaptive fill on a 4 x 2 grid in groups of 4.  In the enclosure every primary hit is an emitter with a BSDF,
    so no view is reused (mvpath_multi.h:205) and every lane is flagged for the fill (:307)."""
    cases = []
    for kind in ("rects", "cube"):
        for depth, rr in DEPTHS:
            cases.append(dict(id="%s-path-D%d-rr%d" % (kind, depth, rr), kind=kind, integrator="path", grid=None,
                              depth=depth, rr=rr, adaptive=0))
        for grid in GRIDS:
            for depth, rr in DEPTHS[1:]:
                cases.append(dict(id="%s-mvpath-%dx%d-G%d-D%d-rr%d" % ((kind,) + grid + (depth, rr)), kind=kind,
                                  integrator="mvpath", grid=grid, depth=depth, rr=rr, adaptive=0))
    for adaptive in (1, 2, 3):
        for depth in (2, 6):
            cases.append(dict(id="rects-mvpath-4x2-G4-D%d-adaptive%d" % (depth, adaptive), kind="rects",
                              integrator="mvpath", grid=(4, 2, 4), depth=depth, rr=5, adaptive=adaptive))
    return cases


N_ENCLOSURE_CASES = 2 * (6 + 2 * 5) + 6


def enclosure_frames(case, render, K, res, spp):
    """K raw frames of an enclosure case, frame k with render seed k.  The adaptive fill forks the sampler and seeds
    it with its own lane count alone (mvpath_multi.h:87-88; sampler.cpp:125-129: base seed + that count), so with one
    sampler the fill of every pass of every frame draws the same numbers whatever the render seed.  Frames are then
    not independent, and neither are the passes of one frame.  The adaptive cases therefore give each frame its own
    sampler `seed` property and render it in one pass."""
    assert K <= 16   # mvpath seeds pass p of frame k with 16 p + k (mvpath.cpp:227): frame k + 16 would repeat streams

    def xml(k):
        adaptive = case["adaptive"]
        return scene_xml(enclosure_shapes(case["kind"]), case["integrator"], case["depth"], case["rr"], res=res, spp=spp,
                         grid=case["grid"], adaptive=adaptive, spp_pass=spp if adaptive else 16,
                         sampler_seed=1000 * (k + 1) if adaptive else 0, **ENCLOSURE_CAMERA)
    return np.stack([np.asarray(render(xml(k), k), np.float64) for k in range(K)])


FLOOR_LIGHTS = (("sphere", dict(sphere=1.0)), ("rect", dict(rect=1.0)),
                ("both-w1-1", dict(sphere=1.0, rect=1.0)), ("both-w0.2-3", dict(sphere=0.2, rect=3.0)),
                ("both-w3-0.5", dict(sphere=3.0, rect=0.5)),
                ("env-w1-1", dict(sphere=1.0, rect=1.0, env=ENV_RADIANCE)),
                ("env-w0.2-3", dict(sphere=0.2, rect=3.0, env=ENV_RADIANCE)),
                ("env-w3-0.5", dict(sphere=3.0, rect=0.5, env=ENV_RADIANCE)))


def floor_cases():
    """Family B: every light set through `path` and through `mvpath` on a 2 x 2 grid, groups of 4."""
    return [dict(id="%s-%s" % (name, integ), lights=kw, integrator=integ, grid=grid)
            for name, kw in FLOOR_LIGHTS for integ, grid in (("path", None), ("mvpath", (2, 2, 4)))]


N_FLOOR_CASES = 16


def floor_case(case, render, hits, K, res, spp):
    """(raw frames, analytic image, 1 x against 3 x difference of the image mean) of a floor case"""
    kw = case["lights"]
    assert K <= 16   # as in enclosure_frames

    def xml(r):
        return scene_xml(floor_shapes(**kw), case["integrator"], 2, 5, res=r, spp=spp, grid=case["grid"], cam_dist=0.3,
                         **FLOOR_CAMERA)
    analytic, d13 = floor_image(lambda scale: hits(xml(res * scale)), sphere="sphere" in kw, rect="rect" in kw,
                                env=kw.get("env"))
    raw = np.stack([np.asarray(render(xml(res), k), np.float64) for k in range(K)])
    return raw, analytic, d13


# |pooled ratio - 1| of the CPU oracle at 16 frames of 8 x 8 pixels x 5120 spp (5.2e6 samples per case, SE 1.3e-4 to
# 2.6e-4) against the exact albedo.  The reference's Beckmann G1 is a rational fit and its visible-normal sampling
# inverts a fitted erf, so these are not derivable; the gate's floor is max(2e-4, twice the value).  DESIGN.md
# section 2 lists them.
PLATE_MEASURED = {("ggx", True, (0.3, 0.3)): 8e-5, ("ggx", False, (0.3, 0.3)): 2e-5,
                  ("ggx", True, (0.15, 0.45)): 2e-5, ("ggx", False, (0.15, 0.45)): 4e-5,
                  ("beckmann", True, (0.3, 0.3)): 1.7e-4, ("beckmann", False, (0.3, 0.3)): 1.4e-4,
                  ("beckmann", True, (0.15, 0.45)): 8e-5, ("beckmann", False, (0.15, 0.45)): 1.4e-4}


def plate_cases():
    return [dict(id="%s-%s-a%g-%g" % ((distr, "visible" if vis else "plain") + alpha), distr=distr, vis=vis, alpha=alpha)
            for distr in ("ggx", "beckmann") for vis in (True, False) for alpha in ((0.3, 0.3), (0.15, 0.45))]


def plate_floor(case):
    measured = PLATE_MEASURED[(case["distr"], case["vis"], case["alpha"])]
    assert measured <= 5e-4, "a deviation above 5e-4 is a finding to explain, not a floor"
    return max(FLOOR, 2.0 * measured)


def plate_frames(case, render, K, res, spp):
    xml = scene_xml(plate_shapes(case["distr"], case["vis"], case["alpha"]), "path", 2, 5, res=res, spp=spp,
                    extra=FURNACE_ENV, **PLATE_CAMERA)
    return np.stack([np.asarray(render(xml, k), np.float64) for k in range(K)]), xml


def furnace_sphere_frames(render, K, res, spp):
    xml = scene_xml(furnace_sphere_shapes(), "path", 2, 5, res=res, spp=spp, extra=FURNACE_ENV, **FURNACE_SPHERE_CAMERA)
    return np.stack([np.asarray(render(xml, k), np.float64) for k in range(K)]), xml


# ---------------------------------------------------------------------------------------------------------------
# the checks themselves (one body for both files; `sizes` = dict(K, res, spp_path, spp_mvpath, spp_adaptive))

_FRAMES = {}   # (backend name, family, case id) -> (frames, analytic) of the cases the power checks reuse


def _keep(name, family, case_id, raw, analytic):
    if (family, case_id) in POWER_CASES:
        _FRAMES[(name, family, case_id)] = (raw, analytic)


def _spp(sizes, integrator, adaptive=0):
    """the adaptive cases render in ONE pass (enclosure_frames), so they carry their own, smaller sample count"""
    if adaptive:
        return sizes["spp_adaptive"]
    return sizes["spp_path"] if integrator == "path" else sizes["spp_mvpath"]


def check_enclosure(backend, case, sizes):
    name, render, _ = backend
    raw = enclosure_frames(case, render, sizes["K"], sizes["res"], _spp(sizes, case["integrator"], case["adaptive"]))
    assert np.isfinite(raw).all() and (raw[..., 3] > 0).all()
    analytic = enclosure_radiance(case["depth"])
    ratio, se = pooled_ratio(raw, analytic)
    _keep(name, "enclosure", case["id"], raw, analytic)
    print(describe(case["id"], ratio, se))
    assert exact_gate(ratio, se), "enclosure radiance off: " + describe(case["id"], ratio, se)


def check_floor(backend, case, sizes):
    name, render, hits = backend
    raw, analytic, d13 = floor_case(case, render, hits, sizes["K"], sizes["res"], _spp(sizes, case["integrator"]))
    assert np.isfinite(raw).all()
    ratio, se = pooled_ratio(raw, analytic)
    _keep(name, "floor", case["id"], raw, analytic)
    frac, pmin, alpha = pixel_z_gate(raw, analytic)
    print(describe(case["id"], ratio, se), " 1x/3x %.2e  pixel gate %.5f (min p %.3g, level %.3g)" % (d13, frac, pmin, alpha))
    assert d13 < 0.1 * (4.0 * se.min() + FLOOR), "the analytic image is not converged: 1x against 3x %.2e" % d13
    assert exact_gate(ratio, se), "floor radiance off: " + describe(case["id"], ratio, se)
    assert frac >= 0.9975, "Z-test rejects: only %.4f of the pixel channels pass" % frac


def check_furnace_sphere(backend, sizes):
    name, render, hits = backend
    raw, xml = furnace_sphere_frames(render, sizes["K"], sizes["res"], sizes["spp_path"])
    assert (hits(xml)[..., 0] == 0).all(), "the sphere does not fill the frame"
    analytic = np.asarray(RHO)
    ratio, se = pooled_ratio(raw, analytic)
    _keep(name, "sphere", "sphere", raw, analytic)
    print(describe("furnace-diffuse-sphere", ratio, se))
    assert exact_gate(ratio, se), "furnace sphere off: " + describe("sphere", ratio, se)


def check_plate(backend, case, sizes):
    name, render, hits = backend
    raw, xml = plate_frames(case, render, sizes["K"], sizes["res"], sizes["spp_path"])
    assert (hits(xml)[..., 0] == 0).all(), "the plate does not fill the frame"
    albedo, qerr, spread = plate_albedo(case["distr"], case["alpha"])
    ratio, se = pooled_ratio(raw, albedo)
    floor = plate_floor(case)
    _keep(name, "plate", case["id"], raw, albedo)
    print(describe(case["id"], ratio, se), " floor %.1e  quadrature %.1e  over the frame %.1e" % (
        floor, (qerr / albedo).max(), (spread / albedo).max()))
    tenth = 0.1 * (4.0 * se.min() + floor)
    assert (qerr / albedo).max() < tenth and (spread / albedo).max() < tenth, "the quadrature is not converged"
    assert exact_gate(ratio, se, floor), "conductor albedo off: " + describe(case["id"], ratio, se)


POWER_CASES = (("enclosure", "rects-path-D6-rr5"), ("enclosure", "rects-mvpath-4x2-G8-D6-rr5"),
               ("floor", "both-w1-1-path"), ("sphere", "sphere"), ("plate", "ggx-visible-a0.15-0.45"))


def check_power(backend, family, case_id, sizes):
    """The gate rejects a 1 % error: the same frames against 1.01 x the analytic value."""
    key = (backend[0], family, case_id)
    if key not in _FRAMES:
        if family == "enclosure":
            check_enclosure(backend, [c for c in enclosure_cases() if c["id"] == case_id][0], sizes)
        elif family == "floor":
            check_floor(backend, [c for c in floor_cases() if c["id"] == case_id][0], sizes)
        elif family == "sphere":
            check_furnace_sphere(backend, sizes)
        else:
            check_plate(backend, [c for c in plate_cases() if c["id"] == case_id][0], sizes)
    raw, analytic = _FRAMES[key]
    ratio, se = pooled_ratio(raw, 1.01 * np.asarray(analytic))
    floor = FLOOR if family != "plate" else plate_floor([c for c in plate_cases() if c["id"] == case_id][0])
    print(describe(case_id + " x1.01", ratio, se))
    assert not exact_gate(ratio, se, floor), "a 1 %% error passes: " + describe(case_id, ratio, se)

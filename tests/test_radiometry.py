"""The CPU oracle against closed-form radiometry (tests/radiometry.py), on every CPU run.

The GPU tests pin the HIP pipeline to the oracle bit for bit, and the oracle is a restatement of the reference:
an error the two share is invisible to them.  These scenes have exact answers -- a uniform enclosure, direct light
on a diffuse floor, a furnace -- so they check the oracle's emitter sampling and pdfs (rectangle, sphere cone,
mesh area CDF, constant environment, sampling_weight), the BSDF / emitter MIS, max_depth / rr_depth bookkeeping,
Russian roulette, flip_normals, emitting reflectors and the rough-conductor product against something that is not a
restatement.  About 2e5 samples per case (16 frames): errors of a percent fail; tests/test_gpu_radiometry.py runs the
same cases on the device at 1e7 samples.

Gate (tests/test_gpu_unbiased.py's): the pooled ratio of means over the frames against the analytic value,
|ratio - 1| < 4 SE + 2e-4, SE by jackknife over the frames; per pixel on the floor, the Sidak Z-gate.
"""
import os

import numpy as np
import pytest

import radiometry as R

SIZES = dict(K=16, res=8, spp_path=192, spp_mvpath=32, spp_adaptive=32)
# the floor's analytic image converges as 1 / res^2 (radiometry.floor_image): 16 x 16 keeps 1 x against 3 x under a
# tenth of this file's gate
FLOOR_SIZES = dict(K=16, res=16, spp_path=48, spp_mvpath=16)


@pytest.fixture(scope="module")
def backend(amvpt_mod, oracle):
    threads = min(16, os.cpu_count() or 4)
    last = {}

    def scene(xml):
        if last.get("xml") != xml:
            last["xml"], last["scene"] = xml, amvpt_mod.load_string(xml)
        return last["scene"]

    def render(xml, seed):
        sd, vd, p = scene(xml).describe(0, seed, 0)
        return oracle.render(sd, vd, p, threads=threads)[0]

    def hits(xml):
        sd, vd, p = scene(xml).describe(0, 0, 0)
        return oracle.primary_hits(sd, vd, p)
    return "oracle", render, hits


def test_case_counts():
    """every case the families list is parametrised below: none is dropped silently"""
    assert len(R.enclosure_cases()) == R.N_ENCLOSURE_CASES == 38
    assert len(R.floor_cases()) == R.N_FLOOR_CASES == 16
    assert len(R.plate_cases()) == len(R.PLATE_MEASURED) == 8
    ids = [c["id"] for c in R.enclosure_cases() + R.floor_cases() + R.plate_cases()]
    assert len(set(ids)) == len(ids)
    assert not [c for c in R.enclosure_cases() if c["integrator"] == "mvpath" and c["depth"] == 1]


def test_closed_forms_agree_with_each_other():
    """the float64 answers against independent forms: the enclosure series written out, the polygon formula against
    a brute-force form-factor sum over the light, and the conductor quadrature against a bound that is tight for a
    smooth plate with F = 1"""
    assert np.allclose(R.enclosure_radiance(3, (0.5,), (2.0,)), 2.0 * (1 + 0.5 + 0.25))
    assert np.allclose(R.enclosure_radiance(-1, (0.5,), (2.0,)), 4.0)
    # Lambert's formula against cos cos A / (pi d^2) summed over a fine grid of the light
    p = np.array([0.3, 0.0, -0.4])
    c, (hx, hz) = np.asarray(R.RECT_LIGHT["center"]), R.RECT_LIGHT["half"]
    n = 400
    u = (np.arange(n) + 0.5) / n * 2 - 1
    q = c + np.stack(np.meshgrid(u * hx, [0.0], u * hz, indexing="ij"), -1).reshape(-1, 3)
    v = q - p
    d2 = (v * v).sum(-1)
    brute = ((v[:, 1] / np.sqrt(d2)) ** 2 / d2).sum() * (4 * hx * hz / n ** 2) / np.pi
    assert abs(R._rect_factor(p) / brute - 1) < 1e-5
    # (r/d)^2 cos(theta) against the same sum over the side of the sphere that faces the point
    sc, r = np.asarray(R.SPHERE_LIGHT["center"]), R.SPHERE_LIGHT["radius"]
    mu, ph = (np.arange(n) + 0.5) / n * 2 - 1, (np.arange(2 * n) + 0.5) / (2 * n) * 2 * np.pi
    st = np.sqrt(1 - mu * mu)[:, None]
    ns = np.stack([st * np.cos(ph), st * np.sin(ph), mu[:, None] + 0 * ph], -1).reshape(-1, 3)
    v = sc + r * ns - p
    d2 = (v * v).sum(-1)
    facing = np.maximum(-(ns * v).sum(-1) / np.sqrt(d2), 0.0)
    brute = (v[:, 1] / np.sqrt(d2) * facing / d2).sum() * (4 * np.pi * r * r / len(ns)) / np.pi
    assert abs(R._sphere_factor(p) / brute - 1) < 1e-4
    # conductor quadrature with F = 1 (k huge) at normal incidence: the integrand is D cos(theta_m) G1(wo), and wo
    # leaves the hemisphere where theta_m > 45 degrees, which holds 1 - 1 / (1 + alpha^2) of GGX's projected area.
    # So the albedo is at most 1 / (1 + alpha^2), and at alpha 0.05 shadowing takes little more (measured 9e-5).
    saved = R.ETA, R.KAPPA
    try:
        R.ETA, R.KAPPA = (1.0,) * 3, (1e6,) * 3
        a = R.conductor_albedo("ggx", (0.05, 0.05), np.array([0.0, 0.0, 1.0]), 800, 800)
    finally:
        R.ETA, R.KAPPA = saved
    bound = 1.0 / (1.0 + 0.05 ** 2)
    assert (a <= bound).all() and (a > bound - 3e-4).all(), (a, bound)


@pytest.mark.parametrize("case", R.enclosure_cases(), ids=[c["id"] for c in R.enclosure_cases()])
def test_enclosure(backend, case):
    R.check_enclosure(backend, case, SIZES)


@pytest.mark.parametrize("case", R.floor_cases(), ids=[c["id"] for c in R.floor_cases()])
def test_floor(backend, case):
    R.check_floor(backend, case, FLOOR_SIZES)


def test_furnace_diffuse_sphere(backend):
    R.check_furnace_sphere(backend, SIZES)


@pytest.mark.parametrize("case", R.plate_cases(), ids=[c["id"] for c in R.plate_cases()])
def test_furnace_rough_conductor(backend, case):
    R.check_plate(backend, case, SIZES)


@pytest.mark.parametrize("family,case_id", R.POWER_CASES, ids=[c[1] for c in R.POWER_CASES])
def test_gate_rejects_one_percent(backend, family, case_id):
    R.check_power(backend, family, case_id, FLOOR_SIZES if family == "floor" else SIZES)

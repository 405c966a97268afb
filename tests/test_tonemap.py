"""The tone-mapping stage on the host (include/amvpt_tonemap.h): the host entries against a numpy restatement of the
header's definition written here -- the binning from the float's bits, the exposure from the histogram in float64, the
three operators in float64 -- and the properties the definition is there for.  The device entries are held to these
host entries bit for bit by tests/test_gpu_tonemap.py."""
import ctypes
import math

import numpy as np
import pytest

f32 = np.float32
# 2^(j/16), j = 1 .. 15, rounded to float32: the table of csrc/dtonemap.h
TABLE = np.array([2.0 ** (j / 16.0) for j in range(1, 16)], dtype=np.float64).astype(np.float32)
FLT_MAX = float(np.finfo(np.float32).max)
# skipped: 0, -0, negatives, denormals, NaN, +-inf and 2^-17; counted: 2^-16 (bin 0), 2^16 and FLT_MAX (bin 511)
SKIPPED = [0.0, -0.0, -1.0, -1e-30, 1e-40, 1.4e-45, float("nan"), float("inf"), float("-inf"), 2.0 ** -17]
COUNTED = [(2.0 ** -16, 0), (2.0 ** 16, 511), (FLT_MAX, 511)]


@pytest.fixture(scope="module")
def A(amvpt_mod):
    amvpt_mod.hip_lib()
    return amvpt_mod


def lum32(img):
    """pp_lum: float32, unfused, Rec. 709."""
    img = np.asarray(img, dtype=np.float32)
    return (f32(0.2126) * img[..., 0] + f32(0.7152) * img[..., 1]) + f32(0.0722) * img[..., 2]


def bins_ref(L):
    """The bin of every float32 luminance (-1: skipped), from the bits as the header says."""
    L = np.ascontiguousarray(L, dtype=np.float32).ravel()
    u = L.view(np.uint32)
    e = ((u >> 23) & 0xff).astype(np.int64)
    s = ((u & np.uint32(0x7fffff)) | np.uint32(0x3f800000)).view(np.float32)
    j = (s[:, None] >= TABLE[None, :]).sum(axis=1)
    b = 16 * (e - 111) + j
    b[e >= 143] = 511
    b[((u >> 31) != 0) | (e == 255) | (e < 111)] = -1
    return b


def hist_ref(img, rect=None):
    if rect is not None:
        x0, y0, w, h = rect
        img = img[y0:y0 + h, x0:x0 + w]
    b = bins_ref(lum32(img))
    return np.bincount(b[b >= 0], minlength=512).astype(np.uint32), int((b < 0).sum())


def exposure_ref(A, hist, q, frames, l_prev, exposure_prev):
    """The exposure step of the header over Python ints and float64 -> (frames, exposure, log2_exposure)."""
    N = int(hist.sum())
    if N == 0:
        if frames == 0:
            return 0, f32(float(q.key) * A.tonemap_exp2_host(float(q.ev))), float(q.ev)
        return frames, exposure_prev, l_prev
    n_lo, n_hi = int(math.floor(float(q.lo) * N)), int(math.floor(float(q.hi) * N))
    n_hi = min(max(n_hi, n_lo + 1), N)
    S = M = cum = 0
    for b in range(512):
        end = cum + int(hist[b])
        ov = max(0, min(end, n_hi) - max(cum, n_lo))
        S, M, cum = S + ov * b, M + ov, end
    mean = -16.0 + (S / M + 0.5) / 16.0
    target = min(max(float(q.ev) - mean, float(q.min_ev)), float(q.max_ev))
    l = target if frames == 0 else l_prev + (target - l_prev) * float(q.adapt)
    return frames + 1, f32(float(q.key) * A.tonemap_exp2_host(l)), l


def check_state(A, s, img, q, before=(0, 0.0, f32(0)), rect=None):
    """The whole state after metering `img` against the restatement; `before` is (frames, l, exposure) going in."""
    hist, skipped = hist_ref(img, rect)
    assert np.array_equal(s.histogram(), hist)
    assert (s.counted, s.skipped) == (int(hist.sum()), skipped)
    frames, ex, l = exposure_ref(A, hist, q, before[0], before[1], before[2])
    assert s.frames == frames
    assert f32(s.exposure).view(np.uint32) == f32(ex).view(np.uint32), (s.exposure, ex)
    assert np.float64(s.log2_exposure).view(np.uint64) == np.float64(l).view(np.uint64), (s.log2_exposure, l)
    return frames, l, f32(ex)


def gray(values, channels=3):
    v = np.asarray(values, dtype=np.float32).reshape(1, -1, 1)
    img = np.repeat(v, channels, axis=2)
    if channels == 4:
        img[..., 3] = 0.25
    return np.ascontiguousarray(img)


def bin_gray(counts):
    """A gray image with counts[b] pixels in the middle of bin b."""
    vals = [2.0 ** ((b + 0.5) / 16.0 - 16.0) for b, n in counts.items() for _ in range(n)]
    img = gray(vals)
    got = np.bincount(bins_ref(lum32(img)), minlength=512)
    assert all(got[b] == n for b, n in counts.items()) and got.sum() == sum(counts.values())
    return img


# ---------------------------------------------------------------------------------------------------- binning

def test_version_and_defaults(A):
    assert A.tonemap_version() == 1
    q = A.tonemap_default_params()
    assert q.values() == A.TonemapParams().values()
    assert (q.op, q.auto_exposure, q.ev, q.adapt, q.white, q.min_ev, q.max_ev) == (0, 0, 0.0, 1.0, 4.0, -16.0, 16.0)
    assert (f32(q.key), f32(q.lo), f32(q.hi)) == (f32(0.18), f32(0.10), f32(0.95))
    assert ctypes.sizeof(A.TonemapState) == 512 * 4 + 16 + 8


def test_bins_follow_log2(A):
    """10^5 luminances over 2^-20 .. 2^20: the bin is floor(16 (log2 L + 16)) in float64, away from the bin edges (within
    1e-6 relative of one the float32 table decides); below 2^-16 skipped, from 2^16 on bin 511."""
    rng = np.random.default_rng(3)
    L = np.exp2(rng.uniform(-20.0, 20.0, 100000)).astype(np.float32)
    img = gray(L)
    assert np.array_equal(lum32(img).ravel() > 0, np.ones(L.size, dtype=bool))
    lum = lum32(img).ravel().astype(np.float64)
    t = 16.0 * (np.log2(lum) + 16.0)
    want = np.clip(np.floor(t), -1, 511).astype(np.int64)
    want[t < 0] = -1
    got = bins_ref(lum32(img))
    away = np.abs(t - np.rint(t)) > 16.0 * 1e-6 / math.log(2.0) * 1.01
    assert away.mean() > 0.99
    assert np.array_equal(got[away], want[away])
    s = A.tonemap_meter_host(img)
    assert np.array_equal(s.histogram(), np.bincount(got[got >= 0], minlength=512))
    assert (s.counted, s.skipped) == (int((got >= 0).sum()), int((got < 0).sum()))
    # one pixel at a time, so that a pixel in a wrong bin cannot hide behind another
    for v in L[:200]:
        one = A.tonemap_meter_host(gray([v]))
        b = int(bins_ref(lum32(gray([v])))[0])
        assert (one.skipped == 1 and one.counted == 0) if b < 0 else (one.hist[b] == 1 and one.counted == 1)


def test_lower_edges_and_specials(A):
    """Exact powers of two and the fifteen table values land on the lower edge of their bin, the float below them in
    the bin before; the specials split as the header says.  An edge is metered through the host entry where a pixel
    (0, g, 0) exists whose float32 luminance is exactly the edge (more than half of them), else through the
    restatement alone."""
    def exact(L):
        with np.errstate(over="ignore"):
            g = f32(np.float64(L) / np.float64(f32(0.7152)))
        for cand in (g, np.nextafter(g, f32(np.inf)), np.nextafter(g, f32(0))):
            if (f32(0.2126) * f32(0) + f32(0.7152) * cand) + f32(0.0722) * f32(0) == f32(L):
                return [0.0, float(cand), 0.0]
        return None
    edges = [(f32(2.0 ** e), 16 * (e + 16)) for e in range(-16, 16)]
    edges += [(TABLE[j - 1] * f32(2.0 ** e), 16 * (e + 16) + j) for e in (-16, -3, 0, 15) for j in range(1, 16)]
    hit = 0
    for L, b in edges:
        assert int(bins_ref(np.array([L]))[0]) == b
        below = np.nextafter(f32(L), f32(0))
        assert int(bins_ref(np.array([below]))[0]) == b - 1
        px = exact(L)
        if px is None:
            continue
        hit += 1
        s = A.tonemap_meter_host(np.array([[px]], dtype=np.float32))
        assert s.hist[b] == 1 and s.counted == 1, (L, b)
    assert hit > len(edges) // 2
    for v in SKIPPED:
        s = A.tonemap_meter_host(gray([v]))
        assert (s.counted, s.skipped, int(s.histogram().sum())) == (0, 1, 0), v
    for v, b in COUNTED:
        px = exact(v) or [v, v, v]
        s = A.tonemap_meter_host(np.array([[px]], dtype=np.float32))
        assert (s.counted, s.skipped, s.hist[b]) == (1, 0, 1), v
    # a NaN in one channel only is a NaN luminance
    s = A.tonemap_meter_host(np.array([[[1.0, float("nan"), 1.0]]], dtype=np.float32))
    assert (s.counted, s.skipped) == (0, 1)


def test_rect_restricts_the_metering(A):
    rng = np.random.default_rng(5)
    img = np.exp2(rng.uniform(-8, 8, (13, 17, 4))).astype(np.float32)
    q = A.TonemapParams(auto_exposure=True)
    for rect in ((3, 1, 7, 5), (0, 2, 17, 3), (16, 12, 1, 1), (0, 0, 17, 13)):
        check_state(A, A.tonemap_meter_host(img, q, rect=rect), img, q, rect=rect)
    whole, full = A.tonemap_meter_host(img, q), A.tonemap_meter_host(img, q, rect=(0, 0, 17, 13))
    assert bytes(whole) == bytes(full)


# ---------------------------------------------------------------------------------------------------- exp2_pm

def test_exp2_pm(A):
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-40.0, 40.0, 10000), np.arange(-40.0, 41.0), [-0.5, 0.5, 39.5, -39.5]])
    got = np.array([A.tonemap_exp2_host(v) for v in x])
    want = np.exp2(x)
    rel = np.abs(got - want) / want
    assert rel.max() < 1e-12, rel.max()
    ints = np.arange(-40.0, 41.0)
    assert np.array_equal(np.array([A.tonemap_exp2_host(v) for v in ints]), np.exp2(ints))


# ---------------------------------------------------------------------------------------------------- exposure

def test_exposure_cases_equal_the_restatement(A):
    q = A.TonemapParams(auto_exposure=True)
    # a trimmed window that cuts a bin at both ends: n_lo = 10 inside bin 100, n_hi = 95 inside bin 300
    img = bin_gray({100: 37, 200: 50, 300: 13})
    check_state(A, A.tonemap_meter_host(img, q), img, q)
    # lo = 0, hi = 1: every counted pixel
    q01 = A.TonemapParams(auto_exposure=True, lo=0.0, hi=1.0)
    check_state(A, A.tonemap_meter_host(img, q01), img, q01)
    # N == 0 on a fresh state: l = ev, frames stays 0
    black = np.zeros((3, 5, 3), dtype=np.float32)
    qe = A.TonemapParams(auto_exposure=True, ev=1.5)
    s = A.tonemap_meter_host(black, qe)
    check_state(A, s, black, qe)
    assert (s.frames, s.counted, s.skipped, s.log2_exposure) == (0, 0, 15, 1.5)
    # ... and on a used one: l, exposure and frames stay, the histogram is the black frame's
    s = A.tonemap_meter_host(img, q)
    before = (s.frames, s.log2_exposure, f32(s.exposure))
    assert before[0] == 1
    A.tonemap_meter_host(black, q, state=s)
    check_state(A, s, black, q, before=before)
    assert (s.frames, s.log2_exposure, f32(s.exposure)) == before and s.counted == 0
    # N == 1: n_lo = n_hi = 0, n_hi raised to 1
    one = np.zeros((2, 2, 3), dtype=np.float32)
    one[1, 0] = 0.37
    s = A.tonemap_meter_host(one, q)
    check_state(A, s, one, q)
    assert (s.counted, s.skipped, s.frames) == (1, 3, 1)
    # n_hi raised to n_lo + 1 inside a larger frame: N = 5, lo = 0.5, hi = 0.55 -> [2, 3)
    qn = A.TonemapParams(auto_exposure=True, lo=0.5, hi=0.55)
    img5 = bin_gray({10: 1, 20: 1, 250: 1, 400: 1, 500: 1})
    s = A.tonemap_meter_host(img5, qn)
    check_state(A, s, img5, qn)
    assert s.log2_exposure == -(-16.0 + 250.5 / 16.0)
    # both clamps
    lo_clamp = A.TonemapParams(auto_exposure=True, min_ev=-2.0, max_ev=3.0)
    dark, bright = bin_gray({40: 9}), bin_gray({480: 9})
    s = A.tonemap_meter_host(dark, lo_clamp)
    check_state(A, s, dark, lo_clamp)
    assert s.log2_exposure == 3.0
    s = A.tonemap_meter_host(bright, lo_clamp)
    check_state(A, s, bright, lo_clamp)
    assert s.log2_exposure == -2.0


def test_a_uniform_frame_is_brought_to_the_key(A):
    """exposure * L is within a factor 2^(1/32) of the key: the histogram knows L to the middle of a bin of a sixteenth
    of an octave.  L = 1 lies on a bin's lower edge, where the factor is reached exactly: log2_exposure, the float64 the
    exposure is formed from, is held to the bound itself (|l + log2 L| <= 1/32), the float32 exposure to the bound and
    its own rounding (a relative 2^-24, and as much again for exp2_pm and the product)."""
    q = A.TonemapParams(auto_exposure=True)
    for L in (3e-4, 0.02, 0.18, 1.0, 346.9, 5e3):
        s = A.tonemap_meter_host(np.full((4, 6, 3), L, dtype=np.float32), q)
        lum = float(lum32(np.full((1, 1, 3), L, dtype=np.float32))[0, 0])
        assert abs(s.log2_exposure + math.log2(lum)) <= 1 / 32 + 1e-15, (L, s.log2_exposure)
        ratio = s.exposure * lum / float(q.key)
        slack = 1.0 + 2.0 ** -23
        assert 2.0 ** (-1 / 32) / slack <= ratio <= 2.0 ** (1 / 32) * slack, (L, ratio)


def test_scaling_the_frame_scales_the_exposure(A):
    rng = np.random.default_rng(11)
    img = np.exp2(rng.normal(-2.0, 1.5, (24, 31, 3))).astype(np.float32)
    q = A.TonemapParams(auto_exposure=True)
    base = A.tonemap_meter_host(img, q)
    for k in range(-3, 4):
        s = A.tonemap_meter_host(img * f32(2.0 ** k), q)
        assert abs(s.log2_exposure) < 15.0
        assert abs(s.exposure * 2.0 ** k / base.exposure - 1.0) < 1e-6, k


def test_a_few_burnt_pixels_do_not_move_the_exposure(A):
    """The brightest 3 % of the pixels raised a thousandfold stay inside the 5 % the default window trims."""
    rng = np.random.default_rng(13)
    img = np.exp2(rng.normal(-1.0, 1.0, (40, 50, 3))).astype(np.float32)
    q = A.TonemapParams(auto_exposure=True)
    lum = lum32(img).ravel()
    top = np.argsort(lum)[-int(0.03 * lum.size):]
    burnt = img.copy().reshape(-1, 3)
    burnt[top] *= f32(1000.0)
    a, b = A.tonemap_meter_host(img, q), A.tonemap_meter_host(burnt.reshape(img.shape), q)
    assert not np.array_equal(a.histogram(), b.histogram())
    assert f32(a.exposure).view(np.uint32) == f32(b.exposure).view(np.uint32) and a.log2_exposure == b.log2_exposure


def test_adaptation_closes_a_quarter_of_the_gap(A):
    q = A.TonemapParams(auto_exposure=True, adapt=0.25)
    first, then = bin_gray({120: 20}), bin_gray({330: 20})
    s = A.tonemap_meter_host(first, q)
    before = check_state(A, s, first, q)
    jump = -(-16.0 + 120.5 / 16.0)
    assert s.log2_exposure == jump and s.frames == 1      # a fresh state jumps
    target = -(-16.0 + 330.5 / 16.0)
    gap = target - s.log2_exposure
    for n in range(1, 7):
        A.tonemap_meter_host(then, q, state=s)
        before = check_state(A, s, then, q, before=before)
        assert s.frames == n + 1
        assert abs((target - s.log2_exposure) / gap - 0.75 ** n) < 1e-12


# ---------------------------------------------------------------------------------------------------- operators

GRID = [0.0, -0.0, -1.0, -0.25, 1e-8, 1e-3, 0.18, 0.5, 1.0, 7.5, 1e4, 2.0 ** 61, float("inf"), float("nan")]
W = [float(f32(0.2126)), float(f32(0.7152)), float(f32(0.0722))]
C = {k: float(f32(k)) for k in (2.51, 0.03, 2.43, 0.59, 0.14)}


def operator_ref(img, q, exposure):
    """The three operators in float64 over the float32 inputs (H, W, 3)."""
    x = img[..., :3].astype(np.float64) * float(exposure)
    with np.errstate(all="ignore"):
        if q.op == 0:
            return x
        if q.op == 1:
            L = (W[0] * x[..., 0] + W[1] * x[..., 1]) + W[2] * x[..., 2]
            s = (1.0 + L / (float(q.white) * float(q.white))) / (1.0 + L)
            s = np.where(np.isfinite(L) & (L > 0), s, 1.0)
            return x * s[..., None]
        y = x * (C[2.51] * x + C[0.03]) / (x * (C[2.43] * x + C[0.59]) + C[0.14])
        y = np.where(x > 2.0 ** 60, C[2.51] / C[2.43], y)
        y = np.where(x <= 0, 0.0, y)
        return np.where(np.isnan(x), np.nan, y)


def manual_exposure(A, q):
    return f32(float(q.key) / 0.18 * A.tonemap_exp2_host(float(q.ev)))


def assert_within_ulp(got, want, n=4):
    got = np.asarray(got, dtype=np.float32)
    with np.errstate(all="ignore"):
        w32 = want.astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    inf = np.isinf(w32)
    assert np.array_equal(got[inf], w32[inf])
    ok = ~nan & ~inf
    tol = n * np.spacing(np.abs(w32[ok])).astype(np.float64)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    assert (err <= tol).all(), (got[ok][err > tol][:4], want[ok][err > tol][:4])


def operator_image():
    rng = np.random.default_rng(17)
    colours = np.exp2(rng.uniform(-12, 6, (40, 3))).astype(np.float32)
    return np.concatenate([gray(GRID)[0], colours]).reshape(2, -1, 3)


@pytest.mark.parametrize("op", ["linear", "reinhard", "aces"])
@pytest.mark.parametrize("ev", [0.0, -2.0, 3.0])
def test_operators_against_float64(A, op, ev):
    img = operator_image()
    q = A.TonemapParams(op=op, ev=ev, white=2.5)
    got = A.tonemap_host(img, q)
    assert_within_ulp(got, operator_ref(img, q, manual_exposure(A, q)))
    if op == "aces":   # the ends of the fit
        ex = float(manual_exposure(A, q))
        g = A.tonemap_host(gray([-1.0, 0.0, 2.0 ** 61, float("inf")]), q)[0, :, 0]
        assert g.tolist() == [0.0, 0.0, float(f32(2.51) / f32(2.43)), float(f32(2.51) / f32(2.43))] and ex > 0


@pytest.mark.parametrize("op", ["linear", "reinhard", "aces"])
def test_the_metered_exposure_is_the_one_applied(A, op):
    img = operator_image()
    q = A.TonemapParams(op=op, auto_exposure=True)
    s = A.tonemap_meter_host(img, q)
    assert s.frames == 1 and s.exposure > 0
    assert_within_ulp(A.tonemap_host(img, q, state=s), operator_ref(img, q, f32(s.exposure)))
    auto8 = A.tonemap_srgb8_host(img, q, state=s)
    import amvpt.display as D
    assert np.array_equal(auto8, D.srgb8(A.tonemap_host(img, q, state=s)))


def test_linear_at_ev_0_is_srgb8(A):
    import amvpt.display as D
    rng = np.random.default_rng(19)
    for c in (3, 4):
        img = (rng.random((23, 37, c), dtype=np.float32) * f32(1.25) - f32(0.125))
        img[3, 5, :3] = (np.nan, np.inf, -np.inf)
        assert manual_exposure(A, A.TonemapParams()) == f32(1.0)
        assert np.array_equal(A.tonemap_srgb8_host(img), D.srgb8(img))
        same = A.tonemap_host(img)
        assert np.array_equal(same.view(np.uint32), img.view(np.uint32))
    for op in ("reinhard", "aces"):   # the fused bytes are the curve of the mapped floats
        q = A.TonemapParams(op=op, ev=1.0)
        assert np.array_equal(A.tonemap_srgb8_host(img, q), D.srgb8(A.tonemap_host(img, q)))


def test_alpha_passes_and_in_place_equals_out_of_place(A):
    rng = np.random.default_rng(23)
    img = np.exp2(rng.uniform(-6, 6, (9, 11, 4))).astype(np.float32)
    img[..., 3] = rng.random((9, 11), dtype=np.float32)
    img[0, 0, 3] = np.nan
    for op in ("linear", "reinhard", "aces"):
        q = A.TonemapParams(op=op, ev=-1.0)
        out = A.tonemap_host(img, q)
        assert np.array_equal(out[..., 3].view(np.uint32), img[..., 3].view(np.uint32))
        three = A.tonemap_host(np.ascontiguousarray(img[..., :3]), q)
        assert np.array_equal(out[..., :3].view(np.uint32), three.view(np.uint32))
        work = img.copy()
        assert A.tonemap_host(work, q, in_place=True) is work
        assert np.array_equal(work.view(np.uint32), out.view(np.uint32))


def test_display_keyword(A):
    """tonemap=None is the default (the device test compares the bytes); a tone mapper needs a fresh frame."""
    import inspect

    import amvpt.display as D
    from conftest import SCENES
    assert inspect.signature(D.display).parameters["tonemap"].default is None
    s = A.load_file(SCENES + "/cbox_grid.xml", res=8, spp=4)
    with pytest.raises(ValueError, match="tone mapping needs a fresh frame"):
        D.display(s, size=(16, 8), tonemap=A.ToneMapper(), rerender=False)


# ---------------------------------------------------------------------------------------------------- refusals

def test_refusals_by_name(A):
    L = A.hip_lib()
    img = np.full((3, 4, 3), 0.5, dtype=np.float32)
    P = A.TonemapParams

    def refuses(match, fn, *a, **k):
        with pytest.raises(RuntimeError, match=match):
            fn(*a, **k)

    bad = [(P(op=3), "unknown op 3"), (P(key=0.0), "key must be above 0"), (P(key=-1.0), "key must be above 0"),
           (P(white=0.0), "white must be above 0"), (P(lo=-0.1), "lo and hi"), (P(hi=1.5), "lo and hi"),
           (P(lo=0.5, hi=0.5), "lo and hi"), (P(lo=0.7, hi=0.6), "lo and hi"), (P(adapt=-0.1), "adapt must be 0 .. 1"),
           (P(adapt=1.5), "adapt must be 0 .. 1"), (P(min_ev=2.0, max_ev=1.0), "min_ev is above max_ev")]
    for field in ("ev", "key", "lo", "hi", "adapt", "white", "min_ev", "max_ev"):
        for v in (float("nan"), float("inf")):
            bad.append((P(**{field: v}), "params: %s is not finite" % field))
    for q, words in bad:
        refuses("amvpt_tonemap_srgb8_host: .*" + words, A.tonemap_srgb8_host, img, q)
        refuses("amvpt_tonemap_apply_host: .*" + words, A.tonemap_host, img, q)
        refuses("amvpt_tonemap_meter_host: .*" + words, A.tonemap_meter_host, img, q)
    auto = P(auto_exposure=True)
    refuses("amvpt_tonemap_srgb8_host: null state with auto_exposure set", A.tonemap_srgb8_host, img, auto)
    refuses("amvpt_tonemap_apply_host: null state with auto_exposure set", A.tonemap_host, img, auto)
    for c in (1, 2, 5):
        other = np.zeros((3, 4, c), dtype=np.float32)
        refuses("channels must be 3 or 4, not %d" % c, A.tonemap_srgb8_host, other)
        refuses("channels must be 3 or 4, not %d" % c, A.tonemap_host, other)
        refuses("channels must be 3 or 4, not %d" % c, A.tonemap_meter_host, other)
    refuses("amvpt_tonemap_srgb8_host: width is 0", A.tonemap_srgb8_host, np.zeros((3, 0, 3), dtype=np.float32))
    refuses("amvpt_tonemap_apply_host: height is 0", A.tonemap_host, np.zeros((0, 4, 3), dtype=np.float32))
    refuses("amvpt_tonemap_meter_host: width is 0", A.tonemap_meter_host, np.zeros((3, 0, 3), dtype=np.float32))
    for rect, words in (((0, 0, 0, 2), "rect: zero area"), ((0, 0, 2, 0), "rect: zero area"),
                        ((4, 0, 1, 1), "rect: outside the image"), ((2, 0, 3, 1), "rect: outside the image"),
                        ((0, 3, 1, 1), "rect: outside the image"), ((0, 1, 1, 3), "rect: outside the image"),
                        ((1, 1, 2 ** 32 - 1, 1), "rect: outside the image")):
        refuses("amvpt_tonemap_meter_host: " + words, A.tonemap_meter_host, img, rect=rect)

    # what the numpy wrappers cannot form: null pointers, 2^32 pixels (refused before a byte is read), overlaps
    q, s = P(), A.TonemapState()
    out = np.zeros((3, 4, 3), dtype=np.float32)
    ptr = img.ctypes.data

    def rc(code, words):
        assert code == 1 and words in L.amvpt_last_error().decode(), L.amvpt_last_error().decode()

    rc(L.amvpt_tonemap_meter_host(None, 3, 4, 3, None, ctypes.byref(q), ctypes.addressof(s)), "null image")
    rc(L.amvpt_tonemap_meter_host(ptr, 3, 4, 3, None, None, ctypes.addressof(s)), "null params")
    rc(L.amvpt_tonemap_meter_host(ptr, 3, 4, 3, None, ctypes.byref(q), None), "null state")
    rc(L.amvpt_tonemap_apply_host(ptr, 3, 4, 3, ctypes.byref(q), None, None), "null out")
    rc(L.amvpt_tonemap_srgb8_host(None, 3, 4, 3, ctypes.byref(q), None, out.ctypes.data), "null image")
    rc(L.amvpt_tonemap_meter_host(ptr, 3, 65536, 65536, None, ctypes.byref(q), ctypes.addressof(s)),
       "width * height is 2^32 pixels or more")
    big = (ctypes.c_uint32 * 4)(0, 0, 2 ** 31, 2)
    rc(L.amvpt_tonemap_meter_host(ptr, 3, 2 ** 31, 2, ctypes.byref(big), ctypes.byref(q), ctypes.addressof(s)),
       "rect: 2^32 pixels or more")
    rc(L.amvpt_tonemap_apply_host(ptr, 3, 4, 3, ctypes.byref(q), None, ptr + 4), "out overlaps the image")
    rc(L.amvpt_tonemap_srgb8_host(ptr, 3, 4, 3, ctypes.byref(q), None, ptr), "out overlaps the image")
    rc(L.amvpt_tonemap_meter_host(ptr, 3, 4, 3, None, ctypes.byref(q), ptr + 8), "state overlaps the image")
    assert bytes(s) == bytes(A.TonemapState())   # no refused call touched the state

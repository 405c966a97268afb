"""The display stage on the host: 8-bit sRGB quilt, lenticular interlacing, presets.csv, PNG (amvpt_display.h).

The interlacer is integer and unfused IEEE float32 arithmetic ending in a byte, so it is pinned byte for byte:
`restate_interlace` / `restate_views` below restate the screenshot branch of Program::display_image
(src/mitsuba/program.cpp:199-276) and interpolate2d (src/mitsuba/util.h:104-129) in numpy, every operation in
np.float32 and every truncating cast where the reference truncates.  The known answers (tests/golden/
display_kats.json) are CRC-32s of such restated images; a fused multiply-add in `z` moves 5 of the 15552 view
indices of the 96 x 54 case, so equality also catches a contracted build.  The sRGB curve is compared with
IEC 61966-2-1 evaluated in float64; where that value lies within 1e-3 of a half-integer either neighbouring code is
accepted (a float32 powf evaluation deviates by at most 4.3e-5 code units, so the band leaves a factor of 20; the
library evaluates the curve in float64 and stays 1e-12 from it), and the band may exempt at most 1 % of the ramp (the
float64 reference alone puts 9 of 4096 values inside).  None of this needs a GPU.
"""
import ctypes
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest

from conftest import REPO, SCENES

F = np.float32
KATS = json.load(open(os.path.join(REPO, "tests", "golden", "display_kats.json")))
CBOX = os.path.join(SCENES, "cbox_grid.xml")
DISPLAY_HEADER = os.path.join(REPO, "include", "amvpt_display.h")
HOST_HEADER = os.path.join(REPO, "include", "amvpt_host.h")
INVALID = 1   # AMVPT_ERR_INVALID


@pytest.fixture(scope="module")
def D(amvpt_mod):
    import amvpt.display as display
    return display


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def _clip(v):
    return np.minimum(np.maximum(v, F(0)), F(1))


def _coords(preset, quilt, dw, dh):
    """(x, y, z1) of every subpixel, shape (dh, dw, 3), float32: steps 1-3 of display_image."""
    center, focus, pitch, tilt, subp = (F(preset[k]) for k in ("center", "focus", "pitch", "tilt", "subp"))
    vx, vy = F(preset["view"][0]), F(preset["view"][1])
    gx, gy = F(preset["grid"][0]), F(preset["grid"][1])
    grid_n = F(preset["grid"][0] * preset["grid"][1])
    grid_scl = F(1) / grid_n
    igx, igy = F(1) / gx, F(1) / gy
    sx = F(1) / (F(3 * dw) - F(1))
    sy = F(1) / (F(dh) - F(1))
    y0 = (np.arange(dh, dtype=np.uint32).astype(F) * sy)[:, None, None]
    x0 = ((np.arange(dw, dtype=np.uint32) * np.uint32(3)).astype(F) * sx)[None, :, None]   # over the byte index
    c = np.arange(3, dtype=np.uint32).astype(F)[None, None, :]
    x0 = np.broadcast_to(x0, (dh, dw, 3)).astype(F)
    y0 = np.broadcast_to(y0, (dh, dw, 3)).astype(F)
    z = pitch * ((x0 + c * subp) + (F(1) - y0) * tilt) - center
    z = F(1) - (z - np.floor(z))
    z1 = np.floor(z * grid_n)
    z2 = np.floor((F(1) - z) * grid_n)
    w = focus * (F(1) - F(2) * _clip(z1 * grid_scl))
    X = (z1 - gx * np.floor(z1 / gx)) + _clip(x0 + w)
    Y = np.floor(z2 * igx) + y0          # igrid.x, as the reference has it
    for a in (z, z1, z2, w, X, Y):
        assert a.dtype == F
    if quilt:
        return x0, y0, z1
    return _clip((vx * igx) * X), _clip((vy * igy) * Y), z1


def _lerp2_u8(a, b, t):
    v = (F(1) - t) * a.astype(F) + t * b.astype(F)
    assert v.dtype == F
    return v.astype(np.uint8)   # T = uint8_t: truncated


def restate_interlace(src, preset, dw, dh, quilt=False, nearest=False):
    sh, sw, _ = src.shape
    X, Y, _ = _coords(preset, quilt, dw, dh)
    x = (F(sw) - F(1)) * X
    y = (F(sh) - F(1)) * Y
    ci = np.broadcast_to(np.arange(3)[None, None, :], x.shape)
    if nearest:
        return src[(y + F(0.5)).astype(np.uint32), (x + F(0.5)).astype(np.uint32), ci]
    x1, y1 = x.astype(np.uint32), y.astype(np.uint32)
    tx, ty = x - x1.astype(F), y - y1.astype(F)
    x2 = np.where(x1 + 1 < sw, x1 + 1, x1)
    y2 = np.where(y1 + 1 < sh, y1 + 1, y1)
    top = _lerp2_u8(src[y1, x1, ci], src[y1, x2, ci], tx)
    bottom = _lerp2_u8(src[y2, x1, ci], src[y2, x2, ci], tx)
    return _lerp2_u8(top, bottom, ty)


def restate_views(preset, dw, dh):
    return _coords(preset, False, dw, dh)[2].astype(np.int32)


def pattern(w, h, nch=3):
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(nch), indexing="ij")
    return ((7 * x + 13 * y + 29 * c + (x * y) % 11) % 256).astype(np.uint8)


def kat_preset(D, name):
    p = KATS["presets"][name]
    return D.Preset(p["center"], p["focus"], p["pitch"], p["tilt"], p["subp"], tuple(p["view"]), tuple(p["grid"]),
                    name=name)


def srgb_f64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0), 1 / 2.4) - 0.055)


def check_srgb8_ramp(codes):
    """`codes`: the 8-bit codes of the ramp i/4095 (as float32), against rint(255 srgb(x)) in float64."""
    spec = KATS["srgb8_ramp"]
    n = spec["n"]
    x = (np.arange(n, dtype=np.float64) / (n - 1)).astype(F)
    v = 255.0 * srgb_f64(x.astype(np.float64))
    want = np.rint(v)
    near_half = np.abs(v - np.floor(v) - 0.5) <= spec["band"]
    assert near_half.sum() <= spec["band_cap"] * n
    codes = np.asarray(codes).astype(np.int64)
    ok = (codes == want) | (near_half & ((codes == np.floor(v)) | (codes == np.ceil(v))))
    assert ok.all(), (np.flatnonzero(~ok)[:8], codes[~ok][:8], v[~ok][:8])
    for i, code in spec["spots"].items():
        assert codes[int(i)] == code, (i, codes[int(i)], code)
    return int(near_half.sum())


def ramp_image():
    n = KATS["srgb8_ramp"]["n"]
    x = (np.arange(n, dtype=np.float64) / (n - 1)).astype(F)
    return np.repeat(x.reshape(64, n // 64, 1), 3, axis=2).copy()   # 64 x 64 x 3, every channel the ramp


def special_values():
    s = KATS["srgb8_special"]
    return np.array([float(t) for t in s["in"]], dtype=F), np.array(s["out"], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# known answers: the restatement itself, then the library against it
# ---------------------------------------------------------------------------------------------------------------
def _case_id(k):
    return "%dx%d-%dx%d-%s-%s-%s" % (k["src"][0], k["src"][1], k["dst"][0], k["dst"][1], k["preset"],
                                     "quilt" if k["quilt"] else "lenticular", "nearest" if k["nearest"] else "bilinear")


@pytest.mark.parametrize("k", KATS["interlace"], ids=_case_id)
def test_interlace_known_answers(D, k):
    src = pattern(*k["src"])
    dw, dh = k["dst"]
    want = restate_interlace(src, KATS["presets"][k["preset"]], dw, dh, k["quilt"], k["nearest"])
    if "crc" in k:
        assert "%08x" % zlib.crc32(want.tobytes()) == k["crc"]
    if "pixel00" in k:
        assert want[0, 0].tolist() == k["pixel00"]
    if "image" in k:
        assert want.tolist() == k["image"]
    got = D.interlace(src, kat_preset(D, k["preset"]), (dw, dh), quilt=k["quilt"], nearest=k["nearest"])
    assert got.shape == (dh, dw, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # a 4-channel source gives the same bytes as its 3-channel part
    src4 = np.concatenate([src, (255 - src[:, :, :1])], axis=2)
    got4 = D.interlace(src4, kat_preset(D, k["preset"]), (dw, dh), quilt=k["quilt"], nearest=k["nearest"])
    assert np.array_equal(got4, want)


@pytest.mark.parametrize("k", KATS["views"], ids=lambda k: k["preset"])
def test_view_map_known_answers(D, k):
    dw, dh = k["dst"]
    want = restate_views(KATS["presets"][k["preset"]], dw, dh)
    counts = np.bincount(want.ravel())
    assert want.min() == 0 and want.max() == k["n_views"] - 1 and len(counts) == k["n_views"] and counts.min() > 0
    if "crc_u8" in k:
        assert "%08x" % zlib.crc32(want.astype(np.uint8).tobytes()) == k["crc_u8"]
        assert want[0, 0].tolist() == k["first"] and want[-1, -1].tolist() == k["last"]
        assert counts.min() == k["count_min"] and counts.max() == k["count_max"]
    got = D.views(kat_preset(D, k["preset"]), (dw, dh))
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_default_preset_is_lkg4x8(D):
    p = D.default_preset()
    assert p == kat_preset(D, "LKG4x8")
    assert p.values() == (F(-0.5), F(-0.05), F(354.548), F(-0.114), F(0.00013), (1.0, 1.0), (4, 8), False)
    assert D.version() == 1


# ---------------------------------------------------------------------------------------------------------------
# sRGB
# ---------------------------------------------------------------------------------------------------------------
def test_srgb8_ramp_against_float64(D):
    out = D.srgb8(ramp_image())
    assert out.shape == (64, 64, 3) and out.dtype == np.uint8
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    assert check_srgb8_ramp(out[..., 0].ravel()) == KATS["srgb8_ramp"]["float64_in_band"]


def test_srgb8_special_values_and_alpha(D):
    x, want = special_values()
    img3 = np.repeat(x.reshape(1, -1, 1), 3, axis=2)
    got = D.srgb8(img3)
    assert np.array_equal(got, np.repeat(want.reshape(1, -1, 1), 3, axis=2)), got[0, :, 0]
    # alpha is dropped: a 4-channel image gives the codes of its RGB part
    rng = np.random.default_rng(7)
    img4 = rng.random((23, 37, 4), dtype=np.float32) * F(1.25) - F(0.125)
    assert np.array_equal(D.srgb8(img4), D.srgb8(img4[..., :3]))


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
def _refused(L, rc, *words):
    assert rc == INVALID, rc
    msg = L.amvpt_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_refusals_name_the_argument(D, amvpt_mod):
    L, _ = D._libs()
    src = pattern(8, 8)
    dst = np.zeros((4, 4, 3), dtype=np.uint8)
    views = np.zeros((4, 4, 3), dtype=np.int32)
    p = D.default_preset()
    ref = ctypes.byref

    def interlace(sp=src.ctypes.data, sw=8, sh=8, ch=3, preset=ref(p), dp=dst.ctypes.data, dw=4, dh=4):
        return L.amvpt_interlace_host(sp, sw, sh, ch, preset, 0, 0, dp, dw, dh)

    assert interlace() == 0
    _refused(L, interlace(dw=1), "amvpt_interlace_host", "dst_w")
    _refused(L, interlace(dw=0), "dst_w")
    _refused(L, interlace(dh=1), "dst_h")
    _refused(L, interlace(sw=0), "src_w")
    _refused(L, interlace(sh=0), "src_h")
    _refused(L, interlace(ch=2), "src_channels")
    _refused(L, interlace(ch=5), "src_channels")
    _refused(L, interlace(sp=None), "null src")
    _refused(L, interlace(dp=None), "null dst")
    _refused(L, interlace(preset=None), "null preset")
    for i in (0, 1):
        bad = D.default_preset()
        bad.grid[i] = 0
        _refused(L, interlace(preset=ref(bad)), "grid[%d]" % i)
        _refused(L, L.amvpt_interlace_views_host(ref(bad), views.ctypes.data, 4, 4), "amvpt_interlace_views_host",
                 "grid[%d]" % i)
    _refused(L, L.amvpt_interlace_views_host(ref(p), views.ctypes.data, 1, 4), "dst_w")
    _refused(L, L.amvpt_interlace_views_host(ref(p), views.ctypes.data, 4, 1), "dst_h")
    _refused(L, L.amvpt_interlace_views_host(ref(p), None, 4, 4), "null views")
    _refused(L, L.amvpt_interlace_views_host(None, views.ctypes.data, 4, 4), "null preset")

    img = np.zeros((4, 4, 3), dtype=np.float32)
    out = np.zeros((4, 4, 3), dtype=np.uint8)
    assert L.amvpt_srgb8_host(img.ctypes.data, 3, 4, 4, out.ctypes.data) == 0
    _refused(L, L.amvpt_srgb8_host(img.ctypes.data, 2, 4, 4, out.ctypes.data), "amvpt_srgb8_host", "channels")
    _refused(L, L.amvpt_srgb8_host(img.ctypes.data, 3, 0, 4, out.ctypes.data), "width")
    _refused(L, L.amvpt_srgb8_host(img.ctypes.data, 3, 4, 0, out.ctypes.data), "height")
    _refused(L, L.amvpt_srgb8_host(None, 3, 4, 4, out.ctypes.data), "null image")
    _refused(L, L.amvpt_srgb8_host(img.ctypes.data, 3, 4, 4, None), "null out")

    # the device entries refuse the same arguments before they look for a device
    _refused(L, L.amvpt_interlace(src.ctypes.data, 8, 8, 3, ref(p), 0, 0, dst.ctypes.data, 1, 4, None),
             "amvpt_interlace", "dst_w")
    _refused(L, L.amvpt_interlace(None, 8, 8, 3, ref(p), 0, 0, dst.ctypes.data, 4, 4, None), "null src")
    _refused(L, L.amvpt_srgb8(img.ctypes.data, 7, 4, 4, out.ctypes.data, None), "amvpt_srgb8", "channels")
    # one launch covers the image: above 2^33 pixels the device entries refuse by name, before any launch
    _refused(L, L.amvpt_interlace(src.ctypes.data, 8, 8, 3, ref(p), 0, 0, dst.ctypes.data, 1 << 17, 1 << 17, None),
             "dst_w * dst_h", "2^33")
    _refused(L, L.amvpt_srgb8(img.ctypes.data, 3, 1 << 17, 1 << 17, out.ctypes.data, None), "width * height", "2^33")
    with pytest.raises(RuntimeError, match="dst_h"):
        D.interlace(src, p, (4, 1))


def test_host_entries_need_no_device(D, amvpt_mod):
    """The host entries never return AMVPT_ERR_NO_DEVICE: they ran above whether or not a device is visible; the
    device entries without one refuse with that status instead of computing on the CPU."""
    if amvpt_mod.device_count() > 0:
        return
    L, _ = D._libs()
    src = pattern(8, 8)
    dst = np.zeros((4, 4, 3), dtype=np.uint8)
    p = D.default_preset()
    assert L.amvpt_interlace(src.ctypes.data, 8, 8, 3, ctypes.byref(p), 0, 0, dst.ctypes.data, 4, 4, None) == 5
    img = np.zeros((4, 4, 3), dtype=np.float32)
    assert L.amvpt_srgb8(img.ctypes.data, 3, 4, 4, dst.ctypes.data, None) == 5
    s = amvpt_mod.load_file(CBOX, res=8, spp=4)
    with pytest.raises(RuntimeError):
        D.display(s, size=(16, 8))
    with pytest.raises(RuntimeError):
        D.display(s, size=(16, 8), rerender=False)


# ---------------------------------------------------------------------------------------------------------------
# presets.csv, preset_for_scene, PNG
# ---------------------------------------------------------------------------------------------------------------
def test_presets_round_trip_through_csv(D, tmp_path):
    a = D.default_preset()
    b = kat_preset(D, "second")
    c = D.Preset(1 / 3, -2 / 7, 1e-7 + 123.456789, 3e-5, -1.2345678e-4, (0.123456789, 0.987654321), (7, 3),
                 flip_rgb=True, name="odd one")
    path = str(tmp_path / "presets.csv")
    D.write_presets(path, [a, b, c])
    back = D.read_presets(path)
    assert back == [a, b, c]
    assert [p.name for p in back] == ["LKG4x8", "second", "odd one"] and back[2].flip_rgb == 1
    lines = open(path).read().splitlines()
    assert len(lines) == 3 and all(len(l.split(";")) == 11 for l in lines)
    assert lines[0].split(";")[0] == "LKG4x8" and lines[0].split(";")[8:] == ["4", "8", "0"]


def test_hand_written_preset_line_is_the_default(D, tmp_path):
    path = str(tmp_path / "presets.csv")
    with open(path, "w") as f:
        f.write("LKG4x8;-0.5;-0.05;354.548;-0.114;0.00013;1;1;4;8;0\n")
    assert D.read_presets(path) == [D.default_preset()]
    with pytest.raises(RuntimeError, match="Error opening file for reading"):
        D.read_presets(str(tmp_path / "missing.csv"))
    with open(path, "w") as f:
        f.write("short;1;2;3\n")
    with pytest.raises(RuntimeError, match="fields"):
        D.read_presets(path)


def test_preset_for_scene_takes_the_sensor_grid(D, amvpt_mod):
    s = amvpt_mod.load_file(CBOX, res=8, spp=4, gx=4, gy=2)
    p = D.preset_for_scene(s)
    assert tuple(p.grid) == (4, 2)
    d = D.default_preset()
    assert p.values()[:6] == d.values()[:6]
    b = amvpt_mod.load_file(os.path.join(SCENES, "cbox_batch.xml"), res=8, spp=4)
    _, _, bp = b.describe(0, 0, 0)
    assert tuple(D.preset_for_scene(b).grid) == (bp.n_views, 1)


def parse_png(data):
    """(width, height, RGB bytes) of an 8-bit RGB PNG: signature, chunk CRCs, IHDR, zlib.decompress of IDAT."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert zlib.crc32(kind + body) == crc, kind
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    idat = b"".join(body for kind, body in chunks if kind == b"IDAT")
    assert idat
    raw = zlib.decompress(idat)
    assert len(raw) == h * (3 * w + 1)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 3 * w + 1)
    assert not rows[:, 0].any()   # filter type None
    return w, h, rows[:, 1:].tobytes()


@pytest.mark.parametrize("size", [(37, 23), (1, 1), (300, 120)], ids=lambda s: "%dx%d" % s)
def test_write_png_parses_back(D, tmp_path, size):
    """300 x 120 needs more than one stored deflate block (108120 bytes > 65535)."""
    w, h = size
    img = pattern(w, h)
    path = str(tmp_path / "image.png")
    D.write_png(path, img)
    assert parse_png(open(path, "rb").read()) == (w, h, img.tobytes())


# ---------------------------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------------------------
def declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    names = set(re.findall(r"\b(amvpt_[a-z0-9_]+)\s*\(", src))
    return sorted(n for n in names if not n.endswith("_t"))


def test_display_header_is_exported(amvpt_mod):
    L = amvpt_mod.hip_lib()
    names = declared(DISPLAY_HEADER)
    for fn in ("amvpt_display_version", "amvpt_display_default_preset", "amvpt_srgb8", "amvpt_interlace",
               "amvpt_srgb8_host", "amvpt_interlace_host", "amvpt_interlace_views_host"):
        assert fn in names
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_host_header_display_entries_are_exported(amvpt_mod):
    H = amvpt_mod.host_lib()
    names = declared(HOST_HEADER)
    for fn in ("amvpt_host_display", "amvpt_host_display_stream", "amvpt_host_redisplay_stream",
               "amvpt_host_preset_for_scene",
               "amvpt_host_read_presets", "amvpt_host_write_presets", "amvpt_host_write_png"):
        assert fn in names and hasattr(H, fn), fn


def test_abi_version_is_unchanged(amvpt_mod):
    assert amvpt_mod.hip_lib().amvpt_abi_version() == 12

"""The fixed-point film as a first-class target (include/amvpt_fixed.h) on the device: exact frames from any
partition, and the integer LDS-window splat.

`want` is the oracle's fixed-point film of the WHOLE frame (oracle.render(fixed_film=True)); "equal" is every float
bit-equal after ONE fixed_resolve of the summed integers into zeros.  Every partition is driven from this one
process: shares are rendered one after another into integer buffers of their own and summed as integers (a tensor
add, or fixed_accumulate for windows and overflow lists).  The only tolerance in this module is zero.

The window splat (the default) and AMVPT_OPT_FIXED_DIRECT (one global integer atomic per cell add, the parent's
deterministic put) must leave EQUAL int64 films: the same multiset of integers is summed, grouped differently.  That
is the test of the new kernel proper; the comparison with the oracle is the test of the object.

The tent filter is outside the oracle (it knows the Gaussian and the box filter only): its `want` is
tests/test_rfilters.py's numpy restatement of ImageBlock::put over the oracle's records, summed as integers, which
that module anchors on the oracle's own fixed-point film and tests/test_gpu_rfilters.py holds the flag's film to.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENES
from test_adaptive_fill import CBOX, bit_equal, edit_once, oracle_range_counts
from test_rfilters import elem, filter_xml, gaussian_params, put_film, weight_fn_of

pytestmark = pytest.mark.gpu

MESH = os.path.join(SCENES, "cbox_mesh.xml")
VEACH = os.path.join(SCENES, "veach_grid.xml")
CBOX_PATH = os.path.join(SCENES, "cbox_path.xml")
AMVPT_ERR_OOM = 3
G8 = dict(res=16, spp=32, gx=4, gy=2, reuse=8)   # 32768 lanes x 2 passes: test_deterministic_film's shape
BANDS = [(0, 12295), (12295, 20000), (20000, 32768)]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _assert_equal(got, want, what="film"):
    assert got.shape == want.shape and np.abs(want).max() > 0
    bad = np.argwhere(~bit_equal(got, want))
    for y, x, c in bad[:8]:
        print("%s[%d, %d, %d]: got %r, want %r" % (what, y, x, c, got[y, x, c], want[y, x, c]))
    assert len(bad) == 0, "%s: %d of %d floats differ from the oracle's fixed-point film" % (what, len(bad), want.size)


class Frame:
    """A loaded scene, its device scene and (once) the oracle's fixed-point film of the whole frame."""
    _frames = {}

    def __init__(self, amvpt_mod, oracle, scene, xml_edit=None, **kw):
        self.mod, self.oracle = amvpt_mod, oracle
        if xml_edit is not None:
            self.scene = amvpt_mod.load_string(xml_edit(open(scene).read()), **kw)
        else:
            self.scene = amvpt_mod.load_file(scene, **kw)
        self.sd, self.vd, self.p = self.scene.describe(0, 0, 0)
        self.C = 5 if self.p.film_alpha else 4
        self.plan = oracle.plan(self.p)
        self.dev = amvpt_mod.DeviceScene(self.sd)
        self._want = None

    @classmethod
    def of(cls, amvpt_mod, oracle, key, scene, xml_edit=None, **kw):
        if key not in cls._frames:
            cls._frames[key] = cls(amvpt_mod, oracle, scene, xml_edit, **kw)
        return cls._frames[key]

    def want(self):
        if self._want is None:
            film, _, st = self.oracle.render(self.sd, self.vd, self.p, threads=16, fixed_film=True)
            film.setflags(write=False)
            self._want = (film, st)
        return self._want

    def zeros(self, shape=None):
        torch = _torch()
        return torch.zeros(shape or (self.p.film_height, self.p.film_width, self.C), dtype=torch.int64, device="cuda")

    def render_fixed(self, into=None, p=None, **kw):
        """(int64 film tensor, counters) of one render_fixed; `into` accumulates into an existing film."""
        torch = _torch()
        fx = self.zeros() if into is None else into
        cnt = self.mod.Counters()
        self.dev.render_fixed(self.vd, p or self.p, fx.data_ptr(), counters=cnt, **kw)
        torch.cuda.synchronize()
        return fx, cnt

    def resolve(self, fx):
        """One fixed_resolve into zeros (store mode over a film of NaNs would do as well: checked in the whole-frame
        test)."""
        torch = _torch()
        film = torch.zeros(fx.shape, dtype=torch.float32, device="cuda")
        self.mod.fixed_resolve(fx.data_ptr(), film.data_ptr(), fx.numel(), add=True)
        torch.cuda.synchronize()
        return film.cpu().numpy()

    def both_splats(self, **kw):
        """The frame through the integer window and through direct puts: equal int64 films (returned once)."""
        torch = _torch()
        win, cnt = self.render_fixed(**kw)
        direct, cnt_d = self.render_fixed(flags=kw.pop("flags", 0) | self.mod.OPT_FIXED_DIRECT, **kw)
        assert win.abs().max().item() > 0
        ndiff = (win != direct).sum().item()
        assert ndiff == 0, "window splat and direct puts: %d of %d integers differ" % (ndiff, win.numel())
        assert cnt.film_range_drops == cnt_d.film_range_drops
        assert cnt.view_splats == cnt_d.view_splats and cnt.adaptive_lanes == cnt_d.adaptive_lanes
        return win, cnt


@pytest.fixture(scope="module", autouse=True)
def _frames(gpu_ready, amvpt_mod):
    """The process's one-time costs are paid here when this module is the first to use the device (as
    test_gpu_adaptive_fill.py does), so that `--durations` shows each case's own time."""
    torch = _torch()
    s = amvpt_mod.load_file(MESH, res=4, spp=16)
    sd, vd, p = s.describe(0, 0, 0)
    film = torch.zeros((p.film_height, p.film_width, 4), dtype=torch.float32, device="cuda")
    amvpt_mod.DeviceScene(sd).render_ex(vd, p, film.data_ptr())
    torch.cuda.synchronize()
    yield
    Frame._frames.clear()


def _g8(amvpt_mod, oracle, scene="cbox"):
    return Frame.of(amvpt_mod, oracle, "g8_" + scene, CBOX if scene == "cbox" else MESH, **G8)


# ---------------------------------------------------------------------------------------------------
# 1, 2. the whole frame
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["cbox", "mesh"])
def test_whole_frame(gpu_ready, amvpt_mod, oracle, scene):
    """render_fixed, resolved, equal to the oracle; the window splat's integers equal to direct puts'; the same in
    chunks of 3000 lanes (mesh: on chunk streams); and render_ex(OPT_DETERMINISTIC) still gives the same bits."""
    torch = _torch()
    f = _g8(amvpt_mod, oracle, scene)
    assert (f.plan["lanes"], f.plan["passes"]) == (32768, 2)
    want, st = f.want()
    assert st["range_drops"] == 0
    fx, cnt = f.both_splats()
    assert cnt.film_range_drops == 0 and cnt.film_overflow == 0
    assert cnt.as_dict()["kernel_launches"]["k_splat"] > 0
    film = f.resolve(fx)
    _assert_equal(film, want)
    # store mode of the resolve: whatever the film held is overwritten
    stored = torch.full(fx.shape, float("nan"), dtype=torch.float32, device="cuda")
    amvpt_mod.fixed_resolve(fx.data_ptr(), stored.data_ptr(), fx.numel())
    torch.cuda.synchronize()
    _assert_equal(stored.cpu().numpy(), want, "stored film")
    # chunks
    fx3, cnt3 = f.both_splats(chunk_lanes=3000)
    assert cnt3.chunk_lanes == 3000 and f.plan["lanes"] > 3000 * 4
    if scene == "mesh":
        assert cnt3.buffer_sets > 1
    assert (fx3 == fx).all().item()
    # the flag path: a private fixed film over the same kernels, resolved into the caller's float film
    for flags in (amvpt_mod.OPT_DETERMINISTIC, amvpt_mod.OPT_DETERMINISTIC | amvpt_mod.OPT_FIXED_DIRECT):
        ffilm = torch.zeros(fx.shape, dtype=torch.float32, device="cuda")
        fc = amvpt_mod.Counters()
        f.dev.render_ex(f.vd, f.p, ffilm.data_ptr(), flags=flags, counters=fc)
        torch.cuda.synchronize()
        assert fc.film_range_drops == 0
        assert bit_equal(ffilm.cpu().numpy(), film).all()


# ---------------------------------------------------------------------------------------------------
# 3. lane bands
# ---------------------------------------------------------------------------------------------------

def test_lane_bands(gpu_ready, amvpt_mod, oracle):
    """Three uneven lane ranges into three integer films, summed as int64 tensors, resolved once."""
    f = _g8(amvpt_mod, oracle)
    want, _ = f.want()
    total = f.zeros()
    lanes = 0
    for b, e in BANDS:
        fx, cnt = f.render_fixed(lanes=amvpt_mod.LaneSet(b, e, 0, 0, 0, 0))
        assert cnt.lanes == (e - b) * f.plan["passes"] and cnt.film_range_drops == 0
        lanes += cnt.lanes
        total += fx
    assert lanes == f.plan["lanes"] * f.plan["passes"]
    _assert_equal(f.resolve(total), want)


def test_lane_bands_adaptive(gpu_ready, amvpt_mod, oracle):
    """The same bands with adaptive = 2: each band's fill seeds from the whole pass's compressed array, the counts
    for the exchange come from the oracle's count phase (as test_dense_tail_ranges takes them)."""
    f = Frame.of(amvpt_mod, oracle, "g8_adaptive2", CBOX, adaptive=2, **G8)
    assert (f.plan["lanes"], f.plan["passes"]) == (32768, 2)
    want, st = f.want()
    assert st["adaptive_lanes"] > 0
    counts = oracle_range_counts(oracle, f.sd, f.vd, f.p, BANDS)   # [band][pass]
    assert all(len(c) == 2 for c in counts) and sum(sum(c) for c in counts) * 2 == st["adaptive_lanes"]
    total = f.zeros()
    adaptive_lanes = 0
    for r, (b, e) in enumerate(BANDS):
        seen = []

        def exchange(begins, run_counts, r=r, b=b, seen=seen):
            k = len(seen)   # one call per pass
            seen.append((list(begins), list(run_counts)))
            assert (list(begins), list(run_counts)) == ([b], [counts[r][k]])
            return [sum(counts[q][k] for q in range(r))], sum(c[k] for c in counts)
        fx, cnt = f.render_fixed(lanes=amvpt_mod.LaneSet(b, e, 0, 0, 0, 0), exchange=exchange)
        assert len(seen) == 2 and cnt.film_range_drops == 0
        assert cnt.adaptive_lanes == 2 * sum(counts[r])
        adaptive_lanes += cnt.adaptive_lanes
        total += fx
    assert adaptive_lanes == st["adaptive_lanes"]
    _assert_equal(f.resolve(total), want)


# ---------------------------------------------------------------------------------------------------
# 4. view groups with windows and overflow lists
# ---------------------------------------------------------------------------------------------------

C5_SMALL = dict(res=16, spp=16, gx=8, gy=4, reuse=4, adaptive=3)   # test_rect_lanes' shape
OV_CAP = 1 << 19   # direct puts under a tiles-only window list every spilled cell add (2.5e5 a share), the window splat sums first


class ViewGroups:
    """The C5 small frame cut into four view-group shares, and the oracle's run counts of every share."""
    _one = None

    def __init__(self, amvpt_mod, oracle):
        from amvpt import dist as adist
        self.f = Frame.of(amvpt_mod, oracle, "c5_small", CBOX, **C5_SMALL)
        f = self.f
        assert f.plan["group"] == 4 and f.plan["passes"] == 1
        self.part = adist.view_group_partition(f.p, 4, 4)
        assert self.part is not None and len(self.part) == 4
        self.runs = {}
        try:
            for r, (rect, _) in enumerate(self.part):   # count phase, on the oracle
                def counting(begins, counts, r=r):
                    self.runs[r] = (list(begins), list(counts))
                    return adist.exclusive_prefix(begins, counts, begins)
                oracle.set_run_exchange(counting)
                oracle.render_rect(f.sd, f.vd, f.p, rect, threads=16)
        finally:
            oracle.set_run_exchange(None)
        self.allb = sum((self.runs[r][0] for r in range(4)), [])
        self.allc = sum((self.runs[r][1] for r in range(4)), [])

    @classmethod
    def get(cls, amvpt_mod, oracle):
        if cls._one is None:
            cls._one = cls(amvpt_mod, oracle)
        return cls._one

    def exchange(self, rank):
        from amvpt import dist as adist

        def fn(begins, counts):
            # a share of whole pixel rows is one contiguous run on the device: the same lanes, the same count
            assert min(begins) == min(self.runs[rank][0]) and sum(counts) == sum(self.runs[rank][1])
            return adist.exclusive_prefix(self.allb, self.allc, begins)
        return fn

    def render_share(self, rank, window, cap=OV_CAP, flags=0):
        torch = _torch()
        f = self.f
        rect = self.part[rank][0]
        x0, y0, w, h = window
        fx = f.zeros((h, w, f.C))
        ov = torch.zeros(2 + 2 * cap, dtype=torch.int64, device="cuda")
        _, cnt = f.render_fixed(into=fx, lanes=f.mod.LaneSet(0, 0, *rect), window=window, overflow_ptr=ov.data_ptr(),
                                overflow_capacity=cap, exchange=self.exchange(rank), flags=flags)
        return fx, ov, cnt


@pytest.fixture(scope="module")
def view_groups(gpu_ready, amvpt_mod, oracle):
    yield ViewGroups.get(amvpt_mod, oracle)
    ViewGroups._one = None


@pytest.mark.parametrize("border", ["filter_border", "none"])
def test_view_group_windows(gpu_ready, amvpt_mod, oracle, view_groups, border):
    """Four shares, each into its own fixed window and fixed overflow list, assembled with fixed_accumulate and
    resolved once.  With the window cut to the tiles alone every footprint at a tile edge spills: each share's list
    is then not empty (a 5 x 5 footprint on an interior tile edge guarantees it), and the frame is still equal."""
    from amvpt import dist as adist
    torch = _torch()
    vg, f = view_groups, view_groups.f
    want, st = f.want()
    quilt = f.zeros()
    H, W, C = quilt.shape
    adaptive_lanes = 0
    for direct in (False, True):
        quilt.zero_()
        adaptive_lanes = 0
        for rank, (rect, win) in enumerate(vg.part):
            window = tuple(win) if border == "filter_border" else tuple(rect)
            assert window[2] < W or window[3] < H
            fx, ov, cnt = vg.render_share(rank, window, flags=amvpt_mod.OPT_FIXED_DIRECT if direct else 0)
            ent = adist.fixed_overflow_entries(ov)
            assert cnt.film_overflow == ent.shape[0] == int(ov[0].item())
            if border == "none":
                assert cnt.film_overflow > 0
            assert cnt.film_range_drops == 0
            adaptive_lanes += cnt.adaptive_lanes
            amvpt_mod.fixed_accumulate(quilt.data_ptr(), W, H, C, fx.data_ptr(), window,
                                       ent.data_ptr() if ent.shape[0] else None, ent.shape[0])
            torch.cuda.synchronize()
        assert adaptive_lanes == st["adaptive_lanes"]
        _assert_equal(f.resolve(quilt), want, "direct puts" if direct else "window splat")


def test_view_group_overflow_capacity(gpu_ready, amvpt_mod, oracle, view_groups):
    """A 4-entry list under a tiles-only window: the count keeps counting, the render fails with AMVPT_ERR_OOM."""
    torch = _torch()
    vg, f = view_groups, view_groups.f
    rect = vg.part[1][0]
    fx = f.zeros((rect[3], rect[2], f.C))
    ov = torch.zeros(2 + 2 * 4, dtype=torch.int64, device="cuda")
    lanes = amvpt_mod.LaneSet(0, 0, *rect)
    fw = amvpt_mod.FixedWindow(ctypes.c_void_p(fx.data_ptr()), rect[0], rect[1], rect[2], rect[3],
                               ctypes.c_void_p(ov.data_ptr()), 4)
    cb = amvpt_mod.wrap_run_exchange(vg.exchange(1))
    o = amvpt_mod.RenderOpts(0, 0, 0, cb, None, None, 0, 0)
    L = amvpt_mod.hip_lib()
    rc = L.amvpt_render_fixed(f.dev.h, f.vd, ctypes.byref(f.p), ctypes.byref(lanes), ctypes.byref(fw), None,
                              ctypes.byref(o), None)
    torch.cuda.synchronize()
    assert rc == AMVPT_ERR_OOM
    assert "overflow list full" in L.amvpt_last_error().decode()
    assert int(ov[0].item()) > 4


# ---------------------------------------------------------------------------------------------------
# 5. the remaining kernel instances
# ---------------------------------------------------------------------------------------------------

def _rgba(xml):
    return edit_once(xml, 'name="pixel_format" value="rgb"', 'name="pixel_format" value="rgba"')


def _debug(xml):
    line = '<integer name="adaptive" value="$adaptive"/>'
    return edit_once(xml, line, line + '<boolean name="debug" value="true"/>')


SMALL = dict(res=16, spp=16, gx=4, gy=2, reuse=8)
INSTANCES = {
    # RGBAW film: the C = 5 instances, k_splat_adapt<5> with the fill
    "rgba": (CBOX, _rgba, dict(res=16, spp=16, gx=2, gy=2, reuse=4, adaptive=2)),
    "box": (CBOX, None, dict(SMALL, rfilter="box", adaptive=2)),
    # radius 6: 12 / 13-cell footprints, wider than the window's kMaxFoot = 5, so every put takes the miss path
    "gaussian_1.5": (CBOX, lambda xml: filter_xml(elem("gaussian", stddev=1.5)), dict(SMALL, res=12)),
    # glossy plates: the generic (not all-diffuse) instances
    "veach": (VEACH, None, dict(SMALL, adaptive=2)),
    # G = 1, the stock path integrator: k_splat_single
    "stock_path": (CBOX_PATH, None, dict(res=32, spp=16)),
    # the runtime-size group instance (test_gpu_adaptive_fill's wide_g32)
    "wide_g32": (CBOX, None, dict(res=12, spp=16, gx=8, gy=4, reuse=32, adaptive=3)),
    "debug": (CBOX, _debug, dict(SMALL, adaptive=3)),
}


@pytest.mark.parametrize("case", list(INSTANCES))
def test_instances(gpu_ready, amvpt_mod, oracle, case):
    scene, edit, kw = INSTANCES[case]
    f = Frame(amvpt_mod, oracle, scene, edit, **kw)
    assert f.C == (5 if case == "rgba" else 4)
    if case == "stock_path":
        assert f.plan["group"] == 1
    if case == "wide_g32":
        assert f.plan["group"] == 32
    if case == "debug":
        assert f.p.debug == 1
    if case == "gaussian_1.5":
        assert amvpt_mod.rfilter_eval(f.p, np.zeros(1, dtype=np.float32))[1] == 6.0
    want, st = f.want()
    fx, cnt = f.both_splats()
    assert cnt.film_range_drops == st["range_drops"] == 0
    assert cnt.adaptive_lanes == st["adaptive_lanes"]
    if kw.get("adaptive") and case != "debug":
        assert st["adaptive_lanes"] > 0   # the fill ran: k_splat_adapt
    _assert_equal(f.resolve(fx), want)


def test_tent(gpu_ready, amvpt_mod, oracle):
    """The FK_ANY instances (filter by kind at run time).  The oracle has no tent: `want` is the restatement of
    ImageBlock::put over the oracle's records with the tent's weights, summed as 32.32 integers (module docstring)."""
    f = Frame(amvpt_mod, oracle, CBOX, lambda xml: filter_xml(elem("tent")), **SMALL)
    assert f.p.rfilter == amvpt_mod.RFILTER_TENT and f.p.adaptive == 0
    q = gaussian_params(f.p)
    recs = [oracle.render(f.sd, f.vd, q, threads=16, record_pass=k)[1] for k in range(f.plan["passes"])]
    radius = amvpt_mod.rfilter_eval(f.p, np.zeros(1, dtype=np.float32))[1]
    want = put_film(recs, f.plan["group"], f.p, weight_fn_of(amvpt_mod, f.p), radius, f.plan["spp_per_pass"] >= 4,
                    fixed=True)
    fx, cnt = f.both_splats()
    assert cnt.film_range_drops == 0
    _assert_equal(f.resolve(fx), want)


# ---------------------------------------------------------------------------------------------------
# 6. range drops
# ---------------------------------------------------------------------------------------------------

def test_range_drops_through_the_window(gpu_ready, amvpt_mod, oracle):
    """test_deterministic_film_counts_range_drops' 1e12 light through the window splat: the range test is per cell
    add, before anything is summed (a test at the flush would see sums, drop other cells and count differently)."""
    f = Frame(amvpt_mod, oracle, CBOX_PATH,
              lambda x: edit_once(x, 'value="18.387, 13.9873, 6.75357"', 'value="1e12, 1e12, 1e12"'), res=32, spp=4)
    want, st = f.want()
    assert st["range_drops"] > 0
    fx, cnt = f.both_splats()
    assert cnt.film_range_drops == st["range_drops"]
    _assert_equal(f.resolve(fx), want)


# ---------------------------------------------------------------------------------------------------
# 7. accumulation across calls
# ---------------------------------------------------------------------------------------------------

def test_accumulation_across_calls(gpu_ready, amvpt_mod, oracle):
    """Seeds 0 and 1 into ONE integer film equal the int64 sum of two films rendered separately (a progressive
    frame: no rounding between the calls), and each of those resolves to the oracle's film of its seed."""
    f = Frame(amvpt_mod, oracle, CBOX, **SMALL)
    params = []
    for seed in (0, 1):
        _, _, p = f.scene.describe(0, seed, 0)
        params.append(p)
    assert params[0].seed != params[1].seed
    both = f.zeros()
    apart = []
    for p in params:
        f.render_fixed(into=both, p=p)
        fx, _ = f.render_fixed(p=p)
        want = oracle.render(f.sd, f.vd, p, threads=16, fixed_film=True)[0]
        _assert_equal(f.resolve(fx), want)
        apart.append(fx)
    assert (apart[0] != apart[1]).any().item()
    assert (both == apart[0] + apart[1]).all().item()


# ---------------------------------------------------------------------------------------------------
# 8. the flag's refusal stands
# ---------------------------------------------------------------------------------------------------

def test_flag_still_needs_whole_window(gpu_ready, amvpt_mod):
    """A copy of test_gpu_parity.py::test_deterministic_film_needs_whole_window's assertion: render_ex with the flag
    keeps refusing a film window; render_fixed is the entry point that takes one."""
    torch = _torch()
    s = amvpt_mod.load_file(CBOX, res=16, spp=16, gx=4, gy=2, reuse=8)
    sd, vd, p = s.describe(0, 0, 0)
    dev = amvpt_mod.DeviceScene(sd)
    film = torch.zeros((p.film_height, p.film_width // 2, 4), dtype=torch.float32, device="cuda")
    ov = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    with pytest.raises(Exception, match="AMVPT_OPT_DETERMINISTIC needs a whole-quilt film window"):
        dev.render_ex(vd, p, film.data_ptr(), window=(0, 0, p.film_width // 2, p.film_height),
                      overflow_ptr=ov.data_ptr(), overflow_capacity=1000, flags=amvpt_mod.OPT_DETERMINISTIC)
    with pytest.raises(Exception, match="needs an overflow list"):
        fx = torch.zeros((p.film_height, p.film_width // 2, 4), dtype=torch.int64, device="cuda")
        dev.render_fixed(vd, p, fx.data_ptr(), window=(0, 0, p.film_width // 2, p.film_height))

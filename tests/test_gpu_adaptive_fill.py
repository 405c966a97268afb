"""The adaptive fill (mvpath_multi.h:79-115) bit for bit, on masks and sizes the other modules do not reach.

The fill's puts are in no record (it runs with P.record = 0), so the other adaptive tests see them through the float
film only, at 1e-5 of its largest value: a sample one cell off at a footprint's rim, or one wrong weight, passes there.
Here every frame is rendered with AMVPT_OPT_DETERMINISTIC and compared with the oracle's fixed-point film
(oracle.render(fixed_film=True)): every float EQUAL.  test_deterministic_film holds the main pass to that bar with
adaptive = 0 and test_debug_mode_splats_the_adaptive_mask the mask, so what this module adds is the fill: the ordered
compaction (k_select_flagged), k_raygen_adapt's index arithmetic (adapt_index, run_delta), the suffix under
adapt_pass and k_splat_adapt.  The same frames' float-atomic films stay within 1e-5 (the fill's block-window put).

Each case asserts the regime it reached -- the flagged share of the lanes, the compaction's tiles and tail, the
number of fill chunks (launches of k_raygen: for G >= 2 only the fill's k_raygen_adapt counts there) -- so that a
scene that slips out of its regime fails.  Dense masks come from test_adaptive_fill.dense_xml (narrow, widely spaced
views); that module checks the masks on the oracle without a device.  Counts handed to a sharded render come from
the oracle's own count phase, never from the device.
"""
import os

import numpy as np
import pytest

from conftest import SCENES
from test_adaptive_fill import (CBOX, DENSE_ALL, DENSE_MANY_TILES, DENSE_MULTICHUNK, bit_equal, dense_xml, edit_once,
                                oracle_range_counts)

pytestmark = pytest.mark.gpu

MESH = os.path.join(SCENES, "cbox_mesh.xml")
VEACH = os.path.join(SCENES, "veach_grid.xml")
ENV = os.path.join(SCENES, "cbox_env.xml")
TILE = 4096   # kSelTile: lanes per block of k_select_flagged, 16 per thread

G8 = dict(gx=4, gy=2, reuse=8)
SPARSE, TENTH, MOST, ALL = (0.002, 0.05), (0.05, 0.25), (0.5, 0.95), (1.0, 1.0)   # flagged share of the lanes

# case -> (scene, defines, (passes, lanes per pass), flagged share, fill chunks (None: one per pass), n_adapt)
CASES = {
    # every lane flagged: each thread 16 bits, each tile 4096, the compaction's output is the identity
    "dense_all": ("dense", DENSE_ALL, (1, 32768), ALL, 1, 1),
    # 72 tiles: more than one 64-word step of the look-back is possible
    "dense_many_tiles": ("dense", DENSE_MANY_TILES, (1, 294912), ALL, 1, 1),
    # a fill wavefront of 2.59 passes: three fill chunks at the automatic chunk size
    "dense_multichunk": ("dense", DENSE_MULTICHUNK, (1, 36864), MOST, 3, 3),
    # 1.32 tiles and a last 16-lane group of 8 per pass, two passes with their own adapt_seed
    "odd_tail_whole": (CBOX, dict(res=15, spp=12, spp_pass_lim=6, gx=2, gy=2, reuse=4, adaptive=2), (2, 5400), SPARSE,
                       None, 2),
    # 72 tiles, most of them with no flagged lane
    "sparse_72_tiles": (CBOX, dict(res=48, spp=16, adaptive=3, **G8), (1, 294912), SPARSE, None, 3),
    "two_pass_g8": (CBOX, dict(res=24, spp=32, adaptive=3, **G8), (2, 73728), SPARSE, None, 3),
    # n_adapt = min(adaptive, G - 1) = 3, adapt_w = 1/4
    "clamp": (CBOX, dict(res=24, spp=16, gx=2, gy=2, reuse=4, adaptive=7), (1, 36864), SPARSE, None, 3),
    # a BVH in device memory: the fill's suffix as per-depth wavefronts with binned rays
    "mesh": (MESH, dict(res=16, spp=16, adaptive=2, **G8), (1, 32768), SPARSE, None, 2),
    # glossy plates: the generic kernel instances
    "veach": (VEACH, dict(res=16, spp=16, adaptive=2, **G8), (1, 32768), TENTH, None, 2),
    # the runtime-size group instance of k_mv_primary sets LF_ADAPT
    "wide_g32": (CBOX, dict(res=12, spp=16, gx=8, gy=4, reuse=32, adaptive=3), (1, 73728), SPARSE, None, 3),
    # the fill gathers the lane's aperture sample again (needs_ap)
    "thinlens": (CBOX, dict(cam="thinlens", aperture="0.05", res=24, spp=16, adaptive=1), (1, 36864), SPARSE, None, 1),
    # fill paths that leave the room (environment emitter)
    "env": (ENV, dict(res=24, spp=16, adaptive=2), (1, 36864), SPARSE, None, 2),
    "box_filter": (CBOX, dict(rfilter="box", res=24, spp=16, adaptive=2, **G8), (1, 73728), SPARSE, None, 2),
    # RGBAW film: k_splat_adapt<5>
    "rgba": ("rgba", dict(res=24, spp=16, gx=2, gy=2, reuse=4, adaptive=2), (1, 36864), SPARSE, None, 2),
}
WHOLE = pytest.mark.parametrize("case", list(CASES))


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


class Frame:
    """One case's loaded scene, device scene and the oracle's films of it (each rendered once, on first use)."""
    _frames = {}

    def __init__(self, amvpt_mod, oracle, case):
        scene, self.kw, (self.passes, self.lanes), self.share, self.chunks, self.n_adapt = CASES[case]
        if scene == "dense":
            self.scene = amvpt_mod.load_string(dense_xml(), **self.kw)
        elif scene == "rgba":
            self.scene = amvpt_mod.load_string(edit_once(open(CBOX).read(), 'name="pixel_format" value="rgb"',
                                                         'name="pixel_format" value="rgba"'), **self.kw)
        else:
            self.scene = amvpt_mod.load_file(scene, **self.kw)
        self.mod, self.oracle, self.case = amvpt_mod, oracle, case
        self.sd, self.vd, self.p = self.scene.describe(0, 0, 0)
        self.C = 5 if self.p.film_alpha else 4
        assert self.C == (5 if scene == "rgba" else 4)
        self.plan = oracle.plan(self.p)
        assert (self.plan["passes"], self.plan["lanes"]) == (self.passes, self.lanes)
        assert min(self.p.adaptive, self.plan["group"] - 1) == self.n_adapt
        self.dev = amvpt_mod.DeviceScene(self.sd)
        self._films = {}

    @classmethod
    def of(cls, amvpt_mod, oracle, case):
        if case not in cls._frames:
            cls._frames[case] = cls(amvpt_mod, oracle, case)
        return cls._frames[case]

    def oracle_film(self, fixed):
        """(film, stats) of the whole frame: the fixed-point film or the float film."""
        if fixed not in self._films:
            film, _, st = self.oracle.render(self.sd, self.vd, self.p, threads=16, fixed_film=fixed)
            print("%s: oracle %s film in %.2f s" % (self.case, "fixed-point" if fixed else "float", st["seconds"]))
            film.setflags(write=False)
            self._films[fixed] = (film, st)
        return self._films[fixed]

    def render(self, flags=0, chunk_lanes=None, lanes=None, exchange=None):
        torch = _torch()
        film = torch.zeros((self.p.film_height, self.p.film_width, self.C), dtype=torch.float32, device="cuda")
        cnt = self.mod.Counters()
        self.dev.render_ex(self.vd, self.p, film.data_ptr(), flags=flags, counters=cnt, chunk_lanes=chunk_lanes,
                           lanes=lanes, exchange=exchange)
        torch.cuda.synchronize()
        return film.cpu().numpy(), cnt

    def exact(self, flags=0, chunk_lanes=None):
        """The deterministic film of the whole frame, held to the oracle's fixed-point film and counts."""
        xfilm, st = self.oracle_film(True)
        gfilm, cnt = self.render(self.mod.OPT_DETERMINISTIC | flags, chunk_lanes)
        _assert_equal(gfilm, xfilm)
        assert cnt.film_range_drops == st["range_drops"] == 0
        assert cnt.adaptive_lanes == st["adaptive_lanes"]
        return cnt, st


def _assert_equal(got, want):
    """Tolerance 0 (NaN = NaN)."""
    assert np.abs(want).max() > 0
    bad = np.argwhere(~bit_equal(got, want))
    for y, x, c in bad[:8]:
        print("film[%d, %d, %d]: got %r, want %r" % (y, x, c, got[y, x, c], want[y, x, c]))
    assert len(bad) == 0, "deterministic film: %d of %d floats differ from the oracle's" % (len(bad), want.size)


def _assert_close(got, want):
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err < 1e-5, "float film: max relative difference %.3e" % err


def _assert_regime(f, cnt, st, fill_chunks=None):
    """What the case reached: the mask's density, the compaction's tiles and tail, the fill's chunks."""
    k = cnt.as_dict()["kernel_launches"]
    flagged, lanes = st["adaptive_lanes"] // f.n_adapt, f.passes * f.lanes
    tiles, rem, rem16 = -(-f.lanes // TILE), f.lanes % TILE, f.lanes % 16
    print("%s: %d of %d lanes flagged (%.4f), %d tiles per pass (last %d lanes, last group %d), chunk %d, "
          "k_raygen %d, k_select %d, k_bin %d" % (f.case, flagged, lanes, flagged / lanes, tiles, rem or TILE,
                                                   rem16 or 16, cnt.chunk_lanes, k["k_raygen"], k["k_select"], k["k_bin"]))
    assert st["adaptive_lanes"] == flagged * f.n_adapt
    lo, hi = f.share
    assert lo * lanes <= flagged <= hi * lanes
    assert k["k_select"] == cnt.passes == f.passes
    if f.passes == 1:
        want = -(-st["adaptive_lanes"] // cnt.chunk_lanes)
    else:   # every pass's whole fill in one chunk, and no pass without a flagged lane
        assert st["adaptive_lanes"] <= cnt.chunk_lanes
        want = f.passes
    assert k["k_raygen"] == want
    assert want == (fill_chunks or f.chunks or f.passes)
    return k


# (tiles per pass, lanes of the last tile, lanes of the last 16-lane group): the parts of k_select_flagged a case runs
TILES = {"dense_all": (8, 0, 0), "dense_many_tiles": (72, 0, 0), "dense_multichunk": (9, 0, 0),
         "odd_tail_whole": (2, 1304, 8), "sparse_72_tiles": (72, 0, 0), "two_pass_g8": (18, 0, 0)}


@pytest.fixture(scope="module", autouse=True)
def _device_started(gpu_ready, amvpt_mod):
    """The process's one-time costs are paid here when this module is the first to use the device, so that
    `--durations` shows each case's own time."""
    torch = _torch()
    s = amvpt_mod.load_file(MESH, res=4, spp=16)
    sd, vd, p = s.describe(0, 0, 0)
    film = torch.zeros((p.film_height, p.film_width, 4), dtype=torch.float32, device="cuda")
    amvpt_mod.DeviceScene(sd).render_ex(vd, p, film.data_ptr())
    torch.cuda.synchronize()
    yield
    Frame._frames.clear()


@WHOLE
def test_fill_exact(gpu_ready, amvpt_mod, oracle, case):
    """The deterministic film equal to the oracle's fixed-point film, and the regime the case names."""
    f = Frame.of(amvpt_mod, oracle, case)
    cnt, st = f.exact()
    k = _assert_regime(f, cnt, st)
    if case in TILES:
        assert (-(-f.lanes // TILE), f.lanes % TILE, f.lanes % 16) == TILES[case]
    if case == "dense_multichunk":
        assert cnt.chunk_lanes == f.lanes and st["adaptive_lanes"] > 2 * f.lanes
    assert (k["k_bin"] > 0) == (case == "mesh")
    if case == "mesh":
        assert k["k_extend"] > 0 and k["k_suffix"] == 0


@WHOLE
def test_fill_float_film(gpu_ready, amvpt_mod, oracle, case):
    """The same frame with float atomics (the fill's puts through the block window): 1e-5 of the film's scale."""
    f = Frame.of(amvpt_mod, oracle, case)
    ofilm, st = f.oracle_film(False)
    gfilm, cnt = f.render()
    assert cnt.adaptive_lanes == st["adaptive_lanes"] > 0
    _assert_close(gfilm, ofilm)


def test_dense_straddle(gpu_ready, amvpt_mod, oracle):
    """dense_multichunk in chunks of 5000 lanes (5000 % 3 = 2): most fill chunks begin between two repeats of a lane
    (j / n_adapt across chunk_begin), and eight main-pass chunks write one mask.  The same film, bit for bit."""
    f = Frame.of(amvpt_mod, oracle, "dense_multichunk")
    cnt, st = f.exact(chunk_lanes=5000)
    assert cnt.chunk_lanes == 5000 and st["adaptive_lanes"] > 15 * 5000
    _assert_regime(f, cnt, st, fill_chunks=-(-st["adaptive_lanes"] // 5000))
    _assert_close(f.render(chunk_lanes=5000)[0], f.oracle_film(False)[0])


@pytest.mark.parametrize("flag", ["OPT_WAVEFRONT_SUFFIX", "OPT_SPLIT_NEE"])
def test_dense_fused_vs_wavefront(gpu_ready, amvpt_mod, oracle, flag):
    """dense_multichunk with the suffix as per-depth wavefronts, and with NEE in its own kernel: the other two
    forms of the suffix under adapt_pass.  Deterministic films equal to the default's and the oracle's."""
    f = Frame.of(amvpt_mod, oracle, "dense_multichunk")
    default, cnt0 = f.render(amvpt_mod.OPT_DETERMINISTIC)
    k0 = cnt0.as_dict()["kernel_launches"]
    assert k0["k_suffix"] > 0 and k0["k_extend"] == 0 and k0["k_shadow"] == 0
    cnt, st = f.exact(flags=getattr(amvpt_mod, flag))
    k = _assert_regime(f, cnt, st)
    assert k["k_suffix"] == 0 and k["k_extend"] > 0 and (k["k_shadow"] > 0) == (flag == "OPT_SPLIT_NEE")
    film, _ = f.render(amvpt_mod.OPT_DETERMINISTIC | getattr(amvpt_mod, flag))
    assert bit_equal(film, default).all()


@pytest.mark.parametrize("variant", ["four_streams", "one_stream"])
def test_mesh_chunk_streams(gpu_ready, amvpt_mod, oracle, variant):
    """The mesh frame in 16 chunks of 2048 lanes, on four chunk streams that are joined before the fill reads the
    mask, and with every chunk on the render stream (AMVPT_OPT_ONE_STREAM)."""
    f = Frame.of(amvpt_mod, oracle, "mesh")
    cnt, st = f.exact(flags=amvpt_mod.OPT_ONE_STREAM if variant == "one_stream" else 0, chunk_lanes=2048)
    assert cnt.chunk_lanes == 2048 and cnt.buffer_sets == (1 if variant == "one_stream" else 4)
    k = _assert_regime(f, cnt, st)
    assert k["k_bin"] > 0 and k["k_extend"] > 0 and k["k_suffix"] == 0


def test_mesh_render_after_failed_fill(gpu_ready, amvpt_mod, oracle):
    """Two renders of the mesh frame's first half that fail in the fill -- after eight main-pass chunks on four chunk
    streams -- once because the count exchange fails and once because it returns a prefix past the pass's total.
    Both leave through the arena's release (side streams joined, `done` recorded), so the next render of the whole
    frame on the same buffer sets is the oracle's, bit for bit."""
    f = Frame.of(amvpt_mod, oracle, "mesh")
    half = amvpt_mod.LaneSet(0, f.lanes // 2, 0, 0, 0, 0)
    assert f.lanes // 2 == 8 * 2048

    def failing(begins, counts):
        raise RuntimeError("no exchange today")

    def past_total(begins, counts):
        return [1], sum(counts)   # prefix + count > total

    for exchange, message in ((failing, "adaptive count exchange failed"), (past_total, "inconsistent prefixes")):
        with pytest.raises(RuntimeError, match=message):
            f.render(amvpt_mod.OPT_DETERMINISTIC, chunk_lanes=2048, lanes=half, exchange=exchange)
    cnt, _ = f.exact(chunk_lanes=2048)
    assert cnt.chunk_lanes == 2048 and cnt.buffer_sets == 4


def test_dense_tail_ranges(gpu_ready, amvpt_mod, oracle):
    """dense_all as two lane ranges cut at 3 x 4096 + 7, each with the count exchange and into its own film,
    against the oracle's render of that range with the same exchange: spans of 12295 and 20473 lanes end in tiles
    of 7 and 4089 lanes and in 16-lane groups of 7 and 9 (the per-byte branch); the second has a prefix."""
    f = Frame.of(amvpt_mod, oracle, "dense_all")
    cut = 3 * TILE + 7
    ranges = [(0, cut), (cut, f.lanes)]
    assert [((e - b) % TILE, (e - b) % 16) for b, e in ranges] == [(7, 7), (4089, 9)]
    counts = [c for (c,) in oracle_range_counts(oracle, f.sd, f.vd, f.p, ranges)]
    assert counts == [e - b for b, e in ranges]   # every lane flagged
    for r, (b, e) in enumerate(ranges):
        prefix, total = sum(counts[:r]), sum(counts)
        def oracle_exchange(local):
            assert local == counts[r]
            return prefix, total
        oracle.set_exchange(oracle_exchange)
        try:
            xfilm, _, st = oracle.render(f.sd, f.vd, f.p, lane_begin=b, lane_end=e, threads=16, fixed_film=True)
        finally:
            oracle.set_exchange(None)
        seen = []

        def exchange(begins, run_counts):
            seen.append((begins, run_counts))
            return [prefix], total
        gfilm, cnt = f.render(amvpt_mod.OPT_DETERMINISTIC, lanes=amvpt_mod.LaneSet(b, e, 0, 0, 0, 0), exchange=exchange)
        assert seen == [([b], [counts[r]])]
        _assert_equal(gfilm, xfilm)
        assert cnt.film_range_drops == st["range_drops"] == 0
        assert cnt.adaptive_lanes == st["adaptive_lanes"] == e - b
        k = cnt.as_dict()["kernel_launches"]
        assert k["k_select"] == 1 and k["k_raygen"] == 1


def test_rect_lanes(gpu_ready, amvpt_mod, oracle):
    """C5's small shape (32 views, groups of 4, adaptive 3): the tiles of one view group as a rectangle lane set
    (P.rect, k_run_counts, one run_delta per pixel row) into a whole-quilt deterministic film, against
    oracle.render_rect of the same rectangle.  Both are given the run prefixes of the oracle's count phase over
    all eight groups; the device's own run counts must agree with them."""
    from amvpt import dist as adist
    s = amvpt_mod.load_file(CBOX, res=16, spp=16, gx=8, gy=4, reuse=4, adaptive=3)
    sd, vd, p = s.describe(0, 0, 0)
    plan = oracle.plan(p)
    assert plan["group"] == 4 and plan["passes"] == 1
    part = adist.view_group_partition(p, 4, 8)
    assert part is not None and len(part) == 8
    runs = {}
    try:
        for r, (rect, _) in enumerate(part):   # count phase, on the oracle
            def counting(begins, counts, r=r):
                runs[r] = (list(begins), list(counts))
                return adist.exclusive_prefix(begins, counts, begins)
            oracle.set_run_exchange(counting)
            oracle.render_rect(sd, vd, p, rect, threads=16)
        allb, allc = sum((runs[r][0] for r in range(8)), []), sum((runs[r][1] for r in range(8)), [])
        rank = 5
        rect = part[rank][0]
        assert rect[2] < p.film_width and rect[3] > 1   # a true rectangle: several runs, none a whole row
        below = sum(c for b, c in zip(allb, allc) if b < min(runs[rank][0]))
        print("rank %d: rect %s, %d runs, %d flagged of %d in the pass, %d below the first run" % (
            rank, rect, len(runs[rank][0]), sum(runs[rank][1]), sum(allc), below))
        assert below > 0 and sum(runs[rank][1]) > 0 and sum(1 for c in runs[rank][1] if c) > 1

        def exchange(begins, counts):
            assert (list(begins), list(counts)) == runs[rank]
            return adist.exclusive_prefix(allb, allc, begins)
        oracle.set_run_exchange(exchange)
        xfilm, st = oracle.render_rect(sd, vd, p, rect, threads=16, fixed_film=True)
        ofilm, _ = oracle.render_rect(sd, vd, p, rect, threads=16)
    finally:
        oracle.set_run_exchange(None)
    assert st["adaptive_lanes"] == 3 * sum(runs[rank][1])
    torch = _torch()
    dev = amvpt_mod.DeviceScene(sd)
    for flags in (amvpt_mod.OPT_DETERMINISTIC, 0):
        film = torch.zeros((p.film_height, p.film_width, 4), dtype=torch.float32, device="cuda")
        cnt = amvpt_mod.Counters()
        dev.render_ex(vd, p, film.data_ptr(), lanes=amvpt_mod.LaneSet(0, 0, *rect), flags=flags, counters=cnt,
                      exchange=exchange)
        torch.cuda.synchronize()
        assert cnt.lanes == rect[2] * rect[3] * plan["spp_per_pass"]
        assert cnt.adaptive_lanes == st["adaptive_lanes"]
        assert cnt.film_range_drops == st["range_drops"] == 0
        if flags:
            _assert_equal(film.cpu().numpy(), xfilm)
        else:
            _assert_close(film.cpu().numpy(), ofilm)

"""The fixed-point film as an object (include/amvpt_fixed.h), without a device: the version and symbols, the host
entry points against numpy restatements, and the integer collectives of amvpt.dist under gloo.

Every comparison here is integer equality or float bit-equality: 32.32 sums are integers, so there is no tolerance
to choose.  fixed_case3() is also the data the stand-alone sanitizer program (tools/fixed_host_check.cpp) takes as a
file."""
import ctypes
import os
import socket
import tempfile

import numpy as np
import pytest

from conftest import PKG, REPO

SYMBOLS = ("amvpt_fixed_version", "amvpt_render_fixed", "amvpt_fixed_accumulate", "amvpt_fixed_resolve",
           "amvpt_fixed_accumulate_host", "amvpt_fixed_resolve_host")
AMVPT_ERR_INVALID, AMVPT_ERR_NO_DEVICE = 1, 5


def test_versions_and_symbols(amvpt_mod):
    L = amvpt_mod.hip_lib()
    assert L.amvpt_abi_version() == 12
    assert amvpt_mod.fixed_version() == 1
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert amvpt_mod.OPT_FIXED_DIRECT == 1024
    assert ctypes.sizeof(amvpt_mod.FixedWindow) == ctypes.sizeof(amvpt_mod.FilmWindow) == 40


def resolve_restated(i):
    return (i.astype(np.float64) * 2.0 ** -32).astype(np.float32)


def test_fixed_resolve_host(amvpt_mod):
    """(float) ((double) i * 2^-32), stored or added.  Above 2^53 the int64 -> double step rounds (to nearest even,
    numpy's astype and the C cast alike)."""
    rng = np.random.default_rng(7)
    edge = [0, 1, -1, (2 ** 31 - 1) * 2 ** 32, -(2 ** 31 - 1) * 2 ** 32, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53 + 3,
            2 ** 62 + 2 ** 9 + 1, -(2 ** 62 + 2 ** 9 + 1), 2 ** 63 - 1, -2 ** 63, 2 ** 32, -2 ** 32, 2 ** 31, 3 << 8]
    i = np.concatenate([np.array(edge, dtype=np.int64),
                        rng.integers(-2 ** 63, 2 ** 63 - 1, size=4000, dtype=np.int64),
                        rng.integers(-2 ** 40, 2 ** 40, size=4000, dtype=np.int64),
                        rng.integers(2 ** 53, 2 ** 63 - 1, size=1000, dtype=np.int64)])
    assert (np.abs(i.astype(np.float64)) > 2.0 ** 53).sum() > 1000
    want = resolve_restated(i)
    got = amvpt_mod.fixed_resolve_host(i)
    assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all()
    # store mode overwrites whatever the film held
    film = np.full(i.shape, np.float32(np.nan))
    amvpt_mod.fixed_resolve_host(i, film)
    assert (film.view(np.uint32) == want.view(np.uint32)).all()
    # add mode: one float add per element
    base = rng.standard_normal(i.size).astype(np.float32) * np.float32(1000)
    film = base.copy()
    amvpt_mod.fixed_resolve_host(i, film, add=True)
    assert (film.view(np.uint32) == (base + want).astype(np.float32).view(np.uint32)).all()
    shaped = amvpt_mod.fixed_resolve_host(i[:24].reshape(2, 3, 4))
    assert shaped.shape == (2, 3, 4)


def fixed_case3():
    """A 24 x 16 x 4 quilt, two windows overlapping by a 4-pixel border, an overflow list with repeated indices and
    negative values.  (quilt before, [(window film, rect, entries)])."""
    rng = np.random.default_rng(3)
    W, H, C = 24, 16, 4
    quilt = rng.integers(-2 ** 40, 2 ** 40, size=(H, W, C), dtype=np.int64)
    rects = [(0, 0, 16, 16), (8, 0, 16, 16)]   # columns 8..15 belong to both
    parts = []
    for x0, y0, w, h in rects:
        win = rng.integers(-2 ** 45, 2 ** 45, size=(h, w, C), dtype=np.int64)
        idx = rng.integers(0, W * H * C, size=300, dtype=np.int64)
        idx[100:200] = idx[:100]          # repeats
        idx[200:220] = idx[0]             # one element hit 22 times
        val = rng.integers(-2 ** 50, 2 ** 50, size=300, dtype=np.int64)
        val[::3] = -np.abs(val[::3])
        parts.append((win, (x0, y0, w, h), np.stack([idx, val], axis=1)))
    return quilt, parts


def accumulate_restated(quilt, parts):
    out = quilt.copy()
    for win, (x0, y0, w, h), ent in parts:
        out[y0:y0 + h, x0:x0 + w] += win
        np.add.at(out.reshape(-1), ent[:, 0], ent[:, 1])
    return out


def test_fixed_accumulate_host(amvpt_mod):
    quilt, parts = fixed_case3()
    want = accumulate_restated(quilt, parts)
    got = quilt.copy()
    for win, rect, ent in parts:
        amvpt_mod.fixed_accumulate_host(got, win, rect, ent)
    assert (got == want).all()
    assert (got[:, 8:16] != quilt[:, 8:16] + parts[0][0][:, 8:16]).any()   # the border took both windows
    # wrap-around is two's complement, not an error
    q = np.full((1, 1, 4), 2 ** 63 - 1, dtype=np.int64)
    amvpt_mod.fixed_accumulate_host(q, np.ones((1, 1, 4), dtype=np.int64), (0, 0, 1, 1))
    assert (q == -2 ** 63).all()
    # entries alone; an index past the quilt is ignored
    q = np.zeros((2, 2, 4), dtype=np.int64)
    amvpt_mod.fixed_accumulate_host(q, None, (0, 0, 0, 0), np.array([[3, -5], [3, 2], [16, 9]], dtype=np.int64))
    assert q.reshape(-1)[3] == -3 and q.sum() == -3


def test_fixed_accumulate_host_refuses_bad_arguments(amvpt_mod):
    L = amvpt_mod.hip_lib()
    q = np.zeros((16, 24, 4), dtype=np.int64)
    w = np.zeros((4, 4, 4), dtype=np.int64)
    e = np.zeros((2, 2), dtype=np.int64)

    def refused(rc, *words):
        assert rc == AMVPT_ERR_INVALID
        msg = L.amvpt_last_error().decode()
        for word in words:
            assert word in msg, msg

    acc = L.amvpt_fixed_accumulate_host
    refused(acc(None, 24, 16, 4, w.ctypes.data, 0, 0, 4, 4, None, 0), "quilt", "null")
    refused(acc(q.ctypes.data, 24, 16, 4, None, 0, 0, 4, 4, None, 0), "window", "null")
    refused(acc(q.ctypes.data, 24, 16, 4, w.ctypes.data, 0, 0, 4, 4, None, 2), "overflow_entries", "null")
    refused(acc(q.ctypes.data, 24, 16, 4, w.ctypes.data, 21, 0, 4, 4, e.ctypes.data, 2), "window outside the quilt")
    refused(acc(q.ctypes.data, 24, 16, 4, w.ctypes.data, 0, 13, 4, 4, e.ctypes.data, 2), "window outside the quilt")
    refused(acc(q.ctypes.data, 24, 16, 4, w.ctypes.data, 2 ** 32 - 2, 0, 4, 4, None, 0), "window outside the quilt")
    for channels in (0, 3, 6):
        refused(acc(q.ctypes.data, 24, 16, channels, w.ctypes.data, 0, 0, 4, 4, None, 0), "channels")
    assert (q == 0).all()
    refused(L.amvpt_fixed_resolve_host(None, w.ctypes.data, 4, 0), "fixed", "null")
    refused(L.amvpt_fixed_resolve_host(w.ctypes.data, None, 4, 0), "film", "null")


def test_render_fixed_without_a_device(amvpt_mod):
    """As amvpt_render: no device, no render (and no CPU fall-back)."""
    if amvpt_mod.device_count() > 0:
        return
    L = amvpt_mod.hip_lib()
    lanes = amvpt_mod.LaneSet(0, 2 ** 64 - 1, 0, 0, 0, 0)
    fw = amvpt_mod.FixedWindow(None, 0, 0, 8, 8, None, 0)
    p = amvpt_mod.Params()
    assert L.amvpt_render(None, None, ctypes.byref(p), 0, 1, None, None, None) == AMVPT_ERR_NO_DEVICE
    assert L.amvpt_render_fixed(None, None, ctypes.byref(p), ctypes.byref(lanes), ctypes.byref(fw), None, None,
                                None) == AMVPT_ERR_NO_DEVICE
    assert "no HIP device" in L.amvpt_last_error().decode()
    assert L.amvpt_fixed_resolve(None, None, 0, 0, None) == AMVPT_ERR_NO_DEVICE
    assert L.amvpt_fixed_accumulate(None, 1, 1, 4, None, 0, 0, 0, 0, None, 0, None) == AMVPT_ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------
# amvpt.dist under gloo
# ---------------------------------------------------------------------------------------------------

QW, QH, QC = 24, 16, 4
BIG = 2 ** 56   # 2^56 + 1 is no float64 (and no float32): a float sum of (2^56 + 1) + (-2^56) gives 0, not 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def rank_film(rank):
    """Rank `rank`'s whole-quilt integer film; element 0 carries the pair whose float sum would round."""
    f = np.random.default_rng(100 + rank).integers(-2 ** 44, 2 ** 44, size=(QH, QW, QC), dtype=np.int64)
    f.reshape(-1)[0] = (BIG + 1, -BIG, 5)[rank]
    return f


def rank_windows(world):
    """Column bands with a 2-pixel border on each inner side."""
    cuts = [QW * r // world for r in range(world + 1)]
    return [(max(0, cuts[r] - 2), 0, min(QW, cuts[r + 1] + 2) - max(0, cuts[r] - 2), QH) for r in range(world)]


def rank_window(rank, world):
    """(window film, rect, overflow list as the render leaves it) of `rank`."""
    rng = np.random.default_rng(200 + rank)
    x0, y0, w, h = rank_windows(world)[rank]
    win = rng.integers(-2 ** 44, 2 ** 44, size=(h, w, QC), dtype=np.int64)
    n = 0 if (world == 3 and rank == 1) else (7, 12, 12)[rank]   # world 3: one rank with an empty list
    idx = rng.integers(0, QW * QH * QC, size=n, dtype=np.int64)
    val = rng.integers(-2 ** 50, 2 ** 50, size=n, dtype=np.int64)
    if rank == 0:
        x0_, _, _, _ = rank_windows(world)[0]
        win[0, 0, 0] = BIG + 1      # quilt element 0 (rank 0's window starts at the origin)
        assert x0_ == 0
    if rank == world - 1:
        idx[:3], val[:3] = 0, (-BIG, 7, -7)   # the partner of rank 0's 2^56 + 1, through the overflow list
        idx[3] = idx[4]
    cap = 16
    ov = np.zeros(2 + 2 * cap, dtype=np.int64)
    ov[0] = n
    ov[2:2 + 2 * n] = np.stack([idx, val], axis=1).reshape(-1)
    return win, (x0, y0, w, h), ov


def _dist_worker(rank, world, port, out_dir):
    import sys
    for p in (REPO, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    from amvpt import dist as adist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        t = torch.from_numpy(rank_film(rank))
        adist.reduce_fixed(t, dst=0)
        win, rect, ov = rank_window(rank, world)
        quilt = torch.full((QH, QW, QC), 77, dtype=torch.int64)   # gather zeroes it on dst
        got = adist.gather_fixed_windows(torch.from_numpy(win), rect, torch.from_numpy(ov), quilt,
                                         rank_windows(world), dst=0)
        assert (got is None) == (rank != 0)
        if rank == 0:
            np.save(os.path.join(out_dir, "reduced.npy"), t.numpy())
            np.save(os.path.join(out_dir, "gathered.npy"), quilt.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_dist_fixed_collectives(amvpt_mod, world):
    """reduce_fixed and gather_fixed_windows on rank 0 equal the numpy integer sums exactly, including the element
    that holds 2^56 + 1 and -2^56: its float64 sum would be 0 (or 5 with the third rank), the integers give 1 (6)."""
    import torch.multiprocessing as mp
    assert float(BIG + 1) + float(-BIG) == 0.0
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dist_worker, args=(world, _free_port(), d), nprocs=world, join=True)
        reduced, gathered = np.load(os.path.join(d, "reduced.npy")), np.load(os.path.join(d, "gathered.npy"))
    want = sum(rank_film(r) for r in range(world))
    assert reduced.dtype == np.int64 and (reduced == want).all()
    assert reduced.reshape(-1)[0] == (1 if world == 2 else 6)
    parts = []
    for r in range(world):
        win, rect, ov = rank_window(r, world)
        parts.append((win, rect, ov[2:2 + 2 * ov[0]].reshape(-1, 2)))
    wantq = accumulate_restated(np.zeros((QH, QW, QC), dtype=np.int64), parts)
    assert (gathered == wantq).all()
    # 2^56 + 1 from rank 0's window, -2^56 + 7 - 7 from the last rank's list; no other window reaches the origin
    assert gathered.reshape(-1)[0] == 1


def test_fixed_overflow_entries(amvpt_mod):
    import torch
    from amvpt import dist as adist
    ov = torch.zeros(2 + 2 * 4, dtype=torch.int64)
    assert adist.fixed_overflow_entries(ov).shape == (0, 2)
    ov[0] = 2
    ov[2:6] = torch.tensor([9, -4, 9, 2 ** 40])
    assert adist.fixed_overflow_entries(ov).tolist() == [[9, -4], [9, 2 ** 40]]
    ov[0] = 5
    with pytest.raises(RuntimeError, match="full"):
        adist.fixed_overflow_entries(ov)
    with pytest.raises(ValueError, match="int64"):
        adist.reduce_fixed(torch.zeros(4, dtype=torch.float32))

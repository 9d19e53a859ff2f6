"""CPU: distributed.halo_strip_plan — who encodes which strips of a product file in a patch-row-sharded run, and which rows
change hands for that.  Every expected value is computed here from halo_zone_rows, patch_grid_1d and _rows_per_strip.
"""
import socket

import numpy as np
import pytest

from moonsuperresolution_amd.distributed import (halo_strip_plan, halo_zone_rows, patch_grid_1d, strip_plan, tile_origins,
                                                 tile_rows)
from moonsuperresolution_amd.geotiff import _rows_per_strip

GEOMETRIES = [(64, 16, 128), (128, 32, 256), (512, 64, 1024)]
SHAPES = [(1, 1), (47, 300), (128, 128), (300, 64), (300, 256), (300, 300), (513, 40), (1000, 16384), (1024, 1024),
          (1100, 900), (2049, 8200), (5000, 33)]


def zones(shape, S, s, T, world):
    return halo_zone_rows(patch_grid_1d(tile_rows(tile_origins(shape, T)), S, s, T), S, world)


def owned_rows(shape, S, s, T, world):
    """Raster rows each rank finalises: canvas rows [own_lo, own_hi) less the S - s margin, clipped to the raster."""
    H = shape[0]

    def clip(c):
        return H if c is None else max(0, min(H, c - (S - s)))
    return [(clip(z["own_lo"]), clip(z["own_hi"])) for z in zones(shape, S, s, T, world)]


def span(a):
    return set(range(a[0], a[1]))


@pytest.mark.parametrize("S,s,T", GEOMETRIES)
def test_invariants(S, s, T):
    seen = refused = not_local = handed = 0
    for shape in SHAPES:
        H, W = shape
        for world in range(1, 9):
            try:
                want_rows = owned_rows(shape, S, s, T, world)
            except ValueError:
                refused += 1
                for itemsize in (2, 4):
                    with pytest.raises(ValueError):
                        halo_strip_plan(shape, itemsize, S, s, T, world)
                continue
            for itemsize in (2, 4):
                p = halo_strip_plan(shape, itemsize, S, s, T, world)
                what = (shape, world, itemsize)
                rps = _rows_per_strip(H, W * itemsize)
                assert p["rps"] == rps and p["n_strips"] == -(-H // rps), what
                rows, strips, take, give = p["rows"], p["strips"], p["take"], p["give"]
                assert len(rows) == len(strips) == len(take) == len(give) == world, what
                assert rows == want_rows, what
                assert rows[0][0] == 0 and rows[-1][1] == H, what
                assert strips[0][0] == 0 and strips[-1][1] == p["n_strips"], what
                for r in range(world):
                    assert rows[r][0] <= rows[r][1] and strips[r][0] <= strips[r][1], what
                    if r:
                        assert rows[r][0] == rows[r - 1][1] and strips[r][0] == strips[r - 1][1], what
                    # strip k belongs to the rank that owns its first row
                    assert set(range(*strips[r])) == {k for k in range(p["n_strips"]) if rows[r][0] <= k * rps < rows[r][1]}, what
                    assert give[r] == (take[r - 1] if r else (0, 0)), what
                    assert span(take[r]) == (span((rows[r][1], min(strips[r][1] * rps, H))) if strips[r][1] > strips[r][0]
                                             else set()), what
                    s0, s1 = strips[r]
                    if p["local"]:
                        assert (span(rows[r]) - span(give[r])) | span(take[r]) == span((s0 * rps, min(s1 * rps, H))), what
                        assert span(give[r]) <= span(rows[r]), what
                inside = all(span(take[r]) <= span(rows[r + 1]) for r in range(world - 1)) and not span(take[-1])
                assert p["local"] is inside, what
                seen += 1
                not_local += not p["local"]
                handed += any(span(t) for t in take)
    assert seen > 50 and handed > 0        # the sweep met plans with a hand-over
    if (S, s, T) == (64, 16, 128):
        assert not_local > 0 and refused > 0   # ... three-rank strips, and worlds that halo_zone_rows refuses


@pytest.mark.parametrize("itemsize", [4, 2])
def test_big_geometry(itemsize):
    shape, S, s, T, world = (15000, 70000), 512, 64, 1024, 8
    p = halo_strip_plan(shape, itemsize, S, s, T, world)
    assert p["rps"] == 1 and p["n_strips"] == 15000
    assert all(t0 == t1 for t0, t1 in p["take"]) and all(g0 == g1 for g0, g1 in p["give"])
    assert p["local"] is True
    assert p["rows"] == owned_rows(shape, S, s, T, world)
    assert p["strips"] == p["rows"]                   # one row a strip
    assert all(r1 > r0 for r0, r1 in p["rows"])


def test_small_geometry_two_ranks():
    shape, S, s, T, world = (300, 256), 64, 16, 128, 2
    ys = patch_grid_1d(tile_rows(tile_origins(shape, T)), S, s, T)
    boundary = ys[len(ys) - len(ys) // 2] + S // 2 - (S - s)     # rank 1's first patch row, its centre, in raster rows
    assert boundary == halo_zone_rows(ys, S, world)[1]["own_lo"] - (S - s) == 208
    f32, u16 = (halo_strip_plan(shape, n, S, s, T, world) for n in (4, 2))
    assert (f32["rps"], u16["rps"]) == (_rows_per_strip(300, 1024), _rows_per_strip(300, 512)) == (64, 128)
    for p in (f32, u16):
        assert p["rows"] == [(0, boundary), (boundary, 300)]
        assert p["take"] == [(boundary, 256), (300, 300)]
        assert p["give"] == [(0, 0), (boundary, 256)]
        assert p["local"] is True
    assert f32["strips"] == [(0, 4), (4, 5)] and u16["strips"] == [(0, 2), (2, 3)]


def test_narrow_geometry_three_ranks():
    shape, S, s, T, world = (300, 64), 64, 16, 128, 3
    rows = owned_rows(shape, S, s, T, world)
    assert all(r1 > r0 for r0, r1 in rows)
    u16 = halo_strip_plan(shape, 2, S, s, T, world)
    assert u16["rps"] == 300 and u16["n_strips"] == 1 and u16["strips"] == [(0, 1), (1, 1), (1, 1)]
    assert u16["take"][0] == (rows[0][1], 300) and u16["local"] is False
    f32 = halo_strip_plan(shape, 4, S, s, T, world)
    assert f32["rps"] == 256 and f32["rows"] == rows and f32["local"] is True
    assert f32["strips"] == [(0, 1), (1, 2), (2, 2)]
    assert f32["take"] == [(rows[0][1], 256), (rows[1][1], 300), (300, 300)]


def test_one_rank_owns_everything():
    p = halo_strip_plan((300, 300), 4, 64, 16, 128, 1)
    assert p["rows"] == [(0, 300)] and p["strips"] == [(0, p["n_strips"])] and p["local"] is True
    assert p["take"] == [(300, 300)] and p["give"] == [(0, 0)]


@pytest.mark.parametrize("args", [((0, 10), 4, 64, 16, 128, 2), ((10, 0), 4, 64, 16, 128, 2), ((10, 10), 0, 64, 16, 128, 2),
                                  ((10, 10), 4, 64, 16, 0, 2), ((10, 10), 4, 64, 16, 128, 0)])
def test_argument_errors(args):
    with pytest.raises(ValueError) as halo_error:
        halo_strip_plan(*args)
    shape, itemsize, _, _, T, world = args
    with pytest.raises(ValueError) as tile_error:
        strip_plan(shape, itemsize, T, world)
    assert str(halo_error.value) == str(tile_error.value)


def test_more_ranks_than_patch_rows_is_refused():
    with pytest.raises(ValueError, match="more ranks than patch rows"):
        halo_strip_plan((100, 100), 4, 64, 16, 128, 64)


def test_strip_plan_is_unchanged():
    p = strip_plan((300, 256), 4, 128, 2)
    assert p == {"rps": 64, "n_strips": 5, "rows": [(0, 256), (256, 300)], "straddles": False, "strips": [(0, 4), (4, 5)]}


# ---- the hand-over itself, over gloo on host tensors ----
def _full(shape, k):
    """A raster whose every pixel names itself (and its product)."""
    return (np.arange(shape[0] * shape[1], dtype=np.int64).reshape(shape) + 7 * k).astype((np.float32, np.uint8)[k % 2])


def _handover_worker(rank, world, port, q, shape, itemsizes):
    import os
    import torch
    import torch.distributed as dist
    from moonsuperresolution_amd.distributed import exchange_strip_rows
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    plans = [halo_strip_plan(shape, n, 64, 16, 128, world) for n in itemsizes]
    # cropped views, like the driver's: two more columns a side
    slabs = [torch.from_numpy(np.pad(_full(shape, k), ((0, 0), (2, 2))))[p["rows"][rank][0]:p["rows"][rank][1], 2:-2]
             for k, p in enumerate(plans)]
    got = exchange_strip_rows(slabs, plans, rank, world)
    q.put((rank, [g.numpy().copy() for g in got]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("shape,world,itemsizes", [((300, 256), 2, (4, 2)), ((300, 64), 3, (4, 4)), ((300, 300), 3, (4, 2))])
def test_handover_over_gloo(shape, world, itemsizes):
    """exchange_strip_rows on ``world`` gloo ranks, two products in one batch: every rank ends with exactly the rows of its
    strips, [s0 rps, min(s1 rps, H)), whichever rank finalised them."""
    import torch.multiprocessing as mp
    plans = [halo_strip_plan(shape, n, 64, 16, 128, world) for n in itemsizes]
    assert all(p["local"] for p in plans) and any(t1 > t0 for p in plans for t0, t1 in p["take"])
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_handover_worker, args=(r, world, port, q, shape, itemsizes)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        for k, p in enumerate(plans):
            (s0, s1), rps = p["strips"][r], p["rps"]
            want = _full(shape, k)[s0 * rps:max(s0 * rps, min(s1 * rps, shape[0]))]
            assert results[r][k].dtype == want.dtype and np.array_equal(results[r][k], want), (r, k)


def test_handover_refuses_a_plan_that_is_not_local():
    import torch
    from moonsuperresolution_amd.distributed import exchange_strip_rows
    plan = halo_strip_plan((300, 64), 2, 64, 16, 128, 3)
    with pytest.raises(ValueError, match="three ranks"):
        exchange_strip_rows([torch.zeros((plan["rows"][0][1], 64))], [plan], 0, 3)


def test_handover_with_one_rank_needs_no_process_group():
    import torch
    from moonsuperresolution_amd.distributed import exchange_strip_rows
    plan = halo_strip_plan((300, 64), 2, 64, 16, 128, 1)
    t = torch.arange(300 * 64, dtype=torch.float32).reshape(300, 64)
    (got,) = exchange_strip_rows([t], [plan], 0, 1)
    assert got.data_ptr() == t.data_ptr() and got.shape == t.shape

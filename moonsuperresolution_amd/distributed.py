"""Multi-GPU sharding of the tiled path: one process per GPU, tiles partitioned by tile row.

The reference is single-process; its author notes the tile list "can be used to distribute the load"
(process_full_tiles.py:319-320).  Tiles are independent units (each re-computes its halo patches and its own
batches: process_full_tiles.py:449-474), so the exact mode needs NO collective on the data path — batch
composition, and with it SPADE's batch statistics, stay bit-for-bit the reference's.  The only exchange is the
gather of finished rows at the end, done with torch.distributed (backend "nccl" = RCCL over xGMI
on GPUs, "gloo" in the CPU tests).
"""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

import numpy as np


def tile_origins(shape: Tuple[int, int], tile_size: int) -> List[Tuple[int, int]]:
    """generateTileList, process_full_tiles.py:313-325: (xx, yy) of every tile of a raster of ``shape``, y outer."""
    return [(xx, yy) for yy in range(0, shape[0], tile_size) for xx in range(0, shape[1], tile_size)]


def patch_origins_1d(p: int, image_size: int, stride: int, tile_size: int) -> range:
    """Patch origins along one axis of the tile at ``p`` (padded-canvas coordinates), process_full_tiles.py:453-454.
    The ONE statement of that rule on the device side: the tile loop (tiler._prepare_tile, patchOrigins), the halo mode's
    patch grid (halo.patchGrid) and ``input_rows`` below all enumerate origins through it."""
    return range(p, p + tile_size + image_size - stride, stride)


def patch_grid_1d(tile_coords: Sequence[int], image_size: int, stride: int, tile_size: int) -> List[int]:
    """Sorted union of the patch origins of the tiles at ``tile_coords`` along one axis (the halo mode's grid)."""
    return sorted({o for p in tile_coords for o in patch_origins_1d(p, image_size, stride, tile_size)})


def tile_rows(tiles: Sequence[Tuple[int, int]]) -> List[int]:
    return sorted({yy for _, yy in tiles})


def rows_of_rank(n_rows: int, rank: int, world: int) -> Tuple[int, int]:
    """(first, count) of the contiguous block of tile rows rank owns; sizes differ by at most one."""
    base, extra = divmod(n_rows, world)
    return rank * base + min(rank, extra), base + (1 if rank < extra else 0)


def shard_tile_rows(tiles: Sequence[Tuple[int, int]], rank: int, world: int) -> List[Tuple[int, int]]:
    """Contiguous blocks of tile rows per rank, sizes differing by at most one (15 rows on 8 ranks: 2,2,2,2,2,2,2,1)."""
    if not 0 <= rank < world:
        raise ValueError("rank out of range")
    rows = tile_rows(tiles)
    start, count = rows_of_rank(len(rows), rank, world)
    mine = set(rows[start:start + count])
    return [t for t in tiles if t[1] in mine]


def all_gather_rows(local, n_rows: int, T: int, world: int):
    """All-gather the finished rows of one product over the process group (RCCL on GPUs, gloo on CPU tensors).

    local: this rank's [count * T, width] tensor (count = rows_of_rank(n_rows, rank, world)[1]).  Ranks own different
    numbers of tile rows, so every rank contributes a block padded to the largest count; ONE collective writes all
    blocks into one [world * max, width] buffer, which is then compacted in place (ranks with the larger count come
    first, so only blocks after the first short rank move, towards the front) and returned as [n_rows * T, width].
    Peak memory = that buffer + the padded block — not world copies of it."""
    import torch
    import torch.distributed as dist
    base, extra = divmod(n_rows, world)
    max_rows = (base + (1 if extra else 0)) * T
    width = local.shape[1]
    if local.shape[0] == max_rows:
        block = local.contiguous()
    else:
        block = torch.zeros((max_rows, width), dtype=local.dtype, device=local.device)
        block[:local.shape[0]] = local
    out = torch.empty((world * max_rows, width), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, block)
    if extra:   # ranks >= extra hold base rows: close the T-row gap behind each of them
        dst = (extra * (base + 1) + base) * T
        for r in range(extra + 1, world):
            src = r * max_rows
            out[dst:dst + base * T] = out[src:src + base * T].clone()
            dst += base * T
    return out[:n_rows * T]


def process_map_sharded(shape: Tuple[int, int], tile_size: int, tiles: Sequence[Tuple[int, int]],
                        process_tile: Callable[[int, int], Tuple[np.ndarray, np.ndarray, np.ndarray]],
                        rank: int = 0, world: int = 1, gather: bool = True, device=None, as_tensor: bool = False,
                        transfers=None, local: bool = False):
    """Run this rank's tile rows and (optionally) all-gather the finished rows into the full map on every rank.

    process_tile(xx, yy) -> (mean f32 [T,T], std f32 [T,T], good u8 [T,T]) (host arrays or torch tensors).
    Returns (mean, std, good) cropped to ``shape``; without ``gather`` rows of other ranks stay zero.  They are host
    arrays, or with ``as_tensor`` the tensors on ``device`` themselves (the crop is a view): nothing is downloaded.
    ``local`` (with ``as_tensor``): no collective and no full map — only the rows this rank computed, clipped to ``shape``:
    rows strip_plan(...)["rows"][rank] of the products.  ``transfers``: a list that takes ("d2h", bytes, what) for every
    product downloaded (DEMSuperResolution.transfers).
    """
    import torch
    h, w = shape
    T = tile_size
    rows = tile_rows(tiles)
    ncols = len({xx for xx, _ in tiles})
    width = ncols * T
    mine = shard_tile_rows(tiles, rank, world)
    my_rows = tile_rows(mine) if mine else []
    dev = device if device is not None else "cpu"
    mean = torch.zeros((len(my_rows) * T, width), dtype=torch.float32, device=dev)
    std = torch.zeros_like(mean)
    good = torch.zeros((len(my_rows) * T, width), dtype=torch.uint8, device=dev)
    for xx, yy in mine:
        m, s, g = process_tile(xx, yy)
        r0 = my_rows.index(yy) * T
        mean[r0:r0 + T, xx:xx + T] = torch.as_tensor(m).to(dev)
        std[r0:r0 + T, xx:xx + T] = torch.as_tensor(s).to(dev)
        good[r0:r0 + T, xx:xx + T] = torch.as_tensor(g).to(dev)
    if local:
        if not as_tensor:
            raise ValueError("local=True returns this rank's rows as tensors: pass as_tensor=True")
        first = my_rows[0] if my_rows else 0
        return tuple(t[:max(0, min(t.shape[0], h - first)), :w] for t in (mean, std, good))
    if world > 1 and gather:
        mean, std, good = (all_gather_rows(t, len(rows), T, world) for t in (mean, std, good))
    elif world > 1:
        full = [torch.zeros((len(rows) * T, width), dtype=t.dtype, device=dev) for t in (mean, std, good)]
        if my_rows:
            r0 = rows.index(my_rows[0]) * T
            for f, t in zip(full, (mean, std, good)):
                f[r0:r0 + t.shape[0]] = t
        mean, std, good = full
    if as_tensor:
        return tuple(t[:h, :w] for t in (mean, std, good))
    if transfers is not None and mean.is_cuda:
        for name, t in zip(("mean", "std", "good"), (mean, std, good)):
            transfers.append(("d2h", h * w * t.element_size(), f"{name} product"))
    return tuple(t[:h, :w].cpu().numpy() for t in (mean, std, good))


# ----------------------------------------------------------------------------------------------------------------
# Patch-row-sharded ("halo") mode: the exchange step (moonsuperresolution_amd/halo.py holds the GPU side)
# ----------------------------------------------------------------------------------------------------------------
def exchange_halo(send_down, send_up, recv_down_shape, recv_up_shape, rank: int, world: int):
    """Neighbour exchange of the boundary-zone accumulators: every rank sends `send_down` to rank - 1 and `send_up` to
    rank + 1 and receives tensors of the given shapes from them (None at the ends of the chain).  Point-to-point
    send / recv over the process group — RCCL on device tensors (xGMI is point-to-point: neighbour traffic needs no
    ring collective), gloo on host tensors in the CPU tests.  Returns (from_down, from_up)."""
    import torch
    import torch.distributed as dist
    ops, from_down, from_up = [], None, None
    like = send_down if send_down is not None else send_up
    if rank > 0:
        from_down = torch.empty(recv_down_shape, dtype=like.dtype, device=like.device)
        ops.append(dist.P2POp(dist.isend, send_down.contiguous(), rank - 1))
        ops.append(dist.P2POp(dist.irecv, from_down, rank - 1))
    if rank < world - 1:
        from_up = torch.empty(recv_up_shape, dtype=like.dtype, device=like.device)
        ops.append(dist.P2POp(dist.isend, send_up.contiguous(), rank + 1))
        ops.append(dist.P2POp(dist.irecv, from_up, rank + 1))
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    return from_down, from_up


def exchange_halo_start(send_down, send_up, recv_down_shape, recv_up_shape, rank: int, world: int):
    """exchange_halo split in two: the non-blocking sends / receives are started now, the returned ``wait()`` completes them
    and returns (from_down, from_up).  What the caller launches in between (the finalisation of its interior rows) runs
    beside the transfers."""
    import torch
    import torch.distributed as dist
    ops, from_down, from_up = [], None, None
    like = send_down if send_down is not None else send_up
    keep = []
    if rank > 0:
        from_down = torch.empty(recv_down_shape, dtype=like.dtype, device=like.device)
        keep.append(send_down.contiguous())
        ops.append(dist.P2POp(dist.isend, keep[-1], rank - 1))
        ops.append(dist.P2POp(dist.irecv, from_down, rank - 1))
    if rank < world - 1:
        from_up = torch.empty(recv_up_shape, dtype=like.dtype, device=like.device)
        keep.append(send_up.contiguous())
        ops.append(dist.P2POp(dist.isend, keep[-1], rank + 1))
        ops.append(dist.P2POp(dist.irecv, from_up, rank + 1))
    reqs = dist.batch_isend_irecv(ops) if ops else []

    def wait():
        for req in reqs:
            req.wait()
        keep.clear()
        return from_down, from_up
    return wait


def exchange_strip_rows(slabs: Sequence, plans: Sequence[dict], rank: int, world: int) -> list:
    """The hand-over before rank-local encoding in halo mode: per product, ``slabs[i]`` holds this rank's rows
    ``plans[i]["rows"][rank]`` (halo_strip_plan; a cropped view will do).  Rows ``give[rank]`` of it go to rank - 1, rows
    ``take[rank]`` come from rank + 1 — non-blocking send / recv like exchange_halo_start, all products in one batch, the
    contiguous send buffers kept until the wait — and the rows of the rank's strips, [s0 rps, min(s1 rps, H)), are returned as
    one tensor per product: a view of the slab where nothing is taken, else one concatenation.  A rank that neither gives nor
    takes issues nothing (and needs no process group)."""
    import torch
    import torch.distributed as dist
    ops, keep, got, kept = [], [], [], []
    for slab, plan in zip(slabs, plans):
        if not plan["local"]:
            raise ValueError("exchange_strip_rows: a strip of this plan holds rows of three ranks (plan['local'] is False)")
        (r0, r1), (g0, g1), (t0, t1) = plan["rows"][rank], plan["give"][rank], plan["take"][rank]
        if slab.shape[0] != r1 - r0:
            raise ValueError(f"exchange_strip_rows: {slab.shape[0]} rows given for rank {rank}'s rows [{r0}, {r1})")
        n_give, n_take = max(0, g1 - g0), max(0, t1 - t0)
        recv = None
        if n_give:                                       # my first rows complete rank - 1's last strip
            keep.append(slab[:n_give].contiguous())
            ops.append(dist.P2POp(dist.isend, keep[-1], rank - 1))
        if n_take:
            recv = torch.empty((n_take,) + tuple(slab.shape[1:]), dtype=slab.dtype, device=slab.device)
            ops.append(dist.P2POp(dist.irecv, recv, rank + 1))
        kept.append(slab[n_give:])
        got.append(recv)
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
        keep.clear()
    return [k if g is None else torch.cat([k, g], dim=0) for k, g in zip(kept, got)]


def all_gather_var_rows(local, counts: Sequence[int]):
    """All-gather of row slabs whose row counts differ by rank (halo mode: ownership boundaries follow patch rows, not
    tiles): pad to the largest count, one all_gather_into_tensor, trim.  counts[r] = rows of rank r."""
    import torch
    import torch.distributed as dist
    world = len(counts)
    mx = max(counts)
    block = torch.zeros((mx,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    block[:local.shape[0]] = local
    out = torch.empty((world * mx,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, block)
    return torch.cat([out[r * mx:r * mx + counts[r]] for r in range(world)], dim=0)


def halo_zone_rows(ys: Sequence[int], image_size: int, world: int):
    """Geometry of the halo mode for patch-row origins `ys` (sorted, padded-canvas coordinates) split over `world`
    ranks: per rank (g0, g1) = its block of patch rows, (touch_lo, touch_hi) = the canvas rows its own patches reach
    (purged by S // 16 per side, like rebuildTile), (own_lo, own_hi) = the canvas rows it finalises.  Ownership passes
    from rank r - 1 to rank r at the centre of rank r's first patch row."""
    S, p = image_size, image_size // 16
    n = len(ys)
    out = []
    for r in range(world):
        g0, g1 = rows_of_rank(n, r, world)
        g1 = g0 + g1
        if g1 <= g0:
            raise ValueError("halo mode: more ranks than patch rows")
        out.append(dict(g0=g0, g1=g1, touch_lo=ys[g0] + p, touch_hi=ys[g1 - 1] + S - p))
    for r in range(world):
        out[r]["own_lo"] = 0 if r == 0 else ys[out[r]["g0"]] + S // 2
        out[r]["own_hi"] = None if r == world - 1 else ys[out[r + 1]["g0"]] + S // 2
    for r in range(world):       # a pixel may combine at most two ranks: every block must span a whole overlap
        if r + 2 < world and out[r]["touch_hi"] > out[r + 2]["touch_lo"]:
            raise ValueError("halo mode: too few patch rows per rank (a pixel would need three ranks)")
    return out


# ----------------------------------------------------------------------------------------------------------------
# Row windows: which raster rows a rank has to read, pad and upload
# ----------------------------------------------------------------------------------------------------------------
def input_rows(shape: Tuple[int, int], image_size: int, stride: int, tile_size: int, rank: int, world: int,
               mode: str, preprocess: bool = False) -> Tuple[int, int]:
    """Raster rows [r0, r1) (un-padded coordinates) that the patches of ``rank`` can touch.  With ``preprocess``: the rows
    of the input DEM from which those rows of the synthesised DEM are computed (preprocess.window_plan(...)["dem"]: a band
    under 1024 rows wider a side).

    mode "tiles": the patches of the tiles ``shard_tile_rows`` gives the rank; mode "halo": the patch rows
    ``halo_zone_rows`` gives it (the boundary zones it sends and merges are accumulators of those same patches: they
    reach no further raster row).  A patch at canvas origin y reads canvas rows [y, y + S); canvas row c is raster row
    c - (S - s) (padInputs); the range is clipped to the raster.  ``world == 1`` gives (0, H), a rank without work (0, 0).
    Pure arithmetic on the origin enumeration the device code uses (patch_origins_1d): no torch, no library."""
    if mode not in ("tiles", "halo"):
        raise ValueError(f"mode must be 'tiles' or 'halo', got {mode!r}")
    if not 0 <= rank < world:
        raise ValueError("rank out of range")
    if preprocess:
        from .preprocess import window_plan
        r0, r1 = input_rows(shape, image_size, stride, tile_size, rank, world, mode)
        return window_plan(shape, (r0, r1))["dem"] if r1 > r0 else (0, 0)
    H = int(shape[0])
    S, s, T = image_size, stride, tile_size
    if world == 1:
        return 0, H
    tiles = tile_origins(shape, T)
    if mode == "tiles":
        mine = tile_rows(shard_tile_rows(tiles, rank, world))
        if not mine:
            return 0, 0
        first, last = patch_origins_1d(mine[0], S, s, T)[0], patch_origins_1d(mine[-1], S, s, T)[-1]
    else:
        ys = patch_grid_1d(tile_rows(tiles), S, s, T)
        z = halo_zone_rows(ys, S, world)[rank]
        first, last = ys[z["g0"]], ys[z["g1"] - 1]
    r0, r1 = max(0, first - (S - s)), min(H, last + S - (S - s))
    return (r0, r1) if r1 > r0 else (0, 0)


def canvas_shape(shape: Tuple[int, int], image_size: int, stride: int) -> Tuple[int, int]:
    """padInputs, process_full_tiles.py:246-267: the no_value canvas is ((dim // 1024) + 1) * 1024 + 2 (S - s) a side."""
    halo = image_size - stride
    return ((shape[0] // 1024) + 1) * 1024 + 2 * halo, ((shape[1] // 1024) + 1) * 1024 + 2 * halo


def canvas_rows(shape: Tuple[int, int], image_size: int, stride: int, r0: int, r1: int) -> Tuple[int, int]:
    """Canvas rows [c0, c1) that raster rows [r0, r1) occupy in padInputs' canvas: shifted by the S - s margin, and a
    window that touches the raster's first / last row also takes the no_value margin above / below it."""
    H = int(shape[0])
    halo = image_size - stride
    full = canvas_shape(shape, image_size, stride)[0]
    return (0 if r0 == 0 else r0 + halo), (full if r1 == H else r1 + halo)


def crop_for_rank(dsr, rank: int, world: int, mode: str = "tiles") -> Tuple[int, int]:
    """Keep only the raster rows ``rank`` needs of the host rasters a DEMSuperResolution holds (setImages / loadImages
    done, padInputs not yet): the canvas padInputs then builds is that row window, not the whole raster.  Run it before
    ``process_map_sharded(..., dsr.processTile, rank, world)``.  Returns the rows kept."""
    if dsr.img is None or dsr.dem is None:
        raise ValueError("crop_for_rank needs the host rasters: call it after setImages / loadImages, before padInputs")
    r0, r1 = input_rows(dsr.dem_shape, dsr.image_size, dsr.stride, dsr.tile_size, rank, world, mode)
    a, b = r0 - dsr.row0, r1 - dsr.row0
    if a < 0 or b > dsr.dem.shape[0]:
        raise ValueError(f"the rasters held (rows [{dsr.row0}, {dsr.row0 + dsr.dem.shape[0]})) do not contain rank "
                         f"{rank}'s rows [{r0}, {r1})")
    if isinstance(dsr.img, np.ndarray):
        img, dem = np.ascontiguousarray(dsr.img[a:b]), np.ascontiguousarray(dsr.dem[a:b])
    else:                                            # resident rasters: a copy on the device, so that the rest is released
        img, dem = dsr.img[a:b].clone(), dsr.dem[a:b].clone()
    dsr.setImages(img, dem, row0=r0, full_shape=dsr.dem_shape)
    return r0, r1


# ----------------------------------------------------------------------------------------------------------------
# Rank-local product encoding: which strips of a product file a rank can encode from the rows it computed
# ----------------------------------------------------------------------------------------------------------------
def strip_plan(shape: Tuple[int, int], itemsize: int, tile_size: int, world: int) -> dict:
    """The strips of one product file of a raster of ``shape`` = (H, W) with ``itemsize`` bytes a sample, over the ranks of
    a tile-row-sharded run (processFiles(mode="tiles", products="rank0")).  Pure arithmetic; no torch, no library.

      rps        geotiff._rows_per_strip(H, W * itemsize): strip k holds rows [k rps, min((k + 1) rps, H))
      n_strips   ceil(H / rps)
      rows       per rank, the product rows [r0, r1) it computes: its tile rows (rows_of_rank) x tile_size, clipped to H;
                 (H, H) or the like, r0 == r1, for a rank without rows
      straddles  True when a strip holds rows of two ranks: a rank boundary inside the raster that is no multiple of rps.
                 Rank-local encoding needs False (for every product dtype of the run)
      strips     per rank, the strips [s0, s1) it encodes — consecutive ranges that cover every strip once, (s, s) for a
                 rank without rows; None when ``straddles``"""
    from .geotiff import _rows_per_strip
    H, W = int(shape[0]), int(shape[1])
    if H < 1 or W < 1 or itemsize < 1 or tile_size < 1 or world < 1:
        raise ValueError("strip_plan needs a non-empty raster, itemsize, tile_size and world >= 1")
    rps = _rows_per_strip(H, W * int(itemsize))
    n_strips = -(-H // rps)
    n_tile_rows = -(-H // tile_size)
    rows = []
    for r in range(world):
        first, count = rows_of_rank(n_tile_rows, r, world)
        rows.append((min(first * tile_size, H), min((first + count) * tile_size, H)))
    straddles = any(0 < r0 < H and r0 % rps for r0, _ in rows)
    strips = None if straddles else [(-(-r0 // rps), -(-r1 // rps)) for r0, r1 in rows]
    return {"rps": rps, "n_strips": n_strips, "rows": rows, "straddles": straddles, "strips": strips}


def halo_strip_plan(shape: Tuple[int, int], itemsize: int, image_size: int, stride: int, tile_size: int, world: int) -> dict:
    """strip_plan for a patch-row-sharded run (processFiles(mode="halo", products="rank0")).  Ownership follows patch rows
    (halo_zone_rows), not tiles, so a rank boundary is seldom a strip boundary; instead of giving up, the rank that owns a
    strip's first row takes the strip's other rows from the rank above (exchange_strip_rows).  Pure arithmetic.

      rps, n_strips  as in strip_plan
      rows       per rank, the product rows [r0, r1) it finalises: canvas rows [own_lo, own_hi) less the S - s margin, clipped
                 to [0, H].  Consecutive, covering [0, H); (H, H) for a rank whose zone lies below the raster
      strips     per rank, the strips [s0, s1) it encodes: strip k goes to the rank that owns row k rps.  Consecutive,
                 covering every strip once; (s, s) for a rank that owns no first row of a strip
      take       per rank, the rows [t0, t1) it needs from rank + 1 to complete its last strip: [r1, min(s1 rps, H)), empty
                 (t0 == t1) when r1 is a multiple of rps or H, or when the rank encodes no strip
      give       per rank, take[rank - 1]: the rows it hands down; (0, 0) for rank 0
      local      False when some take[r] reaches beyond rows[r + 1] (a strip holds rows of three ranks): rank-local encoding
                 needs True (for every product dtype of the run)"""
    from .geotiff import _rows_per_strip
    H, W = int(shape[0]), int(shape[1])
    if H < 1 or W < 1 or itemsize < 1 or tile_size < 1 or world < 1 or image_size < 1 or not 0 < stride <= image_size:
        raise ValueError("strip_plan needs a non-empty raster, itemsize, tile_size and world >= 1")
    S, halo = int(image_size), int(image_size) - int(stride)
    rps = _rows_per_strip(H, W * int(itemsize))
    n_strips = -(-H // rps)
    ys = patch_grid_1d(tile_rows(tile_origins((H, W), tile_size)), S, stride, tile_size)

    def clip(c):                                          # canvas row -> raster row
        return H if c is None else max(0, min(H, c - halo))
    rows = [(clip(z["own_lo"]), clip(z["own_hi"])) for z in halo_zone_rows(ys, S, world)]
    strips = [(min(n_strips, -(-r0 // rps)), min(n_strips, -(-r1 // rps))) for r0, r1 in rows]
    take = [(r1, min(s1 * rps, H) if s1 > s0 else r1) for (_, r1), (s0, s1) in zip(rows, strips)]
    give = [(0, 0)] + take[:-1]
    local = all(t1 <= rows[r + 1][1] for r, (t0, t1) in enumerate(take) if t1 > t0)
    return {"rps": rps, "n_strips": n_strips, "rows": rows, "strips": strips, "take": take, "give": give, "local": local}

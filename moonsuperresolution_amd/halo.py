"""Patch-row-sharded ("halo") mode of the tiled path — BASELINE.json north_star's "RCCL exchange of overlap halos".

NOT the reference's algorithm: process_full_tiles.py re-generates, for every 1024 x 1024 tile, the S - s wide halo of
patches around it (:449-454), so on a large raster every patch position is generated ~2x (1.995x at S = 512 / s = 64,
SURVEY.md section 5).  Here every position is generated ONCE: ranks own contiguous blocks of patch ROWS, each rank
accumulates the weighted incremental mean / variance of its own patches (msr_stitch_partial: rebuildTile stopped before
its finalisation), and the pixels near a block boundary — reached by patches of two ranks — combine the two ranks'
accumulators pairwise (msr_halo_merge) after a neighbour exchange (distributed.exchange_halo: RCCL send / recv).

Deviations from the reference (documented, inherent; oracle/tiler_ref.py::process_map_halo restates the mode):
  1. batches are cut from a rank's patch rows, not per tile, so SPADE's batch statistics (spade.py:21) see other batch
     mates: generator outputs differ beyond rounding (not for the identity model);
  2. the variance is textbook West, because the reference's aliased update (:400-402) has no pairwise combine;
  3. boundary-zone pixels are combined pairwise instead of sequentially: float32 rounding differs (~1e-7 relative).
The exact, reference-identical multi-GPU mode is the tile-row sharding of distributed.process_map_sharded.

Memory (round 3): a rank works through its patch rows in BANDS (``band_rows`` patch rows at a time, default sized to
``band_bytes`` = 4 GiB of predictions): a band is generated, accumulated into the canvas rows it reaches — in place, block by
block, with only the band's own keys (msr_stitch_accumulate: the running update resumes from what earlier bands left, so the
STITCHER does not depend on the band size, bit for bit, given identical predictions) — and its predictions are freed.  The
predictions themselves are band-invariant only for a model without batch statistics, or under ``batching="rank"`` (below):
with the default ``batching="band"`` every band is compacted and batched on its own and ends in its own zero-padded call, so
the batch mates of a patch — and through SPADE's batch moments its output — follow the band cut.  What stays resident is the rank's
accumulator slab (3 float32 images of the canvas rows its patches reach: 2.1 GB for a 1/8 share of the 15000 x 70000 raster)
plus one band; round 2 kept all predictions of the rank (34 GB at that size).
A band's compaction and its calls (extract, generate) are the tile mode's helpers (tiler._compact_patches, _generator_calls,
_host_model_calls); this module owns the bands, the carry between them, the accumulation and the zones.
Exchange: the two boundary-zone slabs go to the neighbours as non-blocking send / recv while the interior rows (reached by this
rank's patches only) are finalised; the zones are finalised when the neighbours' slabs have arrived.

Two opt-in forms (the defaults are the code paths as they were; whether either default flips is a later decision):
  ``batching="rank"``    the rank's valid patches, in generation order, are ONE sequence cut into calls of B at multiples of B
                         of that sequence (batch_schedule).  A band issues whole calls only; its unfilled tail (< B patches) is
                         carried in front of the next band's patches (msr_compact_patches_carry) and only the rank's last
                         call is zero-padded.  Every issued chunk is a consecutive slice of the all-at-once sequence, so the
                         resumed accumulation still applies each pixel's updates in that sequence's order; the rows a chunk
                         reaches start at the first carried patch row.  With the counter sampler the padding rows of the last
                         call draw (index in the rank's sequence, 0xFFFFFFFE, 0xFFFFFFFF).  The products then equal
                         oracle/tiler_ref.py::process_map_halo's whatever ``band_rows`` / ``band_bytes`` is.
  ``accumulate="band"``  one launch over the canvas rows a band reaches (msr_stitch_accumulate_band) instead of one full-block
                         pass per T x T block the band touches: the same bits, no per-block key tensors, no host syncs.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .distributed import halo_zone_rows, patch_grid_1d
from .tiler import _CARRIED, PRODUCTS, DEMSuperResolution, _need_process_group


def batch_schedule(valid_per_band: Sequence[int], batch_size: int) -> List[Tuple[int, int]]:
    """The calls of ``batching="rank"`` before the final flush: [(calls issued by the band, patches carried after it)].
    A band issues the whole calls of (carry + its valid patches) and carries the rest (< batch_size) on; what the last band
    carries goes into one more, zero-padded call (flush_padding), so the rank makes ceil(total / batch_size) calls and the
    k-th call holds patches [k * batch_size, (k + 1) * batch_size) of the rank's sequence, wherever the bands are cut."""
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size} < 1")
    out, carry = [], 0
    for nv in valid_per_band:
        if nv < 0:
            raise ValueError(f"negative valid count {nv}")
        calls, carry = divmod(carry + int(nv), batch_size)
        out.append((calls, carry))
    return out


def flush_padding(valid_per_band: Sequence[int], batch_size: int) -> List[Tuple[int, int, int]]:
    """Noise ids (as uint32 triples) of the padding rows of the rank's last call under ``batching="rank"``: the row's index
    in the rank's whole compacted sequence — patches issued by earlier calls plus its slot in the flush call — then
    0xFFFFFFFE, 0xFFFFFFFF.  Empty when the sequence fills its last call (or is empty)."""
    sched = batch_schedule(valid_per_band, batch_size)
    issued = batch_size * sum(c for c, _ in sched)
    carry = sched[-1][1] if sched else 0
    return [(issued + slot, 0xFFFFFFFE, 0xFFFFFFFF) for slot in range(carry, batch_size)] if carry else []


class HaloShardedSuperResolution(DEMSuperResolution):
    """DEMSuperResolution with the halo mode added: ``processMapHalo(rank, world)``.

    ``resident`` is accepted and must be False: the halo mode's inputs and its default products still end on the host.
    ``product_tile``, ``overviews``, ``product_layout`` and ``product_predictor`` are DEMSuperResolution's, checked there.

    ``processFiles(mode="halo", rank=, world=)`` is the driver on files (DEMSuperResolution.processFiles; ``batching`` and
    ``accumulate`` go to processMapHalo).  With the default ``products="gathered"`` every rank all-gathers the three slabs,
    downloads them and writes the files.  With ``products="rank0"`` the slabs stay on the rank's device: it crops them (views)
    to its raster rows, hands the rows that belong to a strip begun by the rank below down to it and takes the rest of its own
    last strip from the rank above (distributed.halo_strip_plan / exchange_strip_rows: fewer than rows-per-strip rows a
    product and boundary, recorded in ``handover_rows`` = {product: (give, take)}), encodes its strips with the ``encoder``
    set, and rank 0 alone writes — byte for byte the files of the gathered run with the same ranks.  ``products_path`` is
    "rank0" then (always with one rank, which needs no process group); when a strip holds rows of three ranks the run takes
    the gathered slabs instead, rank 0 alone writes, and ``products_path`` is "gathered"."""

    def __init__(self, *args, resident: bool = False, **kwargs) -> None:
        if not isinstance(resident, bool):
            raise ValueError(f"resident must be a bool, got {resident!r}")
        if resident:
            raise ValueError("resident=True is not built for the halo mode")
        super().__init__(*args, **kwargs)
        self.handover_rows = {}                      # processFiles(products="rank0"): per product (give, take) of this rank

    def patchGrid(self) -> Tuple[list, list]:
        """Unique patch origins the reference's tiles touch (padded-canvas coordinates): (ys, xs), sorted."""
        S, s, T = self.image_size, self.stride, self.tile_size
        if S % s or T % s:
            # msr_stitch_partial bins patches by (origin - block origin) / stride: origins that are not multiples of the
            # stride relative to every T x T block would be dropped silently (and the union grid would be irregular)
            raise ValueError(f"halo mode needs a stride that divides image_size and tile_size (got stride {s}, "
                             f"image_size {S}, tile_size {T}); use the tile mode (processMap) for other strides")
        tiles = self.generateTileList()
        ys = patch_grid_1d(sorted({py for _, py in tiles}), S, s, T)
        xs = patch_grid_1d(sorted({px for px, _ in tiles}), S, s, T)
        return ys, xs

    # ------------------------------------------------------------------------------------------------------------
    def _generate_rows(self, ys: Sequence[int], xs: Sequence[int], carry: Optional[dict] = None, last: bool = True):
        """Validity, normalisation statistics, device-side batch assembly and the generator calls for every patch at
        rows `ys` (the tile mode's helpers, on the caller's stream, the pipeline streams forked from and joined to it): returns
        (preds [ncall * B, S, S], keys [cap, 2] canvas origins, dmm [cap, 2], patches to stitch).
        The kernels that read the canvas get window rows (origin - canvas_row0, tiler.padInputs); the keys stay canvas
        origins (the compaction subtracts tile_y = -canvas_row0).
        ``carry`` (batching="rank"): the rank's state {"n": patches carried, "issued": patches of the calls made so far, and
        the carried rows of the five compaction outputs}.  They stand in front of this band's patches; only whole calls are
        issued, unless ``last``, and the rest is left in ``carry``.  The patches to stitch are the live rows of the calls
        issued (with carry=None: the band's valid patches, as ever)."""
        S, B = self.image_size, self.batch_size
        dev = self.device
        c0 = self._window()[0]
        self._check_rows(f"patch rows {ys[0]} .. {ys[-1]}", ys)
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            xt = torch.tensor(xs, dtype=torch.int32, device=dev)
            yt = torch.tensor([y - c0 for y in ys], dtype=torch.int32, device=dev)
            st = self._compact_patches(xt.repeat(len(ys)), yt.repeat_interleave(len(xs)), 0, -c0, carry)
            cap, keys, dmm = st["cap"], st["keys"], st["dmm"]
            tot, ncall = (int(v) for v in st["meta"].cpu().tolist())
            nv = tot - (0 if carry is None else carry["n"])   # this band's own valid patches
            seq0 = 0                                      # index, in the sequence the calls are cut from, of slot 0
            if carry is not None:
                seq0 = carry["issued"]
                if not last:
                    ncall = tot // B                      # whole calls only: the tail waits for the next band
            n_out = min(tot, ncall * B)
            self._range_retire()                      # range_check: the previous band's scan, read with this band's counts
            preds = torch.empty((max(ncall * B, 1), S, S), dtype=torch.float32, device=dev)
            self.last_noise_ids = None                # [cap, 3] of the band just issued, with the counter sampler
            if self._gen is not None:
                self._ready_pipeline()
                batches = [torch.empty((B, S, S, 2), dtype=torch.float32, device=dev) for _ in self._gens]
                ids = None
                if self.counter_noise:
                    # The noise follows the patch: id (canvas origin x, y, 0xFFFFFFFF), whatever band or batch it lands in;
                    # the padding rows of the last call draw (slot, 0xFFFFFFFE, 0xFFFFFFFF) — the slot in the band, or, with
                    # batching="rank", in the rank's whole sequence, so that they too are the same for every band cut.
                    slot = torch.arange(cap, dtype=torch.int32, device=dev)
                    live = slot < tot
                    ids = torch.full((cap, 3), -1, dtype=torch.int32, device=dev)
                    ids[:, 0] = torch.where(live, keys[:, 0], slot + seq0)
                    ids[:, 1] = torch.where(live, keys[:, 1], torch.full_like(slot, -2))
                self.last_noise_ids = ids
                for ps in self._pstreams:
                    ps.wait_stream(cur)
                self._generator_calls(st, ncall, preds, batches, ids)
                for ps in self._pstreams:
                    cur.wait_stream(ps)
                    for t in batches + [preds, st["sx"], st["sy"], st["mm_sel"]] + ([] if ids is None else [ids]):
                        t.record_stream(ps)
            else:
                self._host_model_calls(st, ncall, preds)
            if carry is not None:
                for name in _CARRIED:
                    carry[name] = st[name][n_out:tot].clone()    # < B rows; the band's arrays go with its predictions
                carry["n"] = tot - n_out
                carry["issued"] = seq0 + ncall * B
            self.last_counts_halo = (nv, ncall)
            return preds, keys, dmm, n_out

    def _accumulate_band(self, acc, y_b0: int, preds, keys, dmm, nv: int, band_lo: int, band_hi: int) -> None:
        """Add the patches of one band (canvas rows [band_lo, band_hi) are the rows they reach) to the accumulator slab
        ``acc`` [3, n_by * T, n_bx * T] whose row 0 is canvas row ``y_b0`` (a multiple of T): every T x T block the band
        touches is continued in place from its current content, with the band's keys only."""
        T, S, s = self.tile_size, self.image_size, self.stride
        halo = S - s
        lib, h, dev = self._lib, self._h, self.device
        pitch = acc.shape[2]
        by0, by1 = (band_lo - y_b0) // T, (band_hi - 1 - y_b0) // T
        with torch.cuda.device(dev):
            for by in range(max(by0, 0), min(by1, acc.shape[1] // T - 1) + 1):
                for bx in range(pitch // T):
                    y0, x0 = y_b0 + by * T, bx * T
                    # patch keys relative to the block's grid origin (x0 - halo, y0 - halo): accumulator coordinate =
                    # block pixel + halo, exactly the tile mode's geometry
                    rel = keys[:max(nv, 1)] - torch.tensor([x0 - halo, y0 - halo], dtype=torch.int32, device=dev)
                    win = acc[:, by * T:(by + 1) * T, bx * T:(bx + 1) * T]
                    rc = lib.msr_stitch_accumulate(h, preds.data_ptr(), rel.data_ptr(), dmm.data_ptr(), nv, T, s,
                                                   win[0].data_ptr(), win[1].data_ptr(), win[2].data_ptr(), pitch, 1,
                                                   self._stream())
                    _lib.raise_for(lib, h, rc, "msr_stitch_accumulate")

    def _accumulate_band_once(self, acc, y_b0: int, preds, keys, dmm, n: int, y_first: int, y_last: int,
                              xs: Sequence[int]) -> None:
        """_accumulate_band in one launch (msr_stitch_accumulate_band): the ``n`` patches, whose rows lie in
        [y_first, y_last] (canvas origins, on the stride), update the canvas rows they reach; the keys go as they are."""
        S, s = self.image_size, self.stride
        p = S // 16
        lib, h, dev = self._lib, self._h, self.device
        pitch = acc.shape[2]
        row_lo, row_hi = max(y_first + p, y_b0), min(y_last + S - p, y_b0 + acc.shape[1])
        if row_hi <= row_lo or n <= 0:
            return
        ngx, ngy = (xs[-1] - xs[0]) // s + 1, (y_last - y_first) // s + 1
        with torch.cuda.device(dev):
            grid = torch.empty(ngx * ngy, dtype=torch.int32, device=dev)
            rc = lib.msr_stitch_accumulate_band(h, preds.data_ptr(), keys.data_ptr(), dmm.data_ptr(), n, s, xs[0], y_first,
                                                ngx, ngy, grid.data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(),
                                                acc[2].data_ptr(), pitch, y_b0, row_lo, row_hi, pitch, self._stream())
            _lib.raise_for(lib, h, rc, "msr_stitch_accumulate_band")

    def _finalize(self, a, b=None):
        """msr_halo_merge over [3, rows, W] accumulators -> (mean, std, good)."""
        rows, w = a.shape[1], a.shape[2]
        with torch.cuda.device(self.device):
            mean = torch.empty((rows, w), dtype=torch.float32, device=self.device)
            std = torch.empty_like(mean)
            good = torch.empty((rows, w), dtype=torch.uint8, device=self.device)
            if rows * w:
                a = a.contiguous()
                bp = [None, None, None]
                if b is not None:
                    b = b.contiguous()
                    bp = [b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr()]
                rc = self._lib.msr_halo_merge(self._h, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), bp[0], bp[1],
                                              bp[2], rows * w, self.no_value, mean.data_ptr(), std.data_ptr(),
                                              good.data_ptr(), self._stream())
                _lib.raise_for(self._lib, self._h, rc, "msr_halo_merge")
        return mean, std, good

    # ------------------------------------------------------------------------------------------------------------
    def cropInputs(self, rank: int, world: int) -> Tuple[int, int]:
        """Keep only the raster rows this rank's patch rows read (distributed.input_rows, mode "halo") of the host rasters
        held; padInputs then builds that row window of the canvas.  Returns the rows kept."""
        from .distributed import crop_for_rank
        return crop_for_rank(self, rank, world, "halo")

    def haloAccumulate(self, rank: int = 0, world: int = 1, band_rows: Optional[int] = None, band_bytes: int = 4 << 30,
                       max_rows: int = 0, crop_inputs: bool = False, batching: str = "band", accumulate: str = "blocks"):
        """Phase 1 (no communication): generate this rank's patch rows band by band and accumulate them.  Returns the
        state ``haloFinish`` takes: the accumulators of the canvas rows the rank's patches reach, what it must send to its
        neighbours and the shapes of what it receives.  ``band_rows`` patch rows per band (default: as many as fit
        ``band_bytes`` of predictions); ``max_rows`` > 0 stops after that many patch rows (benchmarks of a share of a
        large raster: the accumulators of the rows not reached stay empty).  ``crop_inputs``: when the instance still
        holds host rasters, keep only this rank's rows of them (cropInputs) before they are padded and uploaded; the
        accumulators, the zones and the result are the same bits.
        ``batching``: "band" cuts every band's valid patches into calls on their own (each band ends in a zero-padded call);
        "rank" cuts the rank's whole sequence at multiples of B and carries a band's unfilled tail into the next band, so the
        batches — and the products of a model with batch statistics — do not depend on the bands.  ``accumulate``: "blocks"
        stitches a band block by block, "band" in one launch; the same bits.  See the module docstring."""
        if batching not in ("band", "rank"):
            raise ValueError(f"batching must be 'band' or 'rank', got {batching!r}")
        if accumulate not in ("blocks", "band"):
            raise ValueError(f"accumulate must be 'blocks' or 'band', got {accumulate!r}")
        if self.dem_padded is None or self.dem is not None:
            if crop_inputs and self.dem is not None:
                self.cropInputs(rank, world)
            self.padInputs()
        S, T = self.image_size, self.tile_size
        p = S // 16
        hp, wp = self.dem_padded_shape
        ys, xs = self.patchGrid()
        zones = halo_zone_rows(ys, S, world)
        z = zones[rank]
        lo, hi = z["touch_lo"], z["touch_hi"]
        own_lo = z["own_lo"]
        own_hi = hp if z["own_hi"] is None else z["own_hi"]
        if (rank > 0 and own_lo < lo) or (rank < world - 1 and own_hi > hi):
            raise ValueError("halo mode needs overlapping patches (stride <= S/2 - S/16)")
        my_ys = ys[z["g0"]:z["g1"]]
        if band_rows is None:
            band_rows = max(1, int(band_bytes // max(1, len(xs) * S * S * 4)))
        y_b0 = (lo // T) * T
        n_by = (hi - y_b0 + T - 1) // T
        n_bx = (wp + T - 1) // T
        nv_tot = nc_tot = 0
        with torch.cuda.device(self.device):
            slab = torch.zeros((3, n_by * T, n_bx * T), dtype=torch.float32, device=self.device)
            done = 0
            carry = {"n": 0, "issued": 0} if batching == "rank" else None
            first_row = None                             # the patch row the carried patches start at (or lie behind)
            counts, marks = [], []
            for b0 in range(0, len(my_ys), band_rows):
                band = my_ys[b0:b0 + band_rows]
                if max_rows and done + len(band) > max_rows:
                    band = band[:max_rows - done]
                if not band:
                    break
                done += len(band)
                last = b0 + band_rows >= len(my_ys) or bool(max_rows and done >= max_rows)
                if carry is None or carry["n"] == 0:
                    first_row = band[0]
                preds, keys, dmm, n_out = self._generate_rows(band, xs, carry, last)
                marks.append([torch.cuda.Event(enable_timing=True) for _ in range(2)])
                marks[-1][0].record()
                if accumulate == "band":
                    self._accumulate_band_once(slab, y_b0, preds, keys, dmm, n_out, first_row, band[-1], xs)
                elif carry is None or n_out:
                    self._accumulate_band(slab, y_b0, preds, keys, dmm, n_out, first_row + p, band[-1] + S - p)
                marks[-1][1].record()
                if carry is not None and self.last_counts_halo[1]:
                    first_row = band[0]                  # a band that issued a call carries only patches of its own
                counts.append(self.last_counts_halo)
                nv_tot += self.last_counts_halo[0]
                nc_tot += self.last_counts_halo[1]
                del preds, keys, dmm                     # the band's predictions are not needed again
            acc = slab[:, lo - y_b0:hi - y_b0, :wp]
        self._range_retire()                          # the last band's scan
        self.last_counts_halo = (nv_tot, nc_tot)
        self.last_band_counts = counts                # per band: (valid patches of the band, calls it issued)
        self._band_marks = marks
        self.last_band_rows = band_rows
        st = dict(rank=rank, world=world, acc=acc, lo=lo, hi=hi, own_lo=own_lo, own_hi=own_hi, wp=wp,
                  send_down=acc[:, :own_lo - lo] if rank > 0 else None,                     # rows [touch_lo, own_lo)
                  send_up=acc[:, own_hi - lo:] if rank < world - 1 else None,                # rows [own_hi, touch_hi)
                  down_rows=max(0, zones[rank - 1]["touch_hi"] - own_lo) if rank > 0 else 0,
                  up_rows=max(0, own_hi - zones[rank + 1]["touch_lo"]) if rank < world - 1 else 0)
        return st

    def bandStitchSeconds(self) -> List[float]:
        """Device time of every band's accumulation in the last haloAccumulate (waits for the work to finish)."""
        torch.cuda.synchronize(self.device)
        return [a.elapsed_time(b) / 1e3 for a, b in self._band_marks]

    def haloFinish(self, st, from_down=None, from_up=None, *, exchange: Optional[Callable] = None):
        """Phase 2: combine the boundary zones with the neighbours' accumulators (from_down = rank - 1's rows
        [own_lo, own_lo + down_rows), its patches come first; from_up = rank + 1's rows [own_hi - up_rows, own_hi)) and
        finalise.  With ``exchange`` (a callable returning (from_down, from_up), e.g. the ``wait`` of
        distributed.exchange_halo_start) the interior rows are finalised FIRST and the exchange is waited for afterwards:
        the transfer runs beside the interior kernels.
        Returns ((mean, std, good) for canvas rows [own_lo, own_hi), (own_lo, own_hi))."""
        acc, lo, hi, own_lo, own_hi, wp = st["acc"], st["lo"], st["hi"], st["own_lo"], st["own_hi"], st["wp"]
        with torch.cuda.device(self.device):
            mean = torch.full((own_hi - own_lo, wp), self.no_value, dtype=torch.float32, device=self.device)
            std = torch.full_like(mean, self.no_value)
            good = torch.zeros((own_hi - own_lo, wp), dtype=torch.uint8, device=self.device)

            def put(r0, r1, a, b=None):
                # in slabs of T rows: the accumulator is a view with the slab's pitch, so each piece is compacted for
                # the merge kernel — T rows at a time instead of a second copy of the whole interior
                for c0 in range(r0, r1, self.tile_size):
                    c1 = min(r1, c0 + self.tile_size)
                    m, s_, g = self._finalize(a[:, c0 - r0:c1 - r0], None if b is None else b[:, c0 - r0:c1 - r0])
                    mean[c0 - own_lo:c1 - own_lo], std[c0 - own_lo:c1 - own_lo], good[c0 - own_lo:c1 - own_lo] = m, s_, g

            # rows only my patches reach: independent of the neighbours (the zone row counts are known from the geometry)
            d_end = own_lo + (st["down_rows"] if st["rank"] > 0 else 0)
            u_beg = own_hi - (st["up_rows"] if st["rank"] < st["world"] - 1 else 0)
            if exchange is None and from_down is None:
                d_end = own_lo
            if exchange is None and from_up is None:
                u_beg = own_hi
            m0, m1 = max(lo, d_end), min(hi, u_beg)
            put(m0, m1, acc[:, m0 - lo:m1 - lo])
            if exchange is not None:
                from_down, from_up = exchange()
            if d_end > own_lo:                                   # zone shared with the rank below
                put(own_lo, d_end, from_down, acc[:, own_lo - lo:d_end - lo])
            if own_hi > u_beg:                                   # zone shared with the rank above
                put(u_beg, own_hi, acc[:, u_beg - lo:own_hi - lo], from_up)
        return (mean, std, good), (own_lo, own_hi)

    def processMapHalo(self, img: Optional[np.ndarray] = None, dem: Optional[np.ndarray] = None, rank: int = 0,
                       world: int = 1, exchange: Optional[Callable] = None, band_rows: Optional[int] = None,
                       crop_inputs: bool = False, batching: str = "band", accumulate: str = "blocks"):
        """This rank's share of the map in halo mode: accumulate band by band, start the exchange of the boundary zones
        with the neighbours (non-blocking send / recv: distributed.exchange_halo_start, RCCL on the GPUs), finalise the
        interior rows beside it, then the zones.  ``exchange``: a blocking replacement with exchange_halo's signature.
        ``crop_inputs``: pad and upload only the raster rows this rank's patches read; ``batching`` / ``accumulate``: the
        band-invariant batch sequence and the one-launch accumulation (haloAccumulate)."""
        if img is not None:
            self.setImages(img, dem)
        st = self.haloAccumulate(rank, world, band_rows=band_rows, crop_inputs=crop_inputs, batching=batching,
                                 accumulate=accumulate)
        if world == 1:
            return self.haloFinish(st)
        torch.cuda.current_stream(self.device).synchronize()      # the slabs are complete before they are sent
        wp = st["wp"]
        shapes = ((3, st["down_rows"], wp), (3, st["up_rows"], wp))
        if exchange is not None:
            return self.haloFinish(st, *exchange(st["send_down"], st["send_up"], shapes[0], shapes[1], rank, world))
        from .distributed import exchange_halo_start
        wait = exchange_halo_start(st["send_down"], st["send_up"], shapes[0], shapes[1], rank, world)
        return self.haloFinish(st, exchange=wait)

    def cropHalo(self, slabs: Sequence[Tuple[Tuple[torch.Tensor, torch.Tensor, torch.Tensor], Tuple[int, int]]]):
        """Assemble per-rank slabs (in rank order) into the final rasters cropped to the input extent: final pixel
        (y, x) is canvas pixel (y + S - s, x + S - s)."""
        return self._crop_to_raster([torch.cat([sl[0][k] for sl in slabs], dim=0) for k in range(3)])

    def _crop_to_raster(self, parts: Sequence[torch.Tensor]):
        """Whole-canvas-height products -> host arrays of the raster's extent."""
        halo = self.image_size - self.stride
        h, w = self.dem_shape
        return tuple(p[halo:halo + h, halo:halo + w].cpu().numpy() for p in parts)

    def ownedRowCounts(self, world: int) -> List[int]:
        """Canvas rows each rank of ``world`` owns, in rank order: its slab's height, what all_gather_var_rows takes."""
        ys, _ = self.patchGrid()
        hp = self.dem_padded_shape[0]
        zones = halo_zone_rows(ys, self.image_size, world)
        return [(hp if z["own_hi"] is None else z["own_hi"]) - z["own_lo"] for z in zones]

    def _process_files_sharded(self, preprocess: bool, rank: int, world: int, mode: str, gather: bool,
                               swap_dsize: bool = True, batching: str = "band", accumulate: str = "blocks"):
        """processFiles(mode="halo"): this rank reads only the rows its patch rows touch, runs its share (processMapHalo:
        the zone exchange needs an initialised process group when world > 1) and, with ``gather``, all-gathers the slabs;
        without it the rows other ranks own stay zero.  ``batching`` / ``accumulate`` are processMapHalo's."""
        if mode != "halo":
            return super()._process_files_sharded(preprocess, rank, world, mode, gather, swap_dsize)
        from .distributed import all_gather_var_rows
        self._load_rank_rows(preprocess, rank, world, mode, swap_dsize)
        (m, sd, g), (own_lo, own_hi) = self.processMapHalo(rank=rank, world=world, batching=batching, accumulate=accumulate)
        if world > 1 and gather:
            counts = self.ownedRowCounts(world)
            parts = [all_gather_var_rows(t, counts) for t in (m, sd, g)]
        else:
            hp = self.dem_padded_shape[0]
            parts = [torch.zeros((hp,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in (m, sd, g)]
            for full, t in zip(parts, (m, sd, g)):
                full[own_lo:own_hi] = t
        return self._crop_to_raster(parts)

    def _process_files_rank0(self, preprocess: bool, rank: int, world: int, mode: str, swap_dsize: bool = True,
                             batching: str = "band", accumulate: str = "blocks", **sharded) -> None:
        """processFiles(mode="halo", products="rank0"): see processFiles.  The slabs a rank finalised stay on its device until
        they are encoded (``encoder="host"``: the rows of its strips are downloaded once, after the hand-over)."""
        if mode != "halo":
            return super()._process_files_rank0(preprocess, rank, world, mode, swap_dsize, **sharded)
        if sharded:
            raise TypeError(f"processFiles: mode='halo' takes no {sorted(sharded)}")
        from .distributed import all_gather_var_rows, exchange_strip_rows, halo_strip_plan
        _need_process_group(world)
        self._load_rank_rows(preprocess, rank, world, mode, swap_dsize)
        slabs, (own_lo, own_hi) = self.processMapHalo(rank=rank, world=world, batching=batching, accumulate=accumulate)
        (h, w), halo = self.dem_shape, self.image_size - self.stride
        names = [name for name, _ in PRODUCTS]
        plans = [halo_strip_plan((h, w), np.dtype(dt).itemsize, self.image_size, self.stride, self.tile_size, world)
                 for _, dt in PRODUCTS]
        local = all(p["local"] for p in plans)
        self.products_path = "rank0" if local or world == 1 else "gathered"
        self.handover_rows = {}
        if not local:
            # a strip holds rows of three ranks (a narrow raster): the gathered slabs, written by rank 0 alone
            counts = self.ownedRowCounts(world)
            products = self._crop_to_raster([all_gather_var_rows(t, counts) for t in slabs])
            if rank == 0:
                for name, data in zip(names, products):
                    self.saveGTiff(data, data.dtype, name)
            return
        r0, r1 = plans[0]["rows"][rank]                   # the rows are the same for every product: views, nothing moves
        c0 = r0 + halo - own_lo if r1 > r0 else 0        # a zone below the raster: no product row
        assert 0 <= c0 and c0 + r1 - r0 <= own_hi - own_lo, ((r0, r1), (own_lo, own_hi))
        mine = [t[c0:c0 + r1 - r0, halo:halo + w] for t in slabs]
        for name, plan in zip(names, plans):
            self.handover_rows[name] = (plan["give"][rank], plan["take"][rank])
        if world > 1:
            torch.cuda.current_stream(self.device).synchronize()  # the slabs are complete before rows of them are sent
        with torch.cuda.device(self.device):
            mine = exchange_strip_rows(mine, plans, rank, world)
        for name, data, plan in zip(names, mine, plans):
            self._encode_gather_write(name, data, plan, rank, world)

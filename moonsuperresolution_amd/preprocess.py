"""Raster pre-processing of the inference driver (process_full_tiles.py:184-244), SURVEY.md 8f rank 3.

``preprocess`` = nodata in-filling of the ortho-image (result stored, never used — reference quirk), then the
synthesis of the low-resolution DEM: x1/4 INTER_AREA -> in-filling -> x1/4 INTER_AREA -> INTER_CUBIC back to full
size.  The two resamplers run on the GPU through the C ABI (``msr_resize_area_rows`` / ``msr_resize_cubic_rows``, which
also do the no-data <-> NaN marking between the steps; the full-resolution raster is read and written once); the
in-filling stays on the host exactly like the reference: the same ``scipy.interpolate.griddata(method="cubic")`` call on
each tile that has holes, with ``scipy.ndimage.label`` (8-connected) in place of ``cv2.connectedComponents``.

``infill="device"`` (opt-in, a stated deviation: infill.py) fills the same pixels with a local thin-plate fill on the GPU
(``msr_infill_small_holes``): the x1/4 grid then never leaves the device between the two area steps, and no SciPy call is made.

Pre-processing is local in rows: the cubic reads 4 rows of the x1/16 grid, each area step 4 source rows, and the in-filling
works on 256-row tiles of the x1/4 grid.  ``window_plan`` states which rows of each grid a range of output rows depends on,
and ``preprocess_rows`` computes exactly those from a row window of the input DEM — bit-identical to the same rows of the
whole-raster result, which goes through the same code with the window [0, H).  A rank of a sharded run pre-processes its
own band (``DEMSuperResolution.preprocess(rows=)``, ``distributed.input_rows(preprocess=True)``).

OpenCV is not available here and the reference holds no fixture of ``cv2.resize`` output, so the resamplers follow
OpenCV's published algorithm (see oracle/preprocess_ref.py, against which the kernels are bit-exact): parity with a
real OpenCV build is unpinned.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib


def _cv_round(v: float) -> int:
    return int(np.rint(v))


def resize_area(lib, handle, src: torch.Tensor, factor: int = 4) -> torch.Tensor:
    """cv2.resize(src, (0,0), fx=1/factor, fy=1/factor, interpolation=cv2.INTER_AREA) on a CUDA float32 raster."""
    if src.dim() != 2 or src.dtype != torch.float32 or not src.is_cuda:
        raise ValueError("resize_area expects a 2-D float32 CUDA tensor")
    src = src.contiguous()
    h, w = src.shape
    dh, dw = _cv_round(h / factor), _cv_round(w / factor)
    dst = torch.empty((dh, dw), dtype=torch.float32, device=src.device)
    rc = lib.msr_resize_area(handle, src.data_ptr(), h, w, factor, dst.data_ptr(), dh, dw,
                             torch.cuda.current_stream(src.device).cuda_stream)
    _lib.raise_for(lib, handle, rc, "msr_resize_area")
    return dst


def resize_cubic(lib, handle, src: torch.Tensor, dsize_wh: Tuple[int, int]) -> torch.Tensor:
    """cv2.resize(src, (width, height), interpolation=cv2.INTER_CUBIC) on a CUDA float32 raster."""
    if src.dim() != 2 or src.dtype != torch.float32 or not src.is_cuda:
        raise ValueError("resize_cubic expects a 2-D float32 CUDA tensor")
    src = src.contiguous()
    h, w = src.shape
    dw, dh = int(dsize_wh[0]), int(dsize_wh[1])
    dst = torch.empty((dh, dw), dtype=torch.float32, device=src.device)
    rc = lib.msr_resize_cubic(handle, src.data_ptr(), h, w, dst.data_ptr(), dh, dw,
                              torch.cuda.current_stream(src.device).cuda_stream)
    _lib.raise_for(lib, handle, rc, "msr_resize_cubic")
    return dst


def interpolateMissingValues(data: np.ndarray, no_value: float, max_fill_area: int = 256) -> np.ndarray:
    """process_full_tiles.py:184-212 (in place; also returned).  A cubic ``griddata`` surface through the valid pixels of
    the tile; only 8-connected hole regions smaller than ``max_fill_area`` take its values.  Like the reference, the
    region census includes label 0 — the VALID pixels — so it takes part in the "smallest region too large" test and
    in the size filter."""
    from scipy import interpolate, ndimage
    holes = data <= no_value
    if not holes.any() or holes.all():          # nothing to fill / nothing to interpolate from
        return data
    labels, _ = ndimage.label(holes, structure=np.ones((3, 3), dtype=bool))
    sizes = np.bincount(labels.ravel())         # sizes[0] = number of valid pixels, sizes[k] = pixels of hole k
    if sizes.min() > max_fill_area:             # every region (the valid area included) is too large
        return data
    rows, cols = np.nonzero(~holes)             # row-major, the order of the reference's boolean indexing
    grid_r, grid_c = np.mgrid[0:data.shape[0], 0:data.shape[1]]
    surface = interpolate.griddata((cols, rows), data[rows, cols], (grid_c, grid_r), method="cubic")
    take = (sizes < max_fill_area)[labels]
    data[take] = surface[take]
    return data


def fillNan(image: np.ndarray, no_value: float, tile_size: int = 1024, border: int = 128,
            max_fill_area: int = 256) -> np.ndarray:
    """process_full_tiles.py:214-224: tiles of ``tile_size`` every ``tile_size - 2*border`` pixels, each filled on its
    own; only the part of a tile inside its ``border`` frame is written back, clipped ``border`` short of the raster."""
    h, w = image.shape
    out = image.copy()
    step = tile_size - 2 * border
    for top in range(0, h, step):
        bottom = min(top + tile_size - border, h - border)
        for left in range(0, w, step):
            right = min(left + tile_size - border, w - border)
            tile = interpolateMissingValues(image[top:top + tile_size, left:left + tile_size].copy(), no_value,
                                            max_fill_area=max_fill_area)
            out[top + border:bottom, left + border:right] = tile[border:-border, border:-border]
    return out


FILL_TILE, FILL_BORDER, FILL_AREA = 256, 32, 24     # fillNan's arguments on the x1/4 grid (process_full_tiles.py:236)
RESIZE_NODATA_TO_NAN, RESIZE_NAN_TO_NODATA = 1, 2    # MSR_RESIZE_* of include/moonsr.h


def _cubic_tap_rows(d0: int, d1: int, n_src: int, n_dst: int) -> Tuple[int, int]:
    """Source rows [a, b) the cubic taps of destination rows d0 .. d1 - 1 touch, by the kernel's own expression
    (csrc/tiler.hip::cubic_first_tap): s = floor(float32((d + 0.5) * (n_src / n_dst) - 0.5)), taps s - 1 .. s + 2 clamped to
    the source.  s is monotone in d, so the first and the last row bound the rest."""
    scale = n_src / n_dst

    def s(d):
        return int(np.floor(np.float32((d + 0.5) * scale - 0.5)))
    return min(max(s(d0) - 1, 0), n_src - 1), min(max(s(d1 - 1) + 2, 0), n_src - 1) + 1


def _plan_from_d16(shape: Tuple[int, int], a16: int, b16: int) -> Dict[str, object]:
    """The rows of the in-filled x1/4 grid, of the x1/4 grid and of the input that rows [a16, b16) of the x1/16 grid depend
    on, and the in-fill tiles to run (window_plan)."""
    H = int(shape[0])
    h4 = _cv_round(H / 4)
    fill = (4 * a16, min(4 * b16, h4))
    lo, hi = fill
    tiles = []
    for top in range(0, h4, FILL_TILE - 2 * FILL_BORDER):
        w0, w1 = top + FILL_BORDER, min(top + FILL_TILE - FILL_BORDER, h4 - FILL_BORDER)     # the rows the tile writes
        if w1 > w0 and w0 < fill[1] and w1 > fill[0]:
            tiles.append(top)
            lo, hi = min(lo, top), max(hi, min(top + FILL_TILE, h4))
    return {"d16": (a16, b16), "fill": fill, "d4": (lo, hi), "dem": (min(4 * lo, H), min(4 * hi, H)), "tiles": tiles}


def window_plan(shape: Tuple[int, int], out_rows: Tuple[int, int]) -> Dict[str, object]:
    """Row ranges [first, end) that rows ``out_rows`` = [r0, r1) of the synthesised DEM of a raster of ``shape`` = (H, W)
    depend on (``preprocess(..., swap_dsize=False)``; with h4 = rint(H / 4), h16 = rint(h4 / 4), round-half-even):

      d16    rows of the x1/16 grid the cubic taps of output rows r0 .. r1 - 1 touch
      fill   rows [4 a16, min(4 b16, h4)) of the in-filled x1/4 grid: what the second area step reads for them
      d4     rows of the x1/4 grid: ``fill`` and the full row extent [top, min(top + 256, h4)) of every in-fill tile (top in
             range(0, h4, 192)) whose written rows [top + 32, min(top + 224, h4 - 32)) are not empty and meet ``fill``; the
             32 rows at either end of the grid that no tile writes pass through un-filled, as in fillNan
      dem    rows [min(4 A4, H), min(4 B4, H)) of the input DEM: what the first area step reads for d4 = [A4, B4)
      tiles  the tops of those tiles

    Pure arithmetic; needs no GPU.  ``dem`` reaches at most 223 rows of the x1/4 grid (a tile's extent beyond a row it
    writes) plus 3 rows of the x1/16 grid (the cubic's taps) beyond [r0, r1): under 1024 input rows a side."""
    H = int(shape[0])
    r0, r1 = int(out_rows[0]), int(out_rows[1])
    if not 0 <= r0 < r1 <= H:
        raise ValueError(f"rows [{r0}, {r1}) are not rows of a raster of {H}")
    h16 = _cv_round(_cv_round(H / 4) / 4)
    if h16 < 1:
        raise ValueError(f"a raster of {H} rows has no x1/16 grid")
    return _plan_from_d16(shape, *_cubic_tap_rows(r0, r1, h16, H))


def _area_rows(lib, handle, src: torch.Tensor, src_row0: int, full_rows: int, dst_rows: Tuple[int, int], no_value: float,
               flags: int) -> torch.Tensor:
    """Rows ``dst_rows`` of the x1/4 INTER_AREA of a raster of ``full_rows`` of which ``src`` holds the rows from
    ``src_row0`` (msr_resize_area_rows)."""
    n, w = src.shape
    dst = torch.empty((dst_rows[1] - dst_rows[0], _cv_round(w / 4)), dtype=torch.float32, device=src.device)
    rc = lib.msr_resize_area_rows(handle, src.data_ptr(), src_row0, n, full_rows, w, 4, dst.data_ptr(), dst_rows[0],
                                  dst.shape[0], dst.shape[1], no_value, flags,
                                  torch.cuda.current_stream(src.device).cuda_stream)
    _lib.raise_for(lib, handle, rc, "msr_resize_area_rows")
    return dst


def _fill_rows(band: np.ndarray, row0: int, h4: int, tiles, no_value: float) -> np.ndarray:
    """fillNan(tile_size=256, border=32, max_fill_area=24) on rows [row0, row0 + len(band)) of an x1/4 grid of ``h4`` rows,
    for the tiles at the row tops ``tiles`` only (window_plan), all columns.  Each tile is cut at the true ``h4`` and at the
    grid's width, so it is the tile fillNan cuts from the whole grid and takes the same values."""
    w = band.shape[1]
    out = band.copy()
    step = FILL_TILE - 2 * FILL_BORDER
    for top in tiles:
        bottom = min(top + FILL_TILE - FILL_BORDER, h4 - FILL_BORDER)
        for left in range(0, w, step):
            right = min(left + FILL_TILE - FILL_BORDER, w - FILL_BORDER)
            if right <= left + FILL_BORDER:
                continue
            tile = interpolateMissingValues(band[top - row0:min(top + FILL_TILE, h4) - row0, left:left + FILL_TILE].copy(),
                                            no_value, max_fill_area=FILL_AREA)
            out[top + FILL_BORDER - row0:bottom - row0, left + FILL_BORDER:right] = tile[FILL_BORDER:-FILL_BORDER,
                                                                                         FILL_BORDER:-FILL_BORDER]
    return out


INFILL_MODES = ("host", "device")
ORTHO_AREA, ORTHO_BORDER = 8, 128                    # fillNan's max_fill_area and border on the ortho (process_full_tiles.py:229)


def _check_infill(infill: str) -> str:
    if infill not in INFILL_MODES:
        raise ValueError(f"infill must be 'host' or 'device', got {infill!r}")
    return infill


def _log(transfers, direction: str, nbytes: int, what: str) -> None:
    """One host <-> device copy issued here, for the caller's list (DEMSuperResolution.transfers)."""
    if transfers is not None:
        transfers.append((direction, int(nbytes), what))


def _lowres_rows(lib, handle, device, dem_window, row0: int, shape: Tuple[int, int], plan, no_value: float,
                 infill: str = "host", transfers=None) -> torch.Tensor:
    """Rows plan["d16"] of the x1/16 grid (device tensor, no-data as NaN) from a row window of the input DEM that holds
    plan["dem"]: area on the d4 band, in-filling (host: of the plan's tiles; device: in place on the band, whose rows
    plan["fill"] lie 32 rows from its cut edges and so take the whole grid's bits), area on the in-filled rows.
    ``dem_window`` is a NumPy array (its rows plan["dem"] are uploaded) or a float32 CUDA tensor (they are read where they
    lie); with ``infill="host"`` the x1/4 band goes to SciPy and comes back, either way."""
    H = int(shape[0])
    h4 = _cv_round(H / 4)
    (m0, m1), (q0, q1), (f0, f1) = plan["dem"], plan["d4"], plan["fill"]
    if m0 < row0 or m1 > row0 + dem_window.shape[0]:
        raise ValueError(f"the row window [{row0}, {row0 + dem_window.shape[0]}) lacks rows of [{m0}, {m1}), which the "
                         f"pre-processing of x1/16-grid rows {plan['d16']} reads")
    if isinstance(dem_window, torch.Tensor):
        d = dem_window[m0 - row0:m1 - row0].contiguous()      # whole rows of a contiguous raster: a view, no copy
    else:
        _log(transfers, "h2d", (m1 - m0) * dem_window.shape[1] * 4, "DEM rows for the x1/4 area step")
        d = torch.from_numpy(np.ascontiguousarray(dem_window[m0 - row0:m1 - row0], dtype=np.float32)).to(device)
    d4 = _area_rows(lib, handle, d, m0, H, (q0, q1), no_value, RESIZE_NODATA_TO_NAN | RESIZE_NAN_TO_NODATA)
    del d
    if infill == "device":
        from .infill import infill_device
        infill_device(lib, handle, d4, q0, h4, no_value, FILL_AREA, FILL_BORDER)
        d4 = d4[f0 - q0:f1 - q0]
    else:
        _log(transfers, "d2h", d4.numel() * 4, "x1/4 grid for the host in-fill")
        filled = _fill_rows(d4.cpu().numpy(), q0, h4, plan["tiles"], no_value)
        _log(transfers, "h2d", (f1 - f0) * filled.shape[1] * 4, "in-filled x1/4 grid")
        d4 = torch.from_numpy(np.ascontiguousarray(filled[f0 - q0:f1 - q0])).to(device)
    return _area_rows(lib, handle, d4, f0, h4, plan["d16"], no_value, RESIZE_NODATA_TO_NAN)


def _cubic_rows(lib, handle, d16: torch.Tensor, a16: int, h16: int, dst_rows: Tuple[int, int], dst_shape: Tuple[int, int],
                no_value: float, as_tensor: bool = False, transfers=None):
    """Rows ``dst_rows`` of the INTER_CUBIC resize to ``dst_shape`` = (rows, cols) of an x1/16 grid of ``h16`` rows of which
    ``d16`` holds the rows from ``a16``; NaN leaves as no_value.  Host float32, or with ``as_tensor`` the device tensor."""
    dst = torch.empty((dst_rows[1] - dst_rows[0], dst_shape[1]), dtype=torch.float32, device=d16.device)
    rc = lib.msr_resize_cubic_rows(handle, d16.data_ptr(), a16, d16.shape[0], h16, d16.shape[1], dst.data_ptr(), dst_rows[0],
                                   dst.shape[0], dst_shape[0], dst_shape[1], no_value, RESIZE_NAN_TO_NODATA,
                                   torch.cuda.current_stream(d16.device).cuda_stream)
    _lib.raise_for(lib, handle, rc, "msr_resize_cubic_rows")
    if as_tensor:
        return dst
    _log(transfers, "d2h", dst.numel() * 4, "synthesised DEM")
    return dst.cpu().numpy()


def fill_ortho_device(lib, handle, device, img, no_value: float, band_bytes: int = 1 << 28, transfers=None):
    """The device form of fillNan(img, no_value, 1024, 128, 8): msr_infill_small_holes with (max_area, margin) = (8, 128) on
    bands of whole rows of at most ``band_bytes``, so that device memory stays bounded.  Consecutive bands share
    margin + max_area = 136 rows; each gives the rows up to the middle of what it shares, which lie 68 >= max_area rows from
    its cut edge and so hold the whole raster's bits.  Host float32 — or, for a float32 CUDA tensor, a tensor: every band is
    a clone of its rows of ``img`` (which keeps its bits; a band filled in place would show the next one, in the rows they
    share, holes the first had filled in part), and nothing leaves the device."""
    from .infill import infill_device
    H, W = img.shape
    share = ORTHO_BORDER + ORTHO_AREA
    per_band = min(H, int(band_bytes) // (4 * W))
    if per_band < H and per_band <= share:
        raise ValueError(f"band_bytes {band_bytes} holds {per_band} rows of {W} columns: bands need more than {share}")
    on_device = isinstance(img, torch.Tensor)
    out = torch.empty_like(img) if on_device and per_band < H else None if on_device else np.empty_like(img)
    top = 0
    while True:
        end = min(top + per_band, H)
        if on_device:
            band = img[top:end].clone()
        else:
            _log(transfers, "h2d", (end - top) * W * 4, "ortho band for the in-fill")
            band = torch.from_numpy(np.ascontiguousarray(img[top:end])).to(device)
        infill_device(lib, handle, band, top, H, no_value, ORTHO_AREA, ORTHO_BORDER)
        if out is None:                               # the whole raster in one band: the filled clone is the result
            return band
        a = top + share // 2 if top else 0
        b = end - share // 2 if end < H else H
        if on_device:
            out[a:b] = band[a - top:b - top]
        else:
            _log(transfers, "d2h", (b - a) * W * 4, "in-filled ortho band")
            out[a:b] = band[a - top:b - top].cpu().numpy()
        if end == H:
            return out
        top = end - share


def _raster(a):
    """A raster argument as it is worked on: a float32 CUDA tensor stays one (contiguous), anything else is a float32 array."""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda or a.dtype != torch.float32:
            raise ValueError("a raster given as a tensor must be a CUDA float32 tensor")
        return a.contiguous()
    return np.asarray(a, np.float32)


def preprocess_rows(lib, handle, device, dem_window, row0: int, shape: Tuple[int, int],
                    out_rows: Tuple[int, int], no_value: float, infill: str = "host", transfers=None):
    """Rows ``out_rows`` of what ``preprocess(..., swap_dsize=False, infill=infill)[1]`` returns for the whole raster of
    ``shape``, bit for bit, from ``dem_window`` = its rows [row0, row0 + len(dem_window)), which must hold
    window_plan(shape, out_rows)["dem"] (ValueError otherwise).  Only the plan's d4, fill and d16 rows are computed.  Host
    float32 for an array; for a float32 CUDA tensor a tensor, with the same bits."""
    _check_infill(infill)
    H, W = int(shape[0]), int(shape[1])
    dem_window = _raster(dem_window)
    if dem_window.ndim != 2 or dem_window.shape[1] != W:
        raise ValueError(f"the row window must be 2-D with the raster's {W} columns")
    plan = window_plan(shape, out_rows)
    with torch.cuda.device(device):
        d16 = _lowres_rows(lib, handle, device, dem_window, int(row0), shape, plan, no_value, infill, transfers)
        return _cubic_rows(lib, handle, d16, plan["d16"][0], _cv_round(_cv_round(H / 4) / 4), out_rows, (H, W), no_value,
                           isinstance(dem_window, torch.Tensor), transfers)


def preprocess(lib, handle, device, img, dem, no_value: float, swap_dsize: bool = True, infill: str = "host",
               band_bytes: int = 1 << 28, transfers=None):
    """process_full_tiles.py:226-244.  Returns (filled ortho, low-resolution DEM at full size), both host float32 — or,
    each where the argument is a float32 CUDA tensor, a tensor with the same bits: with ``infill="device"`` nothing then
    leaves the device; with ``infill="host"`` the ortho and the x1/4 grid, which SciPy reads, go down and their in-filled
    forms come up.  ``transfers``: a list that takes ``(direction, bytes, what)`` for every copy between host and device
    issued here (DEMSuperResolution.transfers).

    ``infill="host"`` (default) in-fills with SciPy's griddata like the reference; ``"device"`` fills the same pixels on the
    GPU with the values of infill.infill_reference (a stated deviation) and makes no SciPy call: the ortho in bands of at most
    ``band_bytes`` (fill_ortho_device), the x1/4 grid in place between the two area steps.

    ``swap_dsize=True`` reproduces :241, where ``self.dem_shape`` = (rows, cols) is handed to ``cv2.resize`` as
    (width, height): the result then has shape (cols, rows), so — like the reference — only square rasters survive
    the later ``padInputs``.  ``swap_dsize=False`` resizes to (rows, cols) proper: preprocess_rows with the window [0, H)."""
    img, dem = _raster(img), _raster(dem)
    if _check_infill(infill) == "device":
        with torch.cuda.device(device):
            image = fill_ortho_device(lib, handle, device, img, no_value, band_bytes, transfers)
    elif isinstance(img, torch.Tensor):
        _log(transfers, "d2h", img.numel() * 4, "ortho for the host in-fill")
        image = fillNan(img.cpu().numpy(), no_value, tile_size=1024, border=ORTHO_BORDER, max_fill_area=ORTHO_AREA)
        _log(transfers, "h2d", image.size * 4, "in-filled ortho")
        image = torch.from_numpy(image).to(img.device)
    else:
        image = fillNan(img, no_value, tile_size=1024, border=ORTHO_BORDER, max_fill_area=ORTHO_AREA)
    H, W = dem.shape
    if not swap_dsize:
        return image, preprocess_rows(lib, handle, device, dem, 0, (H, W), (0, H), no_value, infill, transfers)
    h16 = _cv_round(_cv_round(H / 4) / 4)
    with torch.cuda.device(device):      # every row of the x1/16 grid, then the cubic to W rows of H columns
        d16 = _lowres_rows(lib, handle, device, dem, 0, (H, W), _plan_from_d16((H, W), 0, h16), no_value, infill, transfers)
        return image, _cubic_rows(lib, handle, d16, 0, h16, (0, W), (W, H), no_value, isinstance(dem, torch.Tensor),
                                  transfers)

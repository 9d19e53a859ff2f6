"""Tiled inference driver on the GPU — the host-side mirror of ``DEMSuperResolution`` (process_full_tiles.py:129-587).

Same names and argument meaning as the reference for the part of the class that is on the hot path
(``DSRConfig``, ``padInputs``, ``generateTileList``, ``processTile``, ``rebuildTile``, ``rebuildMap``) and for the
file boundary either side of it (``loadImages`` / ``saveGTiff`` on ``geotiff.py`` instead of GDAL).  Nodata
in-filling and low-res-DEM synthesis live in preprocess.py (``DEMSuperResolution.preprocess``; with
``rows=`` for the row window of a sharded rank, which ``processFiles(preprocess=True, mode=...)`` uses) — or feed
pre-processed rasters, as files (``processFiles``) or as arrays (``setImages`` / ``processMap``).

What moves to the GPU (libmoonsr_hip.so, csrc/tiler.hip):
  getPatch + normalize     -> msr_patch_stats + msr_extract_patches   (validity, min/max, [-0.5,0.5] scaling)
  processBatch             -> Generator.forward_device (patches never leave HBM) or any host callable
  rebuildTile              -> msr_stitch_tile (gather-form weighted incremental mean / variance, bit-exact)
  batch assembly           -> msr_compact_patches (stable device-side compaction of the valid patches)
Batch composition is exactly the reference's Python loop (invalid patches are skipped, the last batch is
zero-padded: process_full_tiles.py:455-474) — SPADE's batch statistics make that composition part of the result.
It is stated once, for the tiles and for halo.py's bands: _compact_patches, then _generator_calls / _host_model_calls.
The host needs only the two counts (valid patches, calls) of a tile, 8 bytes fetched through pinned memory while
the previous tile is still generating (iterTiles), so the generator stream never drains between tiles.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .distributed import canvas_rows, canvas_shape, patch_origins_1d, tile_origins


@dataclasses.dataclass
class DSRConfig:
    """process_full_tiles.py:53-66, field for field."""
    image_size: int = 256
    stride: int = 32
    batch_size: int = 16
    tile_size: int = 1024
    no_value: float = -32768.0
    upsample_factor: float = 1.0
    map_name: str = None
    save_path: str = None
    source_folder_path: str = None
    ortho_image_name: str = "run-DRG.tif"
    dem_name: str = "run-DEM.tif"
    model_path: str = None


def blend_window(image_size: int) -> np.ndarray:
    """makeGaussianKernel + 1e-7, purged S//16 per side (process_full_tiles.py:347-361, 391-393), float64.

    Evaluated with NumPy exactly as the reference writes it so that the GPU stitcher, which takes this array,
    is bit-identical to the NumPy path (libm's exp may differ from NumPy's in the last bit)."""
    S = image_size

    def gaus2d(x=0, y=0, mx=0, my=0, sx=1, sy=1):
        return 1. / (2. * np.pi * sx * sy) * np.exp(-((x - mx) ** 2. / (2. * sx ** 2.) + (y - my) ** 2. / (2. * sy ** 2.)))
    x = np.linspace(-S / 2, S / 2, S)
    xg, yg = np.meshgrid(x, x)
    kern = gaus2d(xg, yg, sx=S / 5, sy=S / 5)
    kern = (kern - kern.min()) / (kern.max() - kern.min())
    p = S // 16
    return np.ascontiguousarray((kern + 1e-7)[p:-p, p:-p])


_CARRIED = ("sx", "sy", "mm_sel", "keys", "dmm")     # the compaction's five outputs, in the order of the kernel's arguments
PRODUCTS = (("mean", np.float32), ("std", np.float32), ("good", np.uint16))     # (name, dtype of its file), in processMap's order


def _need_process_group(world: int) -> None:
    """The rank-local writers gather their strips to rank 0: with more than one rank that takes a process group."""
    if world > 1:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("products='rank0' needs an initialised process group")


class DEMSuperResolution:
    """GPU tiler/stitcher with the reference's interface (process_full_tiles.py:129-156).

    Args:
        config: DSRConfig.
        model: a ``moonsuperresolution_amd.Generator`` (device fast path) or any callable
            ``model(batch[B,S,S,2], training=False) -> [B,S,S,C]`` like the reference accepts; the default is the
            reference's identity self-check (process_full_tiles.py:143).
        device: HIP device ordinal.
        as_implemented: keep the reference's aliased variance update; False = textbook West.
        range_check: "off" (default: no call is added), "warn" or "raise" — with a ``Generator`` model, scan the activation
            ranges of the FIRST generator call of every tile (``Generator.range_scan_async`` on that call's stream and handle)
            and read the records where the next tile's two counts are read (after the last tile: when the run ends), so
            the loop gains no host wait of its own.  A regime other than "parity" is kept in ``self.range_report`` and
            warned about once per run ("warn"), or raises RuntimeError when that tile's records are read ("raise").
        encoder: "host" (default) or "device" — where saveGTiff differences and LZW-encodes the strips of the files it
            writes (geotiff.write_geotiff); the files are the same byte for byte.
        decoder: "host" (default) or "device" — where loadImages LZW-decodes the strips / tiles of the two input files and
            undoes their predictor (geotiff.read_geotiff); the rasters are the same bit for bit.
        infill: "host" (default) or "device" — where preprocess in-fills the small no-data holes of the ortho and of the x1/4
            grid.  "host" is the reference's griddata surface, tile by tile (SciPy).  "device" fills THE SAME PIXELS with
            other values (infill.py: a local thin-plate fill, defined by infill.infill_reference, which the kernel equals bit
            for bit); the x1/4 grid then stays on the GPU between the two area steps and no SciPy call is made.
        resident: False (default) or True — where the rasters are HELD between the stages, never which arithmetic runs.  With
            True, ``img`` / ``dem`` / ``image`` and the products of processMap / rebuildMap / processTiles are CUDA tensors
            (float32; ``good`` uint8) where they are NumPy arrays otherwise, the canvases are built with device-to-device
            copies, tiles are pasted into device maps and saveGTiff takes the tensors; a stage chosen to run on the host
            (decoder / infill / encoder = "host", a model that is no Generator) keeps its own round trip.  The files written
            are the same byte for byte.
        product_tile, overviews: None and 0 (default: strips, as ever), or what saveGTiff hands to geotiff.write_geotiff as
            ``tile`` and ``overviews``: products in tiles of (tile_h, tile_w), positive multiples of 16, with that many
            reduced-resolution levels (``overviews`` > 0 needs ``product_tile``); with ``encoder="device"`` the levels are
            reduced and the tiles encoded on the GPU.  The rank-local writer (processFiles(products="rank0")) knows strips
            only and refuses ``product_tile``.
        product_layout: "plain" (default) or "cog" (needs ``product_tile``) — what saveGTiff hands to geotiff.write_geotiff as
            ``layout``: the same tiles, levels and tags in the order of a cloud-optimised GeoTIFF, the IFDs first and the
            coarse levels before the fine ones; with ``encoder="device"`` the tiles are encoded where their level lies, those
            of all reduced levels in one launch.
        product_predictor: 2 (default: the horizontal predictor saveGTiff asks GDAL for) or 3 — the floating-point predictor
            (GDAL's PREDICTOR=3; geotiff.fp_predictor_reference) for the float32 products ``mean`` and ``std``, with every
            encoder, layout and writer; ``good`` (uint16) keeps predictor 2.  The rasters read back are the same bit for bit
            (geotiff.read_geotiff with ``decoder="host"``); any other value is a ValueError.

    ``transfers`` is a diagnostic: a list of ``(direction, bytes, what)``, direction "h2d" or "d2h", to which the driver,
    preprocess.py and geotiff.py append every raster-scale copy they issue themselves (and the per-block bookkeeping of the
    device codecs); processFiles empties it when it starts.  ``products_path`` is "rank0" or "gathered" after a sharded
    processFiles: which of the two product writers ran.
    """

    def __init__(self, config: DSRConfig, model: Callable = lambda x, training=False: x, device: int = 0,
                 as_implemented: bool = True, pipeline: int = 2, range_check: str = "off", encoder: str = "host",
                 decoder: str = "host", infill: str = "host", resident: bool = False,
                 product_tile: Optional[Tuple[int, int]] = None, overviews: int = 0, product_layout: str = "plain",
                 product_predictor: int = 2) -> None:
        from . import geotiff
        self.product_tile, self.overviews = geotiff.check_layout(product_tile, overviews)   # saveGTiff: the products' layout
        self.product_layout = geotiff.check_file_order(product_layout, self.product_tile)
        if isinstance(product_predictor, bool) or product_predictor not in (2, 3):
            raise ValueError(f"product_predictor must be 2 or 3, got {product_predictor!r}")
        self.product_predictor = int(product_predictor)   # saveGTiff: the predictor of the float32 products
        if not isinstance(resident, bool):
            raise ValueError(f"resident must be a bool, got {resident!r}")
        self.resident = resident                     # where the rasters are held between the stages: HBM, or host memory
        self.transfers: List[Tuple[str, int, str]] = []
        self.products_path = None
        for name, where in (("encoder", encoder), ("decoder", decoder), ("infill", infill)):
            if where not in ("host", "device"):
                raise ValueError(f"{name} must be 'host' or 'device', got {where!r}")
        self.encoder = encoder                       # saveGTiff: who differences and LZW-encodes the strips (geotiff.py)
        self.decoder = decoder                       # loadImages: who LZW-decodes the blocks and undoes the predictor
        self.infill = infill                         # preprocess: who fills the small no-data holes (preprocess.py, infill.py)
        if range_check not in ("off", "warn", "raise"):
            raise ValueError(f"range_check must be 'off', 'warn' or 'raise', got {range_check!r}")
        self.range_check = range_check
        self.range_report = None                     # the first non-parity RangeReport of a run (else the last one read)
        self._range_pending = None                   # the handle whose scan has not been read yet
        self._range_warned = False
        self.map_name = config.map_name
        self.save_path = config.save_path
        self.folder_path = config.source_folder_path
        self.left_image_name = config.ortho_image_name
        self.dem_name = config.dem_name
        self.no_value = float(config.no_value)
        self.stride = int(config.stride)
        self.image_size = int(config.image_size)
        self.batch_size = int(config.batch_size)
        self.upsample_factor = 1                     # process_full_tiles.py:153
        self.tile_size = int(config.tile_size)
        self.model = model
        self.as_implemented = as_implemented
        self.pipeline = max(1, int(pipeline))        # generator handles / streams the calls of a tile alternate over
        self._gens = None
        self._pstreams = None
        self._prep_stream = None
        self.gated = os.environ.get("MSR_TILER_GATED", "0") != "0"
        self._gate = None
        self._gate_ring = 0
        self._gate_events = [torch.cuda.Event() for _ in range(8)] if torch.cuda.is_available() else []
        self._bufs = None
        self._batches = None
        self._last = (None, 0, 0)
        self._last_calls = None
        S, s = self.image_size, self.stride
        if S < 64 or S & (S - 1):
            # narrower than the reference (any size): the generator's six 2x up-samplings from S/64 and the conv
            # kernels' power-of-two pixel tiles fix S to 64 * 2^k; documented in INTEGRATION.md
            raise ValueError("image_size must be a power of two >= 64")
        if s <= 0 or s > S:
            raise ValueError("stride must be in (0, image_size]")
        if not torch.cuda.is_available():
            raise RuntimeError("moonsuperresolution_amd needs a HIP device (MI355X / gfx950); there is no CPU fallback")
        self.device = torch.device("cuda", device)
        self._lib = _lib.load()
        from .generator import Generator
        self._gen: Optional[Generator] = model if isinstance(model, Generator) else None
        if self._gen is not None:
            if self._gen.image_size != S or self._gen.batch_size != self.batch_size:
                raise ValueError("Generator image_size/batch_size differ from the DSRConfig")
            self._h = self._gen._h
            self._own_handle = False
            self._make_pipeline()
        else:
            # a handle only for the tiler kernels (no weights needed); variant is irrelevant
            cfg = _lib.MsrConfig(S, max(1, min(self.batch_size, 16)), 256, _lib.VARIANT_IDS["gaugan_no_kl"], device, 0)
            h = C.c_void_p()
            _lib.raise_for(self._lib, None, self._lib.msr_create(C.byref(cfg), C.byref(h)), "msr_create")
            self._h = h
            self._own_handle = True
        w = blend_window(S)
        rc = self._lib.msr_set_blend_window(self._h, w.ctypes.data_as(C.c_void_p), w.shape[0])
        _lib.raise_for(self._lib, self._h, rc, "msr_set_blend_window")
        self.dem = self.img = None
        self.dem_padded = self.img_padded = None
        self.row0 = 0                                # first raster row of the arrays given to setImages
        self.canvas_row0 = 0                         # first canvas row of dem_padded / img_padded (padInputs)

    # ------------------------------------------------------------------------------------------------
    def _log(self, direction: str, nbytes: int, what: str) -> None:
        """One copy this class issues itself, for ``transfers``."""
        self.transfers.append((direction, int(nbytes), what))

    def _held(self, a, what: str):
        """A raster as this instance holds it: a float32 CUDA tensor on ``device`` (resident) or a float32 array."""
        if isinstance(a, torch.Tensor):
            if not a.is_cuda or a.dtype != torch.float32:
                raise ValueError("A raster given as a tensor must be a CUDA float32 tensor.")
            if self.resident:
                return a.to(self.device)
            self._log("d2h", a.numel() * 4, f"{what} raster")
            return a.cpu().numpy()
        a = np.asarray(a, np.float32)
        if not self.resident:
            return a
        self._log("h2d", a.size * 4, f"{what} raster")
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def setImages(self, img: np.ndarray, dem: np.ndarray, row0: int = 0,
                  full_shape: Optional[Tuple[int, int]] = None) -> None:
        """Stand-in for loadImages + preprocess (process_full_tiles.py:158-244): takes the arrays directly.

        With ``row0`` / ``full_shape`` the arrays are a ROW WINDOW: raster rows [row0, row0 + img.shape[0]) of a raster
        of ``full_shape`` (what a rank of a sharded run needs: distributed.input_rows).  ``dem_shape`` / ``img_shape``
        stay the full shape, so the tile list, the canvas geometry and the stitched map do not change; only padInputs
        allocates less, and a tile whose patches leave the window is an error (processTile).

        Arrays or CUDA float32 tensors.  They are held where ``resident`` says: with True an array is uploaded (once) and a
        tensor kept as it is; with False a tensor is downloaded and an array kept."""
        img, dem = (a if isinstance(a, torch.Tensor) else np.asarray(a, np.float32) for a in (img, dem))
        if tuple(img.shape) != tuple(dem.shape) or img.ndim != 2:
            raise ValueError("The ortho-image and the DEM must be 2-D arrays of the same shape.")
        full = tuple(int(v) for v in (dem.shape if full_shape is None else full_shape))
        row0 = int(row0)
        if len(full) != 2 or full[1] != dem.shape[1] or row0 < 0 or row0 + dem.shape[0] > full[0]:
            raise ValueError(f"rows [{row0}, {row0 + dem.shape[0]}) x {dem.shape[1]} columns are not a row window of a "
                             f"raster of shape {full}")
        self.img, self.dem = self._held(img, "ortho"), self._held(dem, "DEM")
        self.row0 = row0
        self.dem_shape = full
        self.img_shape = full

    @property
    def windowed(self) -> bool:
        """True when the host rasters held are a row window, not the whole raster."""
        return self.dem is not None and tuple(self.dem.shape) != tuple(self.dem_shape)

    def loadImages(self, rows: Optional[Tuple[int, int]] = None) -> None:
        """process_full_tiles.py:158-182 without GDAL: band 1 of ``<source_folder_path>/<ortho_image_name>`` and
        ``<dem_name>`` as float32 (geotiff.read_geotiff), georeferencing of the DEM kept for saveGTiff.
        ``rows=(r0, r1)`` reads only those raster rows of both files (only the strips / tiles that hold them are decoded)
        and sets them as a row window (setImages).  ``resident``: the device decoder's tensors are kept as they are; arrays
        decoded on the host are uploaded once.

        Raises ValueError if a path does not exist (same messages as the reference)."""
        from . import geotiff
        img_path = os.path.join(self.folder_path, self.left_image_name)
        dem_path = os.path.join(self.folder_path, self.dem_name)
        if not os.path.exists(img_path):
            raise ValueError("The path given for the ortho-image does not exist. Provided path is: " + img_path)
        if not os.path.exists(dem_path):
            raise ValueError("The path given for the dem does not exist. Provided path is: " + dem_path)
        # resident: the device decoder's tensor is kept (a host-decoded array is uploaded by setImages, once)
        how = dict(band=1, rows=rows, decoder=self.decoder, device=self.device, as_tensor=self.resident,
                   transfers=self.transfers)
        img, img_meta = geotiff.read_geotiff(img_path, **how)
        dem, self.geo_meta = geotiff.read_geotiff(dem_path, **how)
        self.geo_transform = geotiff.geotransform(self.geo_meta)
        if rows is None:
            self.setImages(img, dem)
        else:
            if img_meta["shape"] != self.geo_meta["shape"]:
                raise ValueError("The ortho-image and the DEM must be 2-D arrays of the same shape.")
            self.setImages(img, dem, row0=self.geo_meta["window"][0], full_shape=self.geo_meta["shape"])

    def saveGTiff(self, data: np.ndarray, data_type, name: str) -> None:
        """process_full_tiles.py:481-531 without GDAL: ``<save_path>/<map_name>_<name>.tiff``, LZW + PREDICTOR=2,
        the input DEM's georeferencing, nodata = no_value; uint8 data is stored as UInt16 like the reference does.

        ``data`` may be a CUDA tensor (``data_type`` its torch or the NumPy dtype): with ``encoder="device"`` it is converted
        and encoded where it lies, band by band (uint8 becomes uint16 on the device); with ``encoder="host"`` it is
        downloaded once.

        Raises ValueError for unsupported data types and for data that is not 2-dimensional."""
        from . import geotiff
        on_device = isinstance(data, torch.Tensor)
        if on_device:
            data_type = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int16: np.uint16}.get(data_type, data_type)
            if self.encoder == "host":
                self._log("d2h", data.numel() * data.element_size(), f"{name} product")
                data, on_device = data.cpu().numpy(), False
        if data_type == np.float32:
            out_type = np.float32
        elif data_type == np.uint8 or data_type == np.uint16:
            out_type = np.uint16
            if not on_device:                          # a tensor is widened band by band (geotiff._band_bytes_on_device)
                data = data.astype(np.uint16)
        else:
            raise ValueError("Unsupported data-type.")
        if len(data.shape) < 2:
            raise ValueError("Data is of incorrect shape. The array must be 2-dimensional at least.")
        if len(data.shape) == 3 and data.shape[2] == 1:
            data = data[:, :, 0]
        elif len(data.shape) != 2:
            raise ValueError("Data is of incorrect shape")
        geotiff.write_geotiff(self._product_path(name), data, getattr(self, "geo_meta", None), nodata=self.no_value,
                              dtype=out_type, compress="lzw", predictor=self._predictor(out_type), encoder=self.encoder,
                              device=self.device,
                              transfers=self.transfers, tile=self.product_tile, overviews=self.overviews,
                              layout=self.product_layout)

    def _predictor(self, dtype) -> int:
        """The predictor of a product file of ``dtype``: ``product_predictor`` for float32, 2 for the integer ``good``."""
        return self.product_predictor if np.dtype(dtype).kind == "f" else 2

    def _product_path(self, name: str) -> str:
        """``<save_path>/<map_name>_<name>.tiff``, its directory made."""
        os.makedirs(self.save_path, exist_ok=True)
        return os.path.join(self.save_path, self.map_name + "_" + name + ".tiff")

    def preprocess(self, swap_dsize: bool = True, rows: Optional[Tuple[int, int]] = None) -> None:
        """process_full_tiles.py:226-244: in-fill the ortho (stored in ``self.image`` and, as in the reference, never
        used afterwards), then replace ``self.dem`` by the synthesised low-resolution DEM (x1/4 area, in-fill, x1/4
        area, cubic back to full size).  Resamplers on the GPU; in-filling with SciPy on the host, or with ``infill="device"``
        (constructor) on the GPU: the same pixels, other values (preprocess.py, infill.py).

        ``swap_dsize=True`` keeps the reference's (rows, cols)-as-(width, height) argument of :241, so a non-square
        raster ends with a transposed-shape DEM and fails in padInputs exactly as the reference does; pass False to
        resize to the raster's own shape.

        ``rows=(r0, r1)``: synthesise only those raster rows, from the rows held (the whole raster, or a row window:
        setImages(row0=, full_shape=), loadImages(rows=)).  They must contain preprocess.window_plan(dem_shape, rows)["dem"]
        and [r0, r1) itself; a ValueError names the missing rows of the window otherwise.  Afterwards the instance holds
        the row window [r0, r1): ``dem`` = those rows of the whole raster's synthesised DEM, bit for bit, ``img`` = the same
        rows of the ortho as loaded, ``row0`` = r0, ``dem_shape`` unchanged — the state after setImages(row0=, full_shape=).
        ``self.image`` is set to None: the in-filled ortho, which the reference stores and never uses, is not computed for
        a window.  With ``swap_dsize=True`` a square raster gives the same rows as with False; a non-square one raises
        ValueError (the transposed result of :241 has no row windows, and the reference cannot run such a raster either).

        Without ``rows`` the whole raster is pre-processed, and with a row window set this raises ValueError."""
        from . import preprocess as pp
        if self.img is None or self.dem is None:
            raise ValueError("preprocess needs the rasters: call loadImages() or setImages() first.")
        if rows is not None:
            return self._preprocess_rows(pp, swap_dsize, (int(rows[0]), int(rows[1])))
        if self.windowed:
            raise ValueError(f"preprocess works on whole rasters: rows [{self.row0}, {self.row0 + self.dem.shape[0]}) of "
                             f"{self.dem_shape[0]} are set as a row window")
        self.image, self.dem = pp.preprocess(self._lib, self._h, self.device, self.img, self.dem, self.no_value,
                                             swap_dsize=swap_dsize, infill=self.infill, transfers=self.transfers)

    def _preprocess_rows(self, pp, swap_dsize: bool, rows: Tuple[int, int]) -> None:
        H, W = self.dem_shape
        if swap_dsize and H != W:
            raise ValueError(f"preprocess(rows=) on a {H} x {W} raster with swap_dsize=True: process_full_tiles.py:241 hands "
                             "(rows, cols) to cv2.resize as (width, height), so a non-square raster comes out transposed; "
                             "pass swap_dsize=False")
        r0, r1 = rows
        m0, m1 = pp.window_plan(self.dem_shape, rows)["dem"]
        have = (self.row0, self.row0 + self.dem.shape[0])
        need = (min(m0, r0), max(m1, r1))
        if need[0] < have[0] or need[1] > have[1]:
            missing = [f"[{a}, {b})" for a, b in ((need[0], min(need[1], have[0])), (max(need[0], have[1]), need[1])) if b > a]
            raise ValueError(f"preprocess(rows=({r0}, {r1})) reads raster rows [{need[0]}, {need[1]}); the row window "
                             f"[{have[0]}, {have[1]}) held lacks rows {' and '.join(missing)}")
        dem = pp.preprocess_rows(self._lib, self._h, self.device, self.dem, self.row0, self.dem_shape, rows, self.no_value,
                                 infill=self.infill, transfers=self.transfers)
        img = self.img[r0 - self.row0:r1 - self.row0]
        img = img.clone() if isinstance(img, torch.Tensor) else np.ascontiguousarray(img)   # the wider band is released
        self.setImages(img, dem, row0=r0, full_shape=self.dem_shape)
        self.image = None

    def processFiles(self, preprocess: bool = True, rank: int = 0, world: int = 1, mode: Optional[str] = None,
                     gather: bool = True, swap_dsize: bool = True, products: str = "gathered", **sharded) -> None:
        """processMap of the reference on files (process_full_tiles.py:568-587): loadImages -> preprocess ->
        padInputs -> tiles -> rebuildMap -> ``<map>_mean.tiff``, ``<map>_std.tiff``, ``<map>_good.tiff``.
        ``preprocess=False`` skips the low-resolution-DEM synthesis (feed an already pre-processed DEM); ``swap_dsize`` is
        preprocess()'s.

        ``mode="tiles"``: this process is ``rank`` of ``world`` of a tile-row-sharded run.  It reads the shape from the
        header (geotiff.read_info), decodes only the raster rows it needs (loadImages(rows=)) — the rows its tiles touch
        (distributed.input_rows), or with ``preprocess`` the band of input rows their synthesised DEM depends on
        (input_rows(preprocess=True)), which it pre-processes itself (preprocess(rows=)) — uploads only its tiles' rows,
        runs its tile rows (distributed.process_map_sharded) and, with ``gather`` (needs an initialised process group),
        all-gathers the finished rows; without it the rows of other ranks stay zero in the files written.
        ``mode="halo"`` is accepted by HaloShardedSuperResolution.processFiles only; further keywords (``batching``,
        ``accumulate``: halo.py) go to the sharded mode that takes them.

        ``products="rank0"`` (a sharded mode; needs an initialised process group when world > 1; ``gather`` is not looked
        at): no all-gather of the products.  Every rank encodes the strips of the product rows it computed, with the
        ``encoder`` set; the encoded strips are gathered to rank 0, which alone writes the three files — byte for byte those
        of a one-process run.  That needs every rank boundary to be a strip boundary of the float32 and of the uint16
        products (distributed.strip_plan): always so once a row exceeds 32 KiB.  Otherwise the run takes the gathered path,
        and only rank 0 writes.  ``products_path`` says which of the two ran.  The default, "gathered", is the all-gather
        after which every rank writes the files.  With ``mode="halo"`` (HaloShardedSuperResolution) rank boundaries follow
        patch rows, so the rank that owns a strip's first row first receives the strip's other rows from the rank above
        (distributed.halo_strip_plan, exchange_strip_rows); the files are those of the gathered halo run with the same ranks,
        and the fallback is taken only when a strip holds rows of three ranks."""
        if products not in ("gathered", "rank0"):
            raise ValueError(f"products must be 'gathered' or 'rank0', got {products!r}")
        if products == "rank0" and self.product_tile is not None:
            raise ValueError(f"products='rank0' writes strips only: product_tile={self.product_tile!r} needs "
                             "products='gathered'")
        del self.transfers[:]
        self.products_path = None
        if mode is not None:
            if products == "rank0":
                return self._process_files_rank0(preprocess, rank, world, mode, swap_dsize, **sharded)
            self.products_path = "gathered"
            mean, std, good = self._process_files_sharded(preprocess, rank, world, mode, gather, swap_dsize, **sharded)
        else:
            if products != "gathered":
                sharded = dict(sharded, products=products)
            if sharded:
                raise TypeError(f"processFiles: {sorted(sharded)} need a sharded mode")
            self.loadImages()
            if preprocess:
                self.preprocess(swap_dsize=swap_dsize)
            mean, std, good = self.processMap()
        for (name, _), data in zip(PRODUCTS, (mean, std, good)):
            self.saveGTiff(data, data.dtype, name)

    def _load_rank_rows(self, preprocess: bool, rank: int, world: int, mode: str, swap_dsize: bool = True
                        ) -> Tuple[int, int]:
        """read_info -> input_rows -> loadImages(rows=) [-> preprocess(rows=)]: the rows of both files that ``rank`` needs,
        nothing else.  Returns the rows held afterwards: input_rows(preprocess=False)."""
        from . import geotiff
        from .distributed import input_rows
        dem_path = os.path.join(self.folder_path, self.dem_name)
        if not os.path.exists(dem_path):
            raise ValueError("The path given for the dem does not exist. Provided path is: " + dem_path)
        shape = geotiff.read_info(dem_path)["shape"]
        geometry = (shape, self.image_size, self.stride, self.tile_size, rank, world, mode)
        r0, r1 = input_rows(*geometry)
        if r1 > r0 and preprocess:
            # the band the synthesis reads, and [r0, r1) itself for the ortho: the band can end up to two rows short of a
            # raster whose 4 * rint(H / 4) < H, rows that no resampler reads
            m0, m1 = input_rows(*geometry, preprocess=True)
            self.loadImages(rows=(min(m0, r0), max(m1, r1)))
            self.preprocess(swap_dsize=swap_dsize, rows=(r0, r1))
        elif r1 > r0:
            self.loadImages(rows=(r0, r1))
        else:                                         # a rank without work: no pixel is read
            self.geo_meta = geotiff.read_info(dem_path)
            self.geo_transform = geotiff.geotransform(self.geo_meta)
            empty = np.empty((0, shape[1]), np.float32)
            self.setImages(empty, empty, row0=0, full_shape=shape)
        return r0, r1

    def _process_files_sharded(self, preprocess: bool, rank: int, world: int, mode: str, gather: bool,
                               swap_dsize: bool = True):
        from .distributed import process_map_sharded
        if mode != "tiles":
            raise ValueError(f"DEMSuperResolution.processFiles shards by tile rows (mode='tiles'), got {mode!r}; the halo "
                             "mode is HaloShardedSuperResolution.processFiles")
        self._load_rank_rows(preprocess, rank, world, mode, swap_dsize)
        self.padInputs()
        return process_map_sharded(self.dem_shape, self.tile_size, self.generateTileList(), self.processTile, rank, world,
                                   gather=gather, device=self.device, as_tensor=self.resident, transfers=self.transfers)

    def _process_files_rank0(self, preprocess: bool, rank: int, world: int, mode: str, swap_dsize: bool = True,
                             **sharded) -> None:
        """processFiles(products="rank0"): see there.  The rank's rows never leave its device before they are encoded
        (``encoder="host"``: they are downloaded once, by saveGTiff's rule)."""
        from .distributed import process_map_sharded, strip_plan
        if mode != "tiles":
            raise ValueError(f"products='rank0' is built for mode='tiles', got mode={mode!r}")
        if sharded:
            raise TypeError(f"processFiles: mode='tiles' takes no {sorted(sharded)}")
        _need_process_group(world)
        self._load_rank_rows(preprocess, rank, world, mode, swap_dsize)
        shape, T = self.dem_shape, self.tile_size
        plans = {name: strip_plan(shape, np.dtype(dt).itemsize, T, world) for name, dt in PRODUCTS}
        local = world > 1 and not any(p["straddles"] for p in plans.values())
        self.products_path = "rank0" if local or world == 1 else "gathered"
        self.padInputs()
        tiles = self.generateTileList()
        if not local:
            # a strip straddles a rank boundary (a small raster): the gathered rows, written by rank 0 alone
            mean, std, good = process_map_sharded(shape, T, tiles, self.processTile, rank, world, gather=True,
                                                  device=self.device, as_tensor=self.resident, transfers=self.transfers)
            if rank == 0:
                for (name, _), data in zip(PRODUCTS, (mean, std, good)):
                    self.saveGTiff(data, data.dtype, name)
            return
        mine = process_map_sharded(shape, T, tiles, self.processTile, rank, world, device=self.device, as_tensor=True,
                                   local=True)
        for (name, _), data in zip(PRODUCTS, mine):
            r0, r1 = plans[name]["rows"][rank]
            assert tuple(data.shape) == (r1 - r0, shape[1]), (tuple(data.shape), (r0, r1), shape)
            self._encode_gather_write(name, data, plans[name], rank, world)

    def _encode_gather_write(self, name: str, data, plan: dict, rank: int, world: int) -> None:
        """The last steps of both rank-local writers: ``data`` holds the rows of this rank's strips ``plan["strips"][rank]`` of
        product ``name`` (a device tensor; distributed.strip_plan / halo_strip_plan).  They are encoded where ``encoder`` says
        (on the host after one download), the encoded strips are gathered to rank 0 (no process group with one rank), and
        rank 0 writes the file."""
        from . import geotiff
        shape = self.dem_shape
        dt = np.dtype(dict(PRODUCTS)[name])
        s0, s1 = plan["strips"][rank]
        if self.encoder == "host" and data.numel():
            self._log("d2h", data.numel() * data.element_size(), f"{name} product rows")
            data = data.cpu().numpy()
        strips = geotiff.encode_strips(data, dt, plan["rps"], predictor=self._predictor(dt), encoder=self.encoder,
                                       device=self.device, transfers=self.transfers) if data.shape[0] else []
        assert len(strips) == s1 - s0, (name, rank, len(strips), (s0, s1))
        if world > 1:
            import torch.distributed as dist
            gathered = [None] * world if rank == 0 else None
            dist.gather_object(strips, gathered, dst=0)
            if rank == 0:
                strips = [s for part in gathered for s in part]
        if rank == 0:
            assert len(strips) == plan["n_strips"], (len(strips), plan["n_strips"])
            geotiff.write_strips(self._product_path(name), strips, shape, dt, plan["rps"], getattr(self, "geo_meta", None),
                                 nodata=self.no_value, predictor=self._predictor(dt))

    def padInputs(self) -> None:
        """process_full_tiles.py:246-267: no_value canvas ((dim//1024)+1)*1024 + 2(S-s), data at offset (S-s).

        When the rasters set are a row window (setImages), only the canvas rows [c0, c1) those raster rows occupy are
        allocated (distributed.canvas_rows: a window that touches the raster's first / last row keeps the no_value margin
        above / below it).  ``canvas_row0`` = c0 and ``dem_window_shape`` = the tensors' shape; ``dem_padded_shape`` stays
        the full canvas.  The coordinates rule: the kernels that read the canvas (msr_patch_stats, msr_extract_patches,
        and msr_compact_patches' origins) see WINDOW rows, canvas row - c0; keys and everything downstream see canvas
        rows.  With the whole raster given, c0 = 0 and the tensors are the full canvas."""
        S, s = self.image_size, self.stride
        new_y, new_x = canvas_shape(self.dem_shape, S, s)
        self.pad_x = new_x - self.dem_shape[1] - (S - s)
        self.pad_y = new_y - self.dem_shape[0] - (S - s)
        n, w = self.dem.shape
        c0, c1 = canvas_rows(self.dem_shape, S, s, self.row0, self.row0 + n)
        with torch.cuda.device(self.device):
            self.dem_padded = torch.full((c1 - c0, new_x), self.no_value, dtype=torch.float32, device=self.device)
            self.img_padded = torch.full((c1 - c0, new_x), self.no_value, dtype=torch.float32, device=self.device)
            y = self.row0 + (S - s) - c0                           # the first raster row given, in window rows
            if isinstance(self.dem, torch.Tensor):                 # resident: device to device, on the current stream
                self.dem_padded[y:y + n, S - s:S - s + w] = self.dem
                self.img_padded[y:y + n, S - s:S - s + w] = self.img
            else:
                self._log("h2d", self.dem.size * 4, "DEM into its canvas")
                self.dem_padded[y:y + n, S - s:S - s + w] = torch.from_numpy(self.dem).to(self.device)
                self._log("h2d", self.img.size * 4, "ortho into its canvas")
                self.img_padded[y:y + n, S - s:S - s + w] = torch.from_numpy(self.img).to(self.device)
            torch.cuda.current_stream(self.device).synchronize()   # the tile loop reads the canvases on other streams
        self.canvas_row0 = c0
        self.dem_window_shape = self.img_window_shape = tuple(self.dem_padded.shape)
        self.dem_padded_shape = (new_y, new_x)
        self.img_padded_shape = (new_y, new_x)
        self.dem = None
        self.img = None

    def generateTileList(self) -> List[Tuple[int, int]]:
        """process_full_tiles.py:313-325 — (xx, yy), y outer; the unit tiles are sharded by across GPUs."""
        return tile_origins(self.dem_shape, self.tile_size)

    def _window(self) -> Tuple[int, int, int]:
        """(c0, rows, cols) of the canvas tensors: their first canvas row and their own shape — what the kernels that read
        them take.  Tensors a caller assigned to dem_padded / img_padded directly are a whole canvas (c0 = 0)."""
        rows, cols = self.dem_padded.shape
        full = tuple(self.dem_padded_shape) == (rows, cols)
        return (0 if full else self.canvas_row0), rows, cols

    def _check_rows(self, what: str, ys: Sequence[int]) -> None:
        """Every patch row at canvas origin y in ``ys`` reads canvas rows [y, y + S), clipped to the canvas (a patch that
        leaves the CANVAS is invalid, as ever: msr_patch_stats).  They must lie in the row window — unless they lie wholly in
        the no_value margin above or below the raster, where the patch is invalid with or without a window (the kernel sees
        an origin outside its rows and reads nothing)."""
        c0, rows, _ = self._window()
        if c0 == 0 and rows == self.dem_padded_shape[0]:
            return
        halo = self.image_size - self.stride
        for y in ys:
            lo, hi = y, min(y + self.image_size, self.dem_padded_shape[0])
            if not (c0 <= lo and hi <= c0 + rows) and not (hi <= halo or lo >= halo + self.dem_shape[0]):
                raise ValueError(f"{what}: the patch row at {y} reads canvas rows [{lo}, {hi}), outside the row window "
                                 f"[{c0}, {c0 + rows}) this instance holds")

    # ------------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _make_pipeline(self) -> None:
        """`pipeline` generator handles with the same weights, each with its own stream (built once, at construction
        when the model is a Generator).

        HIP binds a stream to a hardware queue at its first use, in order, and queues whose ids are equal modulo 4
        share a dispatch pipe; when two of the four busy streams of a two-handle pipeline (two call streams, two
        auxiliary streams) share one, the pipeline runs ~9 % slower instead of ~5 % faster than one stream
        (profiles/r02_raster_queue_pairing.txt).  So the call streams are used once here and the handles are planned
        right after them: four consecutive queue ids."""
        self._gens = [self._gen] + [self._gen.clone() for _ in range(self.pipeline - 1)]
        with torch.cuda.device(self.device):
            self._pstreams = [torch.cuda.Stream(self.device) for _ in self._gens]
            for st in self._pstreams:
                with torch.cuda.stream(st):
                    torch.zeros(1, device=self.device)
            for g in self._gens:
                g.prepare()
            torch.cuda.synchronize(self.device)

    @property
    def counter_noise(self) -> bool:
        """True when the model is a Generator with sampler="counter": the loops then name every row's noise (noise_ids)."""
        return self._gen is not None and getattr(self._gen, "sampler", "torch") == "counter"

    def patchOrigins(self, px: int, py: int) -> np.ndarray:
        """[n, 2] int32 (xx, yy) in padded coordinates, generation order (process_full_tiles.py:453-454)."""
        S, s, T = self.image_size, self.stride, self.tile_size
        ys = np.array(patch_origins_1d(py, S, s, T), dtype=np.int32)
        xs = np.array(patch_origins_1d(px, S, s, T), dtype=np.int32)
        return np.stack([np.tile(xs, len(ys)), np.repeat(ys, len(xs))], axis=1)

    # -- the batching sequence of both modes (halo.py: _generate_rows): compaction, then per call extract + generate.  The
    # streams, waits, events and record_stream calls around it are the caller's: there the modes differ, and speed is decided
    def _cap(self, n: int) -> int:
        """Rows of the compaction outputs for n candidates: whole calls of B, at least one."""
        return max(1, -(-n // self.batch_size)) * self.batch_size

    def _compact_patches(self, ox: torch.Tensor, oy: torch.Tensor, tile_x: int, tile_y: int,
                         carry: Optional[dict] = None) -> dict:
        """On torch's current stream: getPatch's validity test and normalize's reductions for the candidates at (ox, oy),
        generation order (msr_patch_stats), then the batch assembly of process_full_tiles.py:455-474 on the device
        (msr_compact_patches).  Origins and ``tile_y`` are WINDOW rows (padInputs); the keys, origin - (tile_x, tile_y), come
        out as in the full canvas.  ``carry`` (halo.py, batching="rank"): {"n": rows carried over, and those rows of the five
        outputs}; they are copied to the front and the compaction starts behind them (msr_compact_patches_carry).
        ``meta`` = {valid patches, carried ones included; calls} stays on the device: how the host gets it is the caller's."""
        lib, h, dev = self._lib, self._h, self.device
        _, rows, cols = self._window()
        n = int(ox.numel())
        carry_n = 0 if carry is None else carry["n"]
        cap = self._cap(carry_n + n)
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        valid = torch.empty(n, dtype=torch.uint8, device=dev)
        minmax = torch.empty((n, 4), **f32)
        st = dict(n=n, cap=cap, keep=(ox, oy, valid, minmax), sx=torch.empty(cap, **i32), sy=torch.empty(cap, **i32),
                  mm_sel=torch.empty((cap, 4), **f32), keys=torch.empty((cap, 2), **i32), dmm=torch.empty((cap, 2), **f32),
                  meta=torch.empty(2, **i32))
        stream = self._stream()
        rc = lib.msr_patch_stats(h, self.img_padded.data_ptr(), self.dem_padded.data_ptr(), rows, cols, ox.data_ptr(),
                                 oy.data_ptr(), n, self.no_value, valid.data_ptr(), minmax.data_ptr(), stream)
        _lib.raise_for(lib, h, rc, "msr_patch_stats")
        args = (h, valid.data_ptr(), ox.data_ptr(), oy.data_ptr(), minmax.data_ptr(), n, tile_x, tile_y, self.batch_size, cap)
        outs = tuple(st[name].data_ptr() for name in _CARRIED) + (st["meta"].data_ptr(), stream)
        if carry is None:
            rc = lib.msr_compact_patches(*args, *outs)
            _lib.raise_for(lib, h, rc, "msr_compact_patches")
        else:
            for name in _CARRIED if carry_n else ():
                st[name][:carry_n].copy_(carry[name])               # the earlier band's tail, device to device
            rc = lib.msr_compact_patches_carry(*args, carry_n, *outs)
            _lib.raise_for(lib, h, rc, "msr_compact_patches_carry")
        return st

    def _extract_batch(self, st: dict, c: int, batch: torch.Tensor) -> None:
        """On torch's current stream: the B patches of call ``c`` of the compacted list ``st``, normalised, into ``batch``
        [B, S, S, 2] (msr_extract_patches; rows behind the last valid patch are zero patches)."""
        B = self.batch_size
        _, rows, cols = self._window()                # sx / sy are window origins already (_compact_patches)
        rc = self._lib.msr_extract_patches(self._h, self.img_padded.data_ptr(), self.dem_padded.data_ptr(), rows, cols,
                                           st["sx"][c * B:].data_ptr(), st["sy"][c * B:].data_ptr(),
                                           st["mm_sel"][c * B:].data_ptr(), B, batch.data_ptr(), self._stream())
        _lib.raise_for(self._lib, self._h, rc, "msr_extract_patches")

    def _ready_pipeline(self) -> None:
        """Before a tile's or band's calls: the handles exist (close() drops them); clones follow a load() on the base one."""
        if self._gens is None:
            self._make_pipeline()
        for g in self._gens[1:]:
            if g.weights_version != self._gen.weights_version:
                g.load(self._gen._weights)
                g.weights_version = self._gen.weights_version

    def _generator_calls(self, st: dict, ncall: int, preds: torch.Tensor, batches: Sequence[torch.Tensor],
                         ids: Optional[torch.Tensor] = None, gated: bool = False) -> None:
        """The first ``ncall`` calls of the compacted list ``st``.  They are independent batches: they alternate over the
        pipeline's handles, each on its own stream, so that the low-occupancy head of one call overlaps the tail of the other.
        Call c extracts into ``batches[c % handles]`` and writes ``preds[c * B:(c + 1) * B]``: patches never leave HBM.
        ``ids`` [cap, 3]: every row's noise id (sampler="counter").  ``gated``: the matrix-bound part of a call waits for the
        event the previous call recorded (forward_device).  The first call's handle takes the range scan (range_check)."""
        B = self.batch_size
        for c in range(ncall):
            k = c % len(self._gens)
            with torch.cuda.stream(self._pstreams[k]):
                self._extract_batch(st, c, batches[k])
                self._gens[k].forward_device(batches[k], out=preds[c * B:(c + 1) * B].unsqueeze(-1),
                                             gate=self._gate if gated else None,
                                             noise_ids=None if ids is None else ids[c * B:(c + 1) * B])
                if c == 0:
                    self._range_enqueue(self._gens[k])
                if gated:
                    self._gate_ring = (self._gate_ring + 1) % len(self._gate_events)
                    self._gate = self._gate_events[self._gate_ring]
                    self._gate.record(self._pstreams[k])

    def _host_model_calls(self, st: dict, ncall: int, preds: torch.Tensor) -> None:
        """_generator_calls for a host callable, on the current stream: a stage on the host, resident or not, whose round trip
        per call ``transfers`` lists."""
        S, B = self.image_size, self.batch_size
        batch = torch.empty((B, S, S, 2), dtype=torch.float32, device=self.device)
        for c in range(ncall):
            self._extract_batch(st, c, batch)
            self._log("d2h", batch.numel() * 4, "batch for the host model")
            out = np.array(self.model(batch.cpu().numpy(), training=False))[:, :, :, -1]
            self._log("h2d", out.size * 4, "predictions of the host model")
            preds[c * B:(c + 1) * B] = torch.from_numpy(np.ascontiguousarray(out, dtype=np.float32)).to(self.device)

    # -- one tile = prepare (validity, min/max, device-side batch assembly) -> generate -> stitch -------------------
    def _prepare_tile(self, px: int, py: int):
        """Asynchronous first half of processTile on the handle's preparation stream: the tile's candidate patches and
        their compaction into calls (_compact_patches).  The host gets back two integers {valid patches, calls} through
        pinned memory, behind an event — it fetches them while the GPU is still busy with the previous tile
        (processTiles), so no flag array crosses PCIe and no host-side compaction exists."""
        S, s, T = self.image_size, self.stride, self.tile_size
        dev = self.device
        if self._prep_stream is None:
            self._prep_stream = torch.cuda.Stream(dev)
        # The padded rasters are produced on the caller's stream (padInputs, or tensors the caller built): the preparation
        # stream must not read them before that work is done.  Once per raster pair — waiting on every tile would put
        # tile t + 1's preparation behind tile t's generator calls and undo the pipelining.
        token = (self.img_padded.data_ptr(), self.dem_padded.data_ptr(), getattr(self.img_padded, "_version", 0),
                 getattr(self.dem_padded, "_version", 0))
        if getattr(self, "_raster_token", None) != token:
            self._prep_stream.wait_stream(torch.cuda.current_stream(dev))
            self._raster_token = token
        c0 = self._window()[0]
        rx, ry = patch_origins_1d(px, S, s, T), patch_origins_1d(py, S, s, T)
        self._check_rows(f"tile ({px}, {py})", ry)
        st = {"px": px, "py": py}
        with torch.cuda.device(dev), torch.cuda.stream(self._prep_stream):
            xs = torch.arange(rx.start, rx.stop, rx.step, dtype=torch.int32, device=dev)
            ys = torch.arange(ry.start - c0, ry.stop - c0, ry.step, dtype=torch.int32, device=dev)   # window rows
            ox = xs.repeat(ys.numel())                      # generation order: y outer, x inner (:453-454)
            oy = ys.repeat_interleave(xs.numel())
            if self.counter_noise:
                # Row d of the tile's compacted list draws the noise (d, px, py), padding rows of the last call included: the
                # id names the tile (canvas coordinates) and the position in its compaction, nothing of this rank or run.
                cap = self._cap(int(ox.numel()))
                ids = torch.empty((cap, 3), dtype=torch.int32, device=dev)
                ids[:, 0] = torch.arange(cap, dtype=torch.int32, device=dev)
                ids[:, 1] = px
                ids[:, 2] = py
                st["noise_ids"] = ids
            st.update(self._compact_patches(ox, oy, px, py - c0))   # tile_y in window rows too
            meta_host = torch.empty(2, dtype=torch.int32, pin_memory=True)
            meta_host.copy_(st["meta"], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._prep_stream)
        st.update(meta_host=meta_host, event=ev)
        return st

    def _generate_tile(self, st):
        """Second half of processTile: the tile's generator calls (batches cut from the compacted origins, the last
        one zero-padded) and the stitcher, all on the current stream / the pipeline streams."""
        S, B = self.image_size, self.batch_size
        dev = self.device
        st["event"].synchronize()                     # 8 bytes; the GPU keeps working on what is already queued
        self._range_retire()                          # the previous tile's scan (range_check), read at the same point
        nv, ncall = (int(v) for v in st["meta_host"].tolist())
        sx, sy, mm_sel = st["sx"], st["sy"], st["mm_sel"]
        ids = st.get("noise_ids")                     # sampler="counter" only; None leaves every call as it always was
        self._last = (st["keys"], nv, ncall)
        self._last_calls = None
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            for t in (sx, sy, mm_sel, st["keys"], st["dmm"]):
                t.record_stream(cur)
            if self._gen is not None:
                # The calls go to one of two persistent buffers (no allocation per tile — a fresh 0.5 GB hipMalloc drains the
                # device), and the generator streams wait only for the events they need (this tile's preparation; the stitcher
                # pass that last read this buffer, two tiles ago), so tile t+1 starts generating while tile t is stitched.
                self._ready_pipeline()
                buf = self._tile_buffers(st["cap"])
                for ps in self._pstreams:
                    ps.wait_event(st["event"])
                    if buf["free"] is not None:
                        ps.wait_event(buf["free"])
                    for t in (sx, sy, mm_sel) + (() if ids is None else (ids,)):
                        t.record_stream(ps)
                self._generator_calls(st, ncall, buf["preds"], self._batches, ids, self.gated and len(self._gens) > 1)
                for ps in self._pstreams:
                    cur.wait_stream(ps)
                cur.wait_event(st["event"])
                out = self.rebuildTile(buf["preds"], st["keys"], st["dmm"], nv)
                buf["free"] = torch.cuda.Event()
                buf["free"].record(cur)
                return out
            cur.wait_event(st["event"])
            preds = torch.empty((max(ncall * B, 1), S, S), dtype=torch.float32, device=dev)
            self._host_model_calls(st, ncall, preds)
            return self.rebuildTile(preds, st["keys"], st["dmm"], nv)

    # -- range_check: one scan per tile, read one tile late -------------------------------------------------------------
    def _range_enqueue(self, gen) -> None:
        """After the first generator call of a tile, on that call's stream (the current one): scan its activations."""
        if self.range_check == "off":
            return
        gen.range_scan_async()
        self._range_pending = gen

    def _range_retire(self) -> None:
        """Read the outstanding scan, if any, and act on its regime."""
        gen, self._range_pending = self._range_pending, None
        if gen is None:
            return
        report = gen.range_read()
        if self.range_report is None or self.range_report.regime == "parity":
            self.range_report = report
        if report.regime == "parity":
            return
        if self.range_check == "raise":
            raise RuntimeError(f"range_check: {report}")
        if not self._range_warned:
            import warnings
            self._range_warned = True
            warnings.warn(f"range_check: {report}; the f16c family is outside its parity regime for these weights: use "
                          "precision='bf16x3' or precision='auto'", RuntimeWarning, stacklevel=2)

    def _tile_buffers(self, cap: int):
        """Two persistent prediction buffers [cap, S, S] used by alternate tiles, and one input batch per handle."""
        S, B = self.image_size, self.batch_size
        if self._bufs is None or self._bufs[0]["preds"].shape[0] < cap:
            self._bufs = [{"preds": torch.empty((cap, S, S), dtype=torch.float32, device=self.device), "free": None}
                          for _ in range(2)]
            self._batches = [torch.empty((B, S, S, 2), dtype=torch.float32, device=self.device) for _ in self._gens]
            self._buf_turn = 0
        self._buf_turn ^= 1
        return self._bufs[self._buf_turn]

    def processTile(self, px: int, py: int):
        """process_full_tiles.py:431-479 without the disk write: returns (mean, std, good) device tensors [T,T].

        ``self.last_calls`` gives the patch keys of every generator call of the tile (with (-1,-1) padding
        entries), i.e. the batch composition the reference would have produced; ``self.last_counts`` the
        (valid patches, calls) pair without a read-back."""
        return self._generate_tile(self._prepare_tile(px, py))

    @property
    def last_counts(self) -> Tuple[int, int]:
        return self._last[1], self._last[2]

    @property
    def last_calls(self):
        if self._last_calls is None:
            keys, nv, ncall = self._last
            B = self.batch_size
            k = keys[:ncall * B].cpu().numpy()
            self._last_calls = [[tuple(int(v) for v in kk) for kk in k[c * B:(c + 1) * B]] for c in range(ncall)]
        return self._last_calls

    def rebuildTile(self, preds: torch.Tensor, keys: torch.Tensor, dem_minmax: torch.Tensor, n: Optional[int] = None):
        """process_full_tiles.py:363-414 on the GPU.  preds [n,S,S] raw generator outputs (the +0.5 of :340 is
        applied inside), keys [n,2] int32 (x,y) relative to the tile, dem_minmax [n,2].  Generation order."""
        T = self.tile_size
        n = int(keys.shape[0]) if n is None else n
        with torch.cuda.device(self.device):
            mean = torch.empty((T, T), dtype=torch.float32, device=self.device)
            std = torch.empty((T, T), dtype=torch.float32, device=self.device)
            good = torch.empty((T, T), dtype=torch.uint8, device=self.device)
            rc = self._lib.msr_stitch_tile(self._h, preds.data_ptr(), keys.data_ptr(), dem_minmax.data_ptr(), n, T,
                                           self.stride, self.no_value, 1 if self.as_implemented else 0,
                                           mean.data_ptr(), std.data_ptr(), good.data_ptr(), self._stream())
            _lib.raise_for(self._lib, self._h, rc, "msr_stitch_tile")
        return mean, std, good

    # ------------------------------------------------------------------------------------------------
    def iterTiles(self, tiles: Sequence[Tuple[int, int]]):
        """Yield ((xx, yy), (mean, std, good) device tensors) for every tile, software-pipelined: the preparation of
        tile t+1 (validity, min/max, device-side batch assembly — a few small kernels on their own stream) is queued
        before the host waits for tile t's two counts, so that wait ends while the GPU is still generating tile t-1
        and the generator stream never drains between tiles (the reference is serial: process_full_tiles.py:453-478)."""
        tiles = list(tiles)
        if not tiles:
            return
        self._range_warned = False                    # one warning per run
        nxt = self._prepare_tile(*tiles[0])
        for i, (xx, yy) in enumerate(tiles):
            st = nxt
            nxt = self._prepare_tile(*tiles[i + 1]) if i + 1 < len(tiles) else None
            yield (xx, yy), self._generate_tile(st)
        self._range_retire()                          # the last tile's scan

    def processTiles(self, tiles: Sequence[Tuple[int, int]]):
        """Process a list of tiles (this rank's shard); returns {(xx,yy): (mean, std, good)} of host arrays.
        Results come back through pinned buffers with asynchronous copies retired two tiles late, so the device-to-host
        transfer of tile t never stalls the launches of tile t+1.

        ``resident``: the values are the device tensors themselves (no download); they are written on the current stream,
        after the generator streams (_generate_tile), so work queued on it later sees them whole."""
        if self.resident:
            return dict(self.iterTiles(tiles))
        out = {}
        pending = []

        def retire(item):
            key, ev, bufs = item
            ev.synchronize()
            out[key] = tuple(np.array(b.numpy()) for b in bufs)

        for key, (m, s, g) in self.iterTiles(tiles):
            with torch.cuda.device(self.device):
                bufs = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (m, s, g)]
                for b, t in zip(bufs, (m, s, g)):
                    b.copy_(t, non_blocking=True)
                    self._log("d2h", t.numel() * t.element_size(), f"tile {key} product")
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
            pending.append((key, ev, bufs, (m, s, g)))
            while len(pending) > 2:
                retire(pending.pop(0)[:3])
        for item in pending:
            retire(item[:3])
        return out

    def rebuildMap(self, tiles: dict):
        """process_full_tiles.py:533-566 without file I/O: paste tiles, crop to the input extent.  Device tensors in,
        device tensors out (``resident``: processTiles gives them)."""
        if self.resident or any(isinstance(m, torch.Tensor) for m, _, _ in tiles.values()):
            maps = self._device_maps()
            for key, parts in tiles.items():
                self._paste(maps, key, parts)
            return maps
        hp, wp = self.dem_padded_shape
        T = self.tile_size
        mean = np.zeros((hp, wp), np.float32)
        std = np.zeros((hp, wp), np.float32)
        good = np.zeros((hp, wp), np.uint8)
        for (xx, yy), (m, s, g) in tiles.items():
            mean[yy:yy + T, xx:xx + T] = m
            std[yy:yy + T, xx:xx + T] = s
            good[yy:yy + T, xx:xx + T] = g
        h, w = self.dem_shape
        return mean[:h, :w], std[:h, :w], good[:h, :w]

    def processMap(self, img: Optional[np.ndarray] = None, dem: Optional[np.ndarray] = None):
        """process_full_tiles.py:568-587 on arrays: pad, tile, generate, stitch, assemble."""
        if img is not None:
            self.setImages(img, dem)
        self.padInputs()
        return self.mapTiles(self.generateTileList())

    def mapTiles(self, tiles: Sequence[Tuple[int, int]]):
        """processTiles + rebuildMap for the canvases padInputs built.  ``resident``: every tile is pasted into the device
        maps as iterTiles yields it, so one tile's products are alive at a time, not the whole list's."""
        if not self.resident:
            return self.rebuildMap(self.processTiles(tiles))
        maps = self._device_maps()
        for key, parts in self.iterTiles(tiles):
            self._paste(maps, key, parts)
        return maps

    def _device_maps(self):
        """Zeroed (mean, std, good) of ``dem_shape`` on the device: what rebuildMap's crop of the padded canvas keeps."""
        h, w = self.dem_shape
        with torch.cuda.device(self.device):
            return (torch.zeros((h, w), dtype=torch.float32, device=self.device),
                    torch.zeros((h, w), dtype=torch.float32, device=self.device),
                    torch.zeros((h, w), dtype=torch.uint8, device=self.device))

    def _paste(self, maps, key: Tuple[int, int], parts) -> None:
        """One tile into the device maps, clipped to them, on the current stream: the stream rebuildTile wrote the tile on
        (and on which its tensors were allocated), so no event and no record_stream is needed and the tile loop's pipeline
        is as deep as ever."""
        xx, yy = key
        h, w = maps[0].shape
        th, tw = min(self.tile_size, h - yy), min(self.tile_size, w - xx)
        if th <= 0 or tw <= 0:
            return
        with torch.cuda.device(self.device):
            for full, t in zip(maps, parts):
                full[yy:yy + th, xx:xx + tw] = t[:th, :tw]

    def close(self) -> None:
        for g in (getattr(self, "_gens", None) or [])[1:]:
            g.close()
        self._gens = None
        if getattr(self, "_own_handle", False) and self._h:
            self._lib.msr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

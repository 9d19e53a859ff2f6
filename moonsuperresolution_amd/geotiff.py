"""GeoTIFF raster I/O without GDAL — the data format either side of the hot path.

The reference reads band 1 of ``run-DRG.tif`` / ``run-DEM.tif`` with GDAL as float32 and keeps the geotransform and
projection (``loadImages``, process_full_tiles.py:158-182), and writes ``<map>_mean.tiff`` / ``_std.tiff`` (Float32)
and ``_good.tiff`` (UInt16) as LZW GeoTIFFs with ``PREDICTOR=2`` and a nodata tag (``saveGTiff``, :481-531).

``read_geotiff`` / ``write_geotiff`` do the same on the TIFF 6.0 / BigTIFF container directly:

* read: classic TIFF and BigTIFF, either byte order, strips or tiles, compression none / LZW / Deflate / PackBits,
  predictor 1 / 2 / 3, 8/16/32/64-bit (un)signed integer and IEEE float samples, chunky or planar multi-band files
  (band 1 is returned, like the reference); the result is float32.
  ``rows=(r0, r1)`` reads a row window and decodes only the strips / tiles that intersect it; ``read_info`` returns the
  metadata (shape included) from the header alone — what a rank of a sharded run needs to read only its own rows.
  The blocks are decoded on the host (default) or, ``decoder="device"``, LZW files on the GPU (csrc/geotiff_codec.hip:
  LZW per block, then predictor, conversion and placement) with the same bits out.
* write: single band, little-endian, LZW + horizontal predictor (or none / deflate; ``predictor=3``: the floating-point
  predictor for float samples, fp_predictor_reference), classic TIFF or BigTIFF chosen by size, in blocks that are strips of whole rows (default) or, ``tile=(tile_h, tile_w)``, zero-padded tiles; with tiles,
  ``overviews=n`` adds n reduced-resolution levels as chained IFDs (GDAL's internal-overview layout), each the 2 x 2
  reduction ``overview_reference`` of the one before.  The blocks of either layout are differenced and encoded one by one
  on the host (default; _encode_block) or, ``encoder="device"``, band by band on the GPU (_encode_band_device:
  csrc/geotiff_codec.hip, the levels reduced by csrc/tiff_overview.hip) with the same bytes out; ``layout="cog"`` puts the
  tiles and IFDs of such a file in the order of a cloud-optimised GeoTIFF (IFDs first, coarse levels before fine ones, every
  tile framed by its length), and its device encoder reads the tiles where their level lies (_device_levels_in_place); one
  container writer (_write_container) puts either layout into the file, with the GDAL_NODATA tag and the GeoTIFF georeferencing tags of the
  input **passed through verbatim** (ModelPixelScale 33550, ModelTiepoint 33922, ModelTransformation 34264,
  GeoKeyDirectory 34735, GeoDoubleParams 34736, GeoAsciiParams 34737, GDAL_METADATA 42112) — the output keeps the
  input's geotransform and projection byte for byte, which is what ``saveGTiff`` does with ``SetGeoTransform`` /
  ``SetProjection``.

The LZW codec lives in libmoonsr_hip.so's host code (csrc/host_codecs.cpp).  GDAL is absent here, so the codec and
container are validated against an independent implementation instead: PIL/libtiff reads what this module writes
and this module reads what PIL/libtiff writes (tests/test_geotiff.py).
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

from . import _lib

GEO_TAGS = (33550, 33922, 34264, 34735, 34736, 34737, 42112)
GDAL_NODATA = 42113
_TYPE_FMT = {1: "B", 2: "c", 3: "H", 4: "I", 5: "II", 6: "b", 7: "B", 8: "h", 9: "i", 10: "ii", 11: "f", 12: "d",
             16: "Q", 17: "q", 18: "Q"}
_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 16: 8, 17: 8, 18: 8}


# ---- codecs ----------------------------------------------------------------------------------------------------------
def lzw_decode(data: bytes, out_size: int) -> np.ndarray:
    lib = _lib.load()
    src = np.frombuffer(data, np.uint8)
    out = np.empty(max(out_size, 1), np.uint8)
    n = lib.msr_lzw_decode(src.ctypes.data, src.size, out.ctypes.data, out_size)
    if n < 0:
        raise ValueError("malformed LZW stream")
    if n < out_size:
        out[n:out_size] = 0
    return out[:out_size]


def lzw_encode(data: np.ndarray) -> bytes:
    lib = _lib.load()
    src = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    out = np.empty(src.size + src.size // 2 + 1024, np.uint8)
    n = lib.msr_lzw_encode(src.ctypes.data, src.size, out.ctypes.data, out.size)
    if n < 0:
        raise ValueError("LZW encode failed")
    return out[:n].tobytes()


def _packbits_decode(data: bytes, out_size: int) -> np.ndarray:
    out = bytearray()
    i = 0
    while i < len(data) and len(out) < out_size:
        n = data[i] if data[i] < 128 else data[i] - 256
        i += 1
        if n >= 0:
            out += data[i:i + n + 1]
            i += n + 1
        elif n != -128:
            out += bytes([data[i]]) * (1 - n)
            i += 1
    return np.frombuffer(bytes(out[:out_size]).ljust(out_size, b"\0"), np.uint8)


# ---- reading ------------------------------------------------------------------------------------------------------------
def _read_ifd(buf: bytes, big: bool, bo: str, off: int) -> Dict[int, Tuple[int, int, bytes]]:
    """tag -> (type, count, raw value bytes) of the IFD at ``off``."""
    if big:
        n = struct.unpack_from(bo + "Q", buf, off)[0]
        pos, esz, vsz = off + 8, 20, 8
    else:
        n = struct.unpack_from(bo + "H", buf, off)[0]
        pos, esz, vsz = off + 2, 12, 4
    tags = {}
    for i in range(n):
        e = pos + i * esz
        tag, typ = struct.unpack_from(bo + "HH", buf, e)
        cnt = struct.unpack_from(bo + ("Q" if big else "I"), buf, e + 4)[0]
        size = _TYPE_SIZE.get(typ, 1) * cnt
        voff = e + 4 + vsz
        if size > vsz:
            voff = struct.unpack_from(bo + ("Q" if big else "I"), buf, voff)[0]
        tags[tag] = (typ, cnt, bytes(buf[voff:voff + size]))
    return tags


def _values(entry, bo: str):
    typ, cnt, raw = entry
    if typ == 2:
        return raw
    return struct.unpack(bo + _TYPE_FMT[typ] * cnt, raw)


def _next_ifd(buf, big: bool, bo: str, off: int) -> int:
    """The next-IFD pointer of the IFD at ``off`` (0: the chain ends)."""
    if big:
        n = struct.unpack_from(bo + "Q", buf, off)[0]
        return struct.unpack_from(bo + "Q", buf, off + 8 + 20 * n)[0]
    n = struct.unpack_from(bo + "H", buf, off)[0]
    return struct.unpack_from(bo + "I", buf, off + 2 + 12 * n)[0]


def _overview_ifds(buf, big: bool, bo: str, first: int) -> list:
    """The tag dicts of the reduced-resolution levels: the IFDs chained behind the first one whose NewSubfileType (254)
    has bit 0 set, in file order.  A chain that loops or leaves the file ends where it does."""
    out, seen, off = [], {first}, _next_ifd(buf, big, bo, first)
    while off and off not in seen and off + 8 <= buf.size:
        seen.add(off)
        t = _read_ifd(buf, big, bo, off)
        if 254 in t and _values(t[254], bo)[0] & 1:
            out.append(t)
        off = _next_ifd(buf, big, bo, off)
    return out


def _header(path: str):
    """(memory map, BigTIFF or not, byte order, offset of the first IFD) of a TIFF file."""
    buf = np.memmap(path, dtype=np.uint8, mode="r")
    head = bytes(buf[:16])
    if head[:2] not in (b"II", b"MM"):
        raise ValueError(f"{path}: not a TIFF file")
    bo = "<" if head[:2] == b"II" else ">"
    magic = struct.unpack_from(bo + "H", head, 2)[0]
    if magic not in (42, 43):
        raise ValueError(f"{path}: not a TIFF file (magic {magic})")
    big = magic == 43
    return buf, big, bo, struct.unpack_from(bo + ("Q" if big else "I"), head, 8 if big else 4)[0]


def _open(path: str, overview: int = 0):
    """Header and first IFD of a (Geo)TIFF: (memory map, tag dict, byte order, meta).  No pixel block is touched.
    ``overview=k > 0``: the IFD of the k-th reduced-resolution level instead (read_geotiff)."""
    buf, big, bo, ifd = _header(path)
    t = _read_ifd(buf, big, bo, ifd)
    if overview:
        levels = _overview_ifds(buf, big, bo, ifd)
        if overview > len(levels):
            raise ValueError(f"{path}: overview {overview} does not exist: the file has {len(levels)} reduced level(s)")
        t = levels[overview - 1]

    def val(tag, default=None):
        return _values(t[tag], bo) if tag in t else default

    cols, rows = val(256)[0], val(257)[0]
    bps = val(258, (1,))[0]
    fmt = val(339, (1,))[0]
    kind = {1: "u", 2: "i", 3: "f"}.get(fmt)
    if kind is None or bps not in (8, 16, 32, 64) or (kind == "f" and bps < 32):
        raise ValueError(f"{path}: unsupported sample format {fmt} / {bps} bits")
    dt = np.dtype(f"{bo}{kind}{bps // 8}")
    nodata = None
    if GDAL_NODATA in t:
        try:
            nodata = float(t[GDAL_NODATA][2].split(b"\0")[0].decode())
        except ValueError:
            nodata = None
    meta = {"geo": {k: t[k] for k in GEO_TAGS if k in t}, "nodata": nodata, "dtype": dt.newbyteorder("="),
            "shape": (rows, cols), "byteorder": bo, "window": (0, rows)}
    if overview:
        meta["overview"] = overview
    return buf, t, bo, meta


def read_info(path: str) -> dict:
    """The ``meta`` of ``read_geotiff`` (shape, dtype, nodata, georeferencing; ``window`` = the whole raster) from the
    header alone: no strip or tile is decoded.  A rank needs the shape before it can choose its row window."""
    return _open(path)[3]


def overview_shapes(path: str) -> list:
    """``[(rows, cols), ...]`` of the reduced-resolution levels of a file (write_geotiff(overviews=)), level 1 first, from
    the IFDs alone; ``[]`` for a file without any.  ``read_geotiff(overview=k)`` reads level k."""
    buf, big, bo, first = _header(path)
    return [(_values(t[257], bo)[0], _values(t[256], bo)[0]) for t in _overview_ifds(buf, big, bo, first)]


class _Blocks(NamedTuple):
    """Where the blocks (strips or tiles) that hold one band of an IFD lie, and what is in them: what both readers need."""
    bw: int                 # block width and height in pixels (a strip: the raster's width; the last strip may be shorter)
    bh: int
    across: int             # blocks in a row of blocks, and rows of blocks
    down: int
    tiled: bool
    offs: tuple             # file offset and byte count of every block of the IFD
    cnts: tuple
    plane0: int             # index of the band's first block (a planar file: of its plane)
    ch: int                 # the band's sample among the ``spp`` samples of a block pixel (a chunky file: every band's)
    spp: int
    dt: np.dtype            # the samples as stored, in the file's byte order; their width in bytes and kind "u" / "i" / "f"
    sb: int
    kind: str
    pred: int               # Predictor and Compression tags
    comp: int
    rows: int               # the raster
    cols: int


def _block_geometry(t: dict, bo: str, meta: dict, band: int) -> _Blocks:
    """The _Blocks of band ``band`` (1-based) from the tag dict ``t`` and the ``meta`` of an IFD (_open); ValueError for a band
    the file does not have."""
    def val(tag, default=None):
        return _values(t[tag], bo) if tag in t else default

    rows, cols = meta["shape"]
    dt = np.dtype(meta["dtype"]).newbyteorder(bo)
    spp, planar = val(277, (1,))[0], val(284, (1,))[0]
    if not 1 <= band <= spp:
        raise ValueError(f"band {band} out of range: the file has {spp}")
    tiled = 322 in t
    if tiled:
        bw, bh = val(322)[0], val(323)[0]
        offs, cnts = val(324), val(325)
    else:
        bw, bh = cols, min(val(278, (rows,))[0], rows)
        offs, cnts = val(273), val(279)
    across, down = -(-cols // bw), -(-rows // bh)
    plane0, ch, chunk_spp = ((band - 1) * across * down, 0, 1) if planar == 2 else (0, band - 1, spp)
    return _Blocks(bw, bh, across, down, tiled, offs, cnts, plane0, ch, chunk_spp, dt, dt.itemsize, dt.kind,
                   val(317, (1,))[0], val(259, (1,))[0], rows, cols)


def read_geotiff(path: str, band: int = 1, rows: Optional[Tuple[int, int]] = None, decoder: str = "host", device=None,
                 band_bytes: int = 256 << 20, as_tensor: bool = False, transfers: Optional[list] = None, overview: int = 0):
    """Band ``band`` (1-based, like GDAL's GetRasterBand) of a (Geo)TIFF as float32, plus its metadata:
    ``{"geo": {tag: (type, count, raw bytes)}, "nodata": float | None, "dtype": numpy dtype of the file,
    "shape": (rows, cols), "byteorder": "<" | ">", "window": (r0, r1)}``.  Counterpart of loadImages
    (process_full_tiles.py:158-182).

    ``rows=(r0, r1)`` returns only raster rows [r0, r1) as [r1 - r0, cols] — bit for bit the slice of the full read — and
    decodes only the strips / tiles that intersect them (blocks are compressed independently and both predictors run
    along a row, so a block never needs its neighbours).  ``meta["shape"]`` stays the file's shape; ``meta["window"]``
    is the window returned.  ValueError unless 0 <= r0 < r1 <= rows of the file.

    ``decoder="host"`` (default) decodes block after block on the host; ``device``, ``band_bytes`` and ``as_tensor`` are not
    looked at.  ``decoder="device"`` decodes on the GPU with the same bits out (msr_lzw_decode_strips, then
    msr_tiff_blocks_to_f32 for predictor, conversion and placement): LZW files only, strips or tiles, classic or BigTIFF,
    predictor 1 or 2, little-endian, 8 / 16 / 32-bit integer or 32-bit float samples, one sample per pixel and block (a
    single-band file, or a planar one with ``band`` choosing the plane); anything else is a ValueError that names the
    property, raised before the GPU is touched, and a machine without a GPU is a RuntimeError: there is no fallback.  The
    blocks go through ``device`` (default: the current one) in bands of whole block rows of at most ``band_bytes``
    decoded bytes (plan_read_bands).  ``as_tensor=True`` returns the CUDA float32 tensor instead of a NumPy array.
    ``transfers``: a list that takes ``(direction, bytes, what)`` for every copy between host and device this read issues
    (DEMSuperResolution.transfers): the compressed blocks and their bookkeeping going up, the raster coming down.

    ``overview=k > 0`` reads the k-th reduced-resolution level instead (the k-th IFD of the chain whose NewSubfileType has
    bit 0 set: write_geotiff(overviews=), GDAL's internal overviews), with either decoder and the same keywords: ``rows``
    and ``meta["shape"]`` are that level's, ``meta["geo"]`` is that IFD's (empty in files written here) and
    ``meta["overview"] = k`` is added.  ValueError for a level the file does not have (overview_shapes lists them)."""
    if decoder not in ("host", "device"):
        raise ValueError(f"decoder must be 'host' or 'device', got {decoder!r}")
    if isinstance(overview, bool) or not isinstance(overview, (int, np.integer)) or overview < 0:
        raise ValueError(f"overview must be an integer >= 0, got {overview!r}")
    buf, t, bo, meta = _open(path, int(overview))
    nrows, cols = meta["shape"]
    if rows is None:
        r0, r1 = 0, nrows
    else:
        r0, r1 = int(rows[0]), int(rows[1])
        if not 0 <= r0 < r1 <= nrows:
            raise ValueError(f"{path}: row window ({r0}, {r1}) is not inside the raster's {nrows} rows")
    g = _block_geometry(t, bo, meta, band)
    meta["window"] = (r0, r1)
    if decoder == "device":
        what = (f"compression {g.comp} (only LZW, 5, is decoded)" if g.comp != 5 else
                f"predictor {g.pred} (only 1 and 2 are undone)" if g.pred not in (1, 2) else
                "big-endian samples" if bo == ">" else
                f"{g.sb * 8}-bit samples" if g.sb == 8 else
                f"chunky multi-band blocks ({g.spp} samples per pixel)" if g.spp != 1 else None)
        if what is not None:
            raise ValueError(f"{path}: decoder='device' does not read {what}; decoder='host' does")
        out = _read_blocks_device(buf, g, r0, r1, device, band_bytes, transfers)
        if not as_tensor and transfers is not None:
            transfers.append(("d2h", out.numel() * 4, "decoded raster"))
        return (out if as_tensor else out.cpu().numpy()), meta
    dt, native = g.dt, g.dt.newbyteorder("=")
    out = np.empty((r1 - r0, cols), np.float32)
    for by in range(r0 // g.bh, -(-r1 // g.bh)):          # the block rows that intersect [r0, r1)
        for bx in range(g.across):
            i = g.plane0 + by * g.across + bx
            raw = bytes(buf[g.offs[i]:g.offs[i] + g.cnts[i]])
            h = g.bh if g.tiled else min(g.bh, nrows - by * g.bh)
            nbytes = h * g.bw * g.spp * g.sb
            if g.comp == 1:
                data = np.frombuffer(raw[:nbytes].ljust(nbytes, b"\0"), np.uint8)
            elif g.comp == 5:
                data = lzw_decode(raw, nbytes)
            elif g.comp in (8, 32946):
                data = np.frombuffer(zlib.decompress(raw)[:nbytes].ljust(nbytes, b"\0"), np.uint8)
            elif g.comp == 32773:
                data = _packbits_decode(raw, nbytes)
            else:
                raise ValueError(f"{path}: unsupported compression {g.comp}")
            if g.pred == 3:
                # floating-point predictor: bytes of a row are stored most-significant plane first, byte-differenced
                b = data.reshape(h, nbytes // h).copy()
                b = np.cumsum(b, axis=1, dtype=np.uint8) if g.spp == 1 else _cumsum_stride(b, g.spp)
                b = b.reshape(h, g.sb, g.bw * g.spp).transpose(0, 2, 1)
                if bo == "<":
                    b = b[:, :, ::-1]
                arr = np.ascontiguousarray(b).view(dt).reshape(h, g.bw, g.spp)
            else:
                arr = data.view(dt).reshape(h, g.bw, g.spp)
                if g.pred == 2:
                    ut = np.dtype(f"u{g.sb}")
                    arr = np.cumsum(arr.astype(native).view(ut), axis=1, dtype=ut).view(native)
            y0, x0 = by * g.bh, bx * g.bw
            ya, yb = max(y0, r0), min(y0 + h, nrows, r1)      # the block's rows inside the window
            ww = min(g.bw, cols - x0)
            out[ya - r0:yb - r0, x0:x0 + ww] = arr[ya - y0:yb - y0, :ww, g.ch]
    return out, meta


def _cumsum_stride(b: np.ndarray, stride: int) -> np.ndarray:
    out = b.copy()
    for s in range(stride, out.shape[1]):
        out[:, s] = (out[:, s].astype(np.uint16) + out[:, s - stride]).astype(np.uint8)
    return out


# ---- writing ------------------------------------------------------------------------------------------------------------
def _rows_per_strip(rows: int, row_bytes: int) -> int:
    """Strips are whole rows, at most 64 KiB of them (one row where a row is longer)."""
    return max(1, min(rows, (1 << 16) // max(row_bytes, 1)))


def fp_predictor_reference(block: np.ndarray) -> np.ndarray:
    """The floating-point predictor (PREDICTOR=3, TIFF Technical Note 3) of the rows of ``block``, [h, w] little-endian
    float32 or float64: the NumPy twin that DEFINES what write_geotiff(predictor=3) hands to the compressor and whose bytes the
    device fetch (csrc/lzw_strip.h lzw_fetch_fp) reproduces.  Returns [h, w * itemsize] uint8.  Every row is regrouped into
    ``itemsize`` planes, the most significant byte of every sample first — byte ``p * w + x`` is byte ``itemsize - 1 - p`` of
    sample x — and then every byte but the row's first becomes ``t[q] - t[q - 1]`` modulo 256, over the whole regrouped row and
    so across the plane boundaries (libtiff's fpDiff with stride 1).  It is the inverse of what read_geotiff undoes for
    predictor 3."""
    a = np.asarray(block)
    if a.ndim != 2 or a.dtype.kind != "f" or a.dtype.itemsize not in (4, 8):
        raise ValueError(f"fp_predictor_reference takes a 2-D float32 or float64 array, got {a.dtype} {a.shape}")
    h, w = a.shape
    size = a.dtype.itemsize
    raw = np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("<")).view(np.uint8).reshape(h, w, size)
    t = np.ascontiguousarray(raw[:, :, ::-1].transpose(0, 2, 1)).reshape(h, size * w)
    out = t.copy()
    out[:, 1:] = t[:, 1:] - t[:, :-1]
    return out


def _encode_block(blk: np.ndarray, dt: np.dtype, comp: int, predictor: int) -> bytes:
    """One block of a file — a strip, or a tile padded to its full size — encoded on the host: the horizontal predictor
    differences every row of it in NumPy (the floating-point predictor: fp_predictor_reference), then msr_lzw_encode / zlib /
    nothing."""
    if predictor == 2:
        u = blk.view(np.dtype(f"<u{dt.itemsize}"))
        blk = u.copy()
        blk[:, 1:] = u[:, 1:] - u[:, :-1]
    elif predictor == 3:
        blk = fp_predictor_reference(blk)
    raw = np.ascontiguousarray(blk)
    return raw.tobytes() if comp == 1 else lzw_encode(raw) if comp == 5 else zlib.compress(raw.tobytes(), 6)


def plan_bands(rows: int, row_bytes: int, rps: int, band_bytes: int) -> list:
    """Cut the strips of a raster (``rps`` rows of ``row_bytes`` each, the last one shorter) into bands for the device
    encoder: ``[(s0, s1), ...]``, consecutive half-open strip ranges that cover every strip once.  A band is whole strips
    and holds at most ``band_bytes`` of raw data, unless a single strip is larger than that (then it is that strip)."""
    n_strips = -(-rows // rps)
    per_band = max(1, int(band_bytes) // max(rps * row_bytes, 1))
    return [(s0, min(s0 + per_band, n_strips)) for s0 in range(0, n_strips, per_band)]


def _torch_device(device, what: str = "encoder", data=None):
    """The CUDA device of the device encoder / decoder, or the RuntimeError of a machine without one.  ``device`` None: the
    device of ``data`` where that is a CUDA tensor, else the current one."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f"moonsuperresolution_amd needs a HIP device (MI355X / gfx950) for {what}='device'; there is no "
                           f"CPU fallback ({what}='host' is the host codec)")
    if device is None and getattr(data, "is_cuda", False):
        return data.device
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


def _launch_blocks(who: str, buf, arrays, slots, limit: int, errors, stream, entry: str, call):
    """The launch of a block codec on ``buf``'s device, all but the library call itself.  The checks: ``arrays`` — offsets,
    lengths and what else ``slots`` takes, an entry per block — of one length, every block inside ``buf`` and at most
    ``limit`` bytes long (``errors``: the two ValueError texts).  The output slots: ``slots(lengths, ...)`` gives each block's
    capacity and slot size, and the slots lie back to back in dst, at dst_off.  The tables on the device (int64
    src_off | dst_off, int32 src_len | dst_cap), dst, and dst_len with -1 everywhere.  Then ``call(lib, head, tail)``: the entry
    ``entry`` with the arguments in front of and behind its own, on ``stream`` (default: the current one).  Returns (dst,
    dst_off, dst_len): dst_off a host int64 array; the tensors keep the inputs of the launch alive."""
    import torch
    lib = _lib.load()
    if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous()):
        raise ValueError(f"{who} needs a contiguous uint8 CUDA tensor")
    off, ln, *rest = (np.ascontiguousarray(a, dtype=np.int64).reshape(-1) for a in arrays)
    if any(a.size != off.size for a in (ln, *rest)):
        raise ValueError(errors[0])
    if ln.size and (ln.min() < 0 or off.min() < 0 or int((off + ln).max()) > buf.numel() or ln.max() > limit):
        raise ValueError(errors[1])
    cap, slot = slots(ln, *rest)
    dst_off = np.concatenate(([0], np.cumsum(slot)[:-1])).astype(np.int64) if ln.size else np.zeros(0, np.int64)
    dev = buf.device
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(s):
            table = torch.from_numpy(np.concatenate([off, dst_off])).to(dev)              # int64: src_off | dst_off
            table32 = torch.from_numpy(np.concatenate([ln, cap]).astype(np.int32)).to(dev)   # int32: src_len | dst_cap
            n = int(ln.size)
            dst = torch.empty(max(int(slot.sum()), 1), dtype=torch.uint8, device=dev)
            dst_len = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
            rc = call(lib, (None, buf.data_ptr(), table.data_ptr(), table32.data_ptr(), n),
                      (dst.data_ptr(), table.data_ptr() + 8 * n, table32.data_ptr() + 4 * n, dst_len.data_ptr(),
                       C.c_void_p(s.cuda_stream)))
            _lib.raise_for(lib, None, rc, entry)
            for t in (buf, table, table32):
                t.record_stream(s)
    return dst, dst_off, dst_len[:n]


def _encode_strips_device(buf, offsets, lengths, sample_bytes: int, row_bytes: int, stream=None, predictor: Optional[int] = None):
    """One msr_lzw_encode_strips launch on ``buf``'s device: (dst, dst_off, dst_len) with dst / dst_len device tensors (the
    slots of capacity n + n // 2 + 1024 at dst_off, a host int64 array; dst_len int32, -1 = the slot was too small).
    Asynchronous on ``stream`` (default: the current stream); the tensors it returns keep the inputs of the launch alive.
    ``predictor`` 1 / 2 / 3: msr_tiff_encode_strips with that predictor instead, ``sample_bytes`` the samples' width."""
    if predictor is None:
        entry = "msr_lzw_encode_strips"
        call = lambda lib, head, tail: lib.msr_lzw_encode_strips(*head, int(sample_bytes), int(row_bytes), *tail)
    else:
        entry = "msr_tiff_encode_strips"
        call = lambda lib, head, tail: lib.msr_tiff_encode_strips(*head, int(sample_bytes), int(predictor), int(row_bytes), *tail)
    return _launch_blocks(
        "lzw_encode_device", buf, (offsets, lengths), lambda ln: (ln + ln // 2 + 1024,) * 2, 1 << 30,
        ("offsets and lengths differ in length", "a strip lies outside the buffer (or is longer than 2^30 bytes)"), stream,
        entry, call)


def _download_strips(dst, dst_off: np.ndarray, dst_len) -> list:
    """The streams of one launch as bytes: lengths to the host, streams compacted on the device, one copy back."""
    import torch
    lens = dst_len.cpu().numpy().astype(np.int64)
    if (lens < 0).any():
        raise ValueError(f"LZW encode failed: the stream of strip {int(np.argmax(lens < 0))} does not fit its slot")
    if not lens.size:
        return []
    packed = torch.cat([dst[o:o + l] for o, l in zip(dst_off.tolist(), lens.tolist())]).cpu().numpy().tobytes()
    ends = np.cumsum(lens).tolist()
    return [packed[e - l:e] for e, l in zip(ends, lens.tolist())]


def lzw_encode_device(buf, offsets, lengths, sample_bytes: int = 0, row_bytes: int = 0, stream=None,
                      predictor: Optional[int] = None) -> list:
    """TIFF LZW streams of the strips ``buf[offsets[i] : offsets[i] + lengths[i]]`` of a uint8 CUDA tensor, encoded on its
    device in one launch (msr_lzw_encode_strips): byte for byte ``lzw_encode`` of the same bytes.  ``sample_bytes`` 1 / 2 / 4
    applies the horizontal predictor on the fly to little-endian samples of that width, restarting every ``row_bytes``.
    ``predictor`` 1 / 2 / 3 (default None: the above) names the TIFF predictor instead, with ``sample_bytes`` the samples'
    width (msr_tiff_encode_strips): 3 is the floating-point predictor of float32 rows, ``fp_predictor_reference``.
    ValueError if a stream does not fit its slot of n + n // 2 + 1024 bytes (the host wrapper's rule)."""
    import torch
    dst, dst_off, dst_len = _encode_strips_device(buf, offsets, lengths, sample_bytes, row_bytes, stream, predictor)
    if stream is not None:
        torch.cuda.current_stream(buf.device).wait_stream(stream)
    return _download_strips(dst, dst_off, dst_len)


# ---- reading on the device ------------------------------------------------------------------------------------------
def plan_read_bands(r0: int, r1: int, block_h: int, block_row_bytes: int, band_bytes: int) -> list:
    """Cut the block rows (rows of strips or tiles, ``block_h`` raster rows each) that hold raster rows [r0, r1) into bands
    for the device decoder: ``[(b0, b1), ...]``, consecutive half-open ranges of block rows that cover block rows
    r0 // block_h .. ceil(r1 / block_h) once and nothing else.  A band holds at most ``band_bytes`` of decoded data at
    ``block_row_bytes`` a block row, unless a single block row is larger than that (then it is that block row)."""
    first, last = r0 // block_h, -(-r1 // block_h)
    per_band = max(1, int(band_bytes) // max(int(block_row_bytes), 1))
    return [(b0, min(b0 + per_band, last)) for b0 in range(first, last, per_band)]


def lzw_decode_device(buf, offsets, lengths, out_sizes, stream=None, check: bool = True):
    """One msr_lzw_decode_strips launch on ``buf``'s device: the TIFF LZW blocks ``buf[offsets[i] : offsets[i] + lengths[i]]``
    of a uint8 CUDA tensor decoded into slots of ``out_sizes[i]`` bytes.  Returns (dst, dst_off, dst_len): dst a uint8 device
    tensor holding the slots at dst_off (a host int64 array; the slots start on 16-byte boundaries), dst_len the int32 device
    tensor of what msr_lzw_decode returns for each block; a block that decodes short has its tail zeroed, like ``lzw_decode``.
    Asynchronous on ``stream`` (default: the current stream) with ``check=False``; with ``check=True`` it waits for the
    lengths and raises ValueError("malformed LZW stream") if one is negative, as the host path does."""
    import torch

    def slots(ln, cap):
        if cap.size and (cap.min() < 0 or cap.max() >= (1 << 31)):
            raise ValueError("an output size is negative or above 2^31 - 1 bytes")
        return cap, (cap + 15) // 16 * 16

    dst, dst_off, dst_len = _launch_blocks(
        "lzw_decode_device", buf, (offsets, lengths, out_sizes), slots, (1 << 31) - 1,
        ("offsets, lengths and out_sizes differ in length", "a block lies outside the buffer (or is longer than 2^31 - 1 bytes)"),
        stream, "msr_lzw_decode_strips", lambda lib, head, tail: lib.msr_lzw_decode_strips(*head, *tail))
    if check:
        if stream is not None:
            torch.cuda.current_stream(buf.device).wait_stream(stream)
        _check_decoded(dst_len)
    return dst, dst_off, dst_len


def _check_decoded(dst_len) -> None:
    """The host path's error for a block msr_lzw_decode rejects (waits for the lengths of the launch)."""
    if dst_len.numel() and int(dst_len.min().item()) < 0:
        raise ValueError("malformed LZW stream")


def lzw_decode_device_bytes(buf, offsets, lengths, out_sizes, stream=None) -> list:
    """``lzw_decode_device`` with the decoded blocks as ``bytes`` (each ``out_sizes[i]`` long: ``lzw_decode``'s result)."""
    dst, dst_off, _ = lzw_decode_device(buf, offsets, lengths, out_sizes, stream)
    host = dst.cpu().numpy()
    return [host[o:o + c].tobytes() for o, c in zip(dst_off.tolist(), np.asarray(out_sizes, np.int64).reshape(-1).tolist())]


def _read_blocks_device(buf, g: _Blocks, r0: int, r1: int, device, band_bytes: int, transfers: Optional[list] = None):
    """Raster rows [r0, r1) of the blocks ``g`` of the memory map ``buf`` as a float32 CUDA tensor, decoded on the device band
    by band (plan_read_bands): gather the band's compressed blocks from the memory map into one host array, upload once, one
    decode launch, one placement launch into the [r1 - r0, cols] tensor.  Device memory is the output plus about
    2.5 x band_bytes (compressed + decoded blocks)."""
    import torch
    lib = _lib.load()
    dev = _torch_device(device, "decoder")
    offs, cnts = np.asarray(g.offs, np.int64), np.asarray(g.cnts, np.int64)
    across, bw, bh, sb = g.across, g.bw, g.bh, g.sb
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev)
        out = torch.empty((r1 - r0, g.cols), dtype=torch.float32, device=dev)
        for b0, b1 in plan_read_bands(r0, r1, bh, across * bh * bw * sb, band_bytes):
            by = np.repeat(np.arange(b0, b1, dtype=np.int64), across)
            bx = np.tile(np.arange(across, dtype=np.int64), b1 - b0)
            idx = g.plane0 + by * across + bx
            o = offs[idx]
            c = np.clip(np.minimum(cnts[idx], buf.size - o), 0, None)      # a block that runs past the file's end is cut there
            h = np.full(idx.size, bh, np.int64) if g.tiled else np.minimum(bh, g.rows - by * bh)
            lo, hi = int(o.min()), int((o + c).max())
            total = int(c.sum())
            # the file's bytes go to pinned memory (the one host copy), from where the upload is one DMA transfer
            if hi - lo <= total + total // 4 + 4096:                       # the blocks lie (almost) back to back: one copy
                staged = torch.empty(max(hi - lo, 1), dtype=torch.uint8, pin_memory=True)
                staged.numpy()[:hi - lo] = buf[lo:hi]
                src_off = o - lo
            else:
                src_off = np.concatenate(([0], np.cumsum(c)[:-1]))
                staged = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
                host = staged.numpy()
                for so, fo, n in zip(src_off.tolist(), o.tolist(), c.tolist()):
                    host[so:so + n] = buf[fo:fo + n]
            src = staged.to(dev, non_blocking=True)
            if transfers is not None:
                # per block: offset and slot (2 x int64), length and capacity (2 x int32), decoded offset (int64), origin
                # (2 x int32) going up; the band's smallest decoded length coming down (_check_decoded)
                transfers.append(("h2d", staged.numel(), "compressed input blocks"))
                transfers.append(("h2d", 40 * int(idx.size), "block tables of the decoder"))
                transfers.append(("d2h", 4, "decode status"))
            dst, dst_off, dst_len = lzw_decode_device(src, src_off, c, h * bw * sb, check=False)
            n = int(idx.size)
            blk_off = torch.from_numpy(dst_off).to(dev)
            origin = torch.from_numpy(np.concatenate([bx * bw, by * bh]).astype(np.int32)).to(dev)      # x0 | y0
            rc = lib.msr_tiff_blocks_to_f32(None, dst.data_ptr(), blk_off.data_ptr(), origin.data_ptr(), origin.data_ptr() + 4 * n,
                                            n, int(bw), int(bh), ord(g.kind), int(sb), int(g.pred), out.data_ptr(), int(r0),
                                            int(r1 - r0), int(g.cols), C.c_void_p(s.cuda_stream))
            _lib.raise_for(lib, None, rc, "msr_tiff_blocks_to_f32")
            _check_decoded(dst_len)          # waits for the band: its buffers are free before the next one is gathered
    return out


_TORCH_BITS = {1: "int8", 2: "int16", 4: "int32", 8: "int64"}


def _band_bytes_on_device(data, r0: int, r1: int, dt: np.dtype, dev):
    """Rows [r0, r1) of ``data`` (NumPy array or CUDA tensor) as the little-endian bytes of dtype ``dt`` on ``dev``."""
    import torch
    if not isinstance(data, torch.Tensor):
        return torch.from_numpy(np.ascontiguousarray(data[r0:r1], dtype=dt).view(np.uint8).reshape(-1)).to(dev)
    t = data[r0:r1]                                  # a view: possibly cropped (not contiguous), possibly on another device
    integer = not t.dtype.is_floating_point and t.dtype != torch.bool
    if dt.kind == "f":
        target = torch.float32 if dt.itemsize == 4 else torch.float64
    elif integer and t.element_size() == dt.itemsize:
        target = t.dtype                             # the same bits already
    else:
        target = getattr(torch, _TORCH_BITS[dt.itemsize])
        if not (integer and t.element_size() < dt.itemsize):
            # through int64: narrowing wraps modulo 2^bits like NumPy's astype.  An integer that only widens (uint8 ->
            # 16 bits: the ``good`` product) keeps its value in the direct conversion below and needs no such temporary
            t = t.to(torch.int64)
    # ONE strided copy: conversion, compaction of the cropped view and the change of device at once
    out = torch.empty(t.shape, dtype=target, device=dev)
    out.copy_(t)
    return out.view(torch.uint8).reshape(-1)


def _device_predictor(sb: int, predictor: int) -> Tuple[int, Optional[int]]:
    """(sample_bytes, predictor) as the device encoders take them, for a file's sample width and predictor in force: predictors
    1 and 2 go through the entries that know the horizontal predictor alone (sample_bytes 0: none), 3 through msr_tiff_encode_*."""
    return (sb, 3) if predictor == 3 else (sb if predictor == 2 else 0, None)


def _encode_band_device(blocks, offsets, lengths, sample_bytes: int, row_bytes: int, transfers: Optional[list], kind: str,
                        raw: Optional[int], predictor: Optional[int] = None) -> list:
    """The last steps of a band of the device encoder, strips or tiles (``kind``: "strip" / "tile"): ``blocks``, the band laid
    out block after block as a uint8 device tensor, goes through one launch, compaction and download (lzw_encode_device, which
    ``sample_bytes`` and ``predictor`` go to: _device_predictor), and ``transfers`` takes the band's entries; ``raw``: the bytes
    of the band where it was uploaded from the host, else None."""
    enc = lzw_encode_device(blocks, offsets, lengths, sample_bytes, row_bytes, predictor=predictor)
    if transfers is not None:
        if raw is not None:
            transfers.append(("h2d", raw, "raw product band"))
        # per block: offset and slot (2 x int64), length and capacity (2 x int32) going up, the stream's length coming down
        transfers.append(("h2d", 24 * len(enc), f"{kind} tables of the encoder"))
        transfers.append(("d2h", 4 * len(enc), f"encoded {kind} lengths"))
        transfers.append(("d2h", sum(len(b) for b in enc), f"compressed output {kind}s"))
    return enc


def _device_strips(data, dt: np.dtype, rps: int, predictor: int, device, band_bytes: int,
                   transfers: Optional[list] = None) -> list:
    """The strips of ``data`` LZW-encoded on the device, band by band (plan_bands): upload (or convert) a band, one launch,
    compact, download.  Device memory is bounded by the band: about 2.5 x band_bytes plus 1 KiB per strip."""
    rows, cols = data.shape
    row_bytes = cols * dt.itemsize
    dev = _torch_device(device, data=data)
    psb, pred = _device_predictor(dt.itemsize, predictor)
    strips = []
    for s0, s1 in plan_bands(rows, row_bytes, rps, band_bytes):
        r0, r1 = s0 * rps, min(s1 * rps, rows)
        buf = _band_bytes_on_device(data, r0, r1, dt, dev)
        starts = np.arange(r0, r1, rps, dtype=np.int64)
        lengths = (np.minimum(starts + rps, r1) - starts) * row_bytes
        strips += _encode_band_device(buf, (starts - r0) * row_bytes, lengths, psb, row_bytes, transfers, "strip",
                                      buf.numel() if isinstance(data, np.ndarray) else None, pred)
    return strips


def _checked_format(dtype, compress: str, predictor: int, encoder: str):
    """(little-endian dtype, compression tag, predictor in force) of a file to write, or the ValueError of write_geotiff."""
    if encoder not in ("host", "device"):
        raise ValueError(f"encoder must be 'host' or 'device', got {encoder!r}")
    if encoder == "device" and compress != "lzw":
        raise ValueError(f"encoder='device' encodes LZW only, got compress={compress!r}")
    dt = np.dtype(dtype).newbyteorder("<")
    if dt.kind not in "uif" or dt.itemsize not in (1, 2, 4, 8):
        raise ValueError(f"unsupported dtype {dtype}")
    comp = {"none": 1, "lzw": 5, "deflate": 8}[compress]
    if predictor == 3 and dt.kind != "f":
        raise ValueError(f"predictor 3 is the floating-point predictor: it is not defined for dtype {dt.name}")
    if comp == 1 or dt.itemsize == 8 and predictor == 2:
        predictor = 1
    if encoder == "device" and predictor == 3 and dt.itemsize != 4:
        raise ValueError(f"encoder='device' applies predictor 3 to float32 only, got dtype {dt.name}; encoder='host' does")
    return dt, comp, predictor


def encode_strips(data, dtype, rps: int, compress: str = "lzw", predictor: int = 2, encoder: str = "host", device=None,
                  band_bytes: int = 256 << 20, transfers: Optional[list] = None) -> list:
    """The encoded strips of ``rps`` rows each (the last one shorter) of the 2-D ``data`` converted to ``dtype``: what
    write_geotiff puts into the file for these rows.  Strips are encoded independently, so the strips of rows [a, b) of a
    raster, a a multiple of the raster's ``rps``, are those strips of the whole raster's file: a rank of a sharded run
    encodes the rows it computed (distributed.strip_plan) and write_strips puts the file together.  ``encoder``,
    ``device``, ``band_bytes``: write_geotiff's; ``transfers``: a list that takes ``(direction, bytes, what)`` for every
    copy between host and device the device encoder issues (DEMSuperResolution.transfers)."""
    dt, comp, predictor = _checked_format(dtype, compress, predictor, encoder)
    if data.ndim != 2:
        raise ValueError("Data must be a 2-D array (the reference raises for rank != 2 too, process_full_tiles.py:505-519).")
    if encoder == "device":
        return _device_strips(data, dt, rps, predictor, device, band_bytes, transfers)
    arr = np.ascontiguousarray(data, dtype=dt)
    return [_encode_block(arr[r:r + rps], dt, comp, predictor) for r in range(0, arr.shape[0], rps)]


def write_strips(path: str, strips: list, shape: Tuple[int, int], dtype, rps: int, meta: Optional[dict] = None,
                 nodata: Optional[float] = None, compress: str = "lzw", predictor: int = 2,
                 bigtiff: Optional[bool] = None) -> None:
    """The file write_geotiff writes for a raster of ``shape``, from its encoded strips in order (encode_strips, with the
    same ``dtype``, ``rps``, ``compress`` and ``predictor``)."""
    dt, comp, predictor = _checked_format(dtype, compress, predictor, "host")
    rows, cols = int(shape[0]), int(shape[1])
    if len(strips) != -(-rows // rps):
        raise ValueError(f"{len(strips)} strips for {rows} rows of {rps} a strip")
    _write_container(path, [(rows, cols, strips)], dt, rps, None, comp, predictor, meta, nodata, bigtiff)


# ---- tiles and overviews --------------------------------------------------------------------------------------------
OVERVIEW_DTYPES = ("<f4", "|u1", "<u2")


def overview_reference(a: np.ndarray, nodata: Optional[float] = None) -> np.ndarray:
    """The next reduced-resolution level of the 2-D raster ``a`` (float32, uint8 or uint16): the NumPy twin that DEFINES
    what write_geotiff(overviews=) stores and whose bits csrc/tiff_overview.h (the kernel of msr_overview_half and
    msr_overview_half_host) reproduces.  The result is ceil(rows / 2) x ceil(cols / 2) of ``a``'s dtype; ``dst[i, j]`` comes
    from ``a[2i : 2i + 2, 2j : 2j + 2]`` clipped to the raster.

    float32: a pixel counts iff ``v != float32(nodata)`` (a NaN counts and propagates; ``nodata=None``: every pixel
    counts).  No counting pixel gives ``nodata``; otherwise ``s / float32(n)`` with ``s`` the float32 sum of the n counting
    values in row-major order, started from the first of them and not from 0, so that -0.0 alone stays -0.0: one rounding
    per addition, one for the division.  uint8 / uint16: the maximum of the block (``nodata`` is not looked at), so the
    overview of a ``good`` mask is 1 exactly where the overview of its ``mean`` is not nodata."""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype.newbyteorder("<").str not in OVERVIEW_DTYPES or 0 in a.shape:
        raise ValueError(f"overview_reference takes a non-empty 2-D float32, uint8 or uint16 array, got {a.dtype} {a.shape}")
    rows, cols = a.shape
    dr, dc = -(-rows // 2), -(-cols // 2)
    pad = np.zeros((2 * dr, 2 * dc), a.dtype)
    pad[:rows, :cols] = a
    inside = np.zeros((2 * dr, 2 * dc), bool)
    inside[:rows, :cols] = True
    quads = [(pad[y::2, x::2], inside[y::2, x::2]) for y, x in ((0, 0), (0, 1), (1, 0), (1, 1))]     # row-major
    if a.dtype.kind == "u":
        out = quads[0][0].copy()
        for v, _ in quads[1:]:
            out = np.maximum(out, v)              # outside the raster: 0, the smallest unsigned value
        return out
    nv = None if nodata is None else np.float32(nodata)
    s = np.zeros((dr, dc), np.float32)
    n = np.zeros((dr, dc), np.int32)
    with np.errstate(all="ignore"):
        for v, ins in quads:
            counts = ins if nv is None else ins & (v != nv)
            s = np.where(counts, np.where(n > 0, s + v, v), s).astype(np.float32)
            n += counts
        mean = s / np.maximum(n, 1).astype(np.float32)
    return mean if nv is None else np.where(n > 0, mean, nv).astype(np.float32)


def check_layout(tile, overviews, shape: Optional[Tuple[int, int]] = None, dt: Optional[np.dtype] = None):
    """write_geotiff's ``tile`` and ``overviews`` checked: ``(tile as a pair of ints or None, overviews)``, or the ValueError
    that names the keyword.  What depends on the raster (the largest ``overviews``, the dtype) is checked where ``shape`` /
    ``dt`` are given."""
    if tile is not None:
        ok = isinstance(tile, (tuple, list)) and len(tile) == 2 and all(
            isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v > 0 and v % 16 == 0 for v in tile)
        if not ok:
            raise ValueError(f"tile must be None or (tile_h, tile_w), both positive multiples of 16 (TIFF 6.0), got {tile!r}")
        tile = (int(tile[0]), int(tile[1]))
    if isinstance(overviews, bool) or not isinstance(overviews, (int, np.integer)) or overviews < 0:
        raise ValueError(f"overviews must be an integer >= 0, got {overviews!r}")
    overviews = int(overviews)
    if overviews and tile is None:
        raise ValueError(f"overviews={overviews} needs tile=(tile_h, tile_w): reduced levels are written in tiles")
    if overviews and shape is not None:
        most = (max(int(shape[0]), int(shape[1])) - 1).bit_length()          # ceil(log2(max(rows, cols)))
        if overviews > most:
            raise ValueError(f"overviews={overviews} is more than the {most} level(s) a {shape[0]} x {shape[1]} raster has")
    if overviews and dt is not None and np.dtype(dt).newbyteorder("<").str not in OVERVIEW_DTYPES:
        raise ValueError(f"overviews are built for float32, uint8 and uint16 files, got dtype {np.dtype(dt)}")
    return tile, overviews


def check_file_order(layout, tile) -> str:
    """write_geotiff's ``layout`` checked against its ``tile``: the layout, or the ValueError that names the keyword."""
    if layout not in ("plain", "cog"):
        raise ValueError(f"layout must be 'plain' or 'cog', got {layout!r}")
    if layout == "cog" and tile is None:
        raise ValueError("layout='cog' needs tile=(tile_h, tile_w): a cloud-optimised file is written in tiles")
    return layout


def _host_tiles(arr: np.ndarray, dt: np.dtype, th: int, tw: int, comp: int, predictor: int) -> list:
    """The tiles of ``arr`` in row-major order encoded on the host (_encode_block), an edge tile padded with zero bytes."""
    rows, cols = arr.shape
    tiles = []
    for y in range(0, rows, th):
        for x in range(0, cols, tw):
            t = np.zeros((th, tw), dt)
            blk = arr[y:y + th, x:x + tw]
            t[:blk.shape[0], :blk.shape[1]] = blk
            tiles.append(_encode_block(t, dt, comp, predictor))
    return tiles


def _host_levels(arr: np.ndarray, dt: np.dtype, tile: Tuple[int, int], overviews: int, nodata: Optional[float], comp: int,
                 predictor: int) -> list:
    """``[(rows, cols, tiles), ...]`` of the raster and its ``overviews`` reduced levels (overview_reference)."""
    levels = []
    for k in range(overviews + 1):
        if k:
            arr = overview_reference(arr, nodata if dt.kind == "f" else None)
        levels.append((arr.shape[0], arr.shape[1], _host_tiles(arr, dt, tile[0], tile[1], comp, predictor)))
    return levels


def _device_levels(data, dt: np.dtype, tile: Tuple[int, int], overviews: int, nodata: Optional[float], predictor: int, device,
                   band_bytes: int, transfers: Optional[list] = None) -> list:
    """_host_levels on the device, with the same bytes.  Every level goes through in bands of whole tile rows of at most
    ``band_bytes`` raw bytes (one tile row where that is larger; plan_bands, a tile row counting as a strip of tile_h rows of
    the padded width): the band's bytes (_band_bytes_on_device for level 0; a view for the others), msr_overview_half of the
    band into its rows of the next level (a band starts on a multiple of tile_h, an even row, so those rows depend on this
    band alone), the tile-major arrangement with torch copies (pad, then one permuted copy), then _encode_band_device as for
    strips: one msr_lzw_encode_strips launch with row_bytes = tile_w * sample_bytes, compaction and download.
    Device memory is about 2.5 x band_bytes plus the next level (a quarter of the one being encoded, so at most a third of
    the raster with the level after it)."""
    import torch
    lib = _lib.load()
    dev = _torch_device(device, data=data)
    th, tw = tile
    sb = dt.itemsize
    bits = getattr(torch, _TORCH_BITS[sb])           # the container of a sample's bits: they are only copied here
    psb, pred = _device_predictor(sb, predictor)
    has_nodata = int(dt.kind == "f" and nodata is not None)
    levels = []
    cur = data
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev)
        for k in range(overviews + 1):
            rows, cols = int(cur.shape[0]), int(cur.shape[1])
            across = -(-cols // tw)
            nxt = torch.empty((-(-rows // 2), -(-cols // 2)), dtype=bits, device=dev) if k < overviews else None
            blocks = []
            for t0, t1 in plan_bands(rows, across * tw * sb, th, band_bytes):
                r0, r1 = t0 * th, min(t1 * th, rows)
                if k == 0:
                    band = _band_bytes_on_device(cur, r0, r1, dt, dev).view(bits).reshape(r1 - r0, cols)
                else:
                    band = cur[r0:r1]
                if nxt is not None:
                    rc = lib.msr_overview_half(None, band.data_ptr(), r1 - r0, cols, ord(dt.kind), sb, has_nodata,
                                               float(nodata) if has_nodata else 0.0, nxt[r0 // 2:].data_ptr(),
                                               C.c_void_p(s.cuda_stream))
                    _lib.raise_for(lib, None, rc, "msr_overview_half")
                nt = t1 - t0
                if (r1 - r0, cols) != (nt * th, across * tw):
                    padded = torch.zeros((nt * th, across * tw), dtype=bits, device=dev)
                    padded[:r1 - r0, :cols] = band
                    band = padded
                tiles = band.view(nt, th, across, tw).permute(0, 2, 1, 3).contiguous().view(torch.uint8).reshape(-1)
                lengths = np.full(nt * across, th * tw * sb, np.int64)
                raw = (r1 - r0) * cols * sb if k == 0 and isinstance(data, np.ndarray) else None
                blocks += _encode_band_device(tiles, np.cumsum(lengths) - lengths, lengths, psb, tw * sb, transfers, "tile", raw, pred)
            levels.append((rows, cols, blocks))
            cur = nxt
    return levels


def _encode_blocks_device(buf, offsets, pitches, valid_w_bytes, valid_rows, block_w_bytes: int, block_h: int, sample_bytes: int,
                          stream=None, predictor: Optional[int] = None):
    """One msr_lzw_encode_blocks launch on ``buf``'s device: block i is ``block_h`` rows of ``block_w_bytes`` bytes whose valid
    part, ``valid_rows[i]`` rows of ``valid_w_bytes[i]`` bytes, lies at ``buf[offsets[i]]`` with ``pitches[i]`` bytes between rows
    and is read there; the rest of the block is zero.  What _launch_blocks checks for lengths is checked here for the valid parts:
    one entry per block in every array, each valid part inside its block and every byte of it inside ``buf``.  Returns (dst,
    dst_off, dst_len) as _encode_strips_device does, the slots n + n // 2 + 1024 bytes for the n bytes of a block.
    ``predictor`` 1 / 2 / 3: msr_tiff_encode_blocks with that predictor instead, ``sample_bytes`` the samples' width."""
    import torch
    lib = _lib.load()
    if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous()):
        raise ValueError("lzw_encode_blocks_device needs a contiguous uint8 CUDA tensor")
    off, pitch, wb, vr = (np.ascontiguousarray(a, dtype=np.int64).reshape(-1) for a in (offsets, pitches, valid_w_bytes, valid_rows))
    if any(a.size != off.size for a in (pitch, wb, vr)):
        raise ValueError("offsets, pitches, valid_w_bytes and valid_rows differ in length")
    bw, bh = int(block_w_bytes), int(block_h)
    if off.size and (wb.min() < 0 or wb.max() > bw or vr.min() < 0 or vr.max() > bh):
        raise ValueError(f"a valid part is not inside its block of {bh} rows of {bw} bytes")
    some = (wb > 0) & (vr > 0)                   # a block without a valid byte reads nothing
    if off.size and (off.min() < 0 or pitch.min() < 0 or
                     (some.any() and int((off + (vr - 1) * pitch + wb)[some].max()) > buf.numel())):
        raise ValueError("a block's valid part lies outside the buffer")
    n = int(off.size)
    size = bw * bh
    cap = np.full(n, size + size // 2 + 1024, np.int64)
    dst_off = np.arange(n, dtype=np.int64) * (size + size // 2 + 1024)
    dev = buf.device
    if n == 0:                                   # nothing to launch (and empty tables have no address to hand over)
        return torch.empty(0, dtype=torch.uint8, device=dev), dst_off, torch.empty(0, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(s):
            table = torch.from_numpy(np.concatenate([off, pitch, dst_off])).to(dev)                  # int64: off | pitch | dst_off
            table32 = torch.from_numpy(np.concatenate([wb, vr, cap]).astype(np.int32)).to(dev)       # int32: w | rows | dst_cap
            dst = torch.empty(int(cap.sum()), dtype=torch.uint8, device=dev)
            dst_len = torch.full((n,), -1, dtype=torch.int32, device=dev)
            p64, p32 = table.data_ptr(), table32.data_ptr()
            head = (None, buf.data_ptr(), p64, p64 + 8 * n, p32, p32 + 4 * n, n, bw, bh, int(sample_bytes))
            tail = (dst.data_ptr(), p64 + 16 * n, p32 + 8 * n, dst_len.data_ptr(), C.c_void_p(s.cuda_stream))
            if predictor is None:
                _lib.raise_for(lib, None, lib.msr_lzw_encode_blocks(*head, *tail), "msr_lzw_encode_blocks")
            else:
                _lib.raise_for(lib, None, lib.msr_tiff_encode_blocks(*head, int(predictor), *tail), "msr_tiff_encode_blocks")
            for t in (buf, table, table32):
                t.record_stream(s)
    return dst, dst_off, dst_len[:n]


def lzw_encode_blocks_device(buf, offsets, pitches, valid_w_bytes, valid_rows, block_w_bytes: int, block_h: int,
                             sample_bytes: int = 0, stream=None, predictor: Optional[int] = None) -> list:
    """TIFF LZW streams of blocks (tiles) of ``block_h`` rows of ``block_w_bytes`` bytes read in place from the uint8 CUDA tensor
    ``buf``, encoded on its device in one launch (msr_lzw_encode_blocks; the arguments: _encode_blocks_device): byte for byte
    ``lzw_encode`` of each block padded with zero bytes and, with ``sample_bytes`` 1 / 2 / 4, differenced along its rows
    afterwards.  The pitch is per block, so blocks of several rasters in ``buf`` share the launch.  ``predictor`` 1 / 2 / 3
    (default None: the above): lzw_encode_device's, through msr_tiff_encode_blocks; 3 is ``fp_predictor_reference`` of the
    padded float32 block."""
    import torch
    dst, dst_off, dst_len = _encode_blocks_device(buf, offsets, pitches, valid_w_bytes, valid_rows, block_w_bytes, block_h,
                                                  sample_bytes, stream, predictor)
    if stream is not None:
        torch.cuda.current_stream(buf.device).wait_stream(stream)
    return _download_strips(dst, dst_off, dst_len)


def _tile_table(rows: int, cols: int, th: int, tw: int, sb: int, base: int = 0):
    """The tiles of a [rows, cols] raster of ``sb``-byte samples that lies row-major at byte ``base``, in row-major order, as
    the arrays of _encode_blocks_device: (offsets, pitches, valid_w_bytes, valid_rows)."""
    ty, tx = np.meshgrid(np.arange(-(-rows // th), dtype=np.int64), np.arange(-(-cols // tw), dtype=np.int64), indexing="ij")
    ty, tx = ty.reshape(-1), tx.reshape(-1)
    pitch = cols * sb
    return (base + ty * th * pitch + tx * tw * sb, np.full(ty.size, pitch, np.int64), np.minimum(tw, cols - tx * tw) * sb,
            np.minimum(th, rows - ty * th))


def _device_levels_in_place(data, dt: np.dtype, tile: Tuple[int, int], overviews: int, nodata: Optional[float], predictor: int,
                            device, band_bytes: int, transfers: Optional[list] = None) -> list:
    """_device_levels for layout="cog", with the same bytes: the tiles are encoded where their level lies
    (msr_lzw_encode_blocks reads a tile's rows at the level's pitch and makes the padding of an edge tile itself), so there is
    no zero-padded frame and no tile-major copy.  Level 0 goes through in the bands of _device_levels: the band's bytes
    (_band_bytes_on_device), msr_overview_half of the band into its rows of level 1, one encode launch on the band, compaction
    and download.  Levels 1 .. n lie back to back in ONE allocation, each row-major at its own pitch; levels 2 .. n are the
    chain of msr_overview_half, and the tiles of all of them go through ONE further launch.  A write issues
    len(plan_bands(level 0)) + (1 if overviews else 0) encode launches.  Device memory is about 2.5 x band_bytes, plus 2.5 x the
    reduced levels (a third of the raster), which are held and encoded at once."""
    import torch
    lib = _lib.load()
    dev = _torch_device(device, data=data)
    th, tw = tile
    sb = dt.itemsize
    psb, pred = _device_predictor(sb, predictor)
    has_nodata = int(dt.kind == "f" and nodata is not None)
    shapes = [(int(data.shape[0]), int(data.shape[1]))]
    for _ in range(overviews):
        shapes.append((-(-shapes[-1][0] // 2), -(-shapes[-1][1] // 2)))
    sizes = [(r * c * sb + 15) // 16 * 16 for r, c in shapes[1:]]            # a level starts on a 16-byte boundary
    bases = [int(b) for b in np.cumsum([0] + sizes[:-1])] if sizes else []

    def encode(buf, table, raw):
        enc = _download_strips(*_encode_blocks_device(buf, *table, tw * sb, th, psb, predictor=pred))
        if transfers is not None:
            if raw is not None:
                transfers.append(("h2d", raw, "raw product band"))
            # per block: offset, pitch and slot (3 x int64), valid width, valid rows and capacity (3 x int32) going up
            transfers.append(("h2d", 36 * len(enc), "tile tables of the encoder"))
            transfers.append(("d2h", 4 * len(enc), "encoded tile lengths"))
            transfers.append(("d2h", sum(len(b) for b in enc), "compressed output tiles"))
        return enc

    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev)

        def half(src_ptr, rows, cols, dst_ptr):
            rc = lib.msr_overview_half(None, src_ptr, rows, cols, ord(dt.kind), sb, has_nodata, float(nodata) if has_nodata else 0.0,
                                       dst_ptr, C.c_void_p(s.cuda_stream))
            _lib.raise_for(lib, None, rc, "msr_overview_half")

        pyramid = torch.empty(max(sum(sizes), 1), dtype=torch.uint8, device=dev) if overviews else None
        rows, cols = shapes[0]
        level0 = []
        for t0, t1 in plan_bands(rows, -(-cols // tw) * tw * sb, th, band_bytes):
            r0, r1 = t0 * th, min(t1 * th, rows)
            band = _band_bytes_on_device(data, r0, r1, dt, dev)
            if overviews:            # a band starts on an even row: its rows of level 1 depend on this band alone
                half(band.data_ptr(), r1 - r0, cols, pyramid.data_ptr() + (r0 // 2) * shapes[1][1] * sb)
            level0 += encode(band, _tile_table(r1 - r0, cols, th, tw, sb), band.numel() if isinstance(data, np.ndarray) else None)
        levels = [(rows, cols, level0)]
        if overviews:
            for k in range(1, overviews):
                half(pyramid.data_ptr() + bases[k - 1], shapes[k][0], shapes[k][1], pyramid.data_ptr() + bases[k])
            tables = [_tile_table(r, c, th, tw, sb, base) for (r, c), base in zip(shapes[1:], bases)]
            enc = encode(pyramid, tuple(np.concatenate(col) for col in zip(*tables)), None)
            for (r, c), table in zip(shapes[1:], tables):
                levels.append((r, c, enc[:table[0].size]))
                enc = enc[table[0].size:]
    return levels


def write_geotiff(path: str, data: np.ndarray, meta: Optional[dict] = None, nodata: Optional[float] = None,
                  dtype=np.float32, compress: str = "lzw", predictor: int = 2, bigtiff: Optional[bool] = None,
                  encoder: str = "host", device=None, band_bytes: int = 256 << 20, transfers: Optional[list] = None, *,
                  tile: Optional[Tuple[int, int]] = None, overviews: int = 0, layout: str = "plain") -> None:
    """Write a single-band GeoTIFF the way saveGTiff does (process_full_tiles.py:481-531): LZW, PREDICTOR=2,
    nodata tag, geotransform / projection taken from ``meta`` (as returned by ``read_geotiff``).

    ``encoder="host"`` (default) differences and encodes the strips on the host.  ``encoder="device"`` does both on the
    GPU (msr_lzw_encode_strips) and writes the same file byte for byte: ``data`` is a NumPy array or a CUDA tensor (converted
    to ``dtype`` on the device), ``device`` the HIP device (default: the tensor's, else the current one), and the raster
    goes through the device in bands of whole strips of at most ``band_bytes`` raw bytes.  LZW only; no CPU fallback.
    ``transfers``: encode_strips'.

    ``predictor=3`` (float32 or float64 data; ValueError for an integer ``dtype``) is the floating-point predictor of TIFF
    Technical Note 3, GDAL's PREDICTOR=3: every row of a strip or padded tile goes through ``fp_predictor_reference`` in place of
    the horizontal differencing, in every layout below, and every IFD carries Predictor = 3.  Both encoders write the same
    bytes; the device encoder takes float32 only (msr_tiff_encode_strips / msr_tiff_encode_blocks).  ``read_geotiff`` reads
    these files with ``decoder="host"``; its ``decoder="device"`` refuses predictor 3.  ``compress="none"`` forces predictor 1.

    ``tile=(tile_h, tile_w)`` (positive multiples of 16) writes tiles in row-major order instead of strips: TileWidth /
    TileLength / TileOffsets / TileByteCounts and no strip tag; an edge tile is padded with zero bytes before the predictor,
    which restarts on every tile row; everything else as without it.  ``overviews=n > 0`` (needs ``tile``; at most
    ceil(log2(max(rows, cols))); float32, uint8 or uint16 files) adds n reduced-resolution levels, level k the
    ``overview_reference`` of level k - 1 with this ``nodata``: each an IFD of its own chained behind the main one, with
    NewSubfileType = 1, the nodata tag, the main IFD's tile size, compression, predictor and sample format, and no geo tags.
    File order: header, the tiles of level 0, 1 ... n, then the IFDs in order, each followed by its out-of-line values — GDAL's
    convention for internal overviews.  Both encoders write the same bytes; on the device the levels are reduced there too
    (msr_overview_half; _device_levels).  ``read_geotiff(overview=k)`` reads level k.  With the defaults, None and 0, the file
    is the one written before these keywords existed.

    ``layout="cog"`` (needs ``tile``; default "plain": everything above) writes the same tiles, levels and tags in the order of a
    cloud-optimised GeoTIFF, so that a reader finds all it needs at the front of the file: the header, a 183-byte ASCII block
    that names the organisation (COG_GHOST) and a zero byte; the IFD of level 0 at offset 192 (BigTIFF: 200) followed by its
    out-of-line values except TileOffsets / TileByteCounts, then the IFDs of levels 1 .. n in the same way, chained as above; the
    TileOffsets and TileByteCounts arrays of all levels in IFD order; then the tiles, level n (the smallest) first and level 0
    last, row-major inside a level, each as its length (4 bytes, little-endian), the payload TileOffsets points at, the
    payload's last 4 bytes once more, and a pad byte where the next payload would start odd.  These rules restate the file
    organisation of GDAL's COG driver and are not checked against GDAL here.  Both encoders write the same bytes; on the device
    the tiles are encoded where their level lies, those of all reduced levels in one launch (_device_levels_in_place), and
    ``transfers`` gets one "tile tables" entry per encode launch.  ``read_geotiff`` follows the IFD chain and reads either
    layout."""
    dt, comp, predictor = _checked_format(dtype, compress, predictor, encoder)
    if data.ndim != 2:
        raise ValueError("Data must be a 2-D array (the reference raises for rank != 2 too, process_full_tiles.py:505-519).")
    rows, cols = data.shape
    tile, overviews = check_layout(tile, overviews, (rows, cols), dt)
    check_file_order(layout, tile)
    rps = None
    if tile is None:
        rps = _rows_per_strip(rows, cols * dt.itemsize)
        levels = [(rows, cols, encode_strips(data, dt, rps, compress, predictor, encoder, device, band_bytes, transfers))]
    elif encoder == "device":
        levels = (_device_levels_in_place if layout == "cog" else _device_levels)(data, dt, tile, overviews, nodata, predictor,
                                                                                  device, band_bytes, transfers)
    else:
        levels = _host_levels(np.ascontiguousarray(data, dtype=dt), dt, tile, overviews, nodata, comp, predictor)
    _write_container(path, levels, dt, rps, tile, comp, predictor, meta, nodata, bigtiff, layout)


# What a cloud-optimised file says about its own organisation, straight behind the header (write_geotiff(layout="cog")): the
# first line gives the length of the rest, and the block ends in one space.
COG_GHOST = (b"GDAL_STRUCTURAL_METADATA_SIZE=000140 bytes\n"
             b"LAYOUT=IFDS_BEFORE_DATA\nBLOCK_ORDER=ROW_MAJOR\nBLOCK_LEADER=SIZE_AS_UINT4\n"
             b"BLOCK_TRAILER=LAST_4_BYTES_REPEATED\nKNOWN_INCOMPATIBLE_EDITION=NO\n ")


def _pack_ifd(entries: dict, ifd_off: int, big: bool, last: bool, elsewhere: Optional[dict] = None) -> bytes:
    """The IFD of ``entries`` = {tag: (type, count, raw bytes)} for file offset ``ifd_off``, followed by its out-of-line values on
    word boundaries.  ``elsewhere`` = {tag: file offset}: out-of-line values the caller writes there, not behind the IFD.  The
    IFD points to the position behind the values, which is padded to a word boundary, or with ``last`` ends the chain."""
    off_t = "Q" if big else "I"
    esz, vsz = (20, 8) if big else (12, 4)
    tags = sorted(entries)
    extra_off = ifd_off + (8 if big else 2) + len(tags) * esz + (8 if big else 4)
    ifd = bytearray(struct.pack("<Q" if big else "<H", len(tags)))
    extra = bytearray()
    for tag in tags:
        typ, cnt, raw = entries[tag]
        ifd += struct.pack("<HH", tag, typ) + struct.pack("<" + off_t, cnt)
        if len(raw) <= vsz:
            ifd += raw.ljust(vsz, b"\0")
        elif elsewhere and tag in elsewhere:
            ifd += struct.pack("<" + off_t, elsewhere[tag])
        else:
            if len(extra) & 1:
                extra += b"\0"
            ifd += struct.pack("<" + off_t, extra_off + len(extra))
            extra += raw
    if not last and len(extra) & 1:
        extra += b"\0"                                           # the next IFD starts on a word boundary
    ifd += struct.pack("<" + off_t, 0 if last else extra_off + len(extra))
    return bytes(ifd + extra)


def _write_container(path: str, levels: list, dt: np.dtype, rps: Optional[int], tile: Optional[Tuple[int, int]], comp: int,
                     predictor: int, meta: Optional[dict], nodata: Optional[float], bigtiff: Optional[bool],
                     layout: str = "plain") -> None:
    """The TIFF around the encoded blocks of ``levels`` = [(rows, cols, blocks), ...], the raster first and then its reduced
    levels; classic or BigTIFF by size.  The blocks are strips of ``rps`` rows (``tile`` None; one level) or tiles of
    ``tile`` = (tile_h, tile_w) in row-major order.  The first IFD carries the geo tags; the others NewSubfileType = 1; all
    of them the nodata tag.  ``layout="plain"``: header, the blocks level after level, then one IFD per level, each followed by
    its out-of-line values and chained to the next.  ``layout="cog"`` (tiles): header, COG_GHOST and a zero byte, the same IFDs
    with their values but the offset and count arrays, those arrays in IFD order, then the tiles from the last level to the
    first, each between its length and a repeat of its last four bytes (write_geotiff)."""
    n_blocks = sum(len(blocks) for _, _, blocks in levels)
    total = sum(len(b) for _, _, blocks in levels for b in blocks)
    geo = dict((meta or {}).get("geo", {}))
    cog = layout == "cog"
    big = (total + 8 * n_blocks * (3 if cog else 2) + sum(len(v[2]) for v in geo.values()) + 4096 * len(levels)
           + (256 if cog else 0) > 0xFFFF0000)                   # cog: 8 more bytes frame every tile
    if bigtiff is not None:
        big = bool(bigtiff)
    off_t = "Q" if big else "I"
    vsz = 8 if big else 4
    pos = 16 if big else 8
    ifds = []
    for k, (rows, cols, blocks) in enumerate(levels):
        entries = {
            256: (4, 1, struct.pack("<I", cols)), 257: (4, 1, struct.pack("<I", rows)),
            258: (3, 1, struct.pack("<H", dt.itemsize * 8)), 259: (3, 1, struct.pack("<H", comp)),
            262: (3, 1, struct.pack("<H", 1)), 277: (3, 1, struct.pack("<H", 1)),
            284: (3, 1, struct.pack("<H", 1)),
            339: (3, 1, struct.pack("<H", {"u": 1, "i": 2, "f": 3}[dt.kind])),
        }
        if k:
            entries[254] = (4, 1, struct.pack("<I", 1))          # NewSubfileType: a reduced-resolution version
        if predictor != 1:
            entries[317] = (3, 1, struct.pack("<H", predictor))
        for tag, v in (geo.items() if k == 0 else ()):
            typ, cnt, raw = v
            if (meta or {}).get("byteorder", "<") == ">" and _TYPE_SIZE.get(typ, 1) > 1:
                w = _TYPE_SIZE[typ] if typ not in (5, 10) else 4
                raw = np.frombuffer(raw, np.dtype(f">u{w}")).astype(np.dtype(f"<u{w}")).tobytes()
            entries[tag] = (typ, cnt, raw)
        if nodata is not None:
            txt = (repr(float(nodata)) if float(nodata) != int(nodata) else str(int(nodata))).encode() + b"\0"
            entries[GDAL_NODATA] = (2, len(txt), txt)
        n = len(blocks)
        if tile is None:
            entries[278] = (4, 1, struct.pack("<I", rps))
            tag_off, tag_cnt = 273, 279
        else:
            entries[322] = (4, 1, struct.pack("<I", tile[1]))
            entries[323] = (4, 1, struct.pack("<I", tile[0]))
            tag_off, tag_cnt = 324, 325
        entries[tag_off] = (16 if big else 4, n, bytes(vsz * n))     # set below, where the layout has placed the blocks
        entries[tag_cnt] = (16 if big else 4, n, struct.pack("<" + off_t * n, *(len(b) for b in blocks)))
        ifds.append(entries)

    def place(k: int, frame: int) -> None:
        """Level k's blocks from ``pos`` on, each on a word boundary with ``frame`` bytes in front and behind."""
        nonlocal pos
        offsets = []
        for b in levels[k][2]:
            offsets.append(pos + frame)
            pos += 2 * frame + len(b) + (len(b) & 1)
        ifds[k][tag_off] = ifds[k][tag_off][:2] + (struct.pack("<" + off_t * len(offsets), *offsets),)

    header = (lambda first: b"II" + (struct.pack("<HHHQ", 43, 8, 0, first) if big else struct.pack("<HI", 42, first)))
    if not cog:
        for k in range(len(levels)):
            place(k, 0)
        first_ifd = pos
        tail = bytearray()
        for k, entries in enumerate(ifds):
            tail += _pack_ifd(entries, pos, big, k == len(ifds) - 1)
            pos = first_ifd + len(tail)
        with open(path, "wb") as f:
            f.write(header(first_ifd))
            for _, _, blocks in levels:
                for b in blocks:
                    f.write(b)
                    if len(b) & 1:
                        f.write(b"\0")
            f.write(bytes(tail))
        return
    # cog.  The size of an IFD and of the values behind it does not depend on the offsets it holds, so the IFDs are laid out
    # with the arrays of zeros first, then the arrays and the tiles, and packed once the tiles have their places.
    first_ifd = pos = pos + len(COG_GHOST) + 1
    ifd_offs, arrays = [], []
    for k, entries in enumerate(ifds):
        ifd_offs.append(pos)
        later = dict.fromkeys((t for t in (tag_off, tag_cnt) if len(entries[t][2]) > vsz), 0)
        pos += len(_pack_ifd(entries, pos, big, k == len(ifds) - 1, later))
        pos += pos & 1
        arrays.append(later)
    for k, later in enumerate(arrays):               # the arrays of all levels behind the last IFD, in IFD order
        for t in later:
            later[t] = pos
            pos += len(ifds[k][t][2])
            pos += pos & 1
    for k in reversed(range(len(levels))):           # the smallest level first
        # a tile of 16 x 16 samples or more has a stream of more than 4 bytes: the trailer repeats whole bytes of it
        assert all(len(b) >= 4 for b in levels[k][2]), "a tile payload under 4 bytes"
        place(k, 4)
    with open(path, "wb") as f:
        f.write(header(first_ifd) + COG_GHOST + b"\0")
        for k, (entries, later) in enumerate(zip(ifds, arrays)):
            ifd = _pack_ifd(entries, ifd_offs[k], big, k == len(ifds) - 1, later)
            f.write(ifd + b"\0" * (len(ifd) & 1))
        for k, later in enumerate(arrays):
            for t in later:
                f.write(ifds[k][t][2] + b"\0" * (len(ifds[k][t][2]) & 1))
        for k in reversed(range(len(levels))):
            for b in levels[k][2]:
                f.write(struct.pack("<I", len(b)) + b + b[-4:] + b"\0" * (len(b) & 1))


def geotransform(meta: dict) -> Optional[Tuple[float, float, float, float, float, float]]:
    """GDAL-style geotransform (x0, dx, 0, y0, 0, -dy) from ModelTiepoint + ModelPixelScale, if present."""
    geo = meta.get("geo", {})
    if 33550 not in geo or 33922 not in geo:
        return None
    bo = meta.get("byteorder", "<")
    sx, sy, _ = struct.unpack(bo + "3d", geo[33550][2][:24])
    i, j, _, x, y, _ = struct.unpack(bo + "6d", geo[33922][2][:48])
    return (x - i * sx, sx, 0.0, y + j * sy, 0.0, -sy)

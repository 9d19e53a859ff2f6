"""Shared by tests/test_geotiff_pred3_host.py and tests/test_gpu_geotiff_pred3.py: the rasters and layouts of the predictor-3
files, the blocks the in-place encoder is checked on, and the bytes the encoder has to see, built with the NumPy twin
(geotiff.fp_predictor_reference).  Everything is compared for equal bits or bytes; every reference is computed once."""
import functools
from typing import NamedTuple

import numpy as np

from moonsuperresolution_amd import geotiff as G

NOVAL = -32768.0
CANARY = 64
# (name, shape, keywords of write_geotiff): strips, tiles, and the cloud-optimised order with two reduced levels
LAYOUTS = [("strips", (17, 33), {}), ("tiles", (17, 33), {"tile": (16, 16)}),
           ("cog", (40, 70), {"tile": (16, 32), "overviews": 2, "layout": "cog"})]
# the four values whose arithmetic differs between processors when two of them meet in a sum; then those that are harmless
LONELY = (0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000)       # two NaNs with payloads, +Inf, -Inf
ANYWHERE = (0x00000000, 0x80000000, 0x00000001, 0x807FFFFF)     # +0, -0, the smallest and the largest denormal (negative)


@functools.lru_cache(None)
def raster(shape) -> np.ndarray:
    """Smooth float32 terrain in quarter metres with a no-data corner and the special values: each of LONELY alone in an 8 x 8
    block of its own (aligned to 8, so that two reduced levels never add two of them), the others beside them, in the last
    column and in the last row."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    a = (np.cumsum(rng.integers(-3, 4, shape), axis=1) * 0.25 - 2000.0).astype(np.float32)
    a[h // 2:h // 2 + 3, :5] = NOVAL
    u = a.view(np.uint32)
    slots = [(r, c) for r in range(1, h, 8) for c in range(2, w, 8)]
    assert len(slots) >= len(LONELY) + len(ANYWHERE)
    for (r, c), v in zip(slots, LONELY + ANYWHERE):
        u[r, c] = v
    u[h - 1, w - 1] = ANYWHERE[1]
    u[h - 1, 0] = ANYWHERE[2]
    u[0, w - 1] = ANYWHERE[3]
    a.setflags(write=False)
    return a


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(None)
def levels(shape, n: int) -> tuple:
    """(level 0, ..., level n) of ``raster(shape)`` by the twin of the reduction, with the nodata rule of write_geotiff."""
    out = [raster(shape)]
    for _ in range(n):
        out.append(G.overview_reference(out[-1], NOVAL))
        out[-1].setflags(write=False)
    return tuple(out)


_FILES = {}


def host_file(tmp_path_factory, name: str) -> bytes:
    """The host writer's predictor-3 file of layout ``name``, written once per process."""
    if name not in _FILES:
        _, shape, how = next(x for x in LAYOUTS if x[0] == name)
        path = str(tmp_path_factory.mktemp("pred3") / f"{name}.tif")
        G.write_geotiff(path, raster(shape), nodata=NOVAL, predictor=3, **how)
        _FILES[name] = open(path, "rb").read()
    return _FILES[name]


# ---- strips ------------------------------------------------------------------------------------------------------------------
# (rows, samples in a row, rows in a strip): planes shorter than a chunk of 256 bytes and several rows in a chunk; a row of
# exactly one chunk; one sample more; planes longer than a chunk; rows over 64 KiB, one in a strip; a last strip that is shorter
STRIPS = [(3, 33, 3), (3, 64, 3), (3, 65, 3), (3, 257, 3), (3, 16400, 1), (17, 33, 5)]


@functools.lru_cache(None)
def strip_source(rows: int, w: int) -> np.ndarray:
    rng = np.random.default_rng(rows * 100000 + w)
    a = (np.cumsum(rng.integers(-3, 4, (rows, w)), axis=1) * 0.25 - 2000.0).astype(np.float32)
    u = a.view(np.uint32)
    u[0, 0], u[rows - 1, w - 1], u[rows // 2, w // 2] = LONELY[0], LONELY[3], ANYWHERE[2]
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def strip_streams(rows: int, w: int, rps: int) -> tuple:
    """msr_lzw_encode of the twin's bytes of every strip."""
    a = strip_source(rows, w)
    return tuple(G.lzw_encode(G.fp_predictor_reference(a[r:r + rps])) for r in range(0, rows, rps))


# ---- blocks ------------------------------------------------------------------------------------------------------------------
BLOCK_RASTER = (40, 70)
BLOCK_PITCH = 75 * 4            # larger than a row of the raster
BLOCK_SIZES = [(16, 16), (32, 48), (48, 32)]       # (rows, samples in a row)


class Block(NamedTuple):
    """A block of ``bh`` rows of ``bw`` samples whose valid part, ``vr`` rows of ``vw`` samples, begins at sample (y0, x0) of
    the raster ``src`` ([rows, pitch / 4] float32, of which the first BLOCK_RASTER[1] columns are the raster)."""
    name: str
    y0: int
    x0: int
    vr: int
    vw: int
    bh: int
    bw: int


@functools.lru_cache(None)
def block_raster() -> np.ndarray:
    """BLOCK_RASTER at BLOCK_PITCH: raster() in the first 70 columns, another value behind every row (never to be read)."""
    rows, cols = BLOCK_RASTER
    a = np.full((rows, BLOCK_PITCH // 4), 12345.678, np.float32)
    a[:, :cols] = raster(BLOCK_RASTER)
    a.setflags(write=False)
    return a


def blocks(bh: int, bw: int) -> tuple:
    """The valid parts: one sample, a full block, 17 columns (of 32: a half-empty edge tile), no row, the raster's last row
    only; each where it lies in the raster."""
    rows, cols = BLOCK_RASTER
    part = [("1x1", rows - 1, cols - 1, 1, 1), ("full", 3, 5, min(bh, rows - 3), bw), ("17-columns", 0, cols - 17, min(bh, rows), 17),
            ("no-row", 0, 0, 0, bw), ("last-row", rows - 1, 7, 1, bw)]
    return tuple(Block(f"{bh}x{bw}-{name}", y0, x0, vr, min(vw, bw), bh, bw) for name, y0, x0, vr, vw in part)


def padded(b: Block, src: np.ndarray = None) -> np.ndarray:
    """The bytes the encoder has to see: the valid part in a zero block, then the twin."""
    src = block_raster() if src is None else src
    blk = np.zeros((b.bh, b.bw), np.float32)
    blk[:b.vr, :b.vw] = src[b.y0:b.y0 + b.vr, b.x0:b.x0 + b.vw]
    return G.fp_predictor_reference(blk).reshape(-1)


_STREAMS = {}


def stream(b: Block) -> bytes:
    """The host encoder's stream of the padded block, computed once (the names are unique)."""
    if b.name not in _STREAMS:
        _STREAMS[b.name] = G.lzw_encode(padded(b))
    return _STREAMS[b.name]


def host_entry(lib, src: np.ndarray, offset: int, pitch: int, b: Block, predictor: int = 3, cap: int = None):
    """msr_tiff_encode_block_host on block ``b`` whose first sample is byte ``offset`` of ``src``: the stream, or the entry's
    negative result."""
    n = b.bh * b.bw * 4
    cap = n + n // 2 + 1024 if cap is None else cap
    out = np.full(cap + CANARY, 0xA5, np.uint8)
    raw = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
    got = lib.msr_tiff_encode_block_host(raw.ctypes.data + offset, pitch, b.vw * 4, b.vr, b.bw * 4, b.bh, 4, predictor,
                                         out.ctypes.data, cap)
    assert (out[cap:] == 0xA5).all(), "a byte at or beyond cap was written"
    return out[:got].tobytes() if got >= 0 else got

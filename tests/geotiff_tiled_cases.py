"""Shared by tests/test_geotiff_tiled_host.py and tests/test_gpu_geotiff_tiled.py: the rasters, the file cases and the twin's
chain of reduced levels (each computed once per process and never modified), and the rasters the reduction itself is checked
on.  Everything is compared for equal bits or bytes."""
import functools

import numpy as np

from moonsuperresolution_amd import geotiff as G

NOVAL = -32768.0
CANARY = 64
# (shape, tile): the issue's list — (40, 9) only with tile_w 32, every other shape with both tiles
LAYOUTS = [((70, 101), (16, 16)), ((70, 101), (16, 32)), ((16, 16), (16, 16)), ((16, 16), (16, 32)), ((17, 33), (16, 16)),
           ((17, 33), (16, 32)), ((1, 1), (16, 16)), ((1, 1), (16, 32)), ((40, 9), (16, 32))]
FORMATS = [("float32", 1), ("float32", 2), ("uint16", 2), ("uint8", 2)]           # (file dtype, predictor)
REDUCE_SHAPES = [(1, 1), (2, 2), (3, 5), (71, 101), (64, 257), (130, 66)]


def most_overviews(shape) -> int:
    return (max(shape) - 1).bit_length()                     # ceil(log2(max(rows, cols)))


@functools.lru_cache(None)
def raster(shape, dtype: str) -> np.ndarray:
    """Smooth, quantised terrain with a no-data pattern (float32) or small counts (integers): it compresses, and the
    reduced levels meet blocks with 0 .. 4 counting pixels."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    if dtype == "float32":
        a = (np.cumsum(rng.integers(-3, 4, shape), axis=1) * 0.25 - 2000.0).astype(np.float32)
        a[rng.random(shape) < 0.45] = NOVAL
    else:
        a = rng.integers(0, 4 if dtype == "uint8" else 300, shape).astype(dtype)
        a[rng.random(shape) < 0.5] = 0
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def chain(shape, dtype: str, n: int) -> tuple:
    """(level 0, ..., level n) by the twin, with the nodata rule write_geotiff applies (float files only)."""
    levels = [raster(shape, dtype)]
    for _ in range(n):
        levels.append(G.overview_reference(levels[-1], NOVAL if dtype == "float32" else None))
        levels[-1].setflags(write=False)
    return tuple(levels)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.dtype(f"u{a.dtype.itemsize}"))


@functools.lru_cache(None)
def reduce_input(shape, kind: str) -> np.ndarray:
    """What the reduction is checked on.  "nodata": float32 where every count 0 .. 4 occurs (the first 2 x 2 blocks are set by
    hand where the shape has room), with NaNs, +0.0 and -0.0, values of mixed magnitude so that the order of the sum shows;
    "plain": float32 without any no-data value; "u8" / "u16": integers."""
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] + len(kind))
    if kind in ("u8", "u16"):
        a = rng.integers(0, 256 if kind == "u8" else 65536, shape).astype(np.uint8 if kind == "u8" else np.uint16)
    else:
        a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 8, shape)).astype(np.float32)
        a[rng.random(shape) < 0.08] = np.nan
        a[rng.random(shape) < 0.08] = 0.0
        a[rng.random(shape) < 0.08] = -0.0
        if kind == "nodata":
            a[rng.random(shape) < 0.5] = NOVAL
            for n in range(5):                                # block (0, n): exactly n counting pixels
                if shape[0] >= 2 and shape[1] >= 2 * n + 2:
                    a[0:2, 2 * n:2 * n + 2] = np.where(np.arange(4) < 4 - n, NOVAL, 1.5 + n).astype(np.float32).reshape(2, 2)
    a.setflags(write=False)
    return a


def reduce_cases():
    """[(shape, kind, has_nodata)] of the reduction tests."""
    return [(s, k, k == "nodata") for s in REDUCE_SHAPES for k in ("nodata", "plain", "u8", "u16")]


def counts_of(a: np.ndarray) -> set:
    """The numbers of counting pixels that occur among the 2 x 2 blocks of a float raster with NOVAL as no-data."""
    rows, cols = a.shape
    c = np.zeros((-(-rows // 2) * 2, -(-cols // 2) * 2), np.int32)
    c[:rows, :cols] = a != np.float32(NOVAL)
    return set(np.unique(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]).tolist())

"""Shared by tests/test_geotiff_bytes_pinned.py and tests/test_gpu_geotiff_tiled.py: the files whose bytes, and whose rasters
as read back, are pinned by SHA-256 in tests/golden/geotiff_bytes.json.  Each case is there because a branch of the writer
depends on it; the inputs are the deterministic rasters of tests/geotiff_tiled_cases.py."""
import hashlib
import json
import os
import struct

import numpy as np

from moonsuperresolution_amd import geotiff as G
from tests import geotiff_tiled_cases as tiled

NV = tiled.NOVAL
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geotiff_bytes.json")
ROWS = (3, 11)                                   # the row window read back where the raster has that many rows

# a meta as read_geotiff returns it for a big-endian file: the writer swaps every value of the geo tags (doubles, shorts;
# ASCII stays)
BIG_ENDIAN_META = {"byteorder": ">", "geo": {
    33550: (12, 3, struct.pack(">3d", 2.0, 2.0, 0.0)),
    33922: (12, 6, struct.pack(">6d", 0.0, 0.0, 0.0, 1000.5, -2000.25, 0.0)),
    34735: (3, 16, struct.pack(">16H", 1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2049, 34737, 7, 0)),
    34737: (2, 8, b"WGS 84|\0")}}


def _case(name, shape, raster_dtype, meta=None, **kw):
    kw.setdefault("nodata", NV)
    kw.setdefault("dtype", raster_dtype)
    return name, shape, raster_dtype, meta, kw


_TILED_FORMATS = [(f"{d}-p{p}", d, p) for d, p in tiled.FORMATS]
# (name, raster shape, raster dtype, meta, keywords of write_geotiff)
CASES = [
    _case("strips-f32-p2-last-short", (70, 257), "float32"),
    _case("strips-u16-p2", (70, 101), "uint16"),
    _case("strips-u8-into-u16", (70, 101), "uint8", dtype="uint16"),
    _case("strips-f32-p1-none", (17, 33), "float32", predictor=1, compress="none"),
    _case("strips-f32-p1-deflate", (17, 33), "float32", predictor=1, compress="deflate"),
    _case("strips-f64-drops-p2", (17, 33), "float32", dtype="float64"),
    _case("strips-1x1", (1, 1), "float32"),
    *[_case(f"tiles-16x32-{f}-ov{n}", (70, 101), d, predictor=p, tile=(16, 32), overviews=n)
      for f, d, p in _TILED_FORMATS for n in (0, 2)],
    _case("tiles-16x16-17x33-ov2", (17, 33), "float32", tile=(16, 16), overviews=2),
    _case("tiles-16x16-1x1", (1, 1), "float32", tile=(16, 16)),
    _case("bigtiff-strips", (70, 101), "float32", bigtiff=True),
    _case("bigtiff-tiles-ov2", (70, 101), "float32", bigtiff=True, tile=(16, 32), overviews=2),
    _case("big-endian-meta-strips", (70, 101), "float32", BIG_ENDIAN_META),
    _case("big-endian-meta-tiles-ov2", (70, 101), "uint16", BIG_ENDIAN_META, tile=(16, 32), overviews=2),
    _case("nodata-half", (17, 33), "float32", nodata=0.5),
    _case("nodata-none-strips", (17, 33), "float32", nodata=None),
    _case("nodata-none-tiles-ov2", (17, 33), "float32", nodata=None, tile=(16, 16), overviews=2),
]
IDS = [c[0] for c in CASES]
LZW_CASES = [c for c in CASES if c[4].get("compress", "lzw") == "lzw"]          # what the device encoder takes


def sha(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def write(path: str, case, data=None, **more) -> None:
    """The file of ``case`` (from ``data`` instead of the case's raster where given; ``more``: encoder, band_bytes ...)."""
    _, shape, raster_dtype, meta, kw = case
    G.write_geotiff(path, tiled.raster(shape, raster_dtype) if data is None else data, meta, **kw, **more)


def reads(case) -> list:
    """[(key of the digest, keywords of read_geotiff)] of the reads pinned for ``case``."""
    out = [("read", {})]
    if case[1][0] >= ROWS[1]:
        out.append((f"rows_{ROWS[0]}_{ROWS[1]}", {"rows": ROWS}))
    return out + [(f"overview_{k}", {"overview": k}) for k in range(1, case[4].get("overviews", 0) + 1)]


def digests(path: str, case, **more) -> dict:
    """The digest of the file at ``path`` and of every pinned read of it (``more``: decoder ...)."""
    out = {"file": sha(open(path, "rb").read())}
    for key, kw in reads(case):
        out[key] = sha(np.ascontiguousarray(G.read_geotiff(path, **kw, **more)[0]).tobytes())
    return out


def pinned() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)

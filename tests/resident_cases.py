"""Inputs shared by the resident-raster and rank-0-writer tests (tests/test_gpu_resident.py, tests/test_gpu_products_rank0.py,
their host twins and the two-rank worker): small rasters that compress, with holes around the in-fill limits.

The driver's smallest configuration: S = 64, stride 16, B = 4, T = 128.  A 300-row raster is three tile rows, so two ranks own
two and one; 256 columns give strips of 64 (float32) and 128 (uint16) rows, which divide T; 300 columns give 54 and 109, which
do not.  Both rasters are quantised (DEM to 1/4 m, ortho to 1/64), so the LZW files are well below the raw size.
"""
import os

import numpy as np

NOVAL = -32768.0
S, STRIDE, B, T = 64, 16, 4, 128
SHAPES = {"wide": (300, 256), "square": (272, 272), "odd": (300, 300)}


def f32_identity(x, training=False):
    return np.asarray(x, np.float32)


def cfg(**kw):
    from moonsuperresolution_amd import DSRConfig
    return DSRConfig(image_size=S, stride=STRIDE, batch_size=B, tile_size=T, **kw)


def raster(shape, seed=0):
    """(ortho, DEM): smooth, quantised terrain; a large no-data corner in both; in the ortho holes of 1, 2, 3, 5 and 7 pixels
    (under the limit of 8) and one of 8 (at it: stays) where its in-fill can write (128 pixels from every edge); in the DEM
    4 x 4 blocks that become, on the x1/4 grid, single pixels, a pair, a row of 23 (under the limit of 24) and a row of 24 (at
    it: stays) across the columns the x1/4 in-fill can write (32 from every edge)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    dem = -2000.0 + 0.3 * xx + 0.2 * yy + 5.0 * np.sin(xx / 17.0) * np.cos(yy / 23.0)
    dem = (np.round(dem * 4.0) / 4.0).astype(np.float32)
    img = 0.5 + 0.4 * np.sin(xx / 29.0) * np.sin(yy / 31.0) + 0.02 * rng.integers(0, 3, shape)
    img = (np.round(img * 64.0) / 64.0).astype(np.float32)

    def quarter(r, c0, c1):                             # x1/4-grid pixels (r, c0 .. c1 - 1)
        dem[4 * r:4 * r + 4, 4 * c0:4 * c1] = NOVAL
    quarter(33, 20, 43)                                 # 23 pixels
    quarter(35, 20, 44)                                 # 24 pixels
    quarter(38, 33, 34)
    quarter(40, 33, 35)
    quarter(38, 37, 38)
    r = 130
    for n, c in ((1, 129), (2, 132), (3, 136), (5, 141)):
        img[r, c:c + n] = NOVAL
    img[133, 129:136] = NOVAL                           # 7
    img[136, 129:137] = NOVAL                           # 8
    img[139:141, 130] = NOVAL
    dem[:40, :50] = NOVAL
    img[:40, :50] = NOVAL
    return img, dem


def write_inputs(folder, shape, seed=0):
    """run-DRG.tif / run-DEM.tif of ``raster(shape, seed)`` in ``folder`` (LZW, predictor 2); returns (ortho, DEM)."""
    from moonsuperresolution_amd import geotiff as G
    img, dem = raster(shape, seed)
    os.makedirs(folder, exist_ok=True)
    G.write_geotiff(os.path.join(folder, "run-DRG.tif"), img, nodata=NOVAL)
    G.write_geotiff(os.path.join(folder, "run-DEM.tif"), dem, nodata=NOVAL)
    return img, dem


def product_bytes(folder, map_name="m"):
    """The three product files of a run, as bytes, or None for one that was not written."""
    out = {}
    for name in ("mean", "std", "good"):
        path = os.path.join(folder, f"{map_name}_{name}.tiff")
        out[name] = open(path, "rb").read() if os.path.exists(path) else None
    return out

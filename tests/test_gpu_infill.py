"""GPU (-m gpu): the device in-filling (csrc/infill.hip, preprocess(infill="device")) against its NumPy twin, bit for bit.

  * msr_infill_small_holes equals infill.infill_reference through the uint32 view, with a guard row either side of the buffer
    that keeps its pattern: the 330 x 300 grid at (24, 32), the ortho grid at (8, 128), a 96 x 1100 grid whose components sit
    where the label stage's 64-pixel words and 4-row workgroups meet, at (24, 32) and at the largest max_area (32, 33)
    (tests/infill_cases.py);
  * on the d4 band of preprocess.window_plan, with row0 and full_rows set, the plan's fill rows equal the whole grid's
    (the 3210 x 406 raster of tests/test_gpu_preprocess_window.py: x1/4 grid 802 x 102);
  * preprocess(swap_dsize=False, infill="device") equals the composition oracle area -> twin -> oracle area -> oracle cubic with
    the oracle's no-data marking between the steps, and its in-filled ortho equals the twin at (8, 128), in one band and in six;
  * preprocess(rows=, infill="device") equals the same rows of the whole-raster device result;
  * with scipy.interpolate.griddata and scipy.ndimage.label patched to raise, the device path still runs;
  * processFiles(preprocess=True, swap_dsize=False) of a driver with infill="device" writes, byte for byte, the files of a run
    from setImages(img, composed DEM).
All comparisons are exact.
"""
import os

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import geotiff as G
from moonsuperresolution_amd import infill
from moonsuperresolution_amd import preprocess as pp
from oracle import preprocess_ref as pr
from tests import infill_cases as cases

pytestmark = pytest.mark.gpu
NOVAL = cases.NOVAL
SHAPE = (3210, 406)                                   # x1/4 grid 802 x 102
S, STRIDE, B, T = 64, 32, 16, 128
WINDOWS = [(0, 700), (1000, 1700), (2400, 3210), (1500, 1505)]
DRIVER_SHAPE = (1030, 406)
GUARD = 123456.0


def f32_identity(x, training=False):
    return np.asarray(x, np.float32)


def _cfg(**kw):
    from moonsuperresolution_amd import DSRConfig
    return DSRConfig(image_size=S, stride=STRIDE, batch_size=B, tile_size=T, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(hip_lib):
    from moonsuperresolution_amd import ops
    return ops.OpContext()


def device_fill(ctx, grid, area, margin, row0=0, full_rows=None):
    """msr_infill_small_holes on a copy of ``grid`` that lies between two guard rows; the guards must keep their pattern."""
    n, w = grid.shape
    buf = torch.full((n + 2, w), GUARD, dtype=torch.float32, device="cuda")
    buf[1:-1] = torch.from_numpy(np.ascontiguousarray(grid)).cuda()
    infill.infill_device(ctx.lib, ctx.h, buf[1:-1], row0, n if full_rows is None else full_rows, NOVAL, area, margin)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[0] == GUARD).all() and (out[-1] == GUARD).all()
    return out[1:-1]


# ---- kernel against twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,area,margin", [("grid_330x300", 24, 32), ("grid_ortho", 8, 128), ("grid_96x1100", 24, 32),
                                              ("grid_96x1100", 32, 33), ("grid_96x1100", 2, 3)])
def test_kernel_equals_the_twin_bit_for_bit(ctx, name, area, margin):
    grid = getattr(cases, name)()[0]
    want = infill.infill_reference(grid, NOVAL, area, margin)
    take = infill.fill_set(grid, NOVAL, area, margin)
    assert take.sum() >= 3 and (bits(want) != bits(grid)).sum() == take.sum()
    got = device_fill(ctx, grid, area, margin)
    diff = bits(got) != bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])
    again = device_fill(ctx, got, area, margin)                # what is left is not fillable: a second pass changes nothing
    assert np.array_equal(bits(again), bits(got))


def test_nan_is_a_hole_and_none_is_written(ctx):
    grid = cases.grid_330x300()[0].copy()
    grid[100, 200] = grid[101, 201] = grid[60, 49] = np.nan           # a pair of its own; one that makes line23 a line24
    want = infill.infill_reference(grid, NOVAL, 24, 32)
    got = device_fill(ctx, grid, 24, 32)
    assert not np.isnan(got[100, 200]) and not np.isnan(got[101, 201]) and np.isnan(got[60, 49]) and got[60, 50] == NOVAL
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(np.nan_to_num(got)), bits(np.nan_to_num(want)))


# ---- row windows --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quarter_grid():
    """An x1/4-sized grid (802 x 102) of the 3210 x 406 raster with 70 random holes of 1 .. 26 pixels and one of 400."""
    h4, w4 = pp._cv_round(SHAPE[0] / 4), pp._cv_round(SHAPE[1] / 4)
    g = cases.terrain(h4, w4, ripple=True).astype(np.float32)
    for pix in cases.random_holes((h4, w4), 70, np.random.default_rng(8), 1, 26, edge=0):
        for r, c in pix:
            g[r, c] = NOVAL
    g[300:320, 40:60] = NOVAL
    g.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def quarter_whole(ctx, quarter_grid):
    want = infill.infill_reference(quarter_grid, NOVAL, pp.FILL_AREA, pp.FILL_BORDER)
    got = device_fill(ctx, quarter_grid, pp.FILL_AREA, pp.FILL_BORDER)
    assert np.array_equal(bits(got), bits(want)) and (bits(got) != bits(quarter_grid)).sum() > 200
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("rows", WINDOWS)
def test_the_plans_band_gives_the_whole_grids_fill_rows(ctx, quarter_grid, quarter_whole, rows):
    plan = pp.window_plan(SHAPE, rows)
    (q0, q1), (f0, f1) = plan["d4"], plan["fill"]
    h4 = quarter_grid.shape[0]
    got = device_fill(ctx, quarter_grid[q0:q1], pp.FILL_AREA, pp.FILL_BORDER, row0=q0, full_rows=h4)
    assert np.array_equal(bits(got[f0 - q0:f1 - q0]), bits(quarter_whole[f0:f1])), rows
    assert np.array_equal(bits(got), bits(infill.infill_reference(quarter_grid[q0:q1], NOVAL, pp.FILL_AREA, pp.FILL_BORDER, q0, h4)))


# ---- preprocess ---------------------------------------------------------------------------------------------------------------
def _raster(shape, seed):
    """(ortho, DEM) with holes: the DEM's become components of 1 .. 30 pixels of the x1/4 grid, the ortho's have 1 .. 9 pixels,
    some of them on the rows where fill_ortho_device's bands of 700 rows meet (632, 1196, 1760, ...)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    dem = (-2000.0 + 0.3 * xx + 0.2 * yy + 5.0 * np.sin(xx / 17.0) * np.cos(yy / 23.0)).astype(np.float32)
    for pix in cases.random_holes((h // 4, w // 4), max(8, h // 60), rng, 1, 30, edge=0):
        for r, c in pix:
            dem[4 * r:4 * r + 4, 4 * c:4 * c + 4] = NOVAL
    dem[h // 2:h // 2 + 80, 160:240] = NOVAL                                  # 400 pixels of the x1/4 grid
    img = rng.uniform(0, 1, shape).astype(np.float32)
    for pix in cases.random_holes(shape, max(10, h // 40), rng, 1, 9, edge=110):
        for r, c in pix:
            img[r, c] = NOVAL
    for seam in range(632, h - 140, 564):
        for k, dr in enumerate((-68, -9, -1, 0, 7, 67)):
            img[seam + dr:seam + dr + 3, 140 + 20 * k] = NOVAL
            img[seam + dr, 150 + 20 * k:152 + 20 * k] = NOVAL
    return img, dem


def _composition(dem):
    """oracle area -> twin -> oracle area -> oracle cubic to the raster's own shape, with the oracle's no-data marking."""
    d = np.array(dem, np.float32, copy=True)
    d[d <= NOVAL] = np.nan
    d = pr.resize_area(d, 0.25, 0.25)
    d[np.isnan(d)] = NOVAL
    d = infill.infill_reference(d, NOVAL, pp.FILL_AREA, pp.FILL_BORDER)
    d[d <= NOVAL] = np.nan
    d = pr.resize_area(d, 0.25, 0.25)
    d = pr.resize_cubic(d, (dem.shape[1], dem.shape[0]))
    d[np.isnan(d)] = NOVAL
    return d


@pytest.fixture(scope="module")
def raster():
    return _raster(SHAPE, 3)


@pytest.fixture(scope="module")
def composed(raster):
    img, dem = raster
    image = infill.infill_reference(img, NOVAL, pp.ORTHO_AREA, pp.ORTHO_BORDER)
    assert (bits(image) != bits(img)).sum() > 100 and (image <= NOVAL).any()
    out = _composition(dem)
    assert (out == NOVAL).any()
    image.setflags(write=False)
    out.setflags(write=False)
    return image, out


@pytest.fixture(scope="module")
def whole(hip_lib, raster, composed):
    """DEMSuperResolution(infill="device").preprocess(swap_dsize=False) on the whole raster, checked against the composition."""
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    d = DEMSuperResolution(_cfg(), model=f32_identity, infill="device")
    d.setImages(img, dem)
    d.preprocess(swap_dsize=False)
    out, image = d.dem, d.image
    d.close()
    assert np.array_equal(bits(out), bits(composed[1])) and np.array_equal(bits(image), bits(composed[0]))
    out.setflags(write=False)
    return out


def test_preprocess_equals_the_composition(whole):
    assert whole.shape == SHAPE and whole.dtype == np.float32


def test_the_ortho_in_bands_equals_the_twin(ctx, raster, composed):
    img, dem = raster
    band_bytes = 4 * SHAPE[1] * 700
    image, out = pp.preprocess(ctx.lib, ctx.h, torch.device("cuda", 0), img, dem, NOVAL, swap_dsize=False, infill="device",
                               band_bytes=band_bytes)
    assert np.array_equal(bits(image), bits(composed[0])) and np.array_equal(bits(out), bits(composed[1]))
    with pytest.raises(ValueError, match="band_bytes"):
        pp.fill_ortho_device(ctx.lib, ctx.h, torch.device("cuda", 0), img, NOVAL, 4 * SHAPE[1] * 136)


@pytest.mark.parametrize("rows", WINDOWS)
def test_preprocess_rows_equals_the_rows_of_the_whole_raster(hip_lib, raster, whole, rows):
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    r0, r1 = rows
    m0, m1 = pp.window_plan(SHAPE, rows)["dem"]
    m0, m1 = min(m0, r0), max(m1, r1)
    d = DEMSuperResolution(_cfg(), model=f32_identity, infill="device")
    d.setImages(img[m0:m1].copy(), dem[m0:m1].copy(), row0=m0, full_shape=SHAPE)
    d.preprocess(swap_dsize=False, rows=rows)
    assert d.row0 == r0 and d.dem_shape == SHAPE and d.image is None
    assert np.array_equal(bits(d.dem), bits(whole[r0:r1])) and np.array_equal(d.img, img[r0:r1])
    d.close()


def test_the_device_path_makes_no_scipy_call(ctx, raster, composed, monkeypatch):
    import scipy.interpolate
    import scipy.ndimage

    def refuse(*a, **kw):
        raise AssertionError("SciPy was called on the device in-fill path")
    monkeypatch.setattr(scipy.interpolate, "griddata", refuse)
    monkeypatch.setattr(scipy.ndimage, "label", refuse)
    img, dem = raster
    image, out = pp.preprocess(ctx.lib, ctx.h, torch.device("cuda", 0), img[:1030], dem[:1030], NOVAL, swap_dsize=False,
                               infill="device")
    assert image.shape == out.shape == (1030, SHAPE[1]) and (bits(image) != bits(img[:1030])).any()
    with pytest.raises(AssertionError, match="SciPy"):                      # the host path does call it
        pp.fillNan(np.where(np.eye(300, dtype=bool), NOVAL, 1.0).astype(np.float32), NOVAL, 1024, 128, 8)


# ---- files --------------------------------------------------------------------------------------------------------------------
def test_process_files_with_the_device_infill(hip_lib, tmp_path):
    from moonsuperresolution_amd import DEMSuperResolution, HaloShardedSuperResolution
    img, dem = _raster(DRIVER_SHAPE, 4)
    src = tmp_path / "in"
    os.makedirs(src)
    G.write_geotiff(str(src / "run-DRG.tif"), img, nodata=NOVAL)
    G.write_geotiff(str(src / "run-DEM.tif"), dem, nodata=NOVAL)
    composed = _composition(dem)
    assert (bits(composed) != bits(dem)).any()
    for cls, tag in ((DEMSuperResolution, "a"), (HaloShardedSuperResolution, "b")):
        d = cls(_cfg(source_folder_path=str(src), save_path=str(tmp_path / tag), map_name="m"), model=f32_identity, infill="device")
        d.processFiles(preprocess=True, swap_dsize=False)
        assert np.array_equal(bits(d.image), bits(infill.infill_reference(img, NOVAL, pp.ORTHO_AREA, pp.ORTHO_BORDER)))
        d.close()
    ref = DEMSuperResolution(_cfg(source_folder_path=str(src), save_path=str(tmp_path / "ref"), map_name="m"), model=f32_identity)
    ref.loadImages()
    ref.setImages(ref.img, composed)
    mean, std, good = ref.processMap()
    for data, name in ((mean, "mean"), (std, "std"), (good, "good")):
        ref.saveGTiff(data, data.dtype, name)
    ref.close()
    for name in ("mean", "std", "good"):
        want = open(tmp_path / "ref" / f"m_{name}.tiff", "rb").read()
        for tag in ("a", "b"):
            assert open(tmp_path / tag / f"m_{name}.tiff", "rb").read() == want, (name, tag)

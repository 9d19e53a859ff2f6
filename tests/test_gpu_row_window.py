"""GPU (-m gpu): a rank that reads, pads and uploads only the raster rows it works on produces the bits of a rank that
holds the whole raster.

The window is a host-side matter: the kernels that read the canvas get window rows (canvas row - canvas_row0), keys and
everything downstream stay in canvas rows (tiler.padInputs).  So every comparison here is exact: the windowed instance
against an instance given the whole raster — which the existing tests check against oracle/tiler_ref.py.

Geometry: the one of tests/test_gpu_halo.py (S = 64, s = 16, B = 4, T = 128) on a 300 x 200 raster = three tile rows, with
a nodata hole over raster rows 110 .. 150: across the tile-row boundary at 128 and across the line (raster row 128 too)
where ownership passes from halo rank 0 to rank 1 of 3.
"""
import os

import numpy as np
import pytest

from moonsuperresolution_amd import distributed as D
from moonsuperresolution_amd import geotiff as G
from tests.helpers import synthetic_raster

pytestmark = pytest.mark.gpu
S, STRIDE, B, T = 64, 16, 4, 128
SHAPE = (300, 200)
HOLE = (110, 150, 60, 120)


def f32_identity(x, training=False):
    return np.asarray(x, np.float32)


def _cfg(**kw):
    from moonsuperresolution_amd import DSRConfig
    return DSRConfig(image_size=S, stride=STRIDE, batch_size=B, tile_size=T, **kw)


def _tiles_to_host(d, tiles):
    return {t: tuple(x.cpu().numpy() for x in d.processTile(*t)) for t in tiles}


def _window_instance(cls, img, dem, rows, model=f32_identity):
    """An instance that has only ever seen raster rows [r0, r1)."""
    r0, r1 = rows
    d = cls(_cfg(), model=model)
    d.setImages(img[r0:r1].copy(), dem[r0:r1].copy(), row0=r0, full_shape=img.shape)
    return d


@pytest.fixture(scope="module")
def raster():
    return synthetic_raster(SHAPE[0], SHAPE[1], seed=21, hole=HOLE)


@pytest.fixture(scope="module")
def whole_tiles(hip_lib, raster):
    """Every tile of the raster from an instance that holds all of it (computed once, read-only)."""
    from moonsuperresolution_amd import DEMSuperResolution
    d = DEMSuperResolution(_cfg(), model=f32_identity)
    d.setImages(*raster)
    d.padInputs()
    assert d.canvas_row0 == 0 and d.dem_window_shape == d.dem_padded_shape == tuple(d.dem_padded.shape)
    out = _tiles_to_host(d, d.generateTileList())
    d.close()
    assert any(g.any() for _, _, g in out.values()) and not all(g.all() for _, _, g in out.values())
    return out


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_tile_mode_windowed_rank_equals_whole_raster(hip_lib, raster, whole_tiles, rank):
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    world = 3
    r0, r1 = D.input_rows(SHAPE, S, STRIDE, T, rank, world, "tiles")
    assert (r0, r1) != (0, SHAPE[0])
    d = _window_instance(DEMSuperResolution, img, dem, (r0, r1))
    d.padInputs()
    c0, c1 = D.canvas_rows(SHAPE, S, STRIDE, r0, r1)
    rows, cols = d.dem_window_shape
    assert d.canvas_row0 == c0 and rows == c1 - c0 and cols == d.dem_padded_shape[1]
    assert d.dem_shape == SHAPE and d.dem_padded_shape == (1024 + 2 * (S - STRIDE),) * 2
    assert tuple(d.dem_padded.shape) == tuple(d.img_padded.shape) == d.dem_window_shape
    nbytes = sum(t.numel() * t.element_size() for t in (d.dem_padded, d.img_padded))
    assert nbytes == 2 * rows * cols * 4
    mine = D.shard_tile_rows(d.generateTileList(), rank, world)
    assert mine and d.generateTileList() == sorted(whole_tiles, key=lambda t: (t[1], t[0]))
    got = _tiles_to_host(d, mine)
    for t in mine:
        for a, b in zip(got[t], whole_tiles[t]):
            assert np.array_equal(a, b, equal_nan=True), (rank, t)
    d.close()


def test_crop_for_rank_keeps_the_rows_of_input_rows(hip_lib, raster, whole_tiles):
    from moonsuperresolution_amd import DEMSuperResolution
    d = DEMSuperResolution(_cfg(), model=f32_identity)
    d.setImages(*raster)
    rows = D.crop_for_rank(d, 1, 3)
    assert rows == D.input_rows(SHAPE, S, STRIDE, T, 1, 3, "tiles") and d.row0 == rows[0]
    assert d.dem.shape == (rows[1] - rows[0], SHAPE[1]) and d.dem_shape == SHAPE
    d.padInputs()
    assert d.canvas_row0 == rows[0] + S - STRIDE
    got = D.process_map_sharded(SHAPE, T, d.generateTileList(), d.processTile, rank=1, world=3, gather=False,
                                device=d.device)
    for (xx, yy) in D.shard_tile_rows(d.generateTileList(), 1, 3):
        for a, b in zip(got, whole_tiles[(xx, yy)]):
            h, w = min(T, SHAPE[0] - yy), min(T, SHAPE[1] - xx)
            assert np.array_equal(a[yy:yy + h, xx:xx + w], b[:h, :w], equal_nan=True)
    d.close()


# ---- halo mode ----------------------------------------------------------------------------------------------------------
def _finish(instances, states):
    world = len(states)
    slabs = []
    for r, st in enumerate(states):
        from_down = states[r - 1]["send_up"] if r > 0 else None
        from_up = states[r + 1]["send_down"] if r < world - 1 else None
        slabs.append(instances[r].haloFinish(st, from_down, from_up))
    return instances[0].cropHalo(slabs)


@pytest.mark.parametrize("world,band_rows", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_halo_mode_cropped_ranks_equal_uncropped(hip_lib, raster, world, band_rows):
    """Ranks simulated as in tests/test_gpu_halo.py::run_halo, but every rank is an instance of its own that crops its
    inputs; the uncropped run (one instance, the whole canvas) is what the existing test checks against the oracle."""
    from moonsuperresolution_amd import HaloShardedSuperResolution
    img, dem = raster
    whole = HaloShardedSuperResolution(_cfg(), model=f32_identity)
    whole.setImages(img, dem)
    want = _finish([whole] * world, [whole.haloAccumulate(r, world, band_rows=band_rows) for r in range(world)])
    full_canvas = whole.dem_padded_shape
    ranks, states = [], []
    for r in range(world):
        d = HaloShardedSuperResolution(_cfg(), model=f32_identity)
        d.setImages(img, dem)
        states.append(d.haloAccumulate(r, world, band_rows=band_rows, crop_inputs=True))
        r0, r1 = D.input_rows(SHAPE, S, STRIDE, T, r, world, "halo")
        c0, c1 = D.canvas_rows(SHAPE, S, STRIDE, r0, r1)
        assert d.canvas_row0 == c0 and d.dem_window_shape == (c1 - c0, full_canvas[1]) and c1 - c0 < full_canvas[0]
        assert tuple(d.dem_padded.shape) == d.dem_window_shape and d.dem_padded_shape == full_canvas
        ranks.append(d)
    got = _finish(ranks, states)
    assert got[2].any() and not got[2].all()
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True), (world, band_rows)
    for d in ranks + [whole]:
        d.close()


# ---- a real generator ---------------------------------------------------------------------------------------------------
def test_generator_tile_mode_cropped_equals_uncropped(hip_lib):
    """The same batches through the same kernels: a window offset that leaked into the batch assembly (origins, keys,
    normalisation) would change generator outputs."""
    from moonsuperresolution_amd import DEMSuperResolution, Generator
    # two tile rows, neither rank needs all rows; 36 / 4 / 24 / 2 valid patches in the four tiles (a hole, and last batches
    # that are padded)
    img, dem = synthetic_raster(230, 150, 9, hole=(120, 140, 100, 130))
    shape, world = img.shape, 2
    gen = Generator(S, B, variant="gaugan_no_kl", weights=1234)
    whole = DEMSuperResolution(_cfg(), model=gen)
    whole.setImages(img, dem)
    whole.padInputs()
    tiles = whole.generateTileList()
    want = _tiles_to_host(whole, tiles)
    whole.close()
    for rank in range(world):
        d = _window_instance(DEMSuperResolution, img, dem, D.input_rows(shape, S, STRIDE, T, rank, world, "tiles"), model=gen)
        d.padInputs()
        assert d.dem_window_shape[0] < d.dem_padded_shape[0]
        mine = D.shard_tile_rows(tiles, rank, world)
        got = _tiles_to_host(d, mine)
        for t in mine:
            assert got[t][2].any() and not got[t][2].all()
            for a, b in zip(got[t], want[t]):
                assert np.array_equal(a, b, equal_nan=True), (rank, t)
        d.close()
    gen.close()


# ---- files --------------------------------------------------------------------------------------------------------------
def test_process_files_reads_only_the_ranks_rows(hip_lib, tmp_path, monkeypatch):
    """processFiles(rank=1, world=3, mode="tiles") without gathering writes that rank's rows of the in-memory run, having
    decoded fewer strips than a full read.  write_geotiff cuts strips of 64 KiB: 300 x 420 float32 gives eight strips of 39
    rows per file, of which rank 1's rows [80, 300) need six (at 200 columns the four strips of 81 rows would all be
    needed: row 80 is the last row of the first one)."""
    from moonsuperresolution_amd import DEMSuperResolution
    shape, rank, world = (300, 420), 1, 3
    img, dem = synthetic_raster(shape[0], shape[1], seed=22, hole=(110, 150, 60, 120))
    src, dst = tmp_path / "in", tmp_path / "out"
    os.makedirs(src)
    G.write_geotiff(str(src / "run-DRG.tif"), img, nodata=-32768.0)
    G.write_geotiff(str(src / "run-DEM.tif"), dem, nodata=-32768.0)
    calls = []
    real = G.lzw_decode

    def counting(data, out_size):
        calls.append(out_size)
        return real(data, out_size)
    monkeypatch.setattr(G, "lzw_decode", counting)
    G.read_geotiff(str(src / "run-DEM.tif"))
    G.read_geotiff(str(src / "run-DRG.tif"))
    full_reads = len(calls)
    del calls[:]
    d = DEMSuperResolution(_cfg(source_folder_path=str(src), save_path=str(dst), map_name="m"), model=f32_identity)
    d.processFiles(preprocess=False, rank=rank, world=world, mode="tiles", gather=False)
    r0, r1 = D.input_rows(shape, S, STRIDE, T, rank, world, "tiles")
    assert (r0, r1) == (80, 300) and d.row0 == r0 and d.dem_shape == shape
    assert len(calls) == 2 * len(range(r0 // 39, -(-r1 // 39))) == 12 and full_reads == 16
    monkeypatch.setattr(G, "lzw_decode", real)
    got = [G.read_geotiff(str(dst / f"m_{name}.tiff"))[0] for name in ("mean", "std", "good")]
    d.close()
    ref = DEMSuperResolution(_cfg(), model=f32_identity)
    ref.setImages(img, dem)
    ref.padInputs()
    mine = D.shard_tile_rows(ref.generateTileList(), rank, world)
    assert [yy for _, yy in mine] == [128] * 4
    for (xx, yy), tile in _tiles_to_host(ref, mine).items():
        h, w = min(T, shape[0] - yy), min(T, shape[1] - xx)
        for a, b in zip(got, tile):
            assert np.array_equal(a[yy:yy + h, xx:xx + w], b[:h, :w].astype(np.float32), equal_nan=True), (xx, yy)
    ref.close()
    for a in got:                                          # rows of the other ranks stay zero without the gather
        assert not a[:128].any() and not a[256:].any()
    assert got[2][128:256].any()


def test_process_files_halo_mode_writes_the_in_memory_map(hip_lib, tmp_path, raster):
    """processFiles(mode="halo") through read_info -> input_rows -> loadImages(rows=) with one rank (more ranks exchange
    their zones over a process group): the files hold what processMapHalo + cropHalo give in memory."""
    from moonsuperresolution_amd import HaloShardedSuperResolution
    img, dem = raster
    src, dst = tmp_path / "in", tmp_path / "out"
    os.makedirs(src)
    G.write_geotiff(str(src / "run-DRG.tif"), img, nodata=-32768.0)
    G.write_geotiff(str(src / "run-DEM.tif"), dem, nodata=-32768.0)
    d = HaloShardedSuperResolution(_cfg(source_folder_path=str(src), save_path=str(dst), map_name="h"), model=f32_identity)
    d.processFiles(preprocess=False, rank=0, world=1, mode="halo")
    got = [G.read_geotiff(str(dst / f"h_{name}.tiff"))[0] for name in ("mean", "std", "good")]
    want = d.cropHalo([d.processMapHalo(img, dem)])
    d.close()
    assert want[2].any() and not want[2].all()
    for a, b in zip(got, want):
        assert np.array_equal(a, b.astype(np.float32), equal_nan=True)


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_a_tile_outside_the_window_and_preprocess_on_a_window_raise(hip_lib, raster):
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    d = _window_instance(DEMSuperResolution, img, dem, D.input_rows(SHAPE, S, STRIDE, T, 1, 3, "tiles"))
    with pytest.raises(ValueError, match="window"):
        d.preprocess()
    d.padInputs()
    d.processTile(0, 128)                                  # its own tile row
    with pytest.raises(ValueError, match=r"tile \(0, 0\).*window"):
        d.processTile(0, 0)                                # rank 0's: above the window
    d.close()
    d = _window_instance(DEMSuperResolution, img, dem, D.input_rows(SHAPE, S, STRIDE, T, 0, 3, "tiles"))
    d.padInputs()
    for tile in ((0, 128), (128, 256)):                    # partly and wholly below rank 0's window
        with pytest.raises(ValueError, match=r"tile \(%d, %d\).*window" % tile):
            d.processTile(*tile)
    with pytest.raises(ValueError):
        d.setImages(img[:10], dem[:10], row0=295, full_shape=SHAPE)        # 295 + 10 rows > 300
    with pytest.raises(ValueError):
        d.setImages(img[:10], dem[:10], row0=0, full_shape=(300, 199))     # other width
    d.close()

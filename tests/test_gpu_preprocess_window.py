"""GPU (-m gpu): pre-processing a row window gives the bits of the same rows of the whole-raster pre-processing.

  * msr_resize_area_rows / msr_resize_cubic_rows on a row band equal the rows of msr_resize_area / msr_resize_cubic on the
    whole array (which tests/test_gpu_preprocess.py holds against oracle/preprocess_ref.py), NaNs included; the source window
    given is the smallest one allowed, so the entries' own statement of the rows they need is checked with it; the no-data
    flags equal the torch.where passes they replace; a window that lacks a needed row is refused before any launch;
  * DEMSuperResolution.preprocess(rows=) on the band of preprocess.window_plan equals preprocess(swap_dsize=False) on the
    whole raster, which equals the oracle's composition;
  * processFiles(preprocess=True, mode=...) of a rank writes what the in-memory run on the whole pre-processed raster gives,
    and decodes only its band's strips.

Raster: 3210 x 406 (H % 4 = 2, W % 4 = 2; x1/4 grid 802 x 102, x1/16 grid 200 x 26), in-fill tiles at x1/4 rows 0, 192, 384,
576 writing rows [32, 224), [224, 416), [416, 608), [608, 770).  All comparisons are exact.
"""
import os

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import distributed as D
from moonsuperresolution_amd import geotiff as G
from moonsuperresolution_amd import preprocess as pp
from oracle import preprocess_ref as pr

pytestmark = pytest.mark.gpu
NOVAL = -32768.0
SHAPE = (3210, 406)
S, STRIDE, B, T = 64, 32, 16, 128
# 8 x 8 holes (top row, left column): one or more in every in-fill tile row; 780 and 1560 lie in the rows two tiles share
# (x1/4 rows 192-224, 384-416), 892 and 1660 straddle the rows where the writing tile changes (224, 416); 3100 lies in the
# last 128 rows, which no tile writes: it passes through un-filled
SMALL = [(300, 140), (780, 200), (892, 230), (1560, 150), (1660, 260), (2000, 180), (2700, 250), (3100, 200)]
BIG = (1200, 160)                                         # 80 x 80: 400 pixels of the x1/4 grid, too large to in-fill
WINDOWS = [(0, 700), (1000, 1700), (2400, 3210), (1500, 1505)]


def f32_identity(x, training=False):
    return np.asarray(x, np.float32)


def _cfg(**kw):
    from moonsuperresolution_amd import DSRConfig
    return DSRConfig(image_size=S, stride=STRIDE, batch_size=B, tile_size=T, **kw)


def bits_equal(a, b):
    """Same shape, NaNs in the same places, every other value the same bits."""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.nan_to_num(a).view(np.uint32), np.nan_to_num(b).view(np.uint32))


@pytest.fixture(scope="module")
def ctx(hip_lib):
    from moonsuperresolution_amd import ops
    return ops.OpContext()


@pytest.fixture(scope="module")
def raster():
    h, w = SHAPE
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    dem = (-2000.0 + 0.3 * xx + 0.2 * yy + 5.0 * np.sin(xx / 17.0) * np.cos(yy / 23.0)).astype(np.float32)
    for r, c in SMALL:
        dem[r:r + 8, c:c + 8] = NOVAL
    dem[BIG[0]:BIG[0] + 80, BIG[1]:BIG[1] + 80] = NOVAL
    img = np.random.default_rng(3).uniform(0, 1, dem.shape).astype(np.float32)
    return img, dem


@pytest.fixture(scope="module")
def whole(hip_lib, raster):
    """preprocess(swap_dsize=False) of the whole raster (computed once, read-only), checked against the oracle."""
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    d = DEMSuperResolution(_cfg(), model=f32_identity)
    d.setImages(img, dem)
    d.preprocess(swap_dsize=False)
    out = d.dem
    assert out.shape == SHAPE and out.dtype == np.float32 and np.array_equal(d.image, img) and d.row0 == 0
    d.close()
    out.setflags(write=False)
    return out


# ---- entries ------------------------------------------------------------------------------------------------------------
def _area_rows(ctx, src, src_row0, full_rows, dst_rows, flags=0):
    return pp._area_rows(ctx.lib, ctx.h, src, src_row0, full_rows, dst_rows, NOVAL, flags).cpu().numpy()


def _bands(n):
    """Start at 0, strictly inside, end at n, one row, everything."""
    return [b for b in [(0, n // 3), (n // 3, 2 * n // 3 + 1), (2 * n // 3, n), (n // 2, n // 2 + 1), (0, n)] if b[1] > b[0]]


@pytest.mark.parametrize("shape", [SHAPE, (50, 75), (1030, 517), (1032, 516), (10, 11)])
def test_area_rows_equal_the_rows_of_the_whole_resize(ctx, shape):
    """(1032, 516): the float4 path; (1030, 517) / (10, 11): a partial bottom block; 406 and 75 columns: a partial right one."""
    h, w = shape
    rng = np.random.default_rng(h)
    src = (rng.normal(size=shape) * 1000).astype(np.float32)
    src[rng.uniform(size=shape) < 0.01] = np.nan
    src[1, 1] = src[h - 1, w - 1] = np.nan               # a full block and the last block, whatever the draw gave
    dev = torch.from_numpy(src).cuda()
    want = pp.resize_area(ctx.lib, ctx.h, dev, 4).cpu().numpy()
    dh = want.shape[0]
    assert dh == pr.cv_round(h / 4) and np.isnan(want).any()
    for d0, d1 in _bands(dh):
        s0, s1 = 4 * d0, min(4 * d1, h)                   # the smallest source window
        got = _area_rows(ctx, dev[s0:s1], s0, h, (d0, d1))
        assert bits_equal(got, want[d0:d1]), (shape, d0, d1)
        a, b = max(0, s0 - 3), min(h, s1 + 5)             # a wider one, not aligned to the blocks
        assert bits_equal(_area_rows(ctx, dev[a:b], a, h, (d0, d1)), want[d0:d1]), (shape, d0, d1)


@pytest.mark.parametrize("shape,dsize", [((200, 26), (406, 3210)), ((33, 65), (1000, 517)), ((16, 12), (192, 256)),
                                         ((40, 40), (13, 17)), ((7, 9), (9, 7))])
def test_cubic_rows_equal_the_rows_of_the_whole_resize(ctx, shape, dsize):
    h, w = shape
    dw, dh = dsize
    rng = np.random.default_rng(dw)
    src = (rng.normal(size=shape) * 100 - 2000).astype(np.float32)
    if h > 8:
        src[3, 4] = src[h - 2, 1] = np.nan
    dev = torch.from_numpy(src).cuda()
    want = pp.resize_cubic(ctx.lib, ctx.h, dev, dsize).cpu().numpy()
    idx, _ = pr._cubic_axis(h, dh)                        # the oracle's clamped taps of every destination row
    for d0, d1 in _bands(dh):
        s0, s1 = int(idx[d0:d1].min()), int(idx[d0:d1].max()) + 1      # the smallest source window
        assert (s0, s1) == pp._cubic_tap_rows(d0, d1, h, dh)
        dst = torch.empty((d1 - d0, dw), dtype=torch.float32, device="cuda")
        rc = ctx.lib.msr_resize_cubic_rows(ctx.h, dev[s0:s1].data_ptr(), s0, s1 - s0, h, w, dst.data_ptr(), d0, d1 - d0, dh,
                                           dw, NOVAL, 0, None)
        assert rc == 0, ctx.lib.msr_last_error(ctx.h)
        torch.cuda.synchronize()
        assert bits_equal(dst.cpu().numpy(), want[d0:d1]), (shape, dsize, d0, d1)


@pytest.mark.parametrize("shape", [(1032, 516), (1030, 517)])
def test_no_data_flags_equal_the_where_passes(ctx, shape):
    h, w = shape
    rng = np.random.default_rng(w)
    src = (rng.normal(size=shape) * 1000).astype(np.float32)
    src[rng.uniform(size=shape) < 0.01] = NOVAL
    src[rng.uniform(size=shape) < 0.002] = NOVAL - 5.0    # below no_value is no-data too
    src[rng.uniform(size=shape) < 0.002] = np.nan
    dev = torch.from_numpy(src).cuda()
    marked = torch.where(dev <= NOVAL, torch.full_like(dev, float("nan")), dev)
    a_nan = pp.resize_area(ctx.lib, ctx.h, marked, 4)
    a_nv = torch.where(torch.isnan(a_nan), torch.full_like(a_nan, NOVAL), a_nan)
    dh = a_nan.shape[0]
    assert torch.isnan(a_nan).any() and not torch.isnan(a_nan).all()
    assert bits_equal(_area_rows(ctx, dev, 0, h, (0, dh), pp.RESIZE_NODATA_TO_NAN), a_nan.cpu().numpy())
    assert bits_equal(_area_rows(ctx, marked, 0, h, (0, dh), pp.RESIZE_NAN_TO_NODATA), a_nv.cpu().numpy())
    both = _area_rows(ctx, dev, 0, h, (0, dh), pp.RESIZE_NODATA_TO_NAN | pp.RESIZE_NAN_TO_NODATA)
    assert not np.isnan(both).any() and bits_equal(both, a_nv.cpu().numpy())
    # cubic: the small grid back to (h, w)
    small = a_nv.contiguous()
    c_nan = pp.resize_cubic(ctx.lib, ctx.h, torch.where(small <= NOVAL, torch.full_like(small, float("nan")), small), (w, h))
    c_nv = torch.where(torch.isnan(c_nan), torch.full_like(c_nan, NOVAL), c_nan).cpu().numpy()
    for flags, want in ((pp.RESIZE_NODATA_TO_NAN, c_nan.cpu().numpy()),
                        (pp.RESIZE_NODATA_TO_NAN | pp.RESIZE_NAN_TO_NODATA, c_nv)):
        dst = torch.empty((h, w), dtype=torch.float32, device="cuda")
        rc = ctx.lib.msr_resize_cubic_rows(ctx.h, small.data_ptr(), 0, small.shape[0], small.shape[0], small.shape[1],
                                           dst.data_ptr(), 0, h, h, w, NOVAL, flags, None)
        assert rc == 0, ctx.lib.msr_last_error(ctx.h)
        torch.cuda.synchronize()
        assert bits_equal(dst.cpu().numpy(), want), (shape, flags)
    assert (c_nv == NOVAL).any() and not (c_nv == NOVAL).all()


def test_a_window_that_lacks_a_needed_row_is_refused_before_any_launch(ctx):
    h, w = 200, 52
    dev = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    dst = torch.full((20, 13), 7.0, dtype=torch.float32, device="cuda")

    def area(s0, s1, d0, d1, flags=0):
        return ctx.lib.msr_resize_area_rows(ctx.h, dev[s0:s1].data_ptr(), s0, s1 - s0, h, w, 4, dst.data_ptr(), d0, d1 - d0,
                                            13, NOVAL, flags, None)
    assert area(40, 120, 10, 30) == 0                     # exactly the rows needed
    torch.cuda.synchronize()
    assert (dst == 0).all()
    dst.fill_(7.0)
    for s0, s1 in ((41, 120), (40, 119)):                 # one row short above / below
        assert area(s0, s1, 10, 30) == -1
        msg = ctx.lib.msr_last_error(ctx.h).decode()
        assert "[40, 120)" in msg and f"[{s0}, {s1})" in msg, msg
    assert area(40, 120, 10, 30, flags=4) == -1           # an unknown flag
    up = torch.full((30, 9), 7.0, dtype=torch.float32, device="cuda")
    a, b = pp._cubic_tap_rows(100, 130, h, 640)           # 640 <- 200 rows

    def cubic(s0, s1):
        return ctx.lib.msr_resize_cubic_rows(ctx.h, dev[s0:s1].data_ptr(), s0, s1 - s0, h, w, up.data_ptr(), 100, 30, 640, 9,
                                             NOVAL, 0, None)
    for s0, s1 in ((a + 1, b), (a, b - 1)):
        assert cubic(s0, s1) == -1
        msg = ctx.lib.msr_last_error(ctx.h).decode()
        assert f"[{a}, {b})" in msg and f"[{s0}, {s1})" in msg, msg
    torch.cuda.synchronize()
    assert (dst == 7.0).all() and (up == 7.0).all()       # nothing was written
    assert cubic(a, b) == 0
    torch.cuda.synchronize()
    assert (up == 0).all()
    with pytest.raises(ValueError, match="source rows"):
        pp._area_rows(ctx.lib, ctx.h, dev[41:120], 41, h, (10, 30), NOVAL, 0)


# ---- preprocess(rows=) ----------------------------------------------------------------------------------------------------
def test_whole_raster_preprocess_equals_the_oracle_composition(raster, whole):
    _, dem = raster
    d = np.array(dem, np.float32, copy=True)
    d[d <= NOVAL] = np.nan
    d = pr.resize_area(d, 0.25, 0.25)
    d[np.isnan(d)] = NOVAL
    d = pr.fill_nan(d, NOVAL, tile_size=256, border=32, max_fill_area=24)
    d[d <= NOVAL] = np.nan
    d = pr.resize_area(d, 0.25, 0.25)
    d = pr.resize_cubic(d, (SHAPE[1], SHAPE[0]))
    d[np.isnan(d)] = NOVAL
    assert np.array_equal(whole.view(np.uint32), d.view(np.uint32))
    for r, c in SMALL[:-1]:                               # in-filled ...
        assert (whole[r:r + 8, c:c + 8] != NOVAL).all(), (r, c)
    assert (whole[BIG[0] + 30:BIG[0] + 50, BIG[1] + 30:BIG[1] + 50] == NOVAL).all()      # ... too large ...
    assert (whole[SMALL[-1][0]:SMALL[-1][0] + 8, SMALL[-1][1]:SMALL[-1][1] + 8] == NOVAL).any()   # ... and never written


@pytest.mark.parametrize("rows", WINDOWS)
def test_preprocess_rows_equals_the_rows_of_the_whole_raster(hip_lib, raster, whole, rows):
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    r0, r1 = rows
    m0, m1 = pp.window_plan(SHAPE, rows)["dem"]
    m0, m1 = min(m0, r0), max(m1, r1)                     # the ortho's rows too (SHAPE[0] - 4 * rint(SHAPE[0] / 4) = 2)
    assert m1 - m0 < SHAPE[0]                             # every window here gets by with a band
    d = DEMSuperResolution(_cfg(), model=f32_identity)
    d.setImages(img[m0:m1].copy(), dem[m0:m1].copy(), row0=m0, full_shape=SHAPE)
    d.preprocess(swap_dsize=False, rows=rows)
    assert d.row0 == r0 and d.dem_shape == SHAPE and d.image is None
    assert d.dem.dtype == np.float32 and d.dem.shape == (r1 - r0, SHAPE[1])
    assert np.array_equal(d.dem.view(np.uint32), whole[r0:r1].view(np.uint32))
    assert np.array_equal(d.img, img[r0:r1])
    if rows == (1000, 1700):                              # in-filled holes and a surviving one inside this window
        assert (dem[1560:1568, 150:158] == NOVAL).all() and (d.dem[560:568, 150:158] != NOVAL).all()
        assert (d.dem[230:250, 190:210] == NOVAL).all()
    d.padInputs()                                         # then as after setImages(row0=, full_shape=)
    assert d.canvas_row0 == D.canvas_rows(SHAPE, S, STRIDE, r0, r1)[0]
    d.close()


def test_preprocess_rows_from_the_whole_raster_and_on_a_square_one(hip_lib, raster, whole):
    """rows= with the whole raster held; swap_dsize=True is the same thing on a square raster and an error otherwise."""
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    d = DEMSuperResolution(_cfg(), model=f32_identity)
    d.setImages(img, dem)
    d.preprocess(swap_dsize=False, rows=(1500, 1505))
    assert np.array_equal(d.dem.view(np.uint32), whole[1500:1505].view(np.uint32)) and d.row0 == 1500
    sq_img, sq_dem = img[:400, :400].copy(), dem[:400, :400].copy()
    d.setImages(sq_img, sq_dem)
    d.preprocess(swap_dsize=True)
    want = d.dem
    d.setImages(sq_img, sq_dem)
    d.preprocess(swap_dsize=True, rows=(100, 300))
    assert np.array_equal(d.dem.view(np.uint32), want[100:300].view(np.uint32))
    d.close()


def test_preprocess_rows_errors(hip_lib, raster):
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    d = DEMSuperResolution(_cfg(), model=f32_identity)
    d.setImages(img[1000:1700].copy(), dem[1000:1700].copy(), row0=1000, full_shape=SHAPE)
    m0, m1 = pp.window_plan(SHAPE, (1000, 1700))["dem"]
    assert m0 < 1000 and m1 > 1700
    with pytest.raises(ValueError, match=rf"window.*\[{m0}, 1000\).*\[1700, {m1}\)"):
        d.preprocess(swap_dsize=False, rows=(1000, 1700))
    with pytest.raises(ValueError, match="window"):       # without rows: whole rasters only, as before
        d.preprocess(swap_dsize=False)
    with pytest.raises(ValueError, match=":241"):
        d.preprocess(rows=(1000, 1700))                   # swap_dsize=True on a non-square raster
    with pytest.raises(ValueError, match="window"):
        pp.preprocess_rows(d._lib, d._h, d.device, dem[1000:1700], 1000, SHAPE, (1000, 1700), NOVAL)
    d.close()


# ---- files --------------------------------------------------------------------------------------------------------------
def _write_inputs(tmp_path, img, dem):
    src, dst = tmp_path / "in", tmp_path / "out"
    os.makedirs(src)
    G.write_geotiff(str(src / "run-DRG.tif"), img, nodata=NOVAL)
    G.write_geotiff(str(src / "run-DEM.tif"), dem, nodata=NOVAL)
    return src, dst


def test_process_files_preprocesses_the_ranks_band(hip_lib, tmp_path, monkeypatch, raster, whole):
    """Rank 1 of 3 (tile rows 9 .. 17, raster rows [1120, 2336)) reads its band, pre-processes it and writes, for its tile
    rows, what the run on the whole pre-processed raster gives.  write_geotiff cuts strips of 64 KiB = 40 rows here."""
    from moonsuperresolution_amd import DEMSuperResolution
    img, dem = raster
    rank, world = 1, 3
    src, dst = _write_inputs(tmp_path, img, dem)
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
    d.processFiles(preprocess=True, swap_dsize=False, rank=rank, world=world, mode="tiles", gather=False)
    r0, r1 = D.input_rows(SHAPE, S, STRIDE, T, rank, world, "tiles")
    m0, m1 = D.input_rows(SHAPE, S, STRIDE, T, rank, world, "tiles", preprocess=True)
    assert (r0, r1) == (1120, 2336) and m0 < r0 and r1 < m1 and m1 - m0 < SHAPE[0]
    assert d.row0 == r0 and d.dem_shape == SHAPE
    assert len(calls) == 2 * len(range(m0 // 40, -(-m1 // 40))) < full_reads == 2 * 81
    monkeypatch.setattr(G, "lzw_decode", real)
    got = [G.read_geotiff(str(dst / f"m_{name}.tiff"))[0] for name in ("mean", "std", "good")]
    d.close()
    ref = DEMSuperResolution(_cfg(), model=f32_identity)
    ref.setImages(img, np.array(whole))
    ref.padInputs()
    mine = D.shard_tile_rows(ref.generateTileList(), rank, world)
    assert sorted({yy for _, yy in mine}) == list(range(9 * T, 18 * T, T))
    for xx, yy in mine:
        tile = [t.cpu().numpy() for t in ref.processTile(xx, yy)]
        h, w = min(T, SHAPE[0] - yy), min(T, SHAPE[1] - xx)
        for a, b in zip(got, tile):
            assert np.array_equal(a[yy:yy + h, xx:xx + w], b[:h, :w].astype(np.float32), equal_nan=True), (xx, yy)
    ref.close()
    for a in got:                                          # rows of the other ranks stay zero without the gather
        assert not a[:9 * T].any() and not a[18 * T:].any()
    assert got[2][9 * T:18 * T].any() and not got[2][9 * T:18 * T].all()


def test_process_files_halo_mode_preprocesses(hip_lib, tmp_path, raster, whole):
    """mode="halo" with one rank (more ranks exchange their zones over a process group): the files hold what processMapHalo
    gives in memory on the whole pre-processed raster."""
    from moonsuperresolution_amd import HaloShardedSuperResolution
    img, dem = raster
    src, dst = _write_inputs(tmp_path, img, dem)
    d = HaloShardedSuperResolution(_cfg(source_folder_path=str(src), save_path=str(dst), map_name="h"), model=f32_identity)
    d.processFiles(preprocess=True, swap_dsize=False, rank=0, world=1, mode="halo")
    got = [G.read_geotiff(str(dst / f"h_{name}.tiff"))[0] for name in ("mean", "std", "good")]
    want = d.cropHalo([d.processMapHalo(img, np.array(whole))])
    d.close()
    assert want[2].any() and not want[2].all()
    for a, b in zip(got, want):
        assert np.array_equal(a, b.astype(np.float32), equal_nan=True)

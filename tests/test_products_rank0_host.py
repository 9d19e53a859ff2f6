"""CPU: the geometry and the file assembly of the rank-0 product writer (processFiles(products="rank0")).

  * distributed.strip_plan: W = 256 with T = 128 gives strips of 64 (float32) and 128 (uint16) rows, both divide 128, no strip
    straddles a rank; W = 300 gives 54 rows a strip, strips straddle (the gathered fallback); W = 70000 gives one row a strip;
    over worlds 1, 2, 3 and 8 the per-rank strip ranges cover every strip once, in order — ranks without rows and a short last
    strip included — and each rank's strips hold exactly its rows;
  * the file put together from strips encoded rank by rank (geotiff.encode_strips on each rank's rows, write_strips) is, byte
    for byte, write_geotiff's file of the whole raster: what rank 0 writes.  Host encoder here; the device encoder and the
    two-process run are in tests/test_gpu_products_rank0.py (the driver cannot be built without a GPU).
"""
import numpy as np
import pytest

from moonsuperresolution_amd import distributed as D
from moonsuperresolution_amd import geotiff as G
from tests import resident_cases as cases

WORLDS = (1, 2, 3, 8)


def test_strip_rows_of_the_named_widths():
    for world in WORLDS:
        f32, u16 = D.strip_plan((300, 256), 4, 128, world), D.strip_plan((300, 256), 2, 128, world)
        assert (f32["rps"], u16["rps"]) == (64, 128) and 128 % f32["rps"] == 0 and 128 % u16["rps"] == 0
        assert not f32["straddles"] and not u16["straddles"]
        assert (f32["n_strips"], u16["n_strips"]) == (5, 3)                       # the last strips are short: 44 rows
    odd = D.strip_plan((300, 300), 4, 128, 2)
    assert odd["rps"] == 54 and odd["straddles"] and odd["strips"] is None      # -> the gathered fallback
    assert D.strip_plan((300, 300), 2, 128, 2)["rps"] == 109
    assert not D.strip_plan((300, 300), 4, 128, 1)["straddles"]                   # one rank: no boundary to straddle
    for itemsize in (2, 4):
        big = D.strip_plan((15000, 70000), itemsize, 1024, 8)
        assert big["rps"] == 1 and big["n_strips"] == 15000 and not big["straddles"]
        assert big["rows"][0] == (0, 2048) and big["rows"][7] == (14336, 15000) and big["strips"] == big["rows"]
    assert D.strip_plan((100, 8193), 4, 32, 4)["rps"] == 1                        # a row above 32 KiB


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("shape,itemsize,T", [((300, 256), 4, 128), ((300, 256), 2, 128), ((128, 256), 4, 128),
                                              ((1000, 70000), 4, 128), ((77, 512), 2, 16), ((300, 300), 4, 128)])
def test_the_plan_covers_every_strip_once(shape, itemsize, T, world):
    plan = D.strip_plan(shape, itemsize, T, world)
    H = shape[0]
    rps = plan["rps"]
    assert rps == G._rows_per_strip(H, shape[1] * itemsize) and plan["n_strips"] == -(-H // rps)
    rows = plan["rows"]
    assert len(rows) == world and rows[0][0] == 0 and rows[-1][1] == H
    assert all(a[1] == b[0] for a, b in zip(rows, rows[1:])) and all(r0 <= r1 for r0, r1 in rows)
    tile_rows = -(-H // T)
    for rank, (r0, r1) in enumerate(rows):
        first, count = D.rows_of_rank(tile_rows, rank, world)
        assert (r0, r1) == (min(first * T, H), min((first + count) * T, H))
    straddles = any(r0 % rps for r0, _ in rows if 0 < r0 < H)
    assert plan["straddles"] == straddles
    if straddles:
        assert plan["strips"] is None
        return
    strips = plan["strips"]
    assert strips[0][0] == 0 and strips[-1][1] == plan["n_strips"]
    assert all(a[1] == b[0] for a, b in zip(strips, strips[1:]))                  # consecutive: every strip once, in order
    for (r0, r1), (s0, s1) in zip(rows, strips):
        if r1 == r0:
            assert s0 == s1                                                       # a rank without rows: no strips
        else:
            assert (s0 * rps, min(s1 * rps, H)) == (r0, r1)                       # its strips hold exactly its rows
    if world > tile_rows:
        assert any(r0 == r1 for r0, r1 in rows)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_strips_encoded_rank_by_rank_make_the_same_file(tmp_path, dtype, world):
    shape = cases.SHAPES["wide"]
    img, dem = cases.raster(shape)
    data = dem if dtype == np.float32 else (np.abs(dem).astype(np.int64) % 7).astype(np.uint8)   # uint8, like ``good``
    meta = {"geo": {33550: (12, 3, np.array([2.0, 2.0, 0.0]).tobytes())}, "byteorder": "<"}
    G.write_geotiff(str(tmp_path / "whole.tiff"), data, meta, nodata=cases.NOVAL, dtype=dtype)
    plan = D.strip_plan(shape, np.dtype(dtype).itemsize, cases.T, world)
    assert not plan["straddles"]
    strips = []
    for rank, (r0, r1) in enumerate(plan["rows"]):
        mine = G.encode_strips(data[r0:r1], dtype, plan["rps"]) if r1 > r0 else []
        assert len(mine) == plan["strips"][rank][1] - plan["strips"][rank][0]
        strips += mine
    G.write_strips(str(tmp_path / "ranks.tiff"), strips, shape, dtype, plan["rps"], meta, nodata=cases.NOVAL)
    assert open(tmp_path / "ranks.tiff", "rb").read() == open(tmp_path / "whole.tiff", "rb").read()
    back, _ = G.read_geotiff(str(tmp_path / "ranks.tiff"))
    assert np.array_equal(back, data.astype(np.float32))
    with pytest.raises(ValueError, match="strips for"):
        G.write_strips(str(tmp_path / "short.tiff"), strips[:-1], shape, dtype, plan["rps"])

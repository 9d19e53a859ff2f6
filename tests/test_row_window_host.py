"""CPU: the host half of the row window a sharded rank works on.

  * geotiff.read_geotiff(rows=(r0, r1)) equals the slice of the full read bit for bit (uint32 views: NaN payloads count) for
    every container form the reader knows, and decodes only the strips that intersect the window (a counting wrapper over
    geotiff.lzw_decode); geotiff.read_info decodes none;
  * distributed.input_rows against a brute-force set of touched rows built here from the reference's origin rule
    (process_full_tiles.py:453-454: origins range(py, py + T + S - s, s), each covers S rows, canvas offset S - s).
"""
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from moonsuperresolution_amd import distributed as D
from moonsuperresolution_amd import geotiff as G

ROWS, COLS = 75, 41
WINDOWS = [(0, 1), (5, 37), (7, 8), (72, 75), (0, 75)]


def _raster():
    rng = np.random.default_rng(11)
    a = (-2000 + 300 * rng.standard_normal((ROWS, COLS))).astype(np.float32)
    a[3:9, 4:20] = -32768.0
    a[70:75, 30:] = -32768.0
    a[6, 1] = a[36, 40] = np.nan
    u = a.view(np.uint32)
    u[40, 7] = 0x7FC12345                                  # a NaN with a payload: only a bit comparison sees it
    u[74, 0] = 0xFFC00001
    return a


def _write_tiled(path, a, tw=16, compress=False):
    """Little-endian single-band float32 file in tw x tw tiles (the tile height does not divide 75), hand-built like the
    tiled file of tests/test_geotiff.py; optionally Deflate-compressed."""
    rows, cols = a.shape
    tiles = []
    for ty in range(-(-rows // tw)):
        for tx in range(-(-cols // tw)):
            t = np.zeros((tw, tw), "<f4")
            blk = a[ty * tw:(ty + 1) * tw, tx * tw:(tx + 1) * tw]
            t[:blk.shape[0], :blk.shape[1]] = blk
            tiles.append(zlib.compress(t.tobytes()) if compress else t.tobytes())
    off, offs = 8, []
    for t in tiles:
        offs.append(off)
        off += len(t)
    n = len(tiles)
    ent = [(256, 3, 1, struct.pack("<HH", cols, 0)), (257, 3, 1, struct.pack("<HH", rows, 0)),
           (258, 3, 1, struct.pack("<HH", 32, 0)), (259, 3, 1, struct.pack("<HH", 8 if compress else 1, 0)),
           (262, 3, 1, struct.pack("<HH", 1, 0)), (277, 3, 1, struct.pack("<HH", 1, 0)),
           (322, 3, 1, struct.pack("<HH", tw, 0)), (323, 3, 1, struct.pack("<HH", tw, 0)), (324, 4, n, None),
           (325, 4, n, None), (339, 3, 1, struct.pack("<HH", 3, 0))]
    extra_off = off + 2 + 12 * len(ent) + 4
    ifd, extra = struct.pack("<H", len(ent)), b""
    for tag, typ, cnt, raw in ent:
        if raw is None:
            vals = offs if tag == 324 else [len(t) for t in tiles]
            ifd += struct.pack("<HHII", tag, typ, cnt, extra_off + len(extra))
            extra += struct.pack(f"<{n}I", *vals)
        else:
            ifd += struct.pack("<HHI", tag, typ, cnt) + raw
    ifd += struct.pack("<I", 0)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, off) + b"".join(tiles) + ifd + extra)


def _pil(compression):
    def write(path, a):
        Image.fromarray(a, mode="F").save(path, compression=compression, tiffinfo={278: 8})      # strips of 8 rows
    return write


FORMS = {
    "own_lzw_pred2": lambda path, a: G.write_geotiff(path, a, nodata=-32768.0),
    "pil_lzw_strips8": _pil("tiff_lzw"),
    "pil_deflate_strips8": _pil("tiff_adobe_deflate"),
    "pil_packbits_strips8": _pil("packbits"),
    "pil_raw_strips8": _pil(None),
    "tiles16": lambda path, a: _write_tiled(path, a),
    "tiles16_deflate": lambda path, a: _write_tiled(path, a, compress=True),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_windowed_read_equals_the_slice_of_the_full_read(tmp_path, form):
    a = _raster()
    path = str(tmp_path / "w.tif")
    FORMS[form](path, a)
    full, meta = G.read_geotiff(path)
    assert np.array_equal(full.view(np.uint32), a.view(np.uint32))
    assert meta["shape"] == (ROWS, COLS) and meta["window"] == (0, ROWS)
    info = G.read_info(path)
    assert info["shape"] == (ROWS, COLS) and info["window"] == (0, ROWS)
    assert {k: info[k] for k in ("geo", "nodata", "dtype", "byteorder")} == \
           {k: meta[k] for k in ("geo", "nodata", "dtype", "byteorder")}
    for r0, r1 in WINDOWS:
        win, wmeta = G.read_geotiff(path, band=1, rows=(r0, r1))
        assert win.dtype == np.float32 and win.shape == (r1 - r0, COLS)
        assert np.array_equal(win.view(np.uint32), full[r0:r1].view(np.uint32)), (r0, r1)
        assert wmeta["shape"] == (ROWS, COLS) and wmeta["window"] == (r0, r1)
    for bad in ((-1, 3), (4, 4), (0, 76)):
        with pytest.raises(ValueError):
            G.read_geotiff(path, rows=bad)


def test_only_the_intersecting_strips_are_decoded(tmp_path, monkeypatch):
    a = _raster()
    path = str(tmp_path / "s.tif")
    _pil("tiff_lzw")(path, a)
    calls = []
    real = G.lzw_decode

    def counting(data, out_size):
        calls.append(out_size)
        return real(data, out_size)
    monkeypatch.setattr(G, "lzw_decode", counting)
    for (r0, r1), strips in (((5, 37), 5), ((0, 1), 1), ((7, 8), 1), ((72, 75), 1), ((8, 16), 1), ((0, 75), 10)):
        del calls[:]
        G.read_geotiff(path, rows=(r0, r1))
        assert len(calls) == strips == len(range(r0 // 8, -(-r1 // 8))), (r0, r1, len(calls))
    del calls[:]
    G.read_geotiff(path)
    assert len(calls) == 10
    del calls[:]
    assert G.read_info(path)["shape"] == (ROWS, COLS) and calls == []


# ---- input_rows ---------------------------------------------------------------------------------------------------------
S, s, T = 64, 16, 128


def _touched(shape, rank, world, mode):
    """Raster rows the rank's patches touch, by brute force from the reference's origin rule."""
    H = shape[0]
    tile_ys = list(range(0, H, T))
    if mode == "tiles":
        first, count = D.rows_of_rank(len(tile_ys), rank, world)
        origins = [y for py in tile_ys[first:first + count] for y in range(py, py + T + S - s, s)]
    else:
        grid = sorted({y for py in tile_ys for y in range(py, py + T + S - s, s)})
        first, count = D.rows_of_rank(len(grid), rank, world)
        origins = grid[first:first + count]
    rows = set()
    for y in origins:
        rows.update(r for r in range(y - (S - s), y + S - (S - s)) if 0 <= r < H)
    return rows


@pytest.mark.parametrize("mode", ["tiles", "halo"])
@pytest.mark.parametrize("world", [1, 2, 3, 5])
@pytest.mark.parametrize("shape", [(300, 200), (257, 130)])
def test_input_rows_contains_every_touched_row_and_is_tight(shape, world, mode):
    idle = 0
    for rank in range(world):
        r0, r1 = D.input_rows(shape, S, s, T, rank, world, mode)
        rows = _touched(shape, rank, world, mode)
        if not rows:
            assert (r0, r1) == (0, 0)
            idle += 1
            continue
        assert 0 <= r0 < r1 <= shape[0]
        assert rows <= set(range(r0, r1))
        assert r0 in rows and r1 - 1 in rows
        if world == 1:
            assert (r0, r1) == (0, shape[0])
    if mode == "tiles":
        assert idle == max(0, world - 3)               # three tile rows: two of five ranks have none
    elif world < 5:
        assert idle == 0                               # (with five ranks the last one's patch rows lie in the bottom margin)


def test_input_rows_matches_the_shared_enumeration_and_rejects_bad_arguments():
    # the tile loop, patchGrid and input_rows go through the same helper: its statement of the reference's rule
    assert list(D.patch_origins_1d(128, S, s, T)) == list(range(128, 128 + T + S - s, s))
    assert D.tile_origins((257, 130), T) == [(xx, yy) for yy in range(0, 257, T) for xx in range(0, 130, T)]
    with pytest.raises(ValueError):
        D.input_rows((300, 200), S, s, T, 0, 2, "rows")
    with pytest.raises(ValueError):
        D.input_rows((300, 200), S, s, T, 2, 2, "tiles")


def test_input_rows_at_the_real_size_is_at_most_a_quarter_of_the_raster():
    """15000 x 70000, S = 512, s = 64, T = 1024, rank 3 of 8: the rank owns 2 of 15 tile rows, whose patches touch
    2 * 1024 + 2 * 448 rows; its halo share (31 of 247 patch rows) is smaller."""
    H = 15000
    r0, r1 = D.input_rows((H, 70000), 512, 64, 1024, 3, 8, "tiles")
    assert r1 - r0 == 2 * 1024 + 2 * 448 and r1 - r0 <= H / 4
    h0, h1 = D.input_rows((H, 70000), 512, 64, 1024, 3, 8, "halo")
    assert 0 < h1 - h0 < r1 - r0 and h1 - h0 <= H / 4
    c0, c1 = D.canvas_rows((H, 70000), 512, 64, h0, h1)
    assert c1 - c0 == h1 - h0                            # an interior window: no margin rows

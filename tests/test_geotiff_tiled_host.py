"""CPU: tiled GeoTIFF products with overviews — everything that needs no GPU.

  1. keywords: every ValueError of write_geotiff(tile=, overviews=), read_geotiff(overview=) and the driver's product_tile /
     overviews (raised before the GPU is asked for), the RuntimeError of the device encoder on a machine without a GPU, and
     tile=None, overviews=0 giving the file of a call without the keywords byte for byte;
  2. layout: the tags of the IFD chain, the order of the file's parts, zero-padded edge tiles (the bytes equal those of
     tests/geotiff_decode_cases.write_tiled for one level);
  3. libtiff through PIL reads every level of the tiled files and the project's own reader does (overview=k, rows=,
     overview_shapes): both equal the twin's chain;
  4. the twin, geotiff.overview_reference, against answers worked out by hand;
  5. msr_overview_half_host (the kernel's per-pixel function looped on the host) equals the twin's bits, with 64 canary
     elements behind dst; both entries are declared and bound; msr_overview_half returns each argument error before any launch.
All comparisons are for equal bits or bytes."""
import os
import struct

import numpy as np
import pytest
from PIL import Image, features

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from tests import geotiff_decode_cases as decode_cases
from tests import geotiff_tiled_cases as cases

NV = cases.NOVAL
libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="PIL without libtiff")
f32 = np.float32


# ---- 1. keywords -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [(16, 15), (0, 16), (-16, 16), (16,), (16, 16, 16), 16, (16.0, 16), (8, 8), "ab", (True, 16)])
def test_bad_tile_is_named(tmp_path, tile):
    with pytest.raises(ValueError, match="tile"):
        G.write_geotiff(str(tmp_path / "a.tif"), cases.raster((17, 33), "float32"), tile=tile)
    assert not os.path.exists(tmp_path / "a.tif")


def test_bad_overviews_are_named(tmp_path):
    p = str(tmp_path / "a.tif")
    a = cases.raster((17, 33), "float32")
    for n in (-1, 1.0, "1", True):
        with pytest.raises(ValueError, match="overviews"):
            G.write_geotiff(p, a, tile=(16, 16), overviews=n)
    with pytest.raises(ValueError, match="overviews=1 needs tile"):
        G.write_geotiff(p, a, overviews=1)
    assert cases.most_overviews((17, 33)) == 6 and cases.most_overviews((16, 16)) == 4 and cases.most_overviews((1, 1)) == 0
    G.write_geotiff(p, a, tile=(16, 16), overviews=6)                       # ceil(log2(33)) = 6: the most
    assert G.overview_shapes(p)[-1] == (1, 1)
    with pytest.raises(ValueError, match="overviews=7"):
        G.write_geotiff(p, a, tile=(16, 16), overviews=7)
    with pytest.raises(ValueError, match="overviews=1"):
        G.write_geotiff(p, cases.raster((1, 1), "float32"), tile=(16, 16), overviews=1)
    small = np.abs(a) % 100
    for dtype in (np.int16, np.uint32, np.float64, np.int8):
        with pytest.raises(ValueError, match="overviews.*dtype"):
            G.write_geotiff(p, small, dtype=dtype, tile=(16, 16), overviews=1)
        G.write_geotiff(p, small, dtype=dtype, tile=(16, 16))               # tiles alone take every dtype the writer takes
        assert np.array_equal(G.read_geotiff(p)[0], small.astype(dtype).astype(f32))


def test_keywords_are_keyword_only(tmp_path):
    with pytest.raises(TypeError):
        G.write_geotiff(str(tmp_path / "a.tif"), cases.raster((17, 33), "float32"), None, NV, f32, "lzw", 2, None, "host", None,
                        256 << 20, None, (16, 16))


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_defaults_write_the_same_bytes(tmp_path, dtype):
    a = cases.raster((70, 101), dtype)
    meta = {"geo": {33550: (12, 3, struct.pack("<3d", 2.0, 2.0, 0.0)), 34737: (2, 8, b"WGS 84|\0")}, "byteorder": "<"}
    G.write_geotiff(str(tmp_path / "a.tif"), a, meta, nodata=NV, dtype=dtype)
    G.write_geotiff(str(tmp_path / "b.tif"), a, meta, nodata=NV, dtype=dtype, tile=None, overviews=0)
    want = open(tmp_path / "a.tif", "rb").read()
    assert open(tmp_path / "b.tif", "rb").read() == want
    rps = G._rows_per_strip(70, 101 * a.dtype.itemsize)
    G.write_strips(str(tmp_path / "c.tif"), G.encode_strips(a, dtype, rps), a.shape, dtype, rps, meta, nodata=NV)
    assert open(tmp_path / "c.tif", "rb").read() == want


def test_device_encoder_without_a_gpu_is_an_error(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.write_geotiff(str(tmp_path / "a.tif"), cases.raster((17, 33), "float32"), tile=(16, 16), overviews=2, encoder="device")
    with pytest.raises(ValueError, match="LZW only"):                      # the refusal that was there stays in front
        G.write_geotiff(str(tmp_path / "a.tif"), cases.raster((17, 33), "float32"), tile=(16, 16), compress="deflate",
                        encoder="device")
    with pytest.raises(ValueError, match="tile"):                           # and a bad keyword is named before the device is
        G.write_geotiff(str(tmp_path / "a.tif"), cases.raster((17, 33), "float32"), tile=(16, 8), encoder="device")


def test_read_overview_errors(tmp_path):
    p = str(tmp_path / "a.tif")
    a = cases.raster((17, 33), "float32")
    G.write_geotiff(p, a, nodata=NV, tile=(16, 16), overviews=2)
    for k in (-1, 1.0, "1", True):
        with pytest.raises(ValueError, match="overview"):
            G.read_geotiff(p, overview=k)
    for decoder in ("host", "device"):                                      # raised from the IFDs, before any device is asked for
        with pytest.raises(ValueError, match="overview 3 does not exist"):
            G.read_geotiff(p, overview=3, decoder=decoder)
    with pytest.raises(ValueError, match="row window"):
        G.read_geotiff(p, overview=1, rows=(0, 10))                         # level 1 has 9 rows
    G.write_geotiff(p, a, nodata=NV)
    assert G.overview_shapes(p) == []
    with pytest.raises(ValueError, match="overview 1 does not exist"):
        G.read_geotiff(p, overview=1)
    assert "overview" not in G.read_geotiff(p)[1] and "overview" not in G.read_info(p)


def test_driver_keywords_are_checked_before_the_gpu_is_asked_for(monkeypatch):
    import torch
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, HaloShardedSuperResolution

    def no_gpu():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    cfg = DSRConfig(image_size=64, stride=16, batch_size=4, tile_size=128)
    for cls in (DEMSuperResolution, HaloShardedSuperResolution):
        with pytest.raises(ValueError, match="tile"):
            cls(cfg, product_tile=(16, 24))
        with pytest.raises(ValueError, match="tile"):
            cls(cfg, product_tile=256)
        with pytest.raises(ValueError, match="overviews"):
            cls(cfg, product_tile=(16, 16), overviews=-1)
        with pytest.raises(ValueError, match="overviews=2 needs tile"):
            cls(cfg, overviews=2)


def test_rank_local_writer_refuses_tiles():
    """processFiles(products="rank0") with product_tile: a ValueError before any work (nothing of the instance but the two
    keywords is looked at, so an instance without a device behind it shows it)."""
    from moonsuperresolution_amd import DEMSuperResolution
    d = DEMSuperResolution.__new__(DEMSuperResolution)
    d.product_tile, d.overviews = (16, 16), 0
    with pytest.raises(ValueError, match="rank0.*product_tile"):
        d.processFiles(mode="tiles", products="rank0")


# ---- 2. layout ---------------------------------------------------------------------------------------------------------------
def _ifds(path):
    """[(offset, tag dict)] of the chain of a little-endian classic TIFF."""
    buf = np.fromfile(path, np.uint8)
    out, off = [], struct.unpack_from("<I", buf, 4)[0]
    while off:
        out.append((off, G._read_ifd(buf, False, "<", off)))
        off = G._next_ifd(buf, False, "<", off)
    return out, buf.size


def _v(t, tag):
    return G._values(t[tag], "<")


@pytest.mark.parametrize("dtype,predictor", cases.FORMATS)
def test_layout_of_a_file_with_overviews(tmp_path, dtype, predictor):
    p = str(tmp_path / "a.tif")
    shape, tile = (70, 101), (16, 32)
    meta = {"geo": {33550: (12, 3, struct.pack("<3d", 2.0, 2.0, 0.0)), 34737: (2, 8, b"WGS 84|\0")}, "byteorder": "<"}
    G.write_geotiff(p, cases.raster(shape, dtype), meta, nodata=NV, dtype=dtype, predictor=predictor, tile=tile, overviews=2)
    ifds, size = _ifds(p)
    chain = cases.chain(shape, dtype, 2)
    assert len(ifds) == 3
    end_of_blocks = 8
    for k, (off, t) in enumerate(ifds):
        rows, cols = chain[k].shape
        assert (_v(t, 257)[0], _v(t, 256)[0]) == (rows, cols)
        assert _v(t, 322)[0] == 32 and _v(t, 323)[0] == 16
        assert not {278, 273, 279} & set(t)                                  # no strip tags
        n = -(-rows // 16) * -(-cols // 32)
        offs, cnts = _v(t, 324), _v(t, 325)
        assert len(offs) == len(cnts) == n
        assert offs[0] == end_of_blocks                                      # levels in order, tiles row-major, back to back
        for i in range(n):
            assert offs[i] == end_of_blocks
            end_of_blocks += cnts[i] + (cnts[i] & 1)
        assert (254 in t and _v(t, 254)[0] == 1) if k else 254 not in t
        assert t[G.GDAL_NODATA][2] == b"-32768\0"
        assert ({33550, 34737} <= set(t)) if k == 0 else not set(G.GEO_TAGS) & set(t)
        assert _v(t, 259)[0] == 5 and _v(t, 258)[0] == 8 * np.dtype(dtype).itemsize
        assert (_v(t, 317)[0] == 2) if predictor == 2 else 317 not in t
        assert _v(t, 339)[0] == (3 if dtype == "float32" else 1)
    assert ifds[0][0] == end_of_blocks                                       # then the IFDs, in order, each before its values
    assert [o for o, _ in ifds] == sorted(o for o, _ in ifds) and all(o % 2 == 0 for o, _ in ifds)
    buf = np.fromfile(p, np.uint8)
    for (off, t), nxt in zip(ifds, [o for o, _ in ifds[1:]] + [size]):
        values_at = struct.unpack_from("<I", buf, off + 2 + 12 * sorted(t).index(324) + 8)[0]      # TileOffsets lie out of line
        assert off < values_at < nxt


@pytest.mark.parametrize("predictor", [1, 2])
def test_one_level_equals_the_hand_built_tiled_file_tile_for_tile(tmp_path, predictor):
    """Zero-padded edge tiles and the predictor restarting on every tile row: the tiles are those write_tiled builds."""
    a = cases.raster((70, 101), "uint16")
    G.write_geotiff(str(tmp_path / "a.tif"), a, dtype="uint16", predictor=predictor, tile=(16, 32))
    decode_cases.write_tiled(str(tmp_path / "b.tif"), [a], 32, 16, predictor=predictor)
    tiles = []
    for name in ("a.tif", "b.tif"):
        buf, t, bo, _ = G._open(str(tmp_path / name))
        tiles.append([bytes(buf[o:o + c]) for o, c in zip(G._values(t[324], bo), G._values(t[325], bo))])
    assert len(tiles[0]) == 5 * 4 and tiles[0] == tiles[1]


# ---- 3. readers --------------------------------------------------------------------------------------------------------------
def _file_cases():
    for shape, tile in cases.LAYOUTS:
        for dtype, predictor in cases.FORMATS:
            for n in sorted({0, min(1, cases.most_overviews(shape)), cases.most_overviews(shape)}):
                yield pytest.param(shape, tile, dtype, predictor, n, id=f"{shape[0]}x{shape[1]}-{tile[0]}x{tile[1]}-{dtype}-p{predictor}-o{n}")


@libtiff
@pytest.mark.parametrize("shape,tile,dtype,predictor,n", list(_file_cases()))
def test_libtiff_reads_every_level(tmp_path, shape, tile, dtype, predictor, n):
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, cases.raster(shape, dtype), nodata=NV, dtype=dtype, predictor=predictor, tile=tile, overviews=n)
    chain = cases.chain(shape, dtype, n)
    with Image.open(p) as im:
        assert im.n_frames == n + 1
        for k in range(n + 1):
            im.seek(k)
            assert im.tag_v2[322] == tile[1] and im.tag_v2[323] == tile[0]
            assert im.tag_v2.get(254) == (1 if k else None)
            got = np.array(im)
            assert got.dtype == chain[k].dtype and got.shape == chain[k].shape
            assert np.array_equal(cases.bits(got), cases.bits(chain[k])), k


@pytest.mark.parametrize("shape,tile,dtype,predictor,n", list(_file_cases()))
def test_own_reader_reads_every_level(tmp_path, shape, tile, dtype, predictor, n):
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, cases.raster(shape, dtype), nodata=NV, dtype=dtype, predictor=predictor, tile=tile, overviews=n)
    chain = cases.chain(shape, dtype, n)
    assert G.overview_shapes(p) == [c.shape for c in chain[1:]]
    assert G.read_info(p)["shape"] == shape and "overview" not in G.read_info(p)
    for k in range(n + 1):
        want = chain[k].astype(f32)
        got, meta = G.read_geotiff(p, overview=k)
        assert np.array_equal(cases.bits(got), cases.bits(want)), k
        assert meta["shape"] == want.shape and meta["nodata"] == NV and meta["dtype"] == np.dtype(dtype)
        assert meta.get("overview") == (k if k else None)
        r0, r1 = want.shape[0] // 3, want.shape[0]
        part, meta = G.read_geotiff(p, overview=k, rows=(r0, r1))
        assert np.array_equal(cases.bits(part), cases.bits(want[r0:r1])) and meta["window"] == (r0, r1)


# ---- 4. the twin, by hand ------------------------------------------------------------------------------------------------------
def _one(block, nodata=NV):
    out = G.overview_reference(np.array(block, f32), nodata)
    assert out.shape == (1, 1) and out.dtype == f32
    return out[0, 0]


def test_twin_counts_zero_to_four():
    assert _one([[NV, NV], [NV, NV]]) == f32(NV)
    assert _one([[NV, 3], [NV, NV]]) == 3
    assert _one([[1, NV], [NV, 2]]) == 1.5
    assert _one([[1, 2], [NV, 6]]) == 3
    assert _one([[1, 2], [3, 6]]) == 3
    assert _one([[1, 2], [3, 7]]) == f32(3.25)


def test_twin_nan_and_negative_zero():
    assert np.isnan(_one([[np.nan, 1], [2, 3]])) and np.isnan(_one([[NV, NV], [NV, np.nan]]))
    z = _one([[NV, -0.0], [NV, NV]])
    assert z == 0 and np.signbit(z)                                          # the sum starts from the first value, not from 0
    z = _one([[-0.0, NV], [-0.0, NV]])
    assert z == 0 and np.signbit(z)
    assert not np.signbit(_one([[-0.0, 0.0], [NV, NV]]))


def test_twin_sums_in_row_major_order():
    a, b, c = f32(1e8), f32(-1e8), f32(1)
    assert (a + b) + c != a + (b + c)                                         # 1 and 0: the order shows
    assert _one([[a, b], [c, NV]]) == f32(1) / f32(3)                         # (a + b) + c
    assert _one([[c, b], [a, NV]]) == 0                                       # (c + b) + a = -1e8 + 1e8
    assert _one([[NV, a], [b, c]]) == f32(1) / f32(3)
    x = [f32(0.1), f32(0.2), f32(0.3), f32(1e-3)]
    assert _one([x[:2], x[2:]]) == (((x[0] + x[1]) + x[2]) + x[3]) / f32(4)


def test_twin_edge_blocks_and_no_nodata():
    a = np.array([[1, 2, 10], [3, 6, NV], [5, 8, 7]], f32)
    assert np.array_equal(G.overview_reference(a, NV), np.array([[3, 10], [6.5, 7]], f32))       # 2 x 1, 1 x 2 and 1 x 1 blocks
    assert np.array_equal(G.overview_reference(a[:, 2:], NV), np.array([[10], [7]], f32))
    assert np.array_equal(G.overview_reference(a[1:2, 2:], NV), np.array([[NV]], f32))
    assert _one([[NV, 1], [1, 1]], None) == ((f32(NV) + f32(1)) + f32(1) + f32(1)) / f32(4)    # nodata=None: all count
    assert np.array_equal(G.overview_reference(a), np.array([[3, (f32(10) + f32(NV)) / f32(2)], [6.5, 7]], f32))


def test_twin_integers_take_the_maximum():
    for dt in (np.uint8, np.uint16):
        top = np.iinfo(dt).max
        a = np.array([[1, 0, 0], [0, 0, top], [0, 0, 2]], dt)
        out = G.overview_reference(a, NV)                                     # nodata is not looked at
        assert out.dtype == dt and np.array_equal(out, np.array([[1, top], [0, 2]], dt))
    good = (cases.raster((71, 101), "float32") != f32(NV)).astype(np.uint8)
    mean = G.overview_reference(cases.raster((71, 101), "float32"), NV)
    assert np.array_equal(G.overview_reference(good) == 1, mean != f32(NV))   # good is 1 exactly where mean is not nodata
    for bad in (np.zeros((2, 2), np.int16), np.zeros((2, 2), np.float64), np.zeros(4, f32), np.zeros((0, 4), f32)):
        with pytest.raises(ValueError, match="overview_reference"):
            G.overview_reference(bad)


# ---- 5. entries --------------------------------------------------------------------------------------------------------------
def _host_half(a, has_nodata, nodata=NV):
    lib = _lib.load()
    rows, cols = a.shape
    n = -(-rows // 2) * -(-cols // 2)
    out = np.full(n + cases.CANARY, 0xA5, a.dtype) if a.dtype.kind == "u" else np.full(n + cases.CANARY, 12345.0, f32)
    canary = out[n:].copy()
    src = np.ascontiguousarray(a)
    rc = lib.msr_overview_half_host(src.ctypes.data, rows, cols, ord(a.dtype.kind), a.dtype.itemsize, int(has_nodata), nodata,
                                    out.ctypes.data)
    assert rc == 0 and np.array_equal(out[n:], canary)
    return out[:n].reshape(-(-rows // 2), -(-cols // 2))


def test_host_entry_equals_the_twin_on_the_hand_cases():
    blocks = [[[NV, NV], [NV, NV]], [[NV, 3], [NV, NV]], [[1, NV], [NV, 2]], [[1, 2], [NV, 6]], [[1, 2], [3, 7]],
              [[np.nan, 1], [2, 3]], [[NV, -0.0], [NV, NV]], [[1e8, -1e8], [1, NV]], [[1, -1e8], [1e8, NV]],
              [[1, 2, 10], [3, 6, NV], [5, 8, 7]], [[NV]], [[4, NV]], [[4], [9]]]
    for blk in blocks:
        a = np.array(blk, f32)
        for has_nodata in (True, False):
            want = G.overview_reference(a, NV if has_nodata else None)
            assert np.array_equal(cases.bits(_host_half(a, has_nodata)), cases.bits(want)), (blk, has_nodata)
    for dt in (np.uint8, np.uint16):
        a = np.array([[1, 0, 0], [0, 0, np.iinfo(dt).max], [0, 0, 2]], dt)
        assert np.array_equal(_host_half(a, False), G.overview_reference(a))


@pytest.mark.parametrize("shape,kind,has_nodata", cases.reduce_cases())
def test_host_entry_equals_the_twin_on_random_rasters(shape, kind, has_nodata):
    a = cases.reduce_input(shape, kind)
    if kind == "nodata" and shape[0] >= 2 and shape[1] >= 10:
        assert cases.counts_of(a) == {0, 1, 2, 3, 4}
    want = G.overview_reference(a, NV if has_nodata else None)
    assert np.array_equal(cases.bits(_host_half(a, has_nodata)), cases.bits(want))


def test_entries_are_declared():
    names = [s[0] for s in _lib.SYMBOLS]
    with open(os.path.join(_lib.CSRC, "..", "..", "include", "moonsr.h")) as fh:
        header = fh.read()
    for name, nargs, decl in (("msr_overview_half", 10, "int msr_overview_half(msr_handle* h, const void* src_dev, int32_t rows,"),
                              ("msr_overview_half_host", 8, "int msr_overview_half_host(const void* src, int32_t rows,")):
        assert name in names and decl in header
        assert len(_lib.SYMBOLS[names.index(name)][2]) == nargs
        assert hasattr(_lib.load(), name)
    assert os.path.exists(os.path.join(_lib.CSRC, "tiff_overview.h"))


def test_argument_errors_return_before_any_launch():
    """Every call here is rejected before a launch, so host arrays can stand in for device memory."""
    lib = _lib.load()
    src, dst = np.zeros(16, f32), np.zeros(16, f32)
    #       src               rows cols kind     sb has nv  dst
    good = [src.ctypes.data, 4, 4, ord("f"), 4, 1, NV, dst.ctypes.data]

    def rejected(changes, word):
        bad = list(good)
        for i, v in changes.items():
            bad[i] = v
        assert lib.msr_overview_half(None, *bad, None) == _lib.MSR_ERR_INVALID, changes
        assert word in lib.msr_last_error(None), (changes, lib.msr_last_error(None))
        assert lib.msr_overview_half_host(*bad) == -1, changes

    rejected({0: None}, b"src")
    rejected({7: None}, b"dst")
    for v in (0, -1):
        rejected({1: v}, b"rows")
        rejected({2: v}, b"cols")
    rejected({1: 65536, 2: 32768}, b"2^31 - 1")                              # 2^31 source pixels
    rejected({1: 2 ** 31 - 1, 2: 2}, b"2^31 - 1")
    for kind in (0, ord("i"), ord("F"), ord("d")):
        rejected({3: kind}, b"sample_kind")
    for sb in (0, 1, 2, 8, -4):
        rejected({4: sb}, b"sample_bytes")
    for sb in (0, 4, 3):
        rejected({3: ord("u"), 4: sb, 5: 0}, b"sample_bytes")
    rejected({5: 2}, b"has_nodata")
    for sb in (1, 2):
        rejected({3: ord("u"), 4: sb, 5: 1}, b"has_nodata")
    assert np.array_equal(dst, np.zeros(16, f32))

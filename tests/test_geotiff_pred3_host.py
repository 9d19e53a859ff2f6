"""CPU: the floating-point predictor (PREDICTOR=3) of the GeoTIFF writer — everything that needs no GPU.

  1. the twin, geotiff.fp_predictor_reference, against libtiff: the decoded LZW stream of every strip of a predictor-3 file
     written by PIL equals the twin of that strip's rows, byte for byte;
  2. write_geotiff(predictor=3) as strips, tiles and the cloud-optimised order with two reduced levels: PIL and read_geotiff
     return the input's bits (NaNs with payloads, +-0, +-Inf, denormals, the nodata value), every reduced level is
     overview_reference's, every IFD carries Predictor = 3; float64 on the host; compress="none" forces predictor 1;
  3. refusals: an integer dtype; the arguments the new C entries reject, before any device is used;
  4. the old entry and the new one with predictor 1 / 2 write the same streams on the blocks of tests/geotiff_cog_cases.py;
  5. the one-lane run of the device's fetch (msr_tiff_encode_block_host, predictor 3) against msr_lzw_encode of the twin's
     bytes of the padded block.
All comparisons are for equal bits or bytes."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
from PIL import Image, features

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from tests import geotiff_cog_cases as cog_cases
from tests import geotiff_pred3_cases as cases

NV = cases.NOVAL


# ---- 1. the twin -------------------------------------------------------------------------------------------------------------
def test_twin_by_hand():
    a = np.array([[1.0, -2.5]], np.float32)                              # 3F800000, C0200000
    assert G.fp_predictor_reference(a).tolist() == [[0x3F, 0xC0 - 0x3F, 0x80 - 0xC0 + 256, 0x20 - 0x80 + 256, 0xE0, 0, 0, 0]]
    d = np.array([[1.0], [2.0]], np.float64)                             # 3FF0..., 4000...: a row restarts the differencing
    assert G.fp_predictor_reference(d).tolist() == [[0x3F, 0xF0 - 0x3F, 0x10, 0, 0, 0, 0, 0], [0x40, 0xC0, 0, 0, 0, 0, 0, 0]]
    assert G.fp_predictor_reference(np.zeros((0, 5), np.float32)).shape == (0, 20)
    big = np.array([[1.0, -2.5]], ">f4")                                 # the value decides, not the byte order it came in
    assert np.array_equal(G.fp_predictor_reference(big), G.fp_predictor_reference(a))
    for bad in (np.zeros((2, 2), np.uint16), np.zeros(4, np.float32), np.zeros((2, 2), np.float16)):
        with pytest.raises(ValueError, match="fp_predictor_reference"):
            G.fp_predictor_reference(bad)


def test_twin_against_libtiff(tmp_path):
    assert features.check("libtiff"), "PIL without libtiff: the twin has nothing to be checked against"
    rng = np.random.default_rng(3)
    a = (np.cumsum(rng.normal(0, 1, (300, 200)), axis=1) - 2000.0).astype(np.float32)
    a.view(np.uint32)[5, 7] = 0x7FC12345
    p3, p2 = str(tmp_path / "p3.tif"), str(tmp_path / "p2.tif")
    Image.fromarray(a).save(p3, compression="tiff_lzw", tiffinfo={317: 3})
    Image.fromarray(a).save(p2, compression="tiff_lzw", tiffinfo={317: 2})
    with Image.open(p3) as im:                                           # libtiff honours the tag
        assert im.tag_v2[317] == 3 and np.array_equal(np.array(im).view(np.uint32), a.view(np.uint32))
    assert os.path.getsize(p3) != os.path.getsize(p2)
    buf, t, bo, meta = G._open(p3)
    g = G._block_geometry(t, bo, meta, 1)
    assert (g.pred, g.comp, g.tiled, g.bw) == (3, 5, False, 200) and g.down > 1 and g.rows % g.bh
    for i in range(g.down):
        rows = a[i * g.bh:(i + 1) * g.bh]
        got = G.lzw_decode(bytes(buf[g.offs[i]:g.offs[i] + g.cnts[i]]), rows.size * 4)
        assert np.array_equal(got.reshape(rows.shape[0], -1), G.fp_predictor_reference(rows)), i
    got, _ = G.read_geotiff(p3)
    assert np.array_equal(cases.bits(got), cases.bits(a))


# ---- 2. the host writer ------------------------------------------------------------------------------------------------------
def _ifd_tags(path):
    """The tag dicts of every IFD of the file, in the order of the chain."""
    buf, big, bo, off = G._header(path)
    out = []
    while off:
        out.append({k: G._values(v, bo) for k, v in G._read_ifd(buf, big, bo, off).items()})
        off = G._next_ifd(buf, big, bo, off)
    return out


@pytest.mark.parametrize("name,shape,how", cases.LAYOUTS, ids=[x[0] for x in cases.LAYOUTS])
def test_host_writer_all_layouts(tmp_path, tmp_path_factory, name, shape, how):
    a = cases.raster(shape)
    u = cases.bits(a)
    for v in cases.LONELY + cases.ANYWHERE + (int(np.float32(NV).view(np.uint32)),):
        assert (u == v).any(), hex(v)
    path = str(tmp_path / "p3.tif")
    open(path, "wb").write(cases.host_file(tmp_path_factory, name))
    n = how.get("overviews", 0)
    ifds = _ifd_tags(path)
    assert len(ifds) == n + 1 and all(t[317] == (3,) for t in ifds)
    assert all((322 in t) == ("tile" in how) for t in ifds)
    want = cases.levels(shape, n)
    for k in range(n + 1):
        got, meta = G.read_geotiff(path, overview=k)
        assert got.shape == want[k].shape and np.array_equal(cases.bits(got), cases.bits(want[k])), k
        r0, r1 = got.shape[0] // 3, got.shape[0]
        part, _ = G.read_geotiff(path, overview=k, rows=(r0, r1))
        assert np.array_equal(cases.bits(part), cases.bits(want[k][r0:r1])), k
    if how.get("layout") == "cog":
        cog_cases.check_cog_order(path, n)
    assert features.check("libtiff")
    with Image.open(path) as im:
        for k in range(n + 1):
            im.seek(k)
            assert im.tag_v2[317] == 3
            assert np.array_equal(np.array(im).view(np.uint32), cases.bits(want[k])), k
    other = str(tmp_path / "p2.tif")
    G.write_geotiff(other, a, nodata=NV, **how)                          # the default is the horizontal predictor, as ever
    assert all(t[317] == (2,) for t in _ifd_tags(other)) and open(other, "rb").read() != open(path, "rb").read()
    assert np.array_equal(cases.bits(G.read_geotiff(other)[0]), u)


def test_strips_of_the_file_are_the_twin(tmp_path_factory, tmp_path):
    """What encode_strips returns, and what lies in the file, is msr_lzw_encode of the twin's bytes."""
    a = cases.raster((17, 33))
    strips = G.encode_strips(a, np.float32, 5, predictor=3)
    assert strips == [G.lzw_encode(G.fp_predictor_reference(a[r:r + 5])) for r in range(0, 17, 5)]
    path = str(tmp_path / "s.tif")
    G.write_strips(path, strips, a.shape, np.float32, 5, nodata=NV, predictor=3)
    assert _ifd_tags(path)[0][317] == (3,) and np.array_equal(cases.bits(G.read_geotiff(path)[0]), cases.bits(a))


def test_float64_deflate_and_no_compression(tmp_path):
    rng = np.random.default_rng(8)
    d = np.cumsum(rng.normal(0, 1, (17, 33)), axis=1)
    d[3, 4], d[16, 32] = np.nan, -0.0
    path = str(tmp_path / "d.tif")
    for how in ({}, {"tile": (16, 16)}, {"compress": "deflate"}):
        G.write_geotiff(path, d, dtype=np.float64, predictor=3, **how)
        assert _ifd_tags(path)[0][317] == (3,)
        got, meta = G.read_geotiff(path)                                  # the reader returns float32
        assert meta["dtype"] == np.float64 and np.array_equal(cases.bits(got), cases.bits(d.astype(np.float32)))
    G.write_geotiff(path, cases.raster((17, 33)), predictor=3, compress="none")
    assert 317 not in _ifd_tags(path)[0]
    assert np.array_equal(cases.bits(G.read_geotiff(path)[0]), cases.bits(cases.raster((17, 33))))


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int32"])
def test_integer_dtype_is_refused(tmp_path, dtype):
    a = np.zeros((17, 33), dtype)
    for how in ({}, {"tile": (16, 16)}, {"encoder": "device"}):
        with pytest.raises(ValueError, match=f"predictor 3.*{dtype}"):
            G.write_geotiff(str(tmp_path / "x.tif"), a, dtype=dtype, predictor=3, **how)
    with pytest.raises(ValueError, match=f"predictor 3.*{dtype}"):
        G.encode_strips(a, dtype, 5, predictor=3)
    assert not os.path.exists(str(tmp_path / "x.tif"))


def test_device_encoder_takes_float32_only(tmp_path):
    with pytest.raises(ValueError, match="float32 only.*float64"):
        G.write_geotiff(str(tmp_path / "x.tif"), np.zeros((17, 33)), dtype=np.float64, predictor=3, encoder="device")


def test_driver_keyword_is_checked_before_the_gpu_is_asked_for(monkeypatch):
    import torch
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, HaloShardedSuperResolution

    def no_gpu():
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    cfg = DSRConfig(image_size=64, stride=16, batch_size=4, tile_size=128)
    for cls in (DEMSuperResolution, HaloShardedSuperResolution):
        for bad in (4, 1, 0, "3", True, None, 3.5):
            with pytest.raises(ValueError, match="product_predictor"):
                cls(cfg, product_predictor=bad)


def test_entries_are_declared():
    names = [s[0] for s in _lib.SYMBOLS]
    with open(os.path.join(_lib.CSRC, "..", "..", "include", "moonsr.h")) as fh:
        header = fh.read()
    for name, restype, nargs, decl in (("msr_tiff_encode_strips", C.c_int, 13, "int msr_tiff_encode_strips(msr_handle* h,"),
                                       ("msr_tiff_encode_blocks", C.c_int, 16, "int msr_tiff_encode_blocks(msr_handle* h,"),
                                       ("msr_tiff_encode_block_host", C.c_int64, 10,
                                        "int64_t msr_tiff_encode_block_host(const uint8_t* src, int64_t pitch,")):
        assert name in names and decl in header
        _, rt, argtypes = _lib.SYMBOLS[names.index(name)]
        assert rt is restype and len(argtypes) == nargs
        assert hasattr(_lib.load(), name)


def test_argument_errors_return_before_any_launch():
    """Every call here is rejected (or has nothing to do) before a launch, so host arrays can stand in for device memory."""
    lib = _lib.load()
    b = np.zeros(64, np.uint8)
    o = np.zeros(2, np.int64)
    l32 = np.zeros(2, np.int32)
    p8, p64, p32 = b.ctypes.data, o.ctypes.data, l32.ctypes.data

    def refused(entry, args, *words):
        assert getattr(lib, entry)(None, *args, None) == _lib.MSR_ERR_INVALID, (entry, args)
        msg = lib.msr_last_error(None)
        assert entry.encode() in msg and all(w in msg for w in words), msg

    #         src src_off len n sb pred row_bytes dst dst_off cap len
    strips = [p8, p64, p32, 1, 4, 3, 64, p8, p64, p32, p32]
    #         src off  pitch w    rows n  bw  bh sb pred dst dst_off cap len
    blocks = [p8, p64, p64, p32, p32, 1, 64, 16, 4, 3, p8, p64, p32, p32]
    for entry, good, at in (("msr_tiff_encode_strips", strips, {"n": 3, "sb": 4, "pred": 5, "wb": 6}),
                            ("msr_tiff_encode_blocks", blocks, {"n": 5, "sb": 8, "pred": 9, "wb": 6})):
        def changed(**kw):
            bad = list(good)
            for k, v in kw.items():
                bad[at[k]] = v
            return bad

        for pred in (0, 4, -1, 317):
            refused(entry, changed(pred=pred), b"predictor")
        for sb in (2, 1):
            refused(entry, changed(sb=sb), b"predictor 3", b"sample_bytes")
        for sb in (0, 3, 8, -4):
            for pred in (1, 2, 3):
                refused(entry, changed(sb=sb, pred=pred), b"sample_bytes")
        for wb in (66, 63, 0, -64):
            refused(entry, changed(wb=wb), b"row_bytes" if "strips" in entry else b"block_w_bytes")
        refused(entry, changed(sb=2, pred=1, wb=63), b"row_bytes" if "strips" in entry else b"block_w_bytes")
        refused(entry, changed(n=-1), b"n_strips" if "strips" in entry else b"n_blocks")
        refused(entry, [None] + good[1:], b"null")
        for pred, sb in ((1, 1), (1, 4), (2, 2), (3, 4)):                # nothing to do: no launch
            assert getattr(lib, entry)(None, *changed(n=0, pred=pred, sb=sb), None) == _lib.MSR_OK
    s = np.zeros(256, np.uint8)
    d = np.zeros(2048, np.uint8)
    good = [s.ctypes.data, 16, 16, 8, 16, 8, 4, 3, d.ctypes.data, 2048]
    assert lib.msr_tiff_encode_block_host(*good) > 0
    for i, v in ((7, 0), (7, 4), (6, 2), (6, 1), (6, 0), (4, 18), (4, 0), (0, None), (8, None), (9, -1), (9, 1 << 31), (2, 20), (2, -4),
                 (3, 9), (3, -1), (5, 0)):
        bad = list(good)
        bad[i] = v
        assert lib.msr_tiff_encode_block_host(*bad) == -1, (i, v)


# ---- 4. the old entry and the new one ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sb", cog_cases.SAMPLE_BYTES)
def test_old_and_new_host_entry_agree(sb):
    """sample_bytes 0 of the old entry is predictor 1 of the new one, with any sample width that divides the block row."""
    lib = _lib.load()
    blocks = [b for g in cog_cases.geometries() if g[0] == sb for b in cog_cases.grid(*g)] + [b for b in cog_cases.special() if b.sb == sb]
    assert len(blocks) > 100
    for b in blocks:
        want = cog_cases.stream(b)
        old = np.zeros(len(want), np.uint8)
        new = np.zeros(len(want), np.uint8)
        src = np.array(b.src)
        args = (src.ctypes.data + b.off, b.pitch, b.vw, b.vr, b.bw, b.bh)
        assert lib.msr_lzw_encode_block_host(*args, b.sb, old.ctypes.data, old.size) == len(want), b.name
        widths = (1, 2, 4) if sb == 0 else (sb,)
        for width in (w for w in widths if b.bw % w == 0):
            assert lib.msr_tiff_encode_block_host(*args, width, 2 if sb else 1, new.ctypes.data, new.size) == len(want), b.name
            assert new.tobytes() == old.tobytes() == want, (b.name, width)
            new[:] = 0


# ---- 5. the one-lane run of the device's fetch -------------------------------------------------------------------------------
@pytest.mark.parametrize("bh,bw", cases.BLOCK_SIZES)
def test_one_lane_block_encoder_equals_the_twin(bh, bw):
    lib = _lib.load()
    src = np.array(cases.block_raster())
    for b in cases.blocks(bh, bw):
        want = cases.stream(b)
        off = b.y0 * cases.BLOCK_PITCH + b.x0 * 4
        assert cases.host_entry(lib, src, off, cases.BLOCK_PITCH, b) == want, b.name
        assert cases.host_entry(lib, src, off, cases.BLOCK_PITCH, b, cap=len(want)) == want, b.name
        assert cases.host_entry(lib, src, off, cases.BLOCK_PITCH, b, cap=len(want) - 1) == -1, b.name
        assert np.array_equal(cases.bits(src), cases.bits(cases.block_raster())), "the source was written"
        # rows that do not start on a 4-byte boundary are read byte by byte: the same stream
        raw = np.zeros(src.nbytes + 8, np.uint8)
        for shift in (1, 2, 3):
            raw[shift:shift + src.nbytes] = src.view(np.uint8).reshape(-1)
            assert cases.host_entry(lib, raw, off + shift, cases.BLOCK_PITCH, b) == want, (b.name, shift)
    # the padding is there before the predictor: the host writer's edge tile
    a = cases.raster((17, 33))
    tile = np.zeros((16, 16), np.float32)
    tile[:1, :1] = a[16:, 32:]
    edge = cases.Block("edge", 16, 32, 1, 1, 16, 16)
    assert cases.host_entry(lib, np.array(a), (16 * 33 + 32) * 4, 33 * 4, edge) == G._encode_block(tile, np.dtype("<f4"), 5, 3)


def test_one_lane_block_encoder_random_bytes():
    """A 48 x 48 block of random bytes: the table fills and is cleared, and the stream is longer than the block."""
    lib = _lib.load()
    rng = np.random.default_rng(48)
    noise = rng.integers(0, 256, 48 * 192, dtype=np.uint8).view(np.float32).reshape(48, 48)
    b = cases.Block("random", 0, 0, 48, 48, 48, 48)
    want = G.lzw_encode(G.fp_predictor_reference(noise))
    assert len(want) > 48 * 192
    assert cases.host_entry(lib, noise, 0, 192, b) == want

"""GPU: the device GeoTIFF encoder (csrc/geotiff_codec.hip) against the host one (csrc/host_codecs.cpp).  The criterion is
byte identity: of every strip's LZW stream with ``geotiff.lzw_encode`` of the same bytes, and of every file written with
``encoder="device"`` with the file written with ``encoder="host"``.  PIL/libtiff reading the device-written file back is
the independent check."""
import ctypes as C

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from tests.helpers import synthetic_raster

pytestmark = pytest.mark.gpu
NOVAL = -32768.0


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _streams(dev, data: np.ndarray, offsets, lengths, **kw):
    return G.lzw_encode_device(torch.from_numpy(data).to(dev), offsets, lengths, **kw)


def test_prefix_sweep_one_launch(dev):
    """Prefixes of length 0 .. 4400 of one random buffer, and the whole 12000 bytes, in one launch: the empty and the 1-byte
    strip, every width change (the dictionary reaches 512 / 1024 / 2048 entries at bytes 256 / 775 / 1821) with a prefix
    ending exactly on each (the bump before EOI), the first clear (byte 3946) and a second dictionary; three clears in the
    whole buffer; strips of different lengths side by side."""
    buf = np.random.default_rng(1234).integers(0, 256, 12000, dtype=np.uint8)
    lengths = list(range(0, 4401)) + [12000]
    got = _streams(dev, buf, [0] * len(lengths), lengths)
    assert len(got) == len(lengths)
    bad = [n for n, g in zip(lengths, got) if g != G.lzw_encode(buf[:n])]
    assert not bad, f"{len(bad)} prefixes differ from the host stream, the first at length {bad[0]}"
    assert got[0] == bytes([0x80, 0x40, 0x40])           # Clear, EOI as 9-bit codes, zero padded


@pytest.mark.parametrize("name", ["zeros", "pattern", "four_symbols"])
def test_long_matches(dev, name):
    if name == "zeros":
        data = np.zeros(280000, np.uint8)
    elif name == "pattern":
        data = np.tile(np.array([31, 0], np.uint8), 100000)
    else:
        data = np.random.default_rng(1234).integers(0, 4, 60000, dtype=np.uint8)     # first clear at byte 18194
    (got,) = _streams(dev, data, [0], [data.size])
    assert got == G.lzw_encode(data)


def test_capacity_is_a_hard_bound(dev):
    """Three equal strips, the middle slot one byte short of the stream: its length is -1, the neighbours' streams are
    whole, and the canary behind every slot (the bytes of the short slot's missing byte included) is untouched."""
    lib = _lib.load()
    data = np.random.default_rng(7).integers(0, 64, 5000, dtype=np.uint8)
    want = G.lzw_encode(data)
    n, L = data.size, len(want)
    gap = 64
    caps = np.array([L, L - 1, L], np.int32)
    dst_off = np.array([0, L + gap, 2 * (L + gap)], np.int64)
    src = torch.from_numpy(np.tile(data, 3)).to(dev)
    src_off = torch.tensor([0, n, 2 * n], dtype=torch.int64, device=dev)
    src_len = torch.tensor([n, n, n], dtype=torch.int32, device=dev)
    dst = torch.full((3 * (L + gap),), 0xA5, dtype=torch.uint8, device=dev)
    dst_len = torch.full((3,), -7, dtype=torch.int32, device=dev)
    d_off, d_cap = torch.from_numpy(dst_off).to(dev), torch.from_numpy(caps).to(dev)
    rc = lib.msr_lzw_encode_strips(None, src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), 3, 0, 0, dst.data_ptr(),
                                   d_off.data_ptr(), d_cap.data_ptr(), dst_len.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == _lib.MSR_OK
    torch.cuda.synchronize(dev)
    out = dst.cpu().numpy()
    assert dst_len.cpu().tolist() == [L, -1, L]
    for i in (0, 2):
        assert out[dst_off[i]:dst_off[i] + L].tobytes() == want
    for i in range(3):
        behind = out[dst_off[i] + caps[i]:dst_off[i] + L + gap]
        assert behind.size >= gap and (behind == 0xA5).all(), f"slot {i}: bytes written at or beyond its capacity"
    # the wrapper turns the -1 of a slot that is too small into a ValueError; its own slots never are
    assert G.lzw_encode_device(src, [0, n, 2 * n], [n, n, n]) == [want] * 3


def test_predictor_in_the_fetch(dev):
    """sample_bytes 1 / 2 / 4 on strips of several rows against NumPy differencing + the host encoder, with rows whose byte
    count is no multiple of the 256-byte fetch, so samples' predecessors lie in the previous chunk and rows restart inside one."""
    rng = np.random.default_rng(3)
    for sb, cols, rows in ((1, 301, 7), (2, 257, 5), (4, 300, 6), (4, 1, 3), (2, 70001, 2)):
        u = np.cumsum(rng.integers(-3, 4, (2 * rows, cols)), axis=1).astype(np.dtype(f"<u{sb}"))
        d = u.copy()
        d[:, 1:] = u[:, 1:] - u[:, :-1]
        rb = cols * sb
        got = _streams(dev, u.view(np.uint8).reshape(-1), [0, rows * rb], [rows * rb] * 2, sample_bytes=sb, row_bytes=rb)
        assert got == [G.lzw_encode(d[:rows]), G.lzw_encode(d[rows:])], (sb, cols, rows)


def _data(shape, dtype, seed=5):
    h, w = shape
    img, dem = synthetic_raster(h, w, seed, hole=(h // 4, h // 2, w // 4, w // 2) if h > 8 and w > 8 else None)
    return dem if dtype == np.float32 else (img * (60000 if dtype == np.uint16 else 255)).astype(dtype)


def _geo_meta():
    import struct
    return {"geo": {33550: (12, 3, struct.pack("<3d", 5.0, 5.0, 0.0)),
                    33922: (12, 6, struct.pack("<6d", 0, 0, 0, 7000.0, 900.0, 0))}, "byteorder": "<"}


def _both(tmp_path, data, dtype, device_data=None, **kw):
    """The file by either encoder; returns the device-written path after asserting the two are the same bytes and that
    libtiff reads the data back from it."""
    from PIL import Image
    hp, dp = str(tmp_path / "host.tif"), str(tmp_path / "device.tif")
    common = {k: v for k, v in kw.items() if k != "band_bytes"}
    G.write_geotiff(hp, data, _geo_meta(), nodata=NOVAL, dtype=dtype, **common)
    G.write_geotiff(dp, data if device_data is None else device_data, _geo_meta(), nodata=NOVAL, dtype=dtype,
                    encoder="device", **kw)
    with open(hp, "rb") as a, open(dp, "rb") as b:
        assert a.read() == b.read()
    with Image.open(dp) as im:
        back = np.array(im)
    assert back.shape == data.shape and np.array_equal(back.astype(np.float64), data.astype(dtype).astype(np.float64))
    return dp


@pytest.mark.parametrize("predictor", [2, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.uint8])
@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (5, 70001), (130, 300), (700, 257)])
def test_whole_files(dev, tmp_path, shape, dtype, predictor):
    """One row per strip with an odd width; several rows per 64 KiB strip (the predictor restarts inside a strip) with a
    short last strip; 1-pixel rasters."""
    _both(tmp_path, _data(shape, dtype), dtype, predictor=predictor, device=dev)


def test_whole_file_bigtiff(dev, tmp_path):
    _both(tmp_path, _data((130, 300), np.float32), np.float32, bigtiff=True, device=dev)


def test_whole_file_in_bands(dev, tmp_path):
    """700 x 257 float32 is 11 strips of 63 rows; 150000 bytes per band hold two of them: six bands."""
    assert len(G.plan_bands(700, 257 * 4, 63, 150000)) == 6
    _both(tmp_path, _data((700, 257), np.float32), np.float32, device=dev, band_bytes=150000)
    _both(tmp_path, _data((5, 70001), np.uint16), np.uint16, device=dev, band_bytes=1)      # a band per strip


def test_whole_file_from_a_device_tensor(dev, tmp_path):
    dem = _data((130, 300), np.float32)
    _both(tmp_path, dem, np.float32, device_data=torch.from_numpy(dem).to(dev))             # device defaults to the tensor's
    good = (np.arange(130 * 300).reshape(130, 300) % 41).astype(np.float32)                 # converted on the device
    _both(tmp_path, good, np.uint16, device_data=torch.from_numpy(good).to(dev))
    _both(tmp_path, good.astype(np.uint8), np.uint16, device_data=torch.from_numpy(good.astype(np.uint8)).to(dev))


def test_driver_writes_the_same_files(dev, tmp_path):
    """processFiles() with encoder="device" leaves the three files an object with the default encoder leaves (geometry
    and identity model of test_gpu_tiler.py::test_files_in_files_out)."""
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, HaloShardedSuperResolution

    def identity(x, training=False):
        return np.asarray(x, np.float32)

    img, dem = synthetic_raster(180, 260, 12, hole=(60, 90, 100, 150))
    src = tmp_path / "src"
    src.mkdir()
    G.write_geotiff(str(src / "run-DRG.tif"), img, _geo_meta(), nodata=NOVAL)
    G.write_geotiff(str(src / "run-DEM.tif"), dem, _geo_meta(), nodata=NOVAL)
    files = {}
    for enc, cls in ((None, DEMSuperResolution), ("device", DEMSuperResolution), ("device", HaloShardedSuperResolution)):
        out = tmp_path / f"out_{enc}_{cls.__name__}"
        cfg = DSRConfig(image_size=64, stride=16, batch_size=4, tile_size=128, map_name="apollo", save_path=str(out),
                        source_folder_path=str(src))
        d = cls(cfg, model=identity) if enc is None else cls(cfg, model=identity, encoder=enc)
        assert d.encoder == (enc or "host")
        d.processFiles(preprocess=False)
        d.close()
        files[(enc, cls)] = [(out / f"apollo_{name}.tiff").read_bytes() for name in ("mean", "std", "good")]
    ref = files[(None, DEMSuperResolution)]
    assert all(len(f) > 8 for f in ref)
    assert files[("device", DEMSuperResolution)] == ref and files[("device", HaloShardedSuperResolution)] == ref
    with pytest.raises(ValueError):
        DEMSuperResolution(DSRConfig(image_size=64, stride=16, batch_size=4, tile_size=128), model=identity, encoder="gpu")

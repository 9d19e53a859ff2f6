"""CPU: the parts of the device GeoTIFF encoder that need no GPU — the keyword checks of write_geotiff, the band planner,
the declaration of msr_lzw_encode_strips and its argument errors (which return before any launch)."""
import ctypes as C
import os

import numpy as np
import pytest

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G

SHAPES = [((1, 1), 4), ((3, 1), 4), ((5, 70001), 4), ((130, 300), 4), ((700, 257), 4), ((15000, 70000), 4),
          ((130, 300), 2), ((700, 257), 1)]


def test_keyword_errors(tmp_path):
    a = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match="encoder"):
        G.write_geotiff(str(tmp_path / "a.tif"), a, encoder="gpu")
    with pytest.raises(ValueError, match="LZW only"):
        G.write_geotiff(str(tmp_path / "a.tif"), a, compress="deflate", encoder="device")
    with pytest.raises(ValueError, match="LZW only"):
        G.write_geotiff(str(tmp_path / "a.tif"), a, compress="none", encoder="device")
    assert not (tmp_path / "a.tif").exists()


def test_device_encoder_without_a_gpu_is_an_error(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.write_geotiff(str(tmp_path / "a.tif"), np.zeros((4, 4), np.float32), encoder="device")
    assert not (tmp_path / "a.tif").exists()


def test_default_encoder_is_the_host_one(tmp_path):
    a = np.arange(35, dtype=np.float32).reshape(5, 7)
    G.write_geotiff(str(tmp_path / "a.tif"), a)
    G.write_geotiff(str(tmp_path / "b.tif"), a, encoder="host", device=3, band_bytes=1)
    assert (tmp_path / "a.tif").read_bytes() == (tmp_path / "b.tif").read_bytes()
    assert np.array_equal(G.read_geotiff(str(tmp_path / "a.tif"))[0], a)


@pytest.mark.parametrize("shape,itemsize", SHAPES)
@pytest.mark.parametrize("band_bytes", [1, 1000, 65536, 300000, 1 << 20, 256 << 20])
def test_band_planner(shape, itemsize, band_bytes):
    rows, cols = shape
    row_bytes = cols * itemsize
    rps = G._rows_per_strip(rows, row_bytes)
    n_strips = -(-rows // rps)
    bands = G.plan_bands(rows, row_bytes, rps, band_bytes)
    # whole strips, every strip once, in order
    assert bands[0][0] == 0 and bands[-1][1] == n_strips
    assert all(a1 == b0 for (_, a1), (b0, _) in zip(bands, bands[1:]))
    assert all(s1 > s0 for s0, s1 in bands)
    for s0, s1 in bands:
        raw = (min(s1 * rps, rows) - s0 * rps) * row_bytes
        assert raw <= band_bytes or s1 - s0 == 1          # over the limit only when a single strip is
    # and a band is as full as whole full-size strips allow
    for s0, s1 in bands[:-1]:
        assert (s1 + 1 - s0) * rps * row_bytes > band_bytes


def test_band_planner_config3_product():
    """A float32 product of BASELINE configs[3]: one 280000-byte strip per row, 958 of them in a 256 MiB band."""
    rows, cols = 15000, 70000
    rps = G._rows_per_strip(rows, cols * 4)
    assert rps == 1
    bands = G.plan_bands(rows, cols * 4, rps, 256 << 20)
    assert bands[0] == (0, (256 << 20) // 280000) and len(bands) == -(-15000 // 958) and bands[-1][1] == 15000


def test_entry_is_declared():
    names = [s[0] for s in _lib.SYMBOLS]
    assert "msr_lzw_encode_strips" in names
    _, restype, argtypes = _lib.SYMBOLS[names.index("msr_lzw_encode_strips")]
    assert restype is C.c_int and len(argtypes) == 12
    assert [a for a in argtypes if a is C.c_int32] == [C.c_int32] * 3
    with open(os.path.join(_lib.CSRC, "..", "..", "include", "moonsr.h")) as fh:
        assert "int msr_lzw_encode_strips(msr_handle* h," in fh.read()


def test_argument_errors_return_before_any_launch():
    """Every call here is rejected (or has nothing to do) before a launch, so host arrays can stand in for device memory."""
    lib = _lib.load()
    assert lib.msr_abi_version() == 1
    b = np.zeros(64, np.uint8)
    o = np.zeros(2, np.int64)
    l32 = np.zeros(2, np.int32)
    p8, p64, p32 = b.ctypes.data, o.ctypes.data, l32.ctypes.data

    def call(args):
        return lib.msr_lzw_encode_strips(None, *args, None)

    good = [p8, p64, p32, 1, 0, 0, p8, p64, p32, p32]
    for i in (0, 1, 2, 6, 7, 8, 9):                        # each pointer in turn
        bad = list(good)
        bad[i] = None
        assert call(bad) == _lib.MSR_ERR_INVALID
        assert b"null" in lib.msr_last_error(None)
    assert call([p8, p64, p32, -1, 0, 0, p8, p64, p32, p32]) == _lib.MSR_ERR_INVALID
    assert b"n_strips" in lib.msr_last_error(None)
    for sb in (-1, 3, 5, 8):
        assert call([p8, p64, p32, 1, sb, 8 * 3 * 5, p8, p64, p32, p32]) == _lib.MSR_ERR_INVALID
        assert b"sample_bytes" in lib.msr_last_error(None)
    for sb, rb in ((1, 0), (2, 0), (4, 0), (2, -2), (2, 7), (4, 6), (4, -4)):
        assert call([p8, p64, p32, 1, sb, rb, p8, p64, p32, p32]) == _lib.MSR_ERR_INVALID
        assert b"row_bytes" in lib.msr_last_error(None)
    assert call([p8, p64, p32, 0, 4, 8, p8, p64, p32, p32]) == _lib.MSR_OK    # no strips: nothing to launch
    assert call([p8, p64, p32, 0, 0, 0, p8, p64, p32, p32]) == _lib.MSR_OK    # row_bytes is not looked at without a predictor

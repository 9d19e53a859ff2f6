"""CPU: the parts of the device GeoTIFF decoder that need no GPU — the keyword checks of read_geotiff and the driver, the
declaration of the three entries and the argument errors of the two device ones (which return before any launch), the band
planner, and the automaton the kernel runs (csrc/lzw_unstrip.h) run with one lane on the host (msr_lzw_decode_strip_host)
against msr_lzw_decode: return value, bytes [0, return value), zeroed tail, and 64 canary bytes behind ``cap``."""
import ctypes as C
import os

import numpy as np
import pytest

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from tests import geotiff_decode_cases as cases


# ---- keywords ------------------------------------------------------------------------------------------------------------
def _raster(dtype=np.float32):
    a = np.cumsum(np.random.default_rng(3).integers(-3, 4, (40, 50)), axis=1)
    return (a + 1000).astype(dtype)


def test_unknown_decoder(tmp_path):
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, _raster())
    with pytest.raises(ValueError, match="decoder"):
        G.read_geotiff(p, decoder="gpu")


def _unsupported(tmp_path):
    a = _raster()
    d = lambda name: str(tmp_path / name)                                   # noqa: E731
    G.write_geotiff(d("deflate.tif"), a, compress="deflate")
    G.write_geotiff(d("none.tif"), a, compress="none")
    G.write_geotiff(d("f64.tif"), a, dtype=np.float64)
    cases.write_tiled(d("pred3.tif"), [a], 16, 16, predictor_tag=3)
    cases.write_tiled(d("big_endian.tif"), [a], 16, 16, bo=">")
    cases.write_tiled(d("chunky.tif"), [a, a + 1], 16, 16, planar=1)
    return [("deflate.tif", "compression 8"), ("none.tif", "compression 1"), ("f64.tif", "64-bit"), ("pred3.tif", "predictor 3"),
            ("big_endian.tif", "big-endian"), ("chunky.tif", "chunky")]


def test_unsupported_properties_are_named_before_the_gpu_is_touched(tmp_path, monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("the device was asked for")
    forms = _unsupported(tmp_path)
    monkeypatch.setattr(G, "_torch_device", no_gpu)
    for name, what in forms:
        path = str(tmp_path / name)
        G.read_geotiff(path)                                                 # the host reader takes every one of them
        with pytest.raises(ValueError, match=what):
            G.read_geotiff(path, decoder="device")
        with pytest.raises(ValueError, match=what):
            G.read_geotiff(path, decoder="device", rows=(3, 9), as_tensor=True)


def test_device_decoder_without_a_gpu_is_an_error(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, _raster())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.read_geotiff(p, decoder="device")
    cases.write_tiled(str(tmp_path / "t.tif"), [_raster(np.uint16), _raster(np.uint16)], 16, 16, predictor=2)
    with pytest.raises(RuntimeError, match="decoder='device'"):
        G.read_geotiff(str(tmp_path / "t.tif"), band=2, decoder="device")


def test_default_decoder_is_the_host_one(tmp_path):
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, _raster())
    a, ma = G.read_geotiff(p)
    b, mb = G.read_geotiff(p, decoder="host", device=3, band_bytes=1)
    assert isinstance(b, np.ndarray) and np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ma == mb


def test_driver_keyword():
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, HaloShardedSuperResolution
    cfg = DSRConfig(image_size=64, stride=16, batch_size=4, tile_size=128)
    for cls in (DEMSuperResolution, HaloShardedSuperResolution):
        with pytest.raises(ValueError, match="decoder"):
            cls(cfg, decoder="gpu")


# ---- entries -------------------------------------------------------------------------------------------------------------
def test_entries_are_declared():
    names = [s[0] for s in _lib.SYMBOLS]
    with open(os.path.join(_lib.CSRC, "..", "..", "include", "moonsr.h")) as fh:
        header = fh.read()
    for name, nargs, decl in (("msr_lzw_decode_strips", 10, "int msr_lzw_decode_strips(msr_handle* h,"),
                              ("msr_tiff_blocks_to_f32", 16, "int msr_tiff_blocks_to_f32(msr_handle* h,"),
                              ("msr_lzw_decode_strip_host", 4, "int64_t msr_lzw_decode_strip_host(const uint8_t* in,")):
        assert name in names and decl in header
        assert len(_lib.SYMBOLS[names.index(name)][2]) == nargs
    assert hasattr(_lib.load(), "msr_lzw_decode_strip_host")


def test_argument_errors_return_before_any_launch():
    """Every call here is rejected (or has nothing to do) before a launch, so host arrays can stand in for device memory."""
    lib = _lib.load()
    b = np.zeros(64, np.uint8)
    o = np.zeros(2, np.int64)
    l32 = np.zeros(2, np.int32)
    f = np.zeros(16, np.float32)
    p8, p64, p32, pf = b.ctypes.data, o.ctypes.data, l32.ctypes.data, f.ctypes.data

    def dec(args):
        return lib.msr_lzw_decode_strips(None, *args, None)

    good = [p8, p64, p32, 1, p8, p64, p32, p32]
    for i in (0, 1, 2, 4, 5, 6, 7):
        bad = list(good)
        bad[i] = None
        assert dec(bad) == _lib.MSR_ERR_INVALID and b"null" in lib.msr_last_error(None)
    assert dec([p8, p64, p32, -1, p8, p64, p32, p32]) == _lib.MSR_ERR_INVALID
    assert b"n_strips" in lib.msr_last_error(None)
    assert dec([p8, p64, p32, 0, p8, p64, p32, p32]) == _lib.MSR_OK           # no blocks: nothing to launch

    def place(args):
        return lib.msr_tiff_blocks_to_f32(None, *args, None)

    #       src off  x0   y0   n  bw bh kind     sb pred out r0 rows cols
    good = [p8, p64, p32, p32, 1, 4, 2, ord("u"), 2, 2, pf, 0, 2, 4]
    for i in (0, 1, 2, 3, 10):
        bad = list(good)
        bad[i] = None
        assert place(bad) == _lib.MSR_ERR_INVALID and b"null" in lib.msr_last_error(None)

    def rejected(i, v, word):
        bad = list(good)
        bad[i] = v
        assert place(bad) == _lib.MSR_ERR_INVALID, (i, v)
        assert word in lib.msr_last_error(None), (i, v, lib.msr_last_error(None))

    rejected(4, -1, b"n_blocks")
    for kind in (0, ord("d"), ord("U"), 1):
        rejected(7, kind, b"sample_kind")
    for sb in (0, 3, 8, -1):
        rejected(8, sb, b"sample_bytes")
    for sb in (1, 2):                                                       # float samples are 4 bytes
        bad = list(good)
        bad[7], bad[8] = ord("f"), sb
        assert place(bad) == _lib.MSR_ERR_INVALID and b"sample_bytes" in lib.msr_last_error(None)
    for pred in (0, 3, -1):
        rejected(9, pred, b"predictor")
    for i in (5, 6, 12, 13):
        for v in (0, -1):
            rejected(i, v, b"geometry")
    rejected(11, -1, b"geometry")
    bad = list(good)
    bad[4] = 0
    assert place(bad) == _lib.MSR_OK                                          # no blocks: nothing to launch


# ---- band planner ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,block_h,block_row_bytes", [(1, 1, 4), (75, 8, 8 * 96 * 4), (130, 16, 19 * 16 * 16 * 4),
                                                          (700, 63, 63 * 257 * 4), (700, 256, 2 * 256 * 256 * 2),
                                                          (15000, 1, 280000)])
@pytest.mark.parametrize("band_bytes", [1, 1000, 65536, 300000, 1 << 20, 256 << 20])
def test_band_planner(rows, block_h, block_row_bytes, band_bytes):
    down = -(-rows // block_h)
    windows = {(0, rows), (0, 1), (rows - 1, rows), (rows // 3, rows // 3 + 1), (rows // 4, max(rows // 4 + 1, 3 * rows // 4))}
    for r0, r1 in sorted(windows):
        bands = G.plan_read_bands(r0, r1, block_h, block_row_bytes, band_bytes)
        first, last = r0 // block_h, -(-r1 // block_h)
        # whole block rows, every intersecting one once and in order, nothing outside the window
        assert bands[0][0] == first and bands[-1][1] == last <= down
        assert all(a1 == b0 for (_, a1), (b0, _) in zip(bands, bands[1:]))
        assert all(b1 > b0 for b0, b1 in bands)
        assert first * block_h <= r0 < (first + 1) * block_h and (last - 1) * block_h < r1 <= last * block_h
        for b0, b1 in bands:
            assert (b1 - b0) * block_row_bytes <= band_bytes or b1 - b0 == 1     # over the limit only when one block row is
        for b0, b1 in bands[:-1]:                                               # and a band is as full as the limit allows
            assert (b1 + 1 - b0) * block_row_bytes > band_bytes


def test_band_planner_config3_input():
    """An input of BASELINE configs[3]: 15000 x 70000 float32, one 280000-byte strip per row, 958 of them in a 256 MiB band;
    rank 3 of 8's 4096 rows are five bands."""
    assert G._rows_per_strip(15000, 70000 * 4) == 1
    bands = G.plan_read_bands(0, 15000, 1, 280000, 256 << 20)
    assert bands[0] == (0, (256 << 20) // 280000) and len(bands) == -(-15000 // 958) and bands[-1][1] == 15000
    bands = G.plan_read_bands(5000, 9096, 1, 280000, 256 << 20)
    assert bands[0] == (5000, 5958) and bands[-1][1] == 9096 and len(bands) == 5


# ---- the automaton -----------------------------------------------------------------------------------------------------------
def _one_lane(stream: bytes, cap: int):
    """msr_lzw_decode_strip_host on exact-length arrays with a canary behind cap: (return value, the slot's cap bytes)."""
    lib = _lib.load()
    src = np.frombuffer(stream.ljust(1, b"\0"), np.uint8)
    out = np.full(cap + cases.CANARY, 0xA5, np.uint8)
    n = lib.msr_lzw_decode_strip_host(src.ctypes.data, len(stream), out.ctypes.data, cap)
    assert (out[cap:] == 0xA5).all(), "bytes written at or beyond cap"
    return n, out[:cap]


def _check(case_list):
    bad = []
    for name, stream, cap in case_list:
        want, data = cases.host_decode(stream, cap)
        got, out = _one_lane(stream, cap)
        if got != want or (want >= 0 and (out[:want].tobytes() != data or out[want:].any())):
            bad.append((name, got, want))
    assert not bad, f"{len(bad)} of {len(case_list)} differ from msr_lzw_decode, the first: {bad[0]}"


def test_automaton_prefix_sweep():
    sweep = cases.prefix_cases()
    assert len(sweep) == 4402
    _check(sweep)
    buf = cases.random_buffer()
    for name, stream, cap in sweep[::397]:                                   # and the reference decodes what was encoded
        assert cases.host_decode(stream, cap) == (cap, buf[:cap].tobytes())


def test_automaton_long_matches():
    _check(cases.long_match_cases())
    for name, stream, cap in cases.long_match_cases():
        assert cases.host_decode(stream, cap)[0] == cap


def test_automaton_libtiff_strips():
    strips = cases.libtiff_cases()
    assert len(strips) >= 30
    _check(strips)
    assert all(cases.host_decode(s, cap)[0] == cap for _, s, cap in strips)


def test_automaton_hand_packed_and_malformed():
    hand = cases.hand_cases()
    _check(hand)
    by_name = {name: (stream, cap) for name, stream, cap in hand}
    for name, text in cases.HAND_EXPECT.items():
        assert cases.host_decode(*by_name[name]) == (len(text), text), name
    four, buf = cases.four_symbols(), cases.random_buffer().tobytes()
    for name, text in (("never clears", four), ("never clears, no leading Clear", four), ("never clears, random", buf)):
        assert cases.host_decode(*by_name[name]) == (len(text), text), name   # 12-bit codes after the table is full
    for name in ("cap one short", "cap 0", "cap one short, random", "code above next", "code next + 1",
                 "first code 258 after Clear", "first code 300 after a later Clear", "first code 258 without a Clear"):
        assert cases.host_decode(*by_name[name])[0] == -1, name
    assert cases.host_decode(*by_name["short output"])[0] == 700
    got = [cases.host_decode(s, cap)[0] for name, s, cap in hand if name.startswith(("bit flip", "garbage"))]
    assert len(got) == 300 and -1 in got and any(g >= 0 for g in got)       # both outcomes are in the corpus


def test_one_lane_entry_rejects_bad_arguments():
    lib = _lib.load()
    b = np.zeros(8, np.uint8)
    assert lib.msr_lzw_decode_strip_host(None, 0, b.ctypes.data, 8) == -1
    assert lib.msr_lzw_decode_strip_host(b.ctypes.data, 8, None, 8) == -1
    assert lib.msr_lzw_decode_strip_host(b.ctypes.data, -1, b.ctypes.data, 8) == -1
    assert lib.msr_lzw_decode_strip_host(b.ctypes.data, 8, b.ctypes.data, -1) == -1
    assert lib.msr_lzw_decode_strip_host(b.ctypes.data, 1 << 31, b.ctypes.data, 8) == -1

"""GPU: the device GeoTIFF decoder (csrc/geotiff_codec.hip, csrc/lzw_unstrip.h) against the host one (csrc/host_codecs.cpp
and the NumPy of geotiff.read_geotiff).  Everything is compared bit for bit (float arrays through their uint32 view, so
NaNs count): every block's return value and bytes with msr_lzw_decode's, the placement kernel with NumPy's cumsum and
assignment, and every read with ``decoder="device"`` with the read with ``decoder="host"``."""
import ctypes as C

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from tests import geotiff_decode_cases as cases
from tests.helpers import synthetic_raster

pytestmark = pytest.mark.gpu
NOVAL = -32768.0


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


# ---- msr_lzw_decode_strips -------------------------------------------------------------------------------------------------
def _launch(dev, case_list, caps=None):
    """One msr_lzw_decode_strips launch over the streams of ``case_list``, each slot followed by a canary: the dst_len list and,
    per case, its slot's cap bytes.  Asserts that every canary is untouched."""
    lib = _lib.load()
    streams = [s for _, s, _ in case_list]
    caps = np.array([c for _, _, c in case_list] if caps is None else caps, np.int64)
    lens = np.array([len(s) for s in streams], np.int64)
    src_off = np.concatenate(([0], np.cumsum(lens)[:-1]))
    dst_off = np.concatenate(([0], np.cumsum(caps + cases.CANARY)[:-1]))
    n = len(streams)
    src = torch.from_numpy(np.frombuffer(b"".join(streams).ljust(1, b"\0"), np.uint8).copy()).to(dev)
    dst = torch.full((int((caps + cases.CANARY).sum()),), 0xA5, dtype=torch.uint8, device=dev)
    dst_len = torch.full((n,), -7, dtype=torch.int32, device=dev)
    t64 = torch.from_numpy(np.concatenate([src_off, dst_off])).to(dev)
    t32 = torch.from_numpy(np.concatenate([lens, caps]).astype(np.int32)).to(dev)
    rc = lib.msr_lzw_decode_strips(None, src.data_ptr(), t64.data_ptr(), t32.data_ptr(), n, dst.data_ptr(), t64.data_ptr() + 8 * n,
                                   t32.data_ptr() + 4 * n, dst_len.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == _lib.MSR_OK
    torch.cuda.synchronize(dev)
    out = dst.cpu().numpy()
    slots = []
    for i, (o, c) in enumerate(zip(dst_off.tolist(), caps.tolist())):
        assert (out[o + c:o + c + cases.CANARY] == 0xA5).all(), f"{case_list[i][0]}: bytes written at or beyond its capacity"
        slots.append(out[o:o + c])
    return dst_len.cpu().tolist(), slots


def _against_the_host(dev, case_list):
    got, slots = _launch(dev, case_list)
    bad = []
    for (name, stream, cap), n, slot in zip(case_list, got, slots):
        want, data = cases.host_decode(stream, cap)
        if n != want or (want >= 0 and (slot[:want].tobytes() != data or slot[want:].any())):
            bad.append((name, n, want))
    assert not bad, f"{len(bad)} of {len(case_list)} blocks differ from msr_lzw_decode, the first: {bad[0]}"
    return got


def test_prefix_sweep_one_launch(dev):
    """4402 blocks of different lengths side by side in ONE launch: the empty and the 1-byte block, every width change, the first
    Clear and a second dictionary, three Clears in the whole buffer."""
    sweep = cases.prefix_cases()
    assert len(sweep) == 4402
    assert _against_the_host(dev, sweep) == [cap for _, _, cap in sweep]


def test_long_matches_one_launch(dev):
    long = cases.long_match_cases()
    assert _against_the_host(dev, long) == [cap for _, _, cap in long]


def test_libtiff_strips_one_launch(dev):
    strips = cases.libtiff_cases()
    assert _against_the_host(dev, strips) == [cap for _, _, cap in strips]


def test_capacity_is_a_hard_bound(dev):
    """Three equal blocks, the middle slot one byte short: lengths [L, -1, L], whole neighbours, every canary untouched (_launch)."""
    data = np.random.default_rng(7).integers(0, 64, 5000, dtype=np.uint8)
    stream, L = G.lzw_encode(data), data.size
    got, slots = _launch(dev, [("a", stream, L), ("short", stream, L - 1), ("b", stream, L)])
    assert got == [L, -1, L]
    assert slots[0].tobytes() == data.tobytes() and slots[2].tobytes() == data.tobytes()
    # the wrapper returns the blocks with zeroed tails, and turns a -1 into the host path's error
    src =torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(dev)
    assert G.lzw_decode_device_bytes(src, [0, 0], [len(stream)] * 2, [L, L + 9]) == [data.tobytes(), data.tobytes() + bytes(9)]
    with pytest.raises(ValueError, match="malformed LZW stream"):
        G.lzw_decode_device(src, [0, 0], [len(stream)] * 2, [L, L - 1])


def test_negative_length_gives_minus_one(dev):
    lib = _lib.load()
    stream = G.lzw_encode(np.arange(200, dtype=np.uint8))
    src = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(dev)
    t64 = torch.tensor([0, 0, 0, 256], dtype=torch.int64, device=dev)                    # src_off | dst_off
    t32 = torch.tensor([-1, len(stream), 200, 200], dtype=torch.int32, device=dev)       # src_len | dst_cap
    dst = torch.full((512,), 0xA5, dtype=torch.uint8, device=dev)
    dst_len = torch.full((2,), -7, dtype=torch.int32, device=dev)
    rc = lib.msr_lzw_decode_strips(None, src.data_ptr(), t64.data_ptr(), t32.data_ptr(), 2, dst.data_ptr(), t64.data_ptr() + 16,
                                   t32.data_ptr() + 8, dst_len.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == _lib.MSR_OK
    assert dst_len.cpu().tolist() == [-1, 200]
    out = dst.cpu().numpy()
    assert (out[:256] == 0xA5).all() and out[256:456].tobytes() == bytes(range(200)) and (out[456:] == 0xA5).all()


def test_hand_packed_and_malformed_one_launch(dev):
    """The list tests/test_geotiff_decode_host.py passes on the host, unchanged, in one launch: dst_len is the host's return value
    per block, the tails are zeroed and the canaries intact."""
    hand = cases.hand_cases()
    got = _against_the_host(dev, hand)
    by_name = dict(zip((name for name, _, _ in hand), got))
    assert by_name["never clears"] == len(cases.four_symbols()) and by_name["cap one short"] == -1
    assert by_name["code above next"] == -1 and by_name["short output"] == 700 and by_name["empty"] == 0


# ---- msr_tiff_blocks_to_f32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predictor", [2, 1])
@pytest.mark.parametrize("kind,sb,bw,bh", [("u", 1, 301, 7), ("i", 2, 257, 5), ("u", 2, 70001, 2), ("f", 4, 300, 6), ("i", 4, 1, 3),
                                           ("u", 4, 64, 1)])
def test_blocks_to_f32(dev, kind, sb, bw, bh, predictor):
    """A 2 x 3 grid of blocks that hangs over the right and the bottom edge of the raster, one block left out, every other
    block at an odd byte offset; the window starts and ends inside a block; the output, and a guard row either side of it,
    are pre-filled with a pattern that must survive outside the written footprint."""
    lib = _lib.load()
    rng = np.random.default_rng(sb * 1000 + bw)
    dt, ut = np.dtype(f"<{kind}{sb}"), np.dtype(f"<u{sb}")
    cols = bw + bw // 2 + 1 if bw > 1 else 2
    rows = 2 * bh + max(1, bh // 2)
    r0, r1 = (bh // 2, rows - 1) if bh >= 3 else (0, rows)
    grid = [(bx, by) for by in range(3) for bx in range(2)]
    blocks, offs, pos = [], [], 0
    for i, (bx, by) in enumerate(grid):
        want = rng.integers(0, 1 << (8 * sb), (bh, bw), dtype=np.uint64).astype(ut)
        if kind == "f":
            f = (-2000 + 300 * rng.standard_normal((bh, bw))).astype(np.float32)
            f[0, :3] = NOVAL
            f[bh - 1, bw // 2] = np.nan
            want = f.view(np.uint32).copy()
            want[1, 5], want[2, 7] = 0x7FC12345, 0xFFC00001                  # NaNs with a payload
        raw = want.copy()
        if predictor == 2:
            raw[:, 1:] = want[:, 1:] - want[:, :-1]
        pos += i & 1                                                         # an odd offset for every other block
        offs.append(pos)
        blocks.append(raw)
        pos += raw.nbytes
    src = np.zeros(pos + 1, np.uint8)
    for o, raw in zip(offs, blocks):
        src[o:o + raw.nbytes] = raw.view(np.uint8).reshape(-1)
    skip = 3                                                                 # this block is not in the list
    use = [i for i in range(len(grid)) if i != skip]
    pattern = (np.arange((r1 - r0 + 2) * cols, dtype=np.float32).reshape(-1, cols) * 0.5 - 77).astype(np.float32)
    expect = pattern.copy()
    for i in use:
        bx, by = grid[i]
        raw = blocks[i]
        u = np.cumsum(raw, axis=1, dtype=ut) if predictor == 2 else raw      # NumPy on the unsigned view, as read_geotiff does
        val = u.view(dt)
        x0, y0 = bx * bw, by * bh
        ya, yb = max(y0, r0), min(y0 + bh, rows, r1)
        ww = min(bw, cols - x0)
        if ya < yb and ww > 0:
            expect[1 + ya - r0:1 + yb - r0, x0:x0 + ww] = val[ya - y0:yb - y0, :ww]
    out = torch.from_numpy(pattern).to(dev)
    d_src = torch.from_numpy(src).to(dev)
    d_off = torch.tensor([offs[i] for i in use], dtype=torch.int64, device=dev)
    d_xy = torch.tensor([grid[i][0] * bw for i in use] + [grid[i][1] * bh for i in use], dtype=torch.int32, device=dev)
    n = len(use)
    rc = lib.msr_tiff_blocks_to_f32(None, d_src.data_ptr(), d_off.data_ptr(), d_xy.data_ptr(), d_xy.data_ptr() + 4 * n, n, bw, bh,
                                    ord(kind), sb, predictor, out.data_ptr() + 4 * cols, r0, r1 - r0, cols,
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == _lib.MSR_OK
    got = out.cpu().numpy()
    assert np.array_equal(got[0].view(np.uint32), pattern[0].view(np.uint32)), "the row before the window was written"
    assert np.array_equal(got[-1].view(np.uint32), pattern[-1].view(np.uint32)), "the row behind the window was written"
    diff = got.view(np.uint32) != expect.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} values differ, the first at {tuple(np.argwhere(diff)[0])} (guard row included)"
    assert (expect != pattern).any()


# ---- whole files -------------------------------------------------------------------------------------------------------------
def _data(shape, dtype, seed=5):
    h, w = shape
    img, dem = synthetic_raster(h, w, seed, hole=(h // 4, h // 2, w // 4, w // 2) if h > 8 and w > 8 else None)
    if dtype == np.float32:
        return dem
    if dtype == np.int16:
        return (img * 60000 - 30000).astype(np.int16)
    return (img * (60000 if dtype == np.uint16 else 255)).astype(dtype)


def _same(path, dev, **kw):
    """The read by either decoder is the same bits and the same meta; returns the host read."""
    host, hmeta = G.read_geotiff(path, **{k: v for k, v in kw.items() if k not in ("band_bytes",)})
    got, meta = G.read_geotiff(path, decoder="device", device=dev, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == host.shape
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))
    assert meta == hmeta
    return host


@pytest.mark.parametrize("predictor", [2, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.int16, np.uint8])
@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (5, 70001), (130, 300), (700, 257)])
def test_whole_files(dev, tmp_path, shape, dtype, predictor):
    p = str(tmp_path / "a.tif")
    data = _data(shape, dtype)
    if dtype == np.float32 and shape[0] > 8:
        data = data.copy()
        data[2, 1] = np.nan
        data.view(np.uint32)[3, 2] = 0x7FC12345
    G.write_geotiff(p, data, nodata=NOVAL, dtype=dtype, predictor=predictor)
    host = _same(p, dev)
    assert np.array_equal(host.view(np.uint32), data.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("form", ["u16_pred2", "f32", "u8"])
def test_libtiff_written_files(dev, tmp_path, form):
    from PIL import Image
    p = str(tmp_path / "a.tif")
    if form == "u16_pred2":
        Image.fromarray(_data((130, 300), np.uint16)).save(p, compression="tiff_lzw", tiffinfo={317: 2})
    elif form == "f32":
        Image.fromarray(_data((130, 300), np.float32), mode="F").save(p, compression="tiff_lzw", tiffinfo={278: 8})
    else:
        Image.fromarray(_data((700, 257), np.uint8)).save(p, compression="tiff_lzw")
    _same(p, dev)
    _same(p, dev, rows=(7, 100))


def test_bigtiff(dev, tmp_path):
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, _data((130, 300), np.float32), nodata=NOVAL, bigtiff=True)
    _same(p, dev)
    cases.write_tiled(str(tmp_path / "t.tif"), [_data((130, 300), np.uint16)], 16, 16, predictor=2, bigtiff=True)
    _same(str(tmp_path / "t.tif"), dev)


@pytest.mark.parametrize("tile", [16, 256])
@pytest.mark.parametrize("shape,dtype,predictor", [((130, 300), np.float32, 2), ((700, 257), np.uint16, 2),
                                                   ((700, 257), np.float32, 1), ((130, 300), np.int16, 2)])
def test_tiled_files(dev, tmp_path, tile, shape, dtype, predictor):
    """Hand-built little-endian tiled files with partial edge tiles."""
    p = str(tmp_path / "t.tif")
    data = _data(shape, dtype)
    cases.write_tiled(p, [data], tile, tile, predictor=predictor)
    host = _same(p, dev)
    assert np.array_equal(host, data.astype(np.float32), equal_nan=True)
    _same(p, dev, band_bytes=1)


def test_planar_two_band_file(dev, tmp_path):
    p = str(tmp_path / "t.tif")
    a, b = _data((130, 300), np.uint16, seed=5), _data((130, 300), np.uint16, seed=6)
    cases.write_tiled(p, [a, b], 16, 16, predictor=2)
    assert np.array_equal(_same(p, dev, band=2), b.astype(np.float32))
    assert np.array_equal(_same(p, dev, band=1), a.astype(np.float32))
    assert np.array_equal(_same(p, dev, band=2, rows=(20, 50)), b[20:50].astype(np.float32))


@pytest.mark.parametrize("form", ["strips", "tiles"])
def test_row_windows(dev, tmp_path, form):
    """(0, 1), (H - 1, H), a window inside one block and one crossing three block rows: each is the slice of the full host read."""
    p = str(tmp_path / "w.tif")
    if form == "strips":
        H, data = 700, _data((700, 257), np.float32)                         # strips of 63 rows
        G.write_geotiff(p, data, nodata=NOVAL)
        windows = [(0, 1), (H - 1, H), (70, 80), (100, 200)]
    else:
        H, data = 130, _data((130, 300), np.float32)
        cases.write_tiled(p, [data], 16, 16, predictor=2)
        windows = [(0, 1), (H - 1, H), (17, 30), (20, 50)]
    full, fmeta = G.read_geotiff(p)
    for r0, r1 in windows:
        win = _same(p, dev, rows=(r0, r1))
        assert np.array_equal(win.view(np.uint32), full[r0:r1].view(np.uint32))
        _, meta = G.read_geotiff(p, rows=(r0, r1), decoder="device", device=dev)
        assert meta == dict(fmeta, window=(r0, r1))


def test_bands(dev, tmp_path):
    """700 x 257 float32 is 12 strips of 63 rows; 150000 bytes per band hold two of them: six bands."""
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, _data((700, 257), np.float32), nodata=NOVAL)
    assert len(G.plan_read_bands(0, 700, 63, 63 * 257 * 4, 150000)) == 6
    assert len(G.plan_read_bands(0, 700, 63, 63 * 257 * 4, 1)) == 12
    _same(p, dev)
    _same(p, dev, band_bytes=1)
    _same(p, dev, band_bytes=150000)
    _same(p, dev, band_bytes=150000, rows=(100, 400))


def test_tensor_output(dev, tmp_path):
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, _data((130, 300), np.float32), nodata=NOVAL)
    host, hmeta = G.read_geotiff(p, rows=(3, 77))
    t, meta = G.read_geotiff(p, rows=(3, 77), decoder="device", device=dev, as_tensor=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == host.shape
    assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32)) and meta == hmeta


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _geo_meta():
    import struct
    return {"geo": {33550: (12, 3, struct.pack("<3d", 5.0, 5.0, 0.0)),
                    33922: (12, 6, struct.pack("<6d", 0, 0, 0, 7000.0, 900.0, 0))}, "byteorder": "<"}


def test_driver_reads_the_same_rasters(dev, tmp_path):
    """processFiles() with decoder="device" leaves the three files an object with the default decoder leaves (geometry and
    identity model of test_gpu_geotiff_encode.py::test_driver_writes_the_same_files), whole raster, halo, and as rank 1 of 2 of
    a tile-row-sharded run (which reads a row window)."""
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, HaloShardedSuperResolution

    def identity(x, training=False):
        return np.asarray(x, np.float32)

    img, dem = synthetic_raster(180, 260, 12, hole=(60, 90, 100, 150))
    src = tmp_path / "src"
    src.mkdir()
    G.write_geotiff(str(src / "run-DRG.tif"), img, _geo_meta(), nodata=NOVAL)
    G.write_geotiff(str(src / "run-DEM.tif"), dem, _geo_meta(), nodata=NOVAL)
    files = {}
    runs = [(None, DEMSuperResolution, {}), ("device", DEMSuperResolution, {}), ("device", HaloShardedSuperResolution, {}),
            (None, DEMSuperResolution, dict(rank=1, world=2, mode="tiles", gather=False)),
            ("device", DEMSuperResolution, dict(rank=1, world=2, mode="tiles", gather=False))]
    for dec, cls, kw in runs:
        out = tmp_path / f"out_{dec}_{cls.__name__}_{len(kw)}"
        cfg = DSRConfig(image_size=64, stride=16, batch_size=4, tile_size=128, map_name="apollo", save_path=str(out),
                        source_folder_path=str(src))
        d = cls(cfg, model=identity) if dec is None else cls(cfg, model=identity, decoder=dec)
        assert d.decoder == (dec or "host") and d.encoder == "host"
        d.processFiles(preprocess=False, **kw)
        d.close()
        files[(dec, cls, len(kw))] = [(out / f"apollo_{name}.tiff").read_bytes() for name in ("mean", "std", "good")]
    ref = files[(None, DEMSuperResolution, 0)]
    assert all(len(f) > 8 for f in ref)
    assert files[("device", DEMSuperResolution, 0)] == ref and files[("device", HaloShardedSuperResolution, 0)] == ref
    assert files[("device", DEMSuperResolution, 4)] == files[(None, DEMSuperResolution, 4)] != ref

"""GPU (-m gpu): tiled GeoTIFF products with overviews built on the device.

  1. msr_overview_half (csrc/tiff_overview.hip) equals the twin geotiff.overview_reference bit for bit, with canaries behind
     dst: one pixel, one row / column of blocks, odd shapes, more than one workgroup across and down; float32 with a no-data
     pattern in which every count 0 .. 4 occurs, NaNs and both zeros; float32 without no-data; uint8 and uint16;
  2. the files of write_geotiff(encoder="device", tile=, overviews=) equal the host-encoded files byte for byte: over the shapes,
     dtypes, predictors and tiles of the CPU list, with band_bytes=1 (one tile row per band, several bands) and the default,
     from a NumPy array and from a CUDA tensor, overviews 0 and 2; a uint8 tensor into a uint16 file; and the device encoder
     and decoder meet the digests pinned in tests/golden/geotiff_bytes.json (strips too; tests/geotiff_pinned_cases.py);
  3. read_geotiff(decoder="device", overview=k) returns the host reader's bits;
  4. the driver: product_tile=(16, 16), overviews=2, encoder="device", resident=True on the smallest raster of
     tests/resident_cases.py — level 0 of each product equals the raster of the strip-layout run, levels 1 and 2 the twin, and
     ``transfers`` holds no raw product: each direction is bounded by the file sizes plus 64 B a block.
All comparisons are exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from tests import geotiff_pinned_cases as pinned
from tests import geotiff_tiled_cases as cases
from tests import resident_cases

pytestmark = pytest.mark.gpu
NV = cases.NOVAL


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


# ---- 1. the reduction --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind,has_nodata", cases.reduce_cases())
def test_overview_half_equals_the_twin(dev, shape, kind, has_nodata):
    lib = _lib.load()
    a = cases.reduce_input(shape, kind)
    if kind == "nodata" and shape[0] >= 2 and shape[1] >= 10:
        assert cases.counts_of(a) == {0, 1, 2, 3, 4}
    want = G.overview_reference(a, NV if has_nodata else None)
    ub = np.dtype(f"u{a.dtype.itemsize}")
    fill = np.array([0xA5], np.uint8).repeat(a.dtype.itemsize).view(ub)[0]
    host = np.full(want.size + cases.CANARY, fill, ub)
    src = torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).to(dev)          # a copy: the shared input is read-only
    dst = torch.from_numpy(host.view(np.uint8)).to(dev)
    rc = lib.msr_overview_half(None, src.data_ptr(), shape[0], shape[1], ord(a.dtype.kind), a.dtype.itemsize, int(has_nodata), NV,
                               dst.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.raise_for(lib, None, rc, "msr_overview_half")
    got = dst.cpu().numpy().view(ub)
    assert np.array_equal(got[want.size:], host[want.size:]), "the canary behind dst was written"
    diff = np.flatnonzero(got[:want.size] != cases.bits(want).reshape(-1))
    assert not diff.size, (f"{diff.size} of {want.size} pixels differ from the twin, the first at "
                           f"{divmod(int(diff[0]), want.shape[1])}: {got[diff[0]]:#x} != {cases.bits(want).reshape(-1)[diff[0]]:#x}")
    assert np.array_equal(src.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1))      # src is not modified


# ---- 2. files ----------------------------------------------------------------------------------------------------------------
_HOST_FILES = {}


def _host_file(tmp_path_factory, shape, tile, dtype, file_dtype, predictor, n) -> bytes:
    key = (shape, tile, dtype, file_dtype, predictor, n)
    if key not in _HOST_FILES:
        p = str(tmp_path_factory.mktemp("host") / "a.tif")
        G.write_geotiff(p, cases.raster(shape, dtype), nodata=NV, dtype=file_dtype, predictor=predictor, tile=tile, overviews=n)
        _HOST_FILES[key] = open(p, "rb").read()
    return _HOST_FILES[key]


@pytest.mark.parametrize("dtype,predictor", cases.FORMATS)
@pytest.mark.parametrize("shape,tile", cases.LAYOUTS, ids=[f"{s[0]}x{s[1]}-{t[0]}x{t[1]}" for s, t in cases.LAYOUTS])
def test_device_files_equal_the_host_files(tmp_path, tmp_path_factory, dev, shape, tile, dtype, predictor):
    a = np.array(cases.raster(shape, dtype))                                    # a copy: the shared raster is read-only
    tensor = torch.from_numpy(a).to(dev)
    p = str(tmp_path / "d.tif")
    for n in sorted({0, min(2, cases.most_overviews(shape))}):
        want = _host_file(tmp_path_factory, shape, tile, dtype, dtype, predictor, n)
        for band_bytes in (1, 256 << 20):
            for data in (a, tensor):
                log = []
                G.write_geotiff(p, data, nodata=NV, dtype=dtype, predictor=predictor, tile=tile, overviews=n, encoder="device",
                                band_bytes=band_bytes, transfers=log)
                what = (n, band_bytes, type(data).__name__)
                assert open(p, "rb").read() == want, what
                tiles = sum(-(-r // tile[0]) * -(-c // tile[1]) for r, c in [shape] + G.overview_shapes(p))
                up = sum(b for d, b, _ in log if d == "h2d")
                down = sum(b for d, b, _ in log if d == "d2h")
                raw = a.nbytes if data is a else 0                              # a tensor is never downloaded or uploaded raw
                assert up == raw + 24 * tiles and down <= len(want) + 4 * tiles, what
                bands = sum(1 for _, _, w in log if w == "compressed output tiles")
                rows_of_tiles = sum(-(-r // tile[0]) for r, c in [shape] + G.overview_shapes(p))
                assert bands == (rows_of_tiles if band_bytes == 1 else n + 1), what


def test_uint8_tensor_into_a_uint16_file(tmp_path, tmp_path_factory, dev):
    """The ``good`` product: widened on the device, and the maximum commutes with the widening."""
    shape, tile = (70, 101), (16, 32)
    a = cases.raster(shape, "uint8")
    want = _host_file(tmp_path_factory, shape, tile, "uint8", "uint16", 2, 2)
    p = str(tmp_path / "d.tif")
    for band_bytes in (1, 256 << 20):
        G.write_geotiff(p, torch.from_numpy(np.array(a)).to(dev), nodata=NV, dtype=np.uint16, tile=tile, overviews=2,
                        encoder="device", band_bytes=band_bytes)
        assert open(p, "rb").read() == want
    levels = [G.read_geotiff(p, overview=k)[0] for k in range(3)]
    chain = cases.chain(shape, "uint8", 2)
    assert all(np.array_equal(g, c.astype(np.float32)) for g, c in zip(levels, chain))


def test_cropped_tensor_view_and_strips_unchanged(tmp_path, dev):
    """A non-contiguous view goes through the same band conversion; and without ``tile`` the device file is the strip file."""
    a = cases.raster((70, 101), "float32")
    t = torch.from_numpy(np.array(a)).to(dev)
    G.write_geotiff(str(tmp_path / "h.tif"), a[3:50, 5:90], nodata=NV, tile=(16, 16), overviews=2)
    G.write_geotiff(str(tmp_path / "d.tif"), t[3:50, 5:90], nodata=NV, tile=(16, 16), overviews=2, encoder="device", band_bytes=1)
    assert open(tmp_path / "d.tif", "rb").read() == open(tmp_path / "h.tif", "rb").read()
    G.write_geotiff(str(tmp_path / "hs.tif"), a, nodata=NV)
    G.write_geotiff(str(tmp_path / "ds.tif"), t, nodata=NV, encoder="device", tile=None, overviews=0)
    assert open(tmp_path / "ds.tif", "rb").read() == open(tmp_path / "hs.tif", "rb").read()


@pytest.mark.parametrize("case", pinned.LZW_CASES, ids=[c[0] for c in pinned.LZW_CASES])
def test_device_codecs_meet_the_pinned_digests(tmp_path, dev, case):
    """The cases of tests/test_geotiff_bytes_pinned.py (strips and tiles, BigTIFF, a big-endian meta, the nodata spellings)
    through the device encoder — band_bytes=1 and the default, from an array and from a CUDA tensor — and the device decoder:
    the digests pinned for the host codecs.  The decoder refuses 64-bit samples, and says so."""
    want = pinned.pinned()[case[0]]
    a = np.array(cases.raster(case[1], case[2]))                                # a copy: the shared raster is read-only
    p = str(tmp_path / "d.tif")
    for band_bytes in (1, 256 << 20):
        for data in (a, torch.from_numpy(a).to(dev)):
            pinned.write(p, case, data, encoder="device", band_bytes=band_bytes)
            assert pinned.sha(open(p, "rb").read()) == want["file"], (band_bytes, type(data).__name__)
    if np.dtype(case[4]["dtype"]).itemsize == 8:
        with pytest.raises(ValueError, match="does not read 64-bit samples"):
            G.read_geotiff(p, decoder="device")
    else:
        assert pinned.digests(p, case, decoder="device") == want
        assert pinned.digests(p, case, decoder="device", band_bytes=1) == want


# ---- 3. reading --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,predictor", cases.FORMATS)
def test_device_decoder_reads_the_levels(tmp_path, dev, dtype, predictor):
    p = str(tmp_path / "a.tif")
    shape = (70, 101)
    G.write_geotiff(p, np.array(cases.raster(shape, dtype)), nodata=NV, dtype=dtype, predictor=predictor, tile=(16, 32),
                    overviews=3, encoder="device")
    chain = cases.chain(shape, dtype, 3)
    for k in range(4):
        want, wmeta = G.read_geotiff(p, overview=k)
        assert np.array_equal(cases.bits(want), cases.bits(chain[k].astype(np.float32)))
        got, meta = G.read_geotiff(p, overview=k, decoder="device", band_bytes=1)
        assert np.array_equal(cases.bits(got), cases.bits(want)) and meta == wmeta and meta.get("overview") == (k or None)
        r0, r1 = want.shape[0] // 3, want.shape[0]
        part, meta = G.read_geotiff(p, overview=k, decoder="device", rows=(r0, r1), as_tensor=True)
        assert part.is_cuda and np.array_equal(cases.bits(part.cpu().numpy()), cases.bits(want[r0:r1]))
        assert meta["window"] == (r0, r1) and meta["shape"] == want.shape
    with pytest.raises(ValueError, match="overview 4 does not exist"):
        G.read_geotiff(p, overview=4, decoder="device")


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------
def test_driver_writes_tiled_products_with_overviews(tmp_path, hip_lib):
    from moonsuperresolution_amd import DEMSuperResolution, Generator
    shape = min(resident_cases.SHAPES.values(), key=lambda s: s[0] * s[1])
    assert shape == (272, 272)
    folder = str(tmp_path / "in")
    resident_cases.write_inputs(folder, shape)
    gen = Generator(resident_cases.S, resident_cases.B, weights=11, sampler="counter", seed=5)
    runs = {}
    try:
        for name, kw in (("strips", {}), ("tiled", dict(product_tile=(16, 16), overviews=2))):
            d = DEMSuperResolution(resident_cases.cfg(source_folder_path=folder, save_path=str(tmp_path / name), map_name="m"),
                                   model=gen, decoder="device", infill="device", encoder="device", resident=True, **kw)
            if kw:
                with pytest.raises(ValueError, match="rank0.*product_tile"):
                    d.processFiles(mode="tiles", products="rank0")
            d.processFiles(preprocess=True, swap_dsize=True)
            torch.cuda.synchronize()
            runs[name] = list(d.transfers)
            d.close()
    finally:
        gen.close()
    blocks_out = 0
    for product in ("mean", "std", "good"):
        strips = str(tmp_path / "strips" / f"m_{product}.tiff")
        tiled = str(tmp_path / "tiled" / f"m_{product}.tiff")
        want, wmeta = G.read_geotiff(strips)
        got, meta = G.read_geotiff(tiled)
        assert np.array_equal(cases.bits(got), cases.bits(want)), product            # level 0: the strip-layout run's raster
        assert meta["geo"] == wmeta["geo"] and meta["nodata"] == wmeta["nodata"] == NV and meta["dtype"] == wmeta["dtype"]
        assert G.overview_shapes(strips) == [] and G.overview_shapes(tiled) == [(136, 136), (68, 68)]
        level = want.astype(np.uint16) if product == "good" else want
        for k in (1, 2):
            level = G.overview_reference(level, None if product == "good" else NV)
            got, meta = G.read_geotiff(tiled, overview=k)
            assert np.array_equal(cases.bits(got), cases.bits(level.astype(np.float32))), (product, k)
            assert meta["geo"] == {} and meta["nodata"] == NV
        blocks_out += sum(-(-r // 16) * -(-c // 16) for r, c in [shape] + G.overview_shapes(tiled))
        if product != "good":
            assert (want == np.float32(NV)).any() and (want != np.float32(NV)).any()   # both kinds of pixel are in the product
    in_files = [os.path.join(folder, f) for f in ("run-DRG.tif", "run-DEM.tif")]
    in_bytes = sum(os.path.getsize(f) for f in in_files)
    out_bytes = sum(os.path.getsize(tmp_path / "tiled" / f"m_{product}.tiff") for product in ("mean", "std", "good"))
    blocks_in = 2 * -(-shape[0] // G._rows_per_strip(shape[0], shape[1] * 4))
    raster = shape[0] * shape[1] * 4
    sums = {"h2d": 0, "d2h": 0}
    for direction, nbytes, _ in runs["tiled"]:
        sums[direction] += nbytes
    print("tiled run:", sums, "inputs", in_bytes, "outputs", out_bytes, "blocks", blocks_in, blocks_out, "raster", raster)
    assert 0 < sums["h2d"] <= in_bytes + 64 * (blocks_in + blocks_out)
    assert 0 < sums["d2h"] <= out_bytes + 64 * (blocks_in + blocks_out)
    assert not any("product" in what and "raw" in what for _, _, what in runs["tiled"])
    assert sum(n for d, n, what in runs["tiled"] if d == "d2h" and "compressed" not in what) < raster   # no raster came down

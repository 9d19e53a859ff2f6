"""GPU (-m gpu): cloud-optimised GeoTIFF products — the in-place block encoder and the files built with it.

  1. msr_lzw_encode_blocks (csrc/geotiff_codec.hip) equals the host encoder's stream of the padded, differenced block byte for
     byte: the grid of tests/geotiff_cog_cases.py, one launch per geometry with blocks of different pitch; the random 48 x 48
     float32 block and the constant blocks; 0 and 1 blocks; 1100 tiles of 16 x 16 uint8, more than the grid of workgroups; a slot
     one byte short gives -1 and its canary stays;
  2. the files of write_geotiff(layout="cog", encoder="device") equal the host-encoded files byte for byte, from a NumPy array,
     a CUDA tensor and a cropped view, with band_bytes=1 and the default; ``transfers`` holds one "tables" entry per launch:
     len(plan_bands(level 0)) + (1 if overviews else 0); the device decoder reads every level;
  3. the driver: product_layout="cog" with the identity model — the files pass the order check, every level equals that of the
     "plain" run, and the files are the same with resident True / False and either encoder;
  4. far offsets: blocks whose first valid byte, or a later row of theirs at a pitch of 2^20, lies past 2^31 and past 2^32.
All comparisons are exact."""
import gc

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from tests import far_offset_cases as fc
from tests import geotiff_cog_cases as cases
from tests import geotiff_tiled_cases as tiled
from tests import resident_cases

pytestmark = pytest.mark.gpu
NV = cases.NOVAL


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


# ---- 1. the block encoder ----------------------------------------------------------------------------------------------------
def _launch(dev, blocks):
    """The blocks (one geometry) in one launch, their sources back to back in one buffer: the streams."""
    b0 = blocks[0]
    assert all((b.bw, b.bh, b.sb) == (b0.bw, b0.bh, b0.sb) for b in blocks)
    starts = np.cumsum([0] + [b.src.size for b in blocks[:-1]])
    buf = torch.from_numpy(np.concatenate([b.src for b in blocks])).to(dev)
    return G.lzw_encode_blocks_device(buf, [s + b.off for s, b in zip(starts, blocks)], [b.pitch for b in blocks],
                                      [b.vw for b in blocks], [b.vr for b in blocks], b0.bw, b0.bh, b0.sb)


@pytest.mark.parametrize("sb", cases.SAMPLE_BYTES)
def test_blocks_kernel_equals_the_host_encoder(dev, sb):
    for _, bw, bh in (g for g in cases.geometries() if g[0] == sb):
        blocks = cases.grid(sb, bw, bh)
        assert len({b.pitch for b in blocks}) > 3                      # blocks of different pitch share the launch
        got = _launch(dev, blocks)
        for b, g in zip(blocks, got):
            assert g == cases.stream(b), b.name


def test_blocks_kernel_special_blocks(dev):
    for b in cases.special():
        assert _launch(dev, [b])[0] == cases.stream(b), b.name           # one block


def test_no_block_and_more_blocks_than_workgroups(dev):
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    assert G.lzw_encode_blocks_device(buf, [], [], [], [], 16, 16, 1) == []
    a = np.array(tiled.raster((16 * 20 - 3, 16 * 55 - 5), "uint8"))
    table = G._tile_table(a.shape[0], a.shape[1], 16, 16, 1)
    assert table[0].size == 1100
    got = G.lzw_encode_blocks_device(torch.from_numpy(a.reshape(-1)).to(dev), *table, 16, 16, 1)
    assert got == G._host_tiles(a, np.dtype("u1"), 16, 16, 5, 2)


def test_a_slot_too_small_gives_minus_one(dev):
    lib = _lib.load()
    blocks = [b for b in cases.special() if b.name.startswith("constant")]
    b0 = blocks[0]
    blocks = [b for b in blocks if (b.bw, b.bh) == (b0.bw, b0.bh)]
    assert len(blocks) == 4
    for sb in cases.SAMPLE_BYTES:
        b = next(x for x in blocks if x.sb == sb)
        want = cases.stream(b)
        slot = len(want) + cases.CANARY
        caps = [len(want), len(want) - 1, 0]
        n = len(caps)
        src = torch.from_numpy(np.array(b.src)).to(dev)
        dst = torch.full((n * slot,), 0xA5, dtype=torch.uint8, device=dev)
        t64 = torch.tensor([b.off] * n + [b.pitch] * n + [i * slot for i in range(n)], dtype=torch.int64, device=dev)
        t32 = torch.tensor([b.vw] * n + [b.vr] * n + caps, dtype=torch.int32, device=dev)
        dst_len = torch.full((n,), -7, dtype=torch.int32, device=dev)
        p64, p32 = t64.data_ptr(), t32.data_ptr()
        for count in (0, n):                                             # no block: MSR_OK, and nothing is written
            rc = lib.msr_lzw_encode_blocks(None, src.data_ptr(), p64, p64 + 8 * n, p32, p32 + 4 * n, count, b.bw, b.bh, sb,
                                           dst.data_ptr(), p64 + 16 * n, p32 + 8 * n, dst_len.data_ptr(), None)
            assert rc == _lib.MSR_OK, lib.msr_last_error(None)
            torch.cuda.synchronize()
            if count == 0:
                assert dst_len.cpu().tolist() == [-7] * n and bool((dst == 0xA5).all())
        assert dst_len.cpu().tolist() == [len(want), -1, -1]
        out = dst.cpu().numpy().reshape(n, slot)
        assert out[0, :len(want)].tobytes() == want
        for i, cap in enumerate(caps):
            assert (out[i, cap:] == 0xA5).all(), (sb, cap, "a byte at or beyond cap was written")


def test_wrapper_checks_the_valid_parts(dev):
    buf = torch.zeros(1000, dtype=torch.uint8, device=dev)
    for args, word in ((([0], [100], [17], [4]), "not inside its block"), (([0], [100], [16], [17]), "not inside its block"),
                       (([0], [100], [-1], [4]), "not inside its block"), (([0, 0], [100], [16], [4]), "differ in length"),
                       (([-1], [100], [16], [4]), "outside the buffer"), (([0], [100], [16], [11]), "outside the buffer"),
                       (([985], [0], [16], [16]), "outside the buffer")):
        with pytest.raises(ValueError, match=word):
            G.lzw_encode_blocks_device(buf, *args, 16, 16, 1)
    assert len(G.lzw_encode_blocks_device(buf, [984], [0], [16], [16], 16, 16, 1)) == 1      # the last byte of the buffer is read
    assert len(G.lzw_encode_blocks_device(buf, [0], [100], [16], [10], 16, 16, 1)) == 1


# ---- 2. files ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.FILE_DTYPES)
@pytest.mark.parametrize("shape,tile,n,big", cases.FILES, ids=[f"{s[0]}x{s[1]}-o{n}{'-big' if big else ''}" for s, _, n, big in cases.FILES])
def test_device_files_equal_the_host_files(tmp_path, dev, shape, tile, n, big, dtype):
    a = np.array(tiled.raster(shape, dtype))                                    # a copy: the shared raster is read-only
    how = dict(meta=cases.META, nodata=NV, dtype=dtype, bigtiff=big, tile=tile, overviews=n, layout="cog")
    h, d, plain = str(tmp_path / "h.tif"), str(tmp_path / "d.tif"), str(tmp_path / "p.tif")
    G.write_geotiff(h, a, **how)
    want = open(h, "rb").read()
    cases.check_cog_order(h, n)
    sb = a.dtype.itemsize
    for band_bytes in (1, 256 << 20):
        launches = len(G.plan_bands(shape[0], -(-shape[1] // tile[1]) * tile[1] * sb, tile[0], band_bytes)) + (1 if n else 0)
        assert launches == (-(-shape[0] // tile[0]) if band_bytes == 1 else 1) + (1 if n else 0)
        for data in (a, torch.from_numpy(a).to(dev)):
            log = []
            G.write_geotiff(d, data, encoder="device", band_bytes=band_bytes, transfers=log, **how)
            what = (band_bytes, type(data).__name__)
            assert open(d, "rb").read() == want, what
            assert sum(1 for _, _, w in log if "tables" in w) == launches, what
            tiles = sum(-(-r // tile[0]) * -(-c // tile[1]) for r, c in [shape] + G.overview_shapes(d))
            up = sum(b for dr, b, _ in log if dr == "h2d")
            down = sum(b for dr, b, _ in log if dr == "d2h")
            assert up == (a.nbytes if data is a else 0) + 36 * tiles and down <= len(want) + 4 * tiles, what
    G.write_geotiff(plain, a, **dict(how, layout="plain"))
    cases.same_levels(d, plain, n, decoder="device", band_bytes=1)


def test_cropped_tensor_view_and_a_uint8_tensor_into_a_uint16_file(tmp_path, dev):
    a = tiled.raster((70, 101), "float32")
    t = torch.from_numpy(np.array(a)).to(dev)
    h, d = str(tmp_path / "h.tif"), str(tmp_path / "d.tif")
    how = dict(nodata=NV, tile=(16, 16), overviews=2, layout="cog")
    G.write_geotiff(h, a[3:50, 5:90], **how)
    view = t[3:50, 5:90]
    assert not view.is_contiguous()
    for band_bytes in (1, 256 << 20):
        G.write_geotiff(d, view, encoder="device", band_bytes=band_bytes, **how)
        assert open(d, "rb").read() == open(h, "rb").read()
    good = tiled.raster((70, 101), "uint8")                                     # the ``good`` product: widened on the device
    G.write_geotiff(h, good, dtype=np.uint16, **how)
    for band_bytes in (1, 256 << 20):
        G.write_geotiff(d, torch.from_numpy(np.array(good)).to(dev), dtype=np.uint16, encoder="device", band_bytes=band_bytes, **how)
        assert open(d, "rb").read() == open(h, "rb").read()


# ---- 3. the driver -----------------------------------------------------------------------------------------------------------
def test_driver_writes_cog_products(tmp_path, hip_lib):
    from moonsuperresolution_amd import DEMSuperResolution
    shape = resident_cases.SHAPES["square"]
    assert shape == (272, 272) and (resident_cases.S, resident_cases.STRIDE, resident_cases.T) == (64, 16, 128)
    folder = str(tmp_path / "in")
    resident_cases.write_inputs(folder, shape)
    runs = [("plain", False, "host", "plain")] + [(f"cog-{int(r)}-{e}", r, e, "cog") for r in (False, True) for e in ("host", "device")]
    files = {}
    for name, resident, encoder, layout in runs:
        d = DEMSuperResolution(resident_cases.cfg(source_folder_path=folder, save_path=str(tmp_path / name), map_name="m"),
                               model=resident_cases.f32_identity, encoder=encoder, resident=resident, product_tile=(16, 16),
                               overviews=2, product_layout=layout)
        if layout == "cog":
            with pytest.raises(ValueError, match="rank0.*product_tile"):
                d.processFiles(mode="tiles", products="rank0")
        d.processFiles(preprocess=False)
        torch.cuda.synchronize()
        d.close()
        files[name] = resident_cases.product_bytes(str(tmp_path / name))
    for product in ("mean", "std", "good"):
        cog = str(tmp_path / "cog-1-device" / f"m_{product}.tiff")
        cases.check_cog_order(cog, 2)
        cases.same_levels(cog, str(tmp_path / "plain" / f"m_{product}.tiff"), 2)
        want, meta = G.read_geotiff(cog)
        assert meta["nodata"] == NV and want.shape == shape and (product == "good" or len(np.unique(want)) > 1)
        for name, _, _, layout in runs[2:]:
            assert files[name][product] == files["cog-0-host"][product], (name, product)
        assert files["plain"][product] != files["cog-0-host"][product]


# ---- 4. far offsets ----------------------------------------------------------------------------------------------------------
def test_blocks_past_the_2_gib_and_4_gib_lines(dev):
    """Blocks of a uint8 buffer a little over 4 GiB, read at a pitch of 2^20: the first valid byte past each line, and the
    first valid byte below a line with later rows past it.  The reference is the host encoder on the same bytes, taken from
    the windows that were uploaded; the rest of the buffer is never initialised and never read."""
    L31, L32 = fc.L31, fc.L32
    pitch, bw, bh, vw, vr = 1 << 20, 256, 16, 200, 13
    size = L32 + 32 * pitch
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    src = torch.empty(size, dtype=torch.uint8, device=dev)
    offs = [L31 + 12345, L32 + 777, L31 - 3 * pitch - 5, L32 - 3 * pitch - 9, L32 - 2 * pitch + 4100]
    spans = sorted(o + y * pitch for o in offs for y in range(vr))                          # the blocks share no byte
    assert all(b - a >= vw for a, b in zip(spans, spans[1:]))
    assert L31 <= offs[0] < L32 and offs[1] >= L32                                          # the first valid byte past a line
    assert offs[2] < L31 < offs[2] + 4 * pitch and offs[2] + (vr - 1) * pitch + vw < L32     # a later row past 2^31
    assert all(o < L32 < o + 4 * pitch for o in offs[3:])                                   # a later row past 2^32
    assert max(offs) + (vr - 1) * pitch + vw <= size and any(o % 2 for o in offs)
    rng = np.random.default_rng(31)
    try:
        for sb in (4, 1, 0):
            windows = []
            for o in offs:
                ut = np.dtype(f"<u{sb or 1}")
                rows = (np.cumsum(rng.integers(-3, 4, (vr, vw // ut.itemsize)), axis=1) + 500).astype(ut).view(np.uint8).reshape(vr, vw)
                for y in range(vr):
                    src[o + y * pitch:o + y * pitch + vw] = torch.from_numpy(rows[y].copy()).to(dev)
                windows.append(cases.Block(f"far-{sb}-{o}", rows.reshape(-1), 0, vw, vw, vr, bw, bh, sb))
            n = len(offs)
            got = G.lzw_encode_blocks_device(src, offs, [pitch] * n, [vw] * n, [vr] * n, bw, bh, sb)
            for b, g in zip(windows, got):
                assert g == cases.stream(b), b.name
        peak = torch.cuda.max_memory_allocated()
    finally:
        del src
        gc.collect()
        torch.cuda.empty_cache()
    assert peak <= fc.BUDGET, f"{peak / fc.GIB:.2f} GiB of device memory at the peak"

"""GPU (-m gpu): the floating-point predictor (PREDICTOR=3) of the device GeoTIFF encoder.

  1. msr_tiff_encode_strips, predictor 3 (csrc/geotiff_codec.hip, csrc/lzw_strip.h lzw_fetch_fp) against msr_lzw_encode of the
     twin's bytes (geotiff.fp_predictor_reference): three rows of 33, 64, 65, 257 and 16400 samples, 17 rows of 33 in strips of
     5, each from a source on a 4-byte boundary and one byte off it; canaries behind every dst_cap; a slot one byte short gives
     -1 and writes nothing past its cap;
  2. msr_tiff_encode_blocks, predictor 3, on blocks read in place from a 40 x 70 raster whose pitch is larger than its row, and
     one launch that mixes the tiles of two levels at different pitches: every stream is the one-lane host entry's;
  3. a launch whose blocks' rows cross 2^32 bytes;
  4. the old entries and the new ones with predictor 1 / 2 on the cases of tests/geotiff_cog_cases.py;
  5. files: write_geotiff(predictor=3, encoder="device") writes the host writer's file, from a NumPy array and a CUDA tensor;
  6. the driver: product_predictor=3 with the identity model.
All comparisons are exact."""
import gc

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from tests import far_offset_cases as fc
from tests import geotiff_cog_cases as cog_cases
from tests import geotiff_pred3_cases as cases
from tests import resident_cases

pytestmark = pytest.mark.gpu
NV = cases.NOVAL
CANARY = cases.CANARY


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


# ---- 1. the strip encoder ----------------------------------------------------------------------------------------------------
def _strips_launch(lib, dev, src, src_off, src_len, row_bytes, caps):
    """msr_tiff_encode_strips, predictor 3, with hand-built tables: slot i is caps[i] bytes with a canary behind it.  Returns
    (lengths, [slot i with its canary])."""
    n = len(src_off)
    slots = [c + CANARY for c in caps]
    dst_off = np.concatenate(([0], np.cumsum(slots)[:-1])).astype(np.int64)
    dst = torch.full((int(sum(slots)),), 0xA5, dtype=torch.uint8, device=dev)
    t64 = torch.from_numpy(np.concatenate([np.asarray(src_off, np.int64), dst_off])).to(dev)
    t32 = torch.from_numpy(np.concatenate([np.asarray(src_len, np.int32), np.asarray(caps, np.int32)])).to(dev)
    dst_len = torch.full((n,), -7, dtype=torch.int32, device=dev)
    rc = lib.msr_tiff_encode_strips(None, src.data_ptr(), t64.data_ptr(), t32.data_ptr(), n, 4, 3, row_bytes, dst.data_ptr(),
                                    t64.data_ptr() + 8 * n, t32.data_ptr() + 4 * n, dst_len.data_ptr(), None)
    assert rc == _lib.MSR_OK, lib.msr_last_error(None)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    return dst_len.cpu().tolist(), [out[o:o + s] for o, s in zip(dst_off.tolist(), slots)]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "odd"])
@pytest.mark.parametrize("rows,w,rps", cases.STRIPS, ids=[f"{r}x{w}-rps{p}" for r, w, p in cases.STRIPS])
def test_strips_kernel_equals_the_twin(dev, rows, w, rps, shift):
    lib = _lib.load()
    a = cases.strip_source(rows, w)
    want = cases.strip_streams(rows, w, rps)
    raw = np.zeros(a.nbytes + 4, np.uint8)
    raw[shift:shift + a.nbytes] = a.view(np.uint8).reshape(-1)
    src = torch.from_numpy(raw).to(dev)
    assert src.data_ptr() % 4 == 0
    starts = np.arange(0, rows, rps)
    src_off = shift + starts * w * 4
    src_len = (np.minimum(starts + rps, rows) - starts) * w * 4
    assert len(want) == len(starts) and (rps == rows or len(starts) > 1)
    lens, slots = _strips_launch(lib, dev, src, src_off, src_len, w * 4, [len(s) for s in want])
    assert lens == [len(s) for s in want]
    for i, (s, slot) in enumerate(zip(want, slots)):
        assert slot[:len(s)].tobytes() == s, i
        assert (slot[len(s):] == 0xA5).all(), (i, "a byte at or beyond cap was written")
    lens, slots = _strips_launch(lib, dev, src, src_off, src_len, w * 4, [len(s) - 1 for s in want])     # one byte short
    assert lens == [-1] * len(want)
    for i, (s, slot) in enumerate(zip(want, slots)):
        assert (slot[len(s) - 1:] == 0xA5).all(), (i, "a byte at or beyond cap was written")
    # the wrapper of the Python layer: the same streams
    assert G.lzw_encode_device(src, src_off, src_len, 4, w * 4, predictor=3) == list(want)


# ---- 2. the in-place block encoder -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bh,bw", cases.BLOCK_SIZES)
def test_blocks_kernel_equals_the_one_lane_host_entry(dev, bh, bw):
    lib = _lib.load()
    src = np.array(cases.block_raster())
    blocks = cases.blocks(bh, bw)
    offs = [b.y0 * cases.BLOCK_PITCH + b.x0 * 4 for b in blocks]
    want = [cases.host_entry(lib, src, o, cases.BLOCK_PITCH, b) for o, b in zip(offs, blocks)]
    assert want == [cases.stream(b) for b in blocks]
    for shift in (0, 3):                         # rows on a 4-byte boundary, and off it
        raw = np.zeros(src.nbytes + 4, np.uint8)
        raw[shift:shift + src.nbytes] = src.view(np.uint8).reshape(-1)
        buf = torch.from_numpy(raw).to(dev)
        got = G.lzw_encode_blocks_device(buf, [o + shift for o in offs], [cases.BLOCK_PITCH] * len(blocks), [b.vw * 4 for b in blocks],
                                         [b.vr for b in blocks], bw * 4, bh, 4, predictor=3)
        assert got == want, shift


def test_blocks_of_two_levels_share_a_launch(dev):
    """The tiles of a 40 x 70 level and of its 20 x 35 reduction, each row-major at its own pitch in one allocation."""
    lib = _lib.load()
    l0, l1 = cases.levels((40, 70), 1)
    base1 = (l0.nbytes + 15) // 16 * 16
    raw = np.zeros(base1 + l1.nbytes, np.uint8)
    raw[:l0.nbytes] = l0.view(np.uint8).reshape(-1)
    raw[base1:] = l1.view(np.uint8).reshape(-1)
    th, tw = 16, 32
    tables = [G._tile_table(40, 70, th, tw, 4), G._tile_table(20, 35, th, tw, 4, base1)]
    off, pitch, wb, vr = (np.concatenate(col) for col in zip(*tables))
    assert sorted(set(pitch.tolist())) == [140, 280] and off.size == 9 + 4
    got = G.lzw_encode_blocks_device(torch.from_numpy(raw).to(dev), off, pitch, wb, vr, tw * 4, th, 4, predictor=3)
    for i in range(off.size):
        b = cases.Block(f"tile{i}", 0, 0, int(vr[i]), int(wb[i]) // 4, th, tw)
        assert got[i] == cases.host_entry(lib, raw, int(off[i]), int(pitch[i]), b), i
    dt = np.dtype("<f4")
    assert got == G._host_tiles(np.array(l0), dt, th, tw, 5, 3) + G._host_tiles(np.array(l1), dt, th, tw, 5, 3)


# ---- 3. 64-bit addressing ----------------------------------------------------------------------------------------------------
def test_block_rows_across_4_gib(dev):
    """Blocks of a uint8 buffer a little over 4 GiB read at a pitch of 2^20: blk_off + y * pitch crosses 2^32 inside the block
    (on a 4-byte boundary, and at an odd offset), and a block that begins past it.  The reference is the one-lane host entry on
    the windows that were uploaded; the rest of the buffer is never initialised and never read."""
    lib = _lib.load()
    L32 = fc.L32
    pitch, bh, bw, vr, vw = 1 << 20, 32, 48, 13, 40
    size = L32 + 32 * pitch
    offs = [L32 - 3 * pitch - 8, L32 - 2 * pitch + 4099, L32 + 772]
    assert all(o < L32 < o + (vr - 1) * pitch for o in offs[:2]) and offs[2] >= L32 and offs[0] % 4 == 0 and offs[1] % 2
    assert max(offs) + (vr - 1) * pitch + vw * 4 <= size
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    src = torch.empty(size, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(32)
    try:
        want = []
        for o in offs:
            rows = (np.cumsum(rng.integers(-3, 4, (vr, vw)), axis=1) * 0.25 - 2000.0).astype(np.float32)
            for y in range(vr):
                src[o + y * pitch:o + y * pitch + vw * 4] = torch.from_numpy(rows[y].view(np.uint8).copy()).to(dev)
            want.append(cases.host_entry(lib, rows, 0, vw * 4, cases.Block(f"far-{o}", 0, 0, vr, vw, bh, bw)))
        n = len(offs)
        got = G.lzw_encode_blocks_device(src, offs, [pitch] * n, [vw * 4] * n, [vr] * n, bw * 4, bh, 4, predictor=3)
        assert got == want
        peak = torch.cuda.max_memory_allocated()
    finally:
        del src
        gc.collect()
        torch.cuda.empty_cache()
    assert peak <= fc.BUDGET, f"{peak / fc.GIB:.2f} GiB of device memory at the peak"


# ---- 4. the old entries and the new ones -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sb", cog_cases.SAMPLE_BYTES)
def test_old_and_new_device_entries_agree(dev, sb):
    """Blocks: every geometry of the grid in one launch per entry.  Strips: the blocks whose valid part lies contiguous (a
    pitch equal to its width) as strips of vr rows.  sample_bytes 0 of the old entries is predictor 1 of the new ones."""
    width, predictor = (sb, 2) if sb else (1, 1)
    for _, bw, bh in (g for g in cog_cases.geometries() if g[0] == sb):
        blocks = cog_cases.grid(sb, bw, bh)
        starts = np.cumsum([0] + [b.src.size for b in blocks[:-1]])
        buf = torch.from_numpy(np.concatenate([b.src for b in blocks])).to(dev)
        args = (buf, [s + b.off for s, b in zip(starts, blocks)], [b.pitch for b in blocks], [b.vw for b in blocks],
                [b.vr for b in blocks], bw, bh)
        old = G.lzw_encode_blocks_device(*args, sb)
        assert old == G.lzw_encode_blocks_device(*args, width, predictor=predictor) == [cog_cases.stream(b) for b in blocks], (bw, bh)
        tight = [(s + b.off, b) for s, b in zip(starts, blocks) if b.pitch == b.vw]
        for vw in sorted({b.vw for _, b in tight}):                    # one row length per launch
            some = [(o, b) for o, b in tight if b.vw == vw]
            offs, lens = [o for o, _ in some], [b.vw * b.vr for _, b in some]
            old = G.lzw_encode_device(buf, offs, lens, sb, vw)
            assert old == G.lzw_encode_device(buf, offs, lens, width, vw, predictor=predictor), (bw, bh, vw)
            assert old == [G.lzw_encode(fc.predict(b.src[b.off:b.off + b.vw * b.vr], sb, vw)) for _, b in some]
    for b in (x for x in cog_cases.special() if x.sb == sb):
        args = (torch.from_numpy(np.array(b.src)).to(dev), [b.off], [b.pitch], [b.vw], [b.vr], b.bw, b.bh)
        assert G.lzw_encode_blocks_device(*args, sb) == G.lzw_encode_blocks_device(*args, width, predictor=predictor) \
            == [cog_cases.stream(b)], b.name


# ---- 5. files ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,how", cases.LAYOUTS, ids=[x[0] for x in cases.LAYOUTS])
def test_device_files_equal_the_host_files(tmp_path, tmp_path_factory, dev, name, shape, how):
    want = cases.host_file(tmp_path_factory, name)
    a = np.array(cases.raster(shape))
    d = str(tmp_path / "d.tif")
    for band_bytes in (1, 256 << 20):
        for data in (a, torch.from_numpy(a).to(dev)):
            G.write_geotiff(d, data, nodata=NV, predictor=3, encoder="device", band_bytes=band_bytes, **how)
            assert open(d, "rb").read() == want, (band_bytes, type(data).__name__)
    view = torch.from_numpy(np.pad(a, 3)).to(dev)[3:-3, 3:-3]            # a cropped view: not contiguous
    assert not view.is_contiguous()
    G.write_geotiff(d, view, nodata=NV, predictor=3, encoder="device", **how)
    assert open(d, "rb").read() == want
    with pytest.raises(ValueError, match="predictor 3"):                 # the device reader goes on refusing these files
        G.read_geotiff(d, decoder="device")


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------
def _predictor_tag(path) -> int:
    buf, t, bo, _ = G._open(path)
    return G._values(t[317], bo)[0]


def test_driver_product_predictor(tmp_path, hip_lib):
    from moonsuperresolution_amd import DEMSuperResolution, HaloShardedSuperResolution
    shape = min(resident_cases.SHAPES.values(), key=lambda s: s[0] * s[1])
    assert shape == (272, 272)
    folder = str(tmp_path / "in")
    resident_cases.write_inputs(folder, shape)

    def cfg(name):
        return resident_cases.cfg(source_folder_path=folder, save_path=str(tmp_path / name), map_name="m")

    with pytest.raises(ValueError, match="product_predictor"):
        DEMSuperResolution(cfg("bad"), model=resident_cases.f32_identity, product_predictor=4)
    runs = [("default", False, "host", {})] + [(f"p3-{int(r)}-{e}", r, e, {"product_predictor": 3})
                                               for r in (False, True) for e in ("host", "device")]
    files = {}
    for name, resident, encoder, kw in runs:
        d = DEMSuperResolution(cfg(name), model=resident_cases.f32_identity, encoder=encoder, resident=resident, **kw)
        d.processFiles(preprocess=False)
        torch.cuda.synchronize()
        d.close()
        files[name] = resident_cases.product_bytes(str(tmp_path / name))
    for product, tag in (("mean", 3), ("std", 3), ("good", 2)):
        path = str(tmp_path / "p3-1-device" / f"m_{product}.tiff")
        assert _predictor_tag(path) == tag and _predictor_tag(str(tmp_path / "default" / f"m_{product}.tiff")) == 2
        got, meta = G.read_geotiff(path)
        want, wmeta = G.read_geotiff(str(tmp_path / "default" / f"m_{product}.tiff"))
        assert meta == wmeta and got.shape == shape and np.array_equal(cases.bits(got), cases.bits(want)), product
        assert product == "good" or len(np.unique(want)) > 1
        for name, _, _, _ in runs[2:]:
            assert files[name][product] == files["p3-0-host"][product], (name, product)
        assert (files["default"][product] == files["p3-0-host"][product]) == (product == "good")
    # the rank-local writer (one rank of the halo mode takes it): encode_strips + write_strips with the same predictor
    for name, kw in (("halo-p2", {}), ("halo-p3", {"product_predictor": 3})):
        d = HaloShardedSuperResolution(cfg(name), model=resident_cases.f32_identity, encoder="device", **kw)
        d.processFiles(preprocess=False, mode="halo", rank=0, world=1, products="rank0")
        torch.cuda.synchronize()
        assert d.products_path == "rank0"
        d.close()
    for product, tag in (("mean", 3), ("std", 3), ("good", 2)):
        p3, p2 = (str(tmp_path / n / f"m_{product}.tiff") for n in ("halo-p3", "halo-p2"))
        assert _predictor_tag(p3) == tag and _predictor_tag(p2) == 2
        assert np.array_equal(cases.bits(G.read_geotiff(p3)[0]), cases.bits(G.read_geotiff(p2)[0])), product

"""CPU: what tests/test_gpu_far_offsets.py relies on, checked without a GPU.

  * the row-restricted references of tests/far_offset_cases.py equal the rows of the whole-raster oracles
    (oracle/preprocess_ref.py, infill.infill_reference, geotiff.overview_reference, tiler_ref.halo_partials) at the small shapes
    the suite already uses, bit for bit;
  * the line arithmetic of the case table: every far raster is the smallest whose last rows lie past its line, and stays
    inside what the 32-bit entry checks accept;
  * the device memory of every case, computed from its shapes, stays at or under 20 GiB;
  * the refusals that need no device: one row more than the largest accepted grid.
"""
import ctypes as C

import numpy as np
import pytest

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from moonsuperresolution_amd import infill as I
from oracle import preprocess_ref as pr
from oracle import tiler_ref
from tests import far_offset_cases as fc

NOVAL = fc.NOVAL


def _raster(shape, seed, nodata=True):
    rng = np.random.default_rng(seed)
    a = (rng.normal(size=shape) * 1000).astype(np.float32)
    a[rng.uniform(size=shape) < 0.01] = np.nan
    if nodata:
        a[rng.uniform(size=shape) < 0.02] = NOVAL
        a[rng.uniform(size=shape) < 0.005] = NOVAL - 5.0
    a[1, 1] = a[shape[0] - 1, shape[1] - 1] = np.nan       # a full block and the last block, whatever the draw gave
    return a


def _whole_area(src, flags):
    a = src.copy()
    if flags & fc.NODATA_TO_NAN:
        a[a <= np.float32(NOVAL)] = np.nan
    out = pr.resize_area(a, 0.25, 0.25)
    if flags & fc.NAN_TO_NODATA:
        out[np.isnan(out)] = NOVAL
    return out


# (1030, 517): rows % 8 == 6, a partial bottom block that cvRound keeps; (1032, 516): whole blocks; (50, 75): rows % 4 == 2 whose
# half rounds DOWN (no partial row) and a partial right column; (10, 11), (14, 9): tiny, with and without the partial row
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(1030, 517), (1032, 516), (50, 75), (10, 11), (14, 9)])
def test_area_rows_ref_equals_the_rows_of_the_whole_oracle(shape, flags):
    h, w = shape
    src = _raster(shape, h + flags)
    want = _whole_area(src, flags)
    dh = want.shape[0]
    assert dh == pr.cv_round(h / 4)
    if shape in ((1030, 517), (14, 9)):
        assert h % 4 == 2 and dh == h // 4 + 1            # the last row's block holds two source rows
    for d0, d1 in {(0, dh), (dh // 3, dh), (dh - 1, dh), (dh // 3, 2 * dh // 3 + 1), (0, 1)}:
        s0, s1 = 4 * d0, min(4 * d1, h)
        got = fc.area_rows_ref(src[s0:s1], s0, h, 4, d0, d1, NOVAL, flags)
        assert fc.bits_equal(got, want[d0:d1]), (shape, flags, d0, d1)
    assert np.isnan(want).any() or flags & fc.NAN_TO_NODATA


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("shape,dsize", [((200, 26), (406, 3210)), ((33, 65), (1000, 517)), ((16, 12), (192, 256)),
                                         ((40, 40), (13, 17)), ((7, 9), (9, 7)), ((517, 130), (9, 33))])
def test_cubic_rows_ref_equals_the_rows_of_the_whole_oracle(shape, dsize, flags):
    h, w = shape
    dw, dh = dsize
    src = _raster(shape, dw, nodata=bool(flags))
    a = src.copy()
    if flags & fc.NODATA_TO_NAN:
        a[a <= np.float32(NOVAL)] = np.nan
    want = pr.resize_cubic(a, dsize)
    if flags & fc.NAN_TO_NODATA:
        want[np.isnan(want)] = NOVAL
    for r0, r1 in {(0, dh), (dh // 3, 2 * dh // 3 + 1), (dh - min(dh, 32), dh), (dh // 2, dh // 2 + 1)}:
        s0, s1 = fc.cubic_tap_rows(r0, r1, h, dh)
        assert 0 <= s0 < s1 <= h
        got = fc.cubic_rows_ref(src[s0:s1], s0, h, dh, dw, r0, r1, NOVAL, flags)
        assert fc.bits_equal(got, want[r0:r1]), (shape, dsize, flags, r0, r1)
        wide = fc.cubic_rows_ref(src[max(0, s0 - 2):], max(0, s0 - 2), h, dh, dw, r0, r1, NOVAL, flags)   # a wider window
        assert fc.bits_equal(wide, want[r0:r1])
    with pytest.raises(AssertionError, match="lacks a tapped row"):
        s0, s1 = fc.cubic_tap_rows(0, dh, h, dh)
        fc.cubic_rows_ref(src[s0:s1 - 1], s0, h, dh, dw, 0, dh)


@pytest.mark.parametrize("dtype,nodata", [(np.float32, None), (np.float32, NOVAL), (np.uint16, None), (np.uint8, None)])
@pytest.mark.parametrize("shape", [(1031, 517), (130, 300)])
def test_overview_of_a_tail_from_an_even_row_is_the_tail_of_the_overview(shape, dtype, nodata):
    rng = np.random.default_rng(shape[0])
    if dtype == np.float32:
        a = _raster(shape, 5)
        a[-4:-2, 10:14] = NOVAL                           # whole blocks of no-data
    else:
        a = rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    want = G.overview_reference(a, nodata)
    for t0 in (0, shape[0] - 128 - shape[0] % 2, shape[0] - 2 - shape[0] % 2):
        assert t0 % 2 == 0
        got = fc.overview_tail_ref(a[t0:], nodata)
        if dtype == np.float32:
            assert fc.bits_equal(got, want[t0 // 2:]), (shape, t0)
        else:
            assert np.array_equal(got, want[t0 // 2:]), (shape, t0)


def test_infill_windows_equal_the_rows_of_the_whole_grid():
    """The twin on the head and tail windows (with their row0 / full_rows) writes what the twin on the whole grid does."""
    rows, cols, H = 400, 3400, fc.INFILL_WINDOW
    head, h0, hp = fc.infill_window("head", rows, cols, seed=1)
    tail, t0, tp = fc.infill_window("tail", rows, cols, seed=2)
    assert h0 == 0 and t0 == rows - H
    grid = np.full((rows, cols), -1900.0, np.float32)
    grid[:H], grid[t0:] = head, tail
    want = I.infill_reference(grid, NOVAL, fc.INFILL_MAX_AREA, fc.INFILL_MARGIN)
    got_head = fc.infill_window_ref(head, 0, rows)
    got_tail = fc.infill_window_ref(tail, t0, rows)
    assert np.array_equal(got_head.view(np.uint32), want[:H].view(np.uint32))
    assert np.array_equal(got_tail.view(np.uint32), want[t0:].view(np.uint32))
    assert np.array_equal(want[H:t0], grid[H:t0])
    for got, planted, edge in ((got_head, hp, fc.INFILL_MARGIN), (got_tail, tp, H - fc.INFILL_MARGIN - 1)):
        left = {name: [got[r, c] == np.float32(NOVAL) for r, c in pix] for name, pix in planted.items()}
        for n in range(1, 32):                            # fewer than max_area pixels: filled; the others stay
            assert all(left[f"size{n}"]) == (n >= fc.INFILL_MAX_AREA) and any(left[f"size{n}"]) == (n >= fc.INFILL_MAX_AREA), n
        assert not any(v for n in range(1, 13) for v in left[f"edge{n}"])
        assert any(left["crossing"]) and not all(left["crossing"])
        assert left["right-crossing"] == [False, False, False, True]
        assert not any(left["apart-a"] + left["apart-b"] + left["right"])
        rows_of = sorted({r for pix in planted.values() for r, _ in pix})
        assert edge in rows_of                            # a component reaches the first / last fillable row


def test_band_reference_is_the_oracle_accumulation_and_position_independent():
    S, stride = 64, 16
    pred, key, dmm, acc = fc.band_reference(S, stride, 3, 2, seed=1)
    assert pred.shape == (6, S, S) and pred.dtype == np.float32 and key.tolist()[:4] == [[0, 0], [16, 0], [32, 0], [0, 16]]
    assert acc[0].shape == (80, 96) and (acc[0] > 0).any()
    # the same band somewhere else on a larger canvas, through the oracle's own update lines (rebuild-free): shifted origins
    # give the shifted accumulators
    rng = np.random.default_rng(1)
    img = rng.uniform(0.1, 0.9, (80, 96)).astype(np.float32)
    dem = (-2000.0 + 300.0 * rng.standard_normal((80, 96))).astype(np.float32)
    big_i = np.full((200, 300), 0.5, np.float32)
    big_d = np.full((200, 300), -1000.0, np.float32)
    big_i[48:128, 160:256], big_d[48:128, 160:256] = img, dem
    moved = tiler_ref.halo_partials(big_i, big_d, [48, 64], [160, 176, 192], fc.f32_identity, S, stride, 4, NOVAL)
    for a, b in zip(acc, moved):
        assert np.array_equal(a.view(np.uint32), b[48:128, 160:256].view(np.uint32))
        assert not b[:48].any() and not b[128:].any() and not b[:, :160].any() and not b[:, 256:].any()
    for i, (x, y) in enumerate(key):                      # pred is the identity model's output for the patch
        patch, mm = tiler_ref.normalize(img[y:y + S, x:x + S], dem[y:y + S, x:x + S])
        assert np.array_equal(pred[i], patch[..., 1]) and tuple(dmm[i]) == mm


def test_block_and_predictor_helpers():
    rng = np.random.default_rng(0)
    for kind, sb in fc.BLOCK_KINDS:
        for predictor in (1, 2):
            raw, val = fc.tiff_block(kind, sb, 37, 3, predictor, rng)
            assert raw.dtype == np.uint8 and raw.size == 37 * 3 * sb and val.shape == (3, 37) and val.dtype == np.float32
            u = raw.view(np.dtype(f"<u{sb}")).reshape(3, 37)
            if predictor == 2:
                u = np.cumsum(u, axis=1, dtype=u.dtype)
            back = u.view(np.dtype(f"<{kind}{sb}"))
            assert fc.bits_equal(back if kind == "f" else back.astype(np.float32), val)
    data = rng.integers(0, 256, 5 * 1200, dtype=np.uint8)
    assert fc.predict(data, 0, 0) is not None and np.array_equal(fc.predict(data, 0, 0), data)
    for sb in (2, 4):
        d = fc.predict(data, sb, 1200).view(np.dtype(f"<u{sb}")).reshape(5, -1)
        assert np.array_equal(np.cumsum(d, axis=1, dtype=d.dtype).view(np.uint8).reshape(-1), data)
    stream = G.lzw_encode(fc.predict(data, 4, 1200))
    assert bytes(G.lzw_decode(stream, data.size)) == fc.predict(data, 4, 1200).tobytes()


# ---- the case table ------------------------------------------------------------------------------------------------------------
def test_line_arithmetic_of_the_far_rasters():
    for line in fc.LINES.values():
        for cols in fc.COLS:
            for size in (1, 2, 4):
                rows = fc.far_rows(line, cols, size)
                assert fc.offset(rows - fc.TAIL, cols, size) >= line > fc.offset(rows - fc.TAIL - 1, cols, size)   # the smallest
                assert fc.rows_past(line, rows - fc.TAIL, cols, size) and not fc.rows_past(line, rows - fc.TAIL - 1, cols, size)
    assert fc.far_rows(fc.L32, 70001) * 70001 <= fc.INT32_MAX and 15400 < fc.far_rows(fc.L32, 70001) < 15600
    for name, cols in fc.AREA_CASES:
        rows, _ = fc.area_shape(fc.LINES[name], cols)
        assert rows * cols <= fc.INT32_MAX and fc.rows_past(fc.LINES[name], rows - fc.TAIL, cols)
        if cols % 4:
            assert rows % 4 == 2 and pr.cv_round(rows / 4) == rows // 4 + 1          # a partial bottom block that is kept
        else:
            assert rows % 4 == 0
    for name, (dt, rows, cols, has_nodata) in fc.OVERVIEW_CASES.items():
        assert rows * cols <= fc.INT32_MAX, name
        assert not has_nodata or dt == "<f4"
    dt, rows, cols, _ = fc.OVERVIEW_CASES["u16-L31"]
    assert fc.rows_past(fc.L31, fc.overview_tail_start(rows), cols, 2) and 2 * rows * cols < fc.L32
    dt, rows, cols, _ = fc.OVERVIEW_CASES["u8-largest"]
    assert rows * cols <= fc.INT32_MAX < (rows + 1) * cols and rows * cols < fc.L31
    for name in ("f32-odd", "f32-odd-nodata"):
        _, rows, cols, _ = fc.OVERVIEW_CASES[name]
        assert rows % 2 == 1 and cols % 2 == 1 and fc.rows_past(fc.L32, fc.overview_tail_start(rows), cols)
    rows, cols = fc.INFILL_GRIDS["largest"]()
    assert rows * cols <= fc.INT32_MAX < (rows + 1) * cols and 4 * rows * cols > fc.L32 + fc.L31
    rows, cols = fc.INFILL_GRIDS["L32"]()
    assert fc.INFILL_WINDOW == 160 and fc.rows_past(fc.L32, rows - fc.INFILL_WINDOW, cols)
    assert fc.offset(fc.CANVAS[0] - 1, fc.CANVAS[1]) > fc.L32 and 4 * fc.RASTER[0] * fc.RASTER[1] > fc.L31
    assert fc.rows_past(fc.L32, fc.STITCH_ROWS - fc.TAIL, fc.STITCH_PITCH)
    chunks = fc.merge_chunks()
    assert chunks[0][0] == 0 and chunks[-1][1] == fc.MERGE_COUNT and 4 * chunks[-1][0] < fc.L32 <= 4 * (fc.MERGE_COUNT - 4099)
    assert any(4 * a < fc.L31 < 4 * b for a, b in chunks) and any(4 * a < fc.L32 < 4 * b for a, b in chunks)
    assert fc.MERGE_COUNT % (8192 * 256) not in (0,) and fc.MERGE_COUNT % 256             # a ragged last trip and block
    offs = fc.line_offsets(6000)
    for line in fc.LINES.values():
        assert any(o + 6000 <= line for o in offs) and any(o < line < o + 6000 for o in offs) and any(o >= line for o in offs)
    assert any(o % 2 for o in offs) and max(offs) + 2 * 6000 + 128 < fc.LZW_BYTES


def test_every_case_stays_inside_the_device_memory_budget():
    table = fc.budgets()
    assert len(table) >= 25
    for name, need in table.items():
        assert 0 < need <= fc.BUDGET, (name, need / fc.GIB)
    assert table["halo_merge"] > 16 * fc.GIB              # the case that sets the budget
    assert table["infill-largest"] > 2 * fc.L32           # and the one with the largest single array
    assert fc.infill_workspace_bytes(96, 1100) == 16 + 8 * 96 * 18 + 4 * 48 * 550


# ---- refusals that return before anything touches a device ----------------------------------------------------------------------
def test_one_row_more_than_the_largest_grid_is_refused_on_the_host_side():
    lib = _lib.load()
    for cols in fc.COLS:
        rows = fc.largest_rows(cols)
        assert lib.msr_infill_workspace_bytes(rows, cols) == fc.infill_workspace_bytes(rows, cols)
        assert lib.msr_infill_workspace_bytes(rows + 1, cols) == -1
        grid = np.full(16, 5.0, np.float32)
        work = np.zeros(64, np.uint8)
        rc = lib.msr_infill_small_holes(None, grid.ctypes.data_as(C.c_void_p), 0, rows + 1, rows + 1, cols, NOVAL, 24, 32,
                                        work.ctypes.data_as(C.c_void_p), 1 << 40, None)
        msg = lib.msr_last_error(None).decode()
        assert rc == _lib.MSR_ERR_INVALID and "msr_infill_small_holes" in msg and "exceed 2^31 - 1 pixels" in msg, msg
        out = np.full(16, 7, np.uint8)
        rc = lib.msr_overview_half(None, grid.ctypes.data_as(C.c_void_p), rows + 1, cols, ord("u"), 1, 0, NOVAL,
                                   out.ctypes.data_as(C.c_void_p), None)
        msg = lib.msr_last_error(None).decode()
        assert rc == _lib.MSR_ERR_INVALID and "rows x cols" in msg, msg
        assert (grid == 5.0).all() and (out == 7).all() and not work.any()

"""GPU (-m gpu): the raster kernels past the 2 GiB and 4 GiB offset lines, and the 32-bit entry checks at their boundary.

The production raster (BASELINE configs[3], 15000 x 70000 float32) is 4.2 GB and its padded canvas 4.65 GB; the kernels that
walk such rasters do their index arithmetic by hand.  Every case here puts the region it compares past L31 = 2^31 or
L32 = 2^32 BYTES of a buffer (and says so with an assertion), so a dropped 64-bit cast in an offset reads or writes the
wrong place and fails a comparison; where an entry keeps an index in 32 bits, the largest accepted value runs and the first
refused one returns its error with a canary untouched.

Every comparison is for equal bits.  A reference is never the kernel under test: the NumPy oracles and twins of the project
(oracle/preprocess_ref.py, oracle/tiler_ref.py, infill.infill_reference, geotiff.overview_reference, the host LZW codecs, the
float64 Chan combine), applied to the rows that are compared through the row-restricted forms of tests/far_offset_cases.py,
which tests/test_far_offsets_host.py pins against the whole-raster oracles.  Only tail windows (tens of MB) cross to the host;
fills and whole-array checks run on the device.  No test holds more than 20 GiB of device memory (asserted from
torch.cuda.max_memory_allocated), and each frees what it took.
"""
import functools
import gc

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G
from oracle import preprocess_ref as pr
from oracle import tiler_ref
from tests import far_offset_cases as fc

pytestmark = pytest.mark.gpu
NOVAL = fc.NOVAL
L31, L32 = fc.L31, fc.L32


def budgeted(fn):
    """The device-memory condition of every test here: its peak stays at or under 20 GiB, and it leaves nothing cached."""
    @functools.wraps(fn)
    def wrapper(*args, **kw):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        try:
            fn(*args, **kw)
        finally:
            gc.collect()
            torch.cuda.empty_cache()
        peak = torch.cuda.max_memory_allocated()
        assert peak <= fc.BUDGET, f"{peak / fc.GIB:.2f} GiB of device memory at the peak"
    return wrapper


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from moonsuperresolution_amd import ops
    c = ops.OpContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiler64(hip_lib):
    """A tiler handle for S = 64 that carries NumPy's blend window, as the drivers' handles do."""
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig
    d = DEMSuperResolution(DSRConfig(image_size=64, stride=16, batch_size=4, tile_size=128))
    yield d
    d.close()


def upload(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def far_tensor(rows, cols, tail, dtype=torch.float32, fill=0):
    """rows x cols on the device, ``fill`` everywhere but the last len(tail) rows, which are ``tail`` (a host array)."""
    t = torch.full((rows, cols), fill, dtype=dtype, device="cuda")
    t[rows - len(tail):] = upload(tail)
    return t


def tail_values(rows, cols, seed, nodata=True):
    """Host float32 rows with NaNs and no-data cells (at and below no_value) planted."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((rows, cols), dtype=np.float32) * 1000).astype(np.float32)
    n = rows * cols
    flat = a.reshape(-1)
    flat[rng.integers(0, n, n // 500)] = np.nan
    if nodata:
        flat[rng.integers(0, n, n // 100)] = NOVAL
        flat[rng.integers(0, n, n // 400)] = NOVAL - 5.0
    a[1, 1] = a[rows - 1, cols - 1] = np.nan
    return a


def sentinel(shape, dtype=torch.float32):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), 0x7F, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def untouched(*tensors):
    return all(bool((t.contiguous().view(torch.uint8) == 0x7F).all()) for t in tensors)


def count_not(t, value, chunk=fc.CHECK_CHUNK):
    """How many elements of ``t`` differ from ``value``, counted on the device in chunks: the temporaries stay at 128 MB (a
    whole-array comparison of a far raster would hold a bool image of it, and torch's own count a wider one)."""
    flat = t.contiguous().view(-1)
    return sum(int((flat[i:i + chunk] != value).sum()) for i in range(0, flat.numel(), chunk))


def same_bits(t, a):
    """A float32 device tensor against a host array, bit for bit, NaNs included."""
    return fc.bits_equal(t.cpu().numpy(), a)


# ---- 1. msr_resize_area / msr_resize_area_rows, factor 4 -------------------------------------------------------------------------
@pytest.mark.parametrize("line,cols", fc.AREA_CASES)
@budgeted
def test_area_resize_reads_past_the_line(ctx, line, cols):
    """The whole-raster form on a far source: the destination rows whose source blocks lie past the line.  70001 columns: the
    scalar path and a last destination row whose block holds two source rows; 70000: the float4 path.  A 32-bit
    ``y0 * w`` in resize_area_kernel's ``base`` (tiler.hip) would read another row."""
    L = fc.LINES[line]
    rows, _ = fc.area_shape(L, cols)
    dh, dw = pr.cv_round(rows / 4), pr.cv_round(cols / 4)
    d0 = -(-fc.first_row_past(L, cols) // 4)              # the first destination row whose whole block lies past the line
    s0 = 4 * d0
    assert fc.rows_past(L, s0, cols) and dh - d0 >= 24
    tail = tail_values(rows - s0, cols, seed=cols + (L >> 31))
    src = far_tensor(rows, cols, tail)
    dst = torch.full((dh, dw), 7.0, dtype=torch.float32, device="cuda")
    rc = ctx.lib.msr_resize_area(ctx.h, src.data_ptr(), rows, cols, 4, dst.data_ptr(), dh, dw, None)
    assert rc == 0, ctx.lib.msr_last_error(ctx.h)
    torch.cuda.synchronize()
    want = fc.area_rows_ref(tail, s0, rows, 4, d0, dh)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert same_bits(dst[d0:], want)
    if cols % 4:
        assert rows % 4 == 2 and dh == rows // 4 + 1      # the last row is the partial block's
    assert count_not(dst[:d0 - 1], 0) == 0    # blocks of the zeros before the tail
    del src, dst


@pytest.mark.parametrize("line,cols,flags", fc.AREA_ROWS_CASES)
@budgeted
def test_area_rows_on_a_window_that_straddles_the_line(ctx, line, cols, flags):
    """msr_resize_area_rows on a source window inside the far raster that starts before the line and ends after it, with both
    MSR_RESIZE_* flags off and on; no-data cells and NaNs are planted in the window."""
    L = fc.LINES[line]
    rows, _ = fc.area_shape(L, cols)
    dh, dw = pr.cv_round(rows / 4), pr.cv_round(cols / 4)
    first = fc.first_row_past(L, cols)
    d_lo = first // 4 - 16
    s_lo = 4 * d_lo
    d0 = -(-first // 4)
    assert fc.offset(s_lo, cols) < L < fc.offset(rows, cols) and fc.rows_past(L, 4 * d0, cols) and d_lo < d0 < dh
    window = tail_values(rows - s_lo, cols, seed=cols + flags)
    src = far_tensor(rows, cols, window)
    dst = sentinel((dh - d_lo + 2, dw))                   # a guard row either side
    rc = ctx.lib.msr_resize_area_rows(ctx.h, src.data_ptr() + fc.offset(s_lo, cols), s_lo, rows - s_lo, rows, cols, 4,
                                      dst[1:].data_ptr(), d_lo, dh - d_lo, dw, NOVAL, flags, None)
    assert rc == 0, ctx.lib.msr_last_error(ctx.h)
    torch.cuda.synchronize()
    want = fc.area_rows_ref(window, s_lo, rows, 4, d_lo, dh, NOVAL, flags)
    got = dst[1:-1].cpu().numpy()
    assert fc.bits_equal(got[d0 - d_lo:], want[d0 - d_lo:]), "rows whose source blocks lie past the line"
    assert fc.bits_equal(got, want)
    assert untouched(dst[0], dst[-1])
    if flags:
        assert not np.isnan(want).any() and (want == np.float32(NOVAL)).any()
    else:
        assert np.isnan(want).any()
    del src, dst


# ---- 2. msr_resize_cubic / msr_resize_cubic_rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("line,cols", fc.CUBIC_CASES)
@budgeted
def test_cubic_upsampling_stores_past_the_line(ctx, line, cols):
    """A small source to the far shape: the stores of the last 32 rows and of 32 rows straddling each line, then the _rows form
    writing the last 64 rows into their place of a zeroed far buffer."""
    L = fc.LINES[line]
    rows = fc.far_rows(L, cols)
    sh, sw = -(-rows // fc.CUBIC_SHRINK), -(-cols // fc.CUBIC_SHRINK)
    rng = np.random.default_rng(cols)
    small = (rng.normal(size=(sh, sw)) * 100 - 2000).astype(np.float32)
    small[sh - 2, 5] = small[3, 4] = np.nan
    src = upload(small)
    dst = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    rc = ctx.lib.msr_resize_cubic(ctx.h, src.data_ptr(), sh, sw, dst.data_ptr(), rows, cols, None)
    assert rc == 0, ctx.lib.msr_last_error(ctx.h)
    torch.cuda.synchronize()
    bands = [(rows - 32, rows)]
    assert fc.rows_past(L, rows - 32, cols)
    for other in (L31, L32):
        if other <= L:
            mid = fc.first_row_past(other, cols)
            assert fc.offset(mid - 16, cols) < other < fc.offset(mid + 16, cols)
            bands.append((mid - 16, mid + 16))
    for r0, r1 in bands:
        s0, s1 = fc.cubic_tap_rows(r0, r1, sh, rows)
        want = fc.cubic_rows_ref(small[s0:s1], s0, sh, rows, cols, r0, r1)
        assert same_bits(dst[r0:r1], want), (r0, r1)
        assert (r0, r1) != bands[0] or (np.isnan(want).any() and not np.isnan(want).all())
    # the window form: destination rows [r0, rows) only, stored at their place
    dst.zero_()
    r0 = rows - 64
    s0, s1 = fc.cubic_tap_rows(r0, rows, sh, rows)
    rc = ctx.lib.msr_resize_cubic_rows(ctx.h, src[s0:s1].data_ptr(), s0, s1 - s0, sh, sw, dst[r0:].data_ptr(), r0, rows - r0,
                                       rows, cols, NOVAL, 0, None)
    assert rc == 0, ctx.lib.msr_last_error(ctx.h)
    torch.cuda.synchronize()
    assert fc.rows_past(L, r0, cols)
    assert same_bits(dst[r0:], fc.cubic_rows_ref(small[s0:s1], s0, sh, rows, cols, r0, rows))
    assert count_not(dst[:r0], 0) == 0
    del src, dst


@pytest.mark.parametrize("line,cols", fc.CUBIC_CASES)
@budgeted
def test_cubic_downsampling_reads_past_the_line(ctx, line, cols):
    """The far source to a small destination: the destination rows whose four taps all read past the line, by the whole form
    and by the window form with both no-data flags."""
    L = fc.LINES[line]
    rows = fc.far_rows(L, cols)
    dh, dw = rows // fc.CUBIC_SHRINK, cols // fc.CUBIC_SHRINK
    idx, _ = pr._cubic_axis(rows, dh)
    first = fc.first_row_past(L, cols)
    d0 = int(np.argmax(idx.min(axis=1) >= first))
    s0, s1 = fc.cubic_tap_rows(d0, dh, rows, dh)
    assert s0 >= first and fc.rows_past(L, s0, cols) and dh - d0 >= 4 and s1 <= rows
    tail = tail_values(rows - s0, cols, seed=cols + 1)
    src = far_tensor(rows, cols, tail)
    dst = torch.zeros((dh, dw), dtype=torch.float32, device="cuda")
    rc = ctx.lib.msr_resize_cubic(ctx.h, src.data_ptr(), rows, cols, dst.data_ptr(), dh, dw, None)
    assert rc == 0, ctx.lib.msr_last_error(ctx.h)
    torch.cuda.synchronize()
    want = fc.cubic_rows_ref(tail, s0, rows, dh, dw, d0, dh)
    assert same_bits(dst[d0:], want) and np.isnan(want).any() and not np.isnan(want).all()
    flags = fc.NODATA_TO_NAN | fc.NAN_TO_NODATA
    part = sentinel((dh - d0 + 2, dw))
    rc = ctx.lib.msr_resize_cubic_rows(ctx.h, src.data_ptr() + fc.offset(s0, cols), s0, rows - s0, rows, cols,
                                       part[1:].data_ptr(), d0, dh - d0, dh, dw, NOVAL, flags, None)
    assert rc == 0, ctx.lib.msr_last_error(ctx.h)
    torch.cuda.synchronize()
    want = fc.cubic_rows_ref(tail, s0, rows, dh, dw, d0, dh, NOVAL, flags)
    assert same_bits(part[1:-1], want) and untouched(part[0], part[-1]) and (want == np.float32(NOVAL)).any()
    del src, dst, part


# ---- 3. msr_infill_small_holes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(fc.INFILL_GRIDS))
@budgeted
def test_infill_on_a_far_grid(hip_lib, grid):
    """Components of 1 .. 31 pixels in the first rows and in the last fillable rows of a grid that is valid everywhere else
    ("L32": the tail window lies past 2^32 bytes; "largest": floor(INT32_MAX / cols) rows, 8.6 GB, so that ``r * cols + c`` of
    infill.hip's first-pixel list is within a few rows of INT32_MAX).  Reference: the twin on the head and the tail window."""
    lib = hip_lib
    rows, cols = fc.INFILL_GRIDS[grid]()
    H, area, margin = fc.INFILL_WINDOW, fc.INFILL_MAX_AREA, fc.INFILL_MARGIN
    head, _, _ = fc.infill_window("head", rows, cols, seed=1)
    tail, t0, planted = fc.infill_window("tail", rows, cols, seed=2)
    assert rows * cols <= fc.INT32_MAX and fc.rows_past(L32, t0, cols)
    last = max((t0 + r) * cols + c for pix in planted.values() for r, c in pix if r < H - margin)
    if grid == "largest":
        assert (rows + 1) * cols > fc.INT32_MAX and fc.INT32_MAX - last < (margin + 16) * cols
    g = torch.full((rows, cols), -1900.0, dtype=torch.float32, device="cuda")
    g[:H] = upload(head)
    g[t0:] = upload(tail)
    need = lib.msr_infill_workspace_bytes(rows, cols)
    assert need == fc.infill_workspace_bytes(rows, cols)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.msr_infill_small_holes(None, g.data_ptr(), 0, rows, rows, cols, NOVAL, area, margin, work.data_ptr(), need, None)
    assert rc == 0, lib.msr_last_error(None)
    torch.cuda.synchronize()
    got_head, got_tail = g[:H].cpu().numpy(), g[t0:].cpu().numpy()
    want_head, want_tail = fc.infill_window_ref(head, 0, rows), fc.infill_window_ref(tail, t0, rows)
    assert np.array_equal(got_tail.view(np.uint32), want_tail.view(np.uint32)), "tail window"
    assert np.array_equal(got_head.view(np.uint32), want_head.view(np.uint32)), "head window"
    filled = (want_tail != tail) & (tail == np.float32(NOVAL))
    assert filled.sum() > 200 and (want_tail == np.float32(NOVAL)).sum() > 100      # small ones filled, large ones left
    assert filled[H - margin - 1].any() and not filled[H - margin:].any()           # up to the last fillable row
    assert count_not(g[H:t0], -1900.0) == 0                          # nothing else was written
    del g, work


@budgeted
def test_infill_and_overview_refuse_one_more_row_before_any_launch(hip_lib):
    lib = hip_lib
    cols = 70001
    rows = fc.largest_rows(cols) + 1
    assert lib.msr_infill_workspace_bytes(rows, cols) == -1 and lib.msr_infill_workspace_bytes(rows - 1, cols) > 0
    grid, work, out = sentinel(64), sentinel(64, torch.uint8), sentinel(64, torch.uint8)
    rc = lib.msr_infill_small_holes(None, grid.data_ptr(), 0, rows, rows, cols, NOVAL, 24, 32, work.data_ptr(), 1 << 40, None)
    msg = lib.msr_last_error(None).decode()
    assert rc == _lib.MSR_ERR_INVALID and "msr_infill_small_holes" in msg and "exceed 2^31 - 1 pixels" in msg, msg
    rc = lib.msr_overview_half(None, grid.data_ptr(), rows, cols, ord("u"), 1, 0, NOVAL, out.data_ptr(), None)
    msg = lib.msr_last_error(None).decode()
    assert rc == _lib.MSR_ERR_INVALID and "msr_overview_half" in msg and "rows x cols" in msg, msg
    torch.cuda.synchronize()
    assert untouched(grid, work, out)


# ---- 4. msr_overview_half --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.OVERVIEW_CASES))
@budgeted
def test_overview_of_a_far_raster(hip_lib, name):
    """float32 past 2^32 bytes (odd rows and columns, no-data off and on; an even shape), uint16 past 2^31 bytes, uint8 at the
    largest accepted size (the element index of tiff_overview.h's ``r * cols + c`` just under INT32_MAX): the last destination
    rows against geotiff.overview_reference on the tail."""
    lib = hip_lib
    dt, rows, cols, has_nodata = fc.OVERVIEW_CASES[name]
    dt = np.dtype(dt)
    t0 = fc.overview_tail_start(rows)
    rng = np.random.default_rng(rows)
    if dt.kind == "f":
        assert fc.rows_past(L32, t0, cols)
        tail = tail_values(rows - t0, cols, seed=rows)
        tail[2:4, 10:14] = tail[-2:, -3:] = NOVAL         # whole blocks of no-data (t0 is even), the last block among them
        torch_dt, bits = torch.float32, tail
    else:
        if dt.itemsize == 2:
            assert fc.rows_past(L31, t0, cols, 2)
        else:
            assert fc.INT32_MAX - rows * cols < cols
        tail = rng.integers(0, np.iinfo(dt).max + 1, (rows - t0, cols)).astype(dt)
        torch_dt, bits = (torch.int16, tail.view(np.int16)) if dt.itemsize == 2 else (torch.uint8, tail)
    src = far_tensor(rows, cols, bits, torch_dt)
    dr, dc = -(-rows // 2), -(-cols // 2)
    dst = torch.zeros((dr, dc), dtype=torch_dt, device="cuda")
    rc = lib.msr_overview_half(None, src.data_ptr(), rows, cols, ord(dt.kind), dt.itemsize, has_nodata, NOVAL, dst.data_ptr(), None)
    assert rc == 0, lib.msr_last_error(None)
    torch.cuda.synchronize()
    want = fc.overview_tail_ref(tail, NOVAL if has_nodata else None)
    got = dst[t0 // 2:].cpu().numpy().view(dt)
    assert got.shape == want.shape
    if dt.kind == "f":
        assert fc.bits_equal(got, want) and np.isnan(want).any()
        if has_nodata:
            assert (want[1, 5:7] == np.float32(NOVAL)).all() and want[-1, -1] == np.float32(NOVAL)
    else:
        assert np.array_equal(got, want) and want.any()
    assert count_not(dst[:t0 // 2 - 1], 0) == 0      # the zeros before the tail
    del src, dst


# ---- 5. msr_patch_stats / msr_extract_patches on the configs[3] canvas -------------------------------------------------------------
def _configs3_canvases():
    """The padded canvases of tests/test_gpu_tiler.py::test_config3_geometry_at_size_and_one_tile_of_a_shard (a smooth field +
    noise; no-data outside the raster), built on the device 1024 rows at a time so that the temporaries stay small."""
    hp, wp = fc.CANVAS
    rows, cols = fc.RASTER
    halo = 512 - 64
    g = torch.Generator(device="cuda").manual_seed(5)
    dem = torch.empty((hp, wp), dtype=torch.float32, device="cuda")
    img = torch.empty((hp, wp), dtype=torch.float32, device="cuda")
    xx = torch.arange(wp, device="cuda", dtype=torch.float32)[None, :]
    for r in range(0, hp, 1024):
        yy = torch.arange(r, min(r + 1024, hp), device="cuda", dtype=torch.float32)[:, None]
        n = yy.shape[0]
        dem[r:r + n] = -2000 + 600 * torch.sin(xx / 370.0) * torch.cos(yy / 530.0) + torch.randn((n, wp), generator=g, device="cuda")
        img[r:r + n] = 0.5 + 0.3 * torch.cos(xx / 230.0) * torch.sin(yy / 310.0) + 0.05 * torch.randn((n, wp), generator=g, device="cuda")
    for t in (dem, img):
        t[:halo] = NOVAL; t[:, :halo] = NOVAL; t[halo + rows:] = NOVAL; t[:, halo + cols:] = NOVAL
    return img, dem, halo


@budgeted
def test_patch_stats_and_extract_in_the_last_rows_and_columns_of_the_configs3_canvas(hip_lib):
    """Origins in the last patch rows and columns of the 16256 x 71552 canvas (y + S == 16256, x + S == 71552: no-data margin,
    invalid) and valid patches in the raster's last rows, past 2^32 bytes, at S = 512 and S = 64, aligned (float4) and not.
    A 32-bit ``(y0 + y) * cols`` in patch_stats_kernel / extract_patches_kernel (tiler.hip) would cut another window."""
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig
    hp, wp = fc.CANVAS
    rows, cols = fc.RASTER
    img, dem, halo = _configs3_canvases()
    first = fc.first_row_past(L32, wp)
    for S in (512, 64):
        d = DEMSuperResolution(DSRConfig(image_size=S, stride=S // 8, batch_size=4, tile_size=2 * S))
        y_last = halo + rows - S                          # the raster's last valid patch row
        x_last = halo + cols - S
        org = [(wp - S, hp - S), (halo, hp - S), (wp - S, y_last), (x_last + 1, y_last), (halo, y_last + 1),     # margin: invalid
               (halo, y_last), (halo + 1, y_last), (x_last, y_last), (halo + 34567, y_last), (x_last - 3, y_last - 5)]
        if S == 64:
            org += [(halo, first), (x_last, first + 1), (halo + 40001, first + 7)]
            assert fc.rows_past(L32, first, wp) and first + 7 + S <= halo + rows
        n = len(org)
        # every patch reaches past 2^32 bytes with its last row at least; the S = 64 ones lie there whole
        assert all(fc.offset(y + S - 1, wp, col=x) >= L32 and fc.offset(y, wp) >= L31 for x, y in org)
        assert S == 512 or all(fc.rows_past(L32, y, wp) for _, y in org)
        ox = torch.tensor([x for x, _ in org], dtype=torch.int32, device="cuda")
        oy = torch.tensor([y for _, y in org], dtype=torch.int32, device="cuda")
        valid = sentinel(n, torch.uint8)
        mm = sentinel((n, 4))
        rc = d._lib.msr_patch_stats(d._h, img.data_ptr(), dem.data_ptr(), hp, wp, ox.data_ptr(), oy.data_ptr(), n, NOVAL,
                                    valid.data_ptr(), mm.data_ptr(), None)
        assert rc == 0
        out = torch.empty((n, S, S, 2), dtype=torch.float32, device="cuda")
        rc = d._lib.msr_extract_patches(d._h, img.data_ptr(), dem.data_ptr(), hp, wp, ox.data_ptr(), oy.data_ptr(), mm.data_ptr(),
                                        n, out.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        valid, mm = valid.cpu().numpy(), mm.cpu().numpy()
        flags = []
        for i, (x, y) in enumerate(org):
            ip, dp = img[y:y + S, x:x + S].cpu().numpy(), dem[y:y + S, x:x + S].cpu().numpy()
            ok, ip, dp = tiler_ref.get_patch(ip, dp, 0, 0, S, NOVAL)
            flags.append(ok)
            assert bool(valid[i]) == ok, (S, x, y)
            if ok:
                patch, (lo, hi) = tiler_ref.normalize(ip, dp)
                assert mm[i, 2] == lo and mm[i, 3] == hi and mm[i, 0] == ip.min() and mm[i, 1] == ip.max(), (S, x, y)
                assert np.array_equal(out[i].cpu().numpy(), patch), (S, x, y)
        assert flags[:5] == [False] * 5 and all(flags[5:])
        d.close()
        del out
    del img, dem


# ---- 6. msr_stitch_accumulate_band -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc_row0", [0, 1000])
@budgeted
def test_stitch_band_accumulates_past_the_line(tiler64, acc_row0):
    """Three zeroed slabs of pitch 71552 that pass 2^32 bytes (13 GB together); one band of 3 x 2 patches at the left end of the
    width and 3 x 2 at the right end, in canvas rows whose slab rows lie past the line.  Reference: the oracle's accumulation
    of the same bands on small canvases (the update does not depend on the position).  A 32-bit ``(y - acc_row0) * pitch`` in
    stitch_band_kernel (tiler.hip) would update other rows: the compared windows would stay zero and the rows above row_lo
    would not."""
    d = tiler64
    S, stride, nx, ny = 64, 16, 3, 2
    pitch, slab_rows = fc.STITCH_PITCH, fc.STITCH_ROWS
    bh, bw = (ny - 1) * stride + S, (nx - 1) * stride + S
    top = fc.first_row_past(L32, pitch) + 8               # slab row of the band's first row
    assert fc.rows_past(L32, top, pitch) and top + bh <= slab_rows
    y0 = acc_row0 + top                                   # the same, as a canvas row
    x_right = pitch - bw
    assert x_right % stride == 0
    left, right = fc.band_reference(S, stride, nx, ny, seed=1), fc.band_reference(S, stride, nx, ny, seed=2)
    pred = upload(np.concatenate([left[0], right[0]]))
    key = upload(np.concatenate([left[1] + np.int32([0, y0]), right[1] + np.int32([x_right, y0])]).astype(np.int32))
    dmm = upload(np.concatenate([left[2], right[2]]))
    ngx, ngy = x_right // stride + nx, ny
    ws = sentinel(ngx * ngy, torch.int32)
    acc = torch.zeros((3, slab_rows, pitch), dtype=torch.float32, device="cuda")
    rc = d._lib.msr_stitch_accumulate_band(d._h, pred.data_ptr(), key.data_ptr(), dmm.data_ptr(), 2 * nx * ny, stride, 0, y0, ngx,
                                           ngy, ws.data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), pitch,
                                           acc_row0, y0, y0 + bh, pitch, None)
    assert rc == 0, d._lib.msr_last_error(d._h)
    torch.cuda.synchronize()
    assert sorted(v for v in ws.cpu().tolist() if v >= 0) == list(range(2 * nx * ny))
    for k, what in enumerate(("w_sum", "mean", "S")):
        band = acc[k, top:top + bh]
        assert np.array_equal(band[:, :bw].cpu().numpy().view(np.uint32), left[3][k].view(np.uint32)), (what, "left")
        assert np.array_equal(band[:, x_right:].cpu().numpy().view(np.uint32), right[3][k].view(np.uint32)), (what, "right")
        assert count_not(band[:, bw:x_right], 0) == 0, what
        assert count_not(acc[k, :top], 0) == 0, f"{what}: rows above row_lo were written"
        assert count_not(acc[k, top + bh:], 0) == 0, what
    assert (left[3][0] > 0).sum() > 1000 and left[3][2].any()
    del acc, ws


# ---- 7. msr_halo_merge -------------------------------------------------------------------------------------------------------------
def _merge_ref(a, b, lo, hi):
    """tiler_ref.chan_merge + halo_finalize (the float64 Chan combine of test_halo_merge_*) of elements [lo, hi) in torch, where
    one tensor is (w, mean, S) of a and another of b (b None: a alone).  The float32 division and square root of the
    finalisation are evaluated in float64 and rounded once more, which gives the correctly rounded float32 results."""
    wa = ma = sa = a[lo:hi].double()
    if b is None:
        w, m, s = wa, ma, sa
    else:
        wb = mb = sb = b[lo:hi].double()
        w = wa + wb
        dlt = mb - ma
        m = torch.where(wb > 0, torch.where(wa > 0, ma + dlt * (wb / w), mb), ma)
        s = torch.where(wb > 0, torch.where(wa > 0, sa + sb + dlt * dlt * (wa * wb / w), sb), sa)
    w32, m32, s32 = w.float(), m.float(), s.float()
    good = w32 > 0
    s32 = torch.where(s32 < 0, torch.zeros_like(s32), s32)
    std = (s32.double() / w32.double()).float().double().sqrt().float()
    nv = torch.full_like(m32, NOVAL)
    return torch.where(good, m32, nv), torch.where(good, std, nv), good.to(torch.uint8)


@budgeted
def test_halo_merge_over_two_to_the_thirty_elements(tiler64):
    """count = 2^30 + 4099: 512 whole trips of the grid-stride loop and a ragged one, element offsets past 2^31 and 2^32 bytes.
    One tensor serves as wa, ma and sa and a second as wb, mb and sb (they are only read); the outputs are distinct."""
    d = tiler64
    n = fc.MERGE_COUNT
    g = torch.Generator(device="cuda").manual_seed(11)
    a = torch.empty(n, dtype=torch.float32, device="cuda").uniform_(-1.5, 5.0, generator=g).clamp_(min=0)
    b = torch.empty(n, dtype=torch.float32, device="cuda").uniform_(-1.5, 5.0, generator=g).clamp_(min=0)
    mean = torch.empty(n, dtype=torch.float32, device="cuda")
    std = torch.empty(n, dtype=torch.float32, device="cuda")
    good = torch.empty(n, dtype=torch.uint8, device="cuda")
    chunks = fc.merge_chunks()
    assert 4 * (n - 4099) >= L32 and chunks[-1][1] == n
    for other in (None, b):
        for t in (mean, std, good):
            t.zero_()
        pb = [None] * 3 if other is None else [other.data_ptr()] * 3
        rc = d._lib.msr_halo_merge(d._h, a.data_ptr(), a.data_ptr(), a.data_ptr(), *pb, n, NOVAL, mean.data_ptr(), std.data_ptr(),
                                   good.data_ptr(), None)
        assert rc == 0, d._lib.msr_last_error(d._h)
        torch.cuda.synchronize()
        zeros = 0
        for lo, hi in chunks:
            rm, rs, rg = _merge_ref(a, other, lo, hi)
            form = "finalise" if other is None else "merge"
            assert torch.equal(good[lo:hi], rg), (form, lo, "good")
            assert torch.equal(mean[lo:hi].view(torch.int32), rm.view(torch.int32)), (form, lo, "mean")
            assert torch.equal(std[lo:hi].view(torch.int32), rs.view(torch.int32)), (form, lo, "std")
            zeros += int((rg == 0).sum())
        assert zeros > 1000                               # both forms met pixels that nothing covers
        assert bool(good[-1] == 1) == bool((a[-1] > 0) or (other is not None and other[-1] > 0))
    del a, b, mean, std, good


# ---- 8. msr_tiff_blocks_to_f32 -----------------------------------------------------------------------------------------------------
SENT = -77.25


@pytest.mark.parametrize("kind,sb", fc.BLOCK_KINDS)
@budgeted
def test_blocks_to_f32_far_source_and_far_window(hip_lib, kind, sb):
    """Strips and tiles whose bytes lie past 2^32 in the source buffer (allocated to that size, initialised only where a block
    lies; every other block at an odd offset: the byte-wise path) and whose rows make ``row * cols`` of the float32 window cross
    2^31 and 2^32 bytes.  Unlisted rows keep the sentinel."""
    lib = hip_lib
    cols = fc.BLOCK_COLS
    rows = fc.far_rows(L32, cols)
    out = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    src = torch.empty(fc.BLOCK_SRC_BYTES, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(sb * 100 + ord(kind))
    for predictor in (1, 2):
        for bw, bh, xs in ((cols, 3, (0,)), (272, 16, (0, 257 * 272))):       # strips; tiles, the right one hangs over the edge
            out.fill_(SENT)
            origins = []
            for line in (L31, L32):
                mid = fc.first_row_past(line, cols)
                y0 = mid - 2 if bh == 3 else mid - 5
                assert fc.offset(y0, cols) < line < fc.offset(y0 + bh, cols)
                origins += [(x, y0) for x in xs]
            origins += [(xs[-1], rows - bh)]
            pos, offs, values = L32 + 64, [], []
            for i, _ in enumerate(origins):
                raw, val = fc.tiff_block(kind, sb, bw, bh, predictor, rng)
                pos += (sb - pos % sb) % sb + (i & 1)     # aligned to the sample, then odd for every other block
                assert pos >= L32 and pos + raw.size <= fc.BLOCK_SRC_BYTES
                src[pos:pos + raw.size] = upload(raw)
                offs.append(pos)
                values.append(val)
                pos += raw.size + 7
            n = len(origins)
            d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
            d_xy = torch.tensor([x for x, _ in origins] + [y for _, y in origins], dtype=torch.int32, device="cuda")
            rc = lib.msr_tiff_blocks_to_f32(None, src.data_ptr(), d_off.data_ptr(), d_xy.data_ptr(), d_xy.data_ptr() + 4 * n, n,
                                            bw, bh, ord(kind), sb, predictor, out.data_ptr(), 0, rows, cols, None)
            assert rc == 0, lib.msr_last_error(None)
            torch.cuda.synchronize()
            written = 0
            for (x, y0), val in zip(origins, values):
                w = min(bw, cols - x)
                assert same_bits(out[y0:y0 + bh, x:x + w], val[:, :w]), (predictor, bw, x, y0)
                written += int((val[:, :w] != np.float32(SENT)).sum())
            assert any(o % 2 for o in offs) and any(x + bw > cols for x, _ in origins) == (bw == 272)
            assert count_not(out, SENT) == written, "an element outside the listed blocks was written"
    del out, src


# ---- 9. msr_lzw_encode_strips / msr_lzw_decode_strips ------------------------------------------------------------------------------
def _tables(src_off, src_len, dst_off, dst_cap):
    t64 = torch.tensor(list(src_off) + list(dst_off), dtype=torch.int64, device="cuda")
    t32 = torch.tensor(list(src_len) + list(dst_cap), dtype=torch.int32, device="cuda")
    n = len(src_off)
    return t64, t32, (t64.data_ptr(), t32.data_ptr(), t64.data_ptr() + 8 * n, t32.data_ptr() + 4 * n)


@budgeted
def test_lzw_strips_with_offsets_around_the_lines(hip_lib):
    """Hand-built tables (the Python wrappers pack their slots inside 1 GiB bands): strips whose src_off and dst_off lie just
    below, across and above 2^31 and 2^32 in uint8 buffers larger than 2^32; the encoder with the predictor fused (sample_bytes
    4 and 2) and without, then the decoder.  Streams, lengths and decoded bytes against the host codecs; the bytes before and
    after every slot keep their pattern."""
    lib = hip_lib
    size = fc.LZW_BYTES
    src = torch.empty(size, dtype=torch.uint8, device="cuda")
    dst = torch.empty(size, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(9)
    rb, nrow, guard = 1200, 5, 64
    length = rb * nrow
    for sbytes in (0, 4, 2):
        cap = 2 * length + 64
        src_off, dst_off = fc.line_offsets(length), fc.line_offsets(cap)
        assert any(o < L32 < o + length for o in src_off) and any(o >= L32 for o in src_off) and any(o % 2 for o in src_off)
        assert any(o < L32 < o + cap for o in dst_off) and any(o < L31 < o + cap for o in dst_off) and max(dst_off) > L32
        dst.fill_(0xA5)
        datas = []
        for o in src_off:
            ut = np.dtype(f"<u{sbytes or 1}")
            data = np.cumsum(rng.integers(-3, 4, (nrow, rb // ut.itemsize)), axis=1).astype(ut).view(np.uint8).reshape(-1)
            src[o:o + length] = upload(data)
            datas.append(data)
        n = len(src_off)
        t64, t32, (p_so, p_sl, p_do, p_dc) = _tables(src_off, [length] * n, dst_off, [cap] * n)
        dst_len = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        rc = lib.msr_lzw_encode_strips(None, src.data_ptr(), p_so, p_sl, n, sbytes, rb if sbytes else 0, dst.data_ptr(), p_do, p_dc,
                                       dst_len.data_ptr(), None)
        assert rc == _lib.MSR_OK, lib.msr_last_error(None)
        torch.cuda.synchronize()
        lens = dst_len.cpu().tolist()
        for o, data, got in zip(dst_off, datas, lens):
            want = G.lzw_encode(fc.predict(data, sbytes, rb))
            assert got == len(want), (sbytes, o)
            assert dst[o:o + got].cpu().numpy().tobytes() == want, (sbytes, o)
            around = torch.cat([dst[o - guard:o], dst[o + cap:o + cap + guard]])
            assert bool((around == 0xA5).all()), (sbytes, o, "bytes outside the slot were written")
    # the decoder: the host encoder's streams at the same far offsets, slots a little larger than the data
    dst.fill_(0xA5)
    cap = length + 16
    src_off, dst_off = fc.line_offsets(2 * length), fc.line_offsets(cap)
    datas, streams = [], []
    for o in src_off:
        data = rng.integers(0, 64, length, dtype=np.uint8)
        stream = np.frombuffer(G.lzw_encode(data), np.uint8)
        assert stream.size <= 2 * length
        src[o:o + stream.size] = upload(stream.copy())
        datas.append(data)
        streams.append(stream)
    n = len(src_off)
    t64, t32, (p_so, p_sl, p_do, p_dc) = _tables(src_off, [s.size for s in streams], dst_off, [cap] * n)
    dst_len = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    rc = lib.msr_lzw_decode_strips(None, src.data_ptr(), p_so, p_sl, n, dst.data_ptr(), p_do, p_dc, dst_len.data_ptr(), None)
    assert rc == _lib.MSR_OK, lib.msr_last_error(None)
    torch.cuda.synchronize()
    assert dst_len.cpu().tolist() == [length] * n
    for o, data in zip(dst_off, datas):
        slot = dst[o - guard:o + cap + guard].cpu().numpy()
        assert slot[guard:guard + length].tobytes() == data.tobytes(), o
        assert not slot[guard + length:guard + cap].any(), o              # the zeroed tail of the slot
        assert (slot[:guard] == 0xA5).all() and (slot[guard + cap:] == 0xA5).all(), (o, "bytes outside the slot were written")
    del src, dst


# ---- 10. refusals at their boundary ------------------------------------------------------------------------------------------------
@budgeted
def test_area_rows_refuses_destination_rows_times_factor_past_int32(ctx):
    """dst_row0 + dst_rows == INT32_MAX / 4 + 1 is refused with its message; INT32_MAX / 4 is the largest accepted and runs:
    the block's first source row, 4 * 536870910 = 2147483640, is a valid int and its four rows end at full_rows."""
    lib, h = ctx.lib, ctx.h
    cols, dw = 8, 2
    top = fc.INT32_MAX // 4                               # 536870911
    src = upload(np.random.default_rng(2).normal(size=(4, cols)).astype(np.float32))
    dst = sentinel((3, dw))
    rc = lib.msr_resize_area_rows(h, src.data_ptr(), fc.INT32_MAX - 3, 3, fc.INT32_MAX, cols, 4, dst[1:].data_ptr(), top, 1, dw,
                                  NOVAL, 0, None)
    msg = lib.msr_last_error(h).decode()
    torch.cuda.synchronize()
    assert rc == _lib.MSR_ERR_INVALID and "destination rows x factor exceed int32" in msg and untouched(dst), msg
    y0 = 4 * (top - 1)
    rc = lib.msr_resize_area_rows(h, src.data_ptr(), y0, 4, y0 + 4, cols, 4, dst[1:].data_ptr(), top - 1, 1, dw, NOVAL, 0, None)
    assert rc == 0, lib.msr_last_error(h)
    torch.cuda.synchronize()
    want = pr.resize_area(src.cpu().numpy(), 0.25, 0.25)
    assert want.shape == (1, dw) and same_bits(dst[1:2], want) and untouched(dst[0], dst[2])


@budgeted
def test_band_grid_refusal_and_the_largest_accepted_grid(tiler64):
    """ngx * ngy == 2^31 is refused before any launch; INT32_MAX x 1 cells (an 8.6 GB workspace, stride 1) is the largest
    accepted: the patch keyed at the last cell lands in the last word of the workspace (stitch_band_grid_kernel's 64-bit
    ``gy * ngx + gx`` and the launcher's ``sizeof(int) * ngx * ngy``), the patch at cell 0 is accumulated as the oracle does."""
    d = tiler64
    lib, h = d._lib, d._h
    S = 64
    pred, key, dmm, want = fc.band_reference(S, 1, 1, 1, seed=3)
    t_pred = upload(np.concatenate([pred, pred]))
    t_key = upload(np.array([[0, 0], [fc.INT32_MAX - 1, 0]], np.int32))
    t_dmm = upload(np.concatenate([dmm, dmm]))
    acc = sentinel((3, S, S))
    small = sentinel(16, torch.int32)
    rc = lib.msr_stitch_accumulate_band(h, t_pred.data_ptr(), t_key.data_ptr(), t_dmm.data_ptr(), 2, 1, 0, 0, 1 << 16, 1 << 15,
                                        small.data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), S, 0, 0, S, S,
                                        None)
    msg = lib.msr_last_error(h).decode()
    torch.cuda.synchronize()
    assert rc == _lib.MSR_ERR_INVALID and "msr_stitch_accumulate_band: patch grid 65536 x 32768" in msg, msg
    assert untouched(acc, small)
    ngx = fc.INT32_MAX
    ws = torch.empty(ngx, dtype=torch.int32, device="cuda")
    acc = torch.zeros((3, S, S), dtype=torch.float32, device="cuda")
    rc = lib.msr_stitch_accumulate_band(h, t_pred.data_ptr(), t_key.data_ptr(), t_dmm.data_ptr(), 2, 1, 0, 0, ngx, 1,
                                        ws.data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), S, 0, 0, S, S, None)
    assert rc == 0, lib.msr_last_error(h)
    torch.cuda.synchronize()
    assert int(ws[0]) == 0 and int(ws[-1]) == 1 and count_not(ws, -1) == 2
    assert fc.offset(0, 1, 4, col=ngx - 1) > L32 + L31
    for k in range(3):
        assert np.array_equal(acc[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k
    del ws, acc


@budgeted
def test_sampler_noise_refuses_two_to_the_thirty_three_values(ctx):
    """B * L == 2^33 is refused and leaves the buffer alone.  The largest accepted size (2^33 - 4 values, 32 GiB) is beyond the
    memory budget of this file and is not run."""
    eps = sentinel(64)
    rc = ctx.lib.msr_sampler_noise(ctx.h, 7, None, 0, eps.data_ptr(), 1 << 20, 1 << 13, None)
    msg = ctx.lib.msr_last_error(ctx.h).decode()
    torch.cuda.synchronize()
    assert rc == _lib.MSR_ERR_INVALID and "msr_sampler_noise" in msg and "B * L / 4 < 2^31" in msg, msg
    assert untouched(eps)
    rc = ctx.lib.msr_sampler_noise(ctx.h, 7, None, 0, eps.data_ptr(), 4, 16, None)      # and a good call writes all of it
    torch.cuda.synchronize()
    assert rc == 0 and not (eps.view(torch.uint8) == 0x7F).all() and bool(torch.isfinite(eps).all())

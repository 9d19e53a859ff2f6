"""GPU (-m gpu): the tiler / stitcher / halo kernels of csrc/tiler.hip on the far side of their branches, bit for bit against
NumPy (oracle/tiler_ref.py, or a few lines written here).  tests/test_gpu_tiler.py, test_gpu_halo.py and test_gpu_range_scan.py
keep every kernel on one side of each of these:

  compact_patches   n > 1024: second and later passes of the `for (start...)` loop, the running `base`, `wsum[]` reused
  patch_stats       the scalar branch (x0 % 4 != 0 or cols % 4 != 0), the outside-the-canvas branch, S >= 256 against the oracle
  extract_patches   S >= 256: the grid is capped at 64 blocks, so the grid-stride loop only turns for S > 128
  stitch_tile       strides that divide neither S nor T (lo_idx / hi_idx rounding), T % 16 != 0 (partial 16 x 16 blocks),
                    S = 256 / 512 with predictions that are not constant
  halo_merge        n > 8192 * 256 (the grid-stride loop), one-sided / zero weights, the S < 0 clamp, NaN in S, on purpose

Every comparison is np.array_equal (equal_nan=True only where a NaN is put in on purpose): the kernels mirror NumPy op for op
in the same types, so there is no tolerance to state.  Origins outside the canvas go to msr_patch_stats only (it checks them);
msr_extract_patches is documented not to, and never gets one.

Whole-map geometries satisfy (T + S) % s == 0: otherwise the last grid line's patch overhangs the reference's own
[T + 2(S - s)]^2 accumulator and the reference raises a broadcast error as soon as such a patch is valid (Stitcher).

Wall time on one MI355X box: see WALL_TIME below.
"""
import numpy as np
import pytest
import torch

from oracle import tiler_ref
from tests.helpers import synthetic_raster
from tests.test_gpu_halo import run_halo

pytestmark = pytest.mark.gpu
NOVAL = -32768.0

# WALL_TIME: not measured yet — no MI355X run of this file has been made.  The oracle half of it (everything but the kernel
# launches and the copies) takes 6 s on a CPU, 3 s of which is the 300 x 300 / stride 4 map and its nine tiles of 2209 patches.


def f32_identity(x, training=False):
    """The reference's identity self-check, returning float32 like a real model does."""
    return np.asarray(x, np.float32)


@pytest.fixture(scope="module")
def handle(hip_lib):
    """DEMSuperResolution objects without a model (a handle for the tiler kernels only), one per geometry, shared by the tests
    of this file and closed at the end."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig
    made = {}

    def get(S, stride, T, B=4):
        key = (S, stride, T, B)
        if key not in made:
            made[key] = DEMSuperResolution(DSRConfig(image_size=S, stride=stride, batch_size=B, tile_size=T))
        return made[key]

    yield get
    for d in made.values():
        d.close()


def sentinel(shape, dtype=torch.int32):
    """A device buffer of 0x7F bytes, as `dtype` (int32 / float32 both read 0x7F7F7F7F, uint8 0x7F).  Every output starts as
    this pattern, so a slot the kernel does not write fails the compare."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), 0x7F, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def bits(t):
    """Device float32 / int32 tensor -> host uint32 view: rows that are copied must not be canonicalised."""
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------
# 1. compaction across the 1024 boundary
# ------------------------------------------------------------------------------------------------------------------
def compact_ref(valid, ox, oy, mm_bits, tile_x, tile_y, B, cap):
    """The NumPy twin of compact_patches_kernel: stable selection, keys relative to the tile, tail filled up to `cap`."""
    sel = np.flatnonzero(valid != 0)
    c = len(sel)
    sx, sy = np.full(cap, -1, np.int32), np.full(cap, -1, np.int32)
    key = np.full((cap, 2), -1, np.int32)
    smm, dmm = np.zeros((cap, 4), np.uint32), np.zeros((cap, 2), np.uint32)
    sx[:c], sy[:c], smm[:c] = ox[sel], oy[sel], mm_bits[sel]
    key[:c, 0], key[:c, 1] = ox[sel] - tile_x, oy[sel] - tile_y
    dmm[:c] = mm_bits[sel, 2:4]
    return sx, sy, smm, key, dmm, np.array([c, -(-c // B)], np.int32)


def validity_patterns(n, rng):
    idx = np.arange(n)
    last_pass = (n - 1) // 1024 * 1024
    return {
        "all": np.ones(n, bool),
        "none": np.zeros(n, bool),
        "every third": idx % 3 == 0,
        "random half": rng.random(n) < 0.5,
        "last pass only": idx >= last_pass,
        "first pass only": idx < 1024,
    }


COMPACT_N = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2209, 3713)
COMPACT_LONG_TAIL = (65, 1025, 2209)         # these also run with cap = minimum + 2B


def test_compact_patches_across_1024(handle):
    d = handle(64, 16, 128)
    rng = np.random.default_rng(20)
    tile_x, tile_y = 384, 1152
    launches = 0
    for n in COMPACT_N:
        ox = rng.integers(0, 70000, n).astype(np.int32)
        oy = rng.integers(0, 16000, n).astype(np.int32)
        mm = rng.standard_normal((n, 4)).astype(np.float32)
        mm_bits = mm.view(np.uint32)
        mm_bits[0::5, 1] = 0x7FC12345             # a NaN with a payload
        mm[0::7, 2] = -0.0
        mm[3::11, 3] = np.nan
        assert np.isnan(mm).any() and (mm_bits == 0x80000000).any()
        t_ox, t_oy, t_mm = (torch.from_numpy(a).cuda() for a in (ox, oy, mm))
        for name, mask in validity_patterns(n, rng).items():
            # `valid != 0` is the test: any non-zero byte counts
            valid = np.where(mask, rng.integers(1, 256, n), 0).astype(np.uint8)
            t_valid = torch.from_numpy(valid).cuda()
            for B in (3, 8, 16):
                cap_min = max(B, -(-n // B) * B)
                for cap in (cap_min, cap_min + 2 * B) if n in COMPACT_LONG_TAIL else (cap_min,):
                    out = [sentinel(cap), sentinel(cap), sentinel((cap, 4), torch.float32), sentinel((cap, 2)),
                           sentinel((cap, 2), torch.float32), sentinel(2)]
                    rc = d._lib.msr_compact_patches(d._h, t_valid.data_ptr(), t_ox.data_ptr(), t_oy.data_ptr(),
                                                    t_mm.data_ptr(), n, tile_x, tile_y, B, cap,
                                                    *(t.data_ptr() for t in out), None)
                    assert rc == 0
                    launches += 1
                    ref = compact_ref(valid, ox, oy, mm_bits, tile_x, tile_y, B, cap)
                    for what, got, want in zip(("sel_x", "sel_y", "sel_mm", "key", "dmm", "meta"), out, ref):
                        got = bits(got)
                        want = want.view(np.uint32)
                        if not np.array_equal(got, want):
                            first = int(np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))[0])
                            src = np.flatnonzero(valid != 0)
                            where = f"candidate {src[first]}, pass {src[first] // 1024}" if first < len(src) else "tail fill"
                            raise AssertionError(f"{what} differs: n={n} pattern={name!r} B={B} cap={cap}, first at slot "
                                                 f"{first} of {len(src)} valid ({where})")
    assert launches == (len(COMPACT_N) + len(COMPACT_LONG_TAIL)) * 6 * 3


# ------------------------------------------------------------------------------------------------------------------
# 2. patch statistics and extraction off the aligned path
# ------------------------------------------------------------------------------------------------------------------
def run_stats(d, t_img, t_dem, rows, cols, org):
    n = len(org)
    ox = torch.from_numpy(np.ascontiguousarray(org[:, 0])).cuda()
    oy = torch.from_numpy(np.ascontiguousarray(org[:, 1])).cuda()
    valid = sentinel(n, torch.uint8)
    mm = sentinel((n, 4), torch.float32)
    rc = d._lib.msr_patch_stats(d._h, t_img.data_ptr(), t_dem.data_ptr(), rows, cols, ox.data_ptr(), oy.data_ptr(), n,
                                NOVAL, valid.data_ptr(), mm.data_ptr(), None)
    assert rc == 0
    return valid.cpu().numpy(), mm.cpu().numpy()


def run_extract(d, t_img, t_dem, rows, cols, org, mm, S):
    """`org` holds in-canvas origins and (-1, -1) pads only: msr_extract_patches does not bounds-check."""
    inside = (org[:, 0] >= 0) & (org[:, 1] >= 0) & (org[:, 0] + S <= cols) & (org[:, 1] + S <= rows)
    assert np.all(inside | ((org[:, 0] == -1) & (org[:, 1] == -1)))
    n = len(org)
    ox = torch.from_numpy(np.ascontiguousarray(org[:, 0])).cuda()
    oy = torch.from_numpy(np.ascontiguousarray(org[:, 1])).cuda()
    t_mm = torch.from_numpy(np.ascontiguousarray(mm, np.float32)).cuda()
    out = sentinel((n, S, S, 2), torch.float32)
    rc = d._lib.msr_extract_patches(d._h, t_img.data_ptr(), t_dem.data_ptr(), rows, cols, ox.data_ptr(), oy.data_ptr(),
                                    t_mm.data_ptr(), n, out.data_ptr(), None)
    assert rc == 0
    return out.cpu().numpy()


def check_stats_and_extract(d, img, dem, org, S):
    """patch_stats on every origin of `org`, extract_patches on the in-canvas ones plus one (-1, -1) pad, against
    tiler_ref.get_patch / normalize.  Origins outside the canvas must come out invalid (their minmax is unspecified).
    Returns (patches compared, of which valid)."""
    rows, cols = dem.shape
    t_img, t_dem = torch.from_numpy(img).cuda(), torch.from_numpy(dem).cuda()
    valid, mm = run_stats(d, t_img, t_dem, rows, cols, org)
    inside = (org[:, 0] >= 0) & (org[:, 1] >= 0) & (org[:, 0] + S <= cols) & (org[:, 1] + S <= rows)
    assert not valid[~inside].any(), org[~inside][valid[~inside] != 0]
    org_in, mm_in = org[inside], mm[inside]
    pad = np.array([[-1, -1]], np.int32)
    out = run_extract(d, t_img, t_dem, rows, cols, np.concatenate([org_in, pad]),
                      np.concatenate([mm_in, np.zeros((1, 4), np.float32)]), S)
    nvalid = 0
    for i, (x0, y0) in enumerate(org_in):
        ok, ip, dp = tiler_ref.get_patch(img, dem, int(x0), int(y0), S, NOVAL)
        assert ip.shape == (S, S)
        where = f"origin ({x0}, {y0}), x0 % 4 = {x0 % 4}, cols % 4 = {cols % 4}"
        assert valid[inside][i] == (1 if ok else 0), where
        nvalid += ok
        patch, (lo, hi) = tiler_ref.normalize(ip, dp)
        want = np.array([ip.min(), ip.max(), lo, hi], np.float32)
        assert np.array_equal(mm_in[i], want), (where, mm_in[i], want)
        assert patch.dtype == np.float32 and np.array_equal(out[i], patch), where
    assert not out[-1].any()                          # the (-1, -1) origin is the zero padding patch
    return len(org_in), nvalid


# x0 % 4 in {0, 1, 2, 3}; 268 = 332 - 64 and 269 = 333 - 64 (x0 + S == cols exactly on one raster each, 269 is one column
# outside on the other); 136 = 200 - 64 (y0 + S == rows exactly)
EDGE_XS = (0, 1, 2, 3, 4, 133, 134, 135, 266, 267, 268, 269)
EDGE_YS = (0, 7, 135, 136)
# outside the canvas: x0 + S == cols + 1 (270 on 333 columns, 269 above on 332), y0 + S == rows + 1, negative coordinates
# other than the (-1, -1) pad, aligned and not
OUTSIDE = ((270, 0), (270, 136), (0, 137), (133, 137), (270, 137), (-3, 5), (5, -2), (-4, 8), (8, -4), (-1, 0), (0, -1),
           (-64, -64))


@pytest.mark.parametrize("cols", [333, 332])
def test_patch_stats_and_extract_unaligned(handle, cols):
    """cols % 4 == 1: every origin takes the scalar branch; cols % 4 == 0: the odd origins do, the others the float4 one."""
    S, rows = 64, 200
    d = handle(64, 16, 128)
    img, dem = synthetic_raster(rows, cols, 31, hole=(60, 90, 150, 200))
    org = np.array([(x, y) for y in EDGE_YS for x in EDGE_XS] + list(OUTSIDE), np.int32)
    assert {int(x) % 4 for x in EDGE_XS} == {0, 1, 2, 3}
    assert cols - S in EDGE_XS and cols - S + 1 in {int(x) for x in org[:, 0]} and rows - S in EDGE_YS
    n, nvalid = check_stats_and_extract(d, img, dem, org, S)
    assert n == len(EDGE_YS) * (len(EDGE_XS) - (1 if cols == 332 else 0))
    assert 0 < nvalid < n                             # from the oracle alone


@pytest.mark.parametrize("S,origins", [
    (256, ((0, 0), (1, 3), (2, 100), (3, 344), (444, 344), (441, 17), (200, 200))),
    (512, ((0, 0), (1, 3), (2, 88), (3, 50), (188, 88), (187, 1), (100, 40))),
])
def test_patch_stats_and_extract_large_patches(handle, S, origins):
    """S = 256 / 512 against the oracle; extract_patches' grid (64 blocks at most) strides 4 / 16 times over a patch."""
    d = handle(S, S // 8, 96 if S == 256 else 128)
    img, dem = synthetic_raster(600, 700, S, hole=(0, 4, 0, 4))
    org = np.array(origins, np.int32)
    assert (org[:, 0] + S).max() == 700 and (org[:, 1] + S).max() == 600 and {int(x) % 4 for x in org[:, 0]} == {0, 1, 2, 3}
    n, nvalid = check_stats_and_extract(d, img, dem, org, S)
    assert n == len(origins) and 0 < nvalid < n


# ------------------------------------------------------------------------------------------------------------------
# 3. stitcher index arithmetic
# ------------------------------------------------------------------------------------------------------------------
#   S   s   B   T   shape       hole                as_implemented
MAP_GEOMETRIES = [
    (64, 7, 5, 104, (150, 130), (40, 60, 50, 80), True),     # canvas width % 4 == 2, all four x0 % 4, T % 16 != 0, s ∤ S, s ∤ T
    (64, 7, 5, 104, (150, 130), (40, 60, 50, 80), False),
    (64, 6, 16, 62, (100, 140), (0, 8, 0, 140), True),       # x0 % 4 in {0, 2}, T % 16 != 0
    (64, 24, 4, 128, (140, 150), (60, 70, 60, 75), True),    # s ∤ S, s ∤ T
    (64, 24, 4, 128, (140, 150), (60, 70, 60, 75), False),
    (128, 10, 7, 72, (160, 150), (0, 5, 0, 150), True),      # S = 128, T < S
    (64, 48, 4, 80, (200, 170), (90, 100, 0, 30), True),     # s > S / 2: pixels that no patch covers
    (64, 4, 16, 128, (300, 300), (0, 6, 0, 6), True),        # n = 2209 per tile, valid patches in all three compaction passes
]
# The reference's accumulator is [T + 2(S - s)]^2 and its last grid line starts at s * ((T + S - 1) // s - 1): the patch there
# fits only if (T + S) % s == 0.  For other strides process_full_tiles.py raises; there is nothing to compare with.
assert all((T + S) % s == 0 for S, s, _, T, _, _, _ in MAP_GEOMETRIES)


@pytest.mark.parametrize("S,stride,B,T,shape,hole,as_impl", MAP_GEOMETRIES)
def test_identity_map_bit_exact_odd_strides(hip_lib, S, stride, B, T, shape, hole, as_impl):
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig
    assert (T + S) % stride == 0, "the reference cannot answer this geometry"
    img, dem = synthetic_raster(shape[0], shape[1], seed=S + stride, hole=hole)
    rm, rs, rg = tiler_ref.process_map(img, dem, f32_identity, S, stride, B, T, NOVAL, as_implemented=as_impl)
    assert rg.any() and not rg.all()                   # both good and no-data pixels, from the oracle alone
    d = DEMSuperResolution(DSRConfig(image_size=S, stride=stride, batch_size=B, tile_size=T), model=f32_identity,
                           as_implemented=as_impl)
    mean, std, good = d.processMap(img, dem)
    d.close()
    assert mean.shape == shape and np.array_equal(good, rg)
    # the textbook update can leave S a hair below zero, and both sides then take the root of it: NaN == NaN for std only
    for what, got, want, nan_ok in (("mean", mean, rm, False), ("std", std, rs, not as_impl)):
        if not np.array_equal(got, want, equal_nan=nan_ok):
            y, x = (int(v[0]) for v in np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want)))))
            raise AssertionError(f"{what} differs first at pixel ({y}, {x}): tile ({x // T}, {y // T}), in-tile ({x % T}, {y % T})")


@pytest.mark.parametrize("S,stride,T", [(512, 64, 128), (256, 32, 96)])
def test_rebuild_tile_large_patches_random_predictions(handle, S, stride, T):
    """rebuildTile at the production window (S = 512: purge 32, window 448; depth 7 x 7 patches per pixel) with random
    predictions and a (lo, hi) of its own per patch — constants would hide an index error.  S = 256 / s = 32 / T = 96 has
    T % 16 == 0 but T % s != 0."""
    d = handle(S, stride, T)
    rng = np.random.default_rng(S)
    n_side = len(range(0, T + S - stride, stride))
    keys = [(ix * stride, iy * stride) for iy in range(n_side) for ix in range(n_side)]
    if S == 512:
        assert len(keys) == 81
    keys = np.array([k for i, k in enumerate(keys) if i % 7 != 3], np.int32)
    n = len(keys)
    pred = rng.random((n, S, S), dtype=np.float32) - np.float32(0.5)
    lo = rng.uniform(-3000, -2000, n).astype(np.float32)
    mm = np.stack([lo, lo + rng.uniform(5, 400, n).astype(np.float32)], axis=1)
    assert len({(float(a), float(b)) for a, b in mm}) == n
    gen = {tuple(int(v) for v in k): p + np.float32(0.5) for k, p in zip(keys, pred)}
    mmd = {tuple(int(v) for v in k): (m[0], m[1]) for k, m in zip(keys, mm)}
    t_pred, t_keys, t_mm = torch.from_numpy(pred).cuda(), torch.from_numpy(keys).cuda(), torch.from_numpy(mm).cuda()
    was = d.as_implemented
    try:
        for as_impl in (True, False):
            rm, rs, rg = tiler_ref.rebuild_tile(gen, mmd, T, S, stride, NOVAL, as_implemented=as_impl)
            d.as_implemented = as_impl
            mean, std, good = (t.cpu().numpy() for t in d.rebuildTile(t_pred, t_keys, t_mm))
            assert rg.all()                            # every pixel keeps enough of its 7 x 7 patches
            assert np.array_equal(good, rg), as_impl
            assert np.array_equal(mean, rm), as_impl
            assert np.array_equal(std, rs), as_impl
    finally:
        d.as_implemented = was


def test_halo_mode_band_wider_than_1024_candidates(hip_lib):
    """One band of the halo mode with more than 1024 candidate origins: the compaction's later passes as production runs them
    (about 1110 origins per patch row on the 70000-wide raster)."""
    from moonsuperresolution_amd import DSRConfig, HaloShardedSuperResolution
    S, stride, B, T = 64, 8, 16, 64
    img, dem = synthetic_raster(150, 330, seed=S + stride, hole=(30, 50, 100, 130))
    d = HaloShardedSuperResolution(DSRConfig(image_size=S, stride=stride, batch_size=B, tile_size=T), model=f32_identity)
    d.setImages(img, dem)
    d.padInputs()
    ys, xs = d.patchGrid()
    assert (len(ys), len(xs)) == (31, 55) and len(ys) * len(xs) == 1705
    ref = {w: tiler_ref.process_map_halo(img, dem, f32_identity, S, stride, B, T, NOVAL, world=w) for w in (1, 2)}
    assert ref[1][2].any() and not ref[1][2].all()
    for world, band_rows in ((1, None), (2, None), (1, 20)):
        if world == 1:
            assert (len(ys) if band_rows is None else band_rows) * len(xs) > 1024
        got = run_halo(d, img, dem, world, band_rows=band_rows)
        if band_rows is None:
            assert d.last_band_rows >= len(ys)         # the whole rank in one band
        for what, a, b in zip(("mean", "std", "good"), got, ref[world]):
            assert np.array_equal(a, b, equal_nan=True), (world, band_rows, what)
    d.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. msr_halo_merge, direct
# ------------------------------------------------------------------------------------------------------------------
def run_merge(d, a, b):
    """a, b: triples of float32 host vectors (w, mean, S), b may be None -> (mean, std, good) host arrays."""
    n = len(a[0])
    ta = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for v in a]
    tb = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for v in b] if b is not None else None
    mean, std, good = sentinel(n, torch.float32), sentinel(n, torch.float32), sentinel(n, torch.uint8)
    pb = [t.data_ptr() for t in tb] if tb is not None else [None, None, None]
    rc = d._lib.msr_halo_merge(d._h, *(t.data_ptr() for t in ta), *pb, n, NOVAL, mean.data_ptr(), std.data_ptr(),
                               good.data_ptr(), None)
    assert rc == 0
    return mean.cpu().numpy(), std.cpu().numpy(), good.cpu().numpy()


def merge_ref(a, b):
    with np.errstate(over="ignore"):                   # a float64 sum that leaves float32's range becomes inf on both sides
        return tiler_ref.halo_finalize(tiler_ref.chan_merge(a, b) if b is not None else a, NOVAL)


def assert_merge_equal(got, want, tag):
    for what, g, w in zip(("mean", "std", "good"), got, want):
        assert g.dtype == w.dtype, (tag, what)
        if not np.array_equal(g, w, equal_nan=True):
            bad = np.flatnonzero(~((g == w) | ((g != g) & (w != w))))
            raise AssertionError(f"{tag}: {what} differs at {len(bad)} elements, first {int(bad[0])} "
                                 f"(grid-stride trip {int(bad[0]) // (8192 * 256)}): got {g[bad[0]]!r}, want {w[bad[0]]!r}")


def test_halo_merge_grid_stride_loop(handle):
    """n > 8192 * 256: the kernel's grid is capped there, so the loop turns a second, partial time."""
    d = handle(64, 16, 128)
    n = 8192 * 256 + 12345
    rng = np.random.default_rng(4)

    def triple():
        w = rng.uniform(0.01, 5.0, n).astype(np.float32)
        w[rng.random(n) < 0.25] = 0.0                  # independent quarters: both are zero in about a sixteenth
        return w, (-2000 + 600 * rng.standard_normal(n)).astype(np.float32), rng.uniform(0, 100, n).astype(np.float32)

    a, b = triple(), triple()
    both = (a[0] == 0) & (b[0] == 0)
    assert 0.05 < both.mean() < 0.075 and 0.24 < (a[0] == 0).mean() < 0.26 and 0.24 < (b[0] == 0).mean() < 0.26
    assert_merge_equal(run_merge(d, a, b), merge_ref(a, b), "a with b")
    assert_merge_equal(run_merge(d, a, None), merge_ref(a, None), "a alone")


# (wa, ma, Sa, wb, mb, Sb), by hand.  DENORMAL is a float32 subnormal.
DENORMAL = 1e-40
MERGE_ROWS = [
    # wa == 0, wb > 0: b alone
    (0.0, 0.0, 0.0, 1.5, -2100.25, 3.0),
    (0.0, 123.0, 77.0, 0.25, -1999.5, 0.5),            # what a holds is ignored
    (0.0, -5.0, 9.0, 1e-7, 12.0, 0.0),
    (0.0, 0.0, 0.0, 4.0, -2500.0, 1e-3),
    # wa > 0, wb == 0: a alone
    (2.0, -2050.5, 6.0, 0.0, 0.0, 0.0),
    (0.75, -1800.125, 0.25, 0.0, 55.0, 66.0),          # what b holds is ignored
    (1e-7, 3.0, 0.0, 0.0, 0.0, 0.0),
    (3.5, -2999.0, 40.0, 0.0, -1.0, -1.0),
    # both zero: no_value, no_value, good == 0 (rows 8..11)
    (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    (0.0, -2000.0, 5.0, 0.0, -2100.0, 6.0),
    (0.0, 1.0, -1.0, 0.0, 2.0, -2.0),
    (0.0, float("nan"), float("nan"), 0.0, float("nan"), float("nan")),
    # S a hair below zero from float32 rounding: std exactly 0 (rows 12..15)
    (1.0, -2000.0, -1e-9, 0.0, 0.0, 0.0),
    (1.0, -2000.0, -1e-9, 2.0, -2000.0, 0.0),          # d == 0: Sa + Sb + 0 stays negative
    (0.0, 0.0, 0.0, 1.0, 7.0, -3e-8),
    (0.5, 10.0, -2e-8, 0.5, 10.0, -1e-8),
    # NaN in Sa: std NaN, mean finite (rows 16..18)
    (1.0, -2000.0, float("nan"), 0.0, 0.0, 0.0),
    (1.0, -2000.0, float("nan"), 1.0, -2010.0, 2.0),
    (2.5, 4.0, float("nan"), 0.5, 5.0, 0.0),
    # wb denormal (rows 19..22)
    (1.0, -2000.0, 4.0, DENORMAL, -2100.0, 1.0),
    (0.0, 0.0, 0.0, DENORMAL, -2100.0, 1e-42),
    (DENORMAL, -1900.0, 2e-41, DENORMAL, -2100.0, 1e-41),
    (3.0, 1.0, 0.0, 1.4e-45, 2.0, 0.0),
    # ordinary two-sided rows
    (1.0, -2000.0, 4.0, 1.0, -2010.0, 2.0),
    (2.0, -2000.0, 4.0, 1.0, -1990.0, 2.0),
    (0.125, 100.0, 0.0, 8.0, -100.0, 0.0),
    (5.0, -2345.678, 12.5, 0.001, -2345.0, 0.0),
    (1.0, 1e30, 0.0, 1.0, -1e30, 0.0),                 # d * d overflows float32, not float64
    (1.0, 0.0, 0.0, 1.0, 0.0, 0.0),
    (3.0, -0.0, 0.0, 1.0, 0.0, 0.0),
    (1e-3, -2000.5, 1e-6, 1e3, -2000.25, 1e2),
    (7.0, -2222.0, 70.0, 7.0, -2222.0, 70.0),
]
BOTH_ZERO, NEGATIVE_S, NAN_S = range(8, 12), range(12, 16), range(16, 19)


def test_halo_merge_hand_built_vector(handle):
    d = handle(64, 16, 128)
    rows = MERGE_ROWS + [(wb, mb, sb, wa, ma, sa) for wa, ma, sa, wb, mb, sb in MERGE_ROWS]    # and with a and b swapped
    assert len(rows) == 64
    cols = [np.array(c, np.float32) for c in zip(*rows)]
    a, b = tuple(cols[:3]), tuple(cols[3:])
    assert 0 < float(np.float32(DENORMAL)) < float(np.finfo(np.float32).tiny)
    with_b = run_merge(d, a, b)
    alone = run_merge(d, a, None)
    assert_merge_equal(with_b, merge_ref(a, b), "a with b")
    assert_merge_equal(alone, merge_ref(a, None), "a alone")
    # the expectations that do not rest on the oracle
    for mean, std, good in (with_b, alone):
        for i in BOTH_ZERO:
            assert mean[i] == np.float32(NOVAL) and std[i] == np.float32(NOVAL) and good[i] == 0, i
    mean, std, good = with_b
    for i in NEGATIVE_S:
        assert good[i] == 1 and std[i] == 0.0 and np.isfinite(mean[i]), i
    for i in NAN_S:
        assert good[i] == 1 and np.isnan(std[i]) and np.isfinite(mean[i]), i
    mean, std, good = alone
    assert good[12] == 1 and std[12] == 0.0 and good[16] == 1 and np.isnan(std[16]) and np.isfinite(mean[16])
    # one-sided weights give the other side's figures exactly
    mean, std, good = with_b
    assert mean[0] == np.float32(-2100.25) and std[0] == np.sqrt(np.float32(3.0) / np.float32(1.5)) and good[0] == 1
    assert mean[4] == np.float32(-2050.5) and std[4] == np.sqrt(np.float32(6.0) / np.float32(2.0)) and good[4] == 1

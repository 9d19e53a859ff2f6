"""Shapes, line arithmetic and row-restricted references of tests/test_gpu_far_offsets.py.  Nothing here needs a GPU:
tests/test_far_offsets_host.py pins the restricted references against the whole-raster oracles at small shapes, bit for bit,
and checks the lines and the device-memory budget of every case from its shapes.

Two lines: L31 = 2^31 and L32 = 2^32 BYTES from the start of a buffer.  A "far raster" for a line is the smallest rows x cols
whose last TAIL rows lie wholly past it; only those rows (a "tail window", tens of MB) ever exist on the host.
"""
import numpy as np

from moonsuperresolution_amd import infill as I
from oracle import preprocess_ref as pr
from oracle import tiler_ref

F32 = np.float32
L31, L32 = 1 << 31, 1 << 32
LINES = {"L31": L31, "L32": L32}
COLS = (70000, 70001)          # 70000: vec4 in the area resize, float4 in patch stats; 70001: the unaligned paths
TAIL = 128
INT32_MAX = 2 ** 31 - 1
GIB = 1 << 30
BUDGET = 20 * GIB              # no test may hold more device memory than this at once
NOVAL = -32768.0
CANVAS = (16256, 71552)        # the padded canvas of BASELINE configs[3] (15000 x 70000, S = 512, s = 64, T = 1024)
RASTER = (15000, 70000)
NODATA_TO_NAN, NAN_TO_NODATA = 1, 2


# ---- line arithmetic ---------------------------------------------------------------------------------------------------------
def offset(row, cols, itemsize=4, col=0):
    """Byte offset of element (row, col) of a row-major rows x cols array."""
    return (row * cols + col) * itemsize


def first_row_past(line, cols, itemsize=4):
    """The first row that lies wholly at or past ``line`` bytes."""
    return -(-line // (cols * itemsize))


def far_rows(line, cols, itemsize=4, tail=TAIL, modulus=1, residue=0):
    """Rows of the far raster of ``line``: the smallest count (with rows % modulus == residue) whose last ``tail`` rows lie
    wholly past the line."""
    rows = first_row_past(line, cols, itemsize) + tail
    while rows % modulus != residue:
        rows += 1
    return rows


def rows_past(line, row0, cols, itemsize=4):
    """True iff every byte of the rows from ``row0`` on lies at or past ``line``."""
    return offset(row0, cols, itemsize) >= line


def area_shape(line, cols):
    """Far source of the area resize (factor 4).  70001 columns: rows % 8 == 6, so that rows % 4 == 2 AND cvRound(rows / 4)
    rounds the half up (rows // 4 is odd): the destination has a last row whose block holds two source rows.  70000 columns:
    rows % 4 == 0, whole blocks through the float4 path."""
    return (far_rows(line, cols, modulus=8, residue=6) if cols % 4 else far_rows(line, cols, modulus=4, residue=0)), cols


def largest_rows(cols):
    """The largest row count a 32-bit element index accepts: floor(INT32_MAX / cols)."""
    return INT32_MAX // cols


def infill_workspace_bytes(n_rows, cols):
    """include/moonsr.h: 16 + 8 n_rows ceil(cols / 64) + 4 ceil(n_rows / 2) ceil(cols / 2)."""
    return 16 + 8 * n_rows * -(-cols // 64) + 4 * -(-n_rows // 2) * -(-cols // 2)


# ---- the tables of the GPU cases (tests/test_gpu_far_offsets.py takes its parameters from here) --------------------------------
AREA_CASES = [(name, cols) for name in LINES for cols in COLS]
AREA_ROWS_CASES = [("L32", cols, flags) for cols in COLS for flags in (0, NODATA_TO_NAN | NAN_TO_NODATA)]
CUBIC_CASES = [(name, cols) for name in LINES for cols in COLS]
CUBIC_SHRINK = 16                                          # the small side of the cubic cases is 1 / 16 of the far one
INFILL_GRIDS = {"L32": lambda: (far_rows(L32, 70001, tail=160), 70001), "largest": lambda: (largest_rows(70001), 70001)}
INFILL_WINDOW = 160                                        # rows of the head and tail windows the twin runs on
INFILL_MAX_AREA, INFILL_MARGIN = 24, 32                    # preprocess's setting on the x1/4 grid
OVERVIEW_CASES = {                                         # name -> (dtype, rows, cols, has_nodata)
    "f32-odd": ("<f4", far_rows(L32, 70001, modulus=2, residue=1), 70001, 0),
    "f32-odd-nodata": ("<f4", far_rows(L32, 70001, modulus=2, residue=1), 70001, 1),
    "f32-even-nodata": ("<f4", far_rows(L32, 70000, modulus=2, residue=0), 70000, 1),
    "u16-L31": ("<u2", far_rows(L31, 70001, itemsize=2, modulus=2, residue=1), 70001, 0),
    "u8-largest": ("|u1", largest_rows(70001), 70001, 0),
}
STITCH_PITCH = CANVAS[1]
STITCH_ROWS = far_rows(L32, STITCH_PITCH)                  # rows of each of the three accumulator slabs
MERGE_COUNT = (1 << 30) + 4099
MERGE_CHUNK = 1 << 20
BLOCK_KINDS = [("u", 1), ("i", 2), ("u", 2), ("i", 4), ("f", 4)]
BLOCK_COLS = 70001
BLOCK_SRC_BYTES = L32 + (1 << 24)
LZW_BYTES = L32 + (1 << 20)
CHECK_CHUNK = 1 << 27          # elements a whole-array check on the device compares at a time (a 128 MB bool image)


def merge_chunks(count=MERGE_COUNT, chunk=MERGE_CHUNK, itemsize=4):
    """Element ranges of msr_halo_merge that are compared: the first chunk, one chunk straddling each line, the tail."""
    out = [(0, chunk)]
    for line in (L31, L32):
        e = line // itemsize
        if e < count:
            out.append((e - chunk // 2, min(e + chunk // 2, count)))
    out.append((count - chunk - 4099, count))
    return out


def budgets():
    """Device bytes every GPU case holds at its peak, from its shapes: name -> bytes (tensors of the test, the kernel's
    workspace, and the chunk a device-side whole-array check compares at a time)."""
    out = {}
    for name, cols in AREA_CASES:
        r, c = area_shape(LINES[name], cols)
        out[f"area-{name}-{cols}"] = 4 * r * c + 4 * pr.cv_round(r / 4) * pr.cv_round(c / 4)
    for name, cols, flags in AREA_ROWS_CASES:
        r, c = area_shape(LINES[name], cols)
        out[f"area_rows-{name}-{cols}-{flags}"] = 4 * r * c + 4 * pr.cv_round(r / 4) * pr.cv_round(c / 4)
    for name, cols in CUBIC_CASES:
        r = far_rows(LINES[name], cols)
        small = 4 * -(-r // CUBIC_SHRINK) * -(-cols // CUBIC_SHRINK)
        out[f"cubic_up-{name}-{cols}"] = 4 * r * cols + small + CHECK_CHUNK
        out[f"cubic_down-{name}-{cols}"] = 4 * r * cols + small
    for name, shape in INFILL_GRIDS.items():
        r, c = shape()
        out[f"infill-{name}"] = 4 * r * c + infill_workspace_bytes(r, c) + CHECK_CHUNK
    for name, (dt, r, c, _) in OVERVIEW_CASES.items():
        size = np.dtype(dt).itemsize
        out[f"overview-{name}"] = size * (r * c + -(-r // 2) * -(-c // 2))
    out["patches"] = 2 * 4 * CANVAS[0] * CANVAS[1] + 8 * 4 * 1024 * CANVAS[1]        # two canvases and a 1024-row chunk's temporaries
    out["stitch_band"] = 3 * 4 * STITCH_ROWS * STITCH_PITCH + CHECK_CHUNK
    out["halo_merge"] = (2 * 4 + 2 * 4 + 1) * MERGE_COUNT + 16 * 8 * (MERGE_CHUNK + 4099)
    out["blocks_to_f32"] = BLOCK_SRC_BYTES + 4 * far_rows(L32, BLOCK_COLS) * BLOCK_COLS + CHECK_CHUNK
    out["lzw_strips"] = 2 * LZW_BYTES
    out["band_grid_largest"] = 4 * INT32_MAX + CHECK_CHUNK     # the int32 grid workspace
    return out


# ---- row-restricted references -------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    """Same shape, NaNs in the same places, every other value the same bits."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.nan_to_num(a).view(np.uint32), np.nan_to_num(b).view(np.uint32))


def area_rows_ref(window, s0, full_rows, factor, d0, d1, no_value=NOVAL, flags=0):
    """Rows [d0, d1) of oracle/preprocess_ref.py::resize_area of a full_rows-row raster, from ``window`` = its source rows
    [factor * d0, min(factor * d1, full_rows)).  The window is cropped at a multiple of the factor and its true last rows are
    kept, so a partial bottom block stays partial: the whole blocks go through the oracle as they are; the rows of a partial
    block go through it below ONE block of zeros, which keeps cvRound at two rows ((factor + k) / factor rounds to 2 exactly
    when full_rows / factor rounds up), and the zeros' row is dropped.  flags: MSR_RESIZE_* of include/moonsr.h."""
    window = np.array(window, F32, copy=True)
    assert s0 == factor * d0 and s0 + len(window) == min(factor * d1, full_rows) and d0 < d1 <= pr.cv_round(full_rows / factor)
    if flags & NODATA_TO_NAN:
        window[window <= F32(no_value)] = np.nan
    f = 1.0 / factor
    n_full = min(d1, full_rows // factor) - d0
    parts = []
    if n_full > 0:
        parts.append(pr.resize_area(window[:n_full * factor], f, f))
        assert parts[0].shape[0] == n_full
    if d0 + max(n_full, 0) < d1:
        rest = window[max(n_full, 0) * factor:]
        assert d1 - d0 - max(n_full, 0) == 1 and 0 < len(rest) < factor
        two = pr.resize_area(np.concatenate([np.zeros((factor, window.shape[1]), F32), rest]), f, f)
        assert two.shape[0] == 2
        parts.append(two[1:])
    out = np.concatenate(parts)
    if flags & NAN_TO_NODATA:
        out[np.isnan(out)] = F32(no_value)
    return out


def cubic_tap_rows(r0, r1, full_src_rows, full_dst_rows):
    """Source rows [lo, hi) that destination rows [r0, r1) of the cubic resize tap (the oracle's clamped indices)."""
    idx, _ = pr._cubic_axis(full_src_rows, full_dst_rows)
    return int(idx[r0:r1].min()), int(idx[r0:r1].max()) + 1


def cubic_rows_ref(window, s0, full_src_rows, full_dst_rows, dst_cols, r0, r1, no_value=NOVAL, flags=0):
    """Rows [r0, r1) of oracle/preprocess_ref.py::resize_cubic of a full_src_rows-row raster resized to
    full_dst_rows x dst_cols, from ``window`` = its source rows [s0, s0 + len(window)), which must hold every tapped row: the
    vertical taps and weights come from the FULL sizes (pr._cubic_axis, pr.cubic_coeffs) and only the tap index is rebased;
    the two passes are the oracle's expressions."""
    window = np.array(window, F32, copy=True)
    if flags & NODATA_TO_NAN:
        window[window <= F32(no_value)] = np.nan
    yi, yb = pr._cubic_axis(full_src_rows, full_dst_rows)
    yi, yb = yi[r0:r1] - s0, yb[r0:r1]
    assert yi.min() >= 0 and yi.max() < len(window), "the window lacks a tapped row"
    xi, xa = pr._cubic_axis(window.shape[1], dst_cols)
    rows = (((window[:, xi[:, 0]] * xa[:, 0]) + window[:, xi[:, 1]] * xa[:, 1]) + window[:, xi[:, 2]] * xa[:, 2]) \
        + window[:, xi[:, 3]] * xa[:, 3]
    rows = rows.astype(F32)
    out = (((rows[yi[:, 0]] * yb[:, 0:1]) + rows[yi[:, 1]] * yb[:, 1:2]) + rows[yi[:, 2]] * yb[:, 2:3]) \
        + rows[yi[:, 3]] * yb[:, 3:4]
    out = out.astype(F32)
    if flags & NAN_TO_NODATA:
        out[np.isnan(out)] = F32(no_value)
    return out


def overview_tail_start(rows, tail=TAIL):
    """The first row of the tail window of an overview case: rows - tail rounded UP to an even row (a 2 x 2 block starts there)."""
    return rows - tail + (rows - tail) % 2


def overview_tail_ref(tail, nodata=None):
    """The last rows of geotiff.overview_reference of a raster whose rows from an EVEN row on are ``tail``."""
    from moonsuperresolution_amd import geotiff as G
    return G.overview_reference(tail, nodata)


# ---- in-fill -----------------------------------------------------------------------------------------------------------------
def component_shape(n):
    """n pixels, row-major, in rows 1 + n % 6 wide; odd rows start one column to the right, so the one-pixel-wide shapes are
    zigzags that only 8-connectivity holds together.  At most 31 rows and 7 columns."""
    w = 1 + n % 6
    return [(i // w, (i // w) % 2 + i % w) for i in range(n)]


def plant(window, top, left, pixels, no_value=NOVAL):
    for dr, dc in pixels:
        window[top + dr, left + dc] = no_value


def infill_window(kind, full_rows, cols, seed, rows=INFILL_WINDOW, max_area=INFILL_MAX_AREA, margin=INFILL_MARGIN):
    """The first (kind "head") or last (kind "tail") ``rows`` rows of a full_rows x cols grid that is valid everywhere else:
    (window, row0, planted) with ``planted`` = {name: [(row, col) in the window]}.  Holes: one component of every size 1 .. 31
    (those of max_area pixels and more stay), components ending on the last fillable row (tail) or starting on the first
    (head), one that crosses that row (only its pixels inside the fill set are written), two components one valid pixel apart,
    a component in the last fillable columns and one that crosses the last fillable column.  No hole lies within max_area
    rows of the window's cut edge, so the twin on the window fills what the whole grid's in-fill does."""
    assert rows >= 2 * margin + 80 and full_rows >= 2 * rows and cols >= 3400
    rng = np.random.default_rng(seed)
    yy = np.arange(rows, dtype=F32)[:, None]
    xx = np.arange(cols, dtype=F32)[None, :]
    win = (-2000.0 + 40.0 * np.sin(xx / 37.0) * np.cos(yy / 11.0) + rng.normal(0, 3.0, (rows, cols))).astype(F32)
    row0 = 0 if kind == "head" else full_rows - rows
    # rows of the window inside the fill set: [lo, hi); the cut edge is the other end
    lo, hi = (margin, rows - max_area) if kind == "head" else (max_area, rows - margin)
    edge = lo if kind == "head" else hi - 1               # the first / last fillable row of the whole grid
    planted = {}

    def put(name, top, left, pixels):
        plant(win, top, left, pixels)
        planted[name] = [(top + dr, left + dc) for dr, dc in pixels]

    band = lo + 8 if kind == "head" else lo + 16
    for n in range(1, 32):                                 # every size, 40 columns apart
        put(f"size{n}", band, margin + 8 + 40 * (n - 1), component_shape(n))
    for n in range(1, 13):                                 # against the edge of the fill set, from inside
        shape = component_shape(n)
        height = 1 + max(r for r, _ in shape)
        put(f"edge{n}", edge if kind == "head" else edge - height + 1, 2000 + 40 * n, shape)
    put("crossing", edge - 2, 3000, [(i, 0) for i in range(4)])          # rows edge - 2 .. edge + 1: part of it is outside the fill set
    apart_row = band + 40
    put("apart-a", apart_row, 3100, [(0, 0), (1, 0)])
    put("apart-b", apart_row, 3102, [(0, 0), (1, 0)])
    put("right", apart_row, cols - margin - 8, component_shape(5))       # in the last fillable columns
    put("right-crossing", apart_row + 10, cols - margin - 3, [(0, i) for i in range(4)])    # columns cols - 35 .. cols - 32
    holes = ~(win > F32(NOVAL))
    cut = slice(rows - max_area, rows) if kind == "head" else slice(0, max_area)
    assert not holes[cut].any() and int(holes.sum()) == sum(len(p) for p in planted.values())
    return win, row0, planted


def infill_window_ref(win, row0, full_rows, max_area=INFILL_MAX_AREA, margin=INFILL_MARGIN):
    """The twin on the window, with its row0 / full_rows semantics."""
    return I.infill_reference(win, NOVAL, max_area, margin, row0=row0, full_rows=full_rows)


# ---- stitch band ---------------------------------------------------------------------------------------------------------------
def f32_identity(x, training=False):
    return np.asarray(x, F32)


def band_reference(S, stride, nx, ny, seed, batch=4):
    """An nx x ny band of patches on its own small canvas, accumulated by the oracle (tiler_ref.halo_partials with the float32
    identity model): (pred [n, S, S], key [n, 2] canvas origins (x, y), dmm [n, 2], (w_sum, mean, S) of the canvas), patches
    in generation order.  pred is what the identity model returns for each patch (its normalised DEM channel), so feeding
    (pred, key, dmm) to msr_stitch_accumulate_band repeats the oracle's updates; they do not depend on where the canvas lies."""
    hp, wp = (ny - 1) * stride + S, (nx - 1) * stride + S
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.1, 0.9, (hp, wp)).astype(F32)
    dem = (-2000.0 + 300.0 * rng.standard_normal((hp, wp))).astype(F32)
    ys, xs = [j * stride for j in range(ny)], [i * stride for i in range(nx)]
    acc = tiler_ref.halo_partials(img, dem, ys, xs, f32_identity, S, stride, batch, NOVAL)
    pred, key, dmm = [], [], []
    for y in ys:
        for x in xs:
            ok, ip, dp = tiler_ref.get_patch(img, dem, x, y, S, NOVAL)
            assert ok
            patch, mm = tiler_ref.normalize(ip, dp)
            pred.append(np.asarray(patch[..., 1], F32))
            key.append((x, y))
            dmm.append(mm)
    return np.stack(pred), np.array(key, np.int32), np.array(dmm, F32), acc


# ---- TIFF blocks and strips ----------------------------------------------------------------------------------------------------
def tiff_block(kind, sb, bw, bh, predictor, rng):
    """One decoded TIFF block as msr_tiff_blocks_to_f32 reads it: (raw bytes [bh * bw * sb] uint8, its float32 values
    [bh, bw]) — NumPy's cumsum on the unsigned view for predictor 2, then the sample type's conversion to float32."""
    dt, ut = np.dtype(f"<{kind}{sb}"), np.dtype(f"<u{sb}")
    want = rng.integers(0, 1 << (8 * sb), (bh, bw), dtype=np.uint64).astype(ut)
    if kind == "f":
        f = (-2000 + 300 * rng.standard_normal((bh, bw))).astype(F32)
        f[0, 0] = np.nan
        want = f.view(np.uint32).copy()
        want[bh - 1, bw - 1] = 0x7FC12345                  # a NaN with a payload
    raw = want.copy()
    if predictor == 2:
        raw[:, 1:] = want[:, 1:] - want[:, :-1]
    u = np.cumsum(raw, axis=1, dtype=ut) if predictor == 2 else raw
    val = u.view(dt)
    return raw.view(np.uint8).reshape(-1).copy(), (val if kind == "f" else val.astype(F32))


def predict(data, sample_bytes, row_bytes):
    """The TIFF horizontal predictor (PREDICTOR=2) on the bytes of whole rows; sample_bytes 0: the bytes as they are."""
    data = np.ascontiguousarray(data, np.uint8)
    if not sample_bytes:
        return data
    u = data.view(np.dtype(f"<u{sample_bytes}")).reshape(-1, row_bytes // sample_bytes)
    d = u.copy()
    d[:, 1:] = u[:, 1:] - u[:, :-1]
    return d.view(np.uint8).reshape(-1)


def line_offsets(length, odd=True):
    """Byte offsets of slots of ``length`` bytes just below, across and above each line (odd ones included)."""
    out = []
    for line in (L31, L32):
        out += [line - 3 * length - 1, line - length // 2 - (1 if odd else 0), line + length + 1]
    return out

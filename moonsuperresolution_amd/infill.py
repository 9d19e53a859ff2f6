"""In-filling of small no-data holes on the device (``preprocess(infill="device")``) and its NumPy twin.

The host path (preprocess.fillNan) runs ``scipy.interpolate.griddata(method="cubic")`` on every tile that holds a hole.
The device path fills THE SAME PIXELS with other values: per hole component, the least-squares solution of "5-point
Laplacian = 0 at every pixel of the component and of its 4-neighbour ring" (a discrete thin-plate fill of at most 31
unknowns).  ``fill_set`` is the tile-free rule for which pixels fillNan changes, ``infill_reference`` the twin that
defines the values (Python loops in float64, in the order csrc/infill_solve.h states; the kernels equal it bit for bit),
``infill_device`` the call of ``msr_infill_small_holes`` (include/moonsr.h holds the contract).

Deviations from the host path, all stated: other values at the same pixels; fillNan's label-0 quirk (the valid area takes
part in its "smallest region too large" test, so a tile with fewer than max_area VALID pixels is treated differently) is not
reproduced; no NaN is ever written (griddata gives NaN outside the convex hull of a tile's valid pixels); a NaN input counts
as a hole.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

from . import _lib

MAX_AREA_LIMIT = 32        # INFILL_MAX_AREA of csrc/infill_solve.h
_STENCIL = ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0))      # N, W, centre, E, S: row-major


def _check(grid: np.ndarray, row0: int, full_rows: Optional[int], max_area: int, margin: int) -> Tuple[int, int]:
    if grid.ndim != 2 or grid.dtype != np.float32:
        raise ValueError("the grid must be a 2-D float32 array")
    full_rows = grid.shape[0] if full_rows is None else int(full_rows)
    if not 2 <= max_area <= MAX_AREA_LIMIT:
        raise ValueError(f"max_area {max_area} outside [2, {MAX_AREA_LIMIT}]")
    if margin < max_area + 1:
        raise ValueError(f"margin {margin} < max_area + 1 = {max_area + 1}")
    if row0 < 0 or row0 + grid.shape[0] > full_rows:
        raise ValueError(f"rows [{row0}, {row0 + grid.shape[0]}) are not rows of a grid of {full_rows}")
    return int(row0), full_rows


def _labels(grid: np.ndarray, no_value: float):
    from scipy import ndimage
    holes = ~(grid > np.float32(no_value))
    labels, count = ndimage.label(holes, structure=np.ones((3, 3), dtype=bool))
    return holes, labels, count


def fill_set(grid: np.ndarray, no_value: float, max_area: int, margin: int, row0: int = 0,
             full_rows: Optional[int] = None) -> np.ndarray:
    """The pixels the in-fill writes (bool mask): holes (``!(G > no_value)``) whose 8-connected component has fewer than
    ``max_area`` pixels, at least ``margin`` pixels from every edge of the whole grid and, in a row window (``grid`` = rows
    [row0, row0 + len(grid)) of ``full_rows``), at least ``max_area`` rows from a cut edge.  For the whole grid this is the
    set of pixels ``preprocess.fillNan(grid, no_value, tile, margin, max_area)`` changes (tile - 2 * margin > 0)."""
    row0, full_rows = _check(grid, row0, full_rows, max_area, margin)
    n, w = grid.shape
    holes, labels, _ = _labels(grid, no_value)
    small = (np.bincount(labels.ravel()) < max_area)[labels] & holes
    rows = np.arange(n)[:, None]
    cols = np.arange(w)[None, :]
    inside = (rows + row0 >= margin) & (rows + row0 < full_rows - margin) & (cols >= margin) & (cols < w - margin)
    if row0 > 0:
        inside = inside & (rows >= max_area)
    if row0 + n < full_rows:
        inside = inside & (rows < n - max_area)
    return small & inside


def solve_component(grid: np.ndarray, no_value: float, pix_r, pix_c) -> list:
    """The float64 fill values of one component (its pixels in row-major order), by the loops of csrc/infill_solve.h."""
    n_rows, n_cols = grid.shape
    nv = np.float32(no_value)
    index = {(int(r), int(c)): i for i, (r, c) in enumerate(zip(pix_r, pix_c))}
    n = len(index)

    def centre(r, c):
        s = 0.0
        for t, (dr, dc) in enumerate(_STENCIL):
            rr, cc = r + dr, c + dc
            if not (0 <= rr < n_rows and 0 <= cc < n_cols):
                return None
            if not grid[rr, cc] > nv:
                if (rr, cc) not in index:
                    return None
                continue
            s += (-4.0 if t == 2 else 1.0) * float(grid[rr, cc])
        return -s

    N = [[0.0] * n for _ in range(n)]
    b = [0.0] * n
    for (r, c), i in index.items():
        acc = 0.0
        for t, (dr, dc) in enumerate(_STENCIL):
            q = (r + dr, c + dc)
            d = centre(*q)
            if d is None:
                continue
            wi = -4.0 if t == 2 else 1.0
            acc += wi * d
            for u, (er, ec) in enumerate(_STENCIL):
                j = index.get((q[0] + er, q[1] + ec))
                if j is not None and j <= i:
                    N[i][j] += wi * (-4.0 if u == 2 else 1.0)
        b[i] = acc
    L = N
    diag = [0.0] * n
    for j in range(n):
        for i in range(j, n):
            s = L[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            if i == j:
                diag[j] = math.sqrt(s)
            else:
                L[i][j] = s / diag[j]
    for i in range(n):
        s = b[i]
        for k in range(i):
            s -= L[i][k] * b[k]
        b[i] = s / diag[i]
    for i in range(n - 1, -1, -1):
        s = b[i]
        for k in range(i + 1, n):
            s -= L[k][i] * b[k]
        b[i] = s / diag[i]
    return b


def components(grid: np.ndarray, no_value: float, max_area: int, margin: int, row0: int = 0,
               full_rows: Optional[int] = None):
    """(pix_r, pix_c, in_fill_set) of every component that meets the fill set, pixels in row-major order."""
    from scipy import ndimage
    take = fill_set(grid, no_value, max_area, margin, row0, full_rows)
    _, labels, _ = _labels(grid, no_value)
    out = []
    boxes = ndimage.find_objects(labels)
    for k in np.unique(labels[take]):
        box = boxes[k - 1]
        rr, cc = np.nonzero(labels[box] == k)              # row-major
        rr, cc = rr + box[0].start, cc + box[1].start
        out.append((rr, cc, take[rr, cc]))
    return out


def infill_reference(grid: np.ndarray, no_value: float, max_area: int, margin: int, row0: int = 0,
                     full_rows: Optional[int] = None) -> np.ndarray:
    """The twin of msr_infill_small_holes: a filled copy of ``grid`` (rows [row0, row0 + len(grid)) of a grid of
    ``full_rows``).  Every pixel outside ``fill_set`` keeps its bits."""
    out = grid.copy()
    for rr, cc, keep in components(grid, no_value, max_area, margin, row0, full_rows):
        x = solve_component(grid, no_value, rr, cc)
        vals = np.array(x, dtype=np.float64).astype(np.float32)
        out[rr[keep], cc[keep]] = vals[keep]
    return out


def infill_device(lib, handle, grid, row0: int, full_rows: int, no_value: float, max_area: int, margin: int) -> None:
    """msr_infill_small_holes in place on ``grid``, a contiguous 2-D float32 CUDA tensor holding rows
    [row0, row0 + len(grid)) of a grid of ``full_rows``; on the tensor's device and its current stream."""
    import torch
    if grid.dim() != 2 or grid.dtype != torch.float32 or not grid.is_cuda or not grid.is_contiguous():
        raise ValueError("infill_device expects a contiguous 2-D float32 CUDA tensor")
    n, w = grid.shape
    need = lib.msr_infill_workspace_bytes(n, w)
    if need < 0:
        raise ValueError(f"a window of {n} x {w} pixels is empty or exceeds 2^31 - 1 pixels: use row windows")
    with torch.cuda.device(grid.device):
        workspace = torch.empty(need, dtype=torch.uint8, device=grid.device)
        rc = lib.msr_infill_small_holes(handle, grid.data_ptr(), int(row0), n, int(full_rows), w, float(no_value),
                                        int(max_area), int(margin), workspace.data_ptr(), need,
                                        torch.cuda.current_stream(grid.device).cuda_stream)
    _lib.raise_for(lib, handle, rc, "msr_infill_small_holes")

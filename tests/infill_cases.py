"""Grids with no-data holes for the in-fill tests (tests/test_infill_host.py, tests/test_gpu_infill.py): built once per
process, handed out read-only.  Not a test module."""
import functools

import numpy as np

NOVAL = -32768.0


def terrain(h, w, ripple=False):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    z = -2000.0 + 300.0 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
    if ripple:
        z = z + 40.0 * np.sin(xx / 5.0 + yy / 7.0)
    return z


def _frozen(a):
    a.setflags(write=False)
    return a


def _punch(g, pixels):
    for r, c in pixels:
        g[r, c] = NOVAL


def hline(r, c, n):
    return [(r, c + i) for i in range(n)]


def vline(r, c, n):
    return [(r + i, c) for i in range(n)]


def blob(r, c, n, width=5):
    """The most compact n-pixel shape: rows of ``width`` from (r, c)."""
    return [(r + i // width, c + i % width) for i in range(n)]


@functools.lru_cache(maxsize=None)
def grid_330x300():
    """fillNan(256, 32, 24): tiles at rows 0 / 192 and columns 0 / 192, seams at 192 and 224, margin lines at 32, 298 (rows)
    and 32, 268 (columns).  Returns (grid, {name: pixel list})."""
    h, w = 330, 300
    g = terrain(h, w).astype(np.float32)
    holes = {
        "single": [(100, 100)],
        "line23": hline(60, 50, 23), "line24": hline(70, 50, 24), "line25": hline(80, 50, 25),
        "blob23": blob(110, 40, 23), "blob24": blob(120, 40, 24),
        "diagonal10": [(130 + i, 150 + i) for i in range(10)],
        "anti_diagonal7": [(130 + i, 140 - i) for i in range(7)],
        "seam_row192": vline(190, 100, 5), "seam_row224": vline(222, 130, 5),
        "seam_col192": hline(100, 190, 5), "seam_col224": hline(140, 222, 5),
        "seam_corner192": blob(191, 191, 9, 3), "seam_corner224": blob(223, 223, 9, 3),
        "across_row32": vline(29, 80, 7), "across_col31": hline(90, 28, 7),
        "across_row298": vline(294, 200, 8), "across_col268": hline(150, 264, 8),
        "corner_margin": blob(30, 30, 16, 4),
        "touch_row0": vline(0, 140, 3), "touch_last_row": vline(327, 160, 3),
        "touch_col0": hline(170, 0, 4), "touch_last_col": hline(180, 296, 4),
        "pair_a": [(200, 60), (201, 60)], "pair_b": [(200, 62), (201, 62), (202, 63)],        # one valid pixel between
        "pair_c": hline(210, 70, 3), "pair_d": hline(212, 70, 4),                            # one valid row between
        "l_shape": vline(160, 100, 6) + hline(165, 101, 6),
        "ring": [(r, c) for r in range(175, 179) for c in range(110, 114) if r in (175, 178) or c in (110, 113)],
        "big": [(r, c) for r in range(236, 306) for c in range(20, 111)],                   # 6370 pixels, over two margin lines
    }
    for p in holes.values():
        _punch(g, p)
    return _frozen(g), holes


@functools.lru_cache(maxsize=None)
def grid_ortho():
    """fillNan(1024, 128, 8) on 306 x 310: one tile, interior rows [128, 178) and columns [128, 182)."""
    h, w = 306, 310
    rng = np.random.default_rng(11)
    g = (0.5 + 0.3 * np.sin(np.arange(w)[None, :] / 9.0) * np.cos(np.arange(h)[:, None] / 13.0)
         + 0.01 * rng.standard_normal((h, w))).astype(np.float32)
    holes = {
        "single": [(140, 140)], "line7": hline(145, 135, 7), "line8": hline(148, 135, 8), "line9": hline(151, 135, 9),
        "blob7": blob(155, 136, 7, 3), "diagonal6": [(160 + i, 150 + i) for i in range(6)],
        "across_row128": vline(126, 145, 5), "across_col128": hline(165, 126, 5),
        "across_row178": vline(175, 170, 6), "across_col182": hline(140, 179, 6),
        "outside": blob(60, 60, 4, 2), "touch_row0": vline(0, 150, 3),
        "pair_a": [(170, 140)], "pair_b": [(170, 142), (171, 143)],
        "big": [(r, c) for r in range(130, 150) for c in range(150, 175)],
    }
    for p in holes.values():
        _punch(g, p)
    return _frozen(g), holes


@functools.lru_cache(maxsize=None)
def grid_96x1100():
    """(24, 32): components on the columns where the 64-pixel words of the label stage meet (63/64, 127/128, 1023/1024), on the
    rows where its 4-row workgroups meet, and on their corners; one across the right margin line 1068."""
    h, w = 96, 1100
    g = terrain(h, w, ripple=True).astype(np.float32)
    holes = {
        "col63_64": hline(40, 60, 8), "col127_128": hline(44, 120, 16), "col1023_1024": hline(50, 1013, 23),
        "rows_43_44": vline(38, 200, 12), "corner_64_44": blob(42, 62, 20, 4), "corner_128_48": [(46 + i, 126 + i) for i in range(5)],
        "corner_1024_40": blob(40, 1022, 23, 5), "line24_across_64": hline(56, 52, 24), "line23_across_128": hline(58, 117, 23),
        "across_col1068": hline(45, 1060, 14), "across_row32": vline(28, 640, 9), "across_row64": vline(60, 704, 9),
        "pair_a": hline(36, 63, 1), "pair_b": hline(36, 65, 2), "single_at_64": [(52, 64)], "single_at_63": [(54, 63)],
        "big": [(r, c) for r in range(34, 62) for c in range(300, 400)],
    }
    for p in holes.values():
        _punch(g, p)
    return _frozen(g), holes


def random_holes(shape, n_holes, rng, lo=1, hi=22, edge=40):
    """``n_holes`` random 8-connected shapes of lo .. hi pixels, at least ``edge`` pixels from the border and three pixels
    apart from each other: lists of pixels."""
    h, w = shape
    taken = np.zeros(shape, bool)
    out = []
    while len(out) < n_holes:
        size = int(rng.integers(lo, hi + 1))
        r, c = int(rng.integers(edge + 12, h - edge - 12)), int(rng.integers(edge + 12, w - edge - 12))
        pix = [(r, c)]
        while len(pix) < size:
            br, bc = pix[int(rng.integers(len(pix)))]
            q = (br + int(rng.integers(-1, 2)), bc + int(rng.integers(-1, 2)))
            if q not in pix and abs(q[0] - r) < 11 and abs(q[1] - c) < 11:
                pix.append(q)
        rr, cc = np.array(pix).T
        if taken[max(rr.min() - 3, 0):rr.max() + 4, max(cc.min() - 3, 0):cc.max() + 4].any():
            continue
        taken[rr, cc] = True
        out.append(sorted(pix))
    return out

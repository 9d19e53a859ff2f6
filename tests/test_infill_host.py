"""CPU: the device in-filling's rule, twin and host pieces (moonsuperresolution_amd/infill.py, csrc/infill_solve.h).

  * the keyword and the declarations; every argument error of msr_infill_small_holes, returned before any launch (host arrays
    stand in for device memory);
  * fill_set equals the set of pixels whose bits preprocess.fillNan changes, at (24, 32) on 330 x 300 and at (8, 128) on
    306 x 310 (tests/infill_cases.py: sizes A - 1, A, A + 1, chains, tile seams, margin lines, raster edges, two components one
    valid pixel apart, a hole of thousands of pixels);
  * the twin: bits outside the fill set kept, no NaN, a plane restored, a row window equal to the whole grid;
  * msr_infill_component_host (the kernel's build-and-solve with one lane) equals the twin bit for bit;
  * accuracy against the host's griddata on two analytic terrains: the twin's largest error at the filled pixels is no larger
    than griddata's.  A band-limited noise terrain is recorded without an assertion.  Figures: profiles/infill_parity.json.
"""
import json
import os

import numpy as np
import pytest

from moonsuperresolution_amd import _lib, infill
from moonsuperresolution_amd import preprocess as pp
from tests import infill_cases as cases

NOVAL = cases.NOVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"330x300": (cases.grid_330x300, 24, 32, 256), "ortho": (cases.grid_ortho, 8, 128, 1024)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def twins():
    """The twin's result on each fixture grid, computed once, read-only."""
    out = {}
    for name, (make, area, margin, _) in FIXTURES.items():
        ref = infill.infill_reference(make()[0], NOVAL, area, margin)
        ref.setflags(write=False)
        out[name] = ref
    return out


# ---- keyword, declarations, argument errors --------------------------------------------------------------------------------
def test_driver_keyword():
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, HaloShardedSuperResolution
    cfg = DSRConfig(image_size=64, stride=16, batch_size=4, tile_size=128)
    for cls in (DEMSuperResolution, HaloShardedSuperResolution):
        with pytest.raises(ValueError, match="infill"):
            cls(cfg, infill="gpu")
    with pytest.raises(ValueError, match="infill"):
        pp.preprocess_rows(None, None, None, np.zeros((8, 8), np.float32), 0, (8, 8), (0, 8), NOVAL, infill="gpu")
    with pytest.raises(ValueError, match="infill"):
        pp.preprocess(None, None, None, np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float32), NOVAL, infill="gpu")


def test_entries_are_declared(lib):
    header = open(os.path.join(ROOT, "include", "moonsr.h")).read()
    declared = {name for name, _, _ in _lib.SYMBOLS}
    for name in ("msr_infill_small_holes", "msr_infill_workspace_bytes", "msr_infill_component_host", "msr_debug_infill_stage"):
        assert name + "(" in header and name in declared and hasattr(lib, name), name
    assert lib.msr_infill_workspace_bytes(96, 1100) == 16 + 8 * 96 * 18 + 4 * 48 * 550
    assert lib.msr_infill_workspace_bytes(0, 5) == -1 and lib.msr_infill_workspace_bytes(1 << 16, 1 << 15) == -1


def test_argument_errors_name_the_argument(lib):
    n, w = 70, 80
    grid = np.full((n, w), 1.0, np.float32)
    grid[40, 40] = NOVAL
    before = grid.copy()
    need = lib.msr_infill_workspace_bytes(n, w)
    ws = np.zeros(need // 8 + 1, np.uint64)
    good = dict(grid=grid.ctypes.data, row0=0, n_rows=n, full_rows=n, cols=w, max_area=24, margin=32, ws=ws.ctypes.data,
                ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.msr_infill_small_holes(None, a["grid"], a["row0"], a["n_rows"], a["full_rows"], a["cols"], NOVAL, a["max_area"],
                                        a["margin"], a["ws"], a["ws_bytes"], None)
        return rc, (lib.msr_last_error(None) or b"").decode()
    for kw, word in ((dict(grid=None), "grid_dev"), (dict(ws=None), "workspace_dev"), (dict(n_rows=0), "n_rows"),
                     (dict(full_rows=-1), "full_rows"), (dict(cols=0), "cols"), (dict(max_area=1), "max_area"),
                     (dict(max_area=33, margin=40), "max_area"), (dict(margin=24), "margin"), (dict(row0=-1), "row0"),
                     (dict(row0=1), "full_rows"), (dict(full_rows=n - 1), "full_rows"), (dict(ws_bytes=need - 1), "workspace_bytes"),
                     (dict(ws=ws.ctypes.data + 4), "aligned"), (dict(n_rows=1 << 16, full_rows=1 << 16, cols=1 << 15), "2^31")):
        rc, msg = call(**kw)
        assert rc == _lib.MSR_ERR_INVALID and word in msg and "msr_infill_small_holes" in msg, (kw, rc, msg)
    assert lib.msr_debug_infill_stage(None, good["grid"], 0, n, n, w, NOVAL, 24, 32, good["ws"], need, None, 3) == -1
    assert np.array_equal(bits(grid), bits(before)) and not ws.any()           # nothing ran


# ---- the fill set against the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_fills():
    out = {}
    for name, (make, area, margin, tile) in FIXTURES.items():
        out[name] = pp.fillNan(make()[0], NOVAL, tile, margin, area)
    return out


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fill_set_is_the_set_of_pixels_the_host_changes(name, host_fills):
    make, area, margin, _ = FIXTURES[name]
    grid, holes = make()
    changed = bits(host_fills[name]) != bits(grid)
    take = infill.fill_set(grid, NOVAL, area, margin)
    assert take.sum() > 30 and np.array_equal(take, changed), (int(take.sum()), int(changed.sum()), np.argwhere(take != changed)[:5])
    filled = {k for k, p in holes.items() if any(take[r, c] for r, c in p)}
    whole = {k for k, p in holes.items() if all(take[r, c] for r, c in p)}
    if name == "330x300":
        assert {"single", "line23", "blob23", "diagonal10", "pair_a", "pair_b", "ring", "seam_corner192", "seam_row224"} <= whole
        assert not {"line24", "line25", "blob24", "big", "touch_row0", "touch_last_row", "touch_col0", "touch_last_col"} & filled
        assert {"across_row32", "across_col31", "across_row298", "across_col268", "corner_margin"} <= filled - whole
    else:
        assert {"single", "line7", "blob7", "diagonal6", "pair_a", "pair_b"} <= whole
        assert not {"line8", "line9", "big", "outside", "touch_row0"} & filled
        assert {"across_row128", "across_col128", "across_row178", "across_col182"} <= filled - whole


# ---- the twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXTURES))
def test_twin_writes_the_fill_set_only_and_no_nan(name, twins):
    make, area, margin, _ = FIXTURES[name]
    grid = make()[0]
    take = infill.fill_set(grid, NOVAL, area, margin)
    ref = twins[name]
    assert np.array_equal(bits(ref) != bits(grid), take)
    assert not np.isnan(ref).any() and (ref[take] > NOVAL).all()
    withnan = grid.copy()
    withnan[100, 200] = withnan[140, 141] = np.nan            # NaN is a hole: one alone, one joining "single" of the ortho grid
    out = infill.infill_reference(withnan, NOVAL, area, margin)
    assert infill.fill_set(withnan, NOVAL, area, margin)[140, 141] and not np.isnan(out[140, 141])


def test_twin_restores_a_plane():
    yy, xx = np.mgrid[0:120, 0:130].astype(np.float64)
    plane = (-2000.0 + 0.75 * xx - 1.25 * yy).astype(np.float32)          # exact in float32
    grid = plane.copy()
    rng = np.random.default_rng(5)
    for pix in cases.random_holes(grid.shape, 12, rng, 1, 23, edge=25):
        for r, c in pix:
            grid[r, c] = NOVAL
    out = infill.infill_reference(grid, NOVAL, 24, 25)
    take = infill.fill_set(grid, NOVAL, 24, 25)
    assert take.sum() > 60
    assert np.abs(out.astype(np.float64) - plane)[take].max() <= 2.0 ** -12          # the plane solves the system exactly: half a float32 ulp at 2048 (2^-13) and the float64 solve's 1e-8
    assert np.array_equal(bits(out)[~take], bits(grid)[~take])


@pytest.mark.parametrize("q0,q1", [(0, 256), (60, 330), (70, 290), (160, 256)])
def test_twin_on_a_row_window_gives_the_whole_grid_bits(q0, q1, twins):
    """The rows at least 32 from a cut edge (window_plan's fill rows lie so in its d4 band) take the whole grid's bits; the
    window fills nothing nearer than max_area rows to a cut."""
    grid = cases.grid_330x300()[0]
    whole = twins["330x300"]
    out = infill.infill_reference(grid[q0:q1], NOVAL, 24, 32, row0=q0, full_rows=grid.shape[0])
    a = q0 + 32 if q0 else 0
    b = q1 - 32 if q1 < grid.shape[0] else q1
    assert np.array_equal(bits(out[a - q0:b - q0]), bits(whole[a:b]))
    a24, b24 = (q0 + 24 if q0 else 0), (q1 - 24 if q1 < grid.shape[0] else q1)
    assert np.array_equal(bits(out[a24 - q0:b24 - q0]), bits(whole[a24:b24]))
    assert np.array_equal(bits(out[:a24 - q0]), bits(grid[q0:a24])) and np.array_equal(bits(out[b24 - q0:]), bits(grid[b24:q1]))


# ---- the one-component host entry ----------------------------------------------------------------------------------------------
def _host_component(lib, grid, rr, cc):
    r32, c32 = np.ascontiguousarray(rr, np.int32), np.ascontiguousarray(cc, np.int32)
    out = np.zeros(len(r32), np.float32)
    rc = lib.msr_infill_component_host(grid.ctypes.data, grid.shape[0], grid.shape[1], NOVAL, r32.ctypes.data, c32.ctypes.data,
                                       len(r32), out.ctypes.data)
    assert rc == 0
    return out


def _twin_component(grid, rr, cc):
    return np.array(infill.solve_component(grid, NOVAL, rr, cc), np.float64).astype(np.float32)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_host_entry_equals_the_twin_on_every_fixture_component(name, lib, twins):
    make, area, margin, _ = FIXTURES[name]
    grid = np.ascontiguousarray(make()[0])
    comps = infill.components(grid, NOVAL, area, margin)
    assert len(comps) >= 10
    for rr, cc, keep in comps:
        got = _host_component(lib, grid, rr, cc)
        assert np.array_equal(bits(got), bits(_twin_component(grid, rr, cc))), (name, rr[0], cc[0])
        assert np.array_equal(bits(got[keep]), bits(twins[name][rr[keep], cc[keep]]))


def test_host_entry_equals_the_twin_on_small_and_extreme_shapes(lib):
    base = cases.terrain(80, 90, ripple=True).astype(np.float32)
    shapes = [[(0, 0)]] + [[(0, 0), (dr, dc)] for dr, dc in ((0, 1), (1, -1), (1, 0), (1, 1))]       # all 1- and 2-pixel shapes
    shapes += [cases.hline(0, 0, 23), cases.vline(0, 0, 23), cases.blob(0, 0, 23), [(i, i) for i in range(23)],
               [(i, -i) for i in range(23)], cases.hline(0, 0, 31), cases.blob(0, 0, 31, 6)]
    for k, shape in enumerate(shapes):
        for r0, c0 in ((40, 45), (3, 35)):
            pix = sorted((r0 + dr, c0 + dc) for dr, dc in shape)
            if pix[-1][0] >= 78:
                continue
            grid = base.copy()
            for r, c in pix:
                grid[r, c] = NOVAL
            rr, cc = np.array(pix).T
            got = _host_component(lib, grid, rr, cc)
            assert np.isfinite(got).all()
            assert np.array_equal(bits(got), bits(_twin_component(grid, rr, cc))), (k, r0, c0)
    # the same component elsewhere in another grid, same surroundings: the same bits (only relative positions enter)
    pix = sorted((40 + dr, 45 + dc) for dr, dc in cases.blob(0, 0, 23))
    grid = base.copy()
    for r, c in pix:
        grid[r, c] = NOVAL
    rr, cc = np.array(pix).T
    big = np.full((200, 300), 7.0, np.float32)
    big[100:180, 150:240] = grid
    assert np.array_equal(bits(_host_component(lib, grid, rr, cc)), bits(_host_component(lib, big, rr + 100, cc + 150)))
    out = np.zeros(4, np.float32)
    bad = np.array([[5, 5], [5, 4]], np.int32)                                          # not row-major
    assert lib.msr_infill_component_host(grid.ctypes.data, 80, 90, NOVAL, bad[:, 0].copy().ctypes.data, bad[:, 1].copy().ctypes.data,
                                         2, out.ctypes.data) == -1
    assert lib.msr_infill_component_host(grid.ctypes.data, 80, 90, NOVAL, None, None, 1, out.ctypes.data) == -1


# ---- accuracy against the host's griddata ------------------------------------------------------------------------------------------
def _noise_terrain(h, w):
    from scipy import ndimage
    z = ndimage.gaussian_filter(np.random.default_rng(21).standard_normal((h, w)), 2.0)
    return -2000.0 + 40.0 * z / z.std()


TERRAINS = {"smooth": lambda: cases.terrain(256, 256), "ripple": lambda: cases.terrain(256, 256, ripple=True),
            "noise": lambda: _noise_terrain(256, 256)}
ASSERTED = ("smooth", "ripple")


@pytest.fixture(scope="module")
def accuracy():
    """Per terrain: 40 seeded random holes of 1 .. 22 pixels at least 40 pixels from the edge of a 256 x 256 tile; the host's
    interpolateMissingValues (griddata) and the twin at (24, 32); errors at the fill set against the float64 terrain."""
    out = {}
    for k, (name, make) in enumerate(TERRAINS.items()):
        truth = make()
        grid = truth.astype(np.float32)
        for pix in cases.random_holes(grid.shape, 40, np.random.default_rng(100 + k), 1, 22, edge=40):
            for r, c in pix:
                grid[r, c] = NOVAL
        take = infill.fill_set(grid, NOVAL, 24, 32)
        assert take.sum() == (grid <= NOVAL).sum() > 300
        host = pp.interpolateMissingValues(grid.copy(), NOVAL, max_fill_area=24)
        twin = infill.infill_reference(grid, NOVAL, 24, 32)
        assert np.array_equal(bits(host) != bits(grid), take)

        def fig(a, b):
            d = (np.asarray(a, np.float64) - np.asarray(b, np.float64))[take]
            return {"max": float(np.abs(d).max()), "rms": float(np.sqrt((d * d).mean()))}
        out[name] = {"filled_pixels": int(take.sum()), "host_vs_truth": fig(host, truth), "twin_vs_truth": fig(twin, truth),
                     "twin_vs_host": fig(twin, host)}
    return out


@pytest.mark.parametrize("name", ASSERTED)
def test_twin_is_no_worse_than_griddata_on_analytic_terrain(name, accuracy):
    f = accuracy[name]
    print(name, json.dumps(f))
    assert f["twin_vs_truth"]["max"] <= f["host_vs_truth"]["max"], f


def test_accuracy_record(accuracy):
    """All three terrains, the noise one included (no assertion: there neither fill can know the data), to
    profiles/infill_parity.json.  The content is a function of the seeds alone."""
    record = {"what": "error at the filled pixels, metres at a -2000 m datum: host = scipy griddata(cubic) on the 256 x 256 tile, "
                      "twin = infill.infill_reference (the device in-fill's bits), truth = the float64 terrain",
              "terrains": accuracy}
    print(json.dumps(record, indent=1))
    with open(os.path.join(ROOT, "profiles", "infill_parity.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    assert set(accuracy) == set(TERRAINS)

"""GPU (-m gpu): DEMSuperResolution(resident=True) — the rasters stay on the device from decode to encode.

  1. files: processFiles writes, byte for byte, the three files of resident=False with the same other arguments, for
     (decoder, infill, encoder) all on the device, all on the host and mixed, with and without preprocess (swap_dsize=False on
     300 x 256, swap_dsize=True on 272 x 272), with a Generator (counter sampler: runs are comparable) and with the identity
     model, and for the row window of rank 1 of 2 (mode="tiles", gather=False);
  2. types: after loadImages, preprocess and processMap the rasters held and the products are CUDA tensors (float32; good
     uint8) of dem_shape in resident mode and NumPy arrays otherwise; processTiles gives device tensors per tile; setImages takes
     tensors and arrays in both modes, with the same checks and messages; preprocess leaves the loaded ortho's bits alone;
  3. transfers: all three stages on the device and a Generator: per direction the resident run's ``transfers`` sum to at most the
     two input files (up) / the three output files (down) plus 64 bytes per block — no raster crosses; the non-resident run of
     the same call logs at least the two canvases going up and the three products coming down (the control: the log sees them);
  4. pipeline depth: pipeline=1 and pipeline=2 give the same resident files, and a second processFiles on the same instance
     gives the same files again (persistent buffers, allocator ordering).
All comparisons are exact.  The two-process rank-0 writer is in tests/test_gpu_products_rank0.py.
"""
import os

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import geotiff as G
from tests import resident_cases as cases

pytestmark = pytest.mark.gpu
COMBOS = [("device", "device", "device"), ("host", "host", "host"), ("device", "host", "device")]


@pytest.fixture(scope="module")
def gen(hip_lib):
    from moonsuperresolution_amd import Generator
    g = Generator(cases.S, cases.B, weights=11, sampler="counter", seed=5)
    yield g
    g.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """{name: (folder, ortho, DEM)} of the three rasters, written once."""
    out = {}
    for name, shape in cases.SHAPES.items():
        folder = str(tmp_path_factory.mktemp(f"in_{name}"))
        out[name] = (folder,) + cases.write_inputs(folder, shape)
    return out


def driver(folder, save, model, resident, combo=COMBOS[0], pipeline=2):
    from moonsuperresolution_amd import DEMSuperResolution
    decoder, infill, encoder = combo
    return DEMSuperResolution(cases.cfg(source_folder_path=folder, save_path=str(save), map_name="m"), model=model,
                              pipeline=pipeline, decoder=decoder, infill=infill, encoder=encoder, resident=resident)


def run(folder, save, model, resident, combo=COMBOS[0], pipeline=2, **kw):
    d = driver(folder, save, model, resident, combo, pipeline)
    d.processFiles(**kw)
    torch.cuda.synchronize()
    log = list(d.transfers)
    d.close()
    return cases.product_bytes(str(save)), log


def same_files(got, want):
    for name in ("mean", "std", "good"):
        assert want[name] is not None and len(want[name]) > 1000, name
        assert got[name] == want[name], name


# ---- 1. files ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["generator", "identity"])
@pytest.mark.parametrize("preprocess", [False, True])
@pytest.mark.parametrize("combo", COMBOS, ids=["-".join(c) for c in COMBOS])
def test_resident_files_equal_the_host_held_files(tmp_path, inputs, gen, combo, preprocess, model):
    folder = inputs["square" if preprocess else "wide"][0]
    m = gen if model == "generator" else cases.f32_identity
    kw = dict(preprocess=preprocess, swap_dsize=preprocess)
    want, _ = run(folder, tmp_path / "host", m, False, combo, **kw)
    got, _ = run(folder, tmp_path / "resident", m, True, combo, **kw)
    same_files(got, want)
    good, _ = G.read_geotiff(str(tmp_path / "resident" / "m_good.tiff"))
    assert good.any() and not good.all()              # valid terrain and the no-data corner are both in the products


@pytest.mark.parametrize("preprocess", [False, True])
def test_resident_row_window_of_a_rank(tmp_path, inputs, gen, preprocess):
    folder = inputs["wide"][0]
    kw = dict(preprocess=preprocess, swap_dsize=False, mode="tiles", rank=1, world=2, gather=False)
    want, _ = run(folder, tmp_path / "host", gen, False, **kw)
    got, _ = run(folder, tmp_path / "resident", gen, True, **kw)
    same_files(got, want)
    mean, _ = G.read_geotiff(str(tmp_path / "resident" / "m_mean.tiff"))
    assert not mean[:256].any() and mean[256:].any()   # rank 1 of 2 owns the third tile row; the others' rows stay zero


# ---- 2. types ----------------------------------------------------------------------------------------------------------------
def _is_raster(a, resident, shape, dtype=torch.float32):
    if resident:
        return isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == dtype and tuple(a.shape) == tuple(shape)
    return isinstance(a, np.ndarray) and a.dtype == np.dtype(str(dtype).split(".")[1]) and a.shape == tuple(shape)


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[1]], ids=["device", "host"])
def test_types_of_the_rasters_held(tmp_path, inputs, combo, resident):
    folder, img, dem = inputs["square"]
    shape = cases.SHAPES["square"]
    d = driver(folder, tmp_path, cases.f32_identity, resident, combo)
    d.loadImages()
    assert _is_raster(d.img, resident, shape) and _is_raster(d.dem, resident, shape)
    loaded = d.img
    as_np = (lambda a: a.cpu().numpy()) if resident else np.asarray
    assert np.array_equal(as_np(d.img), img) and np.array_equal(as_np(d.dem), dem)
    d.preprocess(swap_dsize=True)
    assert _is_raster(d.img, resident, shape) and _is_raster(d.dem, resident, shape) and _is_raster(d.image, resident, shape)
    assert d.img is loaded and np.array_equal(as_np(d.img).view(np.uint32), img.view(np.uint32))   # the ortho keeps its bits
    assert (as_np(d.image).view(np.uint32) != img.view(np.uint32)).any()                            # the in-fill did write
    assert (as_np(d.dem) != dem).any()
    mean, std, good = d.processMap()
    assert _is_raster(mean, resident, shape) and _is_raster(std, resident, shape)
    assert _is_raster(good, resident, shape, torch.uint8)
    assert d.img is None and d.dem is None
    d.setImages(img, dem)
    d.padInputs()
    tiles = d.processTiles(d.generateTileList()[:2])
    for parts in tiles.values():
        for t, dt in zip(parts, (torch.float32, torch.float32, torch.uint8)):
            assert _is_raster(t, resident, (cases.T, cases.T), dt)
    again = d.rebuildMap(d.processTiles(d.generateTileList()))
    for a, b, dt in zip(again, d.processMap(img, dem), (torch.float32, torch.float32, torch.uint8)):
        assert _is_raster(a, resident, shape, dt) and _is_raster(b, resident, shape, dt)
        assert np.array_equal(as_np(a), as_np(b), equal_nan=True)
    d.close()


@pytest.mark.parametrize("resident", [True, False])
def test_set_images_takes_tensors_and_arrays(tmp_path, inputs, resident):
    _, img, dem = inputs["wide"]
    d = driver("", tmp_path, cases.f32_identity, resident)
    timg, tdem = torch.from_numpy(img).cuda(), torch.from_numpy(dem).cuda()
    results = []
    for a, b in ((img, dem), (timg, tdem)):
        d.setImages(a, b)
        assert _is_raster(d.img, resident, img.shape) and _is_raster(d.dem, resident, img.shape)
        if resident and a is timg:
            assert d.img is timg and d.dem is tdem    # kept, not copied
        results.append([np.asarray(p.cpu() if resident else p) for p in d.processMap()])
    for p, q in zip(*results):
        assert np.array_equal(p, q, equal_nan=True)
    d.setImages(timg[100:200], tdem[100:200], row0=100, full_shape=img.shape)
    assert d.windowed and d.row0 == 100 and d.dem_shape == img.shape
    with pytest.raises(ValueError, match="must be 2-D arrays of the same shape"):
        d.setImages(timg, tdem[:-1])
    with pytest.raises(ValueError, match=r"rows \[250, 350\) x 256 columns are not a row window"):
        d.setImages(timg[:100], tdem[:100], row0=250, full_shape=img.shape)
    with pytest.raises(ValueError, match="CUDA float32"):
        d.setImages(timg.double(), tdem.double())
    d.close()


# ---- 3. transfers ------------------------------------------------------------------------------------------------------------
def _sums(log):
    out = {"h2d": 0, "d2h": 0}
    for direction, nbytes, what in log:
        assert direction in out and isinstance(nbytes, int) and nbytes >= 0 and isinstance(what, str) and what
        out[direction] += nbytes
    return out


def test_resident_moves_only_compressed_blocks(tmp_path, inputs, gen):
    folder, img, dem = inputs["wide"]
    H, W = cases.SHAPES["wide"]
    kw = dict(preprocess=True, swap_dsize=False)
    want, host_log = run(folder, tmp_path / "host", gen, False, **kw)
    got, log = run(folder, tmp_path / "resident", gen, True, **kw)
    same_files(got, want)
    in_files = [os.path.join(folder, f) for f in ("run-DRG.tif", "run-DEM.tif")]
    in_bytes = sum(os.path.getsize(f) for f in in_files)
    out_bytes = sum(len(b) for b in got.values())
    raster = H * W * 4
    assert in_bytes < raster                          # both files together are smaller than ONE raw raster
    blocks_in = sum(-(-H // G._rows_per_strip(H, W * 4)) for _ in in_files)
    blocks_out = 2 * -(-H // G._rows_per_strip(H, W * 4)) + -(-H // G._rows_per_strip(H, W * 2))
    sums = _sums(log)
    print("resident:", sums, "host-held:", _sums(host_log), "inputs", in_bytes, "outputs", out_bytes, "raster", raster)
    assert 0 < sums["h2d"] <= in_bytes + 64 * (blocks_in + blocks_out)
    assert 0 < sums["d2h"] <= out_bytes + 64 * (blocks_in + blocks_out)
    assert sums["h2d"] < raster                       # so no raster went up
    # the control: the host-held run of the same call does move rasters, and the log sees them
    control = _sums(host_log)
    assert control["h2d"] >= 2 * raster and control["d2h"] >= 2 * raster + H * W
    whats = {what for _, _, what in host_log}
    assert {"DEM into its canvas", "ortho into its canvas", "decoded raster", "synthesised DEM"} <= whats
    assert sum(n for d, n, what in host_log if d == "d2h" and "product" in what) >= 2 * raster + H * W


def test_host_stages_keep_their_own_round_trip_only(tmp_path, inputs):
    """resident with every stage on the host and the identity model: what is logged is those stages' traffic — the upload of
    the decoded rasters, SciPy's grids, the model's batches, the products for the host encoder — and no canvas upload."""
    folder = inputs["wide"][0]
    _, log = run(folder, tmp_path / "resident", cases.f32_identity, True, COMBOS[1], preprocess=True, swap_dsize=False)
    whats = {what for _, _, what in log}
    assert {"ortho raster", "DEM raster", "ortho for the host in-fill", "in-filled ortho", "x1/4 grid for the host in-fill",
            "in-filled x1/4 grid", "batch for the host model", "predictions of the host model", "mean product",
            "std product", "good product"} == whats, whats


# ---- 4. pipeline depth, reuse ------------------------------------------------------------------------------------------------
def test_pipeline_depth_and_reuse(tmp_path, inputs, gen):
    folder = inputs["wide"][0]
    kw = dict(preprocess=True, swap_dsize=False)
    want, _ = run(folder, tmp_path / "p2", gen, True, pipeline=2, **kw)
    got, _ = run(folder, tmp_path / "p1", gen, True, pipeline=1, **kw)
    same_files(got, want)
    d = driver(folder, tmp_path / "twice", gen, True)
    for _ in range(2):
        d.processFiles(**kw)
        same_files(cases.product_bytes(str(tmp_path / "twice")), want)
        for f in os.listdir(tmp_path / "twice"):
            os.remove(tmp_path / "twice" / f)
    d.close()

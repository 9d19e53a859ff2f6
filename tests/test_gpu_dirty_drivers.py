"""GPU (-m gpu): the raster pipeline does not depend on what its ``torch.empty`` buffers held before.

tiler.py, halo.py, geotiff.py, preprocess.py and infill.py hold about forty ``torch.empty`` buffers (patch stacks, index
tables, accumulators, products, codec scratch, pinned staging).  In a test process the caching allocator mostly hands back
zeroed pages; in a long-lived one it hands back the last owner's data.  Every path below runs once as it is and once inside
``dirty_empty`` (tests/dirty_cases.py), where every such buffer starts as 0xFF bytes: NaN in every float format, -1 (the
kernels' own "no entry") in every index table.  The products must be the same arrays and, where files are written, the same
bytes.  No library change, no tolerance.

  * DEMSuperResolution, host-held, pipeline=1 and pipeline=2, with the identity model and with Generator(64, 4);
  * DEMSuperResolution(resident=True, decoder / infill / encoder on the device): strips; product_tile=(16, 16), overviews=2;
    product_layout="cog"; product_predictor=3;
  * HaloShardedSuperResolution on one rank, a band per patch row, batching="band" and "rank";
  * the two row-window resamplers; read_geotiff(decoder="device", rows=...); write_geotiff(encoder="device") from a CUDA tensor;
  * the control: inside the context a fresh torch.empty of every dtype the drivers use reads back as the pattern.
"""
import os

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import geotiff as G
from moonsuperresolution_amd import preprocess as pp
from tests import dirty_cases, resident_cases as cases
from tests import geotiff_tiled_cases as tiled

pytestmark = pytest.mark.gpu
NOVAL = cases.NOVAL


@pytest.fixture(scope="module")
def gen(hip_lib):
    from moonsuperresolution_amd import Generator
    g = Generator(cases.S, cases.B, weights=11, sampler="counter", seed=5)      # Generator(64, 4); counter noise: runs compare
    yield g
    g.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """(folder, ortho, DEM) of the smallest raster of tests/resident_cases.py, written once."""
    folder = str(tmp_path_factory.mktemp("in_wide"))
    return (folder,) + cases.write_inputs(folder, cases.SHAPES["wide"])


def both(monkeypatch, fn):
    """fn('clean'), then fn('dirty') inside the patched empty -> (clean result, dirty result); the dirty run must have
    drawn at least one poisoned buffer, or it showed nothing."""
    clean = fn("clean")
    torch.cuda.synchronize()
    with dirty_cases.dirty_empty(monkeypatch) as count:
        dirty = fn("dirty")
        torch.cuda.synchronize()
    assert sum(count.values()) > 0, "the path under test never called torch.empty: nothing was dirtied"
    return clean, dirty


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_files(got, want):
    for name in ("mean", "std", "good"):
        assert want[name] is not None and len(want[name]) > 1000, name
        assert got[name] == want[name], name


def process_files(folder, save, model, **kw):
    from moonsuperresolution_amd import DEMSuperResolution
    d = DEMSuperResolution(cases.cfg(source_folder_path=folder, save_path=str(save), map_name="m"), model=model, **kw)
    d.processFiles(preprocess=True, swap_dsize=False)
    torch.cuda.synchronize()
    d.close()
    return cases.product_bytes(str(save))


# ---- the tile driver -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["identity", "generator"])
@pytest.mark.parametrize("pipeline", [1, 2])
def test_host_held_driver(monkeypatch, tmp_path, inputs, gen, pipeline, model):
    m = gen if model == "generator" else cases.f32_identity
    clean, dirty = both(monkeypatch, lambda tag: process_files(inputs[0], tmp_path / tag, m, pipeline=pipeline))
    same_files(dirty, clean)
    good, _ = G.read_geotiff(str(tmp_path / "dirty" / "m_good.tiff"))
    assert good.any() and not good.all()                 # valid terrain and the no-data corner are both in the products


RESIDENT = {"strips": {}, "tiled": dict(product_tile=(16, 16), overviews=2),
            "cog": dict(product_tile=(16, 16), overviews=2, product_layout="cog"), "pred3": dict(product_predictor=3)}


@pytest.mark.parametrize("kind", list(RESIDENT))
def test_resident_driver(monkeypatch, tmp_path, inputs, gen, kind):
    kw = dict(resident=True, decoder="device", infill="device", encoder="device", **RESIDENT[kind])
    clean, dirty = both(monkeypatch, lambda tag: process_files(inputs[0], tmp_path / tag, gen, **kw))
    same_files(dirty, clean)
    mean, meta = G.read_geotiff(str(tmp_path / "dirty" / "m_mean.tiff"))
    assert mean.shape == cases.SHAPES["wide"] and np.isfinite(mean).all() and len(np.unique(mean)) > 100


# ---- the halo driver -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batching", ["band", "rank"])
def test_halo_driver_one_rank_banded(monkeypatch, inputs, gen, batching):
    from moonsuperresolution_amd import HaloShardedSuperResolution
    _, img, dem = inputs
    bands = []

    def run(tag):
        d = HaloShardedSuperResolution(cases.cfg(), model=gen)
        gen.reset_sampler(0)
        d.setImages(img, dem)
        st = d.haloAccumulate(0, 1, band_rows=1, batching=batching)
        bands.append(sum(1 for nv, _ in d.last_band_counts if nv))
        out = d.cropHalo([d.haloFinish(st, None, None)])
        out = [np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p) for p in out]
        d.close()
        return out

    clean, dirty = both(monkeypatch, run)
    assert bands[0] == bands[1] >= 2                     # at least two bands made calls
    assert len(clean) == len(dirty) == 3
    for a, b in zip(clean, dirty):
        assert bits_equal(a, b)
    assert clean[2].any() and not clean[2].all()


# ---- the entries the drivers are made of ---------------------------------------------------------------------------------------
def test_row_window_resamplers(monkeypatch, hip_lib):
    from moonsuperresolution_amd import ops
    ctx = ops.OpContext()
    rng = np.random.default_rng(4)
    h, w = 1030, 517                                     # a partial bottom block and a partial right one of the area kernel
    src = (rng.normal(size=(h, w)) * 1000).astype(np.float32)
    src[rng.uniform(size=src.shape) < 0.01] = np.nan
    dev = torch.from_numpy(src).cuda()
    small = torch.from_numpy((rng.normal(size=(33, 65)) * 100 - 2000).astype(np.float32)).cuda()
    small[8, 4] = float("nan")                          # under the taps of the rows asked for
    dh = 517                                             # cubic: 33 x 65 -> 517 x 1000, rows 100 .. 230 from their tap rows
    a, b = pp._cubic_tap_rows(100, 230, 33, dh)

    def run(tag):
        area = [pp._area_rows(ctx.lib, ctx.h, dev[4 * d0:min(4 * d1, h)], 4 * d0, h, (d0, d1), NOVAL, 0).cpu().numpy()
                for d0, d1 in ((0, 86), (86, 173), (172, 258), (129, 130))]
        cubic = pp._cubic_rows(ctx.lib, ctx.h, small[a:b], a, 33, (100, 230), (dh, 1000), NOVAL, as_tensor=True).cpu().numpy()
        return area + [cubic]

    clean, dirty = both(monkeypatch, run)
    for x, y in zip(clean, dirty):
        assert bits_equal(x, y)
    assert np.isnan(clean[0]).any() and (clean[-1] == NOVAL).any() and np.isfinite(clean[-1]).all()


@pytest.mark.parametrize("form", ["strips", "tiles"])
def test_read_geotiff_row_window(monkeypatch, tmp_path, hip_lib, form):
    shape = (70, 101)
    data = tiled.raster(shape, "float32")
    p = str(tmp_path / "a.tif")
    G.write_geotiff(p, data, nodata=NOVAL, **(dict(tile=(16, 32)) if form == "tiles" else {}))
    dev = torch.device("cuda", 0)
    windows = [(0, 70), (3, 50), (17, 18), (60, 70)]

    def run(tag):
        return [G.read_geotiff(p, rows=r, decoder="device", device=dev)[0] for r in windows]

    clean, dirty = both(monkeypatch, run)
    for r, x, y in zip(windows, clean, dirty):
        assert bits_equal(x, y) and bits_equal(x, G.read_geotiff(p, rows=r)[0]), r     # and the host decoder's rows


@pytest.mark.parametrize("how", [dict(), dict(tile=(16, 16), overviews=2), dict(tile=(16, 16), overviews=2, layout="cog"),
                                 dict(predictor=3)], ids=["strips", "tiled", "cog", "pred3"])
def test_write_geotiff_from_a_device_tensor(monkeypatch, tmp_path, hip_lib, how):
    dev = torch.device("cuda", 0)
    dem = tiled.raster((70, 101), "float32").copy()
    good = (np.arange(70 * 101).reshape(70, 101) % 41).astype(np.float32)
    t_dem, t_good = torch.from_numpy(dem).to(dev), torch.from_numpy(good).to(dev)

    def run(tag):
        a, b = str(tmp_path / f"{tag}_dem.tif"), str(tmp_path / f"{tag}_good.tif")
        G.write_geotiff(a, t_dem, nodata=NOVAL, encoder="device", **how)
        if how.get("predictor") != 3:                    # the floating-point predictor is for float samples
            G.write_geotiff(b, t_good, nodata=NOVAL, dtype=np.uint16, encoder="device", **how)
        return [open(f, "rb").read() for f in (a, b) if os.path.exists(f)]

    clean, dirty = both(monkeypatch, run)
    assert clean == dirty and all(len(f) > 200 for f in clean) and len(clean) == (1 if how.get("predictor") == 3 else 2)
    G.write_geotiff(str(tmp_path / "host.tif"), dem, nodata=NOVAL, **how)
    assert open(str(tmp_path / "host.tif"), "rb").read() == dirty[0]


# ---- the control ---------------------------------------------------------------------------------------------------------------
def test_control_empty_is_the_pattern_on_the_device(monkeypatch, hip_lib):
    dev = torch.device("cuda", 0)
    real = torch.empty
    with dirty_cases.dirty_empty(monkeypatch) as count:
        for dtype in dirty_cases.DRIVER_DTYPES:
            for t in (torch.empty((5, 7), dtype=dtype, device=dev), torch.empty(33, dtype=dtype, pin_memory=True),
                      torch.empty_like(torch.zeros((3, 4), dtype=dtype, device=dev)),
                      torch.zeros(2, dtype=dtype, device=dev).new_empty((6,))):
                raw = dirty_cases.storage_bytes(t).cpu()
                assert raw.numel() == t.numel() * t.element_size() and bool((raw == dirty_cases.PATTERN).all()), (dtype, t.device)
            assert torch.empty(33, dtype=dtype, pin_memory=True).is_pinned()
        f = torch.empty(4, dtype=torch.float32, device=dev)
        i = torch.empty(4, dtype=torch.int32, device=dev)
        assert torch.isnan(f).all() and (i == -1).all()
        assert count["empty"] >= 2 * len(dirty_cases.DRIVER_DTYPES) and count["empty_like"] and count["new_empty"]
    assert torch.empty is real

"""CPU: the parts of the resident mode that need no GPU.

  * ``resident`` must be a bool: the check runs before the GPU is looked for, so it raises ValueError here too;
    HaloShardedSuperResolution accepts the keyword and refuses True;
  * geotiff._band_bytes_on_device (on CPU tensors: the function is device-agnostic) gives NumPy's ``astype`` bytes for the
    cropped, non-contiguous views saveGTiff hands it: uint8 -> uint16 directly (the ``good`` product), same-width integers,
    narrowing and float -> integer through int64, float32 -> float32;
  * process_map_sharded(as_tensor=True) returns the tensors of the default call's arrays; ``local=True`` this rank's rows only;
  * the test rasters compress: the input files are under half the raw size (the transfer test of tests/test_gpu_resident.py
    rests on that).
"""
import os

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import DEMSuperResolution, HaloShardedSuperResolution
from moonsuperresolution_amd import distributed as D
from moonsuperresolution_amd import geotiff as G
from tests import resident_cases as cases


@pytest.mark.parametrize("bad", [1, 0, "yes", None, np.True_])
def test_resident_must_be_a_bool(bad):
    with pytest.raises(ValueError, match="resident must be a bool"):
        DEMSuperResolution(cases.cfg(), resident=bad)
    with pytest.raises(ValueError, match="resident must be a bool"):
        HaloShardedSuperResolution(cases.cfg(), resident=bad)


def test_the_halo_mode_refuses_resident():
    with pytest.raises(ValueError, match="resident=True is not built for the halo mode"):
        HaloShardedSuperResolution(cases.cfg(), resident=True)


def test_products_must_be_known():
    # processFiles checks the keyword before anything else; no instance can be built here, so the check is called unbound
    class Stub:
        transfers = []
    with pytest.raises(ValueError, match="products must be 'gathered' or 'rank0'"):
        DEMSuperResolution.processFiles(Stub(), products="rank1")


@pytest.mark.parametrize("src,dst", [("uint8", "<u2"), ("int8", "<u2"), ("int16", "<u2"), ("int32", "<u2"), ("uint8", "<u1"),
                                     ("float32", "<u2"), ("float32", "<f4"), ("float64", "<f4"), ("int32", "<f4")])
def test_band_bytes_equal_numpy_astype(src, dst):
    rng = np.random.default_rng(3)
    if src.startswith("float"):
        a = rng.uniform(-70000.0, 70000.0, (37, 29)).astype(src)
    else:
        info = np.iinfo(src)
        a = rng.integers(info.min, int(info.max) + 1, (37, 29)).astype(src)
    t = torch.from_numpy(a)[:33, :21]                 # cropped: not contiguous
    assert not t.is_contiguous()
    dt = np.dtype(dst)
    got = G._band_bytes_on_device(t, 5, 30, dt, torch.device("cpu")).numpy()
    with np.errstate(invalid="ignore"):
        want = a[5:30, :21]
        want = (want.astype(np.int64).astype(dt) if dt.kind != "f" else want.astype(dt))
    assert got.dtype == np.uint8 and np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(-1))
    assert np.array_equal(torch.from_numpy(a).numpy(), a)      # the source keeps its bits


def _tiles(shape, T):
    return D.tile_origins(shape, T)


def _tile(shape, T):
    def process_tile(xx, yy):
        yy_, xx_ = np.mgrid[yy:yy + T, xx:xx + T]
        m = (yy_ * 1000 + xx_).astype(np.float32)
        return m, -m, ((yy_ + xx_) % 251).astype(np.uint8)
    return process_tile


@pytest.mark.parametrize("shape", [(300, 256), (300, 300), (128, 100)])
def test_process_map_sharded_as_tensor_and_local(shape):
    T = 128
    tiles = _tiles(shape, T)
    want = D.process_map_sharded(shape, T, tiles, _tile(shape, T))
    got = D.process_map_sharded(shape, T, tiles, _tile(shape, T), as_tensor=True)
    for w, g, dt in zip(want, got, (torch.float32, torch.float32, torch.uint8)):
        assert isinstance(w, np.ndarray) and isinstance(g, torch.Tensor) and g.dtype == dt
        assert tuple(g.shape) == shape and np.array_equal(g.numpy(), w)
    for world in (1, 2, 3, 8):
        plan = D.strip_plan(shape, 4, T, world)
        for rank in range(world):
            r0, r1 = plan["rows"][rank]
            mine = D.process_map_sharded(shape, T, tiles, _tile(shape, T), rank, world, as_tensor=True, local=True)
            for w, g in zip(want, mine):
                assert tuple(g.shape) == (r1 - r0, shape[1]) and np.array_equal(g.numpy(), w[r0:r1]), (world, rank)
    with pytest.raises(ValueError, match="as_tensor"):
        D.process_map_sharded(shape, T, tiles, _tile(shape, T), local=True)


def test_the_transfer_log_of_process_map_sharded_is_silent_on_the_cpu():
    log = []
    D.process_map_sharded((128, 100), 128, _tiles((128, 100), 128), _tile((128, 100), 128), transfers=log)
    assert log == []                                   # host tensors: nothing crosses to a device


@pytest.mark.parametrize("name", sorted(cases.SHAPES))
def test_the_input_files_compress(tmp_path, name):
    shape = cases.SHAPES[name]
    img, dem = cases.write_inputs(str(tmp_path), shape)
    assert (img == cases.NOVAL).sum() > 2000 and (dem == cases.NOVAL).sum() > 2000
    raw = shape[0] * shape[1] * 4
    for f in ("run-DRG.tif", "run-DEM.tif"):
        size = os.path.getsize(tmp_path / f)
        assert size < raw // 2, (f, size, raw)
        back, _ = G.read_geotiff(str(tmp_path / f))
        assert np.array_equal(back, img if "DRG" in f else dem)

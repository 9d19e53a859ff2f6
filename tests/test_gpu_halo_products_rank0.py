"""GPU (-m gpu): processFiles(mode="halo", products="rank0") in fresh child processes on one device over gloo (the manner of
tests/test_gpu_products_rank0.py; at most three children hold the GPU beside this process).

The reference for "the same files" is the default path with the same ranks: every worker runs products="gathered" first and
products="rank0" second, in the same process group, into different folders.  (A one-process run is no reference: boundary
zones are merged pairwise, so a two-rank map is not bitwise the one-rank map.)

  * two ranks, 300 x 256: the rank boundary is raster row 208, inside a strip of the float32 products (64 rows) and of the
    uint16 product (128 rows); rank 1 hands rows [208, 256) down, each rank encodes its strips and rank 0 writes: its three
    files equal its gathered files byte for byte, ``products_path == "rank0"``, rank 1's folder stays empty.  Once with every
    stage on the device (no product raster is downloaded), once on the host, once with batching="rank", accumulate="band";
  * three ranks, 300 x 64: the uint16 product is one strip over three ranks, the run takes the gathered path, and only rank 0
    writes;
  * one rank, no process group: the rank-local writer gives the bytes of the default path;
  * world 2 without a process group is refused before any file is read.
All comparisons are exact.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import resident_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW = (300, 64)
PRODUCTS = (("mean", np.float32), ("std", np.float32), ("good", np.uint16))


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """Input folders: 300 x 256 as cases.write_inputs writes it, and its first 64 columns (cases.raster places its holes at
    columns past 128, so it cannot make a raster that narrow itself) written the same way."""
    from moonsuperresolution_amd import geotiff as G
    out = {name: str(tmp_path_factory.mktemp(f"halo_in_{name}")) for name in ("wide", "narrow")}
    img, dem = cases.write_inputs(out["wide"], cases.SHAPES["wide"])
    for file, a in (("run-DRG.tif", img), ("run-DEM.tif", dem)):
        G.write_geotiff(os.path.join(out["narrow"], file), np.ascontiguousarray(a[:, :NARROW[1]]), nodata=cases.NOVAL)
    return out


def run_ranks(tmp, world, job_cases):
    """Start ``world`` workers on the cases, wait for them (each under its own time limit) and return (job, reports by rank).
    Nothing more is started once a child has failed: the first failure ends the test."""
    os.makedirs(tmp, exist_ok=True)
    job = {"cases": [dict(c, **{products: [os.path.join(tmp, f"{c['name']}_{products}_rank{r}") for r in range(world)]
                                for products in ("gathered", "rank0")}) for c in job_cases]}
    for case in job["cases"]:
        for products in ("gathered", "rank0"):
            for save in case[products]:
                os.makedirs(save)
    with open(os.path.join(tmp, "job.json"), "w") as f:
        json.dump(job, f)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "halo_rank0_worker.py"),
                                       os.path.join(tmp, "job.json"), os.path.join(tmp, f"out{rank}.json")], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        logs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    return job, [json.load(open(os.path.join(tmp, f"out{rank}.json"))) for rank in range(world)]


@pytest.fixture(scope="module")
def two_ranks(hip_lib, folders, tmp_path_factory):
    """One pair of workers for the three two-rank cases."""
    switches = {"device": {}, "host": {}, "rank_band": {"batching": "rank", "accumulate": "band"}}
    job, reports = run_ranks(str(tmp_path_factory.mktemp("halo_two") / "run"), 2,
                             [{"name": name, "folder": folders["wide"], "stage": "host" if name == "host" else "device",
                               "switches": sw} for name, sw in switches.items()])
    return {c["name"]: c for c in job["cases"]}, reports


def plans_of(shape, world):
    from moonsuperresolution_amd.distributed import halo_strip_plan
    return {name: halo_strip_plan(shape, np.dtype(dt).itemsize, cases.S, cases.STRIDE, cases.T, world) for name, dt in PRODUCTS}


def check_same_files(case, world, shape):
    from moonsuperresolution_amd import geotiff as G
    want, got = cases.product_bytes(case["gathered"][0]), cases.product_bytes(case["rank0"][0])
    good, _ = G.read_geotiff(os.path.join(case["gathered"][0], "m_good.tiff"))
    assert good.shape == tuple(shape) and good.any()                          # the reference is a map, not an empty file
    for product, _ in PRODUCTS:
        assert want[product] is not None, product
        assert got[product] == want[product], (case["name"], product)
    for rank in range(1, world):
        assert os.listdir(case["rank0"][rank]) == [], (case["name"], rank)       # the other ranks wrote nothing
        assert cases.product_bytes(case["gathered"][rank]) == want                # ... where the default path writes on each


@pytest.mark.parametrize("name", ["device", "host", "rank_band"])
def test_two_ranks_one_writer(two_ranks, name):
    by_name, reports = two_ranks
    case = by_name[name]
    plans = plans_of(cases.SHAPES["wide"], 2)
    assert all(p["local"] for p in plans.values())
    assert plans["mean"]["take"][0] == plans["good"]["take"][0] == (208, 256)      # rows do change hands in this case
    for rank in range(2):
        rep = reports[rank][name]
        assert rep["gathered"]["products_path"] == "gathered" and rep["rank0"]["products_path"] == "rank0", (rank, rep)
        assert rep["gathered"]["handover_rows"] == {}
        assert rep["rank0"]["handover_rows"] == {product: [list(p["give"][rank]), list(p["take"][rank])]
                                                 for product, p in plans.items()}, (rank, rep)
        if case["stage"] == "device":                                            # no product raster came down
            assert rep["rank0"]["product_bytes_down"] == 0, (rank, rep)
        else:                                                                    # the rows of the rank's strips, once
            w = cases.SHAPES["wide"][1]
            rows = {product: min(p["strips"][rank][1] * p["rps"], 300) - p["strips"][rank][0] * p["rps"]
                    for product, p in plans.items()}
            assert rep["rank0"]["product_bytes_down"] == w * (4 * rows["mean"] + 4 * rows["std"] + rows["good"]), (rank, rep)
    check_same_files(case, 2, cases.SHAPES["wide"])


def test_three_ranks_fall_back_to_the_gathered_path(hip_lib, folders, tmp_path):
    plans = plans_of(NARROW, 3)
    assert plans["mean"]["local"] and not plans["good"]["local"]
    job, reports = run_ranks(str(tmp_path / "run"), 3, [{"name": "narrow", "folder": folders["narrow"], "stage": "device",
                                                         "switches": {}}])
    for rank in range(3):
        rep = reports[rank]["narrow"]
        assert rep["rank0"]["products_path"] == "gathered" and rep["rank0"]["handover_rows"] == {}, (rank, rep)
    check_same_files(job["cases"][0], 3, NARROW)


def test_one_rank_without_a_process_group(hip_lib, folders, tmp_path):
    from moonsuperresolution_amd import Generator, HaloShardedSuperResolution
    gen = Generator(cases.S, cases.B, weights=11, sampler="counter", seed=5)
    files = {}
    for products in ("gathered", "rank0"):
        save = str(tmp_path / products)
        d = HaloShardedSuperResolution(cases.cfg(source_folder_path=folders["wide"], save_path=save, map_name="m"), model=gen,
                                       decoder="device", infill="device", encoder="device")
        d.processFiles(preprocess=True, swap_dsize=False, mode="halo", products=products, world=1)
        assert d.products_path == products
        if products == "rank0":
            assert d.handover_rows == {name: ((0, 0), (300, 300)) for name, _ in PRODUCTS}
            assert sum(n for way, n, what in d.transfers if way == "d2h" and "product" in what) == 0
        d.close()
        files[products] = cases.product_bytes(save)
    gen.close()
    assert all(b is not None and len(b) > 1000 for b in files["gathered"].values())
    assert files["rank0"] == files["gathered"]


def test_more_ranks_need_a_process_group(hip_lib, tmp_path):
    """Refused before any file is read: the source folder does not exist."""
    from moonsuperresolution_amd import HaloShardedSuperResolution
    d = HaloShardedSuperResolution(cases.cfg(source_folder_path=str(tmp_path / "none"), save_path=str(tmp_path / "out"),
                                             map_name="m"), model=cases.f32_identity)
    with pytest.raises(RuntimeError, match="products='rank0' needs an initialised process group"):
        d.processFiles(mode="halo", products="rank0", world=2)
    with pytest.raises(ValueError, match="resident=True is not built for the halo mode"):
        HaloShardedSuperResolution(cases.cfg(), resident=True)
    d.close()

"""GPU (-m gpu): processFiles(mode="tiles", products="rank0") in two fresh child processes on one device over gloo (the manner
of tests/test_gpu_multiprocess.py; at most two children hold the GPU beside this process).

  * 300 x 256: no strip straddles the rank boundary (strips of 64 and 128 rows, T = 128), so each rank encodes the strips of
    its own rows and rank 0 writes: the three files equal the one-process files byte for byte, ``products_path == "rank0"``, and
    rank 1's save folder — a different one — stays empty;
  * 300 x 300: strips of 54 rows straddle, the run takes the gathered path, ``products_path == "gathered"``; the files are the
    same again and only rank 0 has written;
  * once with resident=True and every stage on the device (no product raster is downloaded on the rank-local path), once with
    resident=False and every stage on the host.
All comparisons are exact.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

from tests import resident_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2


@pytest.fixture(scope="module")
def one_process(hip_lib, tmp_path_factory):
    """{(shape name, stage): product bytes} of the one-process processFiles, and the input folders."""
    from moonsuperresolution_amd import DEMSuperResolution, Generator
    gen = Generator(cases.S, cases.B, weights=11, sampler="counter", seed=5)
    folders, files = {}, {}
    for name in ("wide", "odd"):
        folders[name] = str(tmp_path_factory.mktemp(f"in_{name}"))
        cases.write_inputs(folders[name], cases.SHAPES[name])
        for stage in ("device", "host"):
            save = str(tmp_path_factory.mktemp(f"one_{name}_{stage}"))
            d = DEMSuperResolution(cases.cfg(source_folder_path=folders[name], save_path=save, map_name="m"), model=gen,
                                   decoder=stage, infill=stage, encoder=stage)
            d.processFiles(preprocess=True, swap_dsize=False)
            d.close()
            files[name, stage] = cases.product_bytes(save)
            assert all(b is not None and len(b) > 1000 for b in files[name, stage].values())
    gen.close()
    return folders, files


@pytest.mark.parametrize("resident,stage", [(True, "device"), (False, "host")], ids=["resident-device", "host"])
def test_two_ranks_one_writer(tmp_path, one_process, resident, stage):
    folders, files = one_process
    job = {"resident": resident, "stage": stage, "cases": [
        {"name": name, "folder": folders[name], "save": [str(tmp_path / f"{name}_rank{r}") for r in range(WORLD)]}
        for name in ("wide", "odd")]}
    for case in job["cases"]:
        for save in case["save"]:
            os.makedirs(save)
    with open(tmp_path / "job.json", "w") as f:
        json.dump(job, f)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for rank in range(WORLD):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(WORLD), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "rank0_worker.py"), str(tmp_path / "job.json"),
                                       str(tmp_path / f"out{rank}.json")], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    try:
        logs = [p.communicate(timeout=300)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    reports = [json.load(open(tmp_path / f"out{rank}.json")) for rank in range(WORLD)]
    for case, path in zip(job["cases"], ("rank0", "gathered")):
        name = case["name"]
        for rank in range(WORLD):
            assert reports[rank][name]["products_path"] == path, (name, rank, reports[rank])
        got = cases.product_bytes(case["save"][0])
        for product in ("mean", "std", "good"):
            assert got[product] == files[name, stage][product], (name, product)
        assert os.listdir(case["save"][1]) == [], name          # the other rank wrote nothing
    if resident:                                                  # rank-local, device encoder: no product raster came down
        assert [r["wide"]["product_bytes_down"] for r in reports] == [0, 0]

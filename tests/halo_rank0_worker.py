"""One rank of tests/test_gpu_halo_products_rank0.py: processFiles(mode="halo") over gloo on device 0, per case first with
products="gathered" (the reference: every rank writes) and then with products="rank0", into different save folders.

    python halo_rank0_worker.py <json in> <json out>      with RANK, WORLD_SIZE, MASTER_ADDR and MASTER_PORT in the environment

The input names, per case, the source folder, this rank's two save folders and the switches; the output records, per case, which
product path ran, what was handed over and how many product bytes came down.  Started as a fresh process by the test (never an
exec of a process that has touched the GPU).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    from moonsuperresolution_amd import Generator, HaloShardedSuperResolution
    from tests import resident_cases as cases
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    job = json.load(open(sys.argv[1]))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    gen = Generator(cases.S, cases.B, weights=11, sampler="counter", seed=5)
    out = {}
    for case in job["cases"]:
        stage = case["stage"]
        report = {}
        for products in ("gathered", "rank0"):
            d = HaloShardedSuperResolution(cases.cfg(source_folder_path=case["folder"], save_path=case[products][rank],
                                                     map_name="m"), model=gen, decoder=stage, infill=stage, encoder=stage)
            d.processFiles(preprocess=True, swap_dsize=False, mode="halo", rank=rank, world=world, products=products,
                           **case["switches"])
            torch.cuda.synchronize()
            report[products] = {"products_path": d.products_path, "handover_rows": d.handover_rows,
                                "product_bytes_down": sum(n for way, n, what in d.transfers
                                                          if way == "d2h" and "product" in what)}
            d.close()
        out[case["name"]] = report
    dist.barrier()
    dist.destroy_process_group()
    gen.close()
    with open(sys.argv[2], "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()

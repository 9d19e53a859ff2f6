"""Diagnostic (not a pytest): the float32 products with the horizontal and with the floating-point predictor, device encoder,
on one GPU.
    python3 tools/gpu_geotiff_pred3_bench.py [--out profiles/geotiff_pred3.json] [--reps 3] [--rows 4096 --cols 16384]
The float32 DEM-like raster of tools/gpu_geotiff_encode_bench.py (4096 x 16384), already on the device as the resident driver
hands it over, written with geotiff.write_geotiff(encoder="device") in four variants: predictor 2 and predictor 3, each as
strips and as layout="cog" with tile=(256, 256) and 4 overviews.  One process; after a warm-up of every variant the four
alternate ``--reps`` times; the medians and spreads (max - min) of the wall times are recorded, the file sizes, what predictor
3 costs or saves in time against predictor 2 of the same layout, the size ratio, and whether the predictor-3 files of the
device encoder are the host encoder's (they must be).  No threshold is set: a time difference counts only beyond the larger
of the two variants' spreads, and ``time_difference_beyond_spread`` says whether it does."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LAYOUTS = {"strips": {}, "cog_ov4": dict(tile=(256, 256), overviews=4, layout="cog")}
VARIANTS = {f"{name}_p{p}": dict(how, predictor=p) for name, how in LAYOUTS.items() for p in (2, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/geotiff_pred3.json")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--cols", type=int, default=16384)
    args = ap.parse_args()
    import torch
    from gpu_geotiff_encode_bench import product
    from moonsuperresolution_amd import geotiff as G
    dev = torch.device("cuda", 0)
    data = product(args.rows, args.cols, "f32")
    tensor = torch.from_numpy(data).to(dev)
    torch.cuda.synchronize()
    times = {v: [] for v in VARIANTS}
    sizes, same = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        def write(v):
            t0 = time.perf_counter()
            G.write_geotiff(os.path.join(tmp, v + ".tif"), tensor, nodata=-32768.0, encoder="device", **VARIANTS[v])
            return time.perf_counter() - t0

        for v in VARIANTS:                                   # warm-up: code objects, the allocator's blocks, the page cache
            write(v)
            sizes[v] = os.path.getsize(os.path.join(tmp, v + ".tif"))
        for rep in range(args.reps):
            for v in VARIANTS:
                times[v].append(write(v))
                print(f"rep {rep} {v}: {times[v][-1]:.3f} s", flush=True)
        for name in LAYOUTS:
            v = name + "_p3"
            t0 = time.perf_counter()
            G.write_geotiff(os.path.join(tmp, "host.tif"), data, nodata=-32768.0, **VARIANTS[v])
            host_s = time.perf_counter() - t0
            with open(os.path.join(tmp, "host.tif"), "rb") as a, open(os.path.join(tmp, v + ".tif"), "rb") as b:
                same[v] = a.read() == b.read()
            print(f"host {v}: {host_s:.3f} s, identical {same[v]}", flush=True)
    rec = {"tool": "tools/gpu_geotiff_pred3_bench.py", "reps": args.reps, "shape": [args.rows, args.cols], "dtype": "float32",
           "raw_bytes": int(data.nbytes), "tile_of_cog": [256, 256], "variants": {}, "predictor_3_against_2": {}}
    for v in VARIANTS:
        t = times[v]
        rec["variants"][v] = {"wall_s": t, "median_s": statistics.median(t), "spread_s": max(t) - min(t), "file_bytes": sizes[v]}
    for name in LAYOUTS:
        p2, p3 = rec["variants"][name + "_p2"], rec["variants"][name + "_p3"]
        spread = max(p2["spread_s"], p3["spread_s"])
        diff = p3["median_s"] - p2["median_s"]
        rec["predictor_3_against_2"][name] = {"median_difference_s": diff, "larger_spread_s": spread,
                                              "time_difference_beyond_spread": abs(diff) > spread,
                                              "size_ratio": p3["file_bytes"] / p2["file_bytes"]}
    rec["host_and_device_identical"] = same
    print(json.dumps(rec), flush=True)
    path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

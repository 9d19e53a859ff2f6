"""Diagnostic (not a pytest): tiled GeoTIFF products in the two file orders, device encoder, on one GPU.
    python3 tools/gpu_geotiff_cog_bench.py [--out profiles/geotiff_cog.json] [--reps 3] [--rows 4096 --cols 16384]
The float32 DEM-like raster of tools/gpu_geotiff_encode_bench.py (4096 x 16384, the one of profiles/geotiff_tiled.json),
already on the device as the resident driver hands it over, written with geotiff.write_geotiff(encoder="device",
tile=(256, 256)) in four variants: layout="plain" with 0 and with 4 overviews (the padded frame, the tile-major copy and one
encode launch per band of every level) and layout="cog" with 0 and with 4 overviews (the tiles read in place, the tiles of
all reduced levels in one launch).  One process; after a warm-up of every variant the four alternate ``--reps`` times; the
medians and spreads (max - min) of the wall times are recorded, torch.cuda.max_memory_allocated of a write of each variant,
the file sizes, the number of encode launches, and whether the cog file of the device encoder is the host encoder's (it must
be).  A difference between two variants counts only beyond the larger of their spreads."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

VARIANTS = {"plain_ov0": dict(layout="plain", overviews=0), "plain_ov4": dict(layout="plain", overviews=4),
            "cog_ov0": dict(layout="cog", overviews=0), "cog_ov4": dict(layout="cog", overviews=4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/geotiff_cog.json")
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
    held = torch.cuda.memory_allocated()
    times = {v: [] for v in VARIANTS}
    peak, sizes, launches = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        def write(v, log=None):
            t0 = time.perf_counter()
            G.write_geotiff(os.path.join(tmp, v + ".tif"), tensor, nodata=-32768.0, encoder="device", tile=(256, 256), transfers=log,
                            **VARIANTS[v])
            return time.perf_counter() - t0

        for v in VARIANTS:                                   # warm-up: code objects, the allocator's blocks, the page cache
            log = []
            torch.cuda.reset_peak_memory_stats()
            write(v, log)
            peak[v] = torch.cuda.max_memory_allocated() - held
            sizes[v] = os.path.getsize(os.path.join(tmp, v + ".tif"))
            launches[v] = sum(1 for _, _, what in log if "tables" in what)
        for rep in range(args.reps):
            for v in VARIANTS:
                times[v].append(write(v))
                print(f"rep {rep} {v}: {times[v][-1]:.3f} s", flush=True)
        t0 = time.perf_counter()
        G.write_geotiff(os.path.join(tmp, "host.tif"), data, nodata=-32768.0, tile=(256, 256), **VARIANTS["cog_ov4"])
        host_s = time.perf_counter() - t0
        with open(os.path.join(tmp, "host.tif"), "rb") as a, open(os.path.join(tmp, "cog_ov4.tif"), "rb") as b:
            same = a.read() == b.read()
        print(f"host cog_ov4: {host_s:.3f} s, identical {same}", flush=True)
    rec = {"tool": "tools/gpu_geotiff_cog_bench.py", "reps": args.reps, "shape": [args.rows, args.cols], "dtype": "float32",
           "raw_bytes": int(data.nbytes), "tile": [256, 256], "raster_held_bytes": int(held), "variants": {}}
    for v in VARIANTS:
        t = times[v]
        rec["variants"][v] = {"wall_s": t, "median_s": statistics.median(t), "spread_s": max(t) - min(t), "file_bytes": sizes[v],
                              "encode_launches": launches[v], "peak_device_bytes_above_the_raster": int(peak[v])}
    med = {v: rec["variants"][v]["median_s"] for v in VARIANTS}
    spread = max(rec["variants"][v]["spread_s"] for v in VARIANTS)
    rec["larger_spread_s"] = spread
    rec["overview_bytes_over_level0"] = {k: sizes[k + "_ov4"] / sizes[k + "_ov0"] - 1.0 for k in ("plain", "cog")}
    rec["overview_time_over_level0"] = {k: med[k + "_ov4"] / med[k + "_ov0"] - 1.0 for k in ("plain", "cog")}
    rec["cog_minus_plain_s"] = {ov: med["cog_" + ov] - med["plain_" + ov] for ov in ("ov0", "ov4")}
    rec["host_and_device_identical"] = same
    print(json.dumps(rec), flush=True)
    path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""gpu_resident_bench.py — wall time of processFiles phase by phase, resident=False against resident=True, in one process.

    python tools/gpu_resident_bench.py                          # 2048 x 3072, S=256 s=32 B=16, f16c Generator, all stages on
                                                                # the device; three alternations; writes profiles/resident.json
    python tools/gpu_resident_bench.py --rows 4096 --cols 16384 --no-preprocess --key large
    python tools/gpu_resident_bench.py --single resident        # ONE processFiles and its ``transfers`` sums: the program of a
                                                                # memory-copy trace (rocprofv3 --memory-copy-trace -- python ...)
    python tools/gpu_resident_bench.py --copy-trace DIR --key copy_trace_resident
                                                                # sum a rocprofv3 --memory-copy-trace CSV under DIR into the JSON

The phases are loadImages, preprocess, padInputs, the tile loop (mapTiles) and the three saveGTiff calls, each ended by a device
synchronisation; the two modes alternate so that clock ramp and page cache hit both alike.  Reported per phase and mode: the
three times, their median and spread (max - min); the difference of the medians is stated only where it exceeds the larger
spread.  Peak torch allocation and the ``transfers`` sums per direction go into the same file.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import sys
import tempfile
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "resident.json")
PHASES = ("load", "preprocess", "pad", "tiles", "save")


def merge(key, value):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data[key] = value
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def sums(log):
    out = {"h2d": 0, "d2h": 0}
    for way, n, _ in log:
        out[way] += n
    return out


def copy_trace(folder):
    """Bytes per direction of every *memory_copy_trace.csv under ``folder`` (the columns are found by name)."""
    out, files = {}, sorted(glob.glob(os.path.join(folder, "**", "*memory_copy_trace.csv"), recursive=True))
    columns = None
    for path in files:
        with open(path, newline="") as f:
            rows = csv.DictReader(f)
            columns = rows.fieldnames
            way = next((c for c in columns if "direction" in c.lower()), None)
            size = next((c for c in columns if c.lower() in ("bytes", "size", "size_bytes") or "bytes" in c.lower()), None)
            for row in rows:
                k = row.get(way, "all") if way else "all"
                rec = out.setdefault(k, {"copies": 0, "bytes": 0 if size else None})
                rec["copies"] += 1
                if size:
                    rec["bytes"] += int(float(row[size]))
    return {"files": [os.path.relpath(p, folder) for p in files], "columns": columns, "by_direction": out}


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--cols", type=int, default=3072)
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--stride", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--no-preprocess", dest="preprocess", action="store_false")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--key", default="raster")
    ap.add_argument("--single", choices=("resident", "host"), default=None)
    ap.add_argument("--copy-trace", default=None)
    ap.add_argument("--out", default=OUT, help="the JSON file the record is merged into")
    args = ap.parse_args()
    OUT = os.path.abspath(args.out)
    if args.copy_trace:
        merge(args.key, copy_trace(args.copy_trace))
        print(json.dumps({args.key: json.load(open(OUT))[args.key]}))
        return

    import numpy as np
    import torch
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, Generator
    from moonsuperresolution_amd import geotiff as G
    from raster_bench import synthetic_raster

    S, s, B = args.image_size, args.stride, args.batch_size
    work = tempfile.mkdtemp(prefix="resident_bench_")
    src = os.path.join(work, "in")
    os.makedirs(src)
    img, dem = synthetic_raster(args.rows, args.cols, seed=0)
    img = np.round(img * 256.0) / 256.0                 # quantised like real 8 / 16-bit sources, so that LZW has something to do
    dem = np.round(dem * 4.0) / 4.0
    dem[args.rows // 3:args.rows // 3 + 3, 500:503] = -32768.0
    G.write_geotiff(os.path.join(src, "run-DRG.tif"), img.astype(np.float32), nodata=-32768.0)
    G.write_geotiff(os.path.join(src, "run-DEM.tif"), dem.astype(np.float32), nodata=-32768.0)
    in_bytes = sum(os.path.getsize(os.path.join(src, f)) for f in os.listdir(src))
    del img, dem
    gen = Generator(S, B, variant="gaugan", weights=1234, eps=7, precision="f16c")

    def driver(resident, tag):
        cfg = DSRConfig(image_size=S, stride=s, batch_size=B, tile_size=1024, source_folder_path=src,
                        save_path=os.path.join(work, tag), map_name="m")
        return DEMSuperResolution(cfg, model=gen, decoder="device", infill="device", encoder="device", resident=resident)

    def sync():
        torch.cuda.synchronize()

    def phases(d):
        """processFiles, phase by phase."""
        del d.transfers[:]
        t = {}
        torch.cuda.reset_peak_memory_stats()
        sync()
        t0 = time.perf_counter()
        d.loadImages()
        sync()
        t["load"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        if args.preprocess:
            d.preprocess(swap_dsize=False)
        sync()
        t["preprocess"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        d.padInputs()
        sync()
        t["pad"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        products = d.mapTiles(d.generateTileList())
        sync()
        t["tiles"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        for data, name in zip(products, ("mean", "std", "good")):
            d.saveGTiff(data, data.dtype, name)
        sync()
        t["save"] = time.perf_counter() - t0
        t["total"] = sum(t.values())
        return t, torch.cuda.max_memory_allocated(), sums(d.transfers)

    if args.single:
        d = driver(args.single == "resident", args.single)
        d.processFiles(preprocess=args.preprocess, swap_dsize=False)
        sync()
        out_bytes = sum(os.path.getsize(os.path.join(work, args.single, f)) for f in os.listdir(os.path.join(work, args.single)))
        rec = {"mode": args.single, "raster": [args.rows, args.cols], "transfers": sums(d.transfers),
               "input_file_bytes": in_bytes, "output_file_bytes": out_bytes, "raw_raster_bytes": args.rows * args.cols * 4}
        merge(args.key, rec)
        print(json.dumps(rec))
        d.close()
        gen.close()
        shutil.rmtree(work, ignore_errors=True)
        return

    modes = {"host": driver(False, "host"), "resident": driver(True, "resident")}
    phases(modes["host"])                               # warm-up: streams, clones, buffers, clocks, page cache
    runs = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m, d in modes.items():
            runs[m].append(phases(d))
    same = all(open(os.path.join(work, "host", f), "rb").read() == open(os.path.join(work, "resident", f), "rb").read()
               for f in os.listdir(os.path.join(work, "host")))
    rec = {"raster": [args.rows, args.cols], "image_size": S, "stride": s, "batch_size": B, "precision": "f16c",
           "stages": "decoder, infill, encoder = device", "preprocess": args.preprocess, "rounds": args.rounds,
           "files_equal": same, "input_file_bytes": in_bytes, "raw_raster_bytes": args.rows * args.cols * 4,
           "output_file_bytes": sum(os.path.getsize(os.path.join(work, "resident", f))
                                    for f in os.listdir(os.path.join(work, "resident"))),
           "seconds": {}, "difference_resident_minus_host": {}}
    for m in modes:
        rec["seconds"][m] = {}
        for p in PHASES + ("total",):
            v = [r[0][p] for r in runs[m]]
            rec["seconds"][m][p] = {"runs": v, "median": float(np.median(v)), "spread": max(v) - min(v)}
        rec[f"peak_allocated_bytes_{m}"] = max(r[1] for r in runs[m])
        rec[f"transfers_{m}"] = runs[m][-1][2]
    for p in PHASES + ("total",):
        a, b = rec["seconds"]["host"][p], rec["seconds"]["resident"][p]
        diff, spread = b["median"] - a["median"], max(a["spread"], b["spread"])
        rec["difference_resident_minus_host"][p] = {"seconds": diff, "larger_spread": spread,
                                                    "verdict": "within the spread" if abs(diff) <= spread else
                                                    ("resident slower" if diff > 0 else "resident faster")}
    merge(args.key, rec)
    print(json.dumps(rec))
    for d in modes.values():
        d.close()
    gen.close()
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()

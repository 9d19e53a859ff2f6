"""Diagnostic (not a pytest): strip, tiled and tiled-with-overviews GeoTIFF products, host and device encoder, on one GPU.
    python3 tools/gpu_geotiff_tiled_bench.py [--out profiles/geotiff_tiled.json] [--reps 3] [--rows 4096 --cols 16384]
The two products of tools/gpu_geotiff_encode_bench.py (a 4096 x 16384 float32 DEM-like raster, the uint16 `good`-like one of
the same shape), each written with geotiff.write_geotiff to a temporary file in three layouts — strips (the code as it was:
the baseline), 256 x 256 tiles, tiles with 4 overviews — by both encoders (the device one from a tensor already on the device,
as the resident driver hands it over).  One process; the six variants of a product alternate ``--reps`` times; medians and
spreads (max - min) of the wall times are recorded, the file sizes, and whether the host and the device file of a layout
are the same bytes (they must be).  A difference between two variants counts only beyond the larger of their spreads.

Also the msr_overview_half launch alone (level 0 -> level 1 of each product) between two HIP events: bytes read plus written
over the time, beside the 6.29 TB/s a float4 copy reaches on this part (8.0 TB/s spec)."""
import argparse
import ctypes as C
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

HBM_COPY_TBPS, HBM_SPEC_TBPS = 6.29, 8.0
LAYOUTS = {"strips": {}, "tiles": dict(tile=(256, 256)), "tiles_ov4": dict(tile=(256, 256), overviews=4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/geotiff_tiled.json")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--cols", type=int, default=16384)
    args = ap.parse_args()
    import torch
    from gpu_geotiff_encode_bench import product
    from moonsuperresolution_amd import _lib
    from moonsuperresolution_amd import geotiff as G
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        G.write_geotiff(os.path.join(tmp, "warm.tif"), np.zeros((64, 64), np.float32), encoder="device", device=dev,
                        tile=(16, 16), overviews=1)                                      # runtime start-up
        for name, kind in (("dem_f32", "f32"), ("good_u16", "u16")):
            data = product(args.rows, args.cols, kind)
            dtype = data.dtype
            tensor = torch.from_numpy(data.view(np.int16) if kind == "u16" else data).to(dev)
            torch.cuda.synchronize()
            times = {(lay, enc): [] for lay in LAYOUTS for enc in ("host", "device")}
            sizes, same = {}, {}
            for rep in range(args.reps):
                for lay, kw in LAYOUTS.items():
                    for enc in ("host", "device"):
                        path = os.path.join(tmp, f"{lay}_{enc}.tif")
                        src = data if enc == "host" else tensor
                        t0 = time.perf_counter()
                        G.write_geotiff(path, src, nodata=-32768.0, dtype=dtype, encoder=enc, **kw)
                        times[(lay, enc)].append(time.perf_counter() - t0)
                        print(f"{name} rep {rep} {lay} {enc}: {times[(lay, enc)][-1]:.3f} s", flush=True)
                    if rep == 0:
                        files = [open(os.path.join(tmp, f"{lay}_{enc}.tif"), "rb").read() for enc in ("host", "device")]
                        sizes[lay], same[lay] = len(files[0]), files[0] == files[1]
                        del files
            rec = {"case": name, "shape": [args.rows, args.cols], "dtype": str(dtype), "raw_bytes": int(data.nbytes), "layouts": {}}
            for lay in LAYOUTS:
                rec["layouts"][lay] = {"file_bytes": sizes[lay], "host_and_device_identical": same[lay]}
                for enc in ("host", "device"):
                    t = times[(lay, enc)]
                    rec["layouts"][lay][enc] = {"wall_s": t, "median_s": statistics.median(t), "spread_s": max(t) - min(t)}
            rec["overview_bytes_over_level0"] = sizes["tiles_ov4"] / sizes["tiles"] - 1.0
            # the reduction alone: level 0 -> level 1
            rows, cols, sb = args.rows, args.cols, dtype.itemsize
            nxt = torch.empty((-(-rows // 2), -(-cols // 2)), dtype=tensor.dtype, device=dev)
            s = torch.cuda.current_stream(dev)
            ms = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = lib.msr_overview_half(None, tensor.data_ptr(), rows, cols, ord("f" if kind == "f32" else "u"), sb,
                                           int(kind == "f32"), -32768.0, nxt.data_ptr(), C.c_void_p(s.cuda_stream))
                b.record()
                _lib.raise_for(lib, None, rc, "msr_overview_half")
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            moved = rows * cols * sb + nxt.numel() * sb
            warm = ms[1:]                                                     # the first launch loads the code object
            rec["overview_half"] = {"ms": ms, "median_ms_after_first": statistics.median(warm), "bytes_read_plus_written": moved,
                                    "TBps": moved / (statistics.median(warm) * 1e-3) / 1e12,
                                    "hbm_float4_copy_TBps": HBM_COPY_TBPS, "hbm_spec_TBps": HBM_SPEC_TBPS}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del tensor, nxt
    out = {"tool": "tools/gpu_geotiff_tiled_bench.py", "reps": args.reps, "cases": records}
    path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0 if all(v["host_and_device_identical"] for r in records for v in r["layouts"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())

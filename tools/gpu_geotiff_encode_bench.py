"""Diagnostic (not a pytest): GeoTIFF strip encoding on the host and on the device, on one GPU.
    python3 tools/gpu_geotiff_encode_bench.py [--out profiles/geotiff_encode.json] [--limit 600]
Three synthetic products: a 4096 x 16384 float32 DEM-like raster (smooth relief + 5 cm noise: one 64 KiB strip per row), a
uint16 `good`-like raster of the same shape (two rows per strip), and 2048 rows of 70000 float32 samples (the width of
BASELINE configs[3]: one 280000-byte strip per row).  For each: the wall time of geotiff.write_geotiff to a temporary
file with encoder="host" (csrc/host_codecs.cpp, single-threaded) and with encoder="device" (csrc/geotiff_codec.hip; from
the NumPy array, upload and download included, and again from a tensor already on the device), the time of the
msr_lzw_encode_strips launch alone between two HIP events, the compressed size, and whether the two files are the same
bytes (they must be).

Without --case the script touches no GPU itself: it runs each case as a child process under a time limit of its own and
stops at the first one that fails or runs out of time."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"dem_f32": (4096, 16384, "f32"), "good_u16": (4096, 16384, "u16"), "wide_f32": (2048, 70000, "f32")}


def product(rows, cols, kind):
    """DEM-like: relief of a few hundred metres over wavelengths of hundreds of pixels + 5 cm of noise.  good-like: the
    count of estimates per pixel, a plateau with a lower rim and a few holes."""
    rng = np.random.default_rng(2024)
    y = np.arange(rows, dtype=np.float64)[:, None]
    x = np.arange(cols, dtype=np.float64)[None, :]
    if kind == "f32":
        z = -2000 + 600 * np.sin(x / 370.0) * np.cos(y / 530.0) + 300 * np.sin((x + 2 * y) / 910.0)
        return (z + 0.05 * rng.standard_normal((rows, cols))).astype(np.float32)
    g = np.full((rows, cols), 16, np.uint16)
    g[:48] = 8; g[-48:] = 8; g[:, :48] = 8; g[:, -48:] = 8
    for _ in range(40):
        r, c = int(rng.integers(0, rows - 64)), int(rng.integers(0, cols - 64))
        g[r:r + 64, c:c + 64] = 0
    return g


def run_case(name):
    import torch
    from moonsuperresolution_amd import geotiff as G
    rows, cols, kind = CASES[name]
    data = product(rows, cols, kind)
    dtype = data.dtype
    dev = torch.device("cuda", 0)
    rec = {"case": name, "shape": [rows, cols], "dtype": str(dtype), "raw_bytes": int(data.nbytes)}
    with tempfile.TemporaryDirectory() as tmp:
        hp, dp, tp = (os.path.join(tmp, f) for f in ("host.tif", "device.tif", "tensor.tif"))
        G.write_geotiff(os.path.join(tmp, "warm.tif"), data[:64], dtype=dtype, encoder="device", device=dev)   # runtime start-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G.write_geotiff(dp, data, dtype=dtype, encoder="device", device=dev)
        rec["device_wall_s"] = time.perf_counter() - t0
        td = torch.from_numpy(data.view(np.int16) if kind == "u16" else data).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G.write_geotiff(tp, td, dtype=dtype, encoder="device")
        rec["device_wall_from_tensor_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        G.write_geotiff(hp, data, dtype=dtype, encoder="host")
        rec["host_wall_s"] = time.perf_counter() - t0
        files = [open(p, "rb").read() for p in (hp, dp, tp)]
        rec["file_bytes"] = len(files[0])
        rec["identical"] = files[0] == files[1] == files[2]
        # the launch alone, the whole product in one go
        row_bytes = cols * dtype.itemsize
        rps = G._rows_per_strip(rows, row_bytes)
        starts = np.arange(0, rows, rps, dtype=np.int64)
        lengths = (np.minimum(starts + rps, rows) - starts) * row_bytes
        buf = td.contiguous().view(torch.uint8).reshape(-1)
        ms = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            # (the two small tables of offsets and lengths are uploaded between the events too)
            dst, dst_off, dst_len = G._encode_strips_device(buf, starts * row_bytes, lengths, dtype.itemsize, row_bytes)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        rec["n_strips"] = int(starts.size)
        rec["kernel_ms"] = ms
        rec["compressed_bytes"] = int(dst_len.sum().item())
        del dst
    rec["ratio"] = rec["compressed_bytes"] / rec["raw_bytes"]
    rec["host_MBps"] = rec["raw_bytes"] / rec["host_wall_s"] / 1e6
    rec["device_MBps"] = rec["raw_bytes"] / rec["device_wall_s"] / 1e6
    rec["kernel_GBps"] = rec["raw_bytes"] / (min(ms) * 1e-3) / 1e9
    rec["speedup_end_to_end"] = rec["host_wall_s"] / rec["device_wall_s"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/geotiff_encode.json")
    ap.add_argument("--limit", type=int, default=600, help="seconds a case may take")
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case)), flush=True)
        return 0
    records = []
    for name in CASES:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], capture_output=True, text=True,
                                 timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {args.limit} s; stopping", flush=True)
            return 1
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
        if res.returncode or not lines:
            print(f"{name}: exit status {res.returncode}; stopping\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}", flush=True)
            return 1
        records.append(json.loads(lines[-1][7:]))
        print(json.dumps(records[-1]), flush=True)
    out = {"tool": "tools/gpu_geotiff_encode_bench.py", "cases": records}
    path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0 if all(r["identical"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())

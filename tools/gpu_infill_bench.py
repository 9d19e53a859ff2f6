"""Diagnostic (not a pytest): the in-filling step of preprocess on the host and on the device, on one GPU.
    python3 tools/gpu_infill_bench.py [--out profiles/infill.json] [--rows 1024] [--cols 4096] [--repeats 3] [--cases sparse,every_tile]
Two DEM-like x1/4 bands of --rows x --cols float32 on the device, as the first area step leaves them:
  sparse      about one small hole (1 .. 22 pixels) per 2000 pixels and a few large ones;
  every_tile  one small hole in every 96 x 96 cell, so that each 256 x 256 in-fill tile holds several.
For each, in one process, alternating --repeats times so that the spread is on file:
  host    what preprocess._lowres_rows does with infill="host": download of the band, preprocess._fill_rows (griddata on every
          tile with a hole, single-threaded SciPy), upload of the filled rows;
  device  infill.infill_device in place (workspace allocation included), synchronised.
And the two stages of the device in-fill, each between HIP events of its own (msr_debug_infill_stage), the median of 5.
Both fill the same pixels with different values (infill.py), so the record also holds how many pixels each changed and the
largest difference between the two.  A progress line is printed per measurement.  Every case records its own band size; a
case already in --out that is not run again is kept (the host side of the default size takes minutes per repeat)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOVAL = -32768.0


def band(rows, cols, kind, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    g = (-2000.0 + 300.0 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 40.0 * np.sin(xx / 5.0 + yy / 7.0)).astype(np.float32)

    def grow(r, c, size):
        pix = [(min(max(r, 0), rows - 1), min(max(c, 0), cols - 1))]
        while len(pix) < size:
            br, bc = pix[int(rng.integers(len(pix)))]
            q = (min(max(br + int(rng.integers(-1, 2)), 0), rows - 1), min(max(bc + int(rng.integers(-1, 2)), 0), cols - 1))
            if q not in pix:
                pix.append(q)
        for p in pix:
            g[p] = NOVAL
    if kind == "sparse":
        for _ in range(rows * cols // 2000):
            grow(int(rng.integers(rows)), int(rng.integers(cols)), int(rng.integers(1, 23)))
        for _ in range(4):
            r, c = int(rng.integers(rows - 120)), int(rng.integers(cols - 300))
            g[r:r + int(rng.integers(40, 120)), c:c + int(rng.integers(60, 300))] = NOVAL
    else:
        for r in range(48, rows, 96):
            for c in range(48, cols, 96):
                grow(r + int(rng.integers(-20, 21)), c + int(rng.integers(-20, 21)), int(rng.integers(1, 23)))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infill.json"))
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="sparse,every_tile")
    args = ap.parse_args()
    import torch
    from moonsuperresolution_amd import infill, ops
    from moonsuperresolution_amd import preprocess as pp
    ctx = ops.OpContext()
    lib, h = ctx.lib, ctx.h
    rows, cols = args.rows, args.cols
    tiles = [t for t in range(0, rows, pp.FILL_TILE - 2 * pp.FILL_BORDER)
             if min(t + pp.FILL_TILE - pp.FILL_BORDER, rows - pp.FILL_BORDER) > t + pp.FILL_BORDER]
    record = {"what": "in-filling of an x1/4 band: host = download + preprocess._fill_rows (scipy griddata per tile) + upload; "
                      "device = msr_infill_small_holes in place; seconds, alternating in one process",
              "device_name": torch.cuda.get_device_name(0), "cases": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record["cases"] = json.load(f).get("cases", {})
    for kind, seed in (("sparse", 1), ("every_tile", 2)):
        if kind not in args.cases.split(","):
            continue
        g = band(rows, cols, kind, seed)
        dev = torch.from_numpy(g).cuda()
        torch.cuda.synchronize()
        host_s, dev_s = [], []
        host_out = dev_out = None
        for rep in range(args.repeats):
            d4 = dev.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            filled = pp._fill_rows(d4.cpu().numpy(), 0, rows, tiles, NOVAL)
            up = torch.from_numpy(np.ascontiguousarray(filled)).cuda()
            torch.cuda.synchronize()
            host_s.append(time.perf_counter() - t0)
            host_out = filled
            print(f"{kind} repeat {rep}: host {host_s[-1]:.3f} s", flush=True)
            del up
            d4 = dev.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            infill.infill_device(lib, h, d4, 0, rows, NOVAL, pp.FILL_AREA, pp.FILL_BORDER)
            torch.cuda.synchronize()
            dev_s.append(time.perf_counter() - t0)
            dev_out = d4.cpu().numpy()
            print(f"{kind} repeat {rep}: device {dev_s[-1] * 1e3:.3f} ms", flush=True)
        need = lib.msr_infill_workspace_bytes(rows, cols)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        stage_ms = {1: [], 2: []}
        for _ in range(5):
            d4 = dev.clone()
            for stage in (1, 2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = lib.msr_debug_infill_stage(h, d4.data_ptr(), 0, rows, rows, cols, NOVAL, pp.FILL_AREA, pp.FILL_BORDER,
                                                ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream, stage)
                b.record()
                assert rc == 0, lib.msr_last_error(h)
                torch.cuda.synchronize()
                stage_ms[stage].append(a.elapsed_time(b))
            assert np.array_equal(d4.cpu().numpy().view(np.uint32), dev_out.view(np.uint32))
        changed_h = host_out.view(np.uint32) != g.view(np.uint32)
        changed_d = dev_out.view(np.uint32) != g.view(np.uint32)
        both = changed_h & changed_d
        record["cases"][kind] = {
            "rows": rows, "cols": cols, "tiles": len(tiles) * len(range(0, cols, 192)), "hole_pixels": int((g <= NOVAL).sum()),
            "pixels_changed_host": int(changed_h.sum()), "pixels_changed_device": int(changed_d.sum()), "same_pixels": bool(np.array_equal(changed_h, changed_d)),
            "max_abs_difference_m": float(np.nanmax(np.abs(host_out[both].astype(np.float64) - dev_out[both]))) if both.any() else 0.0,
            "host_seconds": host_s, "device_seconds": dev_s,
            "host_min_max": [min(host_s), max(host_s)], "device_min_max": [min(dev_s), max(dev_s)],
            "label_stage_ms_median": float(np.median(stage_ms[1])), "solve_stage_ms_median": float(np.median(stage_ms[2])),
            "label_stage_ms": stage_ms[1], "solve_stage_ms": stage_ms[2], "workspace_bytes": int(need)}
        print(json.dumps({kind: record["cases"][kind]}), flush=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

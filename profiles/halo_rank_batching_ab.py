#!/usr/bin/env python3
"""Collector of profiles/halo_rank_batching.json: the halo mode's (batching="band", accumulate="blocks") — the code path as
it was — against (batching="rank", accumulate="band"), alternated in ONE process on one GPU.

    python profiles/halo_rank_batching_ab.py --out profiles/halo_rank_batching.json

The workload is raster_bench.py's `--halo --crop-inputs --max-rows 12 --band-rows 1 --simulate-rank 3 --simulate-world 8` on
the synthetic 15000 x 70000 raster at S = 512, s = 64, B = 8 (the geometry of profiles/halo_cropped_inputs.json): the same
raster, generator, handles and row window serve every run, so the pairs differ in the two keywords only.  One warm-up run per
form, then `--pairs` alternations; per run: seconds (haloAccumulate + haloFinish, synchronised), generator calls,
512 x 512-tile equivalents per second and the device time of the stitch per band (events around each band's accumulation).
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")       # as raster_bench.py: two generator handles, four streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=15000)
    ap.add_argument("--cols", type=int, default=70000)
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--stride", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--max-rows", type=int, default=12)
    ap.add_argument("--band-rows", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--precision", default="f16c")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from moonsuperresolution_amd import DSRConfig, Generator, HaloShardedSuperResolution
    from raster_bench import synthetic_raster

    S, s, B = args.image_size, args.stride, args.batch_size
    img, dem = synthetic_raster(args.rows, args.cols, seed=0)
    print("raster built", flush=True)
    gen = Generator(S, B, variant="gaugan", weights=1234, eps=7, precision=args.precision)
    hs = HaloShardedSuperResolution(DSRConfig(image_size=S, stride=s, batch_size=B, tile_size=1024), model=gen, pipeline=2)
    hs.setImages(img, dem)
    del img, dem
    forms = [("band", "blocks"), ("rank", "band")]

    def run(batching, accumulate):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = hs.haloAccumulate(args.rank, args.world, band_rows=args.band_rows, max_rows=args.max_rows, crop_inputs=True,
                               batching=batching, accumulate=accumulate)
        hs.haloFinish(st)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        nv, nc = hs.last_counts_halo
        stitch = hs.bandStitchSeconds()
        del st
        return {"batching": batching, "accumulate": accumulate, "seconds": sec, "patches": nv, "generator_calls": nc,
                "tiles512_per_s": nc * B * (S / 512.0) ** 2 / sec, "bands": len(stitch),
                "stitch_seconds_per_band": sum(stitch) / max(1, len(stitch)), "stitch_seconds": sum(stitch),
                "valid_per_band": [v for v, _ in hs.last_band_counts], "calls_per_band": [c for _, c in hs.last_band_counts]}

    for f in forms:                                   # warm-up: crop + pad + clone handles, clocks
        r = run(*f)
        print("warm-up", json.dumps({k: r[k] for k in ("batching", "accumulate", "seconds", "generator_calls")}), flush=True)
    runs = []
    for _ in range(args.pairs):
        for f in forms:
            runs.append(run(*f))
            print(json.dumps({k: v for k, v in runs[-1].items() if not k.endswith("_per_band") or k.startswith("stitch")}),
                  flush=True)
    per = {f: [r for r in runs if (r["batching"], r["accumulate"]) == f] for f in forms}
    mean = {f: sum(r["tiles512_per_s"] for r in rs) / len(rs) for f, rs in per.items()}
    out = {
        "what": "halo mode, (batching='band', accumulate='blocks') = the code path as it was, against (batching='rank', "
                "accumulate='band'), alternated in one process on one MI355X after one warm-up run of each",
        "workload": f"rank {args.rank} of {args.world} of the synthetic {args.rows} x {args.cols} raster, S={S}, stride={s}, B={B}, "
                    f"T=1024, crop_inputs, band_rows={args.band_rows}, max_rows={args.max_rows}, precision {args.precision}, "
                    "pipeline 2; seconds = haloAccumulate + haloFinish",
        "metric": "tiles512_per_s = generator_calls * B * (S/512)^2 / seconds",
        "canvas_window": list(hs.dem_window_shape), "runs": runs,
        "summary": {f"{b}_{a}": {"tiles512_per_s": [r["tiles512_per_s"] for r in per[(b, a)]],
                                 "generator_calls": per[(b, a)][0]["generator_calls"],
                                 "stitch_seconds_per_band": [r["stitch_seconds_per_band"] for r in per[(b, a)]]}
                    for b, a in forms},
    }
    out["summary"]["ratio_rank_band_over_band_blocks"] = mean[forms[1]] / mean[forms[0]]
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps(out["summary"]))
    hs.close()
    gen.close()


if __name__ == "__main__":
    main()

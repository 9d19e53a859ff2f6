"""Diagnostic (not a pytest): A/B of the f16c mode's cross-term formats on one GPU, through the Generator API.
    python3 tools/gpu_cross_fp6_ab.py [--S 512 --B 8 --steps 20 --warmup 5 --rounds 3] [--oracle out.npy] [--out profiles/cross_fp6_ab.json]
cross="fp8" (the default plan) against cross="fp6" (MSR_FLAG_CROSS_FP6: fp6 cross pieces in the stream-kernel main convs, their
SPADE layers on conv_gb_resident writing the f16c6 image): `rounds` alternating timed runs each (tiles/s = 512 x 512 tiles per
second, as bench.py counts them), one profiled call each for the per-layer conv table (hipEvents around every launch), and the
relative L-inf of both outputs against the CPU oracle at the same shape (--oracle: a saved oracle output of
synthetic_patches(B, S, 0) / make_weights(seed 1234, bias_scale 0.05) / make_latent_noise(B, 256, 7); computed here otherwise)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moonsuperresolution_amd import Generator, make_latent_noise, make_weights, synthetic_patches  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--S", type=int, default=512)
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--oracle", default=None)
ap.add_argument("--out", default="profiles/cross_fp6_ab.json")
args = ap.parse_args()
S, B = args.S, args.B

w = make_weights("gaugan", S, seed=1234, bias_scale=0.05)
eps = make_latent_noise(B, 256, 7)
x = synthetic_patches(B, S, 0)
xd = torch.from_numpy(x).cuda()
gens = {c: Generator(S, B, variant="gaugan", weights=w, eps=eps, precision="f16c", cross=c) for c in ("fp8", "fp6")}
tiles_per_step = B * (S / 512.0) ** 2


def timed(gen):
    out = torch.empty((B, S, S, 1), dtype=torch.float32, device="cuda")
    for _ in range(args.warmup):
        gen.forward_device(xd, out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        gen.forward_device(xd, out=out)
    torch.cuda.synchronize()
    return args.steps * tiles_per_step / (time.perf_counter() - t0)


def layer_table(gen):
    """One row per conv / gbr launch of the plan, in plan order: median ms over `steps` profiled calls."""
    convs = [op for op in gen.conv_forms() if op["kind"] in ("conv", "gbr")]
    gen.profile(1)
    ref = torch.cuda.Event(enable_timing=True)
    ref.record()
    for _ in range(args.steps):
        gen.forward_device(xd)
    torch.cuda.synchronize()
    runs = gen.profile_runs(ref, 0)
    gen.profile(False)
    assert len(runs) == args.steps * len(convs), (len(runs), len(convs))
    rows = []
    for k, op in enumerate(convs):
        ms = statistics.median(runs[c * len(convs) + k][1] - runs[c * len(convs) + k][0] for c in range(args.steps))
        flops = runs[k][2]
        rows.append(dict(layer=op["wt"].replace("gen.", "").replace(".kernel", ""), kind=op["kind"], r=op["r"], cin=op["cin"], N=op["N"],
                         prec=op["prec"], out_split=op["out_split"], img=op["img"], ms=round(ms, 4),
                         tflops=round(flops / ms / 1e9, 1) if ms > 0 else 0.0))
    return rows


res = dict(workload=f"SPADE-{S} B={B} f16c", steps=args.steps, warmup=args.warmup, rounds=args.rounds,
           tiles_per_s={c: [] for c in gens})
for rnd in range(args.rounds):                        # alternating: drift of the box's clocks hits both sides alike
    for c in ("fp8", "fp6"):
        res["tiles_per_s"][c].append(round(timed(gens[c]), 3))
        print(f"round {rnd} cross={c}: {res['tiles_per_s'][c][-1]:.2f} tiles/s", flush=True)
med = {c: statistics.median(v) for c, v in res["tiles_per_s"].items()}
res["tiles_per_s_median"] = med
res["fp6_over_fp8"] = round(med["fp6"] / med["fp8"], 4)
res["conv_layers"] = {c: layer_table(gens[c]) for c in gens}
res["conv_ms_per_call"] = {c: round(sum(r["ms"] for r in res["conv_layers"][c]), 4) for c in gens}
for a, b in zip(res["conv_layers"]["fp8"], res["conv_layers"]["fp6"]):
    mark = "  <- f16c6" if b["out_split"] == 5 or b["img"] == "F16C6" else ""
    print(f"{a['layer']:<24} r={a['r']:<4} cin={a['cin']:<5} N={a['N']:<5} fp8 {a['ms']:.4f} ms {a['tflops']:7.1f} TF/s | "
          f"fp6 {b['ms']:.4f} ms {b['tflops']:7.1f} TF/s{mark}")

outs = {c: g(x, training=False) for c, g in gens.items()}
if args.oracle:
    ref_out, oracle = np.load(args.oracle).astype(np.float64), "saved " + os.path.basename(args.oracle)
else:
    from oracle import generator_ref
    dtype = torch.float64 if S <= 256 else torch.float32
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref_out, oracle = np.asarray(generator_ref.spade_call(x, w, "gaugan", eps, dtype=dtype), np.float64), str(dtype)
rel = lambda y: float(np.abs(y - ref_out).max() / np.abs(ref_out).max())       # noqa: E731
res["oracle"] = oracle
res["rel_linf_vs_oracle"] = {c: rel(outs[c]) for c in gens}
res["rel_linf_fp6_vs_fp8"] = float(np.abs(outs["fp6"] - outs["fp8"]).max() / np.abs(outs["fp8"]).max())
print(json.dumps({k: v for k, v in res.items() if k != "conv_layers"}))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
for g in gens.values():
    g.close()

"""Diagnostic (not a pytest): A/B of the separate and the fused SPADE head on one GPU, through the Generator API.
    python3 tools/gpu_fused_head_ab.py [--S 512 --B 8 --steps 20 --warmup 5 --rounds 3 --latency-calls 40] [--out profiles/fused_head_ab.json]
head="separate" (the default plan: gen.rb6.conv_2 writes ws.gen.rb6.out, head_kernel reads it back) against head="fused"
(MSR_FLAG_FUSED_HEAD: the conv's epilogue writes the head's 32 partial sums per pixel, head_gather_kernel finishes), same process,
same build: `rounds` alternating timed runs each (tiles/s = 512 x 512 tiles per second, as bench.py counts them), one profiled
run each for profile_read()'s ms per family and the two launches' own times (the last conv launch of a call and the head /
gather launch, medians over `steps` calls), the p50 latency of a B = 1 call for both, and the relative L-inf between the outputs."""
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
ap.add_argument("--latency-calls", type=int, default=40)
ap.add_argument("--out", default="profiles/fused_head_ab.json")
args = ap.parse_args()
S, B = args.S, args.B
HEADS = ("separate", "fused")
FAM_CONV, FAM_HEAD = 0, 6          # csrc/forward.hip Family

w = make_weights("gaugan", S, seed=1234, bias_scale=0.05)


def build(batch):
    eps = make_latent_noise(batch, 256, 7)
    return {h: Generator(S, batch, variant="gaugan", weights=w, eps=eps, precision="f16c", head=h) for h in HEADS}


def timed(gen, xd, batch):
    out = torch.empty((batch, S, S, 1), dtype=torch.float32, device="cuda")
    for _ in range(args.warmup):
        gen.forward_device(xd, out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        gen.forward_device(xd, out=out)
    torch.cuda.synchronize()
    return args.steps * batch * (S / 512.0) ** 2 / (time.perf_counter() - t0)


def profiled(gen, xd):
    """profile_read() per call, and the medians of the call's last conv launch and of its head / gather launch."""
    n_conv = sum(1 for op in gen.conv_forms() if op["kind"] in ("conv", "gbr"))
    gen.profile(1)
    ref = torch.cuda.Event(enable_timing=True)
    ref.record()
    for _ in range(args.steps):
        gen.forward_device(xd)
    torch.cuda.synchronize()
    fam = {k: round(v["device_ms"] / args.steps, 4) for k, v in gen.profile_read().items()}
    convs, heads = gen.profile_runs(ref, FAM_CONV), gen.profile_runs(ref, FAM_HEAD)
    gen.profile(False)
    assert len(convs) == args.steps * n_conv and len(heads) == args.steps, (len(convs), n_conv, len(heads))
    last = statistics.median(convs[c * n_conv + n_conv - 1][1] - convs[c * n_conv + n_conv - 1][0] for c in range(args.steps))
    head = statistics.median(b - a for a, b, _, _ in heads)
    return fam, round(last, 4), round(head, 4)


def latency(gen, xd):
    out = torch.empty((1, S, S, 1), dtype=torch.float32, device="cuda")
    for _ in range(args.warmup):
        gen.forward_device(xd, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.latency_calls):
        t0 = time.perf_counter()
        gen.forward_device(xd, out=out)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 4)


x = synthetic_patches(B, S, 0)
xd = torch.from_numpy(x).cuda()
gens = build(B)
res = dict(workload=f"SPADE-{S} B={B} f16c", steps=args.steps, warmup=args.warmup, rounds=args.rounds,
           head_fused={h: gens[h].head_fused for h in HEADS}, device_bytes={h: gens[h].device_bytes() for h in HEADS},
           tiles_per_s={h: [] for h in HEADS})
for rnd in range(args.rounds):                        # alternating: drift of the box's clocks hits both sides alike
    for h in HEADS:
        res["tiles_per_s"][h].append(round(timed(gens[h], xd, B), 3))
        print(f"round {rnd} head={h}: {res['tiles_per_s'][h][-1]:.2f} tiles/s", flush=True)
med = {h: statistics.median(v) for h, v in res["tiles_per_s"].items()}
res["tiles_per_s_median"] = med
res["fused_over_separate"] = round(med["fused"] / med["separate"], 4)
res["family_ms_per_call"], res["last_conv_ms"], res["head_ms"] = {}, {}, {}
for h in HEADS:
    res["family_ms_per_call"][h], res["last_conv_ms"][h], res["head_ms"][h] = profiled(gens[h], xd)
    print(f"head={h}: gen.rb6.conv_2 {res['last_conv_ms'][h]:.4f} ms, head / gather {res['head_ms'][h]:.4f} ms, "
          f"families {res['family_ms_per_call'][h]}", flush=True)
outs = {h: g(x, training=False) for h, g in gens.items()}
res["rel_linf_fused_vs_separate"] = float(np.abs(outs["fused"].astype(np.float64) - outs["separate"]).max() / np.abs(outs["separate"]).max())
for g in gens.values():
    g.close()
del gens
torch.cuda.empty_cache()

x1 = torch.from_numpy(synthetic_patches(1, S, 0)).cuda()
g1 = build(1)
res["head_fused_b1"] = {h: g1[h].head_fused for h in HEADS}
res["p50_ms_per_call_b1"] = {h: [] for h in HEADS}
for rnd in range(args.rounds):
    for h in HEADS:
        res["p50_ms_per_call_b1"][h].append(latency(g1[h], x1))
res["p50_ms_per_call_b1_median"] = {h: statistics.median(v) for h, v in res["p50_ms_per_call_b1"].items()}
for g in g1.values():
    g.close()
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")

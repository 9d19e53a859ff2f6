"""Regenerates the committed golden vectors from the CPU oracle (run from the repo root).

The reference cannot run here (TensorFlow / tfa / OpenCV / GDAL absent; spade/models/model.py does not parse),
so these vectors are outputs of oracle/ — the restatement of the reference — not of the reference itself:
"parity unpinned" for the generator.  They pin the oracle against regressions and give the
GPU tests a fixed target that does not need the oracle's 100 M-parameter weight regeneration to agree by luck.

    spade64_<variant>.npz   S=64 (sw=1), B=2, seeded weights (seed 1234, bias_scale 0.05), eps seed 7,
                            float64 oracle output [2,64,64,1] + per-block checksums (mean |x| of each block output)
    spade64_zero.npz        same, second patch all-zero (the zero padding patch of process_full_tiles.py:468-474)
    pix2pix256.npz          pix2pix S=256 B=1 float64 oracle output: checksum + an 8x8 probe grid
    stitch_small.npz        rebuild_tile on tests/helpers.stitch_inputs() (S=64, s=16, T=128): float32 outputs

NOT regenerated here, on purpose: form_table.json pins the form table as commit d303279 computed it — the last commit in which
the kernel of a layer was decided at launch time (launch_conv_igemm / launch_pp) and predicted by forms.hip — so that the
refactor that put the kernel into the form could be proved to change no form.  It was written once by a scratch program linked
against that commit's libmoonsr_hip.so: for S in {64, 128, 256, 512} x B in {1, 2, 3, 4, 8, 12, 16} x the flag sets of the file
(plus pix2pix at 256) it filled an msr_handle's configuration by hand as msr_create did, called msr::fill_forms,
msr::head_fused_form and msr::conv_gbr_ranges, printed the text msr_debug_form_table prints now, with the `kernel` word derived
by restating that commit's dispatch (fp32 -> generic; bf16x3 by tile / wt_frag; F16X2, FP8 -> pp; F16C6 and EPI_RES_HEAD -> sw;
F16C with K ranges -> pp, whole tiles by msr::f16c_whole_tile_on_stream), and was run once per environment of the file's
"envs" (the switches are read once per process).  Stored: the SHA-256 of every text, and the text itself under no switch for
f16c at (64, 2), (128, 3), (256, 16), (512, 8), (512, 12).  A form that changes ON PURPOSE later regenerates the fixture from
msr_debug_form_table itself (tests/test_forms_host.py run as a script prints the tables of one environment).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from moonsuperresolution_amd import make_latent_noise, make_weights, synthetic_patches  # noqa: E402
from oracle import generator_ref, tiler_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def spade_case(variant, zero_second=False):
    S, B = 64, 2
    w = make_weights(variant, S, seed=1234, bias_scale=0.05)
    eps = make_latent_noise(B, 256, 7)
    x = synthetic_patches(B, S, 0)
    if zero_second:
        x[1] = 0.0
    cap = {}
    y = generator_ref.spade_call(x, w, variant, eps, dtype=torch.float64, capture=cap)
    blocks = {k.replace(".", "_"): np.float64(np.abs(v).mean()) for k, v in cap.items()}
    return dict(output=y.astype(np.float64), **blocks)


def stitch_case():
    from tests.helpers import stitch_inputs
    S, s, T = 64, 16, 128
    keys, pred, mm = stitch_inputs(S, s, T)
    gen = {tuple(int(v) for v in k): p + np.float32(0.5) for k, p in zip(keys, pred)}
    mmd = {tuple(int(v) for v in k): (m[0], m[1]) for k, m in zip(keys, mm)}
    mean, std, good = tiler_ref.rebuild_tile(gen, mmd, T, S, s, -32768.0)
    mean_t, std_t, _ = tiler_ref.rebuild_tile(gen, mmd, T, S, s, -32768.0, as_implemented=False)
    return dict(mean=mean, std=std, good=good, mean_textbook=mean_t, std_textbook=std_t)


if __name__ == "__main__":
    for v in ("gaugan", "gaugan_no_kl"):
        np.savez_compressed(os.path.join(HERE, f"spade64_{v}.npz"), **spade_case(v))
    np.savez_compressed(os.path.join(HERE, "spade64_zero.npz"), **spade_case("gaugan", zero_second=True))
    w = make_weights("pix2pix", 256, seed=1234, bias_scale=0.05)
    y = generator_ref.pix2pix_call(synthetic_patches(1, 256, 3), w, dtype=torch.float64)
    np.savez_compressed(os.path.join(HERE, "pix2pix256.npz"), checksum=np.float64(np.abs(y).mean()),
                        probe=y[0, 16::32, 16::32, 0].astype(np.float64), absmax=np.float64(np.abs(y).max()))
    np.savez_compressed(os.path.join(HERE, "stitch_small.npz"), **stitch_case())
    print("golden vectors written to", HERE)

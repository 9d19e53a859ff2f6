"""Diagnostic (not a pytest, CPU only): error of the fused head's arithmetic against head_kernel's, both against float64.
The head reduces 128 channels x 25 live taps = 3 200 terms per output.  Emulated on random data (activations N(0, 3) after
leaky_relu(0.2), weights at glorot scale 1 / sqrt(16 * 128)):
  split : three fp16 products per term, w_hi a_hi + w_hi a_lo + w_lo a_hi with hi = f16_rn(x), lo = f16_rn(x - hi), products
          exact, fp32 accumulation in 32-deep blocks (one v_mfma_f32_16x16x32_f16 each), the blocks added in fp32 — the head
          epilogue of conv_igemm_f16c_sw (csrc/conv_sw.hip sw_epilogue_head) and the gather;
  fmaf  : one fp32 fmaf chain over the 3 200 terms — head_kernel (csrc/small_kernels.hip).
Prints the worst |error| of each over the outputs, as a fraction of the outputs' range (max - min), and the worst distance between the two:
the tolerances of tests/test_gpu_fused_head.py come from here.   usage: python tools/emulate_head_split.py [outputs] [seed]"""
import sys

import numpy as np

n_out = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
K = 3200
a = rng.normal(0.0, 3.0, (n_out, K))
a = np.where(a >= 0, a, 0.2 * a).astype(np.float32)
w = (rng.normal(0.0, 1.0, K) / np.sqrt(16 * 128)).astype(np.float32)
exact = a.astype(np.float64) @ w.astype(np.float64)
scale = exact.max() - exact.min()       # rel_linf (tests/helpers.py) divides by max |.|: about twice these figures


def split(v):
    hi = v.astype(np.float16).astype(np.float32)
    return hi, (v - hi).astype(np.float16).astype(np.float32)


def mfma_blocks(x, y, acc):
    """acc[block] += sum of 32 exact products, one rounding to fp32 per block (the MFMA's accumulation is at least that good)"""
    p = (x.astype(np.float64) * y.astype(np.float64)).reshape(n_out, K // 32, 32).sum(-1)
    return (acc.astype(np.float64) + p).astype(np.float32)


ah, al = split(a)
wh, wl = split(w)
blk = np.zeros((n_out, K // 32), np.float32)
for x_, y_ in ((ah, wh), (al, wh), (ah, wl)):
    blk = mfma_blocks(x_, y_, blk)
s = np.zeros(n_out, np.float32)
for k in range(K // 32):                 # the waves' partials and the gather's taps: fp32 adds
    s = (s + blk[:, k]).astype(np.float32)
f = np.zeros(n_out, np.float32)
for k in range(K):                       # fmaf: the product is not rounded
    f = (f.astype(np.float64) + a[:, k].astype(np.float64) * np.float64(w[k])).astype(np.float32)
print(f"{n_out} outputs of {K} terms, range {scale:.3f}")
print(f"split fp16 x3, fp32 accumulation : {np.abs(s - exact).max() / scale:.2e} of the range")
print(f"fp32 fmaf chain (head_kernel)    : {np.abs(f - exact).max() / scale:.2e} of the range")
print(f"split against fmaf               : {np.abs(s.astype(np.float64) - f).max() / scale:.2e} of the range")

"""GPU (-m gpu): every op of the planned network against float64 of ITS OWN input.

One forward of GauGAN at the bench shapes; then the plan is walked op by op (Generator.conv_forms, msr_debug_conv_forms).  For
every op the input the GPU itself read is fetched (msr_debug_tensor) and decoded the way the kernel reads it, the reference
is evaluated in float64 from the host fp32 weights passed through the Python twin of the weight image the plan reports
(ops.f16c_weight_image, ...: the "emu" reference of tests/test_gpu_conv_kernel.py), and the whole output tensor is compared.
Errors do not compound, a failure names the layer, and each site carries the bound of the kernel-level test of the same
kernel.  The uploaded weight images (and their .wexp) are compared with the twins bit for bit; the borders of every padded
buffer must be exactly zero.

Bounds (all from the kernel-level tests; rel = max |y - ref| / max |ref| over the tensor):
  conv, fp32 operands                       rel <= 1e-5      test_conv_bias, test_conv_spade_epilogue
  conv, bf16x3 / f16x2 / fp8 / f16c / f16c6 rel <= 5e-5      test_conv_bf16x3, ..._f16x2 (rounded weights), test_conv_fp8..., test_conv_f16c*
  SPADE image outputs                       split-bf16: hi + lo under the conv's bound; bf8: at most 2e-3 of the bytes differ from
                                            e5m2(ref), each by one step; f16c: hi within 2^-11, hi + lo8 within 2^-14 of the range,
                                            h8 within 2^-4 * 1.01 relative (floor 2^-6); f16c6: hi 2^-11, h6 0.07 and hi + l6 2^-13 of
                                            the block maximum (_check_f16c_spade, test_conv_f16c_spade_epilogue_writes_the_f16c6_image);
                                            the kernel tests take the kernel's own fp32 output as the value, here it is the float64
                                            reference, so the conv's bound x range is added to each piece's allowance
  conv_gb_resident (one site: src, x, mean, std, embedding weights -> a_j)   against the exact float64 chain: hi + lo8 rel <= 2e-4,
                                            hi within (2^-11 + 2e-4) of the range, h8 within 2^-4 * 1.01 + 2e-3; the f16 mode against
                                            the chain with fp16-rounded embedding and weights: rel <= 1e-4
                                            (test_spade_layer_resident_kernel, ..._f16)
  conv_smallcin                             |err| <= 20 * 2^-24 * (sum |w| |x| + |bias|) per element (test_conv_smallcin); an image
                                            output adds the format's own rounding of the value: split-bf16 2^-16 |v|
                                            (test_split_bf16_words), split-fp16 2^-21 |v| + 2^-24 (two fp16 roundings, subnormal floor),
                                            f16c 2^-14 of the range, bf8 by the byte rule above
  norm_act                                  2^-21 (|(x - m) / s * gamma| + |beta|) per element (test_gpu_moments._check_norm_act)
  dense                                     (kch + splits + 1) * 2^-24 * (|x| . |W| + |bias|) per element (test_dense)
  latent                                    4 * 2^-24 * (|m| + |exp(v / 2) eps|) per element (test_latent)
  head                                      rel <= 1e-5 (test_head_kernel_known_answers)
A conv whose K (up to 9 x 1024) is longer than the kernel test's may exceed its bound by accumulation alone: then the same
terms on the same decoded operands are evaluated with plain fp32 accumulation in torch, and 4x that evaluation's error
against float64 is allowed instead (accumulation order differs between any two fp32 evaluations).  MEASURED: no site of any
configuration below needed the allowance: the largest error / bound of a conv's value check is 0.61 (fp8, rb6 conv_1,
K = 9 x 256), 0.46 in fp32, 0.13 in bf16x3, 0.08 in f16c; the fp32 evaluation's own error at the one site where it was taken (the
control, K = 1152) is 1.5e-8 absolute, ratio to the bound 2e-4.

Before the sites, the plan's host side is checked line by line (check_plan_against_form_table): every conv and gbr line names the
kernel the launch-time dispatch used to pick (restated in old_dispatch), a gbr line's ranges are conv_gbr_ranges, and the plan runs
the forms msr_debug_form_table gives for the same configuration.

Every site's worst error / bound is printed and appended to parity_network_sites.jsonl in the run-record directory (next to
parity_baseline_configs.jsonl); a copy of one full run is
profiles/network_sites_parity.jsonl.

Wall time on one MI355X box: see WALL_TIME below.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests.helpers import conv_taps, dense_kch, pad_hw, rel_linf, smallcin_ref, unsplit
from tests.helpers import record_dir as _record_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
CONTROL_KEY = "gen.rb3.spade_1.conv_gamma.kernel"

# WALL_TIME, measured on an MI355X: the GPU tests of this file 45 s (ten configurations and the two control runs),
# tests/test_gpu_baseline_configs.py 434 s.  The (512, 8) configuration takes 5.5 s of it: its float64 references run on the GPU,
# one sample at a time, over every pixel.

PREC_F32, PREC_BF16X3, PREC_F16X2, PREC_FP8, PREC_F16C, PREC_F16C6 = range(6)
TILE_128, TILE_64, TILE_128_K16, TILE_PP = 0, 1, 2, 5

# (S, B, precision, MSR_F16C_FP6)
CONFIGS = [(256, 16, "f16c", 0), (512, 8, "f16c", 0), (256, 16, "bf16x3", 0), (256, 4, "bf16x3", 0), (256, 2, "fp32", 0),
           (256, 16, "f16", 0), (256, 16, "fp8", 0), (256, 16, "bf16x3_gbf16", 0), (256, 16, "f16c", 1),
           (256, 16, "fp32", 0),      # for the fp32 128 x 128 tile, which B = 2 never fills
           (128, 3, "f16c", 0)]       # for the f16c gamma|beta convs on the ping-pong kernel: conv_gb_resident takes every such layer of the
                                      # configurations above, and leaves rb5 / rb6 here (conv_gbr_ranges = 0: too few work items)

# (kind, prec, tile, ksplit > 1, wt_frag, no_cross, out_split) the configurations must send to a checked site, from reading
# forms.hip conv_form / spade_form (kinds without a field carry 0):
REQUIRED_FORMS = {
    # f16c (spade_form, gbc && cvc): conv_gb_resident writes the f16c image; its consumer runs the stream kernel on whole tiles
    # (conv_sw.hip, Cin % 128 == 0) or K ranges of the ping-pong kernel + split-K pass where tiles < CUs (pp_ksplit > 1)
    ("gbr", PREC_F16C6, TILE_PP, False, 0, 0, 4), ("conv", PREC_F16C, TILE_PP, False, 0, 0, 0),
    ("conv", PREC_F16C, TILE_PP, True, 0, 0, 0),
    # f16c where conv_gbr_ranges() == 0 while pp_ksplit() >= 1: the gamma|beta conv runs f16c on the ping-pong kernel, whole tiles
    # (LDS-assembled SPADE epilogue) or K ranges (split-K SPADE pass), and writes the f16c image for an f16c consumer (gbc && cvc)
    # or split-bf16 words for a bf16x3 one (gbc && !cvc).  Not required here, left to the kernel test (_check_f16c_spade, out_mode 1,
    # ks = 1): whole tiles writing split-bf16 words, which the planner picks only from S = 1024, B >= 8 on (a consumer input
    # beyond the 2 GiB buffer range), and the same four forms under MSR_GBR=0 at other shapes.
    ("conv", PREC_F16C, TILE_PP, False, 0, 0, 4), ("conv", PREC_F16C, TILE_PP, True, 0, 0, 4),
    ("conv", PREC_F16C, TILE_PP, True, 0, 0, 1),
    # f16 (MSR_FLAG_F16_MAIN): the two big kernels without the cross terms
    ("gbr", PREC_F16C6, TILE_PP, False, 0, 1, 4), ("conv", PREC_F16C, TILE_PP, False, 0, 1, 0),
    # MSR_F16C_FP6=1 (cv6): whole-tile ping-pong f16c gamma|beta conv writing the f16c6 image, f16c6 consumer on the stream kernel
    ("conv", PREC_F16C, TILE_PP, False, 0, 0, 5), ("conv", PREC_F16C6, TILE_PP, False, 0, 0, 0),
    # bf16x3 (conv_form): ping-pong whole tiles (pp_ksplit == 1) and K ranges (> 1), as gamma|beta conv (split-bf16 image out) and
    # as main conv; else the fragment-order small / big tile with split-K (low-resolution and stride-2 layers)
    ("conv", PREC_BF16X3, TILE_PP, False, 0, 0, 0), ("conv", PREC_BF16X3, TILE_PP, False, 0, 0, 1),
    ("conv", PREC_BF16X3, TILE_PP, True, 0, 0, 0), ("conv", PREC_BF16X3, TILE_PP, True, 0, 0, 1),
    ("conv", PREC_BF16X3, TILE_64, True, 1, 0, 0), ("conv", PREC_BF16X3, TILE_64, True, 1, 0, 1),
    ("conv", PREC_BF16X3, TILE_128, True, 1, 0, 0), ("conv", PREC_BF16X3, TILE_64, False, 1, 0, 0),
    ("conv", PREC_BF16X3, TILE_64, False, 1, 0, 1),
    # ... and, for the stride-2 encoder convs that fill the chip (no ping-pong form: pp_ksplit wants stride 1), the big tile with
    # LDS-staged weights, whole K or split
    ("conv", PREC_BF16X3, TILE_128, False, 0, 0, 0), ("conv", PREC_BF16X3, TILE_128, True, 0, 0, 0),
    # bf16x3_gbf16: whole-tile ping-pong gamma|beta convs with 2-term fp16 products
    ("conv", PREC_F16X2, TILE_PP, False, 0, 0, 1),
    # fp8 (gb8 / cv8): fp8 gamma|beta conv writing bf8 bytes for an fp8 consumer, the fp8 consumer
    ("conv", PREC_FP8, TILE_PP, False, 0, 0, 3), ("conv", PREC_FP8, TILE_PP, False, 0, 0, 0),
    ("conv", PREC_FP8, TILE_PP, False, 0, 0, 1),      # gb8 && !cv8: split-bf16 words for a bf16x3 consumer
    # fp32 (conv_pick_tile): small tile with and without split-K, the 16-channel K-step big tile of the SPADE epilogue, the
    # 32-channel K-step big tile of the other epilogues (>= 512 big blocks: B = 16)
    ("conv", PREC_F32, TILE_128, False, 0, 0, 0),
    ("conv", PREC_F32, TILE_64, True, 0, 0, 0), ("conv", PREC_F32, TILE_64, False, 0, 0, 0),
    ("conv", PREC_F32, TILE_128_K16, False, 0, 0, 0),
    # every out_split of the mask embedding / encoder block 1 (split_for) and of norm_act
    ("smallcin", 0, 0, False, 0, 0, 0), ("smallcin", 0, 0, False, 0, 0, 1), ("smallcin", 0, 0, False, 0, 0, 2),
    ("smallcin", 0, 0, False, 0, 0, 3), ("smallcin", 0, 0, False, 0, 0, 4),
    ("norm_act", 0, 0, False, 0, 0, 0), ("norm_act", 0, 0, False, 0, 0, 1),
    ("dense", 0, 0, False, 0, 0, 0), ("latent", 0, 0, False, 0, 0, 0), ("head", 0, 0, False, 0, 0, 0),
}
_SEEN_FORMS = set()


def form_of(op):
    return (op["kind"], op.get("prec", 0), op.get("tile", 0), op.get("ksplit", 1) > 1, op.get("wt_frag", 0),
            op.get("no_cross", 0), op.get("out_split", 0))


def _print_only(**kw):
    print("site", kw)


def _record(**kw):
    try:
        os.makedirs(_record_dir(), exist_ok=True)
        with open(os.path.join(_record_dir(), "parity_network_sites.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")
    except OSError:
        pass
    print("site", kw)


# ------------------------------------------------------------------------------------------------
# decoding what the GPU holds
# ------------------------------------------------------------------------------------------------
def _words(t):
    return t.contiguous().view(torch.int32)


def _fp8_pad(c):
    return 128 if c <= 128 else (c + 255) // 256 * 256


def unsplit_f16(t):
    """split-fp16 chunk image -> (hi, lo) float32 values, same shape."""
    u = t.contiguous().view(torch.float16).reshape(-1, 2, 32).float()
    return u[:, 0].reshape(t.shape), u[:, 1].reshape(t.shape)


def decode(fmt, buf):
    """Image (float32 storage [..., slots]) of out_split / operand format fmt -> tuple of float64 parts [..., channels]."""
    from moonsuperresolution_amd import ops
    if fmt == 0:
        return (buf.double(),)
    if fmt == 1:
        return tuple(t.double() for t in unsplit(buf))
    if fmt == 2:
        return tuple(t.double() for t in unsplit_f16(buf))
    if fmt == 3:
        return (buf.contiguous().view(torch.float8_e5m2).double(),)
    if fmt == 4:
        return ops.f16c_decode(buf)
    return ops.f16c6_decode(buf)


def border_is_zero(buf):
    w = _words(buf)
    return not bool(w[:, 0].any() or w[:, -1].any() or w[:, :, 0].any() or w[:, :, -1].any())


def interior(t):
    return t[:, 1:-1, 1:-1]


# ------------------------------------------------------------------------------------------------
# the weight twins: image (for the bit compare) and de-quantised parts (for the reference)
# ------------------------------------------------------------------------------------------------
def weight_twin(img, w_tnk):
    """img name of the dump, kernel-layout fp32 weights [taps][N][Cin] on the GPU -> (image as int32 words, wexp or None,
    parts): what msr_load_weight must have uploaded, and the values the kernel multiplies."""
    from moonsuperresolution_amd import ops
    if img == "F32":
        return _words(w_tnk).reshape(-1), None, (w_tnk.double(),)
    if img in ("BF16", "BF16_FRAG"):
        im = ops.split_bf16_host(w_tnk)
        hi, lo = unsplit(im)
        if img == "BF16_FRAG":
            im = ops.weights_bf16x3(w_tnk)
        return _words(im).reshape(-1), None, (hi.double(), lo.double())
    if img == "F16":
        return _words(ops.split_f16(w_tnk)).reshape(-1), None, (w_tnk.to(torch.float16).double(),)
    if img == "FP8":
        im, wexp, wdq = ops.fp8_weight_image(w_tnk)
        wpad = torch.zeros(im.shape, dtype=torch.float64, device=w_tnk.device)
        wpad[..., :w_tnk.shape[2]] = wdq.double()
        return im.reshape(-1).view(torch.int32), wexp, (wpad,)
    if img == "F16C":
        im, wexp, parts = ops.f16c_weight_image(w_tnk)
        return _words(im).reshape(-1), wexp, parts
    if img == "F16C6":
        im, parts = ops.f16c6_weight_image(w_tnk)
        return _words(im).reshape(-1), None, parts
    assert img == "GBR", img
    return _words(ops.gbr_weight_image(w_tnk)).reshape(-1), None, ops.f16c6_weight_image(w_tnk)[1]


def product_terms(prec, no_cross, x, w):
    """The (activation part, weight part) pairs whose products the kernel of `prec` adds up."""
    if prec == PREC_F32 or prec == PREC_FP8:
        return [(x[0], w[0])]
    if prec == PREC_BF16X3:                       # a_hi b_hi + a_hi b_lo + a_lo b_hi
        return [(x[0], w[0] + w[1]), (x[1], w[0])]
    if prec == PREC_F16X2:                        # (a_hi + a_lo) w_hi
        return [(x[0] + x[1], w[0])]
    if no_cross:
        return [(x[0], w[0])]
    return [(x[0], w[0]), (x[1], w[2]), (x[2], w[1])]      # x_hi w_hi + x_h8 w_lo + x_lo w_h8 (f16c and f16c6 alike)


class Sites:
    """One forward of one configuration and the checks of its ops."""

    def __init__(self, S, B, precision, weights=None, tag="", record=True):
        from moonsuperresolution_amd import Generator, make_latent_noise, make_weights, synthetic_patches
        self.S, self.B, self.precision, self.tag, self.record = S, B, precision, tag, record
        self.w_loaded = make_weights("gaugan", S, seed=1234, bias_scale=0.05)
        self.w = weights or self.w_loaded                       # what the references use (the control swaps one)
        self.eps = make_latent_noise(B, 256, 7)
        self.x = synthetic_patches(B, S, 0)
        self.gen = Generator(S, B, variant="gaugan", weights=self.w_loaded, eps=self.eps, precision=precision)
        self.y = self.gen(self.x, training=False)
        self.ops = self.gen.conv_forms()
        self.dev = torch.device("cuda")
        self.fp6 = os.environ.get("MSR_F16C_FP6") == "1"
        self._cache = {}
        self._twins = {}

    def close(self):
        self.gen.close()
        self._cache.clear()
        self._twins.clear()
        torch.cuda.empty_cache()

    # -- tensors --------------------------------------------------------------------------------
    def t(self, name, shape):
        if name == "input":
            return torch.from_numpy(self.x).to(self.dev)
        if name == "output":
            return torch.from_numpy(self.y).to(self.dev).reshape(shape)
        if name == "eps":
            return torch.from_numpy(self.eps).to(self.dev)
        key = (name, tuple(shape))
        if key not in self._cache:
            if len(self._cache) > 6:
                self._cache.clear()
            self._cache[key] = torch.from_numpy(self.gen.debug_tensor(name, shape)).to(self.dev)
        return self._cache[key]

    def hw(self, name):
        return torch.from_numpy(np.ascontiguousarray(self.w[name])).to(self.dev)

    def res(self, name):
        """resolution of a generator activation by its name"""
        sw = self.S // 64
        if name == "ws.gen.x0":
            return sw
        return sw << (int(name.split(".rb")[1].split(".")[0]) - 1)

    def conv_weights(self, key):
        """wt key of the dump -> (kernel-layout fp32 weights, bias in GEMM column order) from the host weights"""
        from moonsuperresolution_amd import ops
        if key.endswith(".gb.kernel"):
            base = key[: -len(".gb.kernel")]
            return ops.spade_layout(self.hw(base + ".conv_gamma.kernel"), self.hw(base + ".conv_beta.kernel"),
                                    self.hw(base + ".conv_gamma.bias"), self.hw(base + ".conv_beta.bias"))
        w = ops.kernel_layout(self.hw(key))
        b = key[: -len("kernel")] + "bias"
        bias = self.hw(b) if b in self.w else torch.zeros(w.shape[1], device=self.dev)
        return w, bias

    def twin(self, key, img):
        if key not in self._twins:
            self._twins.clear()
            w_tnk, bias = self.conv_weights(key)
            self._twins[key] = weight_twin(img, w_tnk) + (bias,)
        return self._twins[key]

    def words_equal(self, name, want_words):
        """uploaded tensor `name` == the twin, bit for bit -> number of differing 32-bit words"""
        want = want_words.reshape(-1).cpu().numpy().view(np.uint32)
        got = self.gen.debug_tensor(name, (want.size,)).view(np.uint32)
        try:                                     # the uploaded tensor must end where the twin ends: one more word is refused
            self.gen.debug_tensor(name, (want.size + 1,))
            longer = 1
        except ValueError:
            longer = 0
        return int((got != want).sum()) + longer

    # -- the reference of a product sum -----------------------------------------------------------
    def conv_sum(self, terms, r, stride, dtype=None):
        acc = None
        for xp, wp in terms:
            y = conv_taps(xp, wp, r, stride, dtype)
            acc = y if acc is None else acc + y
        return acc

    def allowance(self, terms, r, stride, ref_lin):
        """4x the error of the plain fp32 evaluation of the same terms (module docstring); ref_lin: their float64 sum"""
        e32 = float((self.conv_sum(terms, r, stride, torch.float32).double() - ref_lin).abs().max())
        return 4 * e32, e32

    # -- image outputs ----------------------------------------------------------------------------
    def image_ratio(self, fmt, buf, want, vb_abs, C):
        """buf: interior of the output image, want: float64 values [..., C], vb_abs: the value bound of the producing kernel
        (absolute).  Returns {check: error / bound}."""
        scale = float(want.abs().max())
        p = decode(fmt, buf)
        if fmt == 0:
            return {"value": float((p[0] - want).abs().max()) / vb_abs}
        if fmt in (1, 2):
            return {"value": float((p[0] + p[1] - want).abs().max()) / vb_abs}
        if fmt == 3:
            got = p[0][..., :C]
            pad_zero = not bool(buf.contiguous().view(torch.uint8)[..., C:].any())
            ref8 = want.float().to(torch.float8_e5m2).double()
            mism = got != ref8
            ulp = torch.maximum(ref8.abs() * 0.25, torch.tensor(2.0 ** -16, device=ref8.device, dtype=torch.float64))
            step = float(((got - ref8).abs() / (ulp * 1.001))[mism].max()) if bool(mism.any()) else 0.0
            return {"bytes_differ": float(mism.double().mean()) / 2e-3, "one_step": step, "pad_zero": 0.0 if pad_zero else 2.0}
        if fmt == 4:
            hi, h8, lo8 = p
            return {"hi": float((hi - want).abs().max()) / (2.0 ** -11 * scale + vb_abs),
                    "value": float((hi + lo8 - want).abs().max()) / (2.0 ** -14 * scale + vb_abs),
                    "h8": float(((h8 - want).abs() / (2.0 ** -4 * 1.01 * want.abs().clamp_min(2.0 ** -6) + vb_abs)).max())}
        hi, h6, l6 = p
        shp = want.shape
        blk = want.abs().reshape(shp[:-1] + (C // 32, 32)).amax(-1, keepdim=True).expand(shp[:-1] + (C // 32, 32)).reshape(shp)
        blk = blk.clamp_min(1e-30)
        raw = buf.contiguous().view(torch.uint8).reshape(-1, 128)
        tail = bool(raw[:, 89:96].any() or raw[:, 121:128].any() or (raw[:, 88].int() - 11 != raw[:, 120].int()).any())
        return {"hi": float((hi - want).abs().max()) / (2.0 ** -11 * scale + vb_abs),
                "h6": float(((h6 - want).abs() / (0.07 * blk + vb_abs)).max()),
                "value": float(((hi + l6 - want).abs() / (2.0 ** -13 * blk + vb_abs)).max()),
                "scales": 2.0 if tail else 0.0}

    # -- ops --------------------------------------------------------------------------------------
    def check_conv(self, op):
        B, r, N, stride, prec, epi = op["B"], op["r"], op["N"], op["stride"], op["prec"], op["epi"]
        in_fmt = {PREC_F32: 0, PREC_BF16X3: 1, PREC_F16X2: 2, PREC_FP8: 3, PREC_F16C: 4, PREC_F16C6: 5}[prec]
        xin = self.t(op["in"], (B, r * stride + 2, r * stride + 2, op["cin"]))
        fig = {"in_border": 0.0 if border_is_zero(xin) else 2.0}
        img_words, wexp, wparts, bias = self.twin(op["wt"], op["img"])
        fig["weight_words_differ"] = float(self.words_equal(op["wt"], img_words))
        if wexp is not None:
            fig["wexp_words_differ"] = float(self.words_equal(op["wexp"], wexp))
        if op["bias"] != "ws.zero_bias":
            fig["bias_words_differ"] = float(self.words_equal(op["bias"], _words(bias)))
        terms = product_terms(prec, op["no_cross"], decode(in_fmt, xin), wparts)
        lin = self.conv_sum(terms, r, stride)
        relb = 1e-5 if prec == PREC_F32 else 5e-5
        if epi == 2:
            C = N // 2
            c = torch.arange(C, device=self.dev)
            rows_g = (c // 32) * 64 + (c % 32)
            gb = lin + bias.double()
            rx = self.res(op["aux"])
            x = self.t(op["aux"], (B, rx, rx, C)).double()
            if rx != r:
                x = x.repeat_interleave(r // rx, 1).repeat_interleave(r // rx, 2)
            xn = (x - self.t(op["mean"], (C,)).double()) / self.t(op["std"], (C,)).double()
            v = gb[..., rows_g] * xn + gb[..., rows_g + 32]
            ref = torch.where(v >= 0, v, 0.2 * v)
            slots = _fp8_pad(C) // 4 if op["out_split"] == 3 else C
            out = self.t(op["out"], (B, r + 2, r + 2, slots))
            fig["out_border"] = 0.0 if border_is_zero(out) else 2.0
            vb = relb * float(ref.abs().max())
            ratios = self.image_ratio(op["out_split"], interior(out), ref, vb, C)
        else:
            ref = lin + bias.double()
            if epi == 1:
                rx = self.res(op["aux"])
                a = self.t(op["aux"], (B, rx, rx, N)).double()
                if rx != r:
                    a = a.repeat_interleave(r // rx, 1).repeat_interleave(r // rx, 2)
                ref = ref + a
            out = self.t(op["out"], (B, r, r, N)).double()
            vb = relb * float(ref.abs().max())
            ratios = {"value": float((out - ref).abs().max()) / vb}
        fig["K"] = 9 * terms[0][0].shape[-1]
        if ratios.get("value", 0) > 1 and op["out_split"] in (0, 1, 2):
            allow, e32 = self.allowance(terms, r, stride, lin)
            fig["fp32_eval_err"] = e32
            if allow > vb:
                ratios["value"] *= vb / allow
                fig["allowance_used"] = allow / vb
        fig.update(ratios)
        return fig

    def check_gbr(self, op):
        from moonsuperresolution_amd import ops
        B, r, N, S = op["B"], op["r"], op["N"], self.S
        C = N // 2
        nox = op["no_cross"]
        base = op["wt"][: -len(".gb.kernel")]
        fig = {}
        img_words, _, _, bias = self.twin(op["wt"], op["img"])
        fig["weight_words_differ"] = float(self.words_equal(op["wt"], img_words))
        if fig["weight_words_differ"]:           # diagnostic: the same twin evaluated on the CPU
            cpu_words = weight_twin(op["img"], self.conv_weights(op["wt"])[0].cpu())[0]
            fig["weight_words_differ_cpu_twin"] = float(self.words_equal(op["wt"], cpu_words))
        fig["embed16_words_differ"] = float(self.words_equal(op["embed16"], _words(ops.gbr_embed_image(self.hw(base + ".conv.kernel")))))
        fig["embed_words_differ"] = float(self.words_equal(op["embed"], _words(self.hw(base + ".conv.kernel"))))
        fig["bias_words_differ"] = float(self.words_equal(op["bias"], _words(bias)))
        e = smallcin_ref(self.t("input", None), self.hw(base + ".conv.kernel"), self.hw(base + ".conv.bias"), r, 1, act=1, device=self.dev)
        w_tnk, _ = self.conv_weights(op["wt"])
        if nox:                                  # the chain with fp16-rounded embedding and weights
            e, w_tnk = e.to(torch.float16).double(), w_tnk.to(torch.float16)
        gb = conv_taps(pad_hw(e), w_tnk.double(), r) + bias.double()
        c = torch.arange(C, device=self.dev)
        rows_g = (c // 32) * 64 + (c % 32)
        rx = self.res(op["aux"])
        x = self.t(op["aux"], (B, rx, rx, C)).double()
        if rx != r:
            x = x.repeat_interleave(r // rx, 1).repeat_interleave(r // rx, 2)
        xn = (x - self.t(op["mean"], (C,)).double()) / self.t(op["std"], (C,)).double()
        v = gb[..., rows_g] * xn + gb[..., rows_g + 32]
        want = torch.where(v >= 0, v, 0.2 * v)
        out = self.t(op["out"], (B, r + 2, r + 2, C))
        fig["out_border"] = 0.0 if border_is_zero(out) else 2.0
        hi, h8, lo8 = (interior(t) for t in ops.f16c_decode(out))
        relb = 1e-4 if nox else 2e-4
        scale = float(want.abs().max())
        fig["value"] = float((hi + lo8 - want).abs().max()) / (relb * scale)
        fig["hi"] = float((hi - want).abs().max()) / ((2.0 ** -11 + relb) * scale)
        fig["h8"] = float(((h8 - want).abs() / want.abs().clamp_min(2.0 ** -6)).max()) / (2.0 ** -4 * 1.01 + 2e-3)
        fig["K"] = 9 * 128
        return fig

    def check_smallcin(self, op):
        B, r, N, fmt = op["B"], op["r"], op["N"], op["out_split"]
        imap = 0 if op["stride"] == 2 else 1
        w = self.hw(op["wt"])
        bias = self.hw(op["wt"][: -len("kernel")] + "bias") if op["bias"] != "-" else None
        fig = {"weight_words_differ": float(self.words_equal(op["wt"], _words(w)))}
        src = self.t("input", None)
        slope = float(np.float32(0.2)) if op["act"] == 2 else 0.0
        ref = smallcin_ref(src, w, bias, r, imap, op["act"], slope, device=self.dev)
        mag = smallcin_ref(src.abs(), w.abs(), bias.abs() if bias is not None else None, r, imap, device=self.dev)
        slots = _fp8_pad(N) // 4 if fmt == 3 else N
        out = self.t(op["out"], (B, r + 2, r + 2, slots))
        fig["out_border"] = 0.0 if border_is_zero(out) else 2.0
        bound = 20 * U * mag
        p = decode(fmt, interior(out))
        scale = float(ref.abs().max())
        if fmt == 3:
            fig.update(self.image_ratio(3, interior(out), ref, 0.0, N))
            return fig
        val = p[0] if fmt == 0 else (p[0] + p[1] if fmt in (1, 2) else p[0] + p[2])
        bound = bound + {0: 0.0, 1: 2.0 ** -16 * ref.abs(), 2: 2.0 ** -21 * ref.abs() + 2.0 ** -24, 4: 2.0 ** -14 * scale}[fmt]
        fig["value"] = float(((val - ref).abs() / bound.clamp_min(1e-300)).max())
        if fmt == 4:
            fig["hi"] = float(((p[0] - ref).abs() / (2.0 ** -11 * scale + 20 * U * mag)).max())
            fig["h8"] = float(((p[1] - ref).abs() / (2.0 ** -4 * 1.01 * ref.abs().clamp_min(2.0 ** -6) + 20 * U * mag)).max())
        return fig

    def check_norm_act(self, op):
        B, r, c, fmt = op["B"], op["r"], op["N"], op["out_split"]
        i = int(op["in"][-1])
        raw = self.t(op["in"], (B, r, r, c)).double()
        m = self.t(op["mean"], (B, c)).double()[:, None, None, :]
        s = self.t(op["std"], (B, c)).double()[:, None, None, :]
        gam, bet = self.hw(f"enc.ds{i}.in.gamma").double(), self.hw(f"enc.ds{i}.in.beta").double()
        fig = {"gamma_words_differ": float(self.words_equal(op["gamma"], _words(self.hw(f"enc.ds{i}.in.gamma")))),
               "beta_words_differ": float(self.words_equal(op["beta"], _words(self.hw(f"enc.ds{i}.in.beta"))))}
        t = (raw - m) / s * gam
        ref = t + bet
        ref = torch.where(ref >= 0, ref, 0.2 * ref)
        if op["out"] == "ws.enc.flat":
            got = self.t(op["out"], (B, r, r, c))
        else:
            out = self.t(op["out"], (B, r + 2, r + 2, c))
            fig["out_border"] = 0.0 if border_is_zero(out) else 2.0
            got = interior(out)
        p = decode(fmt, got)
        val = p[0] if fmt == 0 else p[0] + p[1]
        bound = 2.0 ** -21 * (t.abs() + bet.abs()) + 1e-30 + (2.0 ** -16 * ref.abs() if fmt == 1 else 0.0)
        fig["value"] = float(((val - ref).abs() / bound).max())
        return fig

    def check_dense(self, op):
        from moonsuperresolution_amd import ops
        B, K, N = op["B"], op["cin"], op["N"]
        if op["wt"] == "enc.heads.kernel":
            W = ops.heads_concat(self.hw("enc.mean.kernel"), self.hw("enc.variance.kernel"))
            b = ops.heads_concat(self.hw("enc.mean.bias"), self.hw("enc.variance.bias"))
        else:
            W, b = self.hw("gen.dense.kernel"), self.hw("gen.dense.bias")
        fig = {"weight_words_differ": float(self.words_equal(op["wt"], _words(W))),
               "bias_words_differ": float(self.words_equal(op["bias"], _words(b)))}
        x = self.t(op["in"], (B, K)).double()
        y = self.t(op["out"], (B, N)).double()
        ref = x @ W.double() + b.double()
        mag = x.abs() @ W.double().abs() + b.double().abs()
        kch = dense_kch(K, N)
        bound = (kch + (K + kch - 1) // kch + 1) * U * mag
        fig["value"] = float(((y - ref).abs() / bound).max())
        fig["K"] = K
        return fig

    def check_latent(self, op):
        B, L = op["B"], op["N"]
        mv = self.t(op["in"], (B, 2 * L)).double()
        z = self.t(op["out"], (B, L)).double()
        m, v = mv[:, :L], mv[:, L:]
        tt = torch.exp(v / 2) * self.t("eps", None).double() if op["sampler"] else v
        bound = 4 * U * (m.abs() + tt.abs())
        fig = {"value": float(((z - (m + tt)).abs() / bound.clamp_min(1e-300)).max())}
        fig["last_latent"] = 0.0 if np.array_equal(self.gen.last_latent(), z.float().cpu().numpy()) else 2.0
        return fig

    def check_head(self, op):
        from moonsuperresolution_amd import ops
        B, r, C = op["B"], op["r"], op["cin"]
        k = self.hw("gen.head.kernel")[..., 0]                                # [4, 4, C]
        fig = {"weight_words_differ": float(self.words_equal(op["wt"], _words(ops.head_taps_upconv(k))))}
        x = self.t(op["in"], (B, r, r, C)).double()
        got = self.t("output", (B, 2 * r, 2 * r)).double()
        kd = k.double()
        bias = float(self.w["gen.head.bias"][0])
        ref = torch.empty_like(got)
        for b in range(B):
            a = torch.where(x[b] >= 0, x[b], 0.2 * x[b]).repeat_interleave(2, 0).repeat_interleave(2, 1)
            a = torch.nn.functional.pad(a, (0, 0, 1, 2, 1, 2))                # TF SAME for k = 4: 1 before, 2 after
            acc = torch.zeros((2 * r, 2 * r), dtype=torch.float64, device=self.dev)
            for kh in range(4):
                for kw in range(4):
                    acc += a[kh: kh + 2 * r, kw: kw + 2 * r] @ kd[kh, kw]
            ref[b] = acc + bias
        fig["value"] = float((got - ref).abs().max()) / (1e-5 * float(ref.abs().max()))
        return fig

    def run(self):
        """-> [(op, figures)] of every op but the moments (tests/test_gpu_moments.py walks those)"""
        check = {"conv": self.check_conv, "gbr": self.check_gbr, "smallcin": self.check_smallcin, "norm_act": self.check_norm_act,
                 "dense": self.check_dense, "latent": self.check_latent, "head": self.check_head}
        res = []
        for idx, op in enumerate(self.ops):
            if op["kind"] in ("moments", "moments_slabs"):
                continue
            t0 = time.time()
            fig = check[op["kind"]](op)
            worst = max(over_bound(fig).values())
            (_record if self.record else _print_only)(S=self.S, B=self.B, precision=self.precision + ("+fp6" if self.fp6 else "") + self.tag, op=idx, kind=op["kind"],
                    out=op["out"], wt=op.get("wt", "-"), form=list(form_of(op)), img=op.get("img", "-"),
                    worst_over_bound=worst, seconds=round(time.time() - t0, 2), **fig)
            res.append((op, fig, worst))
        return res


def over_bound(fig):
    """figures of a site -> {check: error / bound}.  A bit-for-bit compare (a count of differing 32-bit words, or a tensor whose
    size is not the twin's) has no bound to stay under: ONE differing word stands at 2."""
    out = {}
    for k, v in fig.items():
        if k in ("K", "fp32_eval_err", "allowance_used"):
            continue
        out[k] = (0.0 if v == 0 else 1.0 + v) if "words_differ" in k else v
    return out


def _failed(res):
    return [(op["kind"], op["out"], {k: v for k, v in over_bound(fig).items() if not v <= 1})
            for op, fig, worst in res if not worst <= 1]


def _expected_op_count(S, B, ops_):
    """17 + per SPADE layer (2 with the resident kernel, else 3) ops that are not moments: smallcin, 4 x (conv, norm_act), 2 dense,
    latent, head"""
    n_gbr = sum(o["kind"] == "gbr" for o in ops_)
    return 1 + 8 + 2 + 1 + 1 + (15 - n_gbr) * 3 + n_gbr * 2


def old_dispatch(lib, op):
    """The kernel a conv line ran before the form named it: the launch-time dispatch (launch_conv_igemm, launch_pp's forward to
    the stream kernel by msr_debug_f16c_kernel's rule, the planner's direct launch of the head epilogue), restated from the line."""
    prec, tile = op["prec"], op["tile"]
    if op["kind"] == "gbr":
        return "gbr"
    if op["epi"] == 5 or prec == PREC_F16C6:
        return "sw"
    if prec in (PREC_F16X2, PREC_FP8):
        return "pp"
    if prec == PREC_F16C:
        whole = op["ksplit"] <= 1
        return "sw" if whole and lib.msr_debug_f16c_kernel(op["cin"], op["epi"], op["out_split"]) else "pp"
    if prec == PREC_BF16X3:
        if tile in (TILE_PP, 3, 4):
            return {TILE_PP: "pp", 3: "halo", 4: "halo16"}[tile]
        if op["wt_frag"]:
            return "bvgpr"
    return "generic"


def check_plan_against_form_table(sites):
    """The plan walk's host-side half: every conv and gbr line names its kernel, the one the old dispatch ran; a gbr line's ranges
    are conv_gbr_ranges; and the plan runs what msr_debug_form_table says for the same configuration (same process, so the same
    environment switches): the same layers in the same forms, the same resident-kernel ranges, the same head."""
    from moonsuperresolution_amd import _lib
    from moonsuperresolution_amd.generator import form_table
    from tests.helpers import gbr_ranges
    table = form_table(sites.S, sites.B, "gaugan", _lib.PRECISION_FLAGS[sites.precision])
    fields = ("prec", "kernel", "tile", "ksplit", "wt_frag", "no_cross", "img")
    planned = {}
    for op in sites.ops:
        if op["kind"] not in ("conv", "gbr"):
            continue
        assert op.get("kernel") in ("generic", "bvgpr", "halo", "halo16", "pp", "sw", "gbr"), op
        assert op["kernel"] == old_dispatch(sites.gen._lib, op), (op["wt"], op["kernel"], old_dispatch(sites.gen._lib, op))
        layer = op["wt"][: -len(".kernel")]
        assert layer not in planned, layer
        planned[layer] = {k: op[k] for k in fields}
        if layer.endswith(".gb"):
            spade = table[layer[: -len(".gb")]]
            assert (spade["gbr"], spade["ranges"], spade["a_split"]) == (int(op["kind"] == "gbr"), op["ranges"], op["out_split"]), (layer, spade)
        if op["kind"] == "gbr":
            assert op["ranges"] == gbr_ranges(op["B"], op["r"], op["N"])[0] > 0, op
    assert planned == {k: {f: v[f] for f in fields} for k, v in table.items() if k != "head_fused" and "prec" in v}
    assert table["head_fused"] == int(any(op["kind"] == "head_gather" for op in sites.ops))


def _run_config(S, B, precision):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sites = Sites(S, B, precision)
    try:
        check_plan_against_form_table(sites)
        res = sites.run()
        checked = [op for op, _, _ in res]
        assert len(checked) == _expected_op_count(S, B, sites.ops), len(checked)
        assert {o["out"] for o in checked} >= {"ws.enc.mv", "ws.z", "ws.gen.x0", "output", "ws.enc.flat", "ws.enc.p1"}
        forms = {form_of(op) for op in checked}
    finally:
        sites.close()
    return res, forms


@pytest.mark.gpu
@pytest.mark.parametrize("S,B,precision,fp6", CONFIGS)
def test_network_sites_against_fp64(hip_lib, tmp_path, S, B, precision, fp6):
    if fp6 and os.environ.get("MSR_F16C_FP6") != "1":
        # MSR_F16C_FP6 is read once per process: this configuration runs in a child, which hands its forms back in a file
        path = str(tmp_path / "forms.json")
        env = dict(os.environ, MSR_F16C_FP6="1", NETWORK_SITES_FORMS_FILE=path)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k",
                            f"test_network_sites_against_fp64 and {S}-{B}-{precision}-1"], env=env, capture_output=True, text=True,
                           timeout=1200, cwd=ROOT)
        assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
        _SEEN_FORMS.update(tuple(f) for f in json.load(open(path)))
        return
    res, forms = _run_config(S, B, precision)
    _SEEN_FORMS.update(forms)
    if os.environ.get("NETWORK_SITES_FORMS_FILE"):
        json.dump(sorted(list(f) for f in forms), open(os.environ["NETWORK_SITES_FORMS_FILE"], "w"))
    assert not _failed(res), _failed(res)


@pytest.mark.gpu
def test_network_configs_run_every_conv_form():
    """Runs after the parametrised test: the configurations must have sent every form of REQUIRED_FORMS to a checked site."""
    if len(_SEEN_FORMS) == 0:
        pytest.fail("the network site test did not run first")
    assert REQUIRED_FORMS <= _SEEN_FORMS, sorted(REQUIRED_FORMS - _SEEN_FORMS)


# ------------------------------------------------------------------------------------------------
# control: what the site checker sees and the end-to-end test cannot
# ------------------------------------------------------------------------------------------------
def _rounded(w):
    w2 = dict(w)
    w2[CONTROL_KEY] = w[CONTROL_KEY].astype(np.float16).astype(np.float32)
    return w2


def test_control_end_to_end_is_blind_to_one_layer_without_cross_terms():
    """CPU, oracle against oracle at GauGAN(256, 16): the weights of ONE gamma|beta conv (gen.rb3.spade_1.conv_gamma) rounded to
    fp16 — the "cross terms lost in one layer" class of bug, 2^-11 per product — move the network's output by a relative
    L-infinity of 7.0e-6 (measured; 7.4e-6 at (256, 2), 1.9e-6 at (64, 16)): 35x below MODE_TOL["f16c"] = 2.5e-4, so
    test_baseline_config_matches_oracle would pass with that layer wrong.  The GPU half below shows the site checker fails
    exactly that site."""
    from moonsuperresolution_amd import make_latent_noise, make_weights, synthetic_patches
    from oracle import generator_ref
    from tests.test_gpu_baseline_configs import MODE_TOL
    S, B = 256, 16
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    w = make_weights("gaugan", S, seed=1234, bias_scale=0.05)
    eps, x = make_latent_noise(B, 256, 7), synthetic_patches(B, S, 0)
    a = np.asarray(generator_ref.spade_call(x, w, "gaugan", eps, dtype=torch.float64), np.float64)
    b = np.asarray(generator_ref.spade_call(x, _rounded(w), "gaugan", eps, dtype=torch.float64), np.float64)
    err = rel_linf(b, a)
    print("control: end-to-end rel L-inf, original against fp16-rounded", CONTROL_KEY, err)
    assert 0 < err < MODE_TOL["f16c"], err


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16c", "bf16x3"])
def test_control_site_checker_names_the_layer(hip_lib, precision):
    """The same GPU tensors, a deliberately wrong reference: gen.rb3.spade_1.conv_gamma.kernel rounded to fp16 in the reference
    only.  Exactly the site that reads gen.rb3.spade_1.gb.kernel fails, and no other, at GauGAN(256, 16).  Measured: under bf16x3
    the layer is a conv site (bound 5e-5) and its value check stands at 2.53x the bound, next to 661888 differing image words;
    under f16c the layer runs conv_gb_resident, whose kernel test bounds it at 2e-4 against the exact chain: the value check
    stands at 0.64x (blind to a 2^-11 weight rounding) and the bit compare of the uploaded stream (262083 words) is what fails."""
    from moonsuperresolution_amd import make_weights
    S, B = 256, 16
    sites = Sites(S, B, precision, weights=_rounded(make_weights("gaugan", S, seed=1234, bias_scale=0.05)),
                  tag=" CONTROL (wrong reference on purpose)", record=False)
    try:
        res = sites.run()
    finally:
        sites.close()
    bad = _failed(res)
    hit = [(op, fig) for op, fig, _ in res if op.get("wt") == "gen.rb3.spade_1.gb.kernel"]
    assert len(hit) == 1
    print("control", precision, hit[0][0]["kind"], {k: v for k, v in hit[0][1].items()})
    assert [b[1] for b in bad] == [hit[0][0]["out"]], bad
    assert hit[0][1]["weight_words_differ"] > 0


def test_one_differing_word_fails_a_site():
    """CPU: a single differing word of a bit-for-bit compare (one channel of .wexp, one bias value) fails the site; a value
    check at its bound does not."""
    op = {"kind": "conv", "out": "ws.gen.rb3.x1"}
    clean = {"K": 9216, "value": 1.0, "weight_words_differ": 0.0, "wexp_words_differ": 0.0, "in_border": 0.0}
    assert _failed([(op, clean, max(over_bound(clean).values()))]) == []
    for key in ("weight_words_differ", "wexp_words_differ", "bias_words_differ"):
        fig = dict(clean, **{key: 1.0})
        bad = _failed([(op, fig, max(over_bound(fig).values()))])
        assert len(bad) == 1 and list(bad[0][2]) == [key], bad


# ------------------------------------------------------------------------------------------------
# CPU: the dump's format
# ------------------------------------------------------------------------------------------------
def test_conv_forms_dump_parses():
    """tests/golden/conv_forms_256_16_f16c.txt is msr_debug_conv_forms of GauGAN(256, 16) under f16c: the parser yields one dict
    per op with integer fields, the ops the network has, and forms that REQUIRED_FORMS names."""
    from moonsuperresolution_amd.generator import parse_conv_forms
    ops_ = parse_conv_forms(open(os.path.join(ROOT, "tests", "golden", "conv_forms_256_16_f16c.txt")).read())
    kinds = [o["kind"] for o in ops_]
    assert kinds[0] == "smallcin" and kinds[-1] == "head" and kinds.count("dense") == 2 and kinds.count("latent") == 1
    assert kinds.count("norm_act") == 4 and kinds.count("moments") + kinds.count("moments_slabs") + \
        sum(o.get("mom", "-") != "-" for o in ops_) == 17
    checked = [o for o in ops_ if not o["kind"].startswith("moments")]
    assert len(checked) == _expected_op_count(256, 16, ops_)
    convs = [o for o in ops_ if o["kind"] in ("conv", "gbr")]
    assert all(isinstance(o[k], int) for o in convs for k in ("prec", "tile", "ksplit", "wt_frag", "no_cross", "epi", "out_split",
                                                             "ranges", "B", "r", "N"))
    assert all(o["img"] in ("F32", "BF16", "BF16_FRAG", "F16", "FP8", "F16C", "F16C6", "GBR") for o in convs)
    assert all((o["kind"] == "gbr") == (o["img"] == "GBR") == (o["ranges"] > 0) == (o["kernel"] == "gbr") for o in convs)
    assert all(o["kernel"] in ("generic", "bvgpr", "halo", "halo16", "pp", "sw", "gbr") for o in convs)
    assert {form_of(o) for o in checked} <= REQUIRED_FORMS
    assert ("gbr", PREC_F16C6, TILE_PP, False, 0, 0, 4) in {form_of(o) for o in checked}
    assert all("?" not in o.values() for o in ops_)

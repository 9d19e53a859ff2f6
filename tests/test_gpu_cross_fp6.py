"""GPU (-m gpu): the f16c mode's opt-in fp6 cross terms (MSR_FLAG_CROSS_FP6, Generator(cross="fp6")).

conv_gb_resident<false, true> (msr_op_spade_gbr_f16c6) writes the consumer's f16c6 chunk image (kernels.h PREC_F16C6): per pixel
and 32 channels 32 x fp16 | 32 x e2m3 of v / 2^E + the scale byte | 32 x e2m3 of (v - hi) / 2^(E - 11) + its scale byte, with
2^E the smallest power of two >= max|v| / 7.5 over the 32 channels — which two waves of the kernel hold, 16 each.
  1. the image, kernel level, against the f16c image of the same launch and the float64 chain;
  2. the image as the stream kernel's input;
  3. the plan under the flag, and the flag's checks in msr_create;
  4. the generator end to end at (128, 16): the first f16c6 tensor, the output against the float64 oracle, the range scan."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import make_latent_noise, make_weights, synthetic_patches
from tests.helpers import ref_conv, rel_linf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16C_TOL = 2.5e-4      # tests/test_gpu_baseline_configs.py: MODE_TOL["f16c"], inside TOL = 1e-3 (north_star)
TOL = 1e-3


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert torch.cuda.is_available()
    from moonsuperresolution_amd import ops
    c = ops.OpContext()
    yield c
    c.close()


_LAYER = {}


def _layer(ctx, B, S, r, C, shift):
    """Inputs of one SPADE layer built like test_spade_layer_resident_kernel builds them, the float64 chain of the layer and
    the two images of the resident kernel (f16c: msr_op_spade_gbr, f16c6: msr_op_spade_gbr_f16c6); once per shape."""
    key = (B, S, r, C, shift)
    if key not in _LAYER:
        from moonsuperresolution_amd import ops
        g = torch.Generator(device="cpu").manual_seed(1000 * B + r + C)
        src = (torch.rand((B, S, S, 2), generator=g) - 0.5).cuda()
        we = (torch.randn((3, 3, 2, 128), generator=g) / 3).cuda()
        be = (0.1 * torch.randn(128, generator=g)).cuda()
        wg = (torch.randn((3, 3, 128, C), generator=g) / 34).cuda()
        wb_ = (torch.randn((3, 3, 128, C), generator=g) / 34).cuda()
        bg, bb = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
        x = (3 + 2 * torch.randn((B, r >> shift, r >> shift, C), generator=g)).cuda()
        mean = x.mean((0, 1, 2)).contiguous()
        std = torch.sqrt(x.var((0, 1, 2), unbiased=False) + 1e-5).contiguous()
        w, bias = ops.spade_layout(wg, wb_, bg, bb)
        wimg = ops.gbr_weight_image(w)
        f = S // r
        mask = src[:, f // 2::f, f // 2::f][:, :r, :r]
        e = torch.relu(ref_conv(mask, we, be, 1))
        xr = x.double().cpu()
        if shift:
            xr = xr.repeat_interleave(2, 1).repeat_interleave(2, 2)
        v = ref_conv(e, wg, bg, 1) * ((xr - mean.double().cpu()) / std.double().cpu()) + ref_conv(e, wb_, bb, 1)
        want = torch.where(v >= 0, v, 0.2 * v)
        y8 = ops.spade_gbr(ctx, src, we, be, wimg, bias, r, x, shift, mean, std)
        y6 = ops.spade_gbr(ctx, src, we, be, wimg, bias, r, x, shift, mean, std, out_mode=5)
        torch.cuda.synchronize()
        _LAYER[key] = (want, y8.cpu(), y6.cpu())
    return _LAYER[key]


def _check_f16c6_against_f16c(y6, y8, what):
    """The f16c6 image ``y6`` and the f16c image ``y8`` (both zero-bordered, CPU) hold the same fp32 values: the piece bounds
    of test 1.  Returns (hi, l6) of the interior."""
    from moonsuperresolution_amd import ops
    cut = lambda t: t[:, 1:-1, 1:-1]                                          # noqa: E731
    hi8, _, lo8 = (cut(t) for t in ops.f16c_decode(y8))
    full = ops.f16c6_decode(y6)
    hi, h6, l6 = (cut(t) for t in full)
    v = hi8 + lo8
    Bn, r, _, Cn = v.shape
    blk = v.abs().reshape(Bn, r, r, Cn // 32, 32).amax(-1, keepdim=True).expand(Bn, r, r, Cn // 32, 32).reshape(v.shape)
    blk = blk.clamp_min(1e-300)
    assert torch.equal(hi, hi8), what                                         # both are f16_rn of the same fp32 value
    e_h6 = float(((h6 - v).abs() / blk).max())
    e_l6 = float(((l6 - lo8).abs() / blk).max())
    got = cut(y6).contiguous().view(torch.uint8).reshape(-1, 128)
    ref = ops.f16c6_activation_image(v.float().contiguous())[0].contiguous().view(torch.uint8).reshape(-1, 128)
    d88 = (got[:, 88].int() - ref[:, 88].int()).abs()
    print(f"{what}: |h6 - v| / blk = {e_h6:.4f} (<= 0.07), |l6 - lo8| / blk = 2^{np.log2(max(e_l6, 1e-300)):.2f} (<= 2^-13), "
          f"{int((d88 != 0).sum())} of {got.shape[0]} scale bytes differ from the host twin's")
    assert e_h6 <= 0.07, (what, e_h6)
    assert e_l6 <= 2.0 ** -13, (what, e_l6)
    assert int((d88 != 0).sum()) <= got.shape[0] // 100 and int(d88.max()) <= 1, what
    assert torch.equal(got[:, 88].int() - 11, got[:, 120].int()), what
    assert int(got[:, 89:96].max()) == 0 and int(got[:, 121:128].max()) == 0, what
    raw = y6.contiguous().view(torch.int32)                                   # the border, bit for bit
    assert int(raw[:, 0].abs().max()) == 0 and int(raw[:, -1].abs().max()) == 0 and \
        int(raw[:, :, 0].abs().max()) == 0 and int(raw[:, :, -1].abs().max()) == 0, what
    return hi, l6


@pytest.mark.parametrize("B,S,r,C,shift", [(1, 64, 16, 64, 0), (3, 64, 32, 128, 1), (2, 128, 32, 256, 1)])
def test_resident_kernel_writes_the_f16c6_image(ctx, B, S, r, C, shift):
    """msr_op_spade_gbr_f16c6 against msr_op_spade_gbr on identical inputs (one tile and one block; several tiles, two blocks,
    folded up-sample; four blocks, resize factor 4): the fp16 piece bit for bit, the fp6 pieces within e2m3's step on the
    block scale (worst cases 0.0667 blk and (2^-14.9 + 2^-15) blk), the scale bytes those of the host twin, zero bytes and
    border zero, and hi + l6 <= 2e-4 of the output range against the float64 chain (the resident kernel's own bound)."""
    want, y8, y6 = _layer(ctx, B, S, r, C, shift)
    hi, l6 = _check_f16c6_against_f16c(y6, y8, f"resident kernel f16c6 image B={B} S={S} r={r} C={C}")
    err = rel_linf((hi + l6).numpy(), want.numpy())
    print(f"  hi + l6 vs float64 chain: {err:.3e}")
    assert err <= 2e-4, err


def test_resident_kernel_feeds_the_stream_kernel(ctx):
    """The image of msr_op_spade_gbr_f16c6 as the input of the f16c6 conv (conv_igemm_f16c_sw, wexp = None): against the
    float64 evaluation of the three terms on the DECODED pieces, <= 5e-5 (test_conv_f16c6's bound)."""
    from moonsuperresolution_amd import ops
    B, S, r, C, shift = 3, 64, 32, 128, 1
    _, _, y6 = _layer(ctx, B, S, r, C, shift)
    g = torch.Generator(device="cpu").manual_seed(67)
    cout = 128
    w = (torch.randn((3, 3, C, cout), generator=g) / np.sqrt(9 * C) * torch.logspace(-2, 1, cout)).cuda()
    b = torch.randn(cout, generator=g).cuda()
    wimg, (wh, w6, wl) = ops.f16c6_weight_image(ops.kernel_layout(w))
    y = ops.conv3x3_f16c(ctx, y6.cuda(), wimg, None, b, r).cpu().numpy()
    xh, x6, xl = (t[:, 1:-1, 1:-1] for t in ops.f16c6_decode(y6))
    hwio = lambda t: t.cpu().permute(0, 2, 1).reshape(3, 3, C, cout)       # noqa: E731
    zero = torch.zeros(cout, dtype=torch.float64)
    emu = ref_conv(xh, hwio(wh), b, 1) + ref_conv(x6, hwio(wl), zero, 1) + ref_conv(xl, hwio(w6), zero, 1)
    err = rel_linf(y, emu.numpy())
    print(f"f16c6 conv on the resident kernel's image: vs its own three terms in fp64 {err:.3e}")
    assert err <= 5e-5, err


def _forms_text(gen):
    gen.prepare()
    buf = C.create_string_buffer(1 << 18)
    assert gen._lib.msr_debug_conv_forms(gen._h, buf, len(buf)) == 0
    return buf.value.decode()


def test_plan_keeps_the_resident_kernel_under_cross_fp6(hip_lib):
    """GauGAN(128, 16), f16c: by forms.hip the three SPADE layers of rb6 (r = 64; consumers 256 -> 128, 128 -> 128, 256 -> 128,
    256 whole tiles each, gamma|beta 512 / 256 columns) take f16c6 consumers; rb5's do not (128 tiles).  Those layers keep
    kind=gbr, now with out_split=5, in front of a consumer in PREC_F16C6 on the F16C6 weight image, and no mask-embedding
    launch reappears for them.  Without cross= nothing of the kind is planned.  The flag goes with F16C and not F16_MAIN."""
    from moonsuperresolution_amd import Generator, _lib
    from moonsuperresolution_amd.generator import parse_conv_forms
    gen = Generator(128, 16, precision="f16c", cross="fp6")
    assert gen.cross == "fp6" and gen.precision == "f16c"
    text = _forms_text(gen)
    forms = parse_conv_forms(text)
    gen.close()
    gbr5 = [op for op in forms if op["kind"] == "gbr" and op["out_split"] == 5]
    assert [op["out"] for op in gbr5] == ["ws.gen.rb6.a1", "ws.gen.rb6.a3", "ws.gen.rb6.a2"], [op["out"] for op in gbr5]
    for op in gbr5:
        assert op["no_cross"] == 0 and op["img"] == "GBR" and op["r"] == 64
        cons = [c for c in forms if c["kind"] == "conv" and c["in"] == op["out"]]
        assert len(cons) == 1 and cons[0]["prec"] == 5 and cons[0]["img"] == "F16C6" and cons[0]["ksplit"] == 1, cons
    # every f16c6 consumer is fed by the resident kernel, and no embedding launch writes an h buffer of rb6
    assert [c["in"] for c in forms if c["kind"] == "conv" and c["prec"] == 5 and c["img"] == "F16C6"] == [op["out"] for op in gbr5]
    assert not [op for op in forms if op["kind"] == "smallcin" and op["out"].startswith("ws.gen.rb6.h")]
    assert all(op["out_split"] == 4 for op in forms if op["kind"] == "gbr" and op["out_split"] != 5)

    plain = Generator(128, 16, precision="f16c")
    assert plain.cross == "fp8"
    ptext = _forms_text(plain)
    plain.close()
    assert "out_split=5" not in ptext and "F16C6" not in ptext
    # same launches otherwise: the two plans differ only in those three layers' formats
    assert [op["kind"] for op in parse_conv_forms(ptext)] == [op["kind"] for op in forms]

    lib = _lib.load()
    for flags in (32, 1 | 32, 1 | 8 | 16 | 32):
        cfg = _lib.MsrConfig(128, 16, 256, _lib.VARIANT_IDS["gaugan"], 0, flags)
        handle = C.c_void_p()
        assert lib.msr_create(C.byref(cfg), C.byref(handle)) == _lib.MSR_ERR_INVALID, flags
        assert b"MSR_FLAG_CROSS_FP6" in lib.msr_last_error(None), flags


def test_generator_with_fp6_cross_terms_matches_oracle(hip_lib):
    """GauGAN(128, 16), same weights, input and noise under cross="fp8" and cross="fp6".  The first f16c6 tensor of the plan
    has the same upstream in both runs: its fp16 piece equals the fp8 run's bit for bit and its pieces satisfy test 1's
    bounds.  The fp6 run's output holds f16c's bound against the float64 oracle; its range scan lists the format-5 tensors,
    none clipped, clamped or non-finite."""
    from moonsuperresolution_amd import Generator
    from oracle import generator_ref
    S, B = 128, 16
    w = make_weights("gaugan", S, seed=1234, bias_scale=0.05)
    eps = make_latent_noise(B, 256, 7)
    x = synthetic_patches(B, S, 0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = np.asarray(generator_ref.spade_call(x, w, "gaugan", eps, dtype=torch.float64), np.float64)
    out, img = {}, {}
    for cross in ("fp6", "fp8"):
        gen = Generator(S, B, variant="gaugan", weights=w, eps=eps, precision="f16c", cross=cross)
        out[cross] = gen(x, training=False)
        if cross == "fp6":
            forms = gen.conv_forms()
            first = next(op for op in forms if op["kind"] == "gbr" and op["out_split"] == 5)   # its name, from the forms line
            fmt5 = [op["out"] for op in forms if op.get("out_split") == 5]
            report = gen.range_report()
        img[cross] = torch.from_numpy(gen.debug_tensor(first["out"], (B, first["r"] + 2, first["r"] + 2, first["N"] // 2)))
        gen.close()
        del gen
        torch.cuda.empty_cache()
    err6, err8 = rel_linf(out["fp6"], ref), rel_linf(out["fp8"], ref)
    rec = dict(S=S, B=B, precision="f16c", oracle="float64", rel_linf_output_cross_fp6=err6, rel_linf_output_cross_fp8=err8)
    print("parity", rec)
    try:
        with open(os.path.join(ROOT, "profiles", "cross_fp6_parity.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    _check_f16c6_against_f16c(img["fp6"], img["fp8"], f"first f16c6 tensor of the plan ({first['out']})")
    assert out["fp6"].shape == (B, S, S, 1) and np.isfinite(out["fp6"]).all()
    assert err6 <= TOL and err6 <= F16C_TOL, (err6, err8)
    five = [r for r in report.records if r["format"] == 5]
    assert sorted(r["tensor"] for r in five) == sorted(fmt5) and len(five) == 3, ([r["tensor"] for r in five], fmt5)
    assert all(r["n_cross_clipped"] == 0 and r["n_clamped"] == 0 and r["n_nonfinite"] == 0 and r["n_total"] > 0 for r in five), five
    assert report.regime == "parity", str(report)

"""The plain fp32 conv with the affine epilogue (EPI_AFFINE: the pix2pix convs) through its kernel-level entry
msr_op_conv_affine, at the smallest shapes at which it can still go wrong.

The pix2pix plan launches conv_igemm_f32 in forms no other entry reaches: 4 x 4 taps at stride 2, 2 x 2 taps, an input that is a
channel slice of a wider buffer (in_px != Cin), an output that is one half of a concat buffer or every second pixel of it
(out_px = 2 * channels: the four parity launches of a Conv2DTranspose), the in-kernel affine epilogue (ksplit 1: scale and shift
per GEMM column, ReLU / LeakyReLU) and splitk_epilogue_kernel<EPI_AFFINE> (ksplit > 1).  Every case runs on the 64 x 64 tile
(tile 1) and on the 128 x 128 tile (tile 0, N = 128).

Reference: float64 of the same fp32 operands through oracle.generator_ref (conv2d_same on the HWIO kernel,
conv2d_transpose_same_s2 on the [kh, kw, Cout, Cin] kernel: neither knows the tap layout or the parity decomposition).  scale in
[0.5, 2] and shift (both signs) differ per channel, so a swapped or shifted channel index is an O(1) error.  Every output buffer is
pre-filled with a canary and compared bit for bit outside the written footprint: the border, the channels beside the written
half, and (after each parity launch) the pixels of the parities not yet written.

Bounds (tests.helpers.affine_site_check): tensor rel L-inf <= 1e-5 (test_conv_bias's fp32 bound); per output channel
max |y - ref| <= max(1e-5 * R_c, 4 * E_c), R_c = max |pre-activation| of the channel in float64 ("range" as everywhere in this
suite: the largest magnitude), E_c = the channel's error of the same oracle functions evaluated in plain fp32 on the CPU.

MEASURED on an MI355X (profiles/conv_affine_parity.jsonl; per form in MEASURED below): the largest per-channel error / bound of
any case is 0.21 (128 x 128 tile, whole K, 16 taps), the largest tensor figure 9.1e-7; the split-K cases stand lower (0.03 to 0.09),
their partial sums being shorter.  Nothing failed and no kernel was changed.

CPU (no gpu marker): the entry refuses what the kernel has no instantiation for before it looks at the handle or the device.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import affine_act, affine_site_check, p2p_parity_images, pad_hw
from tests.helpers import record_dir as _record_dir

# MEASURED on an MI355X, one full run of the 26 GPU cases: form -> (largest per-channel error / bound, largest tensor rel L-inf).
# No case wrote outside its footprint; in no case did 4 * E_c exceed 1e-5 * R_c, so every ratio is against 1e-5 * R_c.
MEASURED = {
    "tile=1 ksplit=1 taps=16 act=2": (0.116, 6.5e-7), "tile=1 ksplit=2 taps=16 act=2": (0.089, 6.1e-7),
    "tile=1 ksplit=16 taps=16 act=2": (0.034, 1.6e-7), "tile=0 ksplit=1 taps=16 act=2": (0.208, 9.1e-7),
    "tile=0 ksplit=2 taps=16 act=2": (0.080, 4.9e-7), "tile=0 ksplit=16 taps=16 act=2": (0.066, 2.0e-7),
    "tile=1 ksplit=1 taps=4 act=1": (0.080, 5.1e-7), "tile=1 ksplit=4 taps=4 act=1": (0.030, 2.2e-7),
    "tile=0 ksplit=1 taps=4 act=1": (0.080, 5.1e-7), "tile=0 ksplit=4 taps=4 act=1": (0.030, 2.2e-7),
    "tile=1 ksplit=1 taps=16 act=0": (0.129, 7.6e-7), "tile=auto taps=16 act=2": (0.035, 1.7e-7),
}

CANARY = 0x4B1DC0DE
LEAK = 0.3


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert torch.cuda.is_available()
    from moonsuperresolution_amd import ops
    c = ops.OpContext()
    yield c
    c.close()


def _record(**kw):
    try:
        os.makedirs(_record_dir(), exist_ok=True)
        with open(os.path.join(_record_dir(), "parity_conv_affine.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")
    except OSError:
        pass
    print("conv_affine", kw)


def _canary(shape):
    return torch.full(shape, CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


def _touched(buf, written):
    """number of 32-bit words outside the bool mask ``written`` (same shape) that no longer hold the canary"""
    return int(((buf.view(torch.int32) != CANARY) & ~written).sum())


def _affine(N, g, with_scale=True):
    scale = (0.5 + 1.5 * torch.rand(N, generator=g)) if with_scale else None
    shift = torch.randn(N, generator=g) * 0.75
    assert float(shift.min()) < 0 < float(shift.max())
    return scale, shift


def _pre(conv, scale, shift):
    return conv * scale.to(conv.dtype) + shift.to(conv.dtype) if scale is not None else conv + shift.to(conv.dtype)


def down_case(ctx, B, rout, N, tile, ks, with_scale=True, act=2, coff=32, cextra=32, cin_off=32, cin_total=96, seed=0):
    """4 x 4 stride 2 'same': Cin = 64 read as channels [cin_off, cin_off + 64) of a zero-bordered cin_total-channel buffer, written to
    channels [coff, coff + N) of the interior of a [B, rout + 2, rout + 2, N + cextra] buffer."""
    from moonsuperresolution_amd import ops
    from oracle import generator_ref
    cin, rin = 64, 2 * rout
    g = torch.Generator(device="cpu").manual_seed(4200 + seed + 7 * B + rout + N)
    x = torch.randn((B, rin, rin, cin_total), generator=g)
    w = torch.randn((4, 4, cin, N), generator=g) / np.sqrt(16 * cin)
    scale, shift = _affine(N, g, with_scale)
    xpad = pad_hw(x).cuda().contiguous()
    w_tnk = w.reshape(16, cin, N).permute(0, 2, 1).contiguous().cuda()
    ct = N + cextra
    out = _canary((B, rout + 2, rout + 2, ct))
    py, pb = (rout + 2) * ct, (rout + 2) * (rout + 2) * ct
    ipy, ipb = (rin + 2) * cin_total, (rin + 2) * (rin + 2) * cin_total
    ops.conv_affine(ctx, xpad, cin_off, (cin_total, ipy, ipb), w_tnk, scale.cuda() if with_scale else None, shift.cuda(), out,
                    py + ct + coff, (ct, py, pb), B, rout, cin, N, 4, 2, act, LEAK if act == 2 else 0.0, tile)
    torch.cuda.synchronize()
    xs = x[..., cin_off:cin_off + cin]
    pre = _pre(generator_ref.conv2d_same(xs.double(), w.double(), None, 2), scale, shift)
    out32 = affine_act(_pre(generator_ref.conv2d_same(xs, w, None, 2), scale, shift), act, LEAK)
    written = torch.zeros(out.shape, dtype=torch.bool, device="cuda")
    written[:, 1:-1, 1:-1, coff:coff + N] = True
    got = out[:, 1:-1, 1:-1, coff:coff + N].cpu()
    what = f"4x4 s2 B={B} rout={rout} N={N} tile={tile} ksplit={ks} scale={'given' if with_scale else 'null'} act={act}"
    res = affine_site_check(got, pre, act, LEAK, out32, what)
    res["canary_words_touched"] = _touched(out, written)
    return what, res


def up_case(ctx, B, r, N, tile, ks, seed=0):
    """Conv2DTranspose(4, 2, 'same') + affine + ReLU as the plan runs it: four 2 x 2 stride-1 launches, one per output parity, into the
    first N channels of a zero-bordered [B, 2 r + 2, 2 r + 2, N + 32] buffer."""
    from moonsuperresolution_amd import ops
    from oracle import generator_ref
    cin = 64
    g = torch.Generator(device="cpu").manual_seed(4300 + seed + 7 * B + r + N)
    x = torch.randn((B, r, r, cin), generator=g)
    k = torch.randn((4, 4, N, cin), generator=g) / np.sqrt(4 * cin)
    scale, shift = _affine(N, g)
    xpad = pad_hw(x).cuda().contiguous()
    imgs = p2p_parity_images(k).cuda()
    ct, R = N + 32, 2 * r + 2
    out = _canary((B, R, R, ct))
    row = R * ct
    ipx, ipy, ipb = cin, (r + 2) * cin, (r + 2) * (r + 2) * cin
    written = torch.zeros(out.shape, dtype=torch.bool, device="cuda")
    touched = 0
    for py in range(2):
        for px in range(2):
            ops.conv_affine(ctx, xpad, py * ipy + px * ipx, (ipx, ipy, ipb), imgs[py * 2 + px], scale.cuda(), shift.cuda(), out,
                            row + ct + py * row + px * ct, (2 * ct, 2 * row, R * row), B, r, cin, N, 2, 1, 1, 0.0, tile)
            torch.cuda.synchronize()
            written[:, 1 + py:-1:2, 1 + px:-1:2, :N] = True
            touched += _touched(out, written)         # the parities not yet launched still hold the canary
    pre = _pre(generator_ref.conv2d_transpose_same_s2(x.double(), k.double()), scale, shift)
    out32 = affine_act(_pre(generator_ref.conv2d_transpose_same_s2(x, k), scale, shift), 1, 0.0)
    got = out[:, 1:-1, 1:-1, :N].cpu()
    what = f"2x2 s1 x 4 parities B={B} r={r} N={N} tile={tile} ksplit={ks}"
    res = affine_site_check(got, pre, 1, 0.0, out32, what, parity=True)
    res["canary_words_touched"] = touched
    return what, res


def _finish(form, what, res):
    _record(case=what, form=form, ok=res["ok"], tensor_rel=res["tensor_rel"], worst_over_bound=res["ratio"], channel=res["channel"],
            error=res["error"], range=res["range"], allowance=res["allowance"], canary_words_touched=res["canary_words_touched"])
    assert res["canary_words_touched"] == 0, f"{what}: {res['canary_words_touched']} words outside the footprint were written"
    assert res["ok"], res["message"]


def _tile(tile, ks):
    return tile + 256 * ks


@pytest.mark.gpu
@pytest.mark.parametrize("with_scale", [True, False], ids=["scale", "noscale"])
@pytest.mark.parametrize("ks", [1, 2, 16])
@pytest.mark.parametrize("tile,N", [(1, 64), (0, 128)])
def test_down_4x4_stride2_slice_input(ctx, tile, N, ks, with_scale):
    """B = 3, rout = 8: M = 192 = one full 128-row tile and a masked tail on tile 0, three 64-row tiles on tile 1; 32 K-steps."""
    what, res = down_case(ctx, 3, 8, N, _tile(tile, ks), ks, with_scale)
    _finish(f"tile={tile} ksplit={ks} taps=16 act=2", what, res)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [1, 16])
@pytest.mark.parametrize("tile,N", [(1, 64), (0, 128)])
def test_bottleneck_one_pixel_per_sample(ctx, tile, N, ks):
    """down8's shape: a 2 x 2 input, one output pixel per sample (M = 3), written into a 1 x 1 padded buffer."""
    what, res = down_case(ctx, 3, 1, N, _tile(tile, ks), ks, coff=0, cextra=0, cin_off=0, cin_total=64, seed=1)
    _finish(f"tile={tile} ksplit={ks} taps=16 act=2", what, res)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [1, 4])
@pytest.mark.parametrize("B,r,N,tile", [(3, 1, 64, 1), (3, 4, 64, 1), (3, 8, 128, 1), (3, 8, 128, 0)])
def test_up_four_parity_launches(ctx, B, r, N, tile, ks):
    """r = 1 (up1: every tap but one reads the zero border), r = 4, and B * r * r = 192 >= 129 rows for the 128-row tile."""
    what, res = up_case(ctx, B, r, N, _tile(tile, ks), ks)
    _finish(f"tile={tile} ksplit={ks} taps=4 act=1", what, res)


@pytest.mark.gpu
def test_no_activation(ctx):
    what, res = down_case(ctx, 3, 8, 64, _tile(1, 1), 1, act=0, seed=2)
    _finish("tile=1 ksplit=1 taps=16 act=0", what, res)


@pytest.mark.gpu
def test_planner_form(ctx):
    """tile = -1: conv_form picks the 64 x 64 tile and ksplit 8 for (B 3, rout 8, N 64, 32 K-steps)."""
    what, res = down_case(ctx, 3, 8, 64, -1, "auto", seed=3)
    _finish("tile=auto taps=16 act=2", what, res)


# ---- CPU: the argument checks need no device --------------------------------------------------------------------------------------
def _call(**kw):
    """msr_op_conv_affine with a null handle and made-up, aligned addresses: valid arguments reach the 'null handle' refusal"""
    from moonsuperresolution_amd import ops
    a = dict(B=3, rout=8, cin=64, n=64, k=4, stride=2, act=2, tile=1, in_pitch=(96, 18 * 96, 18 * 18 * 96), out_off=10 * 96 + 96 + 32,
             out_pitch=(96, 10 * 96, 100 * 96), x=0x10000, w=0x20000, scale=0x30000, shift=0x40000, out=0x50000)
    a.update(kw)
    return ops.conv_affine(None, a["x"], 0, a["in_pitch"], a["w"], a["scale"], a["shift"], a["out"], a["out_off"], a["out_pitch"],
                           a["B"], a["rout"], a["cin"], a["n"], a["k"], a["stride"], a["act"], 0.3, a["tile"])


@pytest.mark.parametrize("bad,text", [
    (dict(rout=12), "power of two"), (dict(cin=48), "multiple of 32"), (dict(n=96), "of 64"), (dict(n=64, tile=0), "128 x 128"),
    (dict(tile=2), "tile"), (dict(tile=1 + 256 * 33), "ksplit"), (dict(stride=3), "stride"), (dict(act=3), "act"),
    (dict(in_pitch=(48, 18 * 96, 18 * 18 * 96)), "in_px >= Cin"), (dict(in_pitch=(96, 18 * 96 + 2, 18 * 18 * 96)), "multiples of 4"),
    (dict(out_off=10 * 96 + 96 + 30), "multiples of 4"), (dict(out_pitch=(32, 10 * 96, 100 * 96)), "out_px >= N"),
    (dict(x=0x10004), "16-byte"), (dict(shift=0), "null"), (dict(out_pitch=(96, 10 * 96, 1 << 30)), "32-bit"),
    (dict(), "null handle")])
def test_conv_affine_rejects_without_a_device(hip_lib, bad, text):
    """Every refusal comes with its message before the handle or a device is looked at (the last case: nothing wrong but the handle)."""
    with pytest.raises(ValueError, match=text):
        _call(**bad)

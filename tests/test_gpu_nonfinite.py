"""GPU (-m gpu): NaN is data.  Every kernel entry, and the generator, on inputs in which a few elements are NaN.

The reference returns NaN for a patch with a NaN pixel (the tiler hands such a patch on as valid: tests/test_gpu_tiler.py::
test_nan_pixel_and_flat_patch_normalise_like_numpy), and the stitched product shows the hole.  The contract pinned here
(include/moonsr.h "Non-finite inputs"; tests.helpers.check_nan_contract, controls in tests/test_nonfinite_host.py):
  1 mask       isnan(out) == isnan(ref) element by element; for an image output "out" is the decoded main piece
  2 no spread  where ref is finite the output is bit-identical to the same launch with the planted elements set to 0.0,
               cross pieces and scale bytes of the other channels of a poisoned pixel's 32-channel block included
  3 value      over the finite elements the bound of the kernel's own existing test (cited at each case; no new tolerance)
  4 cap        at least half of the reference is finite (asserted on the reference first)
ref is the float64 reference the existing test of the kernel uses (torch follows IEEE: relu(NaN) = NaN, 0 * NaN = NaN).

Plants: image corner (0, 0), last pixel (r - 1, r - 1), an interior pixel of the LAST sample, and for r >= 32 one pixel each side
of the 16 x 16 tile seam (x = 15 in row 3, x = 16 in row r - 4: footprints apart); input channels 0, one in the middle of a
32-block (37 where there is one) and the last, in turn.  mean[c] / std[c] plants make one whole output channel NaN (1 / C of the
output: inside the cap).  Every case appends one line to parity_nonfinite.jsonl in the run-record directory.

What the cases pin, site by site (DESIGN.md "Non-finite inputs"): relu written as a comparison, not fmaxf (conv_smallcin act = 1;
EPI_AFFINE in the kernel's own epilogue and in the split-K pass, ReLU and LeakyReLU, through msr_op_conv_affine
(test_conv_affine), and through the pix2pix network); conv_gb_resident's v_med3_f32 clamps (phase 1: the lattice cases; SPADE epilogue: x /
mean / std); the transposed head's absent taps (test_head[True]); and MODE.FP16_OVFL: with the bit set the 16-bit and 8-bit
MFMAs of the MI355X read a NaN operand as a finite number, so no MFMA may run with it set (every case with NaN in a conv's
activation; for a launch that also converts to a narrow image: NaN in h with out_mode 3 / 4 / 5, the lattice cases, the fused head).
Network level: the S = 64 generators (bf16x3 kernels and fp32), the smallest shape whose plan has a resident-kernel op and a
stream-kernel conv in f16c / f16 / fp8 with the range report, pix2pix, and one raster through the tiler.
Not covered at kernel level: conv_direct_kernel (pix2pix down1), which has no entry; the pix2pix network test runs its one
planned form."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import (_ref_f16c, check_nan_contract, later_round_mask, record_dir as _record_dir, ref_conv, rel_linf, smallcin_ref,
                           unsplit)

pytestmark = pytest.mark.gpu
NAN = float("nan")
U = 2.0 ** -24
SW_MODE = os.environ.get("MSR_F16C_SW", "1")


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert torch.cuda.is_available()
    from moonsuperresolution_amd import ops
    c = ops.OpContext()
    yield c
    c.close()


def _record(case, n_planted, rec):
    line = dict(case=case, planted=n_planted, nan_in_ref=rec["n_nan_ref"], outputs=rec["n_total"], worst_finite_error=rec["worst"],
                bound=rec["bound"], MSR_F16C_SW=SW_MODE)
    os.makedirs(_record_dir(), exist_ok=True)
    with open(os.path.join(_record_dir(), "parity_nonfinite.jsonl"), "a") as f:
        f.write(json.dumps(line) + "\n")
    print("nonfinite", line)


def _positions(B, r):
    pos = [(0, 0, 0), (0, r - 1, r - 1), (B - 1, r // 2 - 1, r // 2 + 2)]
    if r >= 32:
        pos += [(0, 3, 15), (0, r - 4, 16)]
    return pos


def _plants(B, r, C):
    ch = (0, 37 if C > 37 else C // 2, C - 1)
    return [(b, y, x, ch[i % 3]) for i, (b, y, x) in enumerate(_positions(B, r))]


def _planted(t, plants):
    """-> (t with NaN at the plants, t with 0.0 there)."""
    a, b = t.clone(), t.clone()
    for p in plants:
        a[p], b[p] = NAN, 0.0
    return a, b


def _check(case, run, ref_fn, inputs, key, plants, bound, err_fn=rel_linf, exempt=None, raw_fn=None):
    """One case: ``run(inputs) -> main values`` (and ``raw_fn(inputs-run state)``), ``ref_fn(inputs) -> float64``; inputs[key] gets
    the plants."""
    nan_t, clean_t = _planted(inputs[key], plants)
    ref = ref_fn(dict(inputs, **{key: nan_t}))
    ref = ref.numpy() if hasattr(ref, "numpy") else ref
    out = run(dict(inputs, **{key: nan_t}))
    clean = run(dict(inputs, **{key: clean_t}))
    raw = None
    if isinstance(out, tuple):
        (out, raw_o), (clean, raw_c) = out, clean
        keep = np.broadcast_to(np.isfinite(ref), raw_o.shape) if raw_fn is None else raw_fn(np.isfinite(ref), raw_o)
        raw = (raw_o, raw_c, keep)
    rec = check_nan_contract(out, ref, clean, bound, err_fn, what=case, exempt=exempt, raw=raw)
    _record(case, len(plants), rec)
    return rec


def _conv_inputs(B, r, cin, cout, stride=1, res=None, seed=0):
    g = torch.Generator(device="cpu").manual_seed(900 + seed + B + r + cin)
    x = torch.randn((B, r * stride, r * stride, cin), generator=g)
    w = torch.randn((3, 3, cin, cout), generator=g) / np.sqrt(9 * cin)
    b = torch.randn(cout, generator=g)
    skip = torch.randn((B, r >> res, r >> res, cout), generator=g) if res is not None else None
    return dict(x=x, w=w, b=b, skip=skip)


def _up(t, shift):
    return t.repeat_interleave(1 << shift, 1).repeat_interleave(1 << shift, 2) if shift else t


def _conv_ref(stride=1, res=None):
    def ref(d):
        y = ref_conv(d["x"], d["w"], d["b"], stride)
        return y + _up(d["skip"].double(), res) if res is not None else y
    return ref


def _spade_inputs(B, r, C, shift, seed=0):
    g = torch.Generator(device="cpu").manual_seed(950 + seed + B + r + C)
    h = torch.relu(torch.randn((B, r, r, 128), generator=g))
    wg, wb = torch.randn((3, 3, 128, C), generator=g) / 34, torch.randn((3, 3, 128, C), generator=g) / 34
    bg, bb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    x = 3 + 2 * torch.randn((B, r >> shift, r >> shift, C), generator=g)
    return dict(h=h, wg=wg, wb=wb, bg=bg, bb=bb, x=x, mean=x.mean((0, 1, 2)).contiguous(),
                std=torch.sqrt(x.var((0, 1, 2), unbiased=False) + 1e-5).contiguous())


def _spade_of(gam, bet, d, shift):
    v = gam * ((_up(d["x"].double(), shift) - d["mean"].double()) / d["std"].double()) + bet
    return torch.where(v >= 0, v, 0.2 * v)


def _spade_ref(shift):
    return lambda d: _spade_of(ref_conv(d["h"], d["wg"], d["bg"], 1), ref_conv(d["h"], d["wb"], d["bb"], 1), d, shift)


def _spade_plant_sets(B, r, C, shift, act="h"):
    """name -> (key, plants, exempt) for the SPADE operands: the activation, x (at its own resolution), mean[c], std[c]."""
    ra = r >> shift
    return {act: (act, _plants(B, r, 128)), "x": ("x", _plants(B, ra, C)), "mean": ("mean", [(0,), (C - 1,)]),
            "std": ("std", [(37 % C,)])}


# ---- conv3x3 fp32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_fp32_activation(ctx, tile, stride):
    """conv_igemm_f32 at (2, 16, 64, 128); bound 1e-5 (tests/test_gpu_conv_kernel.py::test_conv_bias)."""
    from moonsuperresolution_amd import ops
    B, r, cin, cout = 2, 16, 64, 128
    d = _conv_inputs(B, r, cin, cout, stride)
    run = lambda d: ops.conv3x3(ctx, ops.pad_nhwc(d["x"].cuda()), ops.kernel_layout(d["w"].cuda()), d["b"].cuda(), r, stride=stride,   # noqa: E731
                                tile=tile).cpu().numpy()
    _check(f"conv3x3 fp32 tile {tile} stride {stride} activation", run, _conv_ref(stride), d, "x", _plants(B, r * stride, cin), 1e-5)


@pytest.mark.parametrize("shift", [0, 1])
def test_conv_fp32_residual_aux(ctx, shift):
    """EPI_RES, NaN in aux: exactly the pixels that read it (a 2 x 2 block at shift 1), one output channel; bound 1e-5
    (test_conv_residual_with_upsample_fold)."""
    from moonsuperresolution_amd import ops
    B, r, cin, cout = 2, 16, 64, 128
    d = _conv_inputs(B, r, cin, cout, res=shift)
    run = lambda d: ops.conv3x3(ctx, ops.pad_nhwc(d["x"].cuda()), ops.kernel_layout(d["w"].cuda()), d["b"].cuda(), r,      # noqa: E731
                                epilogue=ops.EPI_RES, aux=d["skip"].cuda(), aux_shift=shift, tile=0).cpu().numpy()
    rec = _check(f"conv3x3 fp32 EPI_RES aux shift {shift}", run, _conv_ref(1, shift), d, "skip", _plants(B, r >> shift, cout), 1e-5)
    assert rec["n_nan_ref"] == 3 * (4 if shift else 1)


@pytest.mark.parametrize("where", ["h", "x", "mean", "std"])
def test_conv_fp32_spade(ctx, where):
    """EPI_SPADE at C = 64 (N = 128), x through the folded up-sample; bound 1e-5 (test_conv_spade_epilogue)."""
    from moonsuperresolution_amd import ops
    B, r, C, shift = 2, 16, 64, 1
    d = _spade_inputs(B, r, C, shift)

    def run(d):
        w, bias = ops.spade_layout(d["wg"].cuda(), d["wb"].cuda(), d["bg"].cuda(), d["bb"].cuda())
        y = ops.conv3x3(ctx, ops.pad_nhwc(d["h"].cuda()), w, bias, r, epilogue=ops.EPI_SPADE, aux=d["x"].cuda(), aux_shift=shift,
                        mean=d["mean"].cuda(), std=d["std"].cuda(), out_padded=True, tile=0).cpu()
        assert float(y[:, 0].abs().max()) == 0 and float(y[:, :, -1].abs().max()) == 0        # the border stays zero
        return y[:, 1:-1, 1:-1].numpy()
    key, plants = _spade_plant_sets(B, r, C, shift)[where]
    _check(f"conv3x3 fp32 EPI_SPADE NaN in {where}", run, _spade_ref(shift), d, key, plants, 1e-5)


@pytest.mark.parametrize("ks", [1, 4])
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("where", ["x", "w"])
def test_conv_affine(ctx, where, act, ks):
    """EPI_AFFINE through msr_op_conv_affine, in the kernel's own epilogue (ksplit 1) and in the split-K pass (ksplit 4), ReLU and
    LeakyReLU(0.3): the 4 x 4 stride-2 B = 3 shape of tests/test_gpu_conv_affine.py (Cin = 64 read as channels [32, 96) of a
    96-channel buffer, N = 64, rout = 8, 64 x 64 tile).  NaN in the activation (inside the slice), or in one weight row (tap (1, 2)
    of output channel 37: that whole channel is NaN, 1 / 64 of the output).  Bound 1e-5 (test_conv_bias)."""
    from moonsuperresolution_amd import ops
    from oracle import generator_ref
    from tests.helpers import affine_act, pad_hw
    B, rout, cin, N, off, ctot = 3, 8, 64, 64, 32, 96
    g = torch.Generator(device="cpu").manual_seed(990 + act)
    d = dict(x=torch.randn((B, 2 * rout, 2 * rout, ctot), generator=g), w=torch.randn((4, 4, cin, N), generator=g) / 32,
             scale=0.5 + 1.5 * torch.rand(N, generator=g), shift=torch.randn(N, generator=g) * 0.75)
    slope = 0.3 if act == 2 else 0.0

    def run(d):
        out = torch.zeros((B, rout + 2, rout + 2, N + 32), device="cuda")
        ct, rin = N + 32, 2 * rout + 2
        ops.conv_affine(ctx, pad_hw(d["x"]).cuda().contiguous(), off, (ctot, rin * ctot, rin * rin * ctot),
                        d["w"].reshape(16, cin, N).permute(0, 2, 1).contiguous().cuda(), d["scale"].cuda(), d["shift"].cuda(), out,
                        (rout + 2) * ct + ct + 32, (ct, (rout + 2) * ct, (rout + 2) * (rout + 2) * ct), B, rout, cin, N, 4, 2, act, slope,
                        1 + 256 * ks)
        y = out.cpu()
        assert float(y[:, 0].abs().max()) == 0 and float(y[:, :, -1].abs().max()) == 0 and float(y[..., :32].abs().max()) == 0
        return y[:, 1:-1, 1:-1, 32:].numpy()

    def ref(d):
        pre = generator_ref.conv2d_same(d["x"][..., off:off + cin].double(), d["w"].double(), None, 2) * d["scale"].double() + d["shift"].double()
        return affine_act(pre, act, slope)
    plants = [(b, y, x, off + c) for b, y, x, c in _plants(B, 2 * rout, cin)] if where == "x" else [(1, 2, slice(None), 37)]
    _check(f"conv_affine 4x4 s2 act {act} ksplit {ks} NaN in {where}", run, ref, d, where, plants, 1e-5)


# ---- bf16x3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,shape", [(5, (2, 16, 128, 256)), (3, (2, 16, 128, 256)), (4, (2, 16, 128, 256)), (1 | 0x40, (2, 16, 64, 128)),
                                        (5 + 256 * 2, (2, 16, 128, 256))])
def test_conv_bf16x3_activation(ctx, tile, shape):
    """The activation is split on the device from a NaN-holding fp32 tensor (split_bf16_kernel: hi and lo NaN).  Bound 5e-5
    (test_conv_bf16x3)."""
    from moonsuperresolution_amd import ops
    B, r, cin, cout = shape
    d = _conv_inputs(B, r, cin, cout, seed=1)

    def run(d):
        wk = ops.kernel_layout(d["w"].cuda())
        ws = ops.weights_bf16x3(wk) if tile & 0x40 else ops.split_bf16(ctx, wk)
        return ops.conv3x3(ctx, ops.split_bf16(ctx, ops.pad_nhwc(d["x"].cuda())), ws, d["b"].cuda(), r, tile=tile,
                           precision="bf16x3").cpu().numpy()
    _check(f"conv3x3 bf16x3 tile {tile:#x} activation", run, _conv_ref(), d, "x", _plants(B, r, cin), 5e-5)


@pytest.mark.parametrize("form", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("where", ["h", "x", "mean", "std"])
def test_conv_bf16x3_spade_split_output(ctx, where, form):
    """SPADE epilogue writing split words (out_split): main piece hi; the lo halves of every finite element are bit-identical
    too.  bf16x3 tile 5: bound 5e-5 on hi + lo (test_conv_spade_epilogue_bf16x3_split_output); the f16x2 form: 5e-4
    (test_conv_spade_epilogue_f16x2, against the unrounded chain)."""
    from moonsuperresolution_amd import ops
    B, r, C, shift = 2, 16, 64, 1
    d = _spade_inputs(B, r, C, shift, seed=2)
    split = (lambda t: ops.split_bf16(ctx, t)) if form == "bf16x3" else ops.split_f16
    tile = 5 if form == "bf16x3" else ops.TILE_PP | ops.TILE_F16X2

    def words(y):
        u = y.contiguous().view(torch.int16).reshape(-1, 2, 32)         # both forms write split-bf16 words for their consumer
        return tuple(u[:, k].contiguous().view(torch.bfloat16).float().reshape(y.shape) for k in (0, 1))

    def run(d):
        w, bias = ops.spade_layout(d["wg"].cuda(), d["wb"].cuda(), d["bg"].cuda(), d["bb"].cuda())
        y = ops.conv3x3(ctx, split(ops.pad_nhwc(d["h"].cuda())), split(w), bias, r, epilogue=ops.EPI_SPADE, aux=d["x"].cuda(),
                        aux_shift=shift, mean=d["mean"].cuda(), std=d["std"].cuda(), out_padded=True, tile=tile, precision="bf16x3",
                        out_split=True).cpu()
        hi, lo = words(y)
        assert float(hi[:, 0].abs().max()) == 0 and float(lo[:, :, -1].abs().max()) == 0
        hi, lo = hi[:, 1:-1, 1:-1].numpy(), lo[:, 1:-1, 1:-1].numpy()
        return (hi, lo)
    key, plants = _spade_plant_sets(B, r, C, shift)[where]
    nan_t, clean_t = _planted(d[key], plants)
    ref = _spade_ref(shift)(dict(d, **{key: nan_t})).numpy()
    (hi, lo), (chi, clo) = run(dict(d, **{key: nan_t})), run(dict(d, **{key: clean_t}))
    fin = np.isfinite(ref)
    # value on hi + lo (what the consumer multiplies), mask and bits on hi, bits on lo
    rec = check_nan_contract(hi, ref, chi, 5e-5 if form == "bf16x3" else 5e-4,
                             lambda o, rf: rel_linf(np.where(fin, hi.astype(np.float64) + lo, 0.0), rf),
                             what=f"{form} SPADE out_split NaN in {where}", raw=(lo, clo, fin))
    _record(f"conv3x3 {form} EPI_SPADE out_split NaN in {where}", len(plants), rec)


# ---- f16c family -----------------------------------------------------------------------------------------------------------------
def _f16c_kernel(ctx, cin, epi, out_mode=0, ks=1, direct=False):
    """Which kernel a msr_op_conv3x3_f16c launch runs in this process: the library's answer (msr_debug_f16c_kernel) for whole-tile
    launches, checked against the meaning of MSR_F16C_SW as tests/test_gpu_conv_channels.py states it (1: bias / residual launches
    with Cin % 128 == 0 on the stream kernel; 0: none; 2: all of those but the f16c6 image output).  K ranges always run the
    ping-pong kernel, no_cross and f16c6 launches (``direct``) the stream kernel."""
    if direct:
        return "stream"
    if ks > 1:
        return "ping-pong"
    want = cin % 128 == 0 and not (epi == 2 and out_mode == 5) and (SW_MODE == "2" or (SW_MODE == "1" and epi != 2))
    got = ctx.lib.msr_debug_f16c_kernel(cin, epi, out_mode)
    assert got == int(want), f"MSR_F16C_SW={SW_MODE}: the library sends cin={cin} epi={epi} out_mode={out_mode} to kernel {got}"
    return "stream" if got else "ping-pong"


def _f16c_conv_case(ctx, case, shape, res=None, ks=1, nox=False, f6=False, plants=None, later=None):
    """One bias / residual launch of msr_op_conv3x3_f16c with NaN in the activation image (built by the host twin: NaN hi, NaN
    cross bytes).  Reference: the float64 evaluation of the kernel's own terms on the decoded pieces, bound 5e-5
    (test_conv_f16c, test_conv_f16c6, test_conv_f16c_no_cross's own-terms statement)."""
    from moonsuperresolution_amd import ops
    B, r, cin, cout = shape
    d = _conv_inputs(B, r, cin, cout, res=res, seed=3)
    if f6:
        d["x"] = d["x"] * torch.logspace(-1.5, 0.5, cin)
    wk = ops.kernel_layout(d["w"].cuda())
    wexp = None
    if f6:
        wimg, wparts = ops.f16c6_weight_image(wk)
    else:
        wimg, wexp, wparts = ops.f16c_weight_image(wk)
    image = ops.f16c6_activation_image if f6 else ops.f16c_activation_image
    kernel = _f16c_kernel(ctx, cin, 0 if res is None else 1, ks=ks, direct=f6 or nox)
    print(f"dispatch: {case} under MSR_F16C_SW={SW_MODE} ran the {kernel} kernel")
    hwio = lambda t: t.cpu().permute(0, 2, 1).reshape(3, 3, cin, cout)      # noqa: E731
    zero = torch.zeros(cout, dtype=torch.float64)

    def ref(d):
        xh, x8, xl = (t[:, 1:-1, 1:-1].cpu() for t in image(ops.pad_nhwc(d["x"].cuda()))[1])
        y = ref_conv(xh, hwio(wparts[0]), d["b"], 1)
        if not nox:
            # f16c: x_h8 * w_lo8 + x_lo8 * w_h8 (wparts = hi, h8, lo8); f16c6: x_h6 * w_l6 + x_l6 * w_h6 (wparts = hi, h6, l6)
            y = y + ref_conv(x8, hwio(wparts[2]), zero, 1) + ref_conv(xl, hwio(wparts[1]), zero, 1)
        return y + _up(d["skip"].double(), res) if res is not None else y

    def run(d):
        return ops.conv3x3_f16c(ctx, image(ops.pad_nhwc(d["x"].cuda()))[0], wimg, wexp, d["b"].cuda(), r,
                                epilogue=ops.EPI_BIAS if res is None else ops.EPI_RES, aux=d["skip"].cuda() if res is not None else None,
                                aux_shift=res or 0, ksplit=ks, no_cross=nox).cpu().numpy()
    plants = plants or _plants(B, r, cin)
    nan_t, clean_t = _planted(d["x"], plants)
    refv = ref(dict(d, x=nan_t)).numpy()
    out, clean = run(dict(d, x=nan_t)), run(dict(d, x=clean_t))
    rec = check_nan_contract(out, refv, clean, 5e-5, rel_linf, what=case)
    _record(case, len(plants), rec)
    return out, clean, refv


@pytest.mark.parametrize("case,shape,res,ks,nox", [
    pytest.param("f16c stream bias", (2, 16, 128, 256), None, 1, False, id="B-bias"),
    pytest.param("f16c stream residual shift 1", (2, 16, 128, 256), 1, 1, False, id="B-res1"),
    pytest.param("f16c ping-pong bias", (2, 16, 64, 256), None, 1, False, id="A-pp-bias"),
    pytest.param("f16c K ranges ks=2 bias", (1, 16, 256, 256), None, 2, False, id="C-ks2-bias"),
    pytest.param("f16c K ranges ks=4 residual shift 0", (1, 16, 256, 256), 0, 4, False, id="C-ks4-res0"),
    pytest.param("f16c stream no_cross bias", (2, 16, 128, 256), None, 1, True, id="B-nocross-bias")])
def test_f16c_conv_activation(ctx, case, shape, res, ks, nox):
    _f16c_conv_case(ctx, case, shape, res, ks, nox)


def test_f16c6_conv_activation(ctx):
    """The f16c6 stream kernel at (1, 32, 128, 256): plants on both sides of the tile seam."""
    _f16c_conv_case(ctx, "f16c6 stream bias", (1, 32, 128, 256), f6=True)


def test_f16c_residual_aux(ctx):
    """NaN in the residual of the stream kernel: exactly the 2 x 2 pixels that read it, one channel."""
    from moonsuperresolution_amd import ops
    B, r, cin, cout = 2, 16, 128, 256
    d = _conv_inputs(B, r, cin, cout, res=1, seed=4)
    ximg, xparts = ops.f16c_activation_image(ops.pad_nhwc(d["x"].cuda()))
    wimg, wexp, wparts = ops.f16c_weight_image(ops.kernel_layout(d["w"].cuda()))
    conv = _ref_f16c(tuple(t[:, 1:-1, 1:-1].cpu() for t in xparts), tuple(t.cpu() for t in wparts), d["b"], cin, cout)
    run = lambda d: ops.conv3x3_f16c(ctx, ximg, wimg, wexp, d["b"].cuda(), r, epilogue=ops.EPI_RES, aux=d["skip"].cuda(),       # noqa: E731
                                     aux_shift=1).cpu().numpy()
    rec = _check("f16c stream residual, NaN in aux", run, lambda d: conv + _up(d["skip"].double(), 1), d, "skip", _plants(B, r >> 1, cout), 5e-5)
    assert rec["n_nan_ref"] == 12


def _f16c_raw_keep(fin, raw):
    """Bytes of an f16c chunk image [B, r, r, C * 4] that must not change: everything but the 4 bytes of each NaN element
    (2 of hi at 2c, h8 at 64 + c, l8 at 96 + c of its 128-byte chunk)."""
    B, r, _, C = fin.shape
    keep = np.ones((B, r, r, C // 32, 128), bool)
    f = fin.reshape(B, r, r, C // 32, 32)
    keep[..., 0:64:2], keep[..., 1:64:2], keep[..., 64:96], keep[..., 96:128] = f, f, f, f
    return keep.reshape(raw.shape)


def _f16c6_keep(fin, clean_hi, shape):
    """Elements of the decoded 6-bit pieces [2, B, r, r, C] of an f16c6 image that must equal the clean launch's: the finite ones,
    except in a 32-channel block whose largest clean |value| sits at a NaN position.  The block's scale is the maximum over its
    finite elements (the NaN is dropped from it on purpose); the clean launch has an ordinary value where the NaN is, and where
    that value is the block's largest the two launches rightly pick different scales."""
    B, r, _, C = fin.shape
    f = fin.reshape(B, r, r, C // 32, 32)
    a = np.abs(clean_hi.reshape(f.shape))
    same_scale = np.where(f, a, 0.0).max(-1) >= np.where(f, 0.0, a).max(-1)
    keep = f & same_scale[..., None]
    assert keep.any()
    return np.broadcast_to(keep.reshape(fin.shape), shape)


def _f16c6_scale_bytes_unchanged(case, fin, clean_hi, img_n, img_c):
    """The two scale bytes (88: h6, 120: l6) and the zero bytes behind them of every chunk that holds a finite element and whose
    scale the NaN position does not decide (as _f16c6_keep): those of the clean launch, byte for byte."""
    B, r, _, C = fin.shape
    f = fin.reshape(B, r, r, C // 32, 32)
    a = np.abs(clean_hi.reshape(f.shape))
    blk = f.any(-1) & (np.where(f, a, 0.0).max(-1) >= np.where(f, 0.0, a).max(-1))
    bn, bc = (t.reshape(B, r, r, C // 32, 128) for t in (img_n, img_c))
    assert blk.any()
    for lo, hi in ((88, 96), (120, 128)):
        assert np.array_equal(bn[..., lo:hi][blk], bc[..., lo:hi][blk]), f"{case}: scale bytes {lo}.. changed outside the footprint"


@pytest.mark.parametrize("where", ["h", "x", "mean", "std"])
@pytest.mark.parametrize("mode,ks", [(0, 1), (1, 1), (4, 1), (5, 1), (0, 2), (4, 2)])
def test_f16c_spade(ctx, mode, ks, where):
    """The f16c gamma|beta conv + SPADE epilogue at (2, 16, 128, N = 512), x through the folded up-sample.  Reference: the float64
    SPADE of the kernel's own three terms.  out_mode 0: 5e-5; 1: hi + lo 5e-5; 4 / 5: the main piece hi is the fp16 rounding of
    the value, 2^-11 of the range on top of the 5e-5 (tests/test_gpu_conv_kernel.py::_check_f16c_spade, which states the 2^-11
    against the kernel's own fp32 output).  Images: the bytes (mode 4) or decoded 6-bit pieces and scale bytes (mode 5) of every
    finite element are those of the clean launch."""
    from moonsuperresolution_amd import ops
    B, r, C, shift = 2, 16, 256, 1
    d = _spade_inputs(B, r, C, shift, seed=5)
    w, bias = ops.spade_layout(d["wg"].cuda(), d["wb"].cuda(), d["bg"].cuda(), d["bb"].cuda())
    wimg, wexp, wparts = ops.f16c_weight_image(w)
    rows = (torch.arange(C) // 32) * 64 + torch.arange(C) % 32
    print(f"dispatch: f16c SPADE out_mode {mode} ks={ks} under MSR_F16C_SW={SW_MODE} ran the {_f16c_kernel(ctx, 128, 2, mode, ks)} kernel")

    def ref(d):
        hparts = ops.f16c_activation_image(ops.pad_nhwc(d["h"].cuda()))[1]
        gb = _ref_f16c(tuple(t[:, 1:-1, 1:-1].cpu() for t in hparts), tuple(t.cpu() for t in wparts), bias.cpu(), 128, 2 * C)
        return _spade_of(gb[..., rows], gb[..., rows + 32], d, shift)

    def run(d):
        y = ops.conv3x3_f16c(ctx, ops.f16c_activation_image(ops.pad_nhwc(d["h"].cuda()))[0], wimg, wexp, bias, r, epilogue=ops.EPI_SPADE,
                             aux=d["x"].cuda(), aux_shift=shift, mean=d["mean"].cuda(), std=d["std"].cuda(), out_padded=True,
                             out_mode=mode, ksplit=ks)
        inner = y[:, 1:-1, 1:-1].contiguous()
        border = y.clone()
        border[:, 1:-1, 1:-1] = 0
        assert int(border.view(torch.int32).abs().max()) == 0                     # the border stays zero, NaN or not
        if mode == 0:
            return inner.cpu().numpy()
        if mode == 1:
            hi, lo = unsplit(inner)
            return hi.cpu().numpy(), lo.cpu().numpy()
        if mode == 4:
            return ops.f16c_decode(inner)[0].cpu().numpy(), inner.view(torch.uint8).cpu().numpy()
        hi, h6, l6 = ops.f16c6_decode(inner)
        return hi.cpu().numpy(), torch.stack([h6, l6]).cpu().numpy(), inner.view(torch.uint8).cpu().numpy()
    key, plants = _spade_plant_sets(B, r, C, shift)[where]
    case = f"f16c SPADE out_mode {mode} ks={ks} NaN in {where}"
    nan_t, clean_t = _planted(d[key], plants)
    refv = ref(dict(d, **{key: nan_t})).numpy()
    fin = np.isfinite(refv)
    out, clean = run(dict(d, **{key: nan_t})), run(dict(d, **{key: clean_t}))
    rng = float(np.abs(refv[fin]).max())
    if mode == 0:
        rec = check_nan_contract(out, refv, clean, 5e-5, rel_linf, what=case)
    elif mode == 1:
        rec = check_nan_contract(out[0], refv, clean[0], 5e-5, lambda o, rf: rel_linf(np.where(fin, out[0].astype(np.float64) + out[1], 0.0), rf),
                                 what=case, raw=(out[1], clean[1], fin))
    else:
        keep = _f16c_raw_keep(fin, out[1]) if mode == 4 else _f16c6_keep(fin, clean[0], out[1].shape)
        rec = check_nan_contract(out[0], refv, clean[0], (2.0 ** -11 + 5e-5) * rng, lambda o, rf: np.abs(o - rf).max(), what=case,
                                 raw=(out[1], clean[1], keep))
        if mode == 5:
            _f16c6_scale_bytes_unchanged(case, fin, clean[0], out[2], clean[2])
    _record(case, len(plants), rec)


def test_f16c_second_round_tiles_do_not_see_a_first_round_nan(ctx):
    """Persistent re-use at (5, 64, 128, 512), bias, on the stream kernel (tests/test_gpu_conv_channels.py case G: 320 items on
    one workgroup per CU).  NaN in first-round tiles only, away from the second-round tiles' halos: every second-round tile is
    bit-identical to the clean launch (nothing stale in LDS or registers across tiles) - which rule 2 states for the whole
    tensor; here the second-round set is required to be non-empty and finite."""
    B, r, cin, N = 5, 64, 128, 512
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    later = later_round_mask(B, r, N, n_cu)                       # [B, 4, 4, 4]
    assert later.any(), f"{n_cu} CUs take {later.size} items in one round"
    tiles_later = later.any(-1)                                   # pixel tiles with a second-round item in any channel block
    plants = []
    for b in range(B):
        for ty in range(4):
            for tx in range(4):
                near = tiles_later[b, max(ty - 1, 0):ty + 2, max(tx - 1, 0):tx + 2].any()
                if not near and len(plants) < 6:
                    plants.append((b, 16 * ty + (0, 15, 7)[len(plants) % 3], 16 * tx + (15, 0, 8)[len(plants) % 3], (0, 37, 127)[len(plants) % 3]))
    assert plants, "no first-round tile away from the second-round tiles at this CU count"
    out, clean, refv = _f16c_conv_case(ctx, "f16c stream persistent re-use (5, 64, 128, 512)", (B, r, cin, N), plants=plants)
    px = np.repeat(np.repeat(np.repeat(later, 16, 1), 16, 2), 128, 3)
    assert np.isfinite(refv[px]).all() and np.array_equal(out[px].view(np.uint32), clean[px].view(np.uint32))


_CHILD_TESTS = "test_f16c_conv_activation or test_f16c_spade or test_f16c_residual_aux or test_f16c_second_round"


@pytest.mark.parametrize("mode", ["0", "2"])
def test_f16c_cases_under_the_other_kernel_dispatch(mode):
    """The f16c cases of this file once more in a child process under MSR_F16C_SW = 0 (ping-pong kernel) / 2 (stream kernel
    wherever it has a form), as tests/test_gpu_conv_channels.py does; each case asks the library which kernel it ran."""
    env = dict(os.environ, MSR_F16C_SW=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-rsP", "-k", _CHILD_TESTS],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " skipped" not in r.stdout.splitlines()[-1], r.stdout[-500:]
    ran = {ln.split(" ran the ")[1] for ln in r.stdout.splitlines() if ln.startswith("dispatch: ") and f"MSR_F16C_SW={mode}" in ln}
    assert {"ping-pong kernel", "stream kernel"} <= ran, sorted(ran)          # K ranges stay on ping-pong, no_cross on stream


# ---- fp8 -------------------------------------------------------------------------------------------------------------------------
def test_fp8_conv_bias(ctx):
    """conv3x3_fp8 at (2, 16, 128, 256): the bf8 activation byte of a NaN is a NaN byte; bound 5e-5 against the float64 conv of the
    de-quantised operands (test_conv_fp8_exact_on_quantised_operands)."""
    from moonsuperresolution_amd import ops
    B, r, cin, cout = 2, 16, 128, 256
    d = _conv_inputs(B, r, cin, cout, seed=6)
    wq, wexp, wdq = ops.fp8_weight_image(ops.kernel_layout(d["w"].cuda()))
    w_hwio = wdq.permute(0, 2, 1).reshape(3, 3, cin, cout)
    run = lambda d: ops.conv3x3_fp8(ctx, ops.bf8_activation_image(ops.pad_nhwc(d["x"].cuda()))[0], wq, wexp, d["b"].cuda(), r).cpu().numpy()   # noqa: E731
    ref = lambda d: ref_conv(d["x"].to(torch.float8_e5m2).float(), w_hwio, d["b"], 1)                                                      # noqa: E731
    _check("fp8 ping-pong bias", run, ref, d, "x", _plants(B, r, cin), 5e-5)


@pytest.mark.parametrize("where", ["h", "x", "mean", "std"])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_fp8_spade(ctx, mode, where):
    """The fp8 gamma|beta conv + SPADE epilogue, out_mode 0 (fp32), 1 (split-bf16), 3 (bf8 bytes: the byte is the main piece).
    Bounds of test_conv_fp8_spade_epilogue_bf8_output: 5e-5 (modes 0, 1); mode 3: within one bf8 step (|want| / 4, floor 2^-16)
    of the bf8 rounding of the reference."""
    from moonsuperresolution_amd import ops
    B, r, C, shift = 2, 16, 128, 1
    d = _spade_inputs(B, r, C, shift, seed=7)
    w, bias = ops.spade_layout(d["wg"].cuda(), d["wb"].cuda(), d["bg"].cuda(), d["bb"].cuda())
    wq, wexp, wdq = ops.fp8_weight_image(w)
    wdq_hwio = wdq.permute(0, 2, 1).reshape(3, 3, 128, 2 * C).cpu()
    rows = (torch.arange(C) // 32) * 64 + torch.arange(C) % 32

    def ref(d):
        hdq = d["h"].to(torch.float8_e5m2).float()
        return _spade_of(ref_conv(hdq, wdq_hwio[..., rows], d["bg"], 1), ref_conv(hdq, wdq_hwio[..., rows + 32], d["bb"], 1), d, shift)

    def run(d):
        y = ops.conv3x3_fp8(ctx, ops.bf8_activation_image(ops.pad_nhwc(d["h"].cuda()))[0], wq, wexp, bias, r, epilogue=ops.EPI_SPADE,
                            aux=d["x"].cuda(), aux_shift=shift, mean=d["mean"].cuda(), std=d["std"].cuda(), out_padded=True, out_mode=mode)
        inner = y[:, 1:-1, 1:-1].contiguous()
        if mode == 0:
            return inner.cpu().numpy()
        if mode == 1:
            hi, lo = unsplit(inner)
            return hi.cpu().numpy(), lo.cpu().numpy()
        return inner[..., :C].contiguous().view(torch.float8_e5m2).float().cpu().numpy()
    key, plants = _spade_plant_sets(B, r, C, shift)[where]
    case = f"fp8 SPADE out_mode {mode} NaN in {where}"
    nan_t, clean_t = _planted(d[key], plants)
    refv = ref(dict(d, **{key: nan_t})).numpy()
    fin = np.isfinite(refv)
    out, clean = run(dict(d, **{key: nan_t})), run(dict(d, **{key: clean_t}))
    if mode == 0:
        rec = check_nan_contract(out, refv, clean, 5e-5, rel_linf, what=case)
    elif mode == 1:
        rec = check_nan_contract(out[0], refv, clean[0], 5e-5, lambda o, rf: rel_linf(np.where(fin, out[0].astype(np.float64) + out[1], 0.0), rf),
                                 what=case, raw=(out[1], clean[1], fin))
    else:
        want = torch.from_numpy(np.where(fin, refv, 0.0)).float().to(torch.float8_e5m2).float().numpy()
        step = np.maximum(np.abs(want) * 0.25, 2.0 ** -16) * 1.001
        rec = check_nan_contract(out, refv, clean, step, lambda o, rf: np.abs(o - want), what=case)
    _record(case, len(plants), rec)


# ---- conv_gb_resident ------------------------------------------------------------------------------------------------------------
_GBR_REF = {}


def _gbr_inputs(B, S, r, C, shift):
    g = torch.Generator(device="cpu").manual_seed(1000 * B + r + C + 7)
    src = torch.rand((B, S, S, 2), generator=g) - 0.5
    we, be = torch.randn((3, 3, 2, 128), generator=g) / 3, 0.1 * torch.randn(128, generator=g)
    wg, wb = torch.randn((3, 3, 128, C), generator=g) / 34, torch.randn((3, 3, 128, C), generator=g) / 34
    bg, bb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    x = 3 + 2 * torch.randn((B, r >> shift, r >> shift, C), generator=g)
    return dict(src=src, we=we, be=be, wg=wg, wb=wb, bg=bg, bb=bb, x=x, mean=x.mean((0, 1, 2)).contiguous(),
                std=torch.sqrt(x.var((0, 1, 2), unbiased=False) + 1e-5).contiguous())


def _gbr_ref(d, r, shift, half, key):
    """The float64 chain of test_spade_layer_resident_kernel; ``half``: embedding and gamma|beta weights rounded to fp16 (the
    chain test_spade_layer_resident_kernel_f16 holds the no-cross form to).  The two convs are computed once per ``key`` (shape
    and src plants) and shared by the cases that plant in x, mean or std."""
    if key not in _GBR_REF:
        f = d["src"].shape[1] // r
        torch.set_num_threads(16)
        e = torch.relu(ref_conv(d["src"][:, f // 2::f, f // 2::f][:, :r, :r], d["we"], d["be"], 1))
        wg, wb = (d["wg"].half().float(), d["wb"].half().float()) if half else (d["wg"], d["wb"])
        e = e.half().double() if half else e
        _GBR_REF[key] = (ref_conv(e, wg, d["bg"], 1), ref_conv(e, wb, d["bb"], 1))
    return _spade_of(*_GBR_REF[key], d, shift)


GBR_SHAPES = [pytest.param(2, 256, 64, 128, 0, id="2-256-64-128-s0"), pytest.param(8, 64, 64, 64, 1, id="8-64-64-64-s1")]
GBR_ENTRIES = [pytest.param(False, 4, id="spade_gbr"), pytest.param(True, 4, id="no_cross"), pytest.param(False, 5, id="f16c6-out")]


GBR_CASES = [pytest.param(*s.values, w, id=f"{s.id}-{w}") for s in GBR_SHAPES
             for w in ("lattice-corner", "lattice", "off-lattice", "x", "mean", "std") if not (w == "off-lattice" and s.values[1] == s.values[2])]


@pytest.mark.parametrize("nox,mode", GBR_ENTRIES)
@pytest.mark.parametrize("B,S,r,C,shift,where", GBR_CASES)
def test_gbr(ctx, B, S, r, C, shift, nox, mode, where):
    """conv_gb_resident through its three entries.  A NaN src pixel ON the nearest-resize lattice (source index t * f + f / 2)
    reaches the footprint of the two 3 x 3 convs (5 x 5 pixels, every channel) and only that; OFF the lattice it is never read:
    the output is bit-identical to the clean launch (at S = r every pixel is on the lattice: no such case there).  The corner case pins the embedding's zero padding: halo pixel x = -1 sees the NaN in its window and must stay
    exactly 0 (top = 0 of the phase-1 clamp), or the NaN would reach column 1's neighbours through the halo - the 5 x 5
    footprint clipped at the corner is 3 x 3.  Bounds: 2e-4 on hi + lo8 against the float64 chain (test_spade_layer_resident_kernel;
    f16c6 output: the same on hi + l6); no_cross: 1e-4 against the fp16-rounded chain (test_spade_layer_resident_kernel_f16)."""
    from moonsuperresolution_amd import ops
    f = S // r
    d = _gbr_inputs(B, S, r, C, shift)
    w, bias = ops.spade_layout(d["wg"].cuda(), d["wb"].cuda(), d["bg"].cuda(), d["bb"].cuda())
    wimg = ops.gbr_weight_image(w)
    lat = lambda t: t * f + f // 2                                                 # noqa: E731
    if where == "off-lattice":
        plants = [(0, lat(0) - 1, lat(0), 0), (0, lat(20), lat(20) + 1, 1), (B - 1, lat(r - 1) + 1, lat(r - 1) - 1, 0)]
        key = "src"
    elif where == "lattice-corner":
        key, plants = "src", [(0, lat(0), lat(0), 0)]
    elif where == "lattice":
        key, plants = "src", [(0, lat(r - 1), lat(r - 1), 1), (0, lat(5), lat(15), 0), (0, lat(r - 8), lat(16), 1),
                              (B - 1, lat(r // 2), lat(r // 2 + 3), 0)]
    else:
        key, plants = {"x": ("x", _plants(B, r >> shift, C)), "mean": ("mean", [(0,)]), "std": ("std", [(C - 1,)])}[where]
    nan_t, clean_t = _planted(d[key], plants)
    src_kind = where if where.startswith("lattice") else "clean"
    refv = _gbr_ref(dict(d, **{key: nan_t if where != "off-lattice" else d[key]}), r, shift, nox, (B, S, r, C, shift, nox, src_kind)).numpy()

    def run(d):
        y = ops.spade_gbr(ctx, d["src"].cuda(), d["we"].cuda(), d["be"].cuda(), wimg, bias, r, d["x"].cuda(), shift, d["mean"].cuda(),
                          d["std"].cuda(), no_cross=nox, out_mode=mode)
        border = y.clone()
        border[:, 1:-1, 1:-1] = 0
        assert int(border.view(torch.int32).abs().max()) == 0
        inner = y[:, 1:-1, 1:-1].contiguous()
        if mode == 4:
            hi, _, lo = ops.f16c_decode(inner)
            return hi.cpu().numpy(), lo.cpu().numpy(), inner.view(torch.uint8).cpu().numpy()
        hi, h6, l6 = ops.f16c6_decode(inner)
        return hi.cpu().numpy(), l6.cpu().numpy(), torch.stack([h6, l6]).cpu().numpy(), inner.view(torch.uint8).cpu().numpy()
    out, clean = run(dict(d, **{key: nan_t})), run(dict(d, **{key: clean_t}))
    case = f"conv_gb_resident ({B}, {S}, {r}, {C}, shift {shift}) {'no_cross' if nox else 'out_mode %d' % mode} NaN {where}"
    if where == "off-lattice":
        assert np.array_equal(out[2], clean[2]), f"{case}: a source pixel off the resize lattice changed the output"
        assert np.array_equal(out[2], run(d)[2])
        _record(case, len(plants), dict(n_nan_ref=0, n_total=int(refv.size), worst=0.0, bound=0.0))
        return
    fin = np.isfinite(refv)
    if where == "lattice-corner":
        nan_px = ~fin.all(-1)
        assert int(nan_px.sum()) == 9 and nan_px[0, :3, :3].all()
    keep = _f16c_raw_keep(fin, out[2]) if mode == 4 else _f16c6_keep(fin, clean[0], out[2].shape)
    rec = check_nan_contract(out[0], refv, clean[0], 1e-4 if nox else 2e-4,
                             lambda o, rf: rel_linf(np.where(fin, out[0] + out[1], 0.0), rf), what=case, raw=(out[2], clean[2], keep))
    if mode == 5:
        _f16c6_scale_bytes_unchanged(case, fin, clean[0], out[3], clean[3])
    _record(case, len(plants), rec)


# ---- small kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("index_map,B,S,hout,cout,kernel", [(0, 1, 256, 128, 64, "tiled"), (1, 1, 256, 128, 128, "tiled"),
                                                            (0, 3, 64, 32, 64, "px4"), (1, 2, 64, 16, 128, "px4"), (1, 2, 48, 3, 64, "px1")])
def test_conv_smallcin(ctx, index_map, B, S, hout, cout, kernel, act):
    """conv_smallcin in its three kernels and five output formats, NaN in either source channel (relu(NaN) = NaN: act 1 is the
    mask embedding's and lost it).  Format 0: |y - ref| <= 20 * 2^-24 * (sum |w| |x| + |bias|) (tests/test_gpu_small_kernels.py::
    test_conv_smallcin); formats 1 - 4: NaN main piece, every other element's bytes those of the clean launch."""
    from moonsuperresolution_amd import ops
    g = torch.Generator(device="cpu").manual_seed(77 + index_map + hout)
    src = torch.rand((B, S, S, 2), generator=g) - 0.5
    w, b = torch.randn((3, 3, 2, cout), generator=g) / 3, 0.1 * torch.randn(cout, generator=g)
    slope = float(np.float32(0.2)) if act == 2 else 0.0
    f = S // hout if index_map == 1 else 1
    o = f // 2 if index_map == 1 else 0
    # source pixels that the kernel reads: the resize lattice (map 1), every pixel (map 0)
    pos = [(0, o, o), (0, (hout - 1) * f + o if index_map else S - 1, (hout - 1) * f + o if index_map else S - 1),
           (B - 1, (hout // 2) * f + o, (hout // 2) * f + o)]
    if hout >= 32:
        pos += [(0, 3 * f + o, 15 * f + o if index_map else 31), (0, (hout - 4) * f + o, 16 * f + o if index_map else 32)]
    plants = [p + (i % 2,) for i, p in enumerate(pos)]
    nan_t, clean_t = _planted(src, plants)
    ref = smallcin_ref(nan_t, w, b, hout, index_map, act, slope).numpy()
    mag = smallcin_ref(clean_t.abs(), w.abs(), b.abs(), hout, index_map).numpy()
    run = lambda s, fmt: ops.conv_smallcin(ctx, s.cuda(), w.cuda(), b.cuda(), hout, index_map, act, slope, out_split=fmt).cpu()    # noqa: E731
    case = f"conv_smallcin map {index_map} ({kernel}) Hout={hout} Cout={cout} act {act}"
    exempt = "Hout = 3: every output sees a plant" if hout == 3 else None
    rec = check_nan_contract(run(nan_t, 0).numpy(), ref, run(clean_t, 0).numpy(), 20 * U * mag, lambda o_, rf: np.abs(o_ - rf), what=case,
                             exempt=exempt)
    _record(case, len(plants), rec)
    fin = np.isfinite(ref)
    for fmt in (1, 2, 3, 4):
        yn, yc = run(nan_t, fmt), run(clean_t, fmt)
        if fmt in (1, 2):
            dt = torch.bfloat16 if fmt == 1 else torch.float16
            un, uc = (t.contiguous().view(torch.int16).reshape(-1, 2, 32) for t in (yn, yc))
            hi = un[:, 0].contiguous().view(dt).float().reshape(ref.shape).numpy()
            k2 = np.broadcast_to(fin.reshape(-1, 1, 32), un.shape)
            assert np.array_equal(np.isnan(hi), ~fin), f"{case} format {fmt}: NaN mask of the main piece"
            assert np.array_equal(un.numpy()[k2], uc.numpy()[k2]), f"{case} format {fmt}: another element's bits changed"
        elif fmt == 3:
            bn, bc = (t.contiguous().view(torch.uint8).reshape(ref.shape[:3] + (-1,))[..., :cout] for t in (yn, yc))
            assert np.array_equal(np.isnan(bn.contiguous().view(torch.float8_e5m2).float().numpy()), ~fin), f"{case} bf8: NaN mask"
            assert np.array_equal(bn.numpy()[fin], bc.numpy()[fin]), f"{case} bf8: another element's byte changed"
        else:
            rn, rc = (t.contiguous().view(torch.uint8).numpy() for t in (yn, yc))
            assert np.array_equal(np.isnan(ops.f16c_decode(yn)[0].numpy()), ~fin), f"{case} f16c: NaN mask of hi"
            k4 = _f16c_raw_keep(fin, rn)
            assert np.array_equal(rn[k4], rc[k4]), f"{case} f16c: another element's bytes changed"


_UNTILED_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import pytest
sys.exit(pytest.main([sys.argv[2], "-q", "-x", "-m", "gpu", "-k", "test_conv_smallcin and tiled and not untiled"]))
"""


def test_conv_smallcin_untiled_kernel_at_the_tiled_shapes():
    """MSR_SMALLCIN_TILED=0 (read once per process): the untiled kernel at the shapes the tiled one takes by default."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _UNTILED_CHILD, root, os.path.abspath(__file__)], env=dict(os.environ, MSR_SMALLCIN_TILED="0"),
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("G,P,C", [(1, 3 * 65, 64), (3, 65, 64), (3, 4101, 32)])
def test_moments(ctx, G, P, C):
    """moments with G = 1 (batch statistics) and G = B (instance statistics): exactly the planted (group, channel) statistics are
    NaN - the chunk's pivot (a lane's first value) may be the NaN itself - and all others are bit-identical; finite ones
    within MEAN_BOUND / STD_BOUND of tests/test_gpu_moments.py."""
    from moonsuperresolution_amd import ops
    from tests.test_gpu_moments import MEAN_BOUND, STD_BOUND, make_input, reference
    x = make_input(G, P, C, seed=5 + G + P).cpu()
    plants = [(0, 0, 0), (G - 1, P - 1, C - 1), (G // 2, P // 2, 37 % C)]       # a chunk's first value, the last value, the middle
    nan_t, clean_t = _planted(x, plants)
    m_ref, s_ref, xmax = reference(nan_t, 1e-5)
    xmax = clean_t.abs().amax(1).double()
    (mn, sn), (mc, sc) = ops.moments(ctx, nan_t.cuda(), 1e-5), ops.moments(ctx, clean_t.cuda(), 1e-5)
    case = f"moments G={G} P={P} C={C}"
    rec = check_nan_contract(mn.cpu().numpy(), m_ref.numpy(), mc.cpu().numpy(), (MEAN_BOUND * xmax).numpy(), lambda o, rf: np.abs(o - rf),
                             what=case + " mean")
    assert rec["n_nan_ref"] == len(set((p[0], p[2]) for p in plants))
    _record(case + " mean", len(plants), rec)
    sr = s_ref.double().numpy()
    rec = check_nan_contract(sn.cpu().numpy(), sr, sc.cpu().numpy(), STD_BOUND,
                             lambda o, rf: np.abs(o - rf) / np.where(rf > 0, rf, 1.0), what=case + " std")
    _record(case + " std", len(plants), rec)


@pytest.mark.parametrize("out_split", [False, True])
@pytest.mark.parametrize("where", ["x", "mean", "std"])
def test_norm_act(ctx, where, out_split):
    """norm_act, dense and split-bf16 output; bound 4 * 2^-24 * (|(x - m) / s * gamma| + |beta|) (test_norm_act)."""
    from moonsuperresolution_amd import ops
    B, H, C = 3, 16, 128
    g = torch.Generator(device="cpu").manual_seed(21)
    x = (5 + 3 * torch.randn((B, H, H, C), generator=g)) * torch.logspace(-1, 1, C)
    d = dict(x=x, mean=x.mean((1, 2)) + 0.1 * torch.randn((B, C), generator=g), std=x.std((1, 2)) * (1 + 0.1 * torch.rand((B, C), generator=g)))
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    slope = float(np.float32(0.2))

    def terms(d):
        a = (d["x"].double() - d["mean"].double()[:, None, None]) / d["std"].double()[:, None, None] * gamma.double()
        return a, a + beta.double()

    def ref(d):
        v = terms(d)[1]
        return torch.where(v >= 0, v, slope * v)

    def run(d):
        y = ops.norm_act(ctx, d["x"].cuda(), d["mean"].cuda(), d["std"].cuda(), gamma.cuda(), beta.cuda(), slope=slope, out_padded=True,
                         out_split=out_split).cpu()
        border = y.clone()
        border[:, 1:-1, 1:-1] = 0
        assert int(border.view(torch.int32).abs().max()) == 0
        y = y[:, 1:-1, 1:-1].contiguous()
        if not out_split:
            return y.numpy()
        hi, lo = unsplit(y)
        return hi.numpy(), lo.numpy()
    key, plants = {"x": ("x", _plants(B, H, C)), "mean": ("mean", [(0, 0), (B - 1, 37)]), "std": ("std", [(1, C - 1)])}[where]
    nan_t, clean_t = _planted(d[key], plants)
    refv = ref(dict(d, **{key: nan_t})).numpy()
    fin = np.isfinite(refv)
    a = terms(dict(d, **{key: clean_t}))[0]
    bound = np.where(fin, 4 * U * (a.abs() + beta.double().abs()).numpy(), 0.0)
    out, clean = run(dict(d, **{key: nan_t})), run(dict(d, **{key: clean_t}))
    case = f"norm_act out_split={int(out_split)} NaN in {where}"
    if out_split:
        # hi + lo keeps 16 bits of the fp32 value (test_split_bf16_words: 2^-16), on top of the fp32 bound
        rec = check_nan_contract(out[0], refv, clean[0], bound + 2.0 ** -16 * np.abs(np.where(fin, refv, 0.0)),
                                 lambda o, rf: np.abs(np.where(fin, out[0].astype(np.float64) + out[1], 0.0) - rf), what=case,
                                 raw=(out[1], clean[1], fin))
    else:
        rec = check_nan_contract(out, refv, clean, bound, lambda o, rf: np.abs(o - rf), what=case)
    _record(case, len(plants), rec)


def test_latent_dense_split(ctx):
    """latent (both samplers: NaN in mean, variance, eps), dense (the planted row is all NaN, the other rows bit-identical) and
    split_bf16; bounds of tests/test_gpu_small_kernels.py::test_latent / test_dense, tests/test_gpu_conv_kernel.py::
    test_split_bf16_words."""
    from moonsuperresolution_amd import ops
    from tests.helpers import dense_kch
    g = torch.Generator(device="cpu").manual_seed(31)
    B, L = 3, 256
    mv = torch.cat([torch.randn((B, L), generator=g), 8 * torch.rand((B, L), generator=g) - 4], 1)
    eps = torch.randn((B, L), generator=g)
    mvn, mvc = _planted(mv, [(0, 0), (1, L + 37), (B - 1, 2 * L - 1)])
    en, ec = _planted(eps, [(2, 5)])
    z0n, z0c = ops.latent(ctx, mvn.cuda(), None, 0).cpu().numpy(), ops.latent(ctx, mvc.cuda(), None, 0).cpu().numpy()
    rec = check_nan_contract(z0n, (mvn[:, :L].double() + mvn[:, L:].double()).numpy(), z0c, 0.0,
                             lambda o, rf: np.abs(o - rf.astype(np.float32)), what="latent sampler 0")
    _record("latent sampler 0", 3, rec)
    m, v, e = mvn[:, :L].double(), mvn[:, L:].double(), en.double()
    t = torch.exp(v / 2) * e
    tc = torch.exp(mvc[:, L:].double() / 2) * ec.double()
    z1n, z1c = ops.latent(ctx, mvn.cuda(), en.cuda(), 1).cpu().numpy(), ops.latent(ctx, mvc.cuda(), ec.cuda(), 1).cpu().numpy()
    rec = check_nan_contract(z1n, (m + t).numpy(), z1c, (4 * U * (mvc[:, :L].double().abs() + tc.abs())).numpy(), lambda o, rf: np.abs(o - rf),
                             what="latent sampler 1")
    assert rec["n_nan_ref"] == 4
    _record("latent sampler 1", 4, rec)
    # dense: (5, 1000, 516) ragged K chunks, N % 512 != 0
    Bd, K, N = 5, 1000, 516
    x, w, b = torch.randn((Bd, K), generator=g), torch.randn((K, N), generator=g) / np.sqrt(K), torch.randn(N, generator=g)
    xn, xc = _planted(x, [(1, 0), (Bd - 1, K - 1)])
    yn, yc = ops.dense(ctx, xn.cuda(), w.cuda(), b.cuda()).cpu().numpy(), ops.dense(ctx, xc.cuda(), w.cuda(), b.cuda()).cpu().numpy()
    kch = dense_kch(K, N)
    bound = (kch + (K + kch - 1) // kch + 1) * U * (xc.double().abs() @ w.double().abs() + b.double().abs())
    rec = check_nan_contract(yn, (xn.double() @ w.double() + b.double()).numpy(), yc, bound.numpy(), lambda o, rf: np.abs(o - rf), what="dense")
    assert rec["n_nan_ref"] == 2 * N
    _record("dense", 2, rec)
    # split_bf16: hi NaN at the plants, hi and lo of every other element unchanged
    s = torch.randn(4096, generator=g) * torch.logspace(-6, 6, 4096)
    sn, sc = _planted(s, [(0,), (37,), (4095,)])
    (hn, ln), (hc, lc) = unsplit(ops.split_bf16(ctx, sn.cuda())), unsplit(ops.split_bf16(ctx, sc.cuda()))
    rec = check_nan_contract(hn.cpu().numpy(), sn.double().numpy(), hc.cpu().numpy(), 0.0,
                             lambda o, rf: np.abs(o - torch.from_numpy(rf).float().to(torch.bfloat16).float().numpy()), what="split_bf16",
                             raw=(ln.cpu().numpy(), lc.cpu().numpy(), np.isfinite(sn.numpy())))
    _record("split_bf16", 3, rec)


@pytest.mark.parametrize("transpose_tanh", [False, True])
def test_head(ctx, transpose_tanh):
    """Both head variants at (2, 16, 32); bound 1e-5 (tests/test_gpu_conv_kernel.py::test_head_kernel_known_answers)."""
    import torch.nn.functional as F
    from moonsuperresolution_amd import ops
    B, r, C = 2, 16, 32
    g = torch.Generator(device="cpu").manual_seed(41)
    k, x = torch.randn((4, 4, C), generator=g), torch.randn((B, r, r, C), generator=g)

    def ref(d):
        xin = d["x"].double()
        if transpose_tanh:
            full = F.conv_transpose2d(xin.permute(0, 3, 1, 2), k.double().permute(2, 0, 1)[:, None], stride=2)
            return torch.tanh(full[:, 0, 1:-1, 1:-1] + 0.05)
        a = torch.where(xin >= 0, xin, 0.2 * xin).permute(0, 3, 1, 2)
        up = a.repeat_interleave(2, 2).repeat_interleave(2, 3)
        return F.conv2d(F.pad(up, (1, 2, 1, 2)), k.double().permute(2, 0, 1)[None]).squeeze(1) - 0.1
    run = lambda d: ops.head(ctx, d["x"].cuda(), k.numpy(), 0.05 if transpose_tanh else -0.1, slope=1.0 if transpose_tanh else 0.2,     # noqa: E731
                             transpose_tanh=transpose_tanh).cpu().numpy()
    _check(f"head transpose_tanh={int(transpose_tanh)}", run, ref, dict(x=x), "x", _plants(B, r, C), 1e-5)


def test_fused_head(ctx):
    """conv3x3_f16c_head at (3, 32, 256, shift 1): NaN in the conv's activation reaches the 3 x 3 conv footprint and through the
    head's up-sample + 4 x 4 taps its neighbours; NaN in the residual one pixel block.  Reference and bound of
    tests/test_gpu_fused_head.py::test_fused_head_kernel_against_fp64 (own three terms in float64 + residual, leaky relu, the
    oracle's head): over the finite elements the fused chain may not be further from the reference than the separate chain
    (msr_op_conv3x3_f16c -> msr_op_head on the same NaN-holding operands) by more than 1e-5."""
    from moonsuperresolution_amd import ops
    from oracle import generator_ref as G
    B, r, cin, shift = 3, 32, 256, 1
    d = _conv_inputs(B, r, cin, 128, res=shift, seed=8)
    k = (torch.randn((4, 4, 128), generator=torch.Generator().manual_seed(9)) / np.sqrt(16 * 128)).numpy()
    wimg, wexp, wparts = ops.f16c_weight_image(ops.kernel_layout(d["w"].cuda()))
    k64 = torch.from_numpy(k).double()

    def ref(d):
        xparts = ops.f16c_activation_image(ops.pad_nhwc(d["x"].cuda()))[1]
        v = _ref_f16c(tuple(t[:, 1:-1, 1:-1].cpu() for t in xparts), tuple(t.cpu() for t in wparts), d["b"], cin, 128) + _up(d["skip"].double(), shift)
        return G.conv2d_same(G.leaky_relu(G.upsample2x(v), G.LEAK), k64[..., None], torch.tensor([0.25], dtype=torch.float64))[..., 0]
    run = lambda d: ops.conv3x3_f16c_head(ctx, ops.f16c_activation_image(ops.pad_nhwc(d["x"].cuda()))[0], wimg, wexp, d["b"].cuda(), r,     # noqa: E731
                                          d["skip"].cuda(), shift, k, 0.25).cpu().numpy()

    def separate(d):
        y = ops.conv3x3_f16c(ctx, ops.f16c_activation_image(ops.pad_nhwc(d["x"].cuda()))[0], wimg, wexp, d["b"].cuda(), r, epilogue=ops.EPI_RES,
                             aux=d["skip"].cuda(), aux_shift=shift)
        return ops.head(ctx, y, k, 0.25).cpu().numpy()
    for case, key, plants in (("fused head NaN in the activation", "x", _plants(B, r, cin)),
                              ("fused head NaN in the residual", "skip", _plants(B, r >> shift, 128))):
        nan_t, clean_t = _planted(d[key], plants)
        dn = dict(d, **{key: nan_t})
        refv = ref(dn).numpy()
        fin = np.isfinite(refv)
        sep = np.where(fin, separate(dn).astype(np.float64), 0.0)
        rec = check_nan_contract(run(dn), refv, run(dict(d, **{key: clean_t})), 1e-5,
                                 lambda o, rf: rel_linf(o, rf) - rel_linf(sep, rf), what=case)
        _record(case, len(plants), rec)


# ---- network level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [None, "fp32"])
@pytest.mark.parametrize("variant", ["gaugan", "gaugan_no_kl", "cnn"])
def test_generator_nan_sample(hip_lib, variant, precision):
    """S = 64, B = 4 (the default precision selects the bf16x3 kernels at this size).  (a) sample 1's ortho channel all NaN:
    isnan(y) equals the oracle's mask (every sample, through the batch moments).  (b) gaugan_no_kl, one NaN pixel at (0, 0) and one
    at (1, 1): the oracle's mask decides."""
    from moonsuperresolution_amd import Generator, make_latent_noise, make_weights, synthetic_patches
    from oracle import generator_ref
    S, B = 64, 4
    w = make_weights(variant, S, seed=1234)
    eps = make_latent_noise(B, 256, seed=7) if variant == "gaugan" else None
    kw = {} if precision is None else dict(precision=precision)
    gen = Generator(S, B, variant=variant, weights=w, eps=eps, **kw)
    x = synthetic_patches(B, S, seed=0)
    cases = [("ortho channel of sample 1", (1, slice(None), slice(None), 0))]
    if variant == "gaugan_no_kl":
        cases += [("pixel (0, 0) of sample 0", (0, 0, 0, 0)), ("pixel (1, 1) of sample 2", (2, 1, 1, 0))]
    for name, at in cases:
        xn, xc = x.copy(), x.copy()
        xn[at], xc[at] = np.nan, 0.0
        ref = generator_ref.spade_call(xn, w, variant, eps, dtype=torch.float32)
        y = gen(xn, training=False)
        lost, extra = np.isnan(ref) & ~np.isnan(y), np.isnan(y) & ~np.isnan(ref)
        assert not lost.any() and not extra.any(), (variant, precision, name, int(lost.sum()), int(extra.sum()),
                                                    np.argwhere(lost | extra)[0].tolist())
        fin = np.isfinite(ref)
        if fin.any():
            yc = gen(xc, training=False)
            assert np.array_equal(y[fin].view(np.uint32), yc[fin].view(np.uint32)), (variant, precision, name)
        _record(f"generator {variant} {precision or 'default'} S=64 B=4 NaN {name}", int(np.isnan(xn).sum()),
                dict(n_nan_ref=int(np.isnan(ref).sum()), n_total=int(ref.size), worst=0.0, bound=0.0))


def test_pix2pix_nan_pixel(hip_lib):
    """pix2pix at (256, 2), one NaN pixel in sample 0 (every layer on the fp32 MFMA; the up path's ReLU is EPI_AFFINE's, which was
    fmaxf in conv_epilogue.h, conv_splitk.hip and conv_direct.hip).  Sample 0 is NaN wherever the oracle says (everywhere, through
    the 1 x 1 bottleneck); sample 1 (inference BatchNorm: nothing crosses samples) is bit-identical to the clean run."""
    from moonsuperresolution_amd import Generator, make_weights, synthetic_patches
    from oracle import generator_ref
    w = make_weights("pix2pix", 256, seed=1234, bias_scale=0.05)
    gen = Generator(256, 2, variant="pix2pix", weights=w)
    affine = sorted({(op["kernel"], op["ksplit"]) for op in gen.conv_forms() if op["kind"] == "conv" and op.get("epi") == 4})
    print("pix2pix (256, 2): (kernel, ksplit) of the EPI_AFFINE convs of the plan:", affine)
    x = synthetic_patches(2, 256, seed=3)
    xn, xc = x.copy(), x.copy()
    xn[0, 100, 37, 0], xc[0, 100, 37, 0] = np.nan, 0.0
    torch.set_num_threads(16)
    ref = generator_ref.pix2pix_call(xn, w, dtype=torch.float32)
    assert np.isnan(ref[0]).all() and np.isfinite(ref[1]).all()
    y, yc = gen(xn, training=False), gen(xc, training=False)
    lost, extra = np.isnan(ref) & ~np.isnan(y), np.isnan(y) & ~np.isnan(ref)
    assert not lost.any() and not extra.any(), (int(lost.sum()), int(extra.sum()), np.argwhere(lost | extra)[0].tolist())
    assert np.array_equal(y[1].view(np.uint32), yc[1].view(np.uint32))
    _record("generator pix2pix S=256 B=2 NaN pixel in sample 0", 1, dict(n_nan_ref=int(np.isnan(ref).sum()), n_total=int(ref.size), worst=0.0, bound=0.0))


# the smallest shape whose f16c / f16 plan holds a resident-kernel op AND a stream-kernel conv (csrc/forms.hip conv_gbr_ranges and
# conv_kernel_for, read through the form table: tests/test_nonfinite_host.py::test_smallest_shape_with_resident_and_stream_kernels;
# (256, 8) has both as well, with 3.6 times the pixels).  The test asserts both on the planned network.
LARGE_S, LARGE_B = 128, 9
_LARGE_REF = {}


@pytest.mark.parametrize("precision", ["f16c", "f16", "fp8"])
def test_generator_large_kernels_nan_sample(hip_lib, precision):
    """gaugan_no_kl at (128, 9): sample 1's ortho channel all NaN, through conv_gb_resident, the stream kernel, the K-range and
    split-K launches and the range scan together.  isnan(y) equals the oracle's mask (fp32 oracle: only the mask is needed), and
    range_report() of that call reports non-finite elements and a regime other than "parity"."""
    from moonsuperresolution_amd import Generator, make_weights, synthetic_patches
    from oracle import generator_ref
    S, B = LARGE_S, LARGE_B
    w = make_weights("gaugan_no_kl", S, seed=1234)
    gen = Generator(S, B, variant="gaugan_no_kl", weights=w, precision=precision)
    forms = gen.conv_forms()
    kernels = sorted({op["kernel"] for op in forms if op["kind"] in ("conv", "gbr")})
    print(f"{precision} ({S}, {B}): kernels of the plan {kernels}")
    if precision != "fp8":          # the fp8 mode's chip-filling convs run the ping-pong kernel's fp8 form
        assert "gbr" in kernels and "sw" in kernels, kernels
    x = synthetic_patches(B, S, seed=0)
    x[1, :, :, 0] = np.nan
    if "ref" not in _LARGE_REF:
        torch.set_num_threads(16)
        _LARGE_REF["ref"] = generator_ref.spade_call(x, w, "gaugan_no_kl", None, dtype=torch.float32)
    ref = _LARGE_REF["ref"]
    assert np.isnan(ref).all()                                       # the batch moments hand the NaN to every sample
    y = gen(x, training=False)
    lost, extra = np.isnan(ref) & ~np.isnan(y), np.isnan(y) & ~np.isnan(ref)
    assert not lost.any() and not extra.any(), (precision, int(lost.sum()), int(extra.sum()), np.argwhere(lost | extra)[0].tolist())
    rep = gen.range_report()
    print(f"{precision}: {rep}")
    assert sum(r["n_nonfinite"] for r in rep.records) > 0 and rep.regime != "parity", str(rep)
    _record(f"generator gaugan_no_kl {precision} S={S} B={B} NaN ortho channel of sample 1", int(np.isnan(x).sum()),
            dict(n_nan_ref=int(np.isnan(ref).sum()), n_total=int(ref.size), worst=0.0, bound=0.0))
    gen.close()


@pytest.mark.parametrize("pixel,holed", [((70, 41), True), ((100, 100), False)])
def test_tiler_nan_pixel(hip_lib, pixel, holed):
    """DEMSuperResolution.processMap over Generator(64, 4, "gaugan_no_kl") on a 120 x 120 raster (S = 64, s = 32, T = 128) with
    one NaN ortho pixel, against tiler_ref.process_map over the oracle generator: `good` equal, isnan(mean) and isnan(std)
    equal, the finite part within the 1e-3 x span of tests/test_gpu_tiler.py::test_generator_through_tiler_vs_oracle.  Pixel
    (70, 41) lies in patches of every batch: the batch moments make every generated patch NaN and the stitched map is a hole
    wherever it is good; pixel (100, 100) lies in no valid patch: nothing is NaN and the whole map is the finite part."""
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, Generator, make_weights
    from oracle import generator_ref, tiler_ref
    from tests.helpers import synthetic_raster
    w = make_weights("gaugan_no_kl", 64, seed=1234, bias_scale=0.05)
    img, dem = synthetic_raster(120, 120, 9)
    img[pixel] = np.nan
    gen = Generator(64, 4, variant="gaugan_no_kl", weights=w)
    d = DEMSuperResolution(DSRConfig(image_size=64, stride=32, batch_size=4, tile_size=128), model=gen)
    mean, std, good = d.processMap(img, dem)
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    rm, rs, rg = tiler_ref.process_map(img, dem, lambda x, training=False: generator_ref.spade_call(x, wt, "gaugan_no_kl", dtype=torch.float32),
                                       64, 32, 4, 128, -32768.0)
    assert np.array_equal(good, rg) and good.any()
    assert np.array_equal(np.isnan(mean), np.isnan(rm)) and np.array_equal(np.isnan(std), np.isnan(rs))
    ok = (good == 1) & ~np.isnan(rm)
    assert bool(np.isnan(rm[good == 1]).all()) == holed and bool(ok.any()) == (not holed)
    worst = 0.0
    if ok.any():
        span = float(dem.max() - dem.min())
        worst = float(max(np.abs(mean[ok] - rm[ok]).max(), np.abs(std[ok] - rs[ok]).max()) / span)
        assert worst <= 1e-3, worst
    _record(f"tiler 120 x 120, NaN ortho pixel {pixel}", 1, dict(n_nan_ref=int(np.isnan(rm).sum()), n_total=int(rm.size), worst=worst, bound=1e-3))
    d.close()
    gen.close()

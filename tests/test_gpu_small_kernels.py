"""GPU (-m gpu): kernel-level checks of the small kernels (csrc/small_kernels.hip) against float64 CPU references: the mask
embedding / encoder conv (conv_smallcin) in its three kernels and five output formats, norm_act, the dense layers
(dense_partial + both final passes) and the latent sampler.  Every bound is an a-priori rounding bound of the kernel's own
fp32 arithmetic, stated per element; every test prints the largest fraction of its bound it used."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import dense_kch as _dense_kch, smallcin_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # fp32 unit roundoff


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert torch.cuda.is_available()
    from moonsuperresolution_amd import ops
    c = ops.OpContext()
    yield c
    c.close()


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu()


def _split_bf16_host(y):
    """fp32 [..., C] -> split-bf16 chunk image (hi = bf16_rn(v), lo = bf16_rn(v - hi), [32 hi | 32 lo] per chunk)."""
    hi = y.to(torch.bfloat16)
    lo = (y - hi.float()).to(torch.bfloat16)
    hl = torch.stack([hi.reshape(-1, 32), lo.reshape(-1, 32)], 1).contiguous()
    return hl.view(torch.int16).reshape(-1).view(torch.float32).reshape(y.shape)


# (index map, B, S, Hout, Cout, act, bias, kernel the launcher picks)
SMALLCIN_CASES = [
    (0, 1, 256, 128, 64, 2, False, "tiled"),       # encoder ds1 (stride-2 SAME, no bias, leaky 0.2) at S = 256, B = 1
    (0, 3, 256, 128, 128, 1, True, "tiled"),
    (0, 3, 64, 32, 64, 2, False, "px4"),           # S = 64: 12 tiles, one pixel group per thread
    (0, 2, 16, 8, 128, 0, True, "px4"),
    (0, 5, 12, 6, 64, 2, False, "px1"),            # Hout % 4 != 0
    (0, 3, 4, 2, 128, 1, True, "px1"),
    (1, 1, 256, 128, 128, 1, True, "tiled"),       # mask embedding (nearest resize, SAME, relu), S / r = 2
    (1, 1, 1024, 128, 64, 2, True, "tiled"),       # S / r = 8
    (1, 3, 512, 64, 64, 1, True, "px4"),           # 48 tiles: below the tiled kernel's 64
    (1, 5, 256, 32, 128, 0, False, "px4"),         # S / r = 8, no bias
    (1, 3, 512, 8, 128, 1, True, "px4"),           # S / r = 64
    (1, 2, 64, 16, 64, 2, True, "px4"),
    (1, 3, 64, 1, 128, 1, True, "px1"),            # the S = 64 goldens' rb1 / rb2 embeddings: r = 1, 2
    (1, 1, 64, 2, 64, 0, True, "px1"),
    (1, 4, 128, 2, 128, 2, False, "px1"),
    (1, 2, 48, 3, 64, 1, True, "px1"),             # S / r = 16, odd Hout
]


def _smallcin_inputs(index_map, B, S, Cout, bias, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    src = (torch.rand((B, S, S, 2), generator=g) - 0.5).cuda()
    w = (torch.randn((3, 3, 2, Cout), generator=g) / 3).cuda()
    b = (0.1 * torch.randn(Cout, generator=g)).cuda() if bias else None
    return src, w, b


@pytest.mark.parametrize("index_map,B,S,hout,cout,act,bias,kernel", SMALLCIN_CASES)
def test_conv_smallcin(ctx, index_map, B, S, hout, cout, act, bias, kernel):
    """conv_smallcin (encoder block 1, SPADE mask embedding): 18 fp32 products + bias per output, no FMA contraction.
    Format 0 against the float64 conv of the strided / resized source, element by element:
        |y - ref| <= 20 * 2^-24 * (sum |w| |x| + |bias|)          (18 products and 18 additions, then the activation)
    Formats 1-4 of the same launch (split-bf16, split-fp16, bf8, f16c) are the host restatement of format 0's fp32 output,
    byte for byte; padded outputs equal the dense ones inside and stay zero on the border."""
    from moonsuperresolution_amd import ops
    slope = float(np.float32(0.2)) if act == 2 else 0.0
    src, w, b = _smallcin_inputs(index_map, B, S, cout, bias, 1000 * index_map + 10 * B + hout)
    y = ops.conv_smallcin(ctx, src, w, b, hout, index_map, act=act, slope=slope)
    ref = smallcin_ref(src, w, b, hout, index_map, act, slope)
    mag = smallcin_ref(src.abs(), w.abs(), b.abs() if b is not None else None, hout, index_map)
    err = (y.cpu().double() - ref).abs()
    bound = 20 * U * mag
    print(f"conv_smallcin map={index_map} B={B} S={S} Hout={hout} Cout={cout} act={act} ({kernel}): max |err| / bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    yc = y.cpu()
    assert torch.equal(_bytes(ops.conv_smallcin(ctx, src, w, b, hout, index_map, act, slope, out_split=1)), _bytes(_split_bf16_host(yc)))
    assert torch.equal(_bytes(ops.conv_smallcin(ctx, src, w, b, hout, index_map, act, slope, out_split=2)), _bytes(ops.split_f16(yc)))
    assert torch.equal(_bytes(ops.conv_smallcin(ctx, src, w, b, hout, index_map, act, slope, out_split=3)),
                       ops.bf8_activation_image(yc)[0].contiguous())
    assert torch.equal(_bytes(ops.conv_smallcin(ctx, src, w, b, hout, index_map, act, slope, out_split=4)),
                       _bytes(ops.f16c_activation_image(yc)[0]))
    for fmt in (0, 3, 4):
        yp = ops.conv_smallcin(ctx, src, w, b, hout, index_map, act, slope, out_split=fmt, out_padded=True).cpu()
        yd = ops.conv_smallcin(ctx, src, w, b, hout, index_map, act, slope, out_split=fmt).cpu()
        assert torch.equal(_bytes(yp[:, 1:-1, 1:-1]), _bytes(yd))
        border = yp.clone()
        border[:, 1:-1, 1:-1] = 0
        assert int(_bytes(border).max()) == 0


def test_conv_smallcin_rejects_bad_arguments(ctx):
    """The kernel reads any out_split outside 2, 3, 4 as split-bf16: the entry accepts only the formats 0-4, Cout 64 | 128
    and index maps whose source size matches."""
    from moonsuperresolution_amd import ops
    src, w, b = _smallcin_inputs(1, 1, 64, 64, True, 1)
    for kw in (dict(out_split=5), dict(out_split=-1), dict(act=3)):
        with pytest.raises(ValueError):
            ops.conv_smallcin(ctx, src, w, b, 16, 1, **kw)
    with pytest.raises(ValueError):
        ops.conv_smallcin(ctx, src, w, b, 16, 0)          # stride-2 map needs S = 2 Hout
    with pytest.raises(ValueError):
        ops.conv_smallcin(ctx, src, w, b, 24, 1)          # resize needs S % Hout == 0
    with pytest.raises(ValueError):
        ops.conv_smallcin(ctx, src, torch.zeros((3, 3, 2, 32), device="cuda"), None, 16, 1)


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from moonsuperresolution_amd import ops
from tests.test_gpu_small_kernels import SMALLCIN_CASES, _smallcin_inputs
ctx = ops.OpContext()
out = {}
for i, (m, B, S, hout, cout, act, bias, kernel) in enumerate(SMALLCIN_CASES):
    if kernel != "tiled":
        continue
    src, w, b = _smallcin_inputs(m, B, S, cout, bias, 1000 * m + 10 * B + hout)
    for fmt in (0, 4):
        out[(i, fmt)] = ops.conv_smallcin(ctx, src, w, b, hout, m, act, 0.2 if act == 2 else 0.0, out_split=fmt).cpu()
torch.save(out, sys.argv[2])
ctx.close()
"""


def test_conv_smallcin_tiled_equals_untiled(ctx, tmp_path):
    """small_kernels.hip: the tiled kernel does the same multiplications and additions in the same order as the untiled one, so
    their outputs are bit-identical.  The untiled kernel at the tiled shapes runs in a child process with
    MSR_SMALLCIN_TILED=0 (read once per process)."""
    from moonsuperresolution_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "untiled.pt")
    env = dict(os.environ, MSR_SMALLCIN_TILED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, path], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    untiled = torch.load(path)
    assert len(untiled) == 8
    for (i, fmt), yu in untiled.items():
        m, B, S, hout, cout, act, bias, kernel = SMALLCIN_CASES[i]
        src, w, b = _smallcin_inputs(m, B, S, cout, bias, 1000 * m + 10 * B + hout)
        yt = ops.conv_smallcin(ctx, src, w, b, hout, m, act, 0.2 if act == 2 else 0.0, out_split=fmt).cpu()
        assert torch.equal(_bytes(yt), _bytes(yu)), (SMALLCIN_CASES[i], fmt)


@pytest.mark.parametrize("B,H,C,out_padded,out_split", [(3, 8, 64, False, False), (3, 16, 128, True, False), (1, 32, 32, True, False),
                                                       (3, 8, 256, False, True), (2, 16, 128, True, True)])
def test_norm_act(ctx, B, H, C, out_padded, out_split):
    """norm_act (InstanceNormalization apply + leaky_relu, blocks.py:62-65) with per-sample statistics, against float64:
        |y - ref| <= 4 * 2^-24 * (|(x - m) / s * gamma| + |beta|)        (subtract, divide, multiply, add; then the slope)
    Dense, zero-bordered (border stays zero) and split-bf16 outputs (= the host split of the fp32 output, byte for byte)."""
    from moonsuperresolution_amd import ops
    g = torch.Generator(device="cpu").manual_seed(B * 100 + H + C)
    x = (5 + 3 * torch.randn((B, H, H, C), generator=g)) * torch.logspace(-1, 1, C)
    mean = x.mean((1, 2)) + 0.1 * torch.randn((B, C), generator=g)              # per sample, not quite the data's own
    std = x.std((1, 2)) * (1 + 0.1 * torch.rand((B, C), generator=g))
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    slope = float(np.float32(0.2))
    args = [t.cuda() for t in (x, mean, std, gamma, beta)]
    y = ops.norm_act(ctx, *args, slope=slope, out_padded=out_padded).cpu()
    a = (x.double() - mean.double()[:, None, None]) / std.double()[:, None, None] * gamma.double()
    ref = a + beta.double()
    ref = torch.where(ref >= 0, ref, slope * ref)
    yi = y[:, 1:-1, 1:-1] if out_padded else y
    bound = 4 * U * (a.abs() + beta.double().abs())
    err = (yi.double() - ref).abs()
    print(f"norm_act B={B} H={H} C={C} padded={out_padded}: max |err| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    if out_padded:
        border = y.clone()
        border[:, 1:-1, 1:-1] = 0
        assert float(border.abs().max()) == 0
    if out_split:
        ys = ops.norm_act(ctx, *args, slope=slope, out_padded=out_padded, out_split=True).cpu()
        assert torch.equal(_bytes(ys), _bytes(_split_bf16_host(y)))


@pytest.mark.parametrize("B,K,N,bias", [(1, 1000, 100, True), (2, 7, 1024, False), (3, 1000, 2052, True), (5, 13, 516, True),
                                        (8, 1000, 1000, False), (12, 300, 256, True), (16, 1000, 2048, True), (16, 64, 64, False),
                                        (2, 131072, 512, True),     # encoder heads: 1024 K chunks -> dense_final
                                        (8, 256, 65536, True)])     # generator dense: 8 K chunks -> dense_final_flat
def test_dense(ctx, B, K, N, bias):
    """dense_partial<NB> (NB = B rounded up to 1, 2, 4, 8, 16) + dense_final / dense_final_flat against float64:
        |y - ref| <= (kch + splits + 1) * 2^-24 * (|x| . |W| + |bias|)
    (an FMA chain of <= kch terms per K chunk, the chunks added in order, then the bias).  K = 1000, 300, 13, 7: ragged chunk
    tails and chunks shorter than the 16-row unrolled loop; N % 512 != 0: threads past the last column."""
    from moonsuperresolution_amd import ops
    g = torch.Generator(device="cuda").manual_seed(B * 7 + K + N)
    x = torch.randn((B, K), generator=g, device="cuda")
    w = torch.randn((K, N), generator=g, device="cuda") / np.sqrt(K)
    b = torch.randn(N, generator=g, device="cuda") if bias else None
    y = ops.dense(ctx, x, w, b).cpu().double()
    torch.set_num_threads(16)
    xd, wd = x.double().cpu(), w.double().cpu()
    ref = xd @ wd
    mag = xd.abs() @ wd.abs()
    if bias:
        ref = ref + b.double().cpu()
        mag = mag + b.double().cpu().abs()
    kch = _dense_kch(K, N)
    splits = (K + kch - 1) // kch
    bound = (kch + splits + 1) * U * mag
    err = (y - ref).abs()
    print(f"dense B={B} K={K} N={N} (kch {kch}, {splits} splits): max |err| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_latent(ctx):
    """latent_kernel: sampler 0 (GauGAN_no_KL / CNNSpade: z = mean + variance) is the fp32 sum, bit for bit; sampler 1 (GauGAN:
    z = mean + exp(variance / 2) * eps, sampling.py:16) is within 4 * 2^-24 * (|m| + |exp(v / 2) eps|) of float64."""
    from moonsuperresolution_amd import ops
    g = torch.Generator(device="cpu").manual_seed(9)
    B, L = 3, 256
    mv = torch.cat([torch.randn((B, L), generator=g), 8 * torch.rand((B, L), generator=g) - 4], 1)
    eps = torch.randn((B, L), generator=g)
    z0 = ops.latent(ctx, mv.cuda(), None, 0).cpu()
    assert torch.equal(z0, mv[:, :L] + mv[:, L:])
    z1 = ops.latent(ctx, mv.cuda(), eps.cuda(), 1).cpu().double()
    m, v, e = mv[:, :L].double(), mv[:, L:].double(), eps.double()
    t = torch.exp(v / 2) * e
    bound = 4 * U * (m.abs() + t.abs())
    err = (z1 - (m + t)).abs()
    print(f"latent sampler: max |err| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    with pytest.raises(ValueError):
        ops.latent(ctx, mv.cuda(), None, 1)                # the sampler needs eps

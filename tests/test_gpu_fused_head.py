"""GPU (-m gpu): the opt-in fused head (MSR_FLAG_FUSED_HEAD, Generator(head="fused")).

conv_igemm_f16c_sw<EPI_RES_HEAD> (msr_op_conv3x3_f16c_head) runs the residual conv's K loop, applies leaky_relu(0.2) to the
residual epilogue's value and reduces the 128 channels against the head's 25 live per-parity taps on the fp16 MFMA (three
products per term), writing 32 partial sums per half-resolution pixel; head_gather_kernel adds the neighbours' sums and the bias.
  1. the kernel against float64 at the smallest shapes, with the separate chain (conv -> head_kernel) as the yardstick;
  2. more tiles than workgroups: a workgroup's second tile over the LDS its reduction used; run-to-run bits;
  3. the entry's validation;
  4. the plan under the flag and the flag's checks in msr_create;
  5. the generator end to end at (128, 16), the smallest shape where the plan takes the fused head.
Bounds: a CPU emulation of the three-term fp16 form over 3 200-term sums (tools/emulate_head_split.py, seeds 0 and 1) puts it
at 3.5-5.1e-7 of the output range against float64, head_kernel's fp32 fmaf chain at 1.1e-6, the two 1.0-1.3e-6 apart (twice that
as rel_linf, which divides by max |.|: about 2.5e-6, a quarter of the 1e-5 the comparisons below allow)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import make_latent_noise, make_weights, synthetic_patches
from tests.helpers import _ref_f16c, rel_linf

pytestmark = pytest.mark.gpu
F16C_TOL = 2.5e-4      # tests/test_gpu_baseline_configs.py: MODE_TOL["f16c"], inside TOL = 1e-3 (north_star)
TOL = 1e-3
HEAD_BIAS = 0.1


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert torch.cuda.is_available()
    from moonsuperresolution_amd import ops
    c = ops.OpContext()
    yield c
    c.close()


def _inputs(B, r, cin, shift, seed):
    """Operands of one residual conv built as tests/test_gpu_conv_kernel.py::test_conv_f16c builds them (weights spanning three
    decades), and a head kernel [4, 4, 128] at glorot scale."""
    from moonsuperresolution_amd import ops
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((B, r, r, cin), generator=g).cuda()
    w = (torch.randn((3, 3, cin, 128), generator=g) / np.sqrt(9 * cin) * torch.logspace(-2, 1, 128)).cuda()
    b = torch.randn(128, generator=g).cuda()
    skip = torch.randn((B, r >> shift, r >> shift, 128), generator=g).cuda()
    k = (torch.randn((4, 4, 128), generator=g) / np.sqrt(16 * 128)).numpy()
    ximg, xparts = ops.f16c_activation_image(ops.pad_nhwc(x))
    wimg, wexp, wparts = ops.f16c_weight_image(ops.kernel_layout(w))
    return dict(x=x, w=w, b=b, skip=skip, k=k, ximg=ximg, xparts=xparts, wimg=wimg, wexp=wexp, wparts=wparts)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float((np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))).max())


@pytest.mark.parametrize("B,r,cin,shift", [(1, 16, 128, 0), (3, 32, 256, 1)])
def test_fused_head_kernel_against_fp64(ctx, B, r, cin, shift):
    """(1, 16, 128, 0): one tile, all four borders.  (3, 32, 256, 1): tile seams inside the image, batch boundaries, the
    residual read through the folded 2x up-sample.  Reference: the float64 evaluation of the conv's own three terms on the decoded
    pieces + residual + bias, leaky_relu, the oracle's head in float64.  The fused chain may not be further from it than the
    separate chain (msr_op_conv3x3_f16c -> msr_op_head) by more than 1e-5; the partial sums equal weff . leaky_relu(separate conv
    output) within 1e-5 of their range; the torch restatement of the gather equals the gather kernel within 2 ulp."""
    from moonsuperresolution_amd import ops
    from oracle import generator_ref as G
    d = _inputs(B, r, cin, shift, 700 + B + r)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    xin = tuple(t[:, 1:-1, 1:-1].cpu() for t in d["xparts"])
    up = d["skip"].double().cpu().repeat_interleave(1 << shift, 1).repeat_interleave(1 << shift, 2)
    v = _ref_f16c(xin, tuple(t.cpu() for t in d["wparts"]), d["b"], cin, 128) + up
    k64 = torch.from_numpy(d["k"]).double()
    ref = G.conv2d_same(G.leaky_relu(G.upsample2x(v), G.LEAK), k64[..., None], torch.tensor([HEAD_BIAS], dtype=torch.float64))[..., 0]
    ref = ref.numpy()

    y = ops.conv3x3_f16c(ctx, d["ximg"], d["wimg"], d["wexp"], d["b"], r, epilogue=ops.EPI_RES, aux=d["skip"], aux_shift=shift)
    sep = ops.head(ctx, y, d["k"], HEAD_BIAS).cpu().numpy()
    out, part = ops.conv3x3_f16c_head(ctx, d["ximg"], d["wimg"], d["wexp"], d["b"], r, d["skip"], shift, d["k"], HEAD_BIAS,
                                      want_partial=True)
    err_sep, err_fused = rel_linf(sep, ref), rel_linf(out.cpu().numpy(), ref)
    print(f"fused head B={B} r={r} cin={cin} shift={shift}: separate {err_sep:.3e}, fused {err_fused:.3e} vs fp64")
    assert out.shape == (B, 2 * r, 2 * r) and bool(torch.isfinite(out).all())
    assert err_fused <= err_sep + 1e-5, (err_fused, err_sep)

    P64 = ops.head_partials(y.double().cpu(), k64)
    perr = float((part.double().cpu() - P64).abs().max() / P64.abs().max())
    print(f"  partial sums vs weff . lrelu(separate conv output) in fp64: {perr:.3e} of max|P|")
    assert perr <= 1e-5, perr
    assert float(part[..., 25:].abs().max()) == 0.0
    ulps = _ulps(ops.head_from_partials(part, HEAD_BIAS).cpu().numpy(), out.cpu().numpy())
    print(f"  gather restated in torch vs head_gather_kernel: {ulps:.1f} ulp")
    assert ulps <= 2.0, ulps


def test_fused_head_second_tile_of_a_workgroup(ctx):
    """(5, 128, 128, 0): 320 tiles on 256 persistent workgroups, so 64 workgroups run a second tile whose K loop stages its halo
    into the LDS buffers the first tile's reduction used.  Fused against separate, both on the GPU: rel_linf <= 1e-5 (4x the
    emulation's 2.5e-6).  Two runs give the same bits (no atomics: the waves' partials are summed in a fixed order)."""
    from moonsuperresolution_amd import ops
    B, r, cin = 5, 128, 128
    d = _inputs(B, r, cin, 0, 905)
    y = ops.conv3x3_f16c(ctx, d["ximg"], d["wimg"], d["wexp"], d["b"], r, epilogue=ops.EPI_RES, aux=d["skip"], aux_shift=0)
    sep = ops.head(ctx, y, d["k"], HEAD_BIAS)
    runs = [ops.conv3x3_f16c_head(ctx, d["ximg"], d["wimg"], d["wexp"], d["b"], r, d["skip"], 0, d["k"], HEAD_BIAS, want_partial=True)
            for _ in range(2)]
    err = float((runs[0][0] - sep).abs().max() / sep.abs().max())
    print(f"fused vs separate head at (5, 128, 128): rel_linf {err:.3e}")
    assert err <= 1e-5, err
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_fused_head_entry_validation(ctx):
    """N = 256 (two column blocks: no workgroup holds all channels of a pixel), Cin = 64 (not the stream kernel's form) and a
    rout that is no power of two are refused with MSR_ERR_INVALID before anything runs."""
    from moonsuperresolution_amd import ops
    k = np.zeros((4, 4, 128), np.float32)
    wexp = torch.full((256,), 127 | (127 << 8), dtype=torch.int32, device="cuda")

    def call(r, cin, N):
        x = torch.zeros((1, r + 2, r + 2, cin), device="cuda")
        w = torch.zeros((9, N, cin), device="cuda")
        return ops.conv3x3_f16c_head(ctx, x, w, wexp, torch.zeros(N, device="cuda"), r, torch.zeros((1, r, r, N), device="cuda"),
                                     0, k, 0.0)
    for r, cin, N in ((16, 128, 256), (16, 64, 128), (24, 128, 128)):
        with pytest.raises(ValueError, match="msr_op_conv3x3_f16c_head"):
            call(r, cin, N)
    assert float(call(16, 128, 128).abs().max()) == 0.0      # the accepted form of the same call


def _forms_text(gen):
    gen.prepare()
    buf = C.create_string_buffer(1 << 18)
    assert gen._lib.msr_debug_conv_forms(gen._h, buf, len(buf)) == 0
    return buf.value.decode()


def test_plan_under_fused_head(hip_lib):
    """GauGAN(128, 16): rb6 runs at r = 64 with 256 whole tiles, gen.rb6.conv_2 on the stream kernel: the plan takes the request.
    The fused conv (epi=5) writes ws.gen.head.partial, one head_gather follows, and the head op, the tensor ws.gen.rb6.out and
    the moments of it are gone; every other line equals the default plan's.  GauGAN(64, 4): that conv runs K ranges on the
    ping-pong kernel, so the separate head stays and the forms equal the default's byte for byte.  msr_create refuses the flag
    without F16C, with F16_MAIN, with CROSS_FP6."""
    from moonsuperresolution_amd import Generator, _lib
    from moonsuperresolution_amd.generator import parse_conv_forms
    gen = Generator(128, 16, precision="f16c", head="fused")
    assert gen.head == "fused" and gen.head_fused is True
    ftext = _forms_text(gen)
    gen.close()
    plain = Generator(128, 16, precision="f16c")
    assert plain.head == "separate" and plain.head_fused is False
    ptext = _forms_text(plain)
    plain.close()
    flines, plines = ftext.splitlines(), ptext.splitlines()
    forms = parse_conv_forms(ftext)
    fused = [op for op in forms if op["kind"] == "conv" and op["out"] == "ws.gen.head.partial"]
    assert len(fused) == 1, fused
    cv = fused[0]
    assert (cv["epi"], cv["prec"], cv["ksplit"], cv["no_cross"], cv["stat_slabs"], cv["N"], cv["r"], cv["img"]) == \
        (5, 4, 1, 0, 0, 128, 64, "F16C"), cv
    assert cv["wt"] == "gen.rb6.conv_2.kernel" and cv["mean"] == "gen.head.wfrag" and cv["aux"] == "ws.gen.rb6.skip", cv
    gathers = [op for op in forms if op["kind"] == "head_gather"]
    assert gathers == [dict(kind="head_gather", out="output", B=16, r=64, **{"in": "ws.gen.head.partial"})], gathers
    assert forms[-1]["kind"] == "head_gather" and forms[-2] is cv
    assert not [op for op in forms if op["kind"] == "head"]
    assert "ws.gen.rb6.out" not in ftext and "ws.gen.rb6.meano" not in ftext
    gone = [ln for ln in plines if "out=ws.gen.rb6.out" in ln or "mean=ws.gen.rb6.meano" in ln or ln.startswith("kind=head ")]
    assert len(gone) == 3, gone
    assert [ln for ln in plines if ln not in gone] == [ln for ln in flines if "ws.gen.head.partial" not in ln]

    small = Generator(64, 4, precision="f16c", head="fused")
    assert small.head == "fused" and small.head_fused is False
    stext = _forms_text(small)
    small.close()
    base = Generator(64, 4, precision="f16c")
    btext = _forms_text(base)
    base.close()
    assert stext == btext

    lib = _lib.load()
    for flags in (64, 1 | 64, 1 | 8 | 16 | 64, 1 | 8 | 32 | 64):
        cfg = _lib.MsrConfig(128, 16, 256, _lib.VARIANT_IDS["gaugan"], 0, flags)
        handle = C.c_void_p()
        assert lib.msr_create(C.byref(cfg), C.byref(handle)) == _lib.MSR_ERR_INVALID, flags
        assert b"MSR_FLAG_FUSED_HEAD" in lib.msr_last_error(None), flags
    cfg = _lib.MsrConfig(256, 1, 256, _lib.VARIANT_IDS["pix2pix"], 0, 1 | 8 | 64)
    handle = C.c_void_p()
    assert lib.msr_create(C.byref(cfg), C.byref(handle)) == _lib.MSR_ERR_INVALID
    assert b"MSR_FLAG_FUSED_HEAD" in lib.msr_last_error(None)


def test_generator_with_fused_head_matches_oracle(hip_lib):
    """GauGAN(128, 16), same weights, input and noise under both heads, one float64 oracle call.  The fused output holds f16c's
    bound against the oracle and is within 1e-5 of the separate head's; the algorithmic FLOP count is the same; the workspace
    is smaller by the 96 floats per pixel that are no longer written; ws.gen.rb6.out cannot be read and says why;
    ws.gen.head.partial can; HIP-graph replays and a gated call equal the eager call bit for bit; the range scan's regime is
    unchanged; clone() carries the option."""
    from moonsuperresolution_amd import Generator
    from oracle import generator_ref
    S, B, r = 128, 16, 64
    w = make_weights("gaugan", S, seed=1234, bias_scale=0.05)
    eps = make_latent_noise(B, 256, 7)
    x = synthetic_patches(B, S, 0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = np.asarray(generator_ref.spade_call(x, w, "gaugan", eps, dtype=torch.float64), np.float64)

    sep = Generator(S, B, variant="gaugan", weights=w, eps=eps, precision="f16c")
    out_sep = sep(x, training=False)
    flops_sep, bytes_sep, regime_sep = sep.forward_flops(), sep.device_bytes(), sep.range_report().regime
    sep.close()
    del sep
    torch.cuda.empty_cache()

    gen = Generator(S, B, variant="gaugan", weights=w, eps=eps, precision="f16c", head="fused")
    assert gen.head_fused
    out = gen(x, training=False)
    err, err_sep, diff = rel_linf(out, ref), rel_linf(out_sep, ref), rel_linf(out, out_sep)
    print(f"fused head end to end (128, 16): fused {err:.3e}, separate {err_sep:.3e} vs the fp64 oracle; fused vs separate {diff:.3e}")
    assert out.shape == (B, S, S, 1) and np.isfinite(out).all()
    assert err <= TOL and err <= F16C_TOL, (err, err_sep)
    assert diff <= 1e-5, diff
    assert gen.forward_flops() == flops_sep
    assert bytes_sep - gen.device_bytes() >= B * r * r * (128 - 32) * 4, (bytes_sep, gen.device_bytes())
    with pytest.raises(ValueError, match="MSR_FLAG_FUSED_HEAD"):
        gen.debug_tensor("ws.gen.rb6.out", (B, r, r, 128))
    part = torch.from_numpy(gen.debug_tensor("ws.gen.head.partial", (B, r, r, 32)))
    from moonsuperresolution_amd import ops
    bias = float(np.asarray(w["gen.head.bias"]).reshape(-1)[0])
    assert _ulps(ops.head_from_partials(part, bias).numpy(), out[..., 0]) <= 2.0
    assert gen.range_report().regime == regime_sep

    xd = torch.from_numpy(x).to(gen.device)
    buf = torch.empty((B, S, S, 1), dtype=torch.float32, device=gen.device)
    with torch.cuda.device(gen.device):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            eager = gen.forward_device(xd, out=buf).clone()
            gen.use_graph(True)
            replays = [gen.forward_device(xd, out=buf).clone() for _ in range(3)]     # eager (first sighting), capture, replay
            gen.use_graph(False)
            gate = torch.cuda.Event()
            gate.record(stream)
            gated = gen.forward_device(xd, out=buf, gate=gate).clone()
        stream.synchronize()
    assert np.array_equal(eager.cpu().numpy(), out)
    assert all(torch.equal(t, eager) for t in replays) and torch.equal(gated, eager)

    twin = gen.clone()
    assert twin.head == "fused" and twin.head_fused
    assert np.array_equal(twin(x, training=False), out)
    twin.close()
    gen.close()

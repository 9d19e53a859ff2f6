"""GPU (-m gpu): the activation-range scan (csrc/range_scan.hip) against its host twin ``ops.range_stats`` — exact equality,
max_abs bit for bit — at the kernel level, over the planned network in its three regimes, through precision="auto" and
through the tiler's range_check.

The network-level cases share ONE GauGAN(256, 16) handle whose weights change through ``Generator.load``.  The scale factors of
the degraded / clamped cases come from the float64 oracle of the scaled layer, computed here on the CPU (blocks 1-4 and the
SPADE layer of block 5: the activation is linear in that layer's gamma|beta weights), never from the code under test."""
import re
import warnings

import numpy as np
import pytest
import torch

from oracle import generator_ref as G
from tests.helpers import synthetic_raster

pytestmark = pytest.mark.gpu
NARROW = (2, 3, 4, 5)
GB_NAMES = ("conv_gamma.kernel", "conv_gamma.bias", "conv_beta.kernel", "conv_beta.bias")


def same(a: dict, b: dict) -> bool:
    """Two records agree in the five scanned fields; max_abs compared on its bits."""
    keys = ("n_total", "n_cross_clipped", "n_clamped", "n_nonfinite")
    return all(int(a[k]) == int(b[k]) for k in keys) and \
        np.float32(a["max_abs"]).tobytes() == np.float32(b["max_abs"]).tobytes()


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from moonsuperresolution_amd import ops
    c = ops.OpContext()
    yield c
    c.close()


# ---- 1. kernel against the twin -----------------------------------------------------------------------------------------------
def planted_data(B, r, C, seed, top):
    """Ordinary data (max about 40) with the boundary values of every regime planted at random interior positions.  Values
    beyond the format's largest finite one are clamped to it first, as every producer epilogue does."""
    from moonsuperresolution_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, r, r, C), generator=g) * 10.0
    lim = ops.e4m3_cross_limit()
    nxt = float(np.nextafter(np.float16(lim), np.float16(np.inf)))
    vals = [448.0, -448.0, lim, -lim, nxt, -nxt, 512.0, 1000.0, -1000.0, 65504.0, -65504.0, 1e5, -3e5, 57344.0, -57344.0, 49152.0]
    pos = torch.randperm(x.numel(), generator=g)[:3 * len(vals)]
    flat = x.reshape(-1)
    for k, p in enumerate(pos.tolist()):
        flat[p] = vals[k % len(vals)]
    flat[int(pos[0])] = 1e5                                   # the last element of the tensor and the first carry a value too
    flat[-1], flat[0] = -65504.0, nxt
    return x.clamp(-top, top)


@pytest.mark.parametrize("fmt", NARROW)
@pytest.mark.parametrize("B,r,C,padded", [(3, 24, 96, True), (1, 16, 32, False), (2, 40, 288, True)])
def test_kernel_equals_host_twin(ctx, fmt, B, r, C, padded):
    from moonsuperresolution_amd import ops
    x = planted_data(B, r, C, seed=100 * fmt + r, top=ops.BF8_MAX if fmt == 3 else ops.F16_MAX)
    xp = ops.pad_nhwc(x) if padded else x
    build = {2: ops.split_f16, 3: lambda t: ops.bf8_activation_image(t)[0], 4: lambda t: ops.f16c_activation_image(t)[0],
             5: lambda t: ops.f16c6_activation_image(t)[0]}[fmt]
    img = build(xp)
    want = ops.range_stats(img, fmt, padded, channels=C)
    assert want["n_total"] == B * r * r * C and want["n_clamped"] > 0 and want["n_nonfinite"] == 0
    assert (want["n_cross_clipped"] > want["n_clamped"]) if fmt == 4 else want["n_cross_clipped"] == 0
    dev = img.to(ctx.device)
    got = ops.range_scan(ctx, dev, fmt, B, r, C, padded)
    print(f"fmt {fmt} B={B} r={r} C={C} padded={padded}: kernel {got}  twin {want}")
    assert same(got, want), (got, want)
    assert same(ops.range_scan(ctx, dev, fmt, B, r, C, padded), got)          # deterministic: a second scan is identical
    zero = ops.range_scan(ctx, torch.zeros_like(dev), fmt, B, r, C, padded)
    assert same(zero, dict(max_abs=np.float32(0), n_total=B * r * r * C, n_cross_clipped=0, n_clamped=0, n_nonfinite=0)), zero


def test_kernel_counts_non_finite_main_pieces(ctx):
    """No producer writes one (they clamp), but a record must say so if a tensor ever holds one."""
    from moonsuperresolution_amd import ops
    x = torch.randn(2, 8, 8, 64) * 5
    x[1, 3, 4, 5], x[0, 0, 0, 63], x[1, 7, 7, 0] = float("inf"), float("nan"), 3000.0
    for fmt, img in ((4, ops.f16c_activation_image(x)[0]), (2, ops.split_f16(x))):
        want = ops.range_stats(img, fmt, False)
        assert want["n_nonfinite"] == 2 and want["max_abs"] == np.float32(3000.0)
        got = ops.range_scan(ctx, img.to(ctx.device), fmt, 2, 8, 64, False)
        assert same(got, want), (fmt, got, want)


def test_bad_arguments_are_invalid(ctx):
    from moonsuperresolution_amd import _lib, ops
    img = torch.zeros((1, 8, 8, 32), device=ctx.device)
    for fmt, B, r, C in ((1, 1, 8, 32), (6, 1, 8, 32), (4, 0, 8, 32), (4, 1, 0, 32), (4, 1, 8, 48), (4, 1, 8, 0)):
        with pytest.raises(ValueError):
            ops.range_scan(ctx, img, fmt, B, r, C, False)
    rec = _lib.MsrRangeStat()
    assert ctx.lib.msr_op_range_scan(ctx.h, None, 4, 1, 8, 32, 0, rec, None) == _lib.MSR_ERR_INVALID


# ---- 2, 3. the planned network in its three regimes ----------------------------------------------------------------------------
def op_channels(op):
    return op["N"] // 2 if op["kind"] == "gbr" or (op["kind"] == "conv" and op["epi"] == 2) else op["N"]


def twin_of(gen, forms, record):
    """ops.range_stats of the tensor a record names, read back with debug_tensor (all narrow tensors are zero-bordered)."""
    from moonsuperresolution_amd import ops
    op = forms[record["producer"]]
    assert op["out"] == record["tensor"] and op["out_split"] == record["format"]
    C = op_channels(op)
    slots = C if record["format"] != 3 else (128 if C <= 128 else (C + 255) // 256 * 256) // 4
    img = torch.from_numpy(gen.debug_tensor(record["tensor"], (op["B"], op["r"] + 2, op["r"] + 2, slots)))
    if record["format"] == 3:
        img = img.view(torch.uint8)
    return ops.range_stats(img, record["format"], True, channels=C)


def oracle_a1_max(w, x, eps, variant, block):
    """max |lrelu(SPADE_1(input of block))| of the float64 oracle on the CPU."""
    w64 = {k: torch.from_numpy(np.asarray(v)).double() for k, v in w.items()}
    src = torch.from_numpy(x).double()
    with torch.no_grad():
        m, v = G.encoder(src, w64)
        z = m + torch.exp(0.5 * v) * torch.from_numpy(eps).double() if variant == "gaugan" else m + v
        sw = x.shape[1] // 64
        h = (z @ w64["gen.dense.kernel"] + w64["gen.dense.bias"]).reshape(-1, sw, sw, 1024)
        for i in range(1, block):
            h = G.upsample2x(G.residual_block(h, src, w64, f"gen.rb{i}"))
        a = G.leaky_relu(G.spade(h, src, w64, f"gen.rb{block}.spade_1"), G.LEAK)
    return float(a.abs().max())


def scaled(w, block, factor):
    out = dict(w)
    for n in GB_NAMES:
        out[f"gen.rb{block}.spade_1.{n}"] = (w[f"gen.rb{block}.spade_1.{n}"] * np.float32(factor)).astype(np.float32)
    return out


def test_network_three_regimes(hip_lib):
    from moonsuperresolution_amd import Generator, make_latent_noise, make_weights, synthetic_patches
    S, B = 256, 16
    w = make_weights("gaugan", S, seed=1234)
    eps = make_latent_noise(B, 256, seed=7)
    x = synthetic_patches(B, S, seed=0)
    gen = Generator(S, B, variant="gaugan", weights=w, eps=eps, precision="f16c")
    with pytest.raises(RuntimeError):
        gen.range_scan_async()                                 # MSR_ERR_STATE before the first forward
    # -- parity regime: default weights
    rep = gen.range_report(x)
    forms = gen.conv_forms()
    want_names = {op["out"] for op in forms if op.get("out_split", 0) in NARROW}
    assert want_names and {r["tensor"] for r in rep.records} == want_names and len(rep.records) == len(want_names)
    for r in rep.records:
        assert same(r, twin_of(gen, forms, r)), (r, twin_of(gen, forms, r))
    print("parity:", rep, " max over tensors:", max(float(r["max_abs"]) for r in rep.records))
    assert rep.regime == "parity" and not rep.flagged()
    gbr = [k for k, op in enumerate(forms) if op["kind"] == "gbr"]
    assert gbr and [e["producer"] for e in rep.embed_bounds] == gbr
    for e in rep.embed_bounds:
        name = forms[e["producer"]]["embed"]
        assert e["tensor"] == name and e["format"] == 100
        k, b = w[name].astype(np.float64), w[name[:-6] + "bias"].astype(np.float64)
        bound = (0.5 * np.abs(k).reshape(18, 128).sum(axis=0) + np.abs(b)).max()
        assert np.float32(e["max_abs"]) == np.float32(bound), (name, e["max_abs"], bound)
    # -- the other two regimes: ONE gamma|beta pair scaled, the factor from the oracle's own maximum
    target = "ws.gen.rb5.a1"
    producer = [k for k, op in enumerate(forms) if op.get("out") == target]
    assert len(producer) == 1 and forms[producer[0]]["out_split"] == 4
    amax = oracle_a1_max(w, x, eps, "gaugan", 5)
    print(f"oracle max |{target}| with the default weights: {amax:.6g}")
    for goal, regime in ((2000.0, "degraded"), (4.0e5, "clamped")):     # beyond 464 and far below 65504 | beyond 65504
        gen.load(scaled(w, 5, goal / amax))
        rep = gen.range_report(x)
        print(f"{regime}:", rep)
        assert rep.regime == regime
        assert rep.worst["tensor"] == target and rep.worst["producer"] == producer[0]
        assert target in str(rep) and forms[producer[0]]["wt"] in str(rep)
        assert not [r["tensor"] for r in rep.records if r["producer"] < producer[0] and r["tensor"] in rep.flagged()]
        hit = rep.worst
        assert hit["n_cross_clipped"] > 0 and same(hit, twin_of(gen, forms, hit))
        if regime == "degraded":
            assert hit["n_clamped"] == 0 and hit["n_nonfinite"] == 0 and 464.0 < float(hit["max_abs"]) < 65504.0
        else:
            assert hit["n_clamped"] > 0 and float(hit["max_abs"]) == 65504.0
    gen.load(w)
    assert gen.range_report(x).regime == "parity"
    gen.close()
    # a mode without narrow tensors: an empty report in the parity regime (a small handle; nothing to scan)
    g32 = Generator(64, 2, variant="gaugan_no_kl", weights=3, precision="bf16x3")
    rep = g32.range_report(synthetic_patches(2, 64, seed=1))
    assert rep.records == [] and rep.regime == "parity"
    g32.close()


# ---- 4, 5. precision="auto" and the tiler ----------------------------------------------------------------------------------------
def smallest_size_with_narrow_tensors(B):
    """The smallest image size whose f16c plan writes a narrow tensor by a SPADE_1 layer, found from the plan."""
    from moonsuperresolution_amd import Generator
    tried = []
    for S in (64, 128, 256):
        g = Generator(S, B, variant="gaugan_no_kl", weights=11, precision="f16c")
        forms = g.conv_forms()
        g.close()
        hits = [op["out"] for op in forms if op.get("out_split", 0) in NARROW and re.fullmatch(r"ws\.gen\.rb\d\.a1", op.get("out", ""))]
        tried.append((S, len(hits)))
        if hits:
            return S, int(hits[0][9]), tried
    raise AssertionError(f"no narrow tensor up to S = 256: {tried}")


def test_precision_auto_and_tiler_range_check(hip_lib):
    """At S = 64 no layer runs a narrow format (the plan says so below); the cases run at the smallest size that has one."""
    from moonsuperresolution_amd import DEMSuperResolution, DSRConfig, Generator, make_weights, synthetic_patches
    B = 4
    S, block, tried = smallest_size_with_narrow_tensors(B)
    print(f"narrow SPADE_1 outputs per image size (B = {B}): {tried}; using S = {S}, block {block}")
    if S > 64:
        assert tried[0] == (64, 0)                              # stated: at S = 64 no layer may run a narrow format
    w = make_weights("gaugan_no_kl", S, seed=1234, bias_scale=0.05)
    x = synthetic_patches(B, S, seed=0)
    amax = oracle_a1_max(w, x, None, "gaugan_no_kl", block)
    hot = scaled(w, block, 2000.0 / amax)
    probe = synthetic_patches(B, S, seed=3)
    for weights, mode, regime in ((w, "f16c", "parity"), (hot, "bf16x3", "degraded")):
        auto = Generator(S, B, variant="gaugan_no_kl", weights=weights, precision="auto", calibrate=x)
        assert auto.precision == mode and auto.range.regime == regime, (auto.precision, str(auto.range))
        plain = Generator(S, B, variant="gaugan_no_kl", weights=weights, precision=mode)
        assert np.array_equal(auto(probe), plain(probe))
        twin = auto.clone()
        assert twin.precision == mode and twin.range is auto.range
        for g in (twin, plain, auto):
            g.close()
    dflt = Generator(S, B, variant="gaugan_no_kl", weights=w, precision="auto")      # calibrate=None: synthetic patches
    assert dflt.precision == "f16c" and dflt.range.regime == "parity" and dflt.range.records
    dflt.close()
    # -- tiler: a one-tile raster
    img, dem = synthetic_raster(S + 40, S + 40, 9)
    cfg = DSRConfig(image_size=S, stride=S // 2, batch_size=B, tile_size=2 * S)
    gen = Generator(S, B, variant="gaugan_no_kl", weights=hot, precision="f16c")
    base = DEMSuperResolution(cfg, model=gen)
    ref = base.processMap(img, dem)
    assert base.range_check == "off" and base.range_report is None and ref[2].any()
    base.close()
    off = DEMSuperResolution(cfg, model=gen, range_check="off")
    got = off.processMap(img, dem)
    assert all(np.array_equal(a, b) for a, b in zip(got, ref)) and off.range_report is None
    off.close()
    warn = DEMSuperResolution(cfg, model=gen, range_check="warn")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = warn.processMap(img, dem)
    mine = [m for m in seen if "range_check" in str(m.message)]
    assert len(mine) == 1 and f"ws.gen.rb{block}.a1" in str(mine[0].message), [str(m.message) for m in seen]
    assert warn.range_report is not None and warn.range_report.regime == "degraded"
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    warn.close()
    strict = DEMSuperResolution(cfg, model=gen, range_check="raise")
    with pytest.raises(RuntimeError, match=rf"ws\.gen\.rb{block}\.a1"):
        strict.processMap(img, dem)
    strict.close()
    gen.load(w)                                                 # the same weights in their parity regime: silent
    calm = DEMSuperResolution(cfg, model=gen, range_check="raise")
    calm.processMap(img, dem)
    assert calm.range_report.regime == "parity"
    calm.close()
    gen.close()

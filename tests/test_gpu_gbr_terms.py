"""GPU (-m gpu): conv_gb_resident (csrc/conv_gbr.hip) term by term and per output channel.

The kernel's other tests compare the whole tensor with the float64 chain at rel_linf <= 2e-4, which a kernel without any cross
term nearly meets (tests/test_gbr_terms_host.py states that blind spot on the CPU).  Here:

Exact embedding (tests.helpers.gbr_exact_inputs).  The mask-embedding weights are non-zero only at the centre tap of mask
channel 0, be = 0, the mask is fp16: phase 1 computes e = relu(we[ch] * m[pixel]) as one exact product, so the host knows the
kernel's LDS operands bit for bit (ops.gbr_embedding_pieces: fp16 plane, block exponent as msr_block_e8m0_dev, fp6 pieces).

Term isolation.  The weight image is handed over in four forms (ops.f16c6_weight_keep on the pre-stream image of
ops.gbr_weight_perm_image): main only (both code pieces zeroed), w_l6 only (the x_h6 * w_l6 term), w_h6 only (the x_l6 * w_h6
term), all.  A cross piece that goes alone has both scale bytes raised by LIFT = 12 binades (exact): the term then comes out
on the main term's scale, where the f16c image that the kernel writes resolves 2^-14 of a channel's range (below 2^-7 its
e4m3 lo piece is subnormal).  The epilogue is made transparent one half at a time: "beta" (gamma weights and bias zero: the
output is lrelu(b)), "gamma 1" (beta zero, mean = 0, std = 1, x = 1: lrelu(g)), "gamma nk" (random x, mean, std: lrelu(g nk)).
Reference: float64 evaluation of exactly that term on the decoded operands, then the epilogue in float64, slope = float32(0.2).
Every channel: |hi + lo8 - ref| <= (2^-14 + 4 x the per-channel error of the same evaluation in plain fp32) x the channel's range.
Weights span three decades over the columns (logspace(-1.5, 1.5, N)).

Tie rule.  On exact midpoints (2.2 % of the l6 quotients, ~1e-5 of the h6 quotients with these inputs) the candidates of
v_cvt_scalef32_2xpk16_fp6_f32 are a code step apart.  test_tie_rule_of_the_fp6_converter evaluates the isolated terms under
each rule of ops.E2M3_TIE_RULES: the converter rounds ties to EVEN (share of the bound <= 1 under "even", far beyond it under
"odd", "away" and "zero"), so every bound here is asserted in its tight form, without the tie widening; the widened share is
recorded beside it.

One channel at a time (test_one_output_channel_at_a_time): a repeated launch gives equal bits; then one output channel's w_l6
scale byte (+3), w_h6 scale byte (-3), bias (gamma and beta row each), mean, std and slice of x are changed: every other channel
stays bit-identical, the channel changes and meets the bound against the reference with the same change; under no_cross the
scale changes leave the whole tensor bit-identical.  Channels 0, 3, 4, 15, 16, 31, 32, 47, 63 of each 64-channel block: every
wave (wq), lane group (cg) and k of `ch = ((n0 + (wq >> 1) * 64) >> 1) + (wq & 1) * 16 + 4 * cg + k`.

Work decomposition (tests.helpers.gbr_work restates conv_gbr_ranges of csrc/forms.hip, the entries' fall-back, persistent_grid, xcd_tile_range):
  (1, 32, 16, 256, 0)   one item, all sides on the border, nr = 4 (the w_nxt chain, the last block's self re-read), items % 8 == 1
  (5, 256, 32, 128, 1)  20 items on 24 workgroups (XCDs with 3 and 2 items), nr = 2, resize factor 8, folded up-sample
  (9, 64, 64, 128, 0)   ranges = 2, 288 items on 256 workgroups: 32 workgroups take a second item
Embedding read-back (test_embedding_read_back): generic embedding, one-hot beta weights: the output is hi + l6 of e itself.

Measured on an MI355X (profiles/gbr_terms_parity.jsonl holds the whole run).  Worst per-channel share of the bound over the three
epilogue modes, per case and term (main only / w_l6 only / w_h6 only / all / all under no_cross):
  (1, 32, 16, 256, 0)    0.32 / 0.56 / 0.23 / 0.32 / 0.24
  (5, 256, 32, 128, 1)   0.33 / 0.27 / 0.23 / 0.33 / 0.23
  (9, 64, 64, 128, 0)    0.32 / 0.24 / 0.22 / 0.32 / 0.23; over the 32 second-round items alone 0.31 / 0.24 / 0.20 / 0.31
  whole layer (2, 64, 32, 128, 1) 0.21; the 162 one-channel launches 0.22 at most; embedding read-back 0.08 of its bound.
What is left is the output image's own rounding (the float64 evaluation written through the host's f16c image gives the same
figures to two digits); second-round items show nothing the first-round ones do not.  Tie rule: even (shares 0.21 / 0.21 under
"even"; 270 .. 900 under "odd", "away", "zero"; the widened bound holds under all four, <= 0.997).  No channel needed the fp32
allowance: the largest per-channel error is 3.4e-5 of the channel's range, under 2^-14 = 6.1e-5, and the allowance itself is
2.8e-6 at most."""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import (f16c_terms, gbr_epilogue, gbr_exact_inputs, gbr_spade, gbr_term_figures, gbr_work, gbr_x_parts,
                           record_dir as _record_dir, ref_conv, spade_rows)

pytestmark = pytest.mark.gpu
LIFT = 12
TIE_RULE = "even"      # the rule test_tie_rule_of_the_fp6_converter finds; None: unknown, assert the widened bound
TERMS = {"main only": dict(h6=False, l6=False), "w_l6 only": dict(hi=False, h6=False, lift=LIFT),
         "w_h6 only": dict(hi=False, l6=False, lift=LIFT), "all": {}}
CASES = [(1, 32, 16, 256, 0), (5, 256, 32, 128, 1), (9, 64, 64, 128, 0)]


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
        with open(os.path.join(_record_dir(), "parity_gbr_terms.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")
    except OSError:
        pass
    print("gbr terms", kw)


def _up(t, shift):
    return t.repeat_interleave(1 << shift, 1).repeat_interleave(1 << shift, 2) if shift else t


_LAYERS = {}


class _Layer:
    """The exact-embedding layer on the device, its operand twins and its launches."""

    def __init__(self, ctx, B, S, r, C, shift, ties=None):
        from moonsuperresolution_amd import ops
        self.ctx, self.B, self.S, self.r, self.C, self.shift = ctx, B, S, r, C, shift
        inp = gbr_exact_inputs(B, S, r, 2 * C, seed=100 * B + r + C, shift=shift)
        self.inp = {k: v.cuda() for k, v in inp.items()}
        e = self.inp["e"]
        assert torch.equal(e.float().double(), e.double())
        self.order = ops.gbr_channel_order(128, e.device)
        self.xp, self.tp = gbr_x_parts(ops.gbr_embedding_pieces(e, ties=ties or TIE_RULE or "even"), self.order)
        self.img, _ = ops.gbr_weight_perm_image(self.inp["w"])
        self.rows_g = spade_rows(C).cuda()
        self.rows_b = self.rows_g + 32
        self.x1 = torch.ones_like(self.inp["x"])
        self.m0, self.s1 = torch.zeros_like(self.inp["mean"]), torch.ones_like(self.inp["std"])

    def xn(self, x=None, mean=None, std=None, dtype=torch.float64, ch=None):
        pick = lambda t, d: self.inp[d] if t is None else t      # noqa: E731
        ch = slice(None) if ch is None else ch
        return (_up(pick(x, "x"), self.shift)[..., ch].to(dtype) - pick(mean, "mean")[ch].to(dtype)) / pick(std, "std")[ch].to(dtype)

    def half_image(self, term, half):
        """-> (stream image, decoded (hi, h6, l6) of the kept rows, their GEMM rows, bias) for one term and one half."""
        from moonsuperresolution_amd import ops
        rows = self.rows_g if half == "gamma" else self.rows_b
        keep = torch.zeros(2 * self.C, dtype=torch.bool, device=rows.device)
        keep[rows] = True
        img = ops.f16c6_weight_keep(self.img, rows=keep, **TERMS[term])
        bias = torch.where(keep, self.inp["bias"], torch.zeros_like(self.inp["bias"]))
        return ops.gbr_weight_stream(img), tuple(t[:, rows] for t in ops.f16c6_weight_decode(img)), rows, bias

    def launch(self, stream, bias, x=None, mean=None, std=None, no_cross=False, out_mode=4):
        """-> the interior of the decoded image: (hi, h8, lo8) (out_mode 4) or (hi, h6, l6) (5)."""
        from moonsuperresolution_amd import ops
        pick = lambda t, d: self.inp[d] if t is None else t      # noqa: E731
        y = ops.spade_gbr(self.ctx, self.inp["src"], self.inp["we"], self.inp["be"], stream, bias, self.r, pick(x, "x"), self.shift,
                          pick(mean, "mean"), pick(std, "std"), no_cross=no_cross, out_mode=out_mode)
        dec = ops.f16c_decode(y) if out_mode == 4 else ops.f16c6_decode(y)
        raw = y.view(torch.int32)
        assert int(raw[:, 0].abs().max()) == 0 and int(raw[:, -1].abs().max()) == 0 and int(raw[:, :, 0].abs().max()) == 0 and \
            int(raw[:, :, -1].abs().max()) == 0, "the image's border is not zero"
        return tuple(t[:, 1:-1, 1:-1] for t in dec)

    def term_run(self, term, mode, no_cross=False, terms=(True, True, True)):
        """One isolation run -> (decoded output, ref, tie allowance on ref, fp32 evaluation)."""
        half = "beta" if mode == "beta" else "gamma"
        stream, wp, rows, bias = self.half_image(term, half)
        kw = dict(x=self.x1, mean=self.m0, std=self.s1) if mode == "gamma 1" else {}
        out = self.launch(stream, bias, no_cross=no_cross, **kw)
        nk = None if mode == "beta" else (torch.ones((), dtype=torch.float64, device=bias.device) if mode == "gamma 1" else self.xn())
        nk32 = None if nk is None else (nk.float() if mode == "gamma 1" else self.xn(dtype=torch.float32))
        wid = f16c_terms(self.tp, tuple(t.abs() for t in wp), self.r, terms=terms)
        ref, widen = gbr_epilogue(f16c_terms(self.xp, wp, self.r, terms=terms), rows, bias.double(), nk, widen=wid)
        ref32 = gbr_epilogue(f16c_terms(self.xp, wp, self.r, dtype=torch.float32, terms=terms), rows, bias, nk32)
        return out, ref, widen, ref32


def _layer(ctx, case):
    if case not in _LAYERS:
        _LAYERS.clear()                      # one layer's tensors at a time
        _LAYERS[case] = _Layer(ctx, *case)
    return _LAYERS[case]


def _judge(what, y, ref, ref32, widen, channels=None, **rec):
    """The per-channel bound of one run (module docstring), asserted in its tight form under TIE_RULE (widened if None)."""
    f = gbr_term_figures(y, ref, ref32, widen)
    share = f["share"] if TIE_RULE else f["share_wide"]
    i = int(share.argmax())
    ch = i if channels is None else int(channels[i])
    needed = [int(k) for k in np.nonzero(f["err"] > 2.0 ** -14)[0]]
    assert float(f["range"].min()) >= 2.0 ** -7 and float(f["range"].max()) < 65504, (what, "a channel's range leaves the f16c image's")
    _record(what=what, worst_share=float(share[i]), channel=ch, err=float(f["err"][i]), worst_err=float(f["err"].max()),
            share_tight=float(f["share"].max()), share_widened=float(f["share_wide"].max()), allowance=float(f["allowance"].max()),
            channels_beyond_2m14=len(needed), tie_rule=TIE_RULE, **rec)
    assert share.max() <= 1.0, (what, ch, float(share[i]), float(f["err"][i]))
    return f


def _assert_reaches(case, w):
    """What the case is there for, from the twin of the work decomposition (module docstring)."""
    B, S, r, C, shift = case
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if case == CASES[0]:
        assert (w["items"], w["nr"], w["ranges"], w["items"] % 8) == (1, 4, 1, 1) and r == 16 and w["grid"] == 8
    elif case == CASES[1]:
        assert (w["items"], w["nr"], w["ranges"], S // r, shift) == (20, 2, 1, 8, 1)
        if n_cu >= 24:
            assert w["grid"] == 24 and sorted(set(w["per_xcd"])) == [2, 3] and int(w["rounds"].max()) == 0
    else:
        assert w["ranges"] == 2 and w["nr"] == 1 and int(w["rng"].max()) == 1
        assert int(w["rounds"].max()) >= 1, f"{n_cu} CUs take {w['items']} items in one round: no workgroup gets a second item"


def _case_for_device(case):
    """The third case needs a workgroup with two items: grow B until the twin says so for this device's CU count."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B, S, r, C, shift = case
    if case == CASES[2]:
        while int(gbr_work(B, r, 2 * C, n_cu)["rounds"].max()) < 1:
            B += 1
    return (B, S, r, C, shift), gbr_work(B, r, 2 * C, n_cu)


@pytest.mark.parametrize("term", list(TERMS))
@pytest.mark.parametrize("case", CASES, ids=["one-item-nr4", "20-items-nr2", "second-item"])
def test_isolated_terms(ctx, case, term):
    """Each weight piece alone and all of them, through the three transparent epilogues, per channel; on the third case also
    over the second-round items alone.  The main-only and all images also under no_cross (bit-identical to each other, within
    the main-only bound) and the all image with out_mode 5 (fp16 piece bit for bit that of the f16c image)."""
    real, w = _case_for_device(case)
    _assert_reaches(case, w)
    L = _layer(ctx, real)
    tag = f"{real} {term}"
    for mode in ("beta", "gamma 1", "gamma nk"):
        (hi, _, lo8), ref, widen, ref32 = L.term_run(term, mode)
        extra = {}
        if case == CASES[2]:
            later = torch.from_numpy(w["later"]).cuda().repeat_interleave(16, 1).repeat_interleave(16, 2).repeat_interleave(64, 3)
            assert bool(later.any()) and not bool(later.all())
            f2 = gbr_term_figures(torch.where(later, hi + lo8, ref), ref, ref32, widen)
            extra = dict(second_round_share=float((f2["share"] if TIE_RULE else f2["share_wide"]).max()),
                         second_round_items=int((w["rounds"] >= 1).sum()))
        _judge(f"{tag} {mode}", hi + lo8, ref, ref32, widen, case=list(real), term=term, mode=mode, items=int(w["items"]),
               nr=int(w["nr"]), grid=int(w["grid"]), **extra)
    if term == "all":
        # no_cross: the cross pieces are not read
        out, ref, widen, ref32 = L.term_run("all", "gamma nk", no_cross=True, terms=(True, False, False))
        main = L.term_run("main only", "gamma nk", no_cross=True)[0]
        assert torch.equal(torch.stack(main), torch.stack(out)), f"{tag}: no_cross differs between the main-only and the all image"
        _judge(f"{tag} no_cross gamma nk", out[0] + out[2], ref, ref32, widen, case=list(real), term=term, mode="no_cross")
        stream, _, _, bias = L.half_image("all", "gamma")
        hi4 = L.launch(stream, bias)[0]
        hi5 = L.launch(stream, bias, out_mode=5)[0]
        assert torch.equal(hi4, hi5), f"{tag}: the fp16 piece of the f16c6 image differs from the f16c image's"


def test_tie_rule_of_the_fp6_converter(ctx):
    """The isolated cross terms of the first case under every tie rule of the twin: exactly one rule meets the unwidened bound,
    and it is TIE_RULE.  (The tie elements are a code step off under any other rule: tests/test_gbr_terms_host.py.)"""
    from moonsuperresolution_amd import ops
    case = (2, 64, 32, 64, 0)
    shares = {}
    for rule in ops.E2M3_TIE_RULES:
        L = _Layer(ctx, *case, ties=rule)
        assert float((L.tp[2] > 0).double().mean()) > 0.005, "no l6 ties in these inputs"
        for term in ("w_l6 only", "w_h6 only"):
            (hi, _, lo8), ref, widen, ref32 = L.term_run(term, "beta")
            f = gbr_term_figures(hi + lo8, ref, ref32, widen)
            shares[(rule, term)] = (float(f["share"].max()), float(f["share_wide"].max()))
            _record(what=f"tie rule {rule} {term}", case=list(case), share_tight=shares[(rule, term)][0],
                    share_widened=shares[(rule, term)][1], ties_h6=float((L.tp[1] > 0).double().mean()),
                    ties_l6=float((L.tp[2] > 0).double().mean()))
    fits = sorted({r for r in ops.E2M3_TIE_RULES if all(shares[(r, t)][0] <= 1.0 for t in ("w_l6 only", "w_h6 only"))})
    print("tie rules that meet the unwidened bound:", fits, shares)
    assert all(v[1] <= 1.0 for v in shares.values()), shares          # the widened bound holds whatever the rule
    assert fits == [TIE_RULE], (fits, shares)


BLOCK_CHANNELS = (0, 3, 4, 15, 16, 31, 32, 47, 63)


@pytest.mark.parametrize("block", [0, 1])
def test_one_output_channel_at_a_time(ctx, block):
    """Module docstring, "one channel at a time", at (2, 64, 32, 128, 1): two channel blocks in one item, folded up-sample."""
    from moonsuperresolution_amd import ops
    case = (2, 64, 32, 128, 1)
    L = _layer(ctx, case)
    C, r = L.C, L.r
    bias = L.inp["bias"] * 12                       # the whole layer: biases of 3.4 standard deviations of the conv term
    parts = ops.f16c6_weight_decode(L.img)
    stream = ops.gbr_weight_stream(L.img)
    base = torch.stack(L.launch(stream, bias))
    assert torch.equal(torch.stack(L.launch(stream, bias)), base), "two launches on the same operands differ"
    base_nox = torch.stack(L.launch(stream, bias, no_cross=True))

    def ref_of(ch, dtype, wparts=parts, bias_=bias, tp=False, **xkw):
        rg = L.rows_g[ch]
        xs = L.tp if tp else L.xp
        ws = tuple(t.abs() for t in wparts) if tp else wparts
        gam = f16c_terms(xs, tuple(t[:, rg] for t in ws), r, dtype=dtype)
        bet = f16c_terms(xs, tuple(t[:, rg + 32] for t in ws), r, dtype=dtype)
        return gam, bet, bias_[rg], bias_[rg + 32], L.xn(dtype=dtype, ch=ch, **xkw)

    def judge(what, y, ch, **kw):
        g, b, bg, bb, xn = ref_of(ch, torch.float64, **kw)
        wg_, wb_ = ref_of(ch, torch.float64, tp=True, **kw)[:2]
        ref, widen = gbr_spade(g, b, bg, bb, xn, widen=(wg_, wb_))
        ref32 = gbr_spade(*ref_of(ch, torch.float32, **kw))
        return _judge(what, y, ref, ref32, widen, channels=ch, case=list(case))
    allc = list(range(C))
    judge("whole layer, all channels", base[0] + base[2], allc)
    n = 0
    for c in (64 * block + k for k in BLOCK_CHANNELS):
        rg = int(L.rows_g[c])
        changes = []
        for name, row, dl, dh in (("gamma w_l6 scale + 3", rg, 3, 0), ("gamma w_h6 scale - 3", rg, 0, -3),
                                  ("beta w_l6 scale + 3", rg + 32, 3, 0), ("beta w_h6 scale - 3", rg + 32, 0, -3)):
            img2, parts2 = ops.f16c6_shift_wscale(L.img, parts, row, dl, dh)
            s2 = ops.gbr_weight_stream(img2)
            assert torch.equal(torch.stack(L.launch(s2, bias, no_cross=True)), base_nox), f"{name} of channel {c}: no_cross read a scale"
            changes.append((name, dict(stream=s2), dict(wparts=parts2)))
        for name, row in (("gamma bias", rg), ("beta bias", rg + 32)):
            b2 = bias.clone()
            b2[row] = -1.25 * b2[row]
            changes.append((name, dict(bias=b2), dict(bias_=b2)))
        m2, s2_, x2 = L.inp["mean"].clone(), L.inp["std"].clone(), L.inp["x"].clone()
        m2[c] += 0.75
        s2_[c] *= 1.5
        x2[..., c] = 0.5 * x2[..., c] + 1.0
        changes += [("mean", dict(mean=m2), dict(mean=m2)), ("std", dict(std=s2_), dict(std=s2_)), ("x", dict(x=x2), dict(x=x2))]
        for name, rkw, ekw in changes:
            y2 = torch.stack(L.launch(rkw.pop("stream", stream), rkw.pop("bias", bias), **rkw))
            chk = y2.clone()
            chk[..., c] = base[..., c]
            assert torch.equal(chk, base), f"{name}: a channel other than {c} changed"
            assert not torch.equal(y2[0][..., c], base[0][..., c]), f"{name}: channel {c} did not change"
            judge(f"{name} of channel {c}", (y2[0] + y2[2])[..., c:c + 1], [c], **ekw)
            n += 1
    print(f"block {block}: {n} one-channel launches")


@pytest.mark.parametrize("case", CASES[:2], ids=["one-item", "resize-8-seams"])
def test_embedding_read_back(ctx, case):
    """Generic embedding (random 9-tap two-channel we, random be), one-hot beta weights (column n = 1.0 at the centre tap on
    embedding channel n, gamma zero): the output is hi + l6 of e[..., n] itself.  Per element against the float64 chain
    relu(conv(mask)): <= 2^-13 of the pixel's 32-channel block maximum (the f16c6 piece bound of test_gpu_cross_fp6.py) + 2^-14
    of the element (the output image).  Names relu, the zero padding outside the image, the resize offsets across tile seams
    and GBR_PERM per pixel and channel."""
    from moonsuperresolution_amd import ops
    B, S, r, C, shift = case
    g = torch.Generator(device="cpu").manual_seed(1000 * B + r + C)
    src = (torch.rand((B, S, S, 2), generator=g) - 0.5).cuda()
    we = (torch.randn((3, 3, 2, 128), generator=g) / 3).cuda()
    be = (0.1 * torch.randn(128, generator=g)).cuda()
    x = (3 + 2 * torch.randn((B, r >> shift, r >> shift, C), generator=g)).cuda()
    mean, std = x.mean((0, 1, 2)).contiguous(), torch.sqrt(x.var((0, 1, 2), unbiased=False) + 1e-5).contiguous()
    rows_b = spade_rows(C).cuda() + 32
    w = torch.zeros((9, 2 * C, 128), device="cuda")
    n = torch.arange(min(C, 128), device="cuda")
    w[4, rows_b[n], n] = 1.0
    f = S // r
    e = torch.relu(ref_conv(src[:, f // 2::f, f // 2::f][:, :r, :r], we, be, 1)).cuda()
    y = ops.spade_gbr(ctx, src, we, be, ops.gbr_weight_image(w), torch.zeros(2 * C, device="cuda"), r, x, shift, mean, std)
    hi, _, lo8 = (t[:, 1:-1, 1:-1] for t in ops.f16c_decode(y))
    got = (hi + lo8)[..., :128]
    blk = e.reshape(B, r, r, 4, 32).amax(-1, keepdim=True).expand(B, r, r, 4, 32).reshape(e.shape)
    lim = 2.0 ** -13 * blk + 2.0 ** -14 * e
    share = ((got - e).abs() / lim.clamp_min(1e-300))
    i = int(share.argmax())
    idx = np.unravel_index(i, tuple(share.shape))
    _record(what=f"{case} embedding read-back", worst_share=float(share.reshape(-1)[i]), at=[int(k) for k in idx],
            zero_fraction=float((e == 0).double().mean()))
    assert 0.2 < float((e == 0).double().mean()) < 0.8                       # the relu cuts a real share
    assert float((got[e == 0]).abs().max()) == 0, "an element the relu cuts is not zero"
    assert float(share.max()) <= 1.0, (idx, float(got.reshape(-1)[i]), float(e.reshape(-1)[i]))
    if C > 128:
        assert float((hi + lo8)[..., 128:].abs().max()) == 0

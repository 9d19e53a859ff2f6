"""CPU companion of tests/test_gpu_gbr_terms.py: what the whole-tensor bound of the resident SPADE kernel's tests cannot see,
and that the isolated-term check sees it.

The layer is the exact-embedding one (tests.helpers.gbr_exact_inputs) at B = 2, r = 32, C = 64.  The "kernel" is the float64
evaluation of conv_gb_resident's three terms on the operands of ops.gbr_embedding_pieces and the decoded weight image, with a
fault injected into the x_l6 * w_h6 term:
  (a) a pixel's block scale taken from the row below (inside the image: the last row keeps its own),
  (b) tap 8 (the chunk-crossing GB_DSEL == 2 case of csrc/conv_gbr.hip) dropped,
  (c) one chunk's scale off by one binade,
  (d) all cross terms dropped.
Whole layer (gamma and beta, x = 3 + 2 randn normalised, biases of 3.4 standard deviations of the conv term, the proportions of
test_spade_layer_resident_kernel): every fault stays inside rel_linf <= 2e-4 of the whole tensor against the float64 chain, the
bound of that test.  Handed the w_h6 piece alone (beta columns, gamma zero), (a), (b) and (c) put more than half of the
elements of EVERY channel beyond the per-channel bound of the GPU test, tie widening included.  Figures of the committed
seed: see the tests' docstrings."""
import numpy as np
import pytest
import torch

from moonsuperresolution_amd import ops
from tests.helpers import (f16c_terms, gbr_epilogue, gbr_exact_inputs, gbr_spade, gbr_term_figures, gbr_x_parts, pad_hw, ref_conv,
                           rel_linf, spade_rows)

B, S, R, C = 2, 32, 32, 64
N = 2 * C
SEED = 7
LIFT = 12        # binades added to the scale bytes of a cross piece handed over alone (tests/test_gpu_gbr_terms.py)
BIAS_FULL = 12   # the builder's bias is 0.25 of the column scale (the isolated terms' size); the whole layer uses 3.0


@pytest.fixture(scope="module")
def layer():
    return _build_layer(SEED)


def _build_layer(seed):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    inp = gbr_exact_inputs(B, S, R, N, seed)
    order = ops.gbr_channel_order()
    rows_g = spade_rows(C)
    rows_b = rows_g + 32
    img, _ = ops.gbr_weight_perm_image(inp["w"])
    pieces = {t: ops.gbr_embedding_pieces(inp["e"], ties=t) for t in ("even", "odd")}
    xp, tp = gbr_x_parts(pieces["even"], order)

    def wparts(**kw):
        return ops.f16c6_weight_decode(ops.f16c6_weight_keep(img, **kw))
    # the float64 chain of the original operands: what test_spade_layer_resident_kernel compares with
    xn = (inp["x"].double() - inp["mean"].double()) / inp["std"].double()
    gb = ref_conv(inp["e"], inp["w"].permute(0, 2, 1).reshape(3, 3, 128, N), torch.zeros(N), 1)
    bias = inp["bias"].double() * BIAS_FULL
    chain = gbr_spade(gb[..., rows_g], gb[..., rows_b], bias[rows_g], bias[rows_b], xn)
    return dict(inp=inp, order=order, rows_g=rows_g, rows_b=rows_b, pieces=pieces, xp=xp, tp=tp, wparts=wparts, chain=chain, xn=xn,
                bias_full=bias)


def _faulty(layer, fault, wp):
    """(xparts, wparts) of the evaluation with ``fault`` in the x_l6 * w_h6 term."""
    xh, x6, xl = layer["xp"]
    wh, w6, wl = wp
    if fault == "row-shifted scale":
        eb = layer["pieces"]["even"]["eb"]                                    # [B, r, r, 4]
        s = torch.pow(2.0, (eb - 11 - 127).double())
        below = torch.cat([s[:, 1:], s[:, -1:]], 1)                           # the scale of pixel (y + 1, x)
        l6 = layer["pieces"]["even"]["l6"].reshape(B, R, R, 4, 32)
        xl = pad_hw((l6 / s[..., None] * below[..., None]).reshape(B, R, R, 128)[..., layer["order"]])
    elif fault == "tap 8 dropped":
        w6 = w6.clone()
        w6[8] = 0
    elif fault == "chunk binade":
        xl = xl.clone()
        xl[..., 64:96] *= 2
    elif fault == "cross terms dropped":
        x6, xl = torch.zeros_like(x6), torch.zeros_like(xl)
    else:
        assert fault is None
    return (xh, x6, xl), (wh, w6, wl)


FAULTS = ("row-shifted scale", "tap 8 dropped", "chunk binade")


@pytest.mark.parametrize("fault", (None,) + FAULTS + ("cross terms dropped",))
def test_whole_tensor_bound_does_not_see_the_fault(layer, fault):
    """The stated blind spot: with every fault the whole layer stays within 2e-4 of the tensor range of the float64 chain.
    Measured: no fault 9.3e-6; (a) 1.3e-4, (b) 6.6e-5, (c) 8.0e-5, (d) 1.8e-4 of the tensor range, while the worst channel
    moves by 3.1e-4 .. 9.2e-4 of ITS range."""
    xp, wp = _faulty(layer, fault, layer["wparts"]())
    gb = f16c_terms(xp, wp, R)
    b = layer["bias_full"]
    y = gbr_spade(gb[..., layer["rows_g"]], gb[..., layer["rows_b"]], b[layer["rows_g"]], b[layer["rows_b"]], layer["xn"])
    err = rel_linf(y.numpy(), layer["chain"].numpy())
    d = (y - layer["chain"]).abs().reshape(-1, C).amax(0) / layer["chain"].abs().reshape(-1, C).amax(0)
    print(f"fault {fault}: whole layer against the float64 chain {err:.3e} of the tensor range; per channel {float(d.min()):.3e} .. "
          f"{float(d.max()):.3e} of the channel's range")
    assert err <= 2e-4, (fault, err)


def _isolated(layer, kw):
    """Beta columns of the evaluation with the weight pieces of ``kw`` -> (out, tie allowance on out, fp32 evaluation)."""
    rb, bias = layer["rows_b"], layer["inp"]["bias"]
    wp = tuple(t[:, rb] for t in layer["wparts"](**kw))
    wid = f16c_terms(layer["tp"], tuple(t.abs() for t in wp), R)
    out, widen = gbr_epilogue(f16c_terms(layer["xp"], wp, R), rb, bias.double(), widen=wid)
    out32 = gbr_epilogue(f16c_terms(layer["xp"], wp, R, dtype=torch.float32), rb, bias)
    return wp, out, widen, out32


@pytest.mark.parametrize("fault", FAULTS)
def test_isolated_term_sees_the_fault_in_every_channel(layer, fault):
    """The same fault with the w_h6 piece handed over alone: at least half of the elements of every channel lie beyond the
    per-channel bound (2^-14 of the channel range + the fp32 K-length allowance + the tie widening).  Measured: smallest
    per-channel fraction (a) 0.86, (b) 0.60, (c) 0.84; the faults are 25 % or more of the channel range, the widening at most
    13 % of it at a single element."""
    wp, ref, widen, ref32 = _isolated(layer, dict(hi=False, l6=False, lift=LIFT))
    xp, wpf = _faulty(layer, fault, wp)
    y = gbr_epilogue(f16c_terms(xp, wpf, R), layer["rows_b"], layer["inp"]["bias"].double())
    f = gbr_term_figures(y, ref, ref32, widen)
    wide = float((widen.reshape(-1, C).amax(0) / torch.as_tensor(f["range"])).max())
    print(f"fault {fault}: fraction of a channel's elements beyond the bound: min {f['beyond'].min():.3f} (channel "
          f"{int(f['beyond'].argmin())}), median {np.median(f['beyond']):.3f}; per-channel error {f['err'].min():.3f} .. "
          f"{f['err'].max():.3f} of the channel range; largest tie widening {wide:.3f} of the channel range")
    assert f["beyond"].min() >= 0.5, (fault, f["beyond"].min())


TERMS = {"main only": dict(h6=False, l6=False), "w_l6 only": dict(hi=False, h6=False, lift=LIFT),
         "w_h6 only": dict(hi=False, l6=False, lift=LIFT), "all": {}}


@pytest.mark.parametrize("term", ["w_l6 only", "w_h6 only", "all"])
def test_opposite_tie_rule_stays_inside_the_widened_bound(layer, term):
    """The faultless evaluation whose converter takes the OTHER code on every exact midpoint puts no element beyond the widened
    bound, and is beyond the unwidened one in the isolated terms (the widening is needed there unless the converter's rule is
    the twin's)."""
    wp, ref, widen, ref32 = _isolated(layer, TERMS[term])
    xo, _ = gbr_x_parts(layer["pieces"]["odd"], layer["order"])
    y = gbr_epilogue(f16c_terms(xo, wp, R), layer["rows_b"], layer["inp"]["bias"].double())
    f = gbr_term_figures(y, ref, ref32, widen)
    print(f"{term}, opposite tie rule: largest share of the widened bound {f['share_wide'].max():.3f}, of the unwidened one "
          f"{f['share'].max():.1f}")
    assert f["beyond"].max() == 0 and f["share_wide"].max() <= 1.0, (term, f["share_wide"].max())
    if term != "all":
        assert f["share"].min() > 1.0, term
    # the rule itself: the two twins differ exactly on the tie elements, by the recorded distance
    for k, t in (("h6", "tie_h6"), ("l6", "tie_l6")):
        d = (layer["pieces"]["odd"][k] - layer["pieces"]["even"][k]).abs()
        assert torch.equal(d, layer["pieces"]["even"][t]), k
    frac_h, frac_l = (float((layer["pieces"]["even"][t] > 0).double().mean()) for t in ("tie_h6", "tie_l6"))
    assert frac_h < 1e-4 and 0.01 < frac_l < 0.04, (frac_h, frac_l)          # measured 7.6e-6 and 2.2 % of the elements


def test_main_term_has_no_tie_allowance(layer):
    _, _, widen, _ = _isolated(layer, TERMS["main only"])
    assert float(widen.abs().max()) == 0


def test_exact_embedding_and_block_exponent(layer):
    """The embedding of the exact inputs is one exact product (fp32 holds it, any accumulation order gives it), half of it is
    cut by the relu, and the twin of msr_block_e8m0_dev is the smallest power of two >= max / 7.5 except where the fp32
    product with float32(1 / 7.5) rounds across a binade."""
    inp = layer["inp"]
    e64 = torch.relu(ref_conv(inp["mask"][..., None].expand(B, R, R, 2).contiguous() * torch.tensor([1.0, 0.0]), inp["we"], inp["be"], 1))
    assert torch.equal(e64, inp["e"].double())
    assert 0.4 < float((inp["e"] > 0).double().mean()) < 0.6
    eb = layer["pieces"]["even"]["eb"]
    amax = inp["e"].reshape(B, R, R, 4, 32).amax(-1)
    exact = 127 + ops._ceil_log2_over(amax, 7.5)
    assert int((eb - exact).abs().max()) <= 1 and float((eb != exact).double().mean()) <= 0.01
    assert bool((torch.pow(2.0, (eb - 127).double()) * 7.5 * (1 + 2.0 ** -22) >= amax.double()).all())
    assert int(ops.block_e8m0(torch.tensor([0.0, 7.5, 7.5000005, 3.75, 1e-38, 3e38]))[0]) == 127
    assert ops.block_e8m0(torch.tensor([7.5, 15.0, 3.75, 1e-38, 3e38])).tolist() == [127, 128, 126, 27, 247]


def test_work_decomposition_twin_at_256_compute_units():
    """tests.helpers.gbr_ranges / gbr_work (conv_gbr_ranges, the test entries' fall-back to 1, persistent_grid, xcd_tile_range)
    at the three shapes of the GPU test and at the bench shapes the planner takes, for an MI355X's 256 compute units."""
    from tests.helpers import gbr_ranges, gbr_work
    assert gbr_ranges(1, 16, 512) == (0, 1) and gbr_ranges(5, 32, 256) == (0, 1) and gbr_ranges(9, 64, 256) == (2, 2)
    assert gbr_ranges(8, 32, 2048) == (8, 8) and gbr_ranges(8, 64, 128) == (0, 1) and gbr_ranges(8, 24, 256) == (0, 1)
    w = gbr_work(1, 16, 512, 256)
    assert (w["items"], w["nr"], w["grid"], w["slots"], int(w["rounds"].max())) == (1, 4, 8, 1, 0) and not w["later"].any()
    w = gbr_work(5, 32, 256, 256)
    assert (w["items"], w["nr"], w["grid"], w["per_xcd"]) == (20, 2, 24, [3, 3, 3, 3, 2, 2, 2, 2]) and int(w["rounds"].max()) == 0
    w = gbr_work(9, 64, 256, 256)
    assert (w["items"], w["nr"], w["grid"], w["slots"]) == (288, 1, 256, 32) and int((w["rounds"] == 1).sum()) == 32
    assert w["later"].shape == (9, 4, 4, 2) and int(w["later"].sum()) == 32
    # item = range * pixel tiles + pixel tile: the first 144 items are channel block 0 of every tile, XCD x owns items 36 x ..
    assert w["rng"][:144].max() == 0 and w["rng"][144:].min() == 1 and w["tile"][17].tolist() == [1, 0, 1]
    assert sorted(np.nonzero(w["rounds"] == 1)[0][:4].tolist()) == [32, 33, 34, 35]


def _gbr_weight_image_before_the_split(w_kl):
    """ops.gbr_weight_image as it stood before it became gbr_weight_stream(gbr_weight_perm_image(w)): kept to pin its bytes."""
    N = w_kl.shape[1]
    idx = torch.tensor([32 * c + ops.GBR_PERM[e] for c in range(w_kl.shape[2] // 32) for e in range(32)], device=w_kl.device)
    img = ops.f16c6_weight_image(w_kl[:, :, idx].contiguous())[0]
    rec = img.contiguous().view(torch.uint8).reshape(9, N, 4, 128)
    nt, q, P, j, piece, lane = torch.meshgrid(torch.arange(N // 128), torch.arange(4), torch.arange(18), torch.arange(2),
                                              torch.arange(4), torch.arange(64), indexing="ij")
    px, cg = lane & 15, lane >> 4
    row = 128 * nt + 64 * (q >> 1) + 16 * (q & 1) + 32 * j + px
    T = torch.where(piece < 2, 2 * P + piece, 2 * P + (cg >> 1))
    off = torch.where(piece < 2, 16 * cg, 64 + 32 * (cg & 1) + 16 * (piece - 2))
    byte = off[..., None] + torch.arange(16)
    out = rec[(T % 9)[..., None], row[..., None], (T // 9)[..., None], byte]
    return out.contiguous().reshape(-1).view(torch.float32).reshape(9, N, 128)


def test_weight_image_bytes_survive_the_split(layer):
    w = layer["inp"]["w"]
    w = torch.cat([w, w.flip(1) * 0.5], 1)                                   # two channel blocks
    new, old = ops.gbr_weight_image(w), _gbr_weight_image_before_the_split(w)
    assert torch.equal(new.view(torch.int32), old.view(torch.int32))
    img, parts = ops.gbr_weight_perm_image(w)
    assert torch.equal(ops.gbr_weight_stream(img).view(torch.int32), old.view(torch.int32))
    # the stream is a permutation of the image's bytes 0..87 and 96..119 + the 8 bytes behind each piece, every byte once
    tag = torch.arange(img.numel(), dtype=torch.int32).view(torch.float32).reshape(img.shape)
    got = ops.gbr_weight_stream(tag).view(torch.int32).reshape(-1)
    assert got.unique().numel() == got.numel() == img.numel()
    # and keeping every piece changes nothing, dropping one zeroes exactly that piece of the decoded weights
    assert torch.equal(ops.f16c6_weight_keep(img).view(torch.int32), img.view(torch.int32))
    hi, h6, l6 = ops.f16c6_weight_decode(ops.f16c6_weight_keep(img, hi=False, l6=False, lift=LIFT))
    assert float(hi.abs().max()) == 0 and float(l6.abs().max()) == 0 and torch.equal(h6, parts[1] * 2.0 ** LIFT)
    hi, h6, l6 = ops.f16c6_weight_decode(ops.f16c6_weight_keep(img, hi=False, h6=False, lift=LIFT))
    assert float(hi.abs().max()) == 0 and float(h6.abs().max()) == 0 and torch.equal(l6, parts[2] * 2.0 ** LIFT)

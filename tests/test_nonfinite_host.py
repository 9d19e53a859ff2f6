"""CPU: NaN as data (include/moonsr.h "Non-finite inputs"): the checker every kernel-level NaN test uses, the host twins of the
activation images, and what the oracle does with a NaN patch.

tests.helpers.check_nan_contract states four rules for a launch with planted NaN elements (mask, no spread, value, cap).  The
controls below show on a stand-in (a float64 3x3 conv rounded to fp32) that it refuses one dropped NaN, one NaN too many and one
flipped bit outside the footprint, names the element, and passes the clean stand-in.  The host twins
(ops.f16c_activation_image, f16c6_activation_image, bf8_activation_image, split_bf16_host, split_f16) must encode a NaN element
with a NaN main piece and leave every other element's bytes as they are beside a zero.  oracle/generator_ref on a batch with one
whole-NaN ortho channel returns NaN for every sample of the SPADE variants (batch moments) and for that sample alone for pix2pix
(inference BatchNorm is an affine map per element)."""
import numpy as np
import pytest
import torch

from tests.helpers import check_nan_contract, ref_conv, rel_linf

PLANTS = [(0, 0, 0, 0), (0, 15, 16, 37), (1, 7, 7, 63)]       # (b, y, x, c)


def _stand_in(plant=True):
    """A 3x3 SAME conv in float64 (ref) and rounded to fp32 (the "kernel"), with NaN planted (out) or 0.0 in its place (clean)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 32, 32, 64), generator=g)
    w = torch.randn((3, 3, 64, 32), generator=g) / 24
    b = torch.randn(32, generator=g)
    xn, xc = x.clone(), x.clone()
    for p in PLANTS:
        xn[p], xc[p] = float("nan"), 0.0
    ref = ref_conv(xn, w, b, 1)
    return ref.float().numpy(), ref.numpy(), ref_conv(xc, w, b, 1).float().numpy()


def _finite_at(ref):
    return tuple(int(v) for v in np.argwhere(np.isfinite(ref))[5])


def test_checker_passes_the_clean_stand_in():
    out, ref, clean = _stand_in()
    rec = check_nan_contract(out, ref, clean, 1e-6, rel_linf, what="stand-in")
    assert rec["n_nan_ref"] == (4 + 9 + 9) * 32 and rec["n_total"] == ref.size and 0 < rec["worst"] <= 1e-6


def test_checker_names_one_dropped_nan():
    out, ref, clean = _stand_in()
    out[0, 15, 17, 3] = 0.0
    with pytest.raises(AssertionError, match=r"lost NaN at \(0, 15, 17, 3\)"):
        check_nan_contract(out, ref, clean, 1e-6, rel_linf, what="stand-in")
    out, ref, clean = _stand_in()
    out[0, 15, 17, 3] = -65504.0          # what a v_med3_f32 clamp makes of it
    with pytest.raises(AssertionError, match="lost NaN"):
        check_nan_contract(out, ref, clean, 1e-6, rel_linf, what="stand-in")


def test_checker_names_one_nan_too_many():
    out, ref, clean = _stand_in()
    out[1, 20, 20, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"spread NaN at \(1, 20, 20, 5\)"):
        check_nan_contract(out, ref, clean, 1e-6, rel_linf, what="stand-in")


def test_checker_names_one_flipped_bit_outside_the_footprint():
    out, ref, clean = _stand_in()
    at = _finite_at(ref)
    out.view(np.uint32)[at] ^= 1           # one ulp: far inside the value bound
    with pytest.raises(AssertionError, match=rf"changed bits outside the footprint at \({at[0]}, {at[1]}, {at[2]}, {at[3]}\)"):
        check_nan_contract(out, ref, clean, 1e-6, rel_linf, what="stand-in")
    # ... and inside the footprint the clean launch is free to differ
    out, ref, clean = _stand_in()
    clean[0, 0, 0, 0] += 1.0
    check_nan_contract(out, ref, clean, 1e-6, rel_linf, what="stand-in")


def test_checker_raw_storage_value_bound_and_cap():
    out, ref, clean = _stand_in()
    raw_o, raw_c = np.zeros((4, 8), np.uint8), np.zeros((4, 8), np.uint8)
    keep = np.ones((4, 8), bool)
    raw_o[2, 3], keep[2, 3] = 7, False     # a free cross piece may differ
    check_nan_contract(out, ref, clean, 1e-6, rel_linf, raw=(raw_o, raw_c, keep))
    raw_o[1, 1] = 1
    with pytest.raises(AssertionError, match=r"changed stored bits outside the footprint at \(1, 1\)"):
        check_nan_contract(out, ref, clean, 1e-6, rel_linf, raw=(raw_o, raw_c, keep))
    with pytest.raises(AssertionError, match="beyond its bound"):
        check_nan_contract(out, ref, clean, 1e-9, rel_linf)          # fp32 rounding is ~3e-8 of the range
    big, big_c = out.copy(), clean.copy()
    at = _finite_at(ref)
    big[at] += 1.0
    big_c[at] += 1.0                        # same bits as the clean launch, wrong value: rule 3 sees it
    with pytest.raises(AssertionError, match="beyond its bound"):
        check_nan_contract(big, ref, big_c, 1e-6, rel_linf)
    # cap: a reference that is mostly NaN is refused before the output is looked at, unless the case says why
    ref2 = ref.copy()
    ref2[:, :20] = np.nan
    out2 = ref2.astype(np.float32)
    with pytest.raises(AssertionError, match="reference elements are finite"):
        check_nan_contract(np.zeros_like(out2), ref2, clean, 1e-6, rel_linf)
    check_nan_contract(out2, ref2, clean, 1e-6, rel_linf, exempt="whole rows planted")
    with pytest.raises(AssertionError, match="holds no NaN"):
        check_nan_contract(clean, clean.astype(np.float64), clean, 1e-6, rel_linf)


# ---- host twins --------------------------------------------------------------------------------------------------------------------
def _twin_input():
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 5, 5, 64), generator=g) * torch.logspace(-2, 2, 64)
    plants = [(0, 0, 0, 0), (0, 2, 3, 37), (1, 4, 4, 63)]
    xn, xc = x.clone(), x.clone()
    for p in plants:
        xn[p], xc[p] = float("nan"), 0.0
    return xn, xc, plants


def _u8(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[:-1] + (-1,))


def _check_chunks(img_n, img_c, plants, main, piece_bytes):
    """Chunk images (128 bytes per 32 channels): ``main(img)`` decodes the main piece; piece_bytes(c) -> the byte offsets inside
    the chunk that hold channel c.  Planted elements: NaN main piece; every byte that belongs to another element: unchanged."""
    mn = main(img_n)
    want = torch.zeros(mn.shape, dtype=torch.bool)
    for p in plants:
        want[p] = True
    assert torch.equal(torch.isnan(mn), want)
    bn, bc = _u8(img_n), _u8(img_c)
    free = torch.zeros(bn.shape, dtype=torch.bool)
    for (b, y, x, c) in plants:
        for off in piece_bytes(c % 32):
            free[b, y, x, 128 * (c // 32) + off] = True
    assert torch.equal(bn[~free], bc[~free])


def test_f16c_activation_image_keeps_nan_in_hi_and_other_bytes():
    from moonsuperresolution_amd import ops
    xn, xc, plants = _twin_input()
    _check_chunks(ops.f16c_activation_image(xn)[0], ops.f16c_activation_image(xc)[0], plants, lambda i: ops.f16c_decode(i)[0],
                  lambda c: (2 * c, 2 * c + 1, 64 + c, 96 + c))


def test_f16c6_activation_image_keeps_nan_in_hi_and_the_block_scale():
    """The block scale is the maximum over the chunk's FINITE elements: the other 31 channels' codes and both scale bytes are
    those of the chunk with 0.0 in the NaN's place (a NaN maximum used to move the whole chunk's scale)."""
    from moonsuperresolution_amd import ops
    xn, xc, plants = _twin_input()

    def six(c):                      # the bytes that hold bits 6c .. 6c + 5 of a 24-byte code string
        return {(6 * c) // 8, (6 * c + 5) // 8}
    # a 6-bit code shares its bytes with its neighbours' codes: compare the decoded pieces of the other channels instead
    img_n, img_c = ops.f16c6_activation_image(xn)[0], ops.f16c6_activation_image(xc)[0]
    _check_chunks(img_n, img_c, plants, lambda i: ops.f16c6_decode(i)[0],
                  lambda c: {2 * c, 2 * c + 1} | {64 + o for o in six(c)} | {96 + o for o in six(c)})
    dn, dc = ops.f16c6_decode(img_n), ops.f16c6_decode(img_c)
    other = torch.ones(xn.shape, dtype=torch.bool)
    for p in plants:
        other[p] = False
    for a, b in zip(dn, dc):
        assert torch.equal(a[other], b[other])
    assert torch.equal(_u8(img_n)[..., 88::128], _u8(img_c)[..., 88::128]) and torch.equal(_u8(img_n)[..., 120::128], _u8(img_c)[..., 120::128])


def test_bf8_and_split_images_keep_nan_in_the_main_piece():
    from moonsuperresolution_amd import ops
    xn, xc, plants = _twin_input()
    want = torch.isnan(xn)
    bn, bc = ops.bf8_activation_image(xn)[0], ops.bf8_activation_image(xc)[0]
    assert torch.equal(torch.isnan(bn[..., :64].view(torch.float8_e5m2).float()), want)
    assert torch.equal(bn[..., :64][~want], bc[..., :64][~want]) and int(bn[..., 64:].max()) == 0
    for fn, dt in ((ops.split_bf16_host, torch.bfloat16), (ops.split_f16, torch.float16)):
        hn = fn(xn).contiguous().view(torch.int16).reshape(-1, 2, 32)
        hc = fn(xc).contiguous().view(torch.int16).reshape(-1, 2, 32)
        hi = hn[:, 0].contiguous().view(dt).float().reshape(xn.shape)
        assert torch.equal(torch.isnan(hi), want)
        keep = ~want.reshape(-1, 1, 32).expand(-1, 2, -1)
        assert torch.equal(hn[keep], hc[keep])


_BF16_PROGRAM = r"""
#include "kernels.h"
#include <cstdio>
#include <cstring>
int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        unsigned u = (unsigned)std::strtoul(argv[i], nullptr, 16), hi, lo;
        float f;
        std::memcpy(&f, &u, 4);
        msr::msr_split_bf16(f, hi, lo);
        std::printf("%08x %04x %04x\n", u, msr::msr_bf16_rn(f), hi);
    }
    return 0;
}
"""


def test_msr_bf16_rn_keeps_every_nan_payload(tmp_path):
    """csrc/kernels.h msr_bf16_rn itself (host side of the bf16x3 weight upload, and the split-bf16 SPADE epilogue), in a small
    stand-alone program: the rounding increment alone carried a low NaN payload into the exponent or the sign (0x7f800001 ->
    infinity, 0x7fffffff -> -0); every NaN must stay a NaN of its sign, in msr_bf16_rn and in the hi word of msr_split_bf16, and
    finite values and infinities must round as torch's bfloat16 does."""
    import os
    import re
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moonsuperresolution_amd", "csrc")
    hipcc = re.search(r"^HIPCC\s*\??=\s*(\S+)", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1)
    src, exe = tmp_path / "bf16_rn.hip", tmp_path / "bf16_rn"
    src.write_text(_BF16_PROGRAM)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", csrc, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    nans = [0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFFFFFFFF, 0xFF800001, 0x7F80FFFF, 0x7F808000]
    rng = np.random.default_rng(0)
    vals = np.concatenate([rng.standard_normal(256).astype(np.float32) * 1e3, np.array([np.inf, -np.inf, 0.0, -0.0, 3.3895314e38, 1e-40], np.float32)])
    words = nans + [int(u) for u in vals.view(np.uint32)]
    out = subprocess.run([str(exe)] + [f"{u:08x}" for u in words], capture_output=True, text=True, check=True).stdout.split()
    got = {int(out[3 * k], 16): (int(out[3 * k + 1], 16), int(out[3 * k + 2], 16)) for k in range(len(words))}
    for u in nans:
        for h in got[u]:
            assert (h & 0x7FFF) > 0x7F80 and (h >> 15) == (u >> 31), f"{u:#010x} -> {h:#06x}"
    want = torch.from_numpy(vals).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    for u, wbits in zip(vals.view(np.uint32), want):
        assert got[int(u)] == (int(wbits), int(wbits)), f"{int(u):#010x}"


# ---- oracle masks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["gaugan", "gaugan_no_kl", "cnn"])
def test_oracle_spade_variants_spread_a_nan_sample_over_the_batch(variant):
    """One sample's ortho channel all NaN: its latent is NaN, the dense layer makes its x NaN, and the first SPADE's batch
    moments (mean over N, H, W) hand the NaN to every sample."""
    from moonsuperresolution_amd import make_latent_noise, make_weights, synthetic_patches
    from oracle import generator_ref as G
    x = synthetic_patches(3, 64, 0)
    x[1, :, :, 0] = np.nan
    y = G.spade_call(x, make_weights(variant, 64, seed=1234, bias_scale=0.05), variant,
                     make_latent_noise(3, 256, 7) if variant == "gaugan" else None, dtype=torch.float32)
    assert np.isnan(y).all()


def test_oracle_pix2pix_keeps_a_nan_sample_to_itself():
    from moonsuperresolution_amd import make_weights, synthetic_patches
    from oracle import generator_ref as G
    x = synthetic_patches(2, 256, 3)
    x[0, :, :, 0] = np.nan
    w = make_weights("pix2pix", 256, seed=1234, bias_scale=0.05)
    y = G.pix2pix_call(x, w, dtype=torch.float32)
    assert np.isnan(y[0]).all() and np.isfinite(y[1]).all()
    clean = x.copy()
    clean[0, :, :, 0] = 0.0
    assert np.array_equal(y[1], G.pix2pix_call(clean, w, dtype=torch.float32)[1])


@pytest.mark.parametrize("precision", ["f16c", "f16"])
def test_smallest_shape_with_resident_and_stream_kernels(precision):
    """The shape of tests/test_gpu_nonfinite.py::test_generator_large_kernels_nan_sample, from the form table (csrc/forms.hip
    conv_gbr_ranges, conv_kernel_for): (128, 9) has a conv_gb_resident layer and a stream-kernel conv, and no configuration
    with fewer pixels per call has both ((256, 3), the next, has a third more; the issue's guess (256, 8) has both too)."""
    from moonsuperresolution_amd import _lib
    from moonsuperresolution_amd.generator import form_table

    def both(S, B):
        t = form_table(S, B, "gaugan_no_kl", _lib.PRECISION_FLAGS[precision])
        rows = [v for v in t.values() if isinstance(v, dict)]
        return any(v.get("gbr") == 1 for v in rows) and any(v.get("kernel") == "sw" for v in rows)
    assert both(128, 9) and both(256, 3) and both(256, 8)
    for S in (64, 128, 256):
        for B in range(1, 17):
            if B * S * S < 9 * 128 * 128:
                assert not both(S, B), (S, B)

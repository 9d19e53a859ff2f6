"""CPU: why the conv kernels are checked per output channel (tests/test_gpu_conv_channels.py), shown on a stand-in.

Every conv parity statement of tests/test_gpu_conv_kernel.py is tests.helpers.rel_linf: the largest error anywhere over the
largest reference value anywhere.  With weights spanning three decades over the output channels the denominator comes from the few
largest channels, and a fault in ONE smaller channel of an f16c kernel (a cross term left out, a scale byte of another channel,
the bias of its neighbour) stays below the bounds.  Here the "kernel" is a stand-in: plain fp32 accumulation of the f16c terms
x_hi * w_hi + x_h8 * w_lo8 + x_lo8 * w_h8 on the de-quantised operands that ops.f16c_activation_image / ops.f16c_weight_image
return, with one fault injected into one channel.  The tests state
  (a) tests.helpers.rel_linf_per_channel (per channel: max error over pixels / max reference over pixels) exceeds BOUND in the
      faulted channels and only there;
  (b) the clean stand-in stays under BOUND in every channel: the inputs are such that the reference alone passes;
  (c) at least one of the faults, per shape, satisfies the two whole-tensor asserts of test_conv_f16c (5e-5 against the kernel's
      own terms, 2e-4 against the float64 conv): the recorded reason for the per-channel metric;
Margins of (a), measured: a dropped cross term 1.3e-4 to 2.4e-4, a scale 3 binades off 1.2e-4 to 1.7e-3, the neighbour's bias
3e-2 or more; the smallest is the swap with channel c ^ 16, whose scale bytes differ by ONE binade when they differ at all (the
channels are a factor 1.5 apart): the channel handed the smaller scale keeps half of a ~1.3e-4 cross term, 6.4e-5 to 1.4e-4
against the bound's 5e-5.  The inputs are seeded, so these figures do not move from run to run.
The tests also state that the host twins ops.*_shift_* ("the kernel was handed this scale") agree exactly with decoding the shifted image."""
import numpy as np
import pytest
import torch

from tests.helpers import (_ref_f16c, conv_channel_inputs, conv_walk_item, f16c_terms, later_round_mask, persistent_item_rounds,
                           ref_conv, rel_linf, rel_linf_per_channel)

BOUND = 5e-5                 # tests/test_gpu_conv_channels.py: the "exact up to accumulation" bound, per channel
OLD_EMU, OLD_TRUE = 5e-5, 2e-4   # test_conv_f16c's whole-tensor bounds
SHAPES = [(2, 16, 64, 256), (1, 16, 128, 256), (1, 16, 256, 256)]


def _faults(wexp, wparts, bias, c, cout):
    """name -> (wparts', bias', faulted channels) for every fault injected at channel c."""
    from moonsuperresolution_amd import ops
    wh, w8, wl = wparts

    def zero(t):
        t = t.clone()
        t[:, c] = 0
        return t

    out = {"both cross terms dropped": ((wh, zero(w8), zero(wl)), bias, {c}),
           "x_h8 * w_lo8 dropped": ((wh, w8, zero(wl)), bias, {c}),
           "x_lo8 * w_h8 dropped": ((wh, zero(w8), wl), bias, {c})}
    for name, (dl, dh) in {"lo scale +3": (3, 0), "lo scale -3": (-3, 0), "hi scale +3": (0, 3), "hi scale -3": (0, -3)}.items():
        out[name] = (ops.f16c_shift_wexp(wexp, wparts, c, dl, dh)[1], bias, {c})
    nb = c + 1 if c + 1 < cout else c - 1
    b2 = bias.clone()
    b2[c] = bias[nb]
    out["bias of the neighbouring channel"] = (wparts, b2, {c})
    for name, o in (("scales swapped with c ^ 16", c ^ 16), ("scales swapped with c + 128", (c + 128) % cout)):
        e = wexp.to(torch.int64)
        parts, hit = wparts, set()
        for a, b in ((c, o), (o, c)):        # channel a is handed channel b's two bytes
            dl, dh = int((e[b] & 255) - (e[a] & 255)), int(((e[b] >> 8) & 255) - ((e[a] >> 8) & 255))
            parts = ops.f16c_shift_wexp(wexp, parts, a, dl, dh)[1]
            if dl or dh:
                hit.add(a)
        out[name] = (parts, bias, hit)
    return out


@pytest.mark.parametrize("B,r,cin,cout", SHAPES)
def test_per_channel_metric_sees_one_channel_faults_the_whole_tensor_metric_does_not(B, r, cin, cout):
    from moonsuperresolution_amd import ops
    x, w, b, _ = conv_channel_inputs(B, r, cin, cout, seed=900 + cin)
    _, xparts = ops.f16c_activation_image(ops.pad_nhwc(x))
    _, wexp, wparts = ops.f16c_weight_image(ops.kernel_layout(w))
    emu = _ref_f16c(tuple(t[:, 1:-1, 1:-1] for t in xparts), wparts, b, cin, cout)          # float64, the kernel's own terms
    true = ref_conv(x, w, b, 1)
    standin = lambda wp, bias: (f16c_terms(xparts, wp, r, dtype=torch.float32) + bias.float())   # noqa: E731

    clean = rel_linf_per_channel(standin(wparts, b), emu)
    print(f"clean stand-in ({B}, {r}, {cin}, {cout}): worst channel {clean.max():.2e} at {clean.argmax()}, "
          f"rel_linf {rel_linf(standin(wparts, b).numpy(), emu.numpy()):.2e}")
    assert clean.max() <= BOUND, (clean.max(), clean.argmax())                               # (b)

    blind, swapped16 = [], 0
    for c in (0, cout // 2, cout - 1):
        for name, (wp, bias, hit) in _faults(wexp, wparts, b, c, cout).items():
            y = standin(wp, bias)
            e = rel_linf_per_channel(y, emu)
            others = np.delete(e, sorted(hit))
            print(f"  channel {c:3d} {name:34s} faulted {sorted(hit)}: {[float(f'{e[h]:.2e}') for h in sorted(hit)]}, "
                  f"others <= {others.max():.2e}")
            if name == "scales swapped with c ^ 16":
                swapped16 += len(hit)
            else:
                assert hit, (c, name)
            for h in hit:
                assert e[h] > BOUND, (c, name, h, e[h])                                      # (a) seen where it is ...
            assert others.max() <= BOUND, (c, name, others.max())                            # ... and only there
            if hit and rel_linf(y.numpy(), emu.numpy()) <= OLD_EMU and rel_linf(y.numpy(), true.numpy()) <= OLD_TRUE:
                blind.append((c, name))
    assert swapped16, "no channel pair 16 apart has different scale bytes: the swap fault was never injected"
    print(f"  pass both whole-tensor asserts of test_conv_f16c: {len(blind)} of the faults, e.g. {blind[:3]}")
    assert blind                                                                             # (c)


def test_rel_linf_per_channel_reports_a_zero_reference_channel():
    b = np.zeros((4, 3))
    b[:, 0] = [1, -2, 0.5, 0]
    b[:, 2] = 4
    a = b.copy()
    a[1, 0] += 0.5
    e = rel_linf_per_channel(a, b)
    assert e.tolist() == [0.25, 0.0, 0.0]
    a[2, 1] = 1e-30
    assert rel_linf_per_channel(a, b)[1] == np.inf           # nothing hides a channel that should be zero
    assert rel_linf_per_channel(torch.from_numpy(a), torch.from_numpy(b))[0] == 0.25


@pytest.mark.parametrize("channel", [0, 77, 255])
def test_shift_twins_equal_the_decoded_shifted_images(channel):
    """ops.f16c_shift_wexp / f16c6_shift_wscale / fp8_shift_wexp return the parts a decoder reads out of the shifted image,
    exactly; only ``channel`` changes, by exactly 2^d; every shifted byte is a finite e8m0 exponent."""
    from moonsuperresolution_amd import ops
    _, w, _, _ = conv_channel_inputs(1, 16, 128, 256, seed=7)
    wk = ops.kernel_layout(w)
    rest = torch.arange(256) != channel
    same = lambda p, q: all(torch.equal(a, b) for a, b in zip(p, q))   # noqa: E731

    wimg, wexp, wparts = ops.f16c_weight_image(wk)
    assert same(ops.f16c_weight_decode(wimg, wexp), wparts)
    for dl, dh in ((3, 0), (0, -3), (-3, 3)):
        e2, p2 = ops.f16c_shift_wexp(wexp, wparts, channel, dl, dh)
        assert same(ops.f16c_weight_decode(wimg, e2), p2)
        assert torch.equal(e2[rest], wexp[rest]) and int(e2[channel]) == int(wexp[channel]) + dl + 256 * dh
        assert torch.equal(p2[1][:, channel], wparts[1][:, channel] * 2.0 ** dh) and torch.equal(p2[0], wparts[0])
        assert torch.equal(p2[2][:, channel], wparts[2][:, channel] * 2.0 ** dl) and same([t[:, rest] for t in p2], [t[:, rest] for t in wparts])

    img6, parts6 = ops.f16c6_weight_image(wk)
    assert same(ops.f16c6_weight_decode(img6), parts6)
    for dl, dh in ((3, 0), (0, -3), (-3, 3)):
        i2, p2 = ops.f16c6_shift_wscale(img6, parts6, channel, dl, dh)
        assert same(ops.f16c6_weight_decode(i2), p2)
        by, by2 = (t.contiguous().view(torch.uint8).reshape(9, 256, 4, 128).int() for t in (img6, i2))
        d = by2 - by
        assert int(d[:, rest].abs().max()) == 0 and bool((d[:, channel, :, 88] == dl).all()) and bool((d[:, channel, :, 120] == dh).all())
        d[:, channel, :, 88] = 0
        d[:, channel, :, 120] = 0
        assert int(d.abs().max()) == 0
        assert torch.equal(p2[1][:, channel], parts6[1][:, channel] * 2.0 ** dh) and torch.equal(p2[2][:, channel], parts6[2][:, channel] * 2.0 ** dl)

    img8, wexp8, wdq = ops.fp8_weight_image(wk)
    assert torch.equal(ops.fp8_weight_decode(img8, wexp8, 128), wdq.double())
    for d in (3, -3):
        e2, q2 = ops.fp8_shift_wexp(wexp8, wdq, channel, d)
        assert torch.equal(ops.fp8_weight_decode(img8, e2, 128), q2.double())
        assert torch.equal(e2[rest], wexp8[rest]) and int(e2[channel]) == int(wexp8[channel]) + d * 0x01010101
        assert torch.equal(q2[:, channel], wdq[:, channel] * 2.0 ** d) and torch.equal(q2[:, rest], wdq[:, rest])
    with pytest.raises(ValueError):
        ops.fp8_shift_wexp(wexp8, wdq, channel, 200)


def test_persistent_walk_restatement():
    """tests.helpers.persistent_item_rounds / conv_walk_item (what the GPU tests pick their second-round items with): every item
    is taken once; with more items than workgroups exactly items - grid of them are taken in a later round."""
    for items, n_cu in ((4, 256), (64, 256), (320, 256), (288, 256), (320, 304), (1000, 256)):
        sr = persistent_item_rounds(items, n_cu)
        grid = min((items + 7) & ~7, n_cu & ~7)
        assert int((sr[:, 1] >= 1).sum()) == max(items - grid, 0)
        assert sr[:, 0].max() < grid // 8
    for tiles_m, tiles_n in ((80, 4), (96, 3), (64, 8), (7, 8)):
        seen = {conv_walk_item(t, tiles_m, tiles_n) for t in range(tiles_m * tiles_n)}
        assert seen == {(n, m) for n in range(tiles_n) for m in range(tiles_m)}
    m = later_round_mask(5, 64, 512, 256)
    assert m.shape == (5, 4, 4, 4) and int(m.sum()) == 64 and m.any((0, 1, 2)).all()      # every channel block has such an item
    # ... but at that shape a workgroup's second item (32 items on, 4 channel blocks) is in the channel block of its first;
    # with 3 channel blocks every second item is in another one
    assert int(later_round_mask(5, 64, 512, 256, new_block=True).sum()) == 0
    m = later_round_mask(6, 64, 384, 256, new_block=True)
    assert int(m.sum()) == 32 == int(later_round_mask(6, 64, 384, 256).sum()) and m.any((0, 1, 2)).all()

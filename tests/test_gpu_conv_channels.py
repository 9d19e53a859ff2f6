"""GPU (-m gpu): the f16c / f16c6 / fp8 conv kernels checked per OUTPUT CHANNEL: scales, bias and cross terms.

tests/test_gpu_conv_kernel.py states every conv parity as rel_linf (largest error / largest reference value of the whole tensor);
with weights spanning three decades over the output channels a fault in one small channel stays below its bounds
(tests/test_conv_channels_host.py shows it on a stand-in).  Here every launch is checked two ways:

  (i)  value: tests.helpers.rel_linf_per_channel(y, emu) <= BOUND = 5e-5 in EVERY channel, emu = the float64 evaluation of the
       kernel's own terms on the decoded operands (the "exact up to accumulation" bound of test_conv_f16c, test_conv_f16c6 and
       test_conv_fp8_exact_on_quantised_operands, applied to each channel against its own magnitude; the bias is scaled like its
       channel so that a channel's magnitude is set by its own weights).  Should a correct kernel exceed it in a channel, the
       project's K-length allowance applies there: 4 x the per-channel error of the same terms accumulated in plain fp32 by
       torch (no case needed it, see the figures below);
  (ii) one-hot sensitivity: the launch is repeated (equal bits), then the operands of ONE output channel c are changed (its w_lo
       scale byte + 3 binades, its w_hi byte - 3, its bias, its residual / SPADE operands) and the launch must leave every other
       channel bit-identical, change channel c, and satisfy (i) in c against the emulation with the same change
       (ops.f16c_shift_wexp and its f16c6 / fp8 twins are "the kernel was handed this scale").  Under no_cross both scale changes
       must leave the WHOLE tensor bit-identical: the mode does not compute the cross products.

Channels: one per wave / j / lane-group class of the kernels' scale index expressions (conv_pp.hip: n0 + wn * 64 + j * 16 +
(lane & 15); conv_sw.hip: n0 + (wq >> 1) * 64 + (wq & 1) * 16 + 32 * j + px): 0, 15, 16, 47, 64, 127, the second 128-channel
tile (128 + 33, N - 1); for SPADE a channel in each 32-block of a 64-row (gamma | beta) group of both tiles.

Cases (B, r, Cin, N); figures below measured on an MI355X, one whole run kept in profiles/conv_channels_parity.jsonl:
  A  f16c ping-pong kernel, whole tiles, bias                  (2, 16, 64, 256)    Cin % 128 != 0: never a stream-kernel shape
  B  f16c stream kernel: bias, residual shift 0 / 1, no_cross  (2, 16, 128, 256)
  C  f16c K ranges + split-K pass, bias / residual             (1, 16, 256, 256), ks = 2, 4 (bias and skip indexing: conv_splitk.hip)
  D  f16c gamma | beta conv + SPADE epilogue, ks = 1, 2         (2, 16, 128, N = 512), x at shift 0 / 1; out_modes 4, 5: one-hot on hi
  E  f16c6 stream kernel, bias / residual                      (1, 32, 128, 256)   scale bytes inside the weight image
  F  fp8 ping-pong kernel, bias                                (2, 16, 128, 256) and (6, 64, 128, 384), see test_fp8_*
  G  second tile of a persistent workgroup                     (5, 64, 128, 512): 320 items on one workgroup per CU, second tile in
     the first one's channel block; (6, 64, 128, 384): 288 items, second tile in ANOTHER channel block (scales, bias re-read)
Worst per-channel error of (i) over the base launch and every perturbed one (the bound is 5e-5; the fp32 stand-in of
tests/test_conv_channels_host.py gives 2.6e-7 to 4.8e-7; the smallest fault it injects, 6.4e-5):
  A 6.6e-7 | B bias 9.4e-7, residual 6.7e-7 / 6.5e-7, no_cross 6.5e-7 / 5.2e-7 | C ks = 2: 7.5e-7 / 6.3e-7, ks = 4: 4.5e-7 / 3.7e-7
  D x shift 0 / 1: ks = 1 1.8e-6 / 2.1e-6, ks = 2 1.0e-6 / 8.7e-7 | E 4.8e-7 / 3.2e-7
  G (5, 64, 128, 512) 1.0e-6 (second-round items 8.1e-7) / 7.8e-7; (6, 64, 128, 384) 1.1e-6 / 7.9e-7 (over the 32 items in another
    channel block than the workgroup's first: 8.4e-7 / 7.1e-7)
  F 2.8e-5 at (2, 16, 128, 256), 2.2e-5 at (6, 64, 128, 384) (1.7e-5 over the items B with re-read scales): the scaled fp8 MFMA is
    the one form that comes within a factor two of the bound, as it does whole-tensor in test_conv_fp8_exact_on_quantised_operands.
  MSR_F16C_SW = 0 / 2 (child runs): every f16c case reports the figure and the channel of the default dispatch, digit for digit,
    although the other kernel runs (case B on conv_igemm_bf16x3_pp<EPI_BIAS, PP_F16C> under 0, case D on conv_igemm_f16c_sw<EPI_SPADE>
    under 2, seen in a kernel trace): both kernels add a channel's products in the same order.  Every f16c test therefore asks the
    library which kernel its launch goes to (msr_debug_f16c_kernel: conv_kernel_for, the rule that names a form's kernel), checks the answer against the
    meaning of the mode, and the child-run test requires the answers the mode stands for.
No case needed the fp32-evaluation allowance.

The f16c tests follow the process's MSR_F16C_SW (read once); test_f16c_cases_under_the_other_kernel_dispatch reruns them in a child
process under MSR_F16C_SW = 0 (everything on the ping-pong kernel) and = 2 (everything with Cin % 128 == 0 on the stream kernel).
A form the selected kernel does not have is refused by the entry (ValueError) and skipped per case, explicitly.  Cases skipped:
none under either mode: the rule names the other kernel for a launch the selected kernel has no form for (A: Cin = 64, always
ping-pong; C and D with ks > 1: always ping-pong K ranges + split-K pass; D out_mode 5: always ping-pong; no_cross and f16c6:
always the stream kernel), so under each mode every one of A, B, C, D and G runs, which the child-run test asserts."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import (conv_taps, conv_walk_item, f16c_terms, later_round_mask, persistent_item_rounds, record_dir as _record_dir,
                           rel_linf_per_channel)

pytestmark = pytest.mark.gpu
BOUND = 5e-5
SW_MODE = os.environ.get("MSR_F16C_SW", "1")


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert torch.cuda.is_available()
    from moonsuperresolution_amd import ops
    c = ops.OpContext()
    yield c
    c.close()


def _record(**kw):
    kw["MSR_F16C_SW"] = SW_MODE
    try:
        os.makedirs(_record_dir(), exist_ok=True)
        with open(os.path.join(_record_dir(), "parity_conv_channels.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")
    except OSError:
        pass
    print("conv channels", kw)


def _launch(fn, what):
    """A launch whose form the kernel selected by MSR_F16C_SW does not have is refused by the entry: skip that case, by name."""
    try:
        return fn()
    except ValueError as e:
        if SW_MODE in ("0", "2"):
            pytest.skip(f"{what}: no form under MSR_F16C_SW={SW_MODE} ({e})")
        raise


def _kernel(ctx, cin, epi, out_mode=0, ks=1, direct=False):
    """Which kernel a msr_op_conv3x3_f16c launch runs in this process: the library's own answer (msr_debug_f16c_kernel, the
    rule conv_kernel_for of csrc/forms.hip) for whole-tile launches, checked against the documented meaning of MSR_F16C_SW (1: bias /
    residual launches with Cin % 128 == 0 on the stream kernel; 0: nothing; 2: everything with Cin % 128 == 0 but the f16c6
    image output).  K ranges always run the ping-pong kernel, no_cross and f16c6 launches (``direct``) always the stream kernel."""
    if direct:
        return "stream"
    if ks > 1:
        return "ping-pong"
    want = cin % 128 == 0 and not (epi == 2 and out_mode == 5) and (SW_MODE == "2" or (SW_MODE == "1" and epi != 2))
    got = ctx.lib.msr_debug_f16c_kernel(cin, epi, out_mode)
    assert got == int(want), f"MSR_F16C_SW={SW_MODE}: the library sends cin={cin} epi={epi} out_mode={out_mode} to kernel {got}"
    return "stream" if got else "ping-pong"


class _Tally:
    """Worst per-channel figure of one case over its base launch and every perturbed one; which channels needed the allowance."""

    def __init__(self, case):
        self.case, self.worst, self.channel, self.what, self.allowed, self.launches = case, 0.0, -1, "", [], 0
        self.kernel = None

    def value(self, y, emu, channels, what, f32_fn):
        """(i) for the channels of ``y`` / ``emu`` (last dimension), numbered ``channels``; f32_fn() -> the same terms in plain
        fp32 (called only if a channel exceeds BOUND: the K-length allowance, 4 x its per-channel error against ``emu``)."""
        e = rel_linf_per_channel(y, emu)
        self.launches += 1
        i = int(e.argmax())
        if e[i] > self.worst:
            self.worst, self.channel, self.what = float(e[i]), int(channels[i]), what
        if e.max() > BOUND:
            lim = np.maximum(BOUND, 4 * rel_linf_per_channel(f32_fn(), emu))
            bad = np.nonzero(e > lim)[0]
            self.allowed += [int(channels[k]) for k in np.nonzero(e > BOUND)[0]]
            assert bad.size == 0, (self.case, what, [(int(channels[k]), float(e[k]), float(lim[k])) for k in bad[:8]])
        return e

    def done(self, **kw):
        print(f"{self.case}: worst channel {self.channel} ({self.what}): {self.worst:.3e} over {self.launches} launches")
        print(f"dispatch: case {self.case[0]} under MSR_F16C_SW={SW_MODE} ran the {self.kernel} kernel")
        _record(case=self.case, kernel=self.kernel, worst=self.worst, channel=self.channel, at=self.what, launches=self.launches,
                allowance_channels=sorted(set(self.allowed)), bound=BOUND, **kw)


def _one_hot(tally, base, y2, c, emu_c, what, f32_fn, subsets=()):
    """(ii) for one perturbed launch: every other channel bit-identical to ``base``, channel c changed (inside every pixel
    subset given too) and within (i) of ``emu_c`` [..., 1]."""
    chk = y2.clone()
    chk[..., c] = base[..., c]
    assert torch.equal(chk, base), f"{tally.case} {what}: a channel other than {c} changed"
    assert not torch.equal(y2[..., c], base[..., c]), f"{tally.case} {what}: channel {c} did not change"
    for name, m in subsets:
        assert not torch.equal(y2[..., c][m], base[..., c][m]), f"{tally.case} {what}: channel {c} did not change in {name}"
    tally.value(y2[..., c:c + 1], emu_c, [c], f"{what} of channel {c}", f32_fn)


def _up(t, shift):
    return t.repeat_interleave(1 << shift, 1).repeat_interleave(1 << shift, 2) if shift else t


# ---- bias / residual launches: cases A, B, C, E, G ---------------------------------------------------------------------------------
class _Conv:
    """One bias / residual conv of the f16c family on the per-channel inputs (tests.helpers.conv_channel_inputs)."""

    def __init__(self, ctx, B, r, cin, cout, res, f6=False, ks=1, no_cross=False):
        from moonsuperresolution_amd import ops
        from tests.helpers import conv_channel_inputs
        self.ctx, self.r, self.res, self.f6, self.ks, self.nox = ctx, r, res, f6, ks, no_cross
        x, w, b, skip = conv_channel_inputs(B, r, cin, cout, seed=51 + B + r + cin, res=res, x_decades=(-1.5, 0.5) if f6 else None)
        self.b, self.skip = b.cuda(), skip.cuda() if skip is not None else None
        wk = ops.kernel_layout(w.cuda())
        if f6:
            self.ximg, self.xparts = ops.f16c6_activation_image(ops.pad_nhwc(x.cuda()))
            self.wimg, self.wparts = ops.f16c6_weight_image(wk)
            self.wexp = None
        else:
            self.ximg, self.xparts = ops.f16c_activation_image(ops.pad_nhwc(x.cuda()))
            self.wimg, self.wexp, self.wparts = ops.f16c_weight_image(wk)
        self.terms = (True, False, False) if no_cross else (True, True, True)

    def run(self, wexp=None, wimg=None, b=None, skip=None):
        from moonsuperresolution_amd import ops
        skip = self.skip if skip is None else skip
        return ops.conv3x3_f16c(self.ctx, self.ximg, self.wimg if wimg is None else wimg, self.wexp if wexp is None else wexp,
                                self.b if b is None else b, self.r, epilogue=ops.EPI_BIAS if self.res is None else ops.EPI_RES,
                                aux=skip, aux_shift=self.res or 0, ksplit=self.ks, no_cross=self.nox)

    def emu(self, ch=None, wparts=None, b=None, skip=None, dtype=torch.float64):
        """The kernel's own terms on the decoded operands (+ bias, + residual) for channels ``ch`` (default: all)."""
        ch = slice(None) if ch is None else ch
        wparts, b = self.wparts if wparts is None else wparts, self.b if b is None else b
        y = f16c_terms(self.xparts, tuple(t[:, ch] for t in wparts), self.r, dtype=dtype, terms=self.terms) + b[ch].to(dtype)
        if self.res is not None:
            y = y + _up(self.skip if skip is None else skip, self.res)[..., ch].to(dtype)
        return y

    def shifted(self, c, d_lo, d_hi):
        """-> (run kwargs, wparts) with the scales of channel c moved."""
        from moonsuperresolution_amd import ops
        if self.f6:
            img, parts = ops.f16c6_shift_wscale(self.wimg, self.wparts, c, d_lo, d_hi)
            return dict(wimg=img), parts
        e, parts = ops.f16c_shift_wexp(self.wexp, self.wparts, c, d_lo, d_hi)
        return dict(wexp=e), parts


def _check_conv(cv, case, channels, subsets_of=None):
    """(i) on the base launch, run-to-run bits, then (ii) for every channel of ``channels`` and every perturbation of the form."""
    tally = _Tally(case)
    tally.kernel = _kernel(cv.ctx, cv.ximg.shape[3], 0 if cv.res is None else 1, ks=cv.ks, direct=cv.f6 or cv.nox)
    N = cv.b.numel()
    base = _launch(cv.run, case)
    assert torch.equal(cv.run(), base), f"{case}: two launches on the same operands differ"
    emu = cv.emu()
    e = tally.value(base, emu, np.arange(N), "unperturbed", lambda: cv.emu(dtype=torch.float32))
    print(f"{case}: unperturbed worst channel {int(e.argmax())}: {e.max():.3e} (median {np.median(e):.3e})")
    for c in (c % N for c in channels):
        sub = subsets_of(c) if subsets_of else ()
        for name, (dl, dh) in (("w_lo scale byte + 3", (3, 0)), ("w_hi scale byte - 3", (0, -3))):
            kw, parts = cv.shifted(c, dl, dh)
            y2 = cv.run(**kw)
            if cv.nox:
                assert torch.equal(y2, base), f"{case} {name} of channel {c}: the no-cross form read a cross-term scale"
                continue
            _one_hot(tally, base, y2, c, cv.emu([c], wparts=parts), name, lambda: cv.emu([c], wparts=parts, dtype=torch.float32), sub)
        b2 = cv.b.clone()
        b2[c] = cv.b[c + 1 if c + 1 < N else c - 1] * 1.25
        _one_hot(tally, base, cv.run(b=b2), c, cv.emu([c], b=b2), "bias", lambda: cv.emu([c], b=b2, dtype=torch.float32), sub)
        if cv.res is not None:
            s2 = cv.skip.clone()
            s2[..., c] = 0.5 * s2[..., c] + 0.25
            _one_hot(tally, base, cv.run(skip=s2), c, cv.emu([c], skip=s2), "residual", lambda: cv.emu([c], skip=s2, dtype=torch.float32), sub)
    return tally, base, emu


CLASSES = (0, 15, 16, 47, 64, 127, 128 + 33, -1)


@pytest.mark.parametrize("case,shape,res,ks,nox", [
    pytest.param("A f16c ping-pong bias", (2, 16, 64, 256), None, 1, False, id="A-pp-bias"),
    pytest.param("B f16c stream bias", (2, 16, 128, 256), None, 1, False, id="B-bias"),
    pytest.param("B f16c stream residual shift 0", (2, 16, 128, 256), 0, 1, False, id="B-res0"),
    pytest.param("B f16c stream residual shift 1", (2, 16, 128, 256), 1, 1, False, id="B-res1"),
    pytest.param("B f16c stream no_cross bias", (2, 16, 128, 256), None, 1, True, id="B-nocross-bias"),
    pytest.param("B f16c stream no_cross residual shift 1", (2, 16, 128, 256), 1, 1, True, id="B-nocross-res1"),
    pytest.param("C f16c K ranges ks=2 bias", (1, 16, 256, 256), None, 2, False, id="C-ks2-bias"),
    pytest.param("C f16c K ranges ks=2 residual shift 1", (1, 16, 256, 256), 1, 2, False, id="C-ks2-res1"),
    pytest.param("C f16c K ranges ks=4 bias", (1, 16, 256, 256), None, 4, False, id="C-ks4-bias"),
    pytest.param("C f16c K ranges ks=4 residual shift 0", (1, 16, 256, 256), 0, 4, False, id="C-ks4-res0")])
def test_f16c_bias_residual_per_channel(ctx, case, shape, res, ks, nox):
    """Cases A, B, C.  Measured: see the module docstring."""
    tally, _, _ = _check_conv(_Conv(ctx, *shape, res, ks=ks, no_cross=nox), case, CLASSES)
    tally.done(shape=list(shape), ks=ks)


@pytest.mark.parametrize("res", [None, 0], ids=["E-bias", "E-res0"])
def test_f16c6_bias_residual_per_channel(ctx, res):
    """Case E: the f16c6 stream kernel reads its weight scales from bytes 88 / 120 of every chunk of the weight row."""
    shape = (1, 32, 128, 256)
    tally, _, _ = _check_conv(_Conv(ctx, *shape, res, f6=True), f"E f16c6 stream {'bias' if res is None else 'residual shift 0'}",
                              CLASSES)
    tally.done(shape=list(shape), ks=1)


@pytest.mark.parametrize("res", [None, 1], ids=["bias", "res1"])
@pytest.mark.parametrize("B,r,cin,N", [pytest.param(5, 64, 128, 512, id="G-512"), pytest.param(6, 64, 128, 384, id="G-384-new-block")])
def test_f16c_second_tile_of_a_persistent_workgroup_per_channel(ctx, B, r, cin, N, res):
    """Case G: more (pixel tile, channel block) items than persistent_grid's one workgroup per CU (256 on MI355X), so some
    workgroups move to a second tile and re-read their scales and bias.  tests.helpers.later_round_mask restates persistent_grid,
    xcd_tile_range and the tile walk and says which items those are.
      (5, 64, 128, 512): 320 items; an XCD owns 40 consecutive items and 32 workgroups, workgroups 0..7 take items 32..39 of the
        range in their second round.  With the channel block running fastest (tiles_n = 4: walk (1, 4)) and 32 % 4 == 0 such an
        item lies in the channel block of the workgroup's FIRST item: the reload fetches the values the workgroup already holds,
        and a kernel that kept them across tiles would pass here.  This shape checks the second tile's pixels only.
      (6, 64, 128, 384): 288 items, XCD ranges of 36, tiles_n = 3: a workgroup's second item, 32 items on, lies in channel block
        (t + 32) % 3 != t % 3.  All 32 second-round items need the reload; the test requires that set to be non-empty for the
        device's CU count.  The channel blocks differ by a decade in scale, so stale scales or bias fail (i); and for a perturbed
        channel of each block, (ii) requires the change to show on the pixels of exactly those items, while every other channel,
        the workgroup's first-tile block included, stays bit-identical.
    Errors are reported separately over the re-read items, the second-round items and the rest (whole-channel denominators).
    Stream kernel by default, the ping-pong kernel under MSR_F16C_SW = 0 (child run)."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    later, moved = later_round_mask(B, r, N, n_cu), later_round_mask(B, r, N, n_cu, new_block=True)
    assert later.any(), f"{n_cu} CUs take {later.size} items in one round: no workgroup moves to a second tile"
    if N == 384:
        assert moved.any(), f"{n_cu} CUs: no workgroup's second tile lies in another channel block than its first at this shape"
    to_px = lambda m: torch.from_numpy(m).cuda().repeat_interleave(16, 1).repeat_interleave(16, 2)      # noqa: E731
    px_later, px_moved = to_px(later), to_px(moved)                                                       # [B, r, r, N // 128]

    def subsets(c):
        named = (("second-round items in another channel block than the workgroup's first", px_moved[..., c // 128]),
                 ("second-round items", px_later[..., c // 128]), ("first-round items", ~px_later[..., c // 128]))
        return [(n, k) for n, k in named if bool(k.any())]
    cv = _Conv(ctx, B, r, cin, N, res)
    case = f"G second tile ({B}, {r}, {cin}, {N}), {'bias' if res is None else 'residual shift 1'}"
    tally, base, emu = _check_conv(cv, case, tuple(128 * k + o for k, o in zip(range(N // 128), (0, 33, 47, 127))), subsets)
    err = (base.double() - emu).abs()
    den = emu.abs().reshape(-1, N).amax(0)
    over = lambda m: float((torch.where(m.repeat_interleave(128, 3), err, torch.zeros_like(err)).reshape(-1, N).amax(0) / den).max())   # noqa: E731
    e_moved, e_later, e_first = over(px_moved), over(px_later), over(~px_later)
    print(f"{case}: worst channel over re-read items {e_moved:.3e}, over second-round items {e_later:.3e}, over first-round items "
          f"{e_first:.3e} ({int(later.sum())} of {later.size} items are second-round, {int(moved.sum())} in another channel block)")
    tally.done(shape=[B, r, cin, N], ks=1, second_round_items=int(later.sum()), new_block_items=int(moved.sum()),
               worst_new_block=e_moved, worst_second_round=e_later, worst_first_round=e_first)


# ---- case D: gamma | beta conv with the SPADE epilogue ------------------------------------------------------------------------------
class _Spade:
    def __init__(self, ctx, B, r, C, shift):
        from moonsuperresolution_amd import ops
        self.ctx, self.r, self.C, self.shift = ctx, r, C, shift
        g = torch.Generator(device="cpu").manual_seed(53 + B + C + shift)
        ls = torch.logspace(-2, 1, C)                  # gamma and beta of a channel on that channel's scale: out[c] ~ ls[c]
        h = torch.relu(torch.randn((B, r, r, 128), generator=g)).cuda()
        wg = (torch.randn((3, 3, 128, C), generator=g) / 34 * ls).cuda()
        wb = (torch.randn((3, 3, 128, C), generator=g) / 34 * ls).cuda()
        bg, bb = (torch.randn(C, generator=g) * ls).cuda(), (torch.randn(C, generator=g) * ls).cuda()
        self.x = (3 + 2 * torch.randn((B, r >> shift, r >> shift, C), generator=g)).cuda()
        self.mean = self.x.mean((0, 1, 2)).contiguous()
        self.std = torch.sqrt(self.x.var((0, 1, 2), unbiased=False) + 1e-5).contiguous()
        w, self.bias = ops.spade_layout(wg, wb, bg, bb)
        self.himg, self.hparts = ops.f16c_activation_image(ops.pad_nhwc(h))
        self.wimg, self.wexp, self.wparts = ops.f16c_weight_image(w)
        c = torch.arange(C)
        self.rows_g = (c // 32) * 64 + (c % 32)        # gamma row of channel c; beta: + 32 (ops.spade_layout)

    def run(self, out_mode=0, ks=1, wexp=None, bias=None, x=None, mean=None, std=None):
        from moonsuperresolution_amd import ops
        pick = lambda t, d: d if t is None else t      # noqa: E731
        y = ops.conv3x3_f16c(self.ctx, self.himg, self.wimg, pick(wexp, self.wexp), pick(bias, self.bias), self.r,
                             epilogue=ops.EPI_SPADE, aux=pick(x, self.x), aux_shift=self.shift, mean=pick(mean, self.mean),
                             std=pick(std, self.std), out_padded=True, out_mode=out_mode, ksplit=ks)
        if out_mode == 4:
            y = ops.f16c_decode(y)[0]
        elif out_mode == 5:
            y = ops.f16c6_decode(y)[0]
        return y[:, 1:-1, 1:-1]

    def emu(self, ch=None, wparts=None, bias=None, x=None, mean=None, std=None, dtype=torch.float64):
        ch = list(range(self.C)) if ch is None else ch
        pick = lambda t, d: d if t is None else t      # noqa: E731
        wparts, bias = pick(wparts, self.wparts), pick(bias, self.bias)
        rg = self.rows_g[ch]
        gam = f16c_terms(self.hparts, tuple(t[:, rg] for t in wparts), self.r, dtype=dtype) + bias[rg].to(dtype)
        bet = f16c_terms(self.hparts, tuple(t[:, rg + 32] for t in wparts), self.r, dtype=dtype) + bias[rg + 32].to(dtype)
        xn = (_up(pick(x, self.x), self.shift)[..., ch].to(dtype) - pick(mean, self.mean)[ch].to(dtype)) / pick(std, self.std)[ch].to(dtype)
        v = gam * xn + bet
        return torch.where(v >= 0, v, 0.2 * v)

    def perturbations(self, c):
        """name -> (run kwargs, emu kwargs) for channel c."""
        from moonsuperresolution_amd import ops
        rg = int(self.rows_g[c])
        out = {}
        for name, row, dl, dh in (("gamma row w_lo scale byte + 3", rg, 3, 0), ("gamma row w_hi scale byte - 3", rg, 0, -3),
                                  ("beta row w_lo scale byte + 3", rg + 32, 3, 0), ("beta row w_hi scale byte - 3", rg + 32, 0, -3)):
            e, parts = ops.f16c_shift_wexp(self.wexp, self.wparts, row, dl, dh)
            out[name] = (dict(wexp=e), dict(wparts=parts))
        for name, row in (("gamma bias", rg), ("beta bias", rg + 32)):
            b2 = self.bias.clone()
            b2[row] = -1.25 * b2[row]
            out[name] = (dict(bias=b2), dict(bias=b2))
        m2, s2, x2 = self.mean.clone(), self.std.clone(), self.x.clone()
        m2[c] += 0.75
        s2[c] *= 1.5
        x2[..., c] = 0.5 * x2[..., c] + 1.0
        out["mean"], out["std"], out["x"] = (dict(mean=m2), dict(mean=m2)), (dict(std=s2), dict(std=s2)), (dict(x=x2), dict(x=x2))
        return out


SPADE_CLASSES = (0, 15, 16, 33, 47, 64, 64 + 33, 128 + 47, -1)     # rows 0, 15, 16, 65, 79, 128, 193, 335, 479 (+ 32: beta)


@pytest.mark.parametrize("shift,ks", [pytest.param(0, 1, id="D-x0-ks1"), pytest.param(1, 1, id="D-x1-ks1"),
                                      pytest.param(0, 2, id="D-x0-ks2"), pytest.param(1, 2, id="D-x1-ks2")])
def test_f16c_spade_per_channel(ctx, shift, ks):
    """Case D, out_mode 0 (fp32): (i) against leaky_relu(gamma * (x - mean) / std + beta) of the float64 own-terms gamma | beta,
    (ii) for the scale bytes of the channel's gamma row and of its beta row, their biases, mean[c], std[c] and x[..., c]."""
    B, r, C = 2, 16, 256
    sp = _Spade(ctx, B, r, C, shift)
    case = f"D f16c SPADE x shift {shift} ks={ks}"
    tally = _Tally(case)
    tally.kernel = _kernel(ctx, 128, 2, 0, ks)
    base = _launch(lambda: sp.run(0, ks), case)
    assert torch.equal(sp.run(0, ks), base), f"{case}: two launches on the same operands differ"
    e = tally.value(base, sp.emu(), np.arange(C), "unperturbed", lambda: sp.emu(dtype=torch.float32))
    print(f"{case}: unperturbed worst channel {int(e.argmax())}: {e.max():.3e} (median {np.median(e):.3e})")
    for c in (c % C for c in SPADE_CLASSES):
        for name, (rkw, ekw) in sp.perturbations(c).items():
            _one_hot(tally, base, sp.run(0, ks, **rkw), c, sp.emu([c], **ekw), name,
                     lambda: sp.emu([c], dtype=torch.float32, **ekw))       # noqa: B023
    tally.done(shape=[B, r, 128, 2 * C], ks=ks)


@pytest.mark.parametrize("mode,ks", [pytest.param(4, 1, id="D-f16c-image-ks1"), pytest.param(4, 2, id="D-f16c-image-ks2"),
                                     pytest.param(5, 1, id="D-f16c6-image-ks1")])
def test_f16c_spade_image_outputs_one_hot(ctx, mode, ks):
    """Case D, out_modes 4 (f16c image) and 5 (f16c6 image; whole tiles only): one-hot on the decoded hi = fp16 of the value.
    (The 6-bit pieces of mode 5 share one block scale among 32 channels, so they may follow a neighbour: hi may not.)  The
    changes move channel c by ~1e-3 of its magnitude or more, two fp16 steps: hi changes."""
    sp = _Spade(ctx, 2, 16, 256, 1)
    case = f"D f16c SPADE out_mode {mode} ks={ks}"
    base = _launch(lambda: sp.run(mode, ks), case)
    assert torch.equal(sp.run(mode, ks), base), f"{case}: two launches on the same operands differ"
    n = 0
    for c in (c % sp.C for c in SPADE_CLASSES):
        for name, (rkw, _) in sp.perturbations(c).items():
            y2 = sp.run(mode, ks, **rkw)
            chk = y2.clone()
            chk[..., c] = base[..., c]
            assert torch.equal(chk, base), f"{case} {name}: a channel other than {c} changed"
            assert not torch.equal(y2[..., c], base[..., c]), f"{case} {name}: channel {c} did not change"
            n += 1
    print(f"{case}: {n} one-hot launches")
    print(f"dispatch: case D under MSR_F16C_SW={SW_MODE} ran the {_kernel(ctx, 128, 2, mode, ks)} kernel")


# ---- case F: fp8 ping-pong kernel ----------------------------------------------------------------------------------------------
def _fp8_items_with_other_scales(B, r, N, n_cu):
    """The ONE form of the fp8 kernel (launch_pp: Cpad = 128, one chunk) runs TWO items per unrolled body: item A = the
    workgroup's tile, item B = tile + slots of the XCD's range (conv_pp.hip: `tb = tile + slots < cnt ? tile + slots : tile`), whose
    scales are re-read through n0b after item A's epilogue.  -> (bool [B, r / 16, r / 16, N / 128] of the items B whose channel
    block differs from their item A's, number of items B).  The ONE form does not call conv_walk: channel block fastest."""
    ty, tiles_n = r // 16, N // 128
    items = B * ty * ty * tiles_n
    sr = persistent_item_rounds(items, n_cu)
    slots = (min((items + 7) & ~7, max(n_cu & ~7, 8))) >> 3
    mask, n_b = np.zeros((B, ty, ty, tiles_n), bool), 0
    for t, (_, rnd) in enumerate(sr):
        if rnd % 2 == 1:
            n_b += 1
            (tn_b, tm), (tn_a, _) = conv_walk_item(t, items // tiles_n, tiles_n, walk=False), conv_walk_item(t - slots, items // tiles_n, tiles_n, walk=False)
            if tn_b != tn_a:
                mask[tm // (ty * ty), (tm // ty) % ty, tm % ty, tn_b] = True
    return mask, n_b


@pytest.mark.parametrize("B,r,cin,N", [pytest.param(2, 16, 128, 256, id="F-small"), pytest.param(6, 64, 128, 384, id="F-item-B")])
def test_fp8_bias_per_channel(ctx, B, r, cin, N):
    """Case F.  cin = 128 -> Cpad = 128 -> launch_pp's `one` (p.Cin == 32 floats): the two-items-per-body form.  At (2, 16, 128, 256)
    there are 4 items on 8 workgroups: every workgroup's item B is its item A again (n0b == n0), as in every ONE-form shape of
    test_conv_fp8_exact_on_quantised_operands with N = 128 or fewer items than CUs.  n0b differs from n0 only if (a) there are
    more items than workgroups and (b) slots = grid / 8 is not a multiple of tiles_n (channel block fastest): (6, 64, 128, 384) has
    96 * 3 = 288 items on 256 workgroups, XCD ranges of 36 items for 32 workgroups, so workgroups 0..3 of every XCD take item
    tile + 32 as item B, in channel block (t + 32) % 3 != t % 3.  The test computes that set from the device's CU count and
    requires it to be non-empty at that shape; (i) over the whole tensor then covers the scales read through n0b, and the
    figure over exactly those items is printed.  (ii): the four equal scale bytes of a channel + 3 and - 3, and its bias."""
    from moonsuperresolution_amd import ops
    from tests.helpers import conv_channel_inputs
    case = f"F fp8 ping-pong bias ({B}, {r}, {cin}, {N})"
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    other, n_b = _fp8_items_with_other_scales(B, r, N, n_cu)
    if N == 384:
        assert other.any(), f"{n_cu} CUs: no item B in another channel block than its item A at this shape"
    x, w, b, _ = conv_channel_inputs(B, r, cin, N, seed=41 + B + r)
    b = b.cuda()
    xb, xdq = ops.bf8_activation_image(ops.pad_nhwc(x.cuda()))
    wq, wexp, wdq = ops.fp8_weight_image(ops.kernel_layout(w.cuda()))
    xdq = xdq.double()

    def emu(ch=None, wdq_=None, b_=None, dtype=torch.float64):
        ch = slice(None) if ch is None else ch
        return conv_taps(xdq, (wdq if wdq_ is None else wdq_)[:, ch], r, dtype=dtype) + (b if b_ is None else b_)[ch].to(dtype)
    run = lambda e=wexp, bias=b: ops.conv3x3_fp8(ctx, xb, wq, e, bias, r)      # noqa: E731
    tally = _Tally(case)
    base = run()
    assert torch.equal(run(), base), f"{case}: two launches on the same operands differ"
    ref = emu()
    e = tally.value(base, ref, np.arange(N), "unperturbed", lambda: emu(dtype=torch.float32))
    print(f"{case}: unperturbed worst channel {int(e.argmax())}: {e.max():.3e}; {n_b} items B, {int(other.sum())} of them in "
          f"another channel block than their item A")
    px = torch.from_numpy(other).cuda().repeat_interleave(16, 1).repeat_interleave(16, 2)
    extra = {}
    if other.any():
        err = torch.where(px.repeat_interleave(128, 3), (base.double() - ref).abs(), torch.zeros_like(ref))
        e_b = float((err.reshape(-1, N).amax(0) / ref.abs().reshape(-1, N).amax(0)).max())
        print(f"{case}: worst channel over the items B with re-read scales {e_b:.3e}")
        extra = dict(items_b_other_block=int(other.sum()), worst_items_b=e_b)
    for c in (c % N for c in CLASSES + ((256 + 33,) if N > 256 else ())):
        m = px[..., c // 128]
        sub = [("items B with re-read scales", m)] if bool(m.any()) else []
        for d in (3, -3):
            e2, q2 = ops.fp8_shift_wexp(wexp, wdq, c, d)
            _one_hot(tally, base, run(e=e2), c, emu([c], wdq_=q2), f"scale bytes {d:+d}", lambda: emu([c], wdq_=q2, dtype=torch.float32), sub)
        b2 = b.clone()
        b2[c] = b[c + 1 if c + 1 < N else c - 1] * 1.25
        _one_hot(tally, base, run(bias=b2), c, emu([c], b_=b2), "bias", lambda: emu([c], b_=b2, dtype=torch.float32), sub)
    tally.done(shape=[B, r, cin, N], ks=1, **extra)


# ---- the other kernel dispatch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["0", "2"])
def test_f16c_cases_under_the_other_kernel_dispatch(mode):
    """The f16c tests of this file in a child process under MSR_F16C_SW = 0 / 2 (one child at a time, each under its own timeout),
    as tests/test_gpu_conv_kernel.py::test_f16c_convs_under_the_other_kernel_dispatch does.  Skipped cases: see the module
    docstring (none); every one of cases A, B, C, D and G must have passed at least once in the child, and the child must
    report the kernels the mode stands for."""
    env = dict(os.environ, MSR_F16C_SW=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-v", "-x", "-m", "gpu", "-rsP", "-k",
                        "f16c and not other_kernel_dispatch"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    passed = set(re.findall(r"\[([A-G])-[^\]]*\] PASSED", r.stdout))
    skipped = re.findall(r"^SKIPPED.*$", r.stdout, re.M)
    ran = set(re.findall(rf"^dispatch: case ([A-G]) under MSR_F16C_SW={mode} ran the ([a-z-]+) kernel$", r.stdout, re.M))
    print(f"MSR_F16C_SW={mode}: cases passed {sorted(passed)}, skipped {skipped}, kernels {sorted(ran)}")
    assert {"A", "B", "C", "D", "G"} <= passed, (sorted(passed), skipped)
    assert not skipped, skipped          # the recorded skip list is empty: a new skip is a change of the dispatch
    # the child really ran the other kernel, by the library's own dispatch rule (msr_debug_f16c_kernel; each child test checks
    # it against the meaning of the mode): 0 moves the whole-tile B and G launches to the ping-pong kernel and leaves D there;
    # 2 moves D's whole-tile launches to the stream kernel.  (B keeps its no_cross launches, D its K-range ones: both kernels.)
    if mode == "0":
        assert {("B", "ping-pong"), ("G", "ping-pong")} <= ran and ("G", "stream") not in ran and ("D", "stream") not in ran, sorted(ran)
    else:
        assert {("B", "stream"), ("G", "stream"), ("D", "stream")} <= ran and ("G", "ping-pong") not in ran, sorted(ran)

"""GPU (-m gpu): every op of the planned pix2pix network against float64 of ITS OWN input; the pix2pix twin of
tests/test_gpu_network_sites.py.

Two forwards of Pix2Pix (BASELINE configs[0]) at B = 3 and B = 16 with non-trivial BatchNormalization statistics (the second
must equal the first bit for bit); then the plan is walked op by op (Generator.conv_forms).  Every site reads the input the
GPU itself read and the output it wrote, both fetched AFTER the whole forward (msr_debug_tensor: ws.p2p.cat1..7, ws.p2p.down8),
so errors do not compound, a failure names the layer, and a later op that clobbers an earlier half fails the earlier site too.
B = 16 is the smallest batch whose plan holds the 128 x 128 tile and an unsplit up conv; B = 3 keeps the non-power-of-two tail
and the deep K splits (test_configs_cover_the_forms pins that on the CPU, from msr_debug_form_table).

Uploaded images, bit for bit against Python twins restated from csrc/api.hip and csrc/weight_images.hip: HWIO as it is (down1),
hwio_to_tap_oc_ic (down2..8), the four parity images of W_P2P_UP (up1..7, tests.helpers.p2p_parity_images), head_weff_transpose
(p2p.last.weff).  The folded scale / shift of plan_pix2pix against a float64 fold (FOLD_* below); the sites then use the
UPLOADED scale / shift.

Sites and bounds:
  direct (down1)   the call's input -> channels [64, 128) of cat7: |err| <= 20 * 2^-24 * sum |w| |x| per element
                   (test_conv_smallcin's bound, K = 32).  The plan only ever calls conv_direct_kernel with transposed = 0, c1 = 0,
                   no scale / shift, act = 2: its other branches (a second input, transposed, scale / shift, relu / tanh) have no
                   caller and are not tested.
  down2..8         the skip slice of cat(9 - i) -> the skip slice of cat(8 - i), or ws.p2p.down8: float64 tap matmuls of the
                   4 x 4 stride-2 'same' conv, uploaded scale / shift, leaky 0.3
  up1..7           ONE site per layer (four parity launches): the up half of cat_i against
                   relu(scale * oracle.generator_ref.conv2d_transpose_same_s2(src) + shift); a failure names the parity
                   (y & 1, x & 1) and the channel of the worst element
  conv sites       tests.helpers.affine_site_check: tensor rel <= 1e-5 and, per channel, max |y - ref| <=
                   max(1e-5 * R_c, 4 * E_c) (E_c: plain fp32 tap matmuls in torch, evaluated only where 1e-5 * R_c is exceeded)
  head             cat7 -> the output, tanh: rel <= 1e-5 (test_head_kernel_known_answers)
  borders          of cat1..7 and down8: exactly zero after the second forward

Controls (CPU): the checker fed a reference-derived output with one channel's shift moved by 1e-3 of its range, one channel
pair swapped, one parity shifted by one column fails and names the channel / the parity; the reference rounded to fp32 passes.

Every site is printed and appended to parity_pix2pix_sites.jsonl in the run-record directory; a copy of one full run is
profiles/pix2pix_sites_parity.jsonl.  MEASURED on an MI355X (per form in MEASURED below): nothing failed; the largest conv
figure is 0.68 of the per-channel bound (down4 at B = 16: tile 1, ksplit 2), the head stands at 0.08, down1 at 0.27.  Wall time of
the two GPU tests on an MI355X: 3 s (the network is 11.9 GFLOP per patch; the float64 references run on the GPU).
"""
import json
import os
import time

import numpy as np
import pytest
import torch

from tests.helpers import (affine_act, affine_site_check, conv_taps_k, conv_transpose_scatter, p2p_parity_images, pad_hw,
                           P2P_KMAP, rel_linf)
from tests.helpers import record_dir as _record_dir

U = 2.0 ** -24
LEAK = float(np.float32(0.3))          # keras LeakyReLU() default alpha, as the plan passes it (a float)
BN_EPS = float(np.float32(1e-3))       # plan_pix2pix: v + 1e-3f
P2P_DOWN = (64, 128, 256, 512, 512, 512, 512, 512)       # csrc/host.h kP2PDown, kP2PUp
P2P_UP = (512, 512, 512, 512, 256, 128, 64)
CONFIGS = [(256, 3), (256, 16)]

# The fold of plan_pix2pix, in fp32 on the host: scale = g / sqrt(v + eps), shift = b - m * scale.  Every operation rounds to
# nearest: a relative error of at most u = 2^-24 each.
#   scale: fl(v + eps) = (v + eps)(1 + d1); the square root halves d1 and adds d2; the division adds d3: at most 2.5 u relative,
#          inside FOLD_SCALE_REL = 4 u.
#   shift: fl(m * scale) carries scale's 2.5 u and its own u, the subtraction one u of |b - m * scale| <= |b| + |m * scale|: at most
#          u (|b| + 4.5 |m * scale|) to first order, which FOLD_SHIFT_REL * (|b| + |m * scale|) = 4 u (|b| + |m * scale|) covers
#          wherever |m * scale| <= 6 |b|; elsewhere the stated bound is up to 1 / 9 short of the worst case of five roundings that
#          all err fully and in the same direction, and stands as stated.
FOLD_SCALE_REL = 4 * U
FOLD_SHIFT_REL = 4 * U

# MEASURED on an MI355X, one full run of both configurations (32 sites): form -> (largest per-channel error / bound, largest
# tensor rel / 1e-5, the sites that ran it as (B, layer)).  Every bit compare stands at 0 differing words, every border is zero,
# the second forward equals the first; the fold stands at 0.31 to 0.60 of its bound (at most 2.4 * 2^-24 relative).
# ONE site needed the K-length allowance: p2p.down8 at B = 3 (K = 16 * 512 = 8192 and three output pixels per channel, so R_c is the
# largest of three values): 0.62 of 4 * E_c; at B = 16 the same layer stands at 0.48 of 1e-5 * R_c.
# WALL_TIME: the two GPU tests take 2.0 s (B = 3, with the first-use costs of the process) and 0.9 s (B = 16).
MEASURED = {
    "direct taps=16 act=2": (0.27, None, [(3, "down1"), (16, "down1")]),
    "tile=0 ksplit=1 taps=16 act=2": (0.25, 0.064, [(16, "down2")]),
    "tile=1 ksplit=1 taps=16 act=2": (0.50, 0.157, [(16, "down3")]),
    "tile=1 ksplit=2 taps=16 act=2": (0.68, 0.211, [(16, "down4")]),
    "tile=1 ksplit=4 taps=16 act=2": (0.11, 0.023, [(3, "down2")]),
    "tile=1 ksplit=8 taps=16 act=2": (0.56, 0.082, [(3, "down3"), (16, "down5")]),
    "tile=1 ksplit=16 taps=16 act=2": (0.62, 0.056, [(3, "down4..8"), (16, "down6..8")]),
    "tile=1 ksplit=1 taps=4 act=1": (0.26, 0.132, [(16, "up7")]),
    "tile=1 ksplit=2 taps=4 act=1": (0.13, 0.081, [(16, "up6")]),
    "tile=1 ksplit=4 taps=4 act=1": (0.16, 0.074, [(16, "up5")]),
    "tile=1 ksplit=8 taps=4 act=1": (0.14, 0.057, [(3, "up7"), (16, "up4")]),
    "tile=1 ksplit=16 taps=4 act=1": (0.11, 0.045, [(3, "up1..6"), (16, "up1..3")]),
    "head": (0.083, None, [(3, "last"), (16, "last")]),
}


def _record(**kw):
    try:
        os.makedirs(_record_dir(), exist_ok=True)
        with open(os.path.join(_record_dir(), "parity_pix2pix_sites.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")
    except OSError:
        pass
    print("p2p site", kw)


def cat_channels(i):
    """(up half, skip half) of cat_i = [up_i | down_(8 - i)]"""
    return P2P_UP[i - 1], P2P_DOWN[7 - i]


def head_weff_twin(k44c):
    """head_weff_transpose (csrc/weight_images.hip): [4, 4, C] -> weff[py][px][dy][dx][C], zero where the parity has no tap"""
    C = k44c.shape[-1]
    weff = torch.zeros((2, 2, 3, 3, C), dtype=k44c.dtype)
    for py in range(2):
        for px in range(2):
            for t in range(2):
                for u in range(2):
                    weff[py, px, py + t, px + u] = k44c[P2P_KMAP[py][t], P2P_KMAP[px][u]]
    return weff


def border_words(buf):
    w = buf.contiguous().view(torch.int32)
    return int(w[:, 0].ne(0).sum() + w[:, -1].ne(0).sum() + w[:, 1:-1, 0].ne(0).sum() + w[:, 1:-1, -1].ne(0).sum())


class P2PSites:
    def __init__(self, S, B):
        from moonsuperresolution_amd import Generator, make_weights, synthetic_patches
        assert S == 256
        self.B = B
        self.w = make_weights("pix2pix", 256, seed=1234, bias_scale=0.05)
        self.x = synthetic_patches(B, 256, 0)
        self.gen = Generator(256, B, variant="pix2pix", weights=self.w)
        y1 = self.gen(self.x, training=False)
        self.y = self.gen(self.x, training=False)
        self.repeat_words_differ = int((y1.view(np.uint32) != self.y.view(np.uint32)).sum())
        self.ops = self.gen.conv_forms()
        self.dev = torch.device("cuda")
        self._cache = {}

    def close(self):
        self.gen.close()
        self._cache.clear()
        torch.cuda.empty_cache()

    def buf(self, name):
        """a padded workspace buffer, whole, on the GPU"""
        if name not in self._cache:
            if len(self._cache) > 3:
                self._cache.clear()
            if name == "ws.p2p.down8":
                shape = (self.B, 3, 3, 512)
            else:
                i = int(name[-1])
                shape = (self.B, (1 << i) + 2, (1 << i) + 2, sum(cat_channels(i)))
            self._cache[name] = torch.from_numpy(self.gen.debug_tensor(name, shape)).to(self.dev)
        return self._cache[name]

    def hw(self, name):
        return torch.from_numpy(np.ascontiguousarray(self.w[name]))

    def words_differ(self, name, want):
        want = want.contiguous().reshape(-1).numpy().view(np.uint32)
        got = self.gen.debug_tensor(name, (want.size,)).view(np.uint32)
        try:
            self.gen.debug_tensor(name, (want.size + 1,))
            longer = 1
        except ValueError:
            longer = 0
        return int((got != want).sum()) + longer

    def fold(self, prefix, C):
        """uploaded scale / shift of `prefix`.bn against the float64 fold -> (scale, shift on the GPU, figures)"""
        g, b, m, v = (self.hw(f"{prefix}.{n}").double() for n in ("gamma", "beta", "moving_mean", "moving_variance"))
        sc64 = g / torch.sqrt(v + BN_EPS)
        sh64 = b - m * sc64
        sc = torch.from_numpy(self.gen.debug_tensor(prefix + ".scale", (C,)))
        sh = torch.from_numpy(self.gen.debug_tensor(prefix + ".shift", (C,)))
        fig = {"scale_fold": float(((sc.double() - sc64).abs() / (FOLD_SCALE_REL * sc64.abs())).max()),
               "shift_fold": float(((sh.double() - sh64).abs() / (FOLD_SHIFT_REL * (b.abs() + (m * sc64).abs())).clamp_min(1e-300)).max())}
        return sc.to(self.dev).double(), sh.to(self.dev).double(), fig

    # -- sites ------------------------------------------------------------------------------------
    def check_direct(self, op):
        w = self.hw("p2p.down1.kernel")
        fig = {"weight_words_differ": float(self.words_differ("p2p.down1.kernel", w))}
        cat7 = self.buf("ws.p2p.cat7")
        fig["out_border"] = float(border_words(cat7))
        x = pad_hw(torch.from_numpy(self.x).to(self.dev))
        w_tnk = w.reshape(16, 2, 64).permute(0, 2, 1).contiguous().to(self.dev)
        ref = affine_act(conv_taps_k(x, w_tnk, 128, 4, 2), 2, LEAK)
        mag = conv_taps_k(x.abs(), w_tnk.abs(), 128, 4, 2)
        got = cat7[:, 1:-1, 1:-1, P2P_UP[6]:P2P_UP[6] + 64].double()
        fig["value"] = float(((got - ref).abs() / (20 * U * mag).clamp_min(1e-300)).max())
        return fig, "direct taps=16 act=2"

    def conv_site(self, out, pre, act, eval32, what, parity):
        res = affine_site_check(out, pre, act, LEAK, None, what, parity)
        fig = {}
        if not res["ok"]:                        # K-length allowance: the same terms in plain fp32 (module docstring)
            res = affine_site_check(out, pre, act, LEAK, eval32(), what, parity)
            fig["allowance_used"] = 1.0
        fig.update(value=res["ratio"], tensor=res["tensor_rel"] / 1e-5)
        return fig, res

    def check_down(self, op, i):
        cin, c, r = P2P_DOWN[i - 2], P2P_DOWN[i - 1], 256 >> i
        assert (op["cin"], op["N"], op["r"], op["stride"], op["B"]) == (cin, c, r, 2, self.B), op
        src, off = f"ws.p2p.cat{9 - i}", P2P_UP[8 - i]
        assert op["in"] == src and op["bias"] == f"p2p.down{i}.bn.shift", op
        w = self.hw(f"p2p.down{i}.kernel")
        w_tnk = w.reshape(16, cin, c).permute(0, 2, 1).contiguous()
        fig = {"weight_words_differ": float(self.words_differ(f"p2p.down{i}.kernel", w_tnk))}
        sc, sh, ffig = self.fold(f"p2p.down{i}.bn", c)
        fig.update(ffig)
        xin = self.buf(src)
        fig["in_border"] = float(border_words(xin))
        xs = xin[..., off:off + cin]
        w_dev = w_tnk.to(self.dev)
        pre = conv_taps_k(xs, w_dev, r, 4, 2) * sc + sh
        if i < 8:
            assert op["out"] == f"ws.p2p.cat{8 - i}", op
            o0 = P2P_UP[7 - i]
            out = self.buf(op["out"])[:, 1:-1, 1:-1, o0:o0 + c]
        else:
            assert op["out"] == "ws.p2p.down8", op
            d8 = self.buf("ws.p2p.down8")
            fig["out_border"] = float(border_words(d8))
            out = d8[:, 1:-1, 1:-1]
        eval32 = lambda: affine_act(conv_taps_k(xs, w_dev, r, 4, 2, dtype=torch.float32) * sc.float() + sh.float(), 2, LEAK)   # noqa: E731
        vfig, res = self.conv_site(out, pre, 2, eval32, f"p2p.down{i} B={self.B}", False)
        fig.update(vfig)
        return fig, f"tile={op['tile']} ksplit={op['ksplit']} taps=16 act=2", res

    def check_up(self, ops4, i):
        from oracle import generator_ref
        c = P2P_UP[i - 1]
        r = 1 << (i - 1)
        src = "ws.p2p.down8" if i == 1 else f"ws.p2p.cat{i - 1}"
        cin = 512 if i == 1 else sum(cat_channels(i - 1))
        assert len(ops4) == 4 and len({(o["tile"], o["ksplit"]) for o in ops4}) == 1, ops4
        for o in ops4:
            assert (o["in"], o["out"], o["cin"], o["N"], o["r"], o["stride"], o["bias"]) == \
                (src, f"ws.p2p.cat{i}", cin, c, r, 1, f"p2p.up{i}.bn.shift"), o
        k = self.hw(f"p2p.up{i}.kernel")
        fig = {"weight_words_differ": float(self.words_differ(f"p2p.up{i}.kernel", p2p_parity_images(k)))}
        sc, sh, ffig = self.fold(f"p2p.up{i}.bn", c)
        fig.update(ffig)
        xin = self.buf(src)
        fig["in_border"] = float(border_words(xin))
        xs = xin[:, 1:-1, 1:-1]
        k_dev = k.to(self.dev)
        pre = torch.empty((self.B, 2 * r, 2 * r, c), dtype=torch.float64, device=self.dev)
        k64 = k_dev.double()
        for b in range(self.B):                  # one sample at a time: bounds the float64 temporaries
            pre[b] = generator_ref.conv2d_transpose_same_s2(xs[b:b + 1].double(), k64)[0] * sc + sh
        del k64
        obuf = self.buf(f"ws.p2p.cat{i}")
        fig["out_border"] = float(border_words(obuf))
        out = obuf[:, 1:-1, 1:-1, :c]
        eval32 = lambda: affine_act(conv_transpose_scatter(xs, k_dev, torch.float32) * sc.float() + sh.float(), 1, 0.0)   # noqa: E731
        vfig, res = self.conv_site(out, pre, 1, eval32, f"p2p.up{i} B={self.B}", True)
        fig.update(vfig)
        return fig, f"tile={ops4[0]['tile']} ksplit={ops4[0]['ksplit']} taps=4 act=1", res

    def check_head(self, op):
        from oracle import generator_ref
        assert (op["in"], op["wt"], op["cin"], op["r"], op["tanh"]) == ("ws.p2p.cat7", "p2p.last.weff", 128, 128, 1), op
        k = self.hw("p2p.last.kernel")                                   # [4, 4, 1, C]
        fig = {"weight_words_differ": float(self.words_differ("p2p.last.weff", head_weff_twin(k[:, :, 0])))}
        xs = self.buf("ws.p2p.cat7")[:, 1:-1, 1:-1]
        bias = torch.from_numpy(self.w["p2p.last.bias"]).double().to(self.dev)
        ref = torch.empty((self.B, 256, 256, 1), dtype=torch.float64, device=self.dev)
        for b in range(self.B):
            ref[b] = torch.tanh(generator_ref.conv2d_transpose_same_s2(xs[b:b + 1].double(), k.to(self.dev).double(), bias))[0]
        fig["value"] = rel_linf(self.y, ref.cpu().numpy()) / 1e-5
        return fig, "head"

    def run(self):
        """-> [(site, form, figures, worst error / bound, message)] for the 1 + 7 + 7 + 1 sites"""
        from moonsuperresolution_amd.generator import form_table
        table = form_table(256, self.B, "pix2pix", 0)
        kinds = [o["kind"] for o in self.ops]
        assert kinds == ["direct"] + ["conv"] * 35 + ["head"], kinds
        for o in self.ops[1:36]:
            layer = o["wt"][: -len(".kernel")]
            assert (o["epi"], o["prec"], o["kernel"], o["tile"], o["ksplit"]) == \
                (4, 0, "generic", table[layer]["tile"], table[layer]["ksplit"]), (o, table[layer])
        sites = [("p2p.down1", lambda: self.check_direct(self.ops[0]))]
        sites += [(f"p2p.down{i}", lambda i=i: self.check_down(self.ops[i - 1], i)) for i in range(2, 9)]
        sites += [(f"p2p.up{i}", lambda i=i: self.check_up(self.ops[8 + 4 * (i - 1): 8 + 4 * i], i)) for i in range(1, 8)]
        sites += [("p2p.last", lambda: self.check_head(self.ops[36]))]
        res = []
        for name, fn in sites:
            t0 = time.time()
            got = fn()
            fig, form, msg = got[0], got[1], (got[2]["message"] if len(got) > 2 else name)
            worst = max(over_bound(fig).values())
            _record(S=256, B=self.B, site=name, form=form, worst_over_bound=worst, seconds=round(time.time() - t0, 2), **fig)
            res.append((name, form, fig, worst, msg))
        return res


def over_bound(fig):
    """figures of a site -> {check: error / bound}: a count of differing or non-zero words stands at 1 + the count"""
    return {k: ((0.0 if v == 0 else 1.0 + v) if ("words" in k or "border" in k) else v) for k, v in fig.items()
            if k != "allowance_used"}


@pytest.mark.gpu
@pytest.mark.parametrize("S,B", CONFIGS)
def test_pix2pix_sites_against_fp64(hip_lib, S, B):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sites = P2PSites(S, B)
    try:
        assert sites.repeat_words_differ == 0, f"the second forward differs from the first in {sites.repeat_words_differ} words"
        res = sites.run()
    finally:
        sites.close()
    assert len(res) == 16
    bad = [(name, form, {k: v for k, v in over_bound(fig).items() if not v <= 1}, msg) for name, form, fig, worst, msg in res
           if not worst <= 1]
    assert not bad, bad


# ---- CPU: the forms the two batches run ---------------------------------------------------------------------------------------------
def test_configs_cover_the_forms(hip_lib):
    """msr_debug_form_table for the two batches: together their down convs hold (tile 0, ksplit 1), (tile 1, ksplit 1) and every
    ksplit of 2, 4, 8, 16, their up convs ksplit 1 and ksplit > 1.  If the planner's rule moves, this test stops claiming it."""
    from moonsuperresolution_amd.generator import form_table
    down, up = set(), set()
    for S, B in CONFIGS:
        t = form_table(S, B, "pix2pix", 0)
        down |= {(t[f"p2p.down{i}"]["tile"], t[f"p2p.down{i}"]["ksplit"]) for i in range(2, 9)}
        up |= {(t[f"p2p.up{i}"]["tile"], t[f"p2p.up{i}"]["ksplit"]) for i in range(1, 8)}
    assert {(0, 1), (1, 1)} <= down, down
    assert {2, 4, 8, 16} <= {ks for _, ks in down}, down
    assert 1 in {ks for _, ks in up} and any(ks > 1 for _, ks in up), up


# ---- CPU: controls of the site checker ------------------------------------------------------------------------------------------
def _control_pre():
    g = torch.Generator(device="cpu").manual_seed(31)
    pre = torch.randn((2, 8, 8, 16), generator=g, dtype=torch.float64) * torch.logspace(-1, 1, 16, dtype=torch.float64) + 0.3
    return pre, affine_act(pre, 1, 0.0).float()


def test_control_reference_rounded_to_fp32_passes():
    pre, out = _control_pre()
    res = affine_site_check(out, pre, 1, 0.0, None, "control", parity=True)
    assert res["ok"] and res["ratio"] < 0.01, res


def test_control_shifted_channel_fails_and_is_named():
    """one channel's shift moved by 1e-3 of that channel's range: 100 x the per-channel bound, 1e-4 of the tensor's for channel 5"""
    pre, out = _control_pre()
    c = 5
    moved = pre.clone()
    moved[..., c] += 1e-3 * float(pre[..., c].abs().max())
    bad = out.clone()
    bad[..., c] = affine_act(moved, 1, 0.0).float()[..., c]
    res = affine_site_check(bad, pre, 1, 0.0, None, "control", parity=True)
    assert not res["ok"] and res["channel"] == c and f"channel {c}" in res["message"], res
    assert res["tensor_rel"] < 1e-4          # a tensor-level bound of 1e-4 would not have seen it


def test_control_swapped_channel_pair_fails_and_is_named():
    pre, out = _control_pre()
    bad = out.clone()
    bad[..., 6], bad[..., 7] = out[..., 7], out[..., 6]
    res = affine_site_check(bad, pre, 1, 0.0, None, "control", parity=True)
    assert not res["ok"] and res["channel"] in (6, 7) and f"channel {res['channel']}" in res["message"], res


def test_control_parity_shifted_by_one_column_fails_and_is_named():
    pre, out = _control_pre()
    bad = out.clone()
    bad[:, 1::2, 0::2] = torch.roll(out[:, 1::2, 0::2], 1, dims=2)
    res = affine_site_check(bad, pre, 1, 0.0, None, "control", parity=True)
    assert not res["ok"] and res["parity"] == (1, 0) and "parity (y & 1, x & 1) = (1, 0)" in res["message"], res

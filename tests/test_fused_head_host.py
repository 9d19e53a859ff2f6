"""Host side of the opt-in fused head (no GPU): the Generator option's validation, the flag table, the slot table of the
partial sums and the gather's restatement against the oracle's head."""
import numpy as np
import pytest
import torch

from moonsuperresolution_amd import Generator, _lib, ops
from oracle import generator_ref as G


def test_head_option_is_validated_before_any_device_use(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was loaded before the option was validated")
    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(ValueError, match="head"):
        Generator(64, 4, head="nonsense")
    with pytest.raises(ValueError, match="head"):
        Generator(64, 4, head="fused", precision="bf16x3")
    with pytest.raises(ValueError, match="head"):
        Generator(64, 4, head="fused", precision="f16c", cross="fp6")
    with pytest.raises(ValueError, match="head"):
        Generator(256, 4, head="fused", variant="pix2pix")


def test_head_flags():
    assert _lib.HEAD_FLAGS == {"separate": 0, "fused": 64}
    assert not any(_lib.HEAD_FLAGS["fused"] & v for v in list(_lib.PRECISION_FLAGS.values()) + list(_lib.CROSS_FLAGS.values()))
    assert any(name == "msr_op_conv3x3_f16c_head" for name, _, _ in _lib.SYMBOLS)


def test_head_slots_are_the_25_live_taps():
    slots = ops.head_slots()
    assert len(slots) == 25 and sorted(slots.values()) == list(range(25))
    weff = ops.head_taps_upconv(torch.ones((4, 4, 1)))
    live = {(py, px, dy, dx) for py in range(2) for px in range(2) for dy in range(3) for dx in range(3)
            if float(weff[py, px, dy, dx, 0]) != 0.0}
    assert set(slots) == live
    assert [sum(1 for k in slots if k[:2] == p) for p in ((0, 0), (0, 1), (1, 0), (1, 1))] == [9, 6, 6, 4]


def test_gather_of_fp64_partials_equals_the_oracle_head():
    """P from a random x [2, 16, 16, 128] in float64, gathered by ops.head_from_partials, against the oracle's head
    (leaky_relu -> UpSampling2D(2) -> Conv2D(1, 4, 'same'), oracle/generator_ref.py): equal to float64 rounding.  Pins the slot
    table, the per-parity taps and the zero border (a tile-sized image: all four borders, never the neighbouring sample)."""
    g = torch.Generator().manual_seed(11)
    x = 3 * torch.randn((2, 16, 16, 128), generator=g, dtype=torch.float64)
    k = torch.randn((4, 4, 128, 1), generator=g, dtype=torch.float64) / 45
    bias = 0.37
    want = G.conv2d_same(G.leaky_relu(G.upsample2x(x), G.LEAK), k, torch.tensor([bias], dtype=torch.float64))[..., 0]
    P = ops.head_partials(x, k[..., 0])
    assert P.shape == (2, 16, 16, 32) and P.dtype == torch.float64
    assert float(P[..., 25:].abs().max()) == 0.0
    got = ops.head_from_partials(P, bias)
    assert got.shape == (2, 32, 32)
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-14, err
    # a sample's border reads zeros, not the other sample's lines: the samples are independent
    alone = ops.head_from_partials(P[1:], bias)
    assert torch.equal(alone[0], got[1])

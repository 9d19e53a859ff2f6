"""Host side of the activation-range scan (no GPU): regime classification, the report's text, the host twin of the kernel on
hand-computed images, the 464 boundary of the e4m3 cross piece, and the binding's behaviour on a library without the entries."""
import numpy as np
import pytest
import torch

from moonsuperresolution_amd import _lib, ops
from moonsuperresolution_amd.generator import RangeReport


def rec(tensor, producer=0, fmt=4, max_abs=40.0, total=1000, cross=0, clamped=0, nonfinite=0):
    return dict(tensor=tensor, format=fmt, producer=producer, max_abs=np.float32(max_abs), n_total=total, n_cross_clipped=cross,
                n_clamped=clamped, n_nonfinite=nonfinite)


def test_regime_classification():
    assert RangeReport().regime == "parity" and RangeReport().worst is None
    assert RangeReport([rec("a"), rec("b", 1, max_abs=464.0)]).regime == "parity"
    assert RangeReport([rec("a"), rec("b", 1, max_abs=500.0, cross=3)]).regime == "degraded"
    assert RangeReport([rec("a", cross=5), rec("b", 1, max_abs=65504.0, cross=1, clamped=1)]).regime == "clamped"
    assert RangeReport([rec("a", nonfinite=1)]).regime == "clamped"
    # the embedding of a resident layer is bounded on the host: beyond fp16 it counts as clamped, below it does not
    assert RangeReport([rec("a")], [rec("k", fmt=_lib.RANGE_FORMAT_EMBED, max_abs=65504.0, total=0)]).regime == "parity"
    assert RangeReport([rec("a")], [rec("k", fmt=_lib.RANGE_FORMAT_EMBED, max_abs=7e4, total=0)]).regime == "clamped"


def test_report_text_names_the_worst_tensor_layer_and_counts():
    r = RangeReport([rec("ws.gen.rb4.a1", 30), rec("ws.gen.rb5.a1", 41, max_abs=2000.0, cross=17),
                     rec("ws.gen.rb5.a2", 47, max_abs=470.0, cross=2)], layers={41: "gen.rb5.spade_1.gb.kernel"})
    assert r.worst["tensor"] == "ws.gen.rb5.a1" and r.flagged() == ["ws.gen.rb5.a1", "ws.gen.rb5.a2"]
    text = str(r)
    for word in ("degraded", "ws.gen.rb5.a1", "op 41", "gen.rb5.spade_1.gb.kernel", "17 cross-clipped", "0 clamped",
                 "0 non-finite", "2000", "2 of 3 tensors"):
        assert word in text, (word, text)
    assert "parity" in str(RangeReport())
    # a clamped tensor outranks one with more clipped cross pieces
    assert RangeReport([rec("a", cross=100), rec("b", 1, cross=1, clamped=1)]).worst["tensor"] == "b"


def test_cross_limit_is_464_from_e4m3_rounding():
    """e4m3's grid ends 416, 448 and would continue with 480: under round-to-nearest-even 448 takes everything up to the
    midpoint 464, tie included (448 = 1.75 * 2^8 has the even mantissa), so the saturation at 448 changes nothing up to there."""
    lim = ops.e4m3_cross_limit()
    assert lim == 464.0
    nxt = float(np.nextafter(np.float16(lim), np.float16(np.inf)))
    assert nxt == 464.25
    f8 = lambda v: float(torch.tensor([v]).to(torch.float8_e4m3fn).float())     # noqa: E731
    assert f8(448.0) == 448.0 and f8(lim) == 448.0 and f8(432.0) in (416.0, 448.0)
    assert not f8(nxt) == 448.0                      # no 480 in e4m3fn: the unsaturated conversion overflows
    # pinned against the image builder: up to the limit its h8 piece IS the unsaturated rounding, above it the clip acts
    x = torch.zeros(1, 1, 1, 32)
    x[0, 0, 0, :4] = torch.tensor([448.0, lim, nxt, -nxt])
    h8 = ops.f16c_activation_image(x)[1][1][0, 0, 0]
    assert h8[:4].tolist() == [448.0, 448.0, 448.0, -448.0]
    st = ops.range_stats(ops.f16c_activation_image(x)[0], 4, False)
    assert st["n_cross_clipped"] == 2 and st["n_clamped"] == 0 and st["max_abs"] == np.float32(nxt)


def planted(shape=(1, 2, 2, 32)):
    x = torch.zeros(shape)
    x[0, 0, 0, :8] = torch.tensor([448.0, -464.0, 464.25, 512.0, -1000.0, 65504.0, -65504.0, 30.0])
    return x


@pytest.mark.parametrize("fmt", [2, 4, 5])
def test_range_stats_on_a_hand_made_fp16_image(fmt):
    x = planted()
    img = {2: ops.split_f16, 4: lambda t: ops.f16c_activation_image(t)[0], 5: lambda t: ops.f16c6_activation_image(t)[0]}[fmt](x)
    st = ops.range_stats(img, fmt, False)
    assert st == dict(max_abs=np.float32(65504.0), n_total=128, n_cross_clipped=5 if fmt == 4 else 0, n_clamped=2, n_nonfinite=0)
    # a zero border is left out, and an all-zero image counts its interior only
    st = ops.range_stats(ops.pad_nhwc(img), fmt, True)
    assert st["n_total"] == 128 and st["n_clamped"] == 2
    z = ops.range_stats(torch.zeros(2, 5, 5, 64), fmt, True)
    assert z == dict(max_abs=np.float32(0.0), n_total=2 * 3 * 3 * 64, n_cross_clipped=0, n_clamped=0, n_nonfinite=0)
    if fmt != 5:                                      # an infinity in the main piece: non-finite, not the maximum
        x[0, 1, 1, 3] = float("inf")
        img = ops.split_f16(x) if fmt == 2 else ops.f16c_activation_image(x)[0]
        st = ops.range_stats(img, fmt, False)
        assert st["n_nonfinite"] == 1 and st["max_abs"] == np.float32(65504.0)
        assert st["n_cross_clipped"] == (6 if fmt == 4 else 0)


def test_range_stats_on_a_hand_made_bf8_image():
    x = torch.zeros(1, 2, 2, 32)
    x[0, 0, 0, :5] = torch.tensor([57344.0, -57344.0, 49152.0, 1.5, -3.0])
    img, deq = ops.bf8_activation_image(x)                 # 32 channels in a 128-byte pixel
    assert img.shape[-1] == 128 and deq.abs().max() == 57344.0
    st = ops.range_stats(img, 3, False, channels=32)
    assert st == dict(max_abs=np.float32(57344.0), n_total=128, n_cross_clipped=0, n_clamped=2, n_nonfinite=0)
    img[0, 1, 1, 7] = 0xFC                                  # -inf in e5m2
    st = ops.range_stats(img, 3, False, channels=32)
    assert st["n_nonfinite"] == 1 and st["n_clamped"] == 2 and st["max_abs"] == np.float32(57344.0)
    with pytest.raises(ValueError):
        ops.range_stats(img, 1, False)


def test_auto_is_resolved_above_the_flag_table():
    assert "auto" not in _lib.PRECISION_FLAGS
    assert set(_lib.PRECISION_FLAGS) == {"fp32", "bf16x3", "bf16x3_gbf16", "fp8", "f16c", "f16"}


def test_library_without_the_range_entries_is_a_clear_error():
    new = {"msr_range_scan", "msr_range_read", "msr_range_embed_bounds", "msr_op_range_scan"}
    assert new <= {name for name, _, _ in _lib.SYMBOLS}

    class Fn:
        restype = argtypes = None

    class OldLibrary:                                   # every symbol of the ABI except the new entries
        def __getattr__(self, name):
            if name in new or not name.startswith("msr_"):
                raise AttributeError(name)
            fn = Fn()
            self.__dict__[name] = fn
            return fn

    with pytest.raises(RuntimeError) as e:
        _lib.bind(OldLibrary(), "/somewhere/libmoonsr_hip.so")
    for name in new:
        assert name in str(e.value)
    assert "rebuild" in str(e.value) and "/somewhere/libmoonsr_hip.so" in str(e.value)
    full = OldLibrary()
    new.clear()
    assert _lib.bind(full, "x") is full and full.msr_range_scan.argtypes == [_lib._P, _lib._P]

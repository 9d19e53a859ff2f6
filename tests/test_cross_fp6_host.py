"""Host side of the f16c mode's opt-in fp6 cross terms (Generator(cross=...), MSR_FLAG_CROSS_FP6): the flag table and the
argument checks, which come before the device or the library is touched.  No GPU."""
import pytest

from moonsuperresolution_amd import Generator, _lib


def test_cross_flags():
    assert _lib.CROSS_FLAGS == {"fp8": 0, "fp6": 32}
    # the cross format is an option of f16c, not a precision of its own
    assert _lib.PRECISION_FLAGS == {"fp32": 0, "bf16x3": 1, "bf16x3_gbf16": 3, "fp8": 5, "f16c": 9, "f16": 25}
    assert all(v & 32 == 0 for v in _lib.PRECISION_FLAGS.values())
    assert "msr_op_spade_gbr_f16c6" in [name for name, _, _ in _lib.SYMBOLS]


@pytest.mark.parametrize("kw", [dict(precision="bf16x3", cross="fp6"), dict(precision="f16", cross="fp6"),
                                dict(precision="fp32", cross="fp6"), dict(cross="fp4"), dict(precision="auto", cross="fp4")])
def test_cross_argument_is_checked_before_the_device(kw, monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError, match="cross"):
        Generator(64, 2, **kw)

"""CPU: the host side of the dirty-workspace tests (tests/test_gpu_dirty_workspace.py, tests/test_gpu_dirty_drivers.py).

  1. the patched torch.empty family yields the pattern, for every dtype the drivers allocate, strided and pinned-style
     keywords included, and puts the originals back on exit, also when the body raises;
  2. msr_debug_workspace_list and msr_debug_fill_workspace return MSR_ERR_INVALID for a null handle or a null output, before
     any device is asked for; both are in the symbol table, and a library without them is refused by name;
  3. the line parser of Generator.workspace_list on a literal sample, and the byte count of a fill worked out from it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd.generator import FILL_BORDER, FILL_INTERIOR, FILL_WORKSPACE, parse_conv_forms
from tests import dirty_cases as cases


# ---- 1. the patched empty -----------------------------------------------------------------------------------------------
def _all_pattern(t, byte=cases.PATTERN):
    return bool((cases.storage_bytes(t) == byte).all())


@pytest.mark.parametrize("dtype", cases.DRIVER_DTYPES, ids=str)
def test_dirty_empty_yields_the_pattern(monkeypatch, dtype):
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with cases.dirty_empty(monkeypatch) as count:
        assert torch.empty is not real[0] and torch.empty_like is not real[1] and torch.Tensor.new_empty is not real[2]
        a = torch.empty((3, 5), dtype=dtype)
        b = torch.empty(7, dtype=dtype, device="cpu")
        c = torch.empty_like(a)
        d = torch.empty_like(a.t())                      # strides preserved: the whole storage is filled
        e = a.new_empty((2, 2))
        f = torch.empty(0, dtype=dtype)                  # nothing to fill, nothing to fail
        for t in (a, b, c, d, e):
            assert t.dtype == dtype and _all_pattern(t)
        assert f.numel() == 0 and tuple(d.shape) == (5, 3)
        assert count["empty"] >= 2 and count["empty_like"] == 2 and count["new_empty"] == 1
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    if dtype.is_floating_point:
        assert torch.isnan(a).all()
    elif dtype != torch.uint8:
        assert (a == -1).all()                           # the kernels' own "no entry"
    else:
        assert (a == 255).all()


def test_dirty_empty_other_pattern_and_restore_on_error(monkeypatch):
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pytest.raises(RuntimeError, match="inside"):
        with cases.dirty_empty(monkeypatch, 0x47):
            t = torch.empty(16, dtype=torch.float32)
            assert _all_pattern(t, 0x47) and float(t[0]) == np.frombuffer(b"\x47" * 4, np.float32)[0]
            raise RuntimeError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    assert torch.empty(4).shape == (4,)


# ---- 2. the two entries -----------------------------------------------------------------------------------------------
def test_entries_refuse_null_arguments(hip_lib):
    buf = C.create_string_buffer(64)
    n = C.c_int64(-5)
    assert hip_lib.msr_debug_workspace_list(None, buf, len(buf)) == _lib.MSR_ERR_INVALID
    assert hip_lib.msr_debug_fill_workspace(None, FILL_WORKSPACE, 0xFF, C.byref(n)) == _lib.MSR_ERR_INVALID
    assert n.value == -5                                 # nothing was written
    # a non-null handle with a null output: refused before the handle is looked at (the pointer is never dereferenced)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(4096)))
    assert hip_lib.msr_debug_workspace_list(fake, None, 64) == _lib.MSR_ERR_INVALID
    assert hip_lib.msr_debug_workspace_list(fake, buf, 0) == _lib.MSR_ERR_INVALID
    assert hip_lib.msr_debug_fill_workspace(fake, FILL_WORKSPACE, 0xFF, None) == _lib.MSR_ERR_INVALID
    assert hip_lib.msr_abi_version() == 1                # entries are only ever added: the version stays


def test_library_without_the_new_entries_is_a_clear_error():
    new = {"msr_debug_workspace_list", "msr_debug_fill_workspace"}
    assert new <= {name for name, _, _ in _lib.SYMBOLS}

    class Fn:
        restype = argtypes = None

    class OldLibrary:                                    # every symbol of the ABI except the new entries
        def __getattr__(self, name):
            if name in new or not name.startswith("msr_"):
                raise AttributeError(name)
            fn = Fn()
            self.__dict__[name] = fn
            return fn

    with pytest.raises(RuntimeError) as e:
        _lib.bind(OldLibrary(), "/somewhere/libmoonsr_hip.so")
    assert all(name in str(e.value) for name in new) and "rebuild" in str(e.value)


# ---- 3. the parser ------------------------------------------------------------------------------------------------------
def test_workspace_list_parser_on_a_sample():
    entries = parse_conv_forms(cases.LIST_SAMPLE)
    assert [e["name"] for e in entries] == ["enc.ds2.kernel", "ws.enc.p1", "ws.gen.rb5.a1", "ws.enc.mean2", "ws.zero_bias",
                                            "scratch.mom_partial", "table.range_items", "table.blend_window"]
    assert [e["kind"] for e in entries] == ["weight", "ws", "ws", "ws", "ws", "scratch", "table", "table"]
    assert all(isinstance(e[k], int) for e in entries for k in ("bytes", "zeroed", "counted"))
    assert entries[1] == dict(name="ws.enc.p1", kind="ws", bytes=1183744, zeroed=1, counted=1, r=32, C=64, written=64)
    assert [("r" in e) for e in entries] == [False, True, True, False, False, False, False, False]
    assert sum(e["bytes"] for e in entries if e["counted"]) == sum(e["bytes"] for e in entries) - 25088
    # B = 4: 4 * 34 * 34 * 64 * 4 bytes is ws.enc.p1
    B = 4
    assert entries[1]["bytes"] == B * 34 * 34 * 64 * 4
    assert cases.fill_bytes(entries, B, FILL_WORKSPACE) == 2048 + 3145728           # un-zeroed ws + scratch; never weights, tables, zero_bias
    assert cases.fill_bytes(entries, B, FILL_INTERIOR) == B * 32 * 32 * (64 + 32) * 4
    assert cases.fill_bytes(entries, B, FILL_BORDER) == 2 * B * (34 * 34 - 32 * 32) * 64 * 4
    assert cases.fill_bytes(entries, B, 7) == sum(cases.fill_bytes(entries, B, w) for w in (1, 2, 4))
    assert (cases.FILL_WORKSPACE, cases.FILL_INTERIOR, cases.FILL_BORDER) == (FILL_WORKSPACE, FILL_INTERIOR, FILL_BORDER) == (1, 2, 4)

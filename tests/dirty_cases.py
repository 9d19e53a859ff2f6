"""Shared by the dirty-workspace tests (tests/test_gpu_dirty_workspace.py, tests/test_gpu_dirty_drivers.py and their host twin
tests/test_dirty_workspace_host.py): the patched ``torch.empty`` family, the parser's sample and the byte count of a fill.

A buffer that is "empty" holds whatever its block held before.  In a test process that is almost always zero; in a process
that has run for hours it is the previous owner's data.  ``dirty_empty`` makes the second case the deterministic one: every
tensor that ``torch.empty``, ``torch.empty_like`` or ``Tensor.new_empty`` returns inside the context has all bytes of its
storage set to 0xFF: a NaN in every float format, -1 (the kernels' own "no entry") in every signed integer table.
"""
import contextlib

import torch

FILL_WORKSPACE, FILL_INTERIOR, FILL_BORDER = 1, 2, 4
PATTERN = 0xFF

# dtypes of the torch.empty / empty_like / new_empty calls in tiler.py, halo.py, geotiff.py, preprocess.py and infill.py
DRIVER_DTYPES = (torch.float32, torch.float64, torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)

# msr_debug_workspace_list of a small handle, cut to one line of every shape a line takes
LIST_SAMPLE = """\
name=enc.ds2.kernel kind=weight bytes=294912 zeroed=0 counted=1
name=ws.enc.p1 kind=ws bytes=1183744 zeroed=1 counted=1 r=32 C=64 written=64
name=ws.gen.rb5.a1 kind=ws bytes=1183744 zeroed=1 counted=1 r=32 C=64 written=32
name=ws.enc.mean2 kind=ws bytes=2048 zeroed=0 counted=1
name=ws.zero_bias kind=ws bytes=8192 zeroed=1 counted=1
name=scratch.mom_partial kind=scratch bytes=3145728 zeroed=0 counted=1
name=table.range_items kind=table bytes=400 zeroed=0 counted=1
name=table.blend_window kind=table bytes=25088 zeroed=0 counted=0
"""


def fill_bytes(entries, batch_size, what):
    """The bytes msr_debug_fill_workspace(what, .) must report, from the workspace list alone."""
    total = 0
    for e in entries:
        if what & FILL_WORKSPACE and (e["kind"] == "scratch" or (e["kind"] == "ws" and not e["zeroed"])):
            total += e["bytes"]
        if "r" in e:
            r, c, w = e["r"], e["C"], e["written"]
            if what & FILL_INTERIOR:
                total += batch_size * r * r * w * 4
            if what & FILL_BORDER:
                total += batch_size * ((r + 2) ** 2 - r * r) * c * 4
    return total


def storage_bytes(t):
    """The whole storage of ``t`` as a flat uint8 tensor that aliases it."""
    st = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),))


@contextlib.contextmanager
def dirty_empty(monkeypatch, byte=PATTERN):
    """Inside: torch.empty, torch.empty_like and Tensor.new_empty return tensors whose bytes are all ``byte`` (device, host and
    pinned host alike).  The originals are back on exit.  Yields a dict that counts the poisoned tensors per call."""
    real = {"empty": torch.empty, "empty_like": torch.empty_like, "new_empty": torch.Tensor.new_empty}
    count = {"empty": 0, "empty_like": 0, "new_empty": 0}

    def poisoned(name):
        fn = real[name]

        def call(*a, **kw):
            t = fn(*a, **kw)
            if isinstance(t, torch.Tensor) and t.untyped_storage().nbytes() and t.device.type != "meta":
                storage_bytes(t).fill_(byte)
                count[name] += 1
            return t
        call.__name__ = name
        return call

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", poisoned("empty"))
        m.setattr(torch, "empty_like", poisoned("empty_like"))
        m.setattr(torch.Tensor, "new_empty", poisoned("new_empty"))
        yield count

"""GPU (-m gpu): a forward's result is a function of its inputs and the weights only.

Every other test of the planned network runs on a workspace whose unwritten words are zero: a handle's hipMalloc'ed buffers
read as zero in a fresh process, the zero-bordered buffers are zero by construction.  A kernel that reads a word its producer
never wrote (a masked tile tail of the moments slabs, a split-K partial row beyond M, the unused bytes of an f16c6 chunk, a
pixel that none of pix2pix's four parity launches covers) is right there and wrong in a process whose allocator recycles
blocks.  Here everything a forward is entitled to overwrite is filled with a byte pattern first (msr_debug_fill_workspace:
the un-zeroed ws.* buffers, the four scratch buffers, the interior of the zero-bordered buffers), and the forward must give the
bits it gave on the clean handle.  Per configuration:

  1. control, determinism: forward(x1) twice, equal bits (without it nothing below means anything);
  2. for byte in (0xFF, 0x47): fill, forward(x1): the output, last_latent() and every ws.*mean* / ws.*std* buffer equal the
     clean run's; forward(x2) without another fill equals a FRESH handle's forward(x2), taken as this handle's very first call
     (nothing carries over from x1);
  3. graph replay: capture on the second sighting, fill, replay: the same bits;
  4. after the dirty runs the border of every zero-bordered buffer, and every slot beyond the written count, is all zero bits;
  5. narrow-image configurations: range_report after a dirty forward equals the clean one, n_nonfinite == 0;
  6. control, the comparison can fail (one configuration per precision): the borders filled with 0x47 change the output (the
     convs do read them), filled with 0x00 again the clean bits are back.  0x47 is finite in every format: pure arithmetic;
  7. control, the poison arrives: after a fill a zeroed=0 buffer read back is the pattern, and bytes_filled is the sum
     worked out from workspace_list(), which also accounts for device_bytes().

0xFF is a NaN in fp32, fp16, bf16, e4m3, e5m2 and e8m0 at once; 0x47 is finite and non-zero in each (fp32 5.1e4, fp16 7.3,
e4m3 3.75, e5m2 7) and catches the stale value that a NaN-dropping min / max / clamp swallows.  No tolerance anywhere: every
comparison is bit equality between two runs of the same code.

The configurations are those of tests/test_gpu_network_sites.py (the same REQUIRED_FORMS coverage is asserted here), the
fused head, the fp6 cross terms, the no-KL variant at (64, 2) and pix2pix at B = 3.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.dirty_cases import FILL_BORDER, FILL_INTERIOR, FILL_WORKSPACE, fill_bytes
from tests.test_gpu_network_sites import CONFIGS, REQUIRED_FORMS, form_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRTY = FILL_WORKSPACE | FILL_INTERIOR
BYTES = (0xFF, 0x47)

# (variant, S, B, precision, extra keywords, MSR_F16C_FP6)
CASES = [("gaugan", S, B, p, {}, fp6) for S, B, p, fp6 in CONFIGS] + [
    ("gaugan", 128, 16, "f16c", {"head": "fused"}, 0),
    ("gaugan", 128, 16, "f16c", {"cross": "fp6"}, 0),
    ("gaugan_no_kl", 64, 2, "f16c", {}, 0),
    ("pix2pix", 256, 3, "fp32", {}, 0),
]
# step 6 runs once per precision, on the first (smallest where there is a choice) configuration of it
BORDER_CONTROL = {("gaugan", 128, 3, "f16c"), ("gaugan", 256, 4, "bf16x3"), ("gaugan", 256, 2, "fp32"), ("gaugan", 256, 16, "f16"),
                  ("gaugan", 256, 16, "fp8"), ("gaugan", 256, 16, "bf16x3_gbf16"), ("pix2pix", 256, 3, "fp32")}
_SEEN_FORMS = set()
_WEIGHTS = {}


def case_id(c):
    variant, S, B, p, kw, fp6 = c
    return "-".join([variant, str(S), str(B), p] + [f"{k}_{v}" for k, v in kw.items()] + (["fp6env"] if fp6 else []))


def _weights(variant, S):
    from moonsuperresolution_amd import make_weights
    if (variant, S) not in _WEIGHTS:
        _WEIGHTS.clear()                                 # one set at a time: the (512, .) set alone is several hundred MB
        _WEIGHTS[variant, S] = make_weights(variant, S, seed=1234, bias_scale=0.05)
    return _WEIGHTS[variant, S]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Handle:
    """A Generator with fixed eps, its device input buffers and the reads the comparisons need."""

    def __init__(self, variant, S, B, precision, kw):
        from moonsuperresolution_amd import Generator, make_latent_noise
        eps = make_latent_noise(B, 256, 7) if variant == "gaugan" else None
        self.gen = Generator(S, B, variant=variant, weights=_weights(variant, S), eps=eps, precision=precision, **kw)
        self.variant, self.S, self.B = variant, S, B

    def forward(self, x, out=None):
        y = self.gen.forward_device(x, out=out)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    def moments(self):
        return {e["name"]: self.gen.debug_tensor(e["name"], (e["bytes"] // 4,)) for e in self.gen.workspace_list()
                if e["kind"] == "ws" and ("mean" in e["name"] or "std" in e["name"])}

    def state(self):
        """latent and moments of the last forward"""
        st = self.moments()
        if self.variant != "pix2pix":
            st["last_latent"] = self.gen.last_latent()
        return st

    def close(self):
        self.gen.close()


def check_zero_regions(h, smallest_only=False):
    """Step 4: borders and unwritten slots of every zero-bordered buffer (the border control: of the smallest one) -> names of the
    buffers that hold a non-zero bit."""
    bad = []
    padded = [e for e in h.gen.workspace_list() if "r" in e]
    assert padded
    for e in [min(padded, key=lambda e: e["bytes"])] if smallest_only else padded:
        assert e["zeroed"] == 1 and e["bytes"] == h.B * (e["r"] + 2) ** 2 * e["C"] * 4, e
        t = bits(h.gen.debug_tensor(e["name"], (h.B, e["r"] + 2, e["r"] + 2, e["C"])))
        if t[:, 0].any() or t[:, -1].any() or t[:, :, 0].any() or t[:, :, -1].any():
            bad.append(e["name"] + " border")
        if e["written"] < e["C"] and t[..., e["written"]:].any():
            bad.append(e["name"] + " slots beyond written")
    return bad


def check_poison_arrived(h, entries, byte):
    """Step 7: every un-zeroed ws buffer of at most 1 MiB and the largest one read back as the pattern; the smallest zero-bordered
    buffer holds it in the written slots of its interior and zero bits everywhere else."""
    dirty = [e for e in entries if e["kind"] == "ws" and not e["zeroed"] and e["bytes"] >= 4]
    assert dirty
    largest = max(dirty, key=lambda e: e["bytes"])
    for e in dirty:
        if e["bytes"] <= 1 << 20 or e is largest:
            got = h.gen.debug_tensor(e["name"], (e["bytes"] // 4,)).view(np.uint8)
            assert (got == byte).all(), (e["name"], hex(byte))
    padded = [e for e in entries if "r" in e]
    e = min(padded, key=lambda e: e["bytes"])
    t = h.gen.debug_tensor(e["name"], (h.B, e["r"] + 2, e["r"] + 2, e["C"])).view(np.uint8).reshape(h.B, e["r"] + 2, e["r"] + 2, -1)
    assert (t[:, 1:-1, 1:-1, :4 * e["written"]] == byte).all(), e["name"]
    assert not t[:, 0].any() and not t[:, -1].any() and not t[:, :, 0].any() and not t[:, :, -1].any(), e["name"]
    assert not t[..., 4 * e["written"]:].any(), e["name"]


def run_case(variant, S, B, precision, kw):
    from moonsuperresolution_amd import synthetic_patches
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda")
    x1 = torch.from_numpy(synthetic_patches(B, S, 0)).to(dev)
    x2 = torch.from_numpy(synthetic_patches(B, S, 5)).to(dev)
    h = Handle(variant, S, B, precision, kw)
    try:
        y2_fresh = h.forward(x2)                         # the first call of a fresh handle: what forward(x2) gives with no history
        forms = {form_of(op) for op in h.gen.conv_forms() if op["kind"] not in ("moments", "moments_slabs")}
        # 1. determinism
        clean = h.forward(x1)
        assert np.isfinite(clean).all()
        assert same_bits(h.forward(x1), clean), "two clean forwards of the same input differ: nothing below would mean anything"
        assert not same_bits(clean, y2_fresh)            # x1 and x2 can be told apart
        clean_state = h.state()
        if kw.get("head") == "fused":
            assert h.gen.head_fused
        if variant != "pix2pix":                         # 4 x 2 encoder, 2 + 6 x 4 generator moments buffers, the latent; the
            fused = kw.get("head") == "fused"            # fused head has no moments of the last block's output
            assert len(clean_state) == (33 if fused else 35), sorted(clean_state)
        if kw.get("cross") == "fp6":
            assert any(op.get("prec") == 5 for op in h.gen.conv_forms() if op["kind"] == "conv")
        report = h.gen.range_report() if variant != "pix2pix" else None
        narrow = report is not None and len(report.records) > 0
        if variant == "gaugan" and S >= 128:             # the site configurations: every quantised mode plans narrow images there
            assert narrow == (precision not in ("fp32", "bf16x3"))
        # 7. the list accounts for the handle's memory, and says what a fill writes
        entries = h.gen.workspace_list()
        assert sum(e["bytes"] for e in entries if e["counted"]) == h.gen.device_bytes()
        assert len({e["name"] for e in entries}) == len(entries)
        assert {e["kind"] for e in entries} <= {"ws", "scratch", "weight", "table"}
        if variant != "pix2pix":
            assert {"scratch.mom_partial", "scratch.dense_partial"} <= {e["name"] for e in entries}
        want_bytes = fill_bytes(entries, B, DIRTY)
        assert want_bytes > 0
        # 2. dirty runs
        for byte in BYTES:
            assert h.gen.fill_workspace(DIRTY, byte) == want_bytes
            check_poison_arrived(h, entries, byte)
            y = h.forward(x1)
            assert same_bits(y, clean), f"output differs after a 0x{byte:02X} fill: {int((bits(y) != bits(clean)).sum())} words"
            state = h.state()
            assert state.keys() == clean_state.keys()
            differ = [k for k in state if not same_bits(state[k], clean_state[k])]
            assert not differ, (hex(byte), differ)
            if narrow:                                   # 5. range scan of the dirty forward
                rep = h.gen.range_report()
                assert rep.records == report.records and rep.embed_bounds == report.embed_bounds, hex(byte)
                assert all(r["n_nonfinite"] == 0 for r in rep.records)
            y2 = h.forward(x2)
            assert same_bits(y2, y2_fresh), f"forward(x2) after a dirty forward(x1) is not a fresh handle's (0x{byte:02X})"
        bad = check_zero_regions(h)                      # 4. after the dirty runs
        assert not bad, bad
        # 3. graph replay
        h.gen.use_graph(True)
        st = torch.cuda.Stream()
        out = torch.zeros((B, S, S, 1), dtype=torch.float32, device=dev)
        with torch.cuda.stream(st):
            h.forward(x1, out=out)                       # first sighting: eager
            assert same_bits(h.forward(x1, out=out), clean)   # second: captured and launched
            for byte in BYTES:
                assert h.gen.fill_workspace(DIRTY, byte) == want_bytes
                out.fill_(float("nan"))
                st.synchronize()
                assert same_bits(h.forward(x1, out=out), clean), f"graph replay differs after a 0x{byte:02X} fill"
                state = h.state()
                differ = [k for k in state if not same_bits(state[k], clean_state[k])]
                assert not differ, ("replay", hex(byte), differ)
        h.gen.use_graph(False)
        # 6. the comparison can fail: the convs read their borders
        if (variant, S, B, precision) in BORDER_CONTROL and not kw:
            assert h.gen.fill_workspace(FILL_BORDER, 0x47) == fill_bytes(entries, B, FILL_BORDER) > 0
            assert check_zero_regions(h, smallest_only=True)
            assert not same_bits(h.forward(x1), clean), "0x47 in every border left the output as it was: the control shows nothing"
            h.gen.fill_workspace(FILL_BORDER, 0x00)
            assert not check_zero_regions(h, smallest_only=True)
            assert same_bits(h.forward(x1), clean), "zeroed borders did not bring the clean bits back"
    finally:
        h.close()
        torch.cuda.empty_cache()
    return forms


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dirty_workspace_same_bits(hip_lib, tmp_path, case):
    variant, S, B, precision, kw, fp6 = case
    if fp6 and os.environ.get("MSR_F16C_FP6") != "1":
        # MSR_F16C_FP6 is read once per process: this configuration runs in a child, which hands its forms back in a file
        path = str(tmp_path / "forms.json")
        env = dict(os.environ, MSR_F16C_FP6="1", DIRTY_WORKSPACE_FORMS_FILE=path)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k",
                            f"test_dirty_workspace_same_bits and {case_id(case)}"], env=env, capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
        _SEEN_FORMS.update(tuple(f) for f in json.load(open(path)))
        return
    forms = run_case(variant, S, B, precision, kw)
    if variant == "gaugan" and not kw:
        _SEEN_FORMS.update(forms)
    if os.environ.get("DIRTY_WORKSPACE_FORMS_FILE"):
        json.dump(sorted(list(f) for f in forms), open(os.environ["DIRTY_WORKSPACE_FORMS_FILE"], "w"))


@pytest.mark.gpu
def test_every_required_form_ran_dirty():
    """Runs after the parametrised test: the configurations of tests/test_gpu_network_sites.py, run dirty, must have planned
    every form of its REQUIRED_FORMS."""
    if len(_SEEN_FORMS) == 0:
        pytest.fail("the dirty-workspace test did not run first")
    assert REQUIRED_FORMS <= _SEEN_FORMS, sorted(REQUIRED_FORMS - _SEEN_FORMS)


def test_cases_cover_the_site_configurations():
    """CPU: the case list holds every configuration of the site test, and the four the issue adds; the fused-head and fp6 cases
    plan those forms at their (small) shapes, which needs no GPU to check."""
    from moonsuperresolution_amd import _lib
    from moonsuperresolution_amd.generator import form_table
    assert [(c[1], c[2], c[3], c[5]) for c in CASES[:len(CONFIGS)]] == CONFIGS
    assert {case_id(c) for c in CASES[len(CONFIGS):]} == {"gaugan-128-16-f16c-head_fused", "gaugan-128-16-f16c-cross_fp6",
                                                          "gaugan_no_kl-64-2-f16c", "pix2pix-256-3-fp32"}
    assert len({case_id(c) for c in CASES}) == len(CASES)
    assert {p for _, _, _, p in BORDER_CONTROL} >= {c[3] for c in CASES}
    assert all(any((c[0], c[1], c[2], c[3]) == b and not c[4] for c in CASES) for b in BORDER_CONTROL)
    f16c = _lib.PRECISION_FLAGS["f16c"]
    assert form_table(128, 16, "gaugan", f16c | _lib.HEAD_FLAGS["fused"])["head_fused"] == 1
    fp6 = form_table(128, 16, "gaugan", f16c | _lib.CROSS_FLAGS["fp6"])
    assert any(v["prec"] == 5 for k, v in fp6.items() if k != "head_fused" and "prec" in v and k.endswith(("conv_1", "conv_2", "conv_3")))

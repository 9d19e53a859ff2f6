"""CPU: the form table (csrc/forms.hip: the kernel, tile, K split and weight image of every conv layer; the resident kernel's
ranges; the fused head) of every configuration under every documented kernel switch, against tests/golden/form_table.json.

msr_debug_form_table needs no device: it runs msr_create's validation and fill_forms on a local handle and prints the table.
The fixture holds the SHA-256 of that text as the commit named in it produced it (tests/golden/make_golden.py says how), for
S in {64, 128, 256, 512} x B in {1, 2, 3, 4, 8, 12, 16} x eight flag sets, plus pix2pix at 256, under nine environments.  The
switches are read once per process, so every environment runs in a child: this file as a script, which prints its tables
as JSON.  A mismatch prints the table the library gave (and, where the fixture has it, the expected text).
"""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "form_table.json")
PREC_F16C, TILE_PP, EPI_BIAS, EPI_RES, EPI_SPADE = 4, 5, 0, 1, 2


def _lib_module():
    """moonsuperresolution_amd/_lib.py alone (ctypes only): a child needs neither torch nor the package."""
    spec = importlib.util.spec_from_file_location("msr_lib_only", os.path.join(ROOT, "moonsuperresolution_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _table(mod, lib, S, B, variant, flags):
    cfg = mod.MsrConfig(S, B, 256, variant, 0, flags)
    buf = C.create_string_buffer(1 << 14)
    rc = lib.msr_debug_form_table(C.byref(cfg), buf, len(buf))
    assert rc == mod.MSR_OK, (S, B, variant, flags, rc, lib.msr_last_error(None))
    return buf.value.decode()


def _f16c_kernel_disagreements(lib, text):
    """Every whole-tile PREC_F16C line of a table -> the lines whose kernel word is not what msr_debug_f16c_kernel answers."""
    words = {ln.split()[0]: dict(w.split("=") for w in ln.split()[1:]) for ln in text.splitlines()[:-1]}
    bad = []
    for name, w in words.items():
        if "prec" not in w or int(w["prec"]) != PREC_F16C or int(w["ksplit"]) > 1 or int(w["tile"]) != TILE_PP:
            continue
        if name.endswith(".gb"):
            cin, epi, out_mode = 128, EPI_SPADE, int(words[name[:-3]]["a_split"])
        else:
            layer, j = name.rsplit(".conv_", 1)
            cin, epi, out_mode = int(words[f"{layer}.spade_{j}"]["aslots"]), EPI_RES if j == "2" else EPI_BIAS, 0
        want = "sw" if lib.msr_debug_f16c_kernel(cin, epi, out_mode) else "pp"
        if w["kernel"] != want:
            bad.append((name, w["kernel"], want))
    return bad


def _child():
    """stdout: {"tables": {flag set: {S: [text per batch]}}, "f16c_kernel_disagreements": [...]} of this process's environment"""
    mod = _lib_module()
    lib = mod.bind(C.CDLL(os.environ.get("MSR_LIB", mod.LIB_PATH)), "libmoonsr_hip.so")
    gold = json.load(open(GOLDEN))
    tables, bad = {}, []
    for name, flags in gold["flag_sets"].items():
        for S in gold["sizes"]:
            tables.setdefault(name, {})[str(S)] = [_table(mod, lib, S, B, 0, flags) for B in gold["batches"]]
            for B, text in zip(gold["batches"], tables[name][str(S)]):
                bad += [(name, S, B) + d for d in _f16c_kernel_disagreements(lib, text)]
    tables["pix2pix"] = {"256": [_table(mod, lib, 256, B, 3, 0) for B in gold["batches"]]}
    json.dump({"tables": tables, "f16c_kernel_disagreements": bad}, sys.stdout)


GOLD = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {"envs": {}}


@pytest.mark.parametrize("env_name", sorted(GOLD["envs"]))
def test_form_table_matches_the_golden_digests(hip_lib, env_name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSR_") or k == "MSR_LIB"}
    env.update(GOLD["envs"][env_name])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(r.stdout)
    want = GOLD["digests"][env_name]
    assert set(got["tables"]) == set(want) and len(want) == len(GOLD["flag_sets"]) + 1
    n = 0
    for name, by_size in want.items():
        assert set(got["tables"][name]) == set(by_size)
        for S, digests in by_size.items():
            for B, digest, text in zip(GOLD["batches"], digests, got["tables"][name][S]):
                n += 1
                if hashlib.sha256(text.encode()).hexdigest() != digest:
                    print(f"form table of {name} S={S} B={B} under {GOLD['envs'][env_name]}:\n{text}")
                    expected = GOLD["f16c_texts"].get(f"{S},{B}") if (env_name, name) == ("none", "f16c") else None
                    if expected:
                        print("expected:\n" + expected)
                    pytest.fail(f"form table of {name} S={S} B={B} under {env_name} differs from the golden digest")
    assert n == len(GOLD["sizes"]) * len(GOLD["batches"]) * len(GOLD["flag_sets"]) + len(GOLD["batches"])
    assert got["f16c_kernel_disagreements"] == []


def test_golden_full_texts_match_their_digests():
    """the readable copies in the fixture are the texts its digests were taken from"""
    assert sorted(GOLD["f16c_texts"]) == ["128,3", "256,16", "512,12", "512,8", "64,2"]
    for key, text in GOLD["f16c_texts"].items():
        S, B = key.split(",")
        assert hashlib.sha256(text.encode()).hexdigest() == GOLD["digests"]["none"]["f16c"][S][GOLD["batches"].index(int(B))]


def test_form_table_rejects_what_create_rejects(hip_lib):
    from moonsuperresolution_amd import _lib
    BF, GB, FP8, F16C, F16M, X6, HEAD = 1, 2, 4, 8, 16, 32, 64
    bad = [(100, 2, 256, 0, 0), (32, 2, 256, 0, 0), (64, 0, 256, 0, 0), (64, 17, 256, 0, 0), (64, 2, 256, 9, 0), (64, 2, 6, 0, 0),
           (128, 1, 256, 3, 0), (64, 2, 256, 0, GB), (64, 2, 256, 0, FP8), (64, 2, 256, 0, BF | GB | FP8), (64, 2, 256, 0, F16C),
           (64, 2, 256, 0, BF | F16C | FP8), (64, 2, 256, 0, BF | F16C | GB), (64, 2, 256, 0, BF | F16M),
           (64, 2, 256, 0, BF | X6), (64, 2, 256, 0, BF | F16C | F16M | X6), (64, 2, 256, 0, BF | HEAD),
           (64, 2, 256, 0, BF | F16C | HEAD | F16M), (64, 2, 256, 0, BF | F16C | HEAD | X6), (256, 2, 256, 3, BF | F16C | HEAD)]
    buf = C.create_string_buffer(1 << 14)
    h = C.c_void_p()
    for S, B, L, variant, flags in bad:
        cfg = _lib.MsrConfig(S, B, L, variant, 0, flags)
        assert hip_lib.msr_create(C.byref(cfg), C.byref(h)) == _lib.MSR_ERR_INVALID and not h.value, (S, B, L, variant, flags)
        why = hip_lib.msr_last_error(None)
        assert hip_lib.msr_debug_form_table(C.byref(cfg), buf, len(buf)) == _lib.MSR_ERR_INVALID, (S, B, L, variant, flags)
        assert hip_lib.msr_last_error(None) == why
    cfg = _lib.MsrConfig(64, 2, 256, 0, 0, BF | F16C)
    assert hip_lib.msr_debug_form_table(C.byref(cfg), buf, 16) == _lib.MSR_ERR_INVALID         # cap too small
    assert hip_lib.msr_debug_form_table(C.byref(cfg), buf, len(buf)) == _lib.MSR_OK
    assert buf.value.decode().splitlines()[-1] == "head_fused=0"


if __name__ == "__main__":
    _child()

#!/usr/bin/env python3
"""Compare the kernels of two sets of gfx950 device ELFs, symbol by symbol (a refactor's "same machine code" check).

    hipcc --offload-arch=gfx950 <flags of csrc/Makefile> --cuda-device-only --no-gpu-bundle-output -c X.hip -o X.elf
    tools/isa_compare.py --a old/*.elf --b new/*.elf [--out table.txt]

A kernel may sit in a different file on the two sides.  Per kernel: the resource numbers of its metadata note (vgpr, agpr,
sgpr, private and group segment bytes), its code bytes, and whether the disassembly (addresses and address comments stripped)
is the same text.  Exit status 1 when the name sets or any kernel differ.  Needs no GPU.
"""
import argparse
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels_of(path):
    """{kernel symbol: (five numbers, code bytes, instruction text)}"""
    meta, cur = {}, None
    for line in run(LLVM + "llvm-readelf", "--notes", path).splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'\"")
        if line.startswith("  - ."):
            cur = {}                                    # an entry of amdhsa.kernels: a list item at two spaces
        if cur is None:
            continue
        if key == ".symbol":
            meta[val[:-3] if val.endswith(".kd") else val] = cur
        elif key in FIELDS:
            cur[key] = int(val)
    sizes = {}
    for line in run(LLVM + "llvm-readelf", "-s", "--wide", path).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            sizes[f[7]] = int(f[2], 0)
    text, sym = {}, None
    for line in run(LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", path).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1)
            text[sym] = []
        elif sym and line.strip() and line.strip() != "...":     # "...": zero padding behind a file's last symbol
            text[sym].append(line.split("//")[0].strip())
    out = {}
    for name, res in meta.items():
        out[name] = (tuple(res.get(k, 0) for k in FIELDS), sizes.get(name, 0), "\n".join(text.get(name, [])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--out")
    args = ap.parse_args()
    side = []
    for files in (args.a, args.b):
        ks = {}
        for f in files:
            for name, v in kernels_of(f).items():
                if name in ks:
                    sys.exit("kernel %s appears twice on one side" % name)
                ks[name] = v
        side.append(ks)
    a, b = side
    lines = ["%-6s %5s %5s %5s %8s %8s %8s  %s" % ("same", "vgpr", "agpr", "sgpr", "private", "group", "bytes", "kernel")]
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            lines.append("%-6s %s" % ("only-a" if name in a else "only-b", name))
            bad += 1
            continue
        same = a[name] == b[name]
        bad += not same
        for tag, v in (("yes", b[name]),) if same else (("no:a", a[name]), ("no:b", b[name])):
            lines.append("%-6s %5d %5d %5d %8d %8d %8d  %s" % ((tag,) + v[0] + (v[1], name)))
    lines.append("%d kernels, %d differ or are missing on one side" % (len(set(a) | set(b)), bad))
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

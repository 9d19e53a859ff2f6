"""Diagnostic (not a pytest): GeoTIFF reading with the host and with the device decoder, on one GPU.
    python3 tools/gpu_geotiff_decode_bench.py [--out profiles/geotiff_decode.json] [--limit 600] [--repeats 3]
Four LZW + PREDICTOR=2 files of the products of tools/gpu_geotiff_encode_bench.py: the 4096 x 16384 float32 DEM-like raster
as strips (one 64 KiB strip per row) and as 256 x 256 tiles, 2048 rows of 70000 float32 samples (the width of BASELINE
configs[3]: one 280000-byte strip per row), and the 4096 x 16384 uint16 `good`-like raster.  For each, in one process: the wall
time of geotiff.read_geotiff with decoder="host" (csrc/host_codecs.cpp, block after block, single-threaded) and with
decoder="device" (csrc/geotiff_codec.hip; gather, upload, two launches per band, download of the float32 raster included),
the two alternating --repeats times so that the spread is on file; whether the two rasters are the same bits (they must
be); and the phases of one device read of the whole file in one band, each on its own: allocating pinned memory, gathering
the compressed blocks into it, the upload, the decode launch and the placement launch between HIP events (as GB/s of decoded
bytes), the download to a pageable array (what read_geotiff does) and to freshly allocated pinned memory.

Without --case the script touches no GPU itself: it runs each case as a child process under a time limit of its own and
stops at the first one that fails or runs out of time."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gpu_geotiff_encode_bench import product          # noqa: E402  (the same data as the encode bench)

CASES = {"dem_f32_strips": (4096, 16384, "f32", None), "dem_f32_tiles256": (4096, 16384, "f32", 256),
         "wide_f32_strips": (2048, 70000, "f32", None), "good_u16_strips": (4096, 16384, "u16", None)}


def write_tiled(path, data, tile, dev):
    """A little-endian classic TIFF of ``data`` in tile x tile LZW tiles with PREDICTOR=2, the tiles encoded on the device."""
    import struct
    import torch
    from moonsuperresolution_amd import geotiff as G
    rows, cols = data.shape
    down, across = -(-rows // tile), -(-cols // tile)
    padded = np.zeros((down * tile, across * tile), data.dtype)
    padded[:rows, :cols] = data
    major = np.ascontiguousarray(padded.reshape(down, tile, across, tile).transpose(0, 2, 1, 3))      # tile after tile
    nbytes = tile * tile * data.dtype.itemsize
    buf = torch.from_numpy(major.view(np.uint8).reshape(-1)).to(dev)
    n = down * across
    tiles = G.lzw_encode_device(buf, np.arange(n, dtype=np.int64) * nbytes, [nbytes] * n, data.dtype.itemsize,
                                tile * data.dtype.itemsize)
    pos, offs = 8, []
    for t in tiles:
        offs.append(pos)
        pos += len(t) + (len(t) & 1)
    short = lambda v: (3, 1, struct.pack("<HH", v, 0))                        # noqa: E731
    ent = {256: (4, 1, struct.pack("<I", cols)), 257: (4, 1, struct.pack("<I", rows)), 258: short(data.dtype.itemsize * 8),
           259: short(5), 262: short(1), 277: short(1), 284: short(1), 317: short(2), 322: short(tile), 323: short(tile),
           324: (4, n, struct.pack(f"<{n}I", *offs)), 325: (4, n, struct.pack(f"<{n}I", *(len(t) for t in tiles))),
           339: short({"u": 1, "i": 2, "f": 3}[data.dtype.kind])}
    extra_off = pos + 2 + 12 * len(ent) + 4
    ifd, extra = struct.pack("<H", len(ent)), b""
    for tag in sorted(ent):
        typ, cnt, raw = ent[tag]
        if len(raw) <= 4:
            ifd += struct.pack("<HHI", tag, typ, cnt) + raw.ljust(4, b"\0")
        else:
            ifd += struct.pack("<HHII", tag, typ, cnt, extra_off + len(extra))
            extra += raw
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, pos))
        for t in tiles:
            f.write(t + (b"\0" if len(t) & 1 else b""))
        f.write(ifd + struct.pack("<I", 0) + extra)


def phases(path, dev):
    """One device read of the whole file as a single band, phase by phase (what geotiff._read_blocks_device does per band)."""
    import torch
    from moonsuperresolution_amd import _lib
    from moonsuperresolution_amd import geotiff as G
    lib = _lib.load()
    buf, t, bo, meta = G._open(path)
    rows, cols = meta["shape"]
    sb = meta["dtype"].itemsize
    if 322 in t:
        bw, bh = G._values(t[322], bo)[0], G._values(t[323], bo)[0]
        offs, cnts = G._values(t[324], bo), G._values(t[325], bo)
    else:
        bw, bh = cols, min(G._values(t[278], bo)[0], rows)
        offs, cnts = G._values(t[273], bo), G._values(t[279], bo)
    across, down = -(-cols // bw), -(-rows // bh)
    o, c = np.asarray(offs, np.int64), np.asarray(cnts, np.int64)
    by, bx = np.repeat(np.arange(down), across), np.tile(np.arange(across), down)
    h = np.full(o.size, bh) if 322 in t else np.minimum(bh, rows - by * bh)
    rec = {"n_blocks": int(o.size), "block": [int(bh), int(bw)], "compressed_bytes": int(c.sum())}
    lo, hi = int(o.min()), int((o + c).max())
    t0 = time.perf_counter()
    staged = torch.empty(hi - lo, dtype=torch.uint8, pin_memory=True)
    rec["pinned_alloc_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    staged.numpy()[:] = buf[lo:hi]                                            # the file (page cache) -> pinned memory
    rec["gather_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    src = staged.to(dev, non_blocking=True)
    torch.cuda.synchronize()
    rec["upload_s"] = time.perf_counter() - t0
    out = torch.empty((rows, cols), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dec_ms, place_ms = [], []
    for _ in range(3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        # (the two small tables of offsets and lengths are uploaded between the events too)
        dst, dst_off, dst_len = G.lzw_decode_device(src, o - lo, c, h * bw * sb, check=False)
        e[1].record()
        blk_off = torch.from_numpy(dst_off).to(dev)
        origin = torch.from_numpy(np.concatenate([bx * bw, by * bh]).astype(np.int32)).to(dev)
        e[2].record()
        rc = lib.msr_tiff_blocks_to_f32(None, dst.data_ptr(), blk_off.data_ptr(), origin.data_ptr(), origin.data_ptr() + 4 * o.size,
                                        int(o.size), int(bw), int(bh), ord(meta["dtype"].kind), sb, 2, out.data_ptr(), 0, rows, cols,
                                        stream)
        assert rc == 0
        e[3].record()
        torch.cuda.synchronize()
        dec_ms.append(e[0].elapsed_time(e[1]))
        place_ms.append(e[2].elapsed_time(e[3]))
    assert int(dst_len.min().item()) >= 0
    t0 = time.perf_counter()
    out.cpu()                                                                 # what read_geotiff does: a pageable array
    rec["download_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    pinned = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)     # the alternative, its allocation included
    pinned.copy_(out)
    rec["download_pinned_s"] = time.perf_counter() - t0
    decoded = int((h * bw * sb).sum())
    rec.update(decode_ms=dec_ms, place_ms=place_ms, decoded_bytes=decoded,
               decode_GBps=decoded / (min(dec_ms) * 1e-3) / 1e9, place_GBps=decoded / (min(place_ms) * 1e-3) / 1e9)
    return rec


def run_case(name, repeats):
    import torch
    from moonsuperresolution_amd import geotiff as G
    rows, cols, kind, tile = CASES[name]
    data = product(rows, cols, kind)
    dev = torch.device("cuda", 0)
    rec = {"case": name, "shape": [rows, cols], "dtype": str(data.dtype), "raw_bytes": int(data.nbytes),
           "layout": f"{tile} x {tile} tiles" if tile else "strips"}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.tif")
        if tile:
            write_tiled(path, data, tile, dev)
        else:
            G.write_geotiff(path, data, dtype=data.dtype, encoder="device", device=dev)
        rec["file_bytes"] = os.path.getsize(path)
        G.read_geotiff(path, rows=(0, min(rows, 64)), decoder="device", device=dev)       # runtime start-up
        torch.cuda.synchronize()
        host_s, device_s, same = [], [], True
        for _ in range(repeats):
            t0 = time.perf_counter()
            a, _ = G.read_geotiff(path, decoder="host")
            host_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            b, _ = G.read_geotiff(path, decoder="device", device=dev)
            device_s.append(time.perf_counter() - t0)
            same = same and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            del a, b
        rec.update(host_wall_s=host_s, device_wall_s=device_s, identical=bool(same))
        rec["phases"] = phases(path, dev)
    rec["host_MBps"] = rec["raw_bytes"] / min(host_s) / 1e6
    rec["device_MBps"] = rec["raw_bytes"] / min(device_s) / 1e6
    rec["speedup_end_to_end"] = {"best": min(host_s) / min(device_s), "lowest": min(host_s) / max(device_s),
                                 "highest": max(host_s) / min(device_s)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/geotiff_decode.json")
    ap.add_argument("--limit", type=int, default=600, help="seconds a case may take")
    ap.add_argument("--repeats", type=int, default=3, help="times each decoder reads each file (alternating; at least 3)")
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    repeats = max(3, args.repeats)
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, repeats)), flush=True)
        return 0
    records = []
    for name in CASES:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--repeats", str(repeats)],
                                 capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {args.limit} s; stopping", flush=True)
            return 1
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
        if res.returncode or not lines:
            print(f"{name}: exit status {res.returncode}; stopping\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}", flush=True)
            return 1
        records.append(json.loads(lines[-1][7:]))
        print(json.dumps(records[-1]), flush=True)
    out = {"tool": "tools/gpu_geotiff_decode_bench.py", "cases": records}
    path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0 if all(r["identical"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())

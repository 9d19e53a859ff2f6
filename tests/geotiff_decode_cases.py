"""Shared by tests/test_geotiff_decode_host.py and tests/test_gpu_geotiff_decode.py: the LZW streams both decoders of the
device path (the one-lane host build and the kernel) are checked with against msr_lzw_decode, and a writer of hand-built
tiled TIFFs.  A case is ``(name, stream bytes, cap)``; the lists are built once per process."""
import functools
import struct
import zlib

import numpy as np

from moonsuperresolution_amd import _lib
from moonsuperresolution_amd import geotiff as G

CANARY = 64


def host_decode(stream: bytes, cap: int):
    """msr_lzw_decode(stream, cap): (return value, the bytes [0, return value))."""
    lib = _lib.load()
    src = np.frombuffer(stream.ljust(1, b"\0"), np.uint8)
    out = np.empty(max(cap, 1), np.uint8)
    n = lib.msr_lzw_decode(src.ctypes.data, len(stream), out.ctypes.data, cap)
    return n, out[:max(n, 0)].tobytes()


class Packer:
    """MSB-first codes of explicit widths."""

    def __init__(self):
        self.out, self.buf, self.nbits = bytearray(), 0, 0

    def put(self, code: int, width: int):
        self.buf = (self.buf << width) | code
        self.nbits += width
        while self.nbits >= 8:
            self.out.append((self.buf >> (self.nbits - 8)) & 0xFF)
            self.nbits -= 8
        self.buf &= (1 << self.nbits) - 1
        return self

    def done(self) -> bytes:
        if self.nbits:
            self.out.append((self.buf << (8 - self.nbits)) & 0xFF)
            self.nbits = 0
        return bytes(self.out)


def pack(codes, width: int = 9) -> bytes:
    p = Packer()
    for c in codes:
        p.put(c, width)
    return p.done()


def _width(nxt: int) -> int:
    return 9 if nxt < 511 else 10 if nxt < 1023 else 11 if nxt < 2047 else 12


def encode_never_clearing(raw: bytes, lead: bool = True) -> bytes:
    """A greedy LZW encoder with the TIFF width rule that sends no Clear (but the leading one, with ``lead``): its table
    fills to 4096 entries and 12-bit codes go on without new ones."""
    tab, p = {}, Packer()
    nxt, enc_next, emitted = 258, 258, 0          # nxt: the decoder's next free code when it reads the code being sent
    if lead:
        p.put(256, 9)
    cur = b""
    for i in range(len(raw)):
        ext = cur + raw[i:i + 1]
        if len(ext) == 1 or ext in tab:
            cur = ext
            continue
        p.put(cur[0] if len(cur) == 1 else tab[cur], _width(nxt))
        if emitted and nxt < 4096:                 # the decoder adds an entry for every code but the first
            nxt += 1
        emitted += 1
        if enc_next < 4096:
            tab[ext] = enc_next
            enc_next += 1
        cur = raw[i:i + 1]
    if cur:
        p.put(cur[0] if len(cur) == 1 else tab[cur], _width(nxt))
        if emitted and nxt < 4096:
            nxt += 1
    p.put(257, _width(nxt))
    return p.done()


@functools.lru_cache(None)
def random_buffer() -> np.ndarray:
    return np.random.default_rng(1234).integers(0, 256, 12000, dtype=np.uint8)


@functools.lru_cache(None)
def four_symbols() -> bytes:
    return np.random.default_rng(1234).integers(0, 4, 60000, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def prefix_cases() -> tuple:
    """The streams of lzw_encode for prefixes 0 .. 4400 of the random buffer and the whole buffer: every width change, the
    first Clear and a second dictionary."""
    buf = random_buffer()
    return tuple((f"prefix {n}", G.lzw_encode(buf[:n]), n) for n in list(range(4401)) + [buf.size])


@functools.lru_cache(None)
def long_match_cases() -> tuple:
    zeros = np.zeros(280000, np.uint8)                             # KwKwK chains
    pattern = np.tile(np.array([31, 0], np.uint8), 100000)
    four = np.frombuffer(four_symbols(), np.uint8)
    return tuple((name, G.lzw_encode(d), d.size) for name, d in (("zeros", zeros), ("pattern", pattern), ("four", four)))


@functools.lru_cache(None)
def libtiff_cases() -> tuple:
    """The strips of files PIL/libtiff wrote: another encoder with another Clear policy."""
    import os
    import tempfile
    from PIL import Image
    rng = np.random.default_rng(21)
    smooth = np.cumsum(rng.integers(-3, 4, (75, 300)), axis=1)
    images = {"f32": (smooth * 0.25 - 2000).astype(np.float32), "u16": (smooth + 30000).astype(np.uint16),
              "u8": rng.integers(0, 7, (75, 300)).astype(np.uint8), "u8 noise": rng.integers(0, 256, (200, 300)).astype(np.uint8)}
    cases = []
    with tempfile.TemporaryDirectory() as d:
        for name, a in images.items():
            path = os.path.join(d, "a.tif")
            Image.fromarray(a).save(path, compression="tiff_lzw", tiffinfo={278: 64} if name == "u8 noise" else {278: 8})
            buf, t, bo, meta = G._open(path)
            offs, cnts, rps = G._values(t[273], bo), G._values(t[279], bo), G._values(t[278], bo)[0]
            for i, (o, c) in enumerate(zip(offs, cnts)):
                rows = min(rps, a.shape[0] - i * rps)
                cases.append((f"libtiff {name} strip {i}", bytes(buf[o:o + c]), rows * a.shape[1] * a.dtype.itemsize))
            del buf
    return tuple(cases)


@functools.lru_cache(None)
def hand_cases() -> tuple:
    """Hand-packed and malformed or short streams; the well-formed ones come with the bytes they must decode to."""
    buf, four = random_buffer(), four_symbols()
    cases = [
        ("no leading Clear", pack([65, 66, 258, 260, 257]), 16),            # A B AB ABA (KwKwK)
        ("two Clears in a row", pack([256, 256, 65, 66, 258, 256, 256, 67, 257]), 16),
        ("Clear not at the start only", pack([65, 66, 256, 67, 258, 257]), 16),
        ("bytes after EOI", pack([256, 65, 258, 257]) + b"\xff\x12\x80", 8),
        ("never clears", encode_never_clearing(four), len(four)),
        ("never clears, no leading Clear", encode_never_clearing(four, lead=False), len(four)),
        ("never clears, random", encode_never_clearing(buf.tobytes()), buf.size),
        ("empty", b"", 16),
        ("empty, cap 0", b"", 0),
        ("only EOI", pack([257]), 4),
        ("cap one short", G.lzw_encode(np.frombuffer(four, np.uint8)), len(four) - 1),
        ("cap 0", G.lzw_encode(np.frombuffer(four, np.uint8)), 0),
        ("cap one short, random", G.lzw_encode(buf[:700]), 699),
        ("short output", G.lzw_encode(buf[:700]), 1000),
        ("code above next", pack([256, 65, 66, 300, 257]), 64),
        ("code next + 1", pack([256, 65, 66, 260, 257]), 64),
        ("first code 258 after Clear", pack([256, 258, 257]), 64),
        ("first code 300 after a later Clear", pack([256, 65, 256, 300, 257]), 64),
        ("first code 258 without a Clear", pack([258, 257]), 64),
    ]
    e300 = G.lzw_encode(buf[:280]).ljust(300, b"\0")[:300]
    cases += [(f"truncated at {n}", e300[:n], 280) for n in range(301)]
    rng = np.random.default_rng(99)
    good = np.frombuffer(G.lzw_encode(buf[:3000]), np.uint8)
    for i in range(200):
        s = good.copy()
        bit = int(rng.integers(0, s.size * 8))
        s[bit >> 3] ^= 0x80 >> (bit & 7)
        cases.append((f"bit flip {i} at {bit}", s.tobytes(), 3000))
    for i in range(100):
        s = rng.integers(0, 256, int(rng.integers(1, 2000)), dtype=np.uint8)
        if i & 1 and s.size > 1:                                   # every other one starts with a Clear
            s[0], s[1] = 0x80, s[1] & 0x7F
        cases.append((f"garbage {i}", s.tobytes(), 4096))
    return tuple(cases)


HAND_EXPECT = {"no leading Clear": b"ABABABA", "two Clears in a row": b"ABABC", "Clear not at the start only": b"ABCCC",
               "bytes after EOI": b"AAA", "only EOI": b"", "empty": b"", "empty, cap 0": b""}


def write_tiled(path: str, bands, tw: int, th: int, predictor: int = 1, compression: int = 5, bo: str = "<",
                planar: int = 2, bigtiff: bool = False, predictor_tag=None) -> None:
    """A hand-built TIFF in tw x th tiles (partial edge tiles zero-padded): ``bands`` is a list of equal-shape 2-D arrays
    of one dtype, stored as separate planes (planar = 2) or interleaved (planar = 1, predictor 1 only); compression 1 / 5 /
    8; predictor 2 differences every tile row; ``bo`` the byte order; ``predictor_tag`` overrides the tag's value only."""
    rows, cols = bands[0].shape
    dt = np.dtype(bands[0].dtype).newbyteorder(bo)
    spp = len(bands)
    planes = [np.stack(bands, axis=-1)] if planar == 1 else [b[..., None] for b in bands]
    tiles = []
    for p in planes:
        for ty in range(-(-rows // th)):
            for tx in range(-(-cols // tw)):
                t = np.zeros((th, tw, p.shape[2]), dt)
                blk = p[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
                t[:blk.shape[0], :blk.shape[1]] = blk
                if predictor == 2:
                    assert p.shape[2] == 1
                    u = t.astype(dt.newbyteorder("=")).view(np.dtype(f"u{dt.itemsize}"))
                    d = u.copy()
                    d[:, 1:] = u[:, 1:] - u[:, :-1]
                    t = d.view(dt.newbyteorder("=")).astype(dt)
                raw = t.tobytes()
                tiles.append(raw if compression == 1 else G.lzw_encode(np.frombuffer(raw, np.uint8)) if compression == 5
                             else zlib.compress(raw))
    big = bigtiff
    off_t, head = ("Q", 16) if big else ("I", 8)
    pos, offs = head, []
    for t in tiles:
        offs.append(pos)
        pos += len(t) + (len(t) & 1)
    n = len(tiles)
    short = lambda *v: (3, len(v), struct.pack(bo + "H" * len(v), *v))            # noqa: E731
    entries = {256: (4, 1, struct.pack(bo + "I", cols)), 257: (4, 1, struct.pack(bo + "I", rows)),
               258: short(*[dt.itemsize * 8] * spp), 259: short(compression), 262: short(1), 277: short(spp),
               284: short(planar), 322: short(tw), 323: short(th),
               324: (16 if big else 4, n, struct.pack(bo + off_t * n, *offs)),
               325: (16 if big else 4, n, struct.pack(bo + off_t * n, *(len(t) for t in tiles))),
               339: short(*[{"u": 1, "i": 2, "f": 3}[dt.kind]] * spp)}
    tag317 = predictor if predictor_tag is None else predictor_tag
    if tag317 != 1:
        entries[317] = short(tag317)
    tags = sorted(entries)
    esz, vsz = (20, 8) if big else (12, 4)
    extra_off = pos + (8 if big else 2) + len(tags) * esz + (8 if big else 4)
    ifd, extra = bytearray(struct.pack(bo + ("Q" if big else "H"), len(tags))), bytearray()
    for k in tags:
        typ, cnt, raw = entries[k]
        ifd += struct.pack(bo + "HH", k, typ) + struct.pack(bo + off_t, cnt)
        if len(raw) <= vsz:
            ifd += raw.ljust(vsz, b"\0")
        else:
            if len(extra) & 1:
                extra += b"\0"
            ifd += struct.pack(bo + off_t, extra_off + len(extra))
            extra += raw
    ifd += struct.pack(bo + off_t, 0)
    with open(path, "wb") as f:
        f.write((b"II" if bo == "<" else b"MM") +
                (struct.pack(bo + "HHHQ", 43, 8, 0, pos) if big else struct.pack(bo + "HI", 42, pos)))
        for t in tiles:
            f.write(t + (b"\0" if len(t) & 1 else b""))
        f.write(bytes(ifd) + bytes(extra))

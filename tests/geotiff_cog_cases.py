"""Shared by tests/test_geotiff_cog_host.py and tests/test_gpu_geotiff_cog.py: the blocks the in-place block encoder is checked
on, each with the bytes the encoder has to see built in NumPy (pad with zeros, then difference every block row), the file cases
of layout="cog", and the check of such a file's byte order, which parses the file itself.  Everything is compared for equal
bytes."""
import functools
import struct
from typing import NamedTuple

import numpy as np

from moonsuperresolution_amd import geotiff as G
from tests import geotiff_tiled_cases as tiled

NOVAL = tiled.NOVAL
CANARY = 64
BLOCK_ROW_BYTES = (16, 64, 96, 256, 320)        # a chunk of 256 bytes: 16 block rows, 4, 2 2/3, exactly one, part of two
BLOCK_ROWS = (16, 48)
SAMPLE_BYTES = (0, 1, 2, 4)
# (shape, tile, overviews, bigtiff) of the file tests
FILES = [((70, 101), (16, 16), 3, None), ((17, 33), (16, 16), 2, None), ((1, 1), (16, 16), 0, None), ((70, 101), (16, 16), 3, True)]
FILE_DTYPES = ("float32", "uint8", "uint16")
GHOST = (b"GDAL_STRUCTURAL_METADATA_SIZE=000140 bytes\nLAYOUT=IFDS_BEFORE_DATA\nBLOCK_ORDER=ROW_MAJOR\n"
         b"BLOCK_LEADER=SIZE_AS_UINT4\nBLOCK_TRAILER=LAST_4_BYTES_REPEATED\nKNOWN_INCOMPATIBLE_EDITION=NO\n ")


class Block(NamedTuple):
    """A block of ``bh`` rows of ``bw`` bytes whose valid part, ``vr`` rows of ``vw`` bytes, lies at ``src[off]`` with ``pitch``
    bytes between rows; in the grid ``src`` ends with the last valid byte."""
    name: str
    src: np.ndarray
    off: int
    pitch: int
    vw: int
    vr: int
    bw: int
    bh: int
    sb: int


def padded(b: Block) -> np.ndarray:
    """The bytes the encoder has to see: the valid part in a zero block, then (sb > 0) every row of little-endian samples of
    ``sb`` bytes differenced, the first sample of a row passing through."""
    blk = np.zeros((b.bh, b.bw), np.uint8)
    for y in range(b.vr):
        blk[y, :b.vw] = b.src[b.off + y * b.pitch:b.off + y * b.pitch + b.vw]
    if b.sb:
        u = blk.view(np.dtype(f"<u{b.sb}"))
        d = u.copy()
        d[:, 1:] = u[:, 1:] - u[:, :-1]
        blk = d.view(np.uint8)
    return blk.reshape(-1)


def _source(rng, nbytes: int, sb: int) -> np.ndarray:
    """Terrain-like samples (a random walk in steps of -3 .. 3, so that rows difference to bytes that repeat) as bytes."""
    unit = max(sb, 1)
    n = -(-nbytes // unit) + 1
    walk = np.cumsum(rng.integers(-3, 4, n)) + 1000
    return walk.astype(np.dtype(f"<u{unit}")).view(np.uint8)[:nbytes].copy()


@functools.lru_cache(None)
def grid(sb: int, bw: int, bh: int) -> tuple:
    """The blocks of one geometry (they can share a launch): valid widths of one sample, all but one and all; valid rows of 1,
    bh - 1 and bh; a pitch equal to the valid width, larger, and (1-byte samples) odd; every block begins at an offset of
    its own behind 0 .. 7 samples."""
    unit = max(sb, 1)
    rng = np.random.default_rng(sb * 100000 + bw * 100 + bh)
    out = []
    for vw in (unit, bw - unit, bw):
        for vr in (1, bh - 1, bh):
            pitches = [("tight", vw), ("wide", vw + 5 * unit)] + ([("odd", (vw + 8) | 1)] if unit == 1 else [])
            for pname, pitch in pitches:
                off = int(rng.integers(0, 8)) * unit
                src = _source(rng, off + (vr - 1) * pitch + vw, sb)
                src.setflags(write=False)
                out.append(Block(f"sb{sb}-{bw}x{bh}-w{vw}-r{vr}-{pname}", src, off, pitch, vw, vr, bw, bh, sb))
    return tuple(out)


def geometries():
    return [(sb, bw, bh) for sb in SAMPLE_BYTES for bw in BLOCK_ROW_BYTES for bh in BLOCK_ROWS]


@functools.lru_cache(None)
def special() -> tuple:
    """A 48 x 48 float32 block of random bytes (9216 of them: the table fills and is cleared, and the stream is longer than
    the block), and constant blocks, whose matches run across the edge between the valid part and the padding."""
    rng = np.random.default_rng(48)
    noise = rng.integers(0, 256, 48 * 192, dtype=np.uint8)
    const = np.full(40 * 20, 7, np.uint8)
    out = [Block("random-48x48-f32", noise, 0, 192, 192, 48, 192, 48, 4),
           Block("random-48x48-bytes", noise, 0, 192, 192, 48, 192, 48, 0)]
    for sb in SAMPLE_BYTES:
        unit = max(sb, 1)
        out.append(Block(f"constant-sb{sb}", const, 0, 40, 40 - 40 % unit, 20, 64, 48, sb))
        out.append(Block(f"constant-full-sb{sb}", const, 0, 16, 16, 16, 16, 16, sb))
    for b in out:
        b.src.setflags(write=False)
    return tuple(out)


_STREAMS = {}


def stream(b: Block) -> bytes:
    """The host encoder's stream of the padded block: the reference, computed once (the names are unique)."""
    if b.name not in _STREAMS:
        _STREAMS[b.name] = G.lzw_encode(padded(b))
    return _STREAMS[b.name]


# ---- files ---------------------------------------------------------------------------------------------------------------
META = {"geo": {33550: (12, 3, struct.pack("<3d", 2.0, 2.0, 0.0)), 33922: (12, 6, struct.pack("<6d", 0, 0, 0, 10.0, 20.0, 0)),
                34737: (2, 8, b"WGS 84|\0")}, "byteorder": "<"}


def _ifds(buf: bytes):
    """(BigTIFF or not, [(offset, end of the IFD, {tag: (type, count, offset of an out-of-line value or None, byte size, offset
    of the entry's value field)}), ...] in the order of the chain)."""
    big = struct.unpack_from("<H", buf, 2)[0] == 43
    off = struct.unpack_from("<Q", buf, 8)[0] if big else struct.unpack_from("<I", buf, 4)[0]
    out = []
    while off:
        n = struct.unpack_from("<Q" if big else "<H", buf, off)[0]
        pos, esz, vsz = (off + 8, 20, 8) if big else (off + 2, 12, 4)
        tags = {}
        for i in range(n):
            e = pos + i * esz
            tag, typ = struct.unpack_from("<HH", buf, e)
            cnt = struct.unpack_from("<Q" if big else "<I", buf, e + 4)[0]
            size = G._TYPE_SIZE[typ] * cnt
            voff = struct.unpack_from("<Q" if big else "<I", buf, e + 4 + vsz)[0] if size > vsz else None
            tags[tag] = (typ, cnt, voff, size, e + 4 + vsz)
        end = pos + n * esz + vsz
        out.append((off, end, tags))
        off = struct.unpack_from("<Q" if big else "<I", buf, pos + n * esz)[0]
    return big, out


def check_cog_order(path: str, overviews: int) -> None:
    """Asserts the byte order of a layout="cog" file with ``overviews`` reduced levels, from the file's bytes alone."""
    buf = open(path, "rb").read()
    big, ifds = _ifds(buf)
    head = 16 if big else 8
    assert buf[head:head + 183] == GHOST and len(GHOST) == 183 and len(GHOST[43:]) == 140, "the structural metadata block"
    assert buf[head + 183] == 0
    assert ifds[0][0] == head + 184 == (200 if big else 192), "the first IFD"
    assert len(ifds) == overviews + 1
    fmt = "<Q" if big else "<I"
    payloads = []                                                   # per level: [(offset, count), ...]
    for _, _, tags in ifds:
        typ, cnt, voff, size, inline = tags[324]
        offs = struct.unpack_from(f"<{cnt}{fmt[1]}", buf, inline if voff is None else voff)
        typ, cnt, voff, size, inline = tags[325]
        cnts = struct.unpack_from(f"<{cnt}{fmt[1]}", buf, inline if voff is None else voff)
        payloads.append(list(zip(offs, cnts)))
    first_payload = min(o for level in payloads for o, _ in level)
    last_ifd_end = ifds[-1][1]
    assert [o for o, _, _ in ifds] == sorted(o for o, _, _ in ifds), "the IFDs in level order"
    others = 0
    for k, (off, end, tags) in enumerate(ifds):
        assert off % 2 == 0 and end <= first_payload - 4, ("IFD", k)
        for tag, (typ, cnt, voff, size, _) in tags.items():
            if voff is None:
                continue
            assert voff + size <= first_payload - 4, ("value", k, tag)          # below the first tile's leader
            if tag in (324, 325):
                assert voff >= last_ifd_end, ("array", k, tag)
            else:
                assert end <= voff and (k == len(ifds) - 1 or voff + size <= ifds[k + 1][0]), ("a level's values follow its IFD", k, tag)
                others = max(others, voff + size)
    arrays = [tags[t][2] for _, _, tags in ifds for t in (324, 325) if tags[t][2] is not None]
    assert arrays == sorted(arrays) and all(a >= others for a in arrays), "the arrays in IFD order behind every other value"
    order = [o for level in reversed(payloads) for o, _ in level]           # level n first, level 0 last
    assert order == sorted(order) and len(set(order)) == len(order), "payload offsets increase from level n down to level 0"
    pos = order[0] - 4
    for level in reversed(payloads):
        for o, c in level:
            assert o % 2 == 0 and c >= 4
            assert o == pos + 4, "the tiles lie back to back"
            assert struct.unpack_from("<I", buf, o - 4)[0] == c, "the leader is the count"
            assert buf[o + c:o + c + 4] == buf[o + c - 4:o + c], "the trailer repeats the last four bytes"
            pos = o + c + 4 + (c & 1)
    assert pos == len(buf), "the file ends with the last tile"


def same_levels(cog: str, plain: str, overviews: int, **how) -> None:
    """Every level of the two files read by the project's reader, whole and with rows=, bit for bit the same."""
    assert G.overview_shapes(cog) == G.overview_shapes(plain) and len(G.overview_shapes(cog)) == overviews
    assert G.read_info(cog) == G.read_info(plain)
    for k in range(overviews + 1):
        want, wmeta = G.read_geotiff(plain, overview=k)
        got, meta = G.read_geotiff(cog, overview=k, **how)
        assert meta == wmeta and np.array_equal(tiled.bits(got), tiled.bits(want)), k
        r0, r1 = want.shape[0] // 3, want.shape[0]
        got, meta = G.read_geotiff(cog, overview=k, rows=(r0, r1), **how)
        assert meta["window"] == (r0, r1) and np.array_equal(tiled.bits(got), tiled.bits(want[r0:r1])), k

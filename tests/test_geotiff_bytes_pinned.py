"""CPU: the bytes write_geotiff(encoder="host") writes and the bits read_geotiff reads back are pinned.

tests/golden/geotiff_bytes.json holds, for every case of tests/geotiff_pinned_cases.py, the SHA-256 of the file and of the
raster each pinned read returns (whole, a row window, every reduced level).  It was generated once, before the I/O code was
refactored, by ``python -m tests.test_geotiff_bytes_pinned`` and is read only since: a refactor of geotiff.py that changes
one byte of a file or one bit of a read fails here.  The GPU twin (the device encoder and decoder against the same digests)
is in tests/test_gpu_geotiff_tiled.py.

Also here: plan_bands gives the band cut of the tiled device encoder (the formula it used inline, copied below)."""
import json

import pytest

from moonsuperresolution_amd import geotiff as G
from tests import geotiff_pinned_cases as pinned
from tests import geotiff_tiled_cases as tiled


def test_fixture_lists_the_cases():
    want = pinned.pinned()
    assert sorted(want) == sorted(pinned.IDS) and len(set(pinned.IDS)) == len(pinned.IDS)
    for case in pinned.CASES:
        assert sorted(want[case[0]]) == sorted(["file"] + [k for k, _ in pinned.reads(case)]), case[0]


@pytest.mark.parametrize("case", pinned.CASES, ids=pinned.IDS)
def test_host_file_and_reads_are_the_pinned_ones(tmp_path, case):
    p = str(tmp_path / "a.tif")
    pinned.write(p, case)
    assert pinned.digests(p, case) == pinned.pinned()[case[0]]


@pytest.mark.parametrize("band_bytes", [1, 4096, 256 << 20])
@pytest.mark.parametrize("shape,tile", tiled.LAYOUTS)
def test_plan_bands_is_the_tile_row_cut(shape, tile, band_bytes):
    (rows, cols), (th, tw) = shape, tile
    for sb in (1, 2, 4):
        across, down = -(-cols // tw), -(-rows // th)
        per_band = max(1, int(band_bytes) // (th * across * tw * sb))                       # the inline formula
        inline = [(t0, min(t0 + per_band, down)) for t0 in range(0, down, per_band)]
        assert G.plan_bands(rows, across * tw * sb, th, band_bytes) == inline


if __name__ == "__main__":
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for case in pinned.CASES:
            pinned.write(d + "/a.tif", case)
            out[case[0]] = pinned.digests(d + "/a.tif", case)
    with open(pinned.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {pinned.FIXTURE}")

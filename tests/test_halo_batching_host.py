"""CPU: the call schedule of the halo mode's batching="rank" (moonsuperresolution_amd.halo.batch_schedule / flush_padding).

A rank's valid patches are one sequence cut at multiples of B.  A band issues whole calls of (carry + its own valid patches) and
carries the rest; the rank's last call takes what the last band carried and is the only padded one.  Checked here for random
per-band counts (zeros and counts below B included): the slices the bands issue, put end to end, are the sequence cut at
multiples of B — so a call's batch mates do not depend on where the bands are cut — and the noise ids of the padding rows of
the last call are the same for every cut.
"""
import numpy as np
import pytest

from moonsuperresolution_amd.halo import batch_schedule, flush_padding

BATCHES = (1, 2, 3, 4, 8, 16)


def issued_slices(valid_per_band, B):
    """[(first, last + 1)] in the rank's sequence of every call the bands issue, walked the way halo.py does: the carry stands
    in front of the band's new patches, slot 0 of a band's arrays is patch `issued` of the sequence."""
    out, issued, carry, seen = [], 0, 0, 0
    for nv, (calls, carry_after) in zip(valid_per_band, batch_schedule(valid_per_band, B)):
        assert seen - carry == issued                  # the carried patches are the ones right behind what was issued
        seen += nv
        for c in range(calls):
            out.append((issued + c * B, issued + (c + 1) * B))
        issued += calls * B
        carry = carry_after
        assert 0 <= carry < B and issued + carry == seen
    return out, issued, carry


def random_cuts(rng, total, n_bands):
    """`total` patches spread over `n_bands` bands, zeros allowed."""
    cuts = np.sort(rng.integers(0, total + 1, n_bands - 1))
    return np.diff(np.concatenate([[0], cuts, [total]])).tolist()


@pytest.mark.parametrize("B", BATCHES)
def test_issued_slices_are_the_sequence_cut_at_multiples_of_B(B):
    rng = np.random.default_rng(100 + B)
    for trial in range(200):
        n_bands = int(rng.integers(1, 12))
        if trial % 3 == 0:
            counts = rng.integers(0, max(2, B), n_bands).tolist()        # every band below B: calls only out of the carry
        elif trial % 3 == 1:
            counts = rng.integers(0, 5 * B + 1, n_bands).tolist()
        else:
            counts = [int(c) * int(rng.integers(0, 2)) for c in rng.integers(0, 3 * B, n_bands)]     # many empty bands
        total = sum(counts)
        sched = batch_schedule(counts, B)
        assert len(sched) == len(counts) and all(0 <= carry < B for _, carry in sched)
        slices, issued, carry = issued_slices(counts, B)
        assert slices == [(k * B, (k + 1) * B) for k in range(total // B)]
        assert issued == total // B * B and carry == total - issued
        flush = 1 if carry else 0
        assert sum(c for c, _ in sched) + flush == -(-total // B)         # the final flush pads to ceil(total / B) calls
        assert len(flush_padding(counts, B)) == (B - carry if carry else 0)


def test_small_cases():
    assert batch_schedule([], 4) == [] and flush_padding([], 4) == []
    assert batch_schedule([0, 0], 4) == [(0, 0), (0, 0)] and flush_padding([0, 0], 4) == []
    # 150 x 140 raster at B = 16 with one patch row per band: 5, 10, 15 patches wait, the fourth band issues one call and
    # carries 4, the last call holds 14 patches and 2 padding rows
    counts = [0, 0, 0, 5, 5, 5, 5, 5, 5] + [0] * 10
    sched = batch_schedule(counts, 16)
    assert sched[3:9] == [(0, 5), (0, 10), (0, 15), (1, 4), (0, 9), (0, 14)] and sched[-1] == (0, 14)
    assert flush_padding(counts, 16) == [(30, 0xFFFFFFFE, 0xFFFFFFFF), (31, 0xFFFFFFFE, 0xFFFFFFFF)]
    assert batch_schedule([8, 8], 8) == [(1, 0), (1, 0)] and flush_padding([8, 8], 8) == []
    with pytest.raises(ValueError):
        batch_schedule([1], 0)
    with pytest.raises(ValueError):
        batch_schedule([-1], 4)


@pytest.mark.parametrize("B", BATCHES)
def test_padding_ids_do_not_depend_on_the_cut(B):
    rng = np.random.default_rng(7 * B)
    for total in (0, 1, B - 1, B, B + 1, 30, 123, 135, 16 * B + B // 2):
        want = [(i, 0xFFFFFFFE, 0xFFFFFFFF) for i in range(total, -(-total // B) * B)]
        assert flush_padding([total], B) == want                          # all at once: index in the sequence
        for _ in range(50):
            assert flush_padding(random_cuts(rng, total, int(rng.integers(1, 10))), B) == want

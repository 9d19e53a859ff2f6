"""CPU: the NumPy twin of the counter-based sampler noise (ops.philox4x32_10, ops.sampler_noise; the recipe is stated in
include/moonsr.h).  tests/test_gpu_sampler.py compares the device kernel with this twin bit for bit, so what is shown here
about the twin — the Philox known answers, the distribution, the dependence on (seed, id) alone — holds for the kernel.

The distribution bounds are those a true N(0,1) sample of n = 2^20 values meets with overwhelming probability (5 sigma of
the estimator; Kolmogorov's K = D sqrt(n) exceeds 2.2 with probability ~1e-4).  numpy.random.default_rng(0 | 1 | 2)
.standard_normal(2**20) gives at most 1.2, 2.2, 1.4 and 0.6 for the four statistics."""
import math

import numpy as np
import pytest

from moonsuperresolution_amd import ops

N_ROWS, L = 4096, 256


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32_10: counter / key -> output."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        got = ops.philox4x32_10(np.array(counter, np.uint32), np.array(key, np.uint32))
        assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want
    # vectorised: all three at once, and one key broadcast over many counters
    got = ops.philox4x32_10(np.array([k[0] for k in kat], np.uint32), np.array([k[1] for k in kat], np.uint32))
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in kat]
    many = ops.philox4x32_10(np.zeros((5, 4), np.uint32), np.zeros(2, np.uint32))
    assert many.shape == (5, 4) and (many == np.array(kat[0][2], np.uint32)).all()


@pytest.fixture(scope="module")
def sample():
    ids = np.zeros((N_ROWS, 3), np.uint32)
    ids[:, 0] = np.arange(N_ROWS)
    e = ops.sampler_noise(0, ids=ids, L=L)
    e.setflags(write=False)
    return e


def _corr(a, b):
    a = a.astype(np.float64).ravel() - a.mean(dtype=np.float64)
    b = b.astype(np.float64).ravel() - b.mean(dtype=np.float64)
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_distribution_is_standard_normal(sample):
    assert sample.shape == (N_ROWS, L) and sample.dtype == np.float32
    n = sample.size
    assert n == 1 << 20
    x = sample.astype(np.float64).ravel()
    assert np.isfinite(x).all()
    mean, var = x.mean(), x.var()
    srt = np.sort(x)
    cdf = 0.5 * (1.0 + np.frompyfunc(math.erf, 1, 1)(srt / math.sqrt(2.0)).astype(np.float64))
    k = np.arange(n, dtype=np.float64)
    D = max(np.max((k + 1) / n - cdf), np.max(cdf - k / n))
    r_row = _corr(sample[:, :-1], sample[:, 1:])
    r_col = _corr(sample[:-1], sample[1:])
    stats = dict(mean=abs(mean) * math.sqrt(n), var=abs(var - 1.0) / math.sqrt(2.0 / n), ks=D * math.sqrt(n),
                 lag_row=abs(r_row) * math.sqrt(n), lag_col=abs(r_col) * math.sqrt(n), max_abs=float(np.abs(x).max()))
    print(stats)
    assert stats["mean"] <= 5
    assert stats["var"] <= 5
    assert stats["ks"] <= 2.2
    assert stats["lag_row"] <= 5 and stats["lag_col"] <= 5
    assert stats["max_abs"] >= 4


def test_a_row_depends_on_seed_and_id_only(sample):
    ids = np.array([[9, 0, 0], [3, 0, 0], [4095, 0, 0], [3, 0, 0]], np.uint32)
    e = ops.sampler_noise(0, ids=ids, L=L)
    assert np.array_equal(e.view(np.uint32), sample[[9, 3, 4095, 3]].view(np.uint32))       # any B, any position, repeats
    assert np.array_equal(ops.sampler_noise(0, ids=ids[1:2], L=L).view(np.uint32), sample[3:4].view(np.uint32))
    # a shorter row is a prefix: value l depends on l >> 2, not on L
    assert np.array_equal(ops.sampler_noise(0, ids=ids, L=20).view(np.uint32), e[:, :20].view(np.uint32))
    # the first_row form is the ids form with (first_row + b, 0, 0), modulo 2^32
    assert np.array_equal(ops.sampler_noise(0, B=7, L=L, first_row=100).view(np.uint32), sample[100:107].view(np.uint32))
    wrap = ops.sampler_noise(0, B=3, L=8, first_row=0xFFFFFFFE)
    assert np.array_equal(wrap.view(np.uint32),
                          ops.sampler_noise(0, ids=[[0xFFFFFFFE, 0, 0], [0xFFFFFFFF, 0, 0], [0, 0, 0]], L=8).view(np.uint32))


def test_seed_and_every_id_word_change_the_row():
    base = ops.sampler_noise(5, ids=[[1, 2, 3]], L=L)
    others = [ops.sampler_noise(6, ids=[[1, 2, 3]], L=L), ops.sampler_noise(5 + (1 << 32), ids=[[1, 2, 3]], L=L),
              ops.sampler_noise(5, ids=[[0, 2, 3]], L=L), ops.sampler_noise(5, ids=[[1, 0, 3]], L=L),
              ops.sampler_noise(5, ids=[[1, 2, 0]], L=L), ops.sampler_noise(5, ids=[[2, 1, 3]], L=L)]
    rows = [base] + others
    for i in range(len(rows)):
        for j in range(i + 1, len(rows)):
            assert (rows[i] != rows[j]).mean() > 0.99, (i, j)
            assert abs(_corr(rows[i], rows[j])) < 0.35            # 5.6 sigma of 256 independent pairs


def test_id_words_at_the_ends_of_the_range():
    """0, 0xFFFFFFFF and -1 (which is 0xFFFFFFFF as uint32) are ids like any other; seeds use all 64 bits."""
    as_u32 = ops.sampler_noise(2 ** 63 + 5, ids=np.array([[0, 0, 0], [0xFFFFFFFF] * 3, [0, 0xFFFFFFFF, 0]], np.uint32), L=L)
    as_i32 = ops.sampler_noise(2 ** 63 + 5, ids=np.array([[0, 0, 0], [-1] * 3, [0, -1, 0]], np.int32), L=L)
    as_list = ops.sampler_noise(2 ** 63 + 5, ids=[[0, 0, 0], [0xFFFFFFFF] * 3, [0, -1, 0]], L=L)
    assert np.array_equal(as_u32.view(np.uint32), as_i32.view(np.uint32))
    assert np.array_equal(as_u32.view(np.uint32), as_list.view(np.uint32))
    assert np.isfinite(as_u32).all() and (as_u32[0] != as_u32[1]).mean() > 0.99 and (as_u32[0] != as_u32[2]).mean() > 0.99
    assert (ops.sampler_noise(5, ids=[[0, 0, 0]], L=L) != as_u32[:1]).mean() > 0.99          # the high seed word counts
    with pytest.raises(ValueError):
        ops.sampler_noise(0, B=2, L=6)
    with pytest.raises(ValueError):
        ops.sampler_noise(0, ids=[[0, 0]], L=8)


def test_the_transform_at_the_ends_of_the_integer_range():
    """u = (n + 0.5) / 2^32 is never 0 or 1: the radius is finite and positive at n = 0 and n = 2^32 - 1, and the polynomial
    sin / cos stay on the unit circle to fp32 accuracy in every octant."""
    n = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    r = ops._sampler_radius(n)
    assert r.dtype == np.float32 and np.isfinite(r).all() and (r > 0).all()
    assert abs(float(r[0]) - math.sqrt(66 * math.log(2))) < 1e-5                             # u = 2^-33
    n = np.random.default_rng(3).integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)
    u = (n.astype(np.float64) + 0.5) / 2.0 ** 32
    c, s = ops._sampler_cos_sin(n)
    assert c.dtype == s.dtype == np.float32
    # the angle keeps 23 bits below the octant: 2 pi / 2^27 = 4.7e-8 of argument error, plus fp32 rounding
    assert np.abs(c - np.cos(2 * np.pi * u)).max() < 3e-7 and np.abs(s - np.sin(2 * np.pi * u)).max() < 3e-7
    # the mantissa keeps 24 bits of u: |d ln u| <= 2^-24 + fp32 rounding of a value up to 23
    ln = -0.5 * ops._sampler_radius(n).astype(np.float64) ** 2
    assert np.abs(ln - np.log(u)).max() < 4e-6

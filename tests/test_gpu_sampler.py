"""GPU (-m gpu): the counter-based sampler noise, from the kernel to the tiler.

msr_sampler_noise is compared bit for bit with its NumPy twin (ops.sampler_noise, whose distribution and structure
tests/test_sampler_host.py checks), Generator(sampler="counter") with a plain generator that is handed the twin's array, and
the products of the stochastic model ("gaugan") are shown to be the same bits whatever the pipeline depth, the run, the number
of ranks and their row windows in tile mode.  Every comparison is exact: the same kernels see the same inputs.

Geometry: S = 64, B <= 4, T = 128, as the other tiler tests."""
import numpy as np
import pytest
import torch

from moonsuperresolution_amd import distributed as D
from moonsuperresolution_amd import ops
from tests.helpers import synthetic_raster

pytestmark = pytest.mark.gpu
S, B, T, L = 64, 4, 128, 256
SEED = 11


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def weights():
    from moonsuperresolution_amd import make_weights
    return make_weights("gaugan", S, seed=1234)


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = ops.OpContext()
    yield c
    c.close()


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 4), (3, 20), (4, 256), (16, 256)])
@pytest.mark.parametrize("seed", [0, 2 ** 63 + 5])
def test_device_noise_equals_the_twin_bit_for_bit(ctx, shape, seed):
    """(3, 20) is 15 Philox blocks: the one workgroup is partly idle.  The buffer is longer than B * L: nothing is written
    behind the last row."""
    nb, nl = shape
    rng = np.random.default_rng(nb * 1000 + nl)
    ids = rng.integers(0, 1 << 32, (nb, 3), dtype=np.uint64).astype(np.uint32)
    ids[0] = (0, 0xFFFFFFFF, 0)
    ids[-1, 2] = 0xFFFFFFFF
    if nb > 1:
        ids[1] = 0
    guard = 64
    for dev_ids, first_row, want in [
            (torch.from_numpy(ids.view(np.int32)).to(ctx.device), 0, ops.sampler_noise(seed, ids=ids, L=nl)),
            (None, 0, ops.sampler_noise(seed, B=nb, L=nl)),
            (None, 0xFFFFFFFF, ops.sampler_noise(seed, B=nb, L=nl, first_row=0xFFFFFFFF))]:
        buf = torch.full((nb * nl + guard,), 123.0, dtype=torch.float32, device=ctx.device)
        ops.sampler_noise_device(ctx, seed, nb, nl, ids=dev_ids, first_row=first_row, out=buf)
        got = buf.cpu().numpy()
        assert np.array_equal(bits(got[:nb * nl]).reshape(nb, nl), bits(want)), (shape, seed, dev_ids is None, first_row)
        assert (got[nb * nl:] == 123.0).all()
    assert np.isfinite(want).all()


def test_device_noise_rejects_bad_arguments(ctx):
    buf = torch.empty(64, dtype=torch.float32, device=ctx.device)
    for nb, nl in [(0, 4), (1, 0), (1, 6), (-1, 8)]:
        with pytest.raises(ValueError, match="msr_sampler_noise"):
            ops.sampler_noise_device(ctx, 0, nb, nl, out=buf)
    with pytest.raises(ValueError, match="aligned"):
        ops.sampler_noise_device(ctx, 0, 1, 4, out=buf[1:])


# ---- 2. the generator ---------------------------------------------------------------------------------------------------
def test_counter_mode_equals_explicit_noise(hip_lib, weights):
    from moonsuperresolution_amd import Generator, synthetic_patches
    x = torch.from_numpy(synthetic_patches(B, S, seed=0)).cuda()
    ids = np.array([[0, 0, 0], [5, 64, 128], [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF], [3, 0, 7]], np.uint32)
    other = ids.copy()
    other[2, 1] = 1
    dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()                                # noqa: E731
    gen = Generator(S, B, variant="gaugan", weights=weights, sampler="counter", seed=SEED)
    plain = Generator(S, B, variant="gaugan", weights=weights, eps=None)
    y = gen.forward_device(x, noise_ids=dev(ids)).cpu().numpy()
    want = plain.forward_device(x, eps=torch.from_numpy(ops.sampler_noise(SEED, ids=ids, L=L)).cuda()).cpu().numpy()
    assert np.isfinite(y).all() and np.array_equal(bits(y), bits(want))
    y_other = gen.forward_device(x, noise_ids=dev(other)).cpu().numpy()
    assert not np.array_equal(bits(y_other), bits(y))
    assert np.array_equal(bits(gen.forward_device(x, noise_ids=dev(ids)).cpu().numpy()), bits(y))      # same ids again
    # uint32 ids are the same ids
    if hasattr(torch, "uint32"):
        assert np.array_equal(bits(gen.forward_device(x, noise_ids=dev(ids).view(torch.uint32)).cpu().numpy()), bits(y))
    # without ids: rows calls * B + b of the instance's own counter, on the device path and the host path alike
    for call, run in enumerate([lambda: gen.forward_device(x).cpu().numpy(), lambda: gen(x.cpu().numpy())]):
        e = torch.from_numpy(ops.sampler_noise(SEED, B=B, L=L, first_row=call * B)).cuda()
        assert np.array_equal(bits(run()), bits(plain.forward_device(x, eps=e).cpu().numpy())), call
    gen.reset_sampler()
    first = gen.forward_device(x).cpu().numpy()
    gen.reset_sampler(calls=1)
    second = gen(x.cpu().numpy())
    twin = gen.clone()
    assert (twin.sampler, twin.seed) == ("counter", SEED)
    assert np.array_equal(bits(twin.forward_device(x).cpu().numpy()), bits(first))              # a clone starts at call 0
    assert np.array_equal(bits(twin(x.cpu().numpy())), bits(second)) and not np.array_equal(bits(first), bits(second))
    # range_report runs its call on rows 0 .. B - 1 and leaves the counter alone
    gen.reset_sampler(calls=1)
    assert gen.range_report(x.cpu().numpy()).regime in ("parity", "degraded", "clamped")
    assert np.array_equal(bits(gen.forward_device(x).cpu().numpy()), bits(second))
    # precision="auto" calibrates on the counter noise of rows 0 .. B - 1 and hands over a generator that has drawn nothing
    auto = Generator(S, B, variant="gaugan", weights=weights, precision="auto", sampler="counter", seed=SEED)
    assert (auto.sampler, auto.seed, auto._sampler_calls) == ("counter", SEED, 0) and auto.range is not None
    if auto.precision == gen.precision:
        assert np.array_equal(bits(auto.forward_device(x, noise_ids=dev(ids)).cpu().numpy()), bits(y))
        assert np.array_equal(bits(auto.forward_device(x).cpu().numpy()), bits(first))
    auto.close()
    with pytest.raises(ValueError, match="noise_ids"):
        gen.forward_device(x, noise_ids=dev(ids)[:2])
    with pytest.raises(ValueError, match="noise_ids"):
        gen.forward_device(x, noise_ids=dev(ids).to(torch.int64))
    with pytest.raises(ValueError, match="noise_ids"):
        plain.forward_device(x, noise_ids=dev(ids))
    for g in (gen, plain, twin):
        g.close()


def test_counter_sampler_constructor_errors(hip_lib, weights):
    from moonsuperresolution_amd import Generator
    for variant in ("gaugan_no_kl", "cnn", "pix2pix"):
        with pytest.raises(ValueError, match="counter"):
            Generator(256 if variant == "pix2pix" else S, B, variant=variant, weights=1234, sampler="counter")
    with pytest.raises(ValueError, match="eps"):
        Generator(S, B, variant="gaugan", weights=weights, sampler="counter", eps=7)
    with pytest.raises(ValueError, match="eps"):
        Generator(S, B, variant="gaugan", weights=weights, sampler="counter", eps=np.zeros((B, L), np.float32))
    with pytest.raises(ValueError, match="sampler"):
        Generator(S, B, variant="gaugan", weights=weights, sampler="philox")
    with pytest.raises(ValueError, match="seed"):
        Generator(S, B, variant="gaugan", weights=weights, sampler="counter", seed=-1)


# ---- 3. tile mode -------------------------------------------------------------------------------------------------------
STRIDE = 32
SHAPE = (250, 230)                                    # 2 x 2 tiles of 128; 5 x 5 patch origins per tile
HOLE = (150, 170, 40, 60)                             # leaves 14, 12, 6 and 9 valid patches in the four tiles


def _cfg(stride=STRIDE):
    from moonsuperresolution_amd import DSRConfig
    return DSRConfig(image_size=S, stride=stride, batch_size=B, tile_size=T)


def test_tile_mode_products_do_not_depend_on_pipeline_run_or_ranks(hip_lib, weights):
    from moonsuperresolution_amd import DEMSuperResolution, Generator
    img, dem = synthetic_raster(SHAPE[0], SHAPE[1], seed=9, hole=HOLE)
    gen = Generator(S, B, variant="gaugan", weights=weights, sampler="counter", seed=SEED)

    def run(pipeline):
        d = DEMSuperResolution(_cfg(), model=gen, pipeline=pipeline)
        out = d.processMap(img, dem)
        d.close()
        return out

    want = run(1)
    assert want[2].any() and not want[2].all() and np.isfinite(want[0][want[2] > 0]).all()
    # the geometry the test is about: patches drop out, and some tile's last call is padded
    d = DEMSuperResolution(_cfg(), model=gen, pipeline=1)
    d.setImages(img, dem)
    d.padInputs()
    counts = []
    for t in d.generateTileList():
        d.processTile(*t)
        counts.append(d.last_counts[0])
    d.close()
    assert len(counts) == 4 and all(0 < n < 25 for n in counts) and any(n % B for n in counts), counts
    for name, got in (("pipeline=2", run(2)), ("second run", run(1))):
        for a, b in zip(got, want):
            assert np.array_equal(a, b, equal_nan=True), name
    # two simulated ranks, each holding only its row window
    world = 2
    parts = []
    for rank in range(world):
        d = DEMSuperResolution(_cfg(), model=gen)
        d.setImages(img, dem)
        rows = D.crop_for_rank(d, rank, world)
        assert rows != (0, SHAPE[0])
        d.padInputs()
        parts.append(D.process_map_sharded(SHAPE, T, d.generateTileList(), d.processTile, rank, world, gather=False,
                                           device=d.device))
        d.close()
    for k in range(3):
        both = np.concatenate([parts[0][k][:T], parts[1][k][T:]], axis=0)       # rank 0 owns tile row 0, rank 1 tile row 128
        assert np.array_equal(both, want[k], equal_nan=True), k
    # another seed is another draw
    gen2 = Generator(S, B, variant="gaugan", weights=weights, sampler="counter", seed=SEED + 1)
    d = DEMSuperResolution(_cfg(), model=gen2, pipeline=1)
    other = d.processMap(img, dem)
    d.close()
    assert np.array_equal(other[2], want[2]) and not np.array_equal(other[0], want[0], equal_nan=True)
    gen.close()
    gen2.close()


def test_gated_tile_loop_gives_the_ungated_products(hip_lib, weights, monkeypatch):
    """MSR_TILER_GATED=1 (read at construction): every call of a two-handle pipeline waits, in its matrix-bound part, for the
    event the previous call recorded on the other stream.  An ordering of work only: all three products are the bits of the
    ungated two-handle loop and of the one-handle loop."""
    from moonsuperresolution_amd import DEMSuperResolution, Generator
    img, dem = synthetic_raster(SHAPE[0], SHAPE[1], seed=9, hole=HOLE)
    gen = Generator(S, B, variant="gaugan", weights=weights, sampler="counter", seed=SEED)

    def run(pipeline, gated):
        if gated:
            monkeypatch.setenv("MSR_TILER_GATED", "1")
        else:
            monkeypatch.delenv("MSR_TILER_GATED", raising=False)
        d = DEMSuperResolution(_cfg(), model=gen, pipeline=pipeline)
        assert d.gated == gated and len(d._gens) == pipeline
        out = d.processMap(img, dem)
        d.close()
        return out

    got = run(2, True)
    assert got[2].any() and not got[2].all() and np.isfinite(got[0][got[2] > 0]).all()
    for name, want in (("ungated pipeline=2", run(2, False)), ("pipeline=1", run(1, False))):
        for k in range(3):
            assert np.array_equal(got[k], want[k], equal_nan=True), (name, k)
    gen.close()


def test_pipeline_clones_follow_a_load_on_the_base_generator(hip_lib, weights):
    """load() on the generator a two-handle driver was built on: the next map is the map of a fresh driver on the new weights,
    so the clone (which takes every second call of a tile) holds them too."""
    from moonsuperresolution_amd import DEMSuperResolution, Generator, make_weights
    img, dem = synthetic_raster(SHAPE[0], SHAPE[1], seed=9, hole=HOLE)
    other = make_weights("gaugan", S, seed=4321)
    gen = Generator(S, B, variant="gaugan", weights=weights, sampler="counter", seed=SEED)
    d = DEMSuperResolution(_cfg(), model=gen, pipeline=2)
    first = d.processMap(img, dem)
    gen.load(other)
    second = d.processMap(img, dem)
    assert all(g.weights_version == gen.weights_version for g in d._gens)
    d.close()
    fresh_gen = Generator(S, B, variant="gaugan", weights=other, sampler="counter", seed=SEED)
    fresh = DEMSuperResolution(_cfg(), model=fresh_gen, pipeline=1)      # one handle: nothing of a clone in what is expected
    want = fresh.processMap(img, dem)
    fresh.close()
    for k in range(3):
        assert np.array_equal(second[k], want[k], equal_nan=True), k
    assert np.array_equal(first[2], second[2]) and not np.array_equal(first[0], second[0], equal_nan=True)
    gen.close()
    fresh_gen.close()


# ---- 4. graph replay ----------------------------------------------------------------------------------------------------
def test_graph_replay_follows_the_noise_buffer(hip_lib, weights):
    """The noise pointer never changes, so the second call captures and the third replays; the fill runs on the stream ahead
    of the graph, so each replay reads that call's noise."""
    from moonsuperresolution_amd import Generator, synthetic_patches
    gen = Generator(S, 1, variant="gaugan", weights=weights, sampler="counter", seed=SEED)
    x = torch.from_numpy(synthetic_patches(1, S, seed=3)).cuda()
    a = torch.tensor([[1, 2, 3]], dtype=torch.int32, device="cuda")
    b = torch.tensor([[1, 2, 4]], dtype=torch.int32, device="cuda")
    out = torch.empty((1, S, S, 1), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):                # a capturable stream
        eager = [gen.forward_device(x, out=out, noise_ids=i).cpu().numpy().copy() for i in (a, b)]
        gen.use_graph(True)
        got = [gen.forward_device(x, out=out, noise_ids=i).cpu().numpy().copy() for i in (a, b, a)]
        gen.use_graph(False)
    assert np.array_equal(bits(got[0]), bits(eager[0])) and np.array_equal(bits(got[1]), bits(eager[1]))
    assert np.array_equal(bits(got[2]), bits(eager[0])) and not np.array_equal(bits(got[1]), bits(got[0]))
    gen.close()


# ---- 5. halo mode -------------------------------------------------------------------------------------------------------
def test_halo_mode_noise_follows_the_patch(hip_lib, weights):
    from moonsuperresolution_amd import Generator, HaloShardedSuperResolution
    img, dem = synthetic_raster(150, 140, seed=5, hole=(0, 20, 0, 30))       # 30 patches inside the raster, 4 on the hole
    gen = Generator(S, B, variant="gaugan", weights=weights, sampler="counter", seed=SEED)
    d = HaloShardedSuperResolution(_cfg(stride=16), model=gen, pipeline=1)
    runs = [d.cropHalo([d.processMapHalo(img, dem)]) for _ in range(2)]
    assert runs[0][2].any() and not runs[0][2].all()
    for p, q in zip(*runs):
        assert np.array_equal(p, q, equal_nan=True)
    # the ids a band hands to the generator: the canvas origins of its compacted patches, then the padding slots
    seen = []
    real = gen.forward_device
    gen.forward_device = lambda *a, noise_ids=None, **kw: (seen.append(noise_ids.cpu().numpy()), real(*a, noise_ids=noise_ids, **kw))[1]
    ys, xs = d.patchGrid()
    _, keys, _, nv = d._generate_rows(ys, xs)
    del gen.forward_device
    ids = d.last_noise_ids.cpu().numpy()
    keys = keys.cpu().numpy()
    cap = ids.shape[0]
    assert 0 < nv < len(ys) * len(xs) and nv % B and cap == len(ys) * len(xs) + (-len(ys) * len(xs)) % B
    assert np.array_equal(ids[:nv, :2], keys[:nv]) and (ids[:, 2] == -1).all()
    grid = [(x, y) for y in ys for x in xs]                        # generation order: y outer, x inner
    order = [grid.index((int(x), int(y))) for x, y in ids[:nv, :2]]
    assert order == sorted(order) and len(set(order)) == nv        # compacted, in order, each a patch of the grid
    pad = np.arange(nv, cap)
    assert np.array_equal(ids[nv:, 0], pad) and (ids[nv:, 1] == -2).all()
    ncall = -(-nv // B)
    assert len(seen) == ncall and np.array_equal(np.concatenate(seen), ids[:ncall * B])
    d.close()
    gen.close()

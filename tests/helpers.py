"""Shared seeded input builders for tests and tests/golden/make_golden.py."""
import numpy as np


def record_dir():
    """The repository's directory for run records (where the GPU parity tests append their jsonl lines): the `*_out/` entry of
    .gitignore."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        for line in open(os.path.join(root, ".gitignore")):
            if line.strip().endswith("_out/"):
                return os.path.join(root, line.strip().rstrip("/"))
    except OSError:
        pass
    return os.path.join(root, "run_out")


def rel_linf(a, b):
    """Relative L-infinity error used for every floating-point parity statement: max|a-b| / max|b|."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def stitch_inputs(S=64, s=16, T=128, seed=5, drop=0.15):
    """Random generator outputs for one tile in generation order: keys [n,2] (x,y), pred [n,S,S] (raw model
    output, i.e. before the +0.5 of process_full_tiles.py:340), dem (min,max) [n,2]."""
    rng = np.random.default_rng(seed)
    n_side = len(range(0, T + S - s, s))
    keys, pred, mm = [], [], []
    for iy in range(n_side):
        for ix in range(n_side):
            if rng.uniform() < drop:
                continue   # invalid patches are simply absent (process_full_tiles.py:456-457)
            keys.append((ix * s, iy * s))
            pred.append(rng.uniform(-0.6, 0.6, (S, S)).astype(np.float32))
            lo = np.float32(rng.uniform(-3000, -2000))
            mm.append((lo, np.float32(lo + rng.uniform(5, 400))))
    return np.array(keys, np.int32), np.stack(pred), np.array(mm, np.float32)


def synthetic_raster(h, w, seed=0, hole=None, no_value=-32768.0):
    """Smooth (ortho, DEM) rasters: ortho in [0,1], DEM in [-3000,-1000] m, optional nodata rectangle."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    dem = (-2000 + 600 * np.sin(xx / 37.0) * np.cos(yy / 53.0) + 300 * np.sin((xx + 2 * yy) / 91.0)
           + 5 * rng.standard_normal((h, w)))
    img = 0.5 + 0.3 * np.cos(xx / 23.0) * np.sin(yy / 31.0) + 0.05 * rng.standard_normal((h, w))
    dem = dem.astype(np.float32)
    img = np.clip(img, 0, 1).astype(np.float32)
    if hole is not None:
        y0, y1, x0, x1 = hole
        dem[y0:y1, x0:x1] = no_value
    return img, dem


def smallcin_ref(src, w, bias, hout, index_map, act=0, slope=0.0, device=None):
    """float64 CPU restatement of conv_smallcin (``device``: the same arithmetic as tap matmuls on that device, for the
    network-sized tensors of tests/test_gpu_network_sites.py): src [B,S,S,2] -> [B,hout,hout,Cout].  index_map 0: Conv2D(3, strides=2,
    'same') on S = 2 hout (TF pads 0 before, 1 after); 1: tf.image.resize(nearest, half-pixel centres) to hout x hout, then
    Conv2D(3, 'same'); act 1 relu, 2 leaky_relu(slope)."""
    import torch
    import torch.nn.functional as F
    if device is not None:
        return _smallcin_ref_taps(src, w, bias, hout, index_map, act, slope, device)
    x = src.double().cpu()
    S = x.shape[1]
    if index_map == 1:
        f = S // hout
        x = x[:, f // 2::f, f // 2::f][:, :hout, :hout]
    xn = x.permute(0, 3, 1, 2)
    xn = F.pad(xn, (0, 1, 0, 1)) if index_map == 0 else F.pad(xn, (1, 1, 1, 1))
    b = bias.double().cpu() if bias is not None else None
    y = F.conv2d(xn, w.double().cpu().permute(3, 2, 0, 1), b, stride=2 if index_map == 0 else 1).permute(0, 2, 3, 1)
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.where(y >= 0, y, slope * y)
    return y


def ref_conv(x, w, b, stride):
    """TF SAME conv on NHWC in float64 on the CPU."""
    import torch
    import torch.nn.functional as F
    x, w, b = x.double().cpu(), w.double().cpu(), b.double().cpu()
    xn = x.permute(0, 3, 1, 2)
    xn = F.pad(xn, (1, 1, 1, 1)) if stride == 1 else F.pad(xn, (0, 1, 0, 1))
    return F.conv2d(xn, w.permute(3, 2, 0, 1), b, stride=stride).permute(0, 2, 3, 1)


def unsplit(t):
    """split-bf16 chunk image -> (hi + lo) float32 values, same shape (innermost dim % 32 == 0)."""
    import torch
    u = t.contiguous().view(torch.int16).reshape(-1, 2, 32).to(torch.int32) & 0xFFFF
    hi = (u[:, 0] << 16).view(torch.float32)
    lo = (u[:, 1] << 16).view(torch.float32)
    return hi.reshape(t.shape), lo.reshape(t.shape)


def _ref_f16c(xparts, wparts, bias, cin, cout):
    """What the f16c kernel computes, in float64: x_hi*w_hi + x_h8*w_lo8 + x_lo8*w_h8 (+ bias)."""
    import torch
    (xh, x8, xl), (wh, w8, wl) = xparts, wparts
    hwio = lambda t: t.permute(0, 2, 1).reshape(3, 3, cin, cout)   # noqa: E731
    zero = torch.zeros(cout, dtype=torch.float64)
    return (ref_conv(xh, hwio(wh), bias, 1) + ref_conv(x8, hwio(wl), zero, 1) + ref_conv(xl, hwio(w8), zero, 1))


def conv_taps(xpad, w_tnk, r, stride=1, dtype=None):
    """3x3 conv as nine matmuls, on whatever device the operands live: xpad [B, r * stride + 2, ., C] zero-bordered NHWC (what
    the conv kernels read: tap (kh, kw) of output (y, x) is xpad[b, y * stride + kh, x * stride + kw] at stride 1 and
    xpad[b, 1 + y * stride + kh, 1 + x * stride + kw] at stride 2, TF SAME), w_tnk [9][N][C] -> [B, r, r, N].  float64 unless
    ``dtype`` says otherwise (float32: the plain fp32 accumulation the K-length allowance is measured with)."""
    import torch
    dtype = dtype or torch.float64
    B, C = xpad.shape[0], xpad.shape[3]
    N = w_tnk.shape[1]
    off = 0 if stride == 1 else 1
    w = w_tnk.to(dtype)
    out = torch.empty((B, r, r, N), dtype=dtype, device=xpad.device)
    for b in range(B):                       # per sample: bounds the temporaries at the S = 512 shapes
        xb = xpad[b].to(dtype)
        acc = torch.zeros((r * r, N), dtype=dtype, device=xpad.device)
        for kh in range(3):
            for kw in range(3):
                sl = xb[off + kh: off + kh + stride * r: stride, off + kw: off + kw + stride * r: stride]
                acc += sl.reshape(r * r, C) @ w[kh * 3 + kw].T
        out[b] = acc.reshape(r, r, N)
    return out


def pad_hw(x):
    """[B, r, r, C] -> zero-bordered [B, r + 2, r + 2, C], same dtype and device."""
    import torch.nn.functional as F
    return F.pad(x, (0, 0, 1, 1, 1, 1))


def _smallcin_ref_taps(src, w, bias, hout, index_map, act, slope, device):
    import torch
    x = src.double().to(device)
    S = x.shape[1]
    if index_map == 1:
        f = S // hout
        x = x[:, f // 2::f, f // 2::f][:, :hout, :hout]
    w_tnk = w.double().to(device).reshape(9, 2, -1).permute(0, 2, 1).contiguous()
    y = conv_taps(pad_hw(x), w_tnk, hout, stride=2 if index_map == 0 else 1)
    if bias is not None:
        y = y + bias.double().to(device)
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.where(y >= 0, y, slope * y)
    return y


def dense_kch(K, N):
    """small_kernels.hip dense_kch: K chunk per workgroup (power of two, 16..256) for >= 1024 workgroups."""
    gx = (N // 4 + 127) // 128
    kch = 256
    while kch > 16 and gx * ((K + kch - 1) // kch) < 1024:
        kch >>= 1
    return kch


def rel_linf_per_channel(a, b):
    """One entry per last-dimension channel: max over pixels |a - b| / max over pixels |b| (float64; numpy arrays or torch
    tensors on any device).  A channel whose reference is identically zero reports inf if ``a`` is not zero there (0 if it
    is): no epsilon in the denominator, which would hide such a channel."""
    import torch
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double().to(a.device)
    C = b.shape[-1]
    err = (a - b).abs().reshape(-1, C).amax(0)
    den = b.abs().reshape(-1, C).amax(0)
    out = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                        torch.zeros_like(err)))
    return out.cpu().numpy()


def conv_channel_inputs(B, r, cin, cout, seed, res=None, x_decades=None):
    """Operands for the per-channel conv tests (host tensors): x, w and skip as tests/test_gpu_conv_kernel.py::test_conv_f16c
    builds them (weights spanning three decades over the output channels; ``x_decades`` = (lo, hi): x scaled over its input
    channels as test_conv_f16c6 does), and a bias scaled like its channel (randn * logspace), so that every channel's reference
    magnitude is set by its own weights.  res: the residual's aux_shift (None: no skip)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    ls = torch.logspace(-2, 1, cout)
    x = torch.randn((B, r, r, cin), generator=g)
    if x_decades is not None:
        x = x * torch.logspace(x_decades[0], x_decades[1], cin)
    w = torch.randn((3, 3, cin, cout), generator=g) / np.sqrt(9 * cin) * ls
    b = torch.randn(cout, generator=g) * ls
    skip = torch.randn((B, r >> res, r >> res, cout), generator=g) if res is not None else None
    return x, w, b, skip


def f16c_terms(xparts_pad, wparts, r, dtype=None, terms=(True, True, True)):
    """The f16c family's three terms on de-quantised operands, on whatever device they live, summed in ``dtype`` (float64, or
    float32 = plain fp32 accumulation): x_hi * w_hi + x_h * w_lo + x_lo * w_h.  xparts_pad: zero-bordered [B, r + 2, r + 2, C]
    (hi, h, lo) pieces; wparts [9][N][C] (hi, h, lo); ``terms`` switches a term off."""
    (xh, x8, xl), (wh, w8, wl) = xparts_pad, wparts
    y = conv_taps(xh, wh, r, dtype=dtype) if terms[0] else 0
    if terms[1]:
        y = y + conv_taps(x8, wl, r, dtype=dtype)
    if terms[2]:
        y = y + conv_taps(xl, w8, r, dtype=dtype)
    return y


def persistent_item_rounds(items, n_cu):
    """Host restatement of persistent_grid + xcd_tile_range (csrc/conv_igemm.hip, conv_common.h): for each logical work item
    0..items-1 of a persistent conv launch on a device with ``n_cu`` compute units, (slot, round): the position of its
    workgroup inside the XCD's range and how many items that workgroup took before it (round >= 1: the workgroup has moved to
    another tile).  Workgroup (xcd, slot) takes items base + slot + k * slots of the XCD's range [base, base + cnt)."""
    n_cu = max(n_cu & ~7, 8)
    grid = (items + 7) & ~7 if items < n_cu else n_cu
    slots, tq, tr = grid >> 3, items >> 3, items & 7
    out = np.zeros((items, 2), np.int64)
    for xcd in range(8):
        cnt = tq + (1 if xcd < tr else 0)
        base = xcd * (tq + 1) if xcd < tr else tr * (tq + 1) + (xcd - tr) * tq
        for i in range(cnt):
            out[base + i] = (i % slots, i // slots)
    return out


def conv_walk_item(t, tiles_m, tiles_n, walk=True):
    """Host restatement of conv_walk_pick + MSR_WALK (csrc/conv_igemm.hip, kernels.h): logical tile t -> (channel block,
    pixel tile).  ``walk=False``: channel block fastest (launches that do not call conv_walk)."""
    pb, nb = (8, 4) if walk and tiles_n > 4 and tiles_n % 4 == 0 and tiles_m % 8 == 0 else (1, tiles_n)
    grp, sub = pb * tiles_n, pb * nb
    blk, rem = divmod(t, grp)
    ng, j = divmod(rem, sub)
    jp = j // nb
    return ng * nb + (j - jp * nb), blk * pb + jp


def later_round_mask(B, r, N, n_cu, walk=True, pick=None, new_block=False):
    """bool [B, r // 16, r // 16, N // 128]: the (16 x 16 pixel tile, 128-channel block) items of a whole-tile persistent conv
    launch that ``pick(slot, round)`` selects (default: round >= 1, the items a workgroup computes after its first one).
    ``new_block``: of those, only the items whose channel block differs from that of the workgroup's previous item (item
    t - slots of the same XCD range): the ones for which the workgroup must really re-read its scales and bias."""
    ty = r // 16
    tiles_m, tiles_n = B * ty * ty, N // 128
    items = tiles_m * tiles_n
    slots = min((items + 7) & ~7, max(n_cu & ~7, 8)) >> 3
    pick = pick or (lambda slot, rnd: rnd >= 1)
    mask = np.zeros((B, ty, ty, tiles_n), bool)
    for t, (slot, rnd) in enumerate(persistent_item_rounds(items, n_cu)):
        if pick(slot, rnd):
            tn, tmi = conv_walk_item(t, tiles_m, tiles_n, walk)
            if new_block and (rnd < 1 or conv_walk_item(t - slots, tiles_m, tiles_n, walk)[0] == tn):
                continue
            mask[tmi // (ty * ty), (tmi // ty) % ty, tmi % ty, tn] = True
    return mask


# ---- conv_gb_resident (csrc/conv_gbr.hip): work decomposition, exact-embedding inputs, term references ------------------------
def gbr_ranges(B, r, N):
    """Host restatement of conv_gbr_ranges (csrc/forms.hip, MSR_GBR unset) -> (the planner's answer, 0 = not a layer for
    the resident kernel; what the test entries msr_op_spade_gbr* launch with: the entry falls back to 1)."""
    if r < 16 or (r & (r - 1)) or N % 128:
        return 0, 1
    tiles_p, tiles_n = B * (r // 16) * (r // 16), N // 128
    ranges = 1
    while tiles_p * ranges < 256 and ranges * 2 <= tiles_n and tiles_n % (ranges * 2) == 0:
        ranges *= 2
    if tiles_p * ranges < 128 or (tiles_n // ranges < 2 and tiles_p * ranges < 256 and r > 16):
        return 0, 1
    return ranges, ranges


def gbr_work(B, r, N, n_cu):
    """Host restatement of launch_conv_gbr + the item loop of conv_gb_resident for a launch through the test entries on a device
    with ``n_cu`` compute units: dict(ranges, nr, items, grid, slots, per_xcd (items of each XCD), rounds (int [items]: how many
    items the item's workgroup took before it), later (bool [B, r // 16, r // 16, N // 128]: the (pixel tile, channel block)
    pairs computed by an item of round >= 1), rng (int [items]), tile (int [items, 3]: b, ty, tx))."""
    t = r // 16
    tiles_p, tiles_n = B * t * t, N // 128
    ranges = gbr_ranges(B, r, N)[1]
    nr, items = tiles_n // ranges, tiles_p * ranges
    n_cu = max(n_cu & ~7, 8)
    grid = (items + 7) & ~7 if items < n_cu else n_cu
    sr = persistent_item_rounds(items, n_cu)
    item = np.arange(items)
    rng, tmi = item // tiles_p, item % tiles_p
    tile = np.stack([tmi // (t * t), (tmi // t) % t, tmi % t], 1)
    later = np.zeros((B, t, t, tiles_n), bool)
    for i in np.nonzero(sr[:, 1] >= 1)[0]:
        later[tile[i, 0], tile[i, 1], tile[i, 2], rng[i] * nr:(rng[i] + 1) * nr] = True
    per_xcd = [(items >> 3) + (1 if x < (items & 7) else 0) for x in range(8)]
    return dict(ranges=ranges, nr=nr, items=items, grid=grid, slots=grid >> 3, per_xcd=per_xcd, rounds=sr[:, 1], later=later,
                rng=rng, tile=tile)


def gbr_exact_inputs(B, S, r, N, seed, w_scale=0.25, bias_scale=0.25, m_lo=2.0 ** -6, shift=0):
    """Inputs of one SPADE layer for which the operands of conv_gb_resident's sweep are known bit for bit (host tensors):
      we    [3, 3, 2, 128]: non-zero only at the centre tap of mask channel 0, fp16 values with 2^-3 <= |we| < 1 (normal)
      be    zero
      src   [B, S, S, 2]: channel 0 fp16 values with m_lo <= |m| <= 0.5 (uniform in value, random sign; m_lo >= 2^-6), channel 1 arbitrary
    so that phase 1 computes e = relu(we[ch] * m[pixel]) as ONE exact 22-bit product, whatever its accumulation order, and
      w     [9][N][128] kernel-layout gamma|beta weights (spade_layout rows), randn * w_scale * logspace(-1.5, 1.5, N) over the
            columns, bias [N] = randn * bias_scale * the column's scale.
    -> dict(src, we, be, w, bias, mask [B, r, r] (channel 0 at the resize offsets), e [B, r, r, 128] fp32, exact; x
    [B, r >> shift, r >> shift, N / 2] = 3 + 2 randn with its per-channel mean and std)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)

    def f16_values(shape, e_lo, e_hi):       # sign * (1 + k / 1024) * 2^e, e_lo <= e < e_hi: 11 significant bits
        k = torch.randint(0, 1024, shape, generator=g).double()
        e = torch.randint(e_lo, e_hi, shape, generator=g).double()
        s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
        return (s * (1 + k / 1024) * torch.pow(2.0, e)).float()
    we = torch.zeros((3, 3, 2, 128))
    we[1, 1, 0] = f16_values((128,), -3, 0)
    src = torch.empty((B, S, S, 2))
    sign = torch.randint(0, 2, (B, S, S), generator=g).float() * 2 - 1
    src[..., 0] = sign * (m_lo + (0.5 - m_lo) * torch.rand((B, S, S), generator=g)).half().float()        # uniform in value
    src[..., 1] = torch.rand((B, S, S), generator=g) - 0.5
    ls = torch.logspace(-1.5, 1.5, N)
    w = torch.randn((9, N, 128), generator=g) * w_scale * ls[None, :, None]
    bias = torch.randn(N, generator=g) * bias_scale * ls
    assert m_lo >= 2.0 ** -6 and float(src[..., 0].abs().min()) >= 2.0 ** -6 and float(src[..., 0].abs().max()) <= 0.5
    f = S // r
    mask = src[:, f // 2::f, f // 2::f, 0][:, :r, :r].contiguous()
    e = torch.relu(we[1, 1, 0][None, None, None, :].double() * mask[..., None].double())
    assert torch.equal(e.float().double(), e) and torch.equal(we.half().float(), we) and torch.equal(src[..., 0].half().float(), src[..., 0])
    # the normalised tensor of the epilogue, as test_spade_layer_resident_kernel draws it (drawn last: the rest does not move)
    x = 3 + 2 * torch.randn((B, r >> shift, r >> shift, N // 2), generator=g)
    mean = x.mean((0, 1, 2)).contiguous()
    std = torch.sqrt(x.var((0, 1, 2), unbiased=False) + 1e-5).contiguous()
    return dict(src=src, we=we, be=torch.zeros(128), w=w, bias=bias, mask=mask, e=e.float(), x=x, mean=mean, std=std)


def gbr_x_parts(pieces, order):
    """ops.gbr_embedding_pieces -> the zero-bordered (hi, h6, l6) operands of f16c_terms, channels in the kernel's position
    ``order`` (ops.gbr_channel_order), and the zero-bordered tie distances (0, tie_h6, tie_l6) in the same form."""
    import torch
    pad = lambda t: pad_hw(t[..., order])       # noqa: E731
    zero = torch.zeros_like(pieces["hi"])
    return (tuple(pad(pieces[k]) for k in ("hi", "h6", "l6")), (pad(zero), pad(pieces["tie_h6"]), pad(pieces["tie_l6"])))


GBR_SLOPE = float(np.float32(0.2))


def gbr_epilogue(gb, rows, bias, nk=None, widen=None):
    """The SPADE epilogue on gamma|beta columns ``gb`` [B, r, r, len(rows)] of GEMM rows ``rows`` (all gamma rows or all beta
    rows): leaky_relu(gb + bias[rows]) for beta rows (nk None), leaky_relu((gb + bias[rows]) * nk) for gamma rows, slope =
    float32(0.2), in gb's dtype.  ``widen``: a per-element allowance on gb; returns (out, the allowance on out): |nk| times
    it, and the slope times that where the whole interval is negative (leaky relu is linear there, 1-Lipschitz elsewhere)."""
    import torch
    v = gb + bias[rows].to(gb.dtype)
    if nk is not None:
        v = v * nk.to(gb.dtype)
    out = torch.where(v >= 0, v, v * torch.tensor(GBR_SLOPE, dtype=gb.dtype, device=gb.device))
    if widen is None:
        return out
    wv = widen if nk is None else widen * nk.to(widen.dtype).abs()
    return out, torch.where(v + wv < 0, wv * GBR_SLOPE, wv)


def spade_rows(C):
    """GEMM rows of the gamma columns of output channels 0..C-1 (ops.spade_layout: 32 gamma | 32 beta; beta = + 32)."""
    import torch
    c = torch.arange(C)
    return (c // 32) * 64 + c % 32


def gbr_spade(gam, bet, bias_g, bias_b, xn, widen=None):
    """The whole SPADE epilogue in the operands' dtype: leaky_relu((gam + bias_g) * xn + bet + bias_b), slope = float32(0.2).
    ``widen`` = (allowance on gam, allowance on bet): returns (out, allowance on out) as gbr_epilogue does."""
    import torch
    dt = gam.dtype
    v = (gam + bias_g.to(dt)) * xn.to(dt) + bet + bias_b.to(dt)
    out = torch.where(v >= 0, v, v * torch.tensor(GBR_SLOPE, dtype=dt, device=v.device))
    if widen is None:
        return out
    wv = widen[0] * xn.to(dt).abs() + widen[1]
    return out, torch.where(v + wv < 0, wv * GBR_SLOPE, wv)


def gbr_term_figures(y, ref, ref32, widen=None):
    """The per-channel bound of tests/test_gpu_gbr_terms.py for one run.  y: the kernel's hi + lo8; ref: the float64 evaluation
    of the same terms; ref32: the same in plain fp32 (torch); widen: per-element tie allowance (None: none).
      bound[c] = (2^-14 + 4 * rel_linf_per_channel(ref32, ref)[c]) * max|ref[..., c]|     (f16c image + K-length allowance)
    -> dict(err: rel_linf_per_channel(y, ref); share: per channel, the largest |y - ref| / bound; share_wide: the largest
    |y - ref| / (bound + widen); beyond: per channel, the fraction of elements with |y - ref| > bound + widen;
    allowance: 4 * the fp32 figure per channel)."""
    import torch
    y, ref = torch.as_tensor(y).double(), torch.as_tensor(ref).double()
    C = ref.shape[-1]
    rng = ref.abs().reshape(-1, C).amax(0)
    allow = 4 * torch.as_tensor(rel_linf_per_channel(ref32, ref), device=ref.device)
    bound = (2.0 ** -14 + allow) * rng
    err = (y.to(ref.device) - ref).abs().reshape(-1, C)
    lim = bound[None, :] + (widen.double().reshape(-1, C) if widen is not None else 0)
    tiny = 1e-300
    return dict(err=rel_linf_per_channel(y, ref), share=(err / bound.clamp_min(tiny)[None, :]).amax(0).cpu().numpy(),
                share_wide=(err / lim.clamp_min(tiny)).amax(0).cpu().numpy(), beyond=(err > lim).double().mean(0).cpu().numpy(),
                allowance=allow.cpu().numpy(), range=rng.cpu().numpy())


# ---- NaN as data: one checker for every kernel (tests/test_nonfinite_host.py, tests/test_gpu_nonfinite.py) ------------------------
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_nan_contract(out, ref, clean, bound, err_fn, what="", exempt=None, raw=None):
    """The NaN contract of one launch whose input holds planted NaN elements (include/moonsr.h "Non-finite inputs").
      out    the kernel's output; for an image output the decoded MAIN piece (hi of the split / f16c formats, the bf8 byte)
      ref    the float64 reference of the same operation on the same input (torch follows IEEE: a NaN reaches every element
             that depends on it, so isnan(ref) is the plants' dependency footprint)
      clean  the output of the same launch with the planted elements replaced by 0.0
      bound, err_fn   the value bound of the kernel's own test: err_fn(out, ref) with the elements whose reference is not
             finite set to 0 in both (denominators over the finite reference elements only) must be <= bound everywhere
             (both may be arrays)
      exempt the reason why this case may leave fewer than half of its reference elements finite (None: it may not)
      raw    (out bytes, clean bytes, bool mask): further storage (cross pieces, scale bytes) that must be bit-identical where
             the mask is set
    Rules, in this order: 4 (cap, on the reference alone), 1 (mask: isnan(out) == isnan(ref) element by element), 2 (no spread:
    outside the footprint ``out`` is ``clean`` bit for bit), 3 (value).  An AssertionError names the first offending element.
    Returns dict(n_nan_ref, n_total, worst, bound): worst = the largest err_fn / bound share's numerator, bound its bound."""
    out, ref, clean = _np(out), _np(ref).astype(np.float64), _np(clean)
    assert out.shape == ref.shape == clean.shape, (what, out.shape, ref.shape, clean.shape)
    nan_ref = np.isnan(ref)
    finite = np.isfinite(ref)
    assert not (~finite & ~nan_ref).any(), f"{what}: the reference holds an infinity (out of scope: choose other inputs)"
    assert nan_ref.any(), f"{what}: the reference holds no NaN: nothing was planted where it matters"
    if exempt is None:
        assert 2 * int(finite.sum()) >= ref.size, f"{what}: only {int(finite.sum())} of {ref.size} reference elements are finite"
    nan_out = np.isnan(out.astype(np.float64))
    lost, extra = nan_ref & ~nan_out, nan_out & ~nan_ref
    if lost.any():
        at = tuple(int(v) for v in np.argwhere(lost)[0])
        raise AssertionError(f"{what}: lost NaN at {at}: the kernel wrote {out[at]!r} where the reference is NaN "
                             f"({int(lost.sum())} of {int(nan_ref.sum())} lost)")
    if extra.any():
        at = tuple(int(v) for v in np.argwhere(extra)[0])
        raise AssertionError(f"{what}: spread NaN at {at}: the kernel wrote NaN where the reference is {ref[at]!r} "
                             f"({int(extra.sum())} too many)")
    diff = (_bits(out) != _bits(clean)) & finite
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: changed bits outside the footprint at {at}: {out[at]!r} with the NaN planted, {clean[at]!r} "
                             f"with 0.0 in its place ({int(diff.sum())} elements)")
    if raw is not None:
        ro, rc, keep = _bits(_np(raw[0])), _bits(_np(raw[1])), _np(raw[2]).astype(bool)
        rd = (ro != rc) & keep
        if rd.any():
            at = tuple(int(v) for v in np.argwhere(rd)[0])
            raise AssertionError(f"{what}: changed stored bits outside the footprint at {at}: {ro[at]:#x} against {rc[at]:#x} "
                                 f"({int(rd.sum())} storage units)")
    err = np.asarray(err_fn(np.where(finite, out.astype(np.float64), 0.0), np.where(finite, ref, 0.0)), np.float64)
    lim = np.nan_to_num(np.asarray(bound, np.float64), nan=0.0)
    over = err > lim
    if over.any():
        at = tuple(int(v) for v in np.argwhere(over)[0]) if over.ndim else ()
        raise AssertionError(f"{what}: finite part beyond its bound at {at}: {float(err[at]) if over.ndim else float(err):.3e} > "
                             f"{float(np.broadcast_to(lim, err.shape)[at]) if over.ndim else float(lim):.3e}")
    share = err / np.maximum(lim, 1e-300)
    k = int(np.argmax(share)) if share.ndim else 0
    worst = float(err.reshape(-1)[k]) if err.ndim else float(err)
    return dict(n_nan_ref=int(nan_ref.sum()), n_total=int(ref.size), worst=worst,
                bound=float(np.broadcast_to(lim, err.shape).reshape(-1)[k]) if err.ndim else float(lim))


# ---- the pix2pix convs: EPI_AFFINE (tests/test_gpu_conv_affine.py, tests/test_gpu_pix2pix_sites.py) ------------------------------
P2P_KMAP = ((3, 1), (2, 0))      # upload_conv_weight, W_P2P_UP (csrc/api.hip): kmap[parity][t] = kernel row of 2 x 2 tap t


def p2p_parity_images(k_hwoi):
    """Python twin of the W_P2P_UP branch of upload_conv_weight (csrc/api.hip): Conv2DTranspose kernel [4, 4, Cout, Cin] -> the
    four parity images [py * 2 + px][t * 2 + u][Cout][Cin], image (py, px) tap (t, u) = kernel[kmap[py][t]][kmap[px][u]]."""
    import torch
    return torch.stack([torch.stack([k_hwoi[P2P_KMAP[py][t], P2P_KMAP[px][u]] for t in range(2) for u in range(2)])
                        for py in range(2) for px in range(2)]).contiguous()


def conv_taps_k(xpad, w_tnk, r, K, stride=1, oy=0, ox=0, dtype=None):
    """conv_taps for a K x K kernel read as the igemm kernels read it: tap (kh, kw) of output (y, x) is
    xpad[b, oy + y * stride + kh, ox + x * stride + kw]; w_tnk [K * K][N][C] -> [B, r, r, N] in ``dtype`` (float64)."""
    import torch
    dtype = dtype or torch.float64
    B, C = xpad.shape[0], xpad.shape[3]
    w = w_tnk.to(dtype)
    out = torch.empty((B, r, r, w.shape[1]), dtype=dtype, device=xpad.device)
    for b in range(B):
        xb = xpad[b].to(dtype)
        acc = torch.zeros((r * r, w.shape[1]), dtype=dtype, device=xpad.device)
        for kh in range(K):
            for kw in range(K):
                sl = xb[oy + kh: oy + kh + stride * r: stride, ox + kw: ox + kw + stride * r: stride]
                acc += sl.reshape(r * r, C) @ w[kh * K + kw].T
        out[b] = acc.reshape(r, r, -1)
    return out


def conv_transpose_scatter(x, k_hwoi, dtype=None):
    """Conv2DTranspose(4, strides 2, 'same') by its definition, input pixel (i, j) adds x[i, j] . k[kh, kw] to full-output pixel
    (2 i + kh, 2 j + kw) and 'same' crops one pixel per side: x [B, r, r, Cin], k [4, 4, Cout, Cin] -> [B, 2 r, 2 r, Cout] in
    ``dtype`` (float64).  No parity decomposition; sixteen matmuls, for the plain fp32 evaluation behind the K-length allowance."""
    import torch
    dtype = dtype or torch.float64
    B, r = x.shape[0], x.shape[1]
    k = k_hwoi.to(dtype)
    out = torch.empty((B, 2 * r, 2 * r, k.shape[2]), dtype=dtype, device=x.device)
    for b in range(B):
        full = torch.zeros((2 * r + 2, 2 * r + 2, k.shape[2]), dtype=dtype, device=x.device)
        xb = x[b].to(dtype).reshape(r * r, -1)
        for kh in range(4):
            for kw in range(4):
                full[kh: kh + 2 * r: 2, kw: kw + 2 * r: 2] += (xb @ k[kh, kw].T).reshape(r, r, -1)
        out[b] = full[1:-1, 1:-1]
    return out


def affine_act(pre, act, slope):
    """act of EPI_AFFINE on a pre-activation tensor: 0 none, 1 relu, 2 leaky_relu(slope), in pre's dtype."""
    import torch
    if act == 1:
        return torch.relu(pre)
    if act == 2:
        return torch.where(pre >= 0, pre, pre * slope)
    return pre


AFFINE_REL = 1e-5       # test_conv_bias's fp32 bound; tests/test_gpu_network_sites.py uses it for fp32 convs


def affine_site_check(out, pre, act, slope, out32=None, what="", parity=False):
    """The value check of one EPI_AFFINE conv, a function of (output, reference): ``out`` [B, H, W, C] what the kernel wrote,
    ``pre`` the float64 pre-activation reference scale * conv + shift, ``out32`` a plain fp32 torch evaluation of the same terms
    after the activation (None: no K-length allowance).  With ref = act(pre):
      tensor        max |out - ref| / max |ref| <= 1e-5
      per channel   max over pixels |out - ref| <= max(1e-5 * R_c, 4 * E_c), R_c = max over pixels |pre[..., c]| (before the
                    activation: after a ReLU a channel can be all zero), E_c = max over pixels |out32 - ref| of the channel
    -> dict(ok, tensor_rel, ratio (the largest error / bound over the channels), channel, index (b, y, x of that channel's worst
    element), parity ((y & 1, x & 1) of it when ``parity``), message).  The message of a failure names the channel, and the parity
    for a transposed conv's interleaved output."""
    import torch
    out = torch.as_tensor(out).double()
    pre = torch.as_tensor(pre).double().to(out.device)
    ref = affine_act(pre, act, slope)
    C = ref.shape[-1]
    err = (out - ref).abs()
    tensor_rel = float(err.max() / ref.abs().max().clamp_min(1e-300))
    ec = err.reshape(-1, C).amax(0)
    Rc = pre.abs().reshape(-1, C).amax(0)
    bound = AFFINE_REL * Rc
    allow = None
    if out32 is not None:
        allow = 4 * (torch.as_tensor(out32).double().to(out.device) - ref).abs().reshape(-1, C).amax(0)
        bound = torch.maximum(bound, allow)
    share = ec / bound.clamp_min(1e-300)
    c = int(torch.argmax(share))
    flat = int(torch.argmax(err[..., c].reshape(-1)))
    H, W = ref.shape[1], ref.shape[2]
    idx = (flat // (H * W), (flat // W) % H, flat % W)
    res = dict(ok=bool(tensor_rel <= AFFINE_REL and float(share[c]) <= 1.0), tensor_rel=tensor_rel, ratio=float(share[c]), channel=c,
               index=idx, parity=(idx[1] & 1, idx[2] & 1) if parity else None, range=float(Rc[c]), error=float(ec[c]),
               allowance=float(allow[c]) if allow is not None else 0.0)
    res["message"] = (f"{what}: channel {c}" + (f", parity (y & 1, x & 1) = {res['parity']}" if parity else "") +
                      f", element (b, y, x) = {idx}: |out - ref| = {res['error']:.3e}, {res['ratio']:.3g} x its bound "
                      f"(1e-5 * R_c = {AFFINE_REL * res['range']:.3e}, 4 * E_c = {res['allowance']:.3e}); tensor rel L-inf {tensor_rel:.3e}")
    return res

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

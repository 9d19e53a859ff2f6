"""Kernel-level host wrappers (parity tests and micro-benchmarks of single HIP kernels through the C ABI)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

EPI_BIAS, EPI_RES, EPI_SPADE = 0, 1, 2
EPI_RES_HEAD = 5        # the stream kernel's residual epilogue that emits the head's partial sums (csrc/kernels.h)
TILE_128, TILE_64, TILE_128_K16, TILE_HALO, TILE_HALO16, TILE_PP, TILE_FRAG, TILE_F16X2 = 0, 1, 2, 3, 4, 5, 0x40, 0x80


class OpContext:
    """A bare library handle (no weights) for launching single kernels on one device."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("moonsuperresolution_amd needs a HIP device (MI355X / gfx950); there is no CPU fallback")
        self.device = torch.device("cuda", device)
        cfg = _lib.MsrConfig(64, 1, 256, _lib.VARIANT_IDS["gaugan_no_kl"], device, 0)
        self.h = C.c_void_p()
        _lib.raise_for(self.lib, None, self.lib.msr_create(C.byref(cfg), C.byref(self.h)), "msr_create")

    def close(self):
        if self.h:
            self.lib.msr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pad_nhwc(x: torch.Tensor) -> torch.Tensor:
    """[B,r,r,C] -> zero-bordered [B,r+2,r+2,C] (the layout every conv_igemm input uses)."""
    B, r, _, Cc = x.shape
    p = torch.zeros((B, r + 2, r + 2, Cc), dtype=torch.float32, device=x.device)
    p[:, 1:-1, 1:-1] = x
    return p


def kernel_layout(w_hwio: torch.Tensor) -> torch.Tensor:
    """HWIO [3,3,Cin,Cout] -> [9][Cout][Cin]."""
    kh, kw, ci, co = w_hwio.shape
    return w_hwio.reshape(kh * kw, ci, co).permute(0, 2, 1).contiguous()


def spade_layout(wg: torch.Tensor, wb: torch.Tensor, bg: torch.Tensor, bb: torch.Tensor):
    """gamma / beta HWIO kernels -> one [9][2C][Cin] tensor with (32 gamma | 32 beta) interleaved rows + its bias."""
    Cc = wg.shape[3]
    c = torch.arange(Cc, device=wg.device)
    rows_g = (c // 32) * 64 + (c % 32)
    rows_b = rows_g + 32
    kg, kb = kernel_layout(wg), kernel_layout(wb)
    w = torch.empty((9, 2 * Cc, wg.shape[2]), dtype=torch.float32, device=wg.device)
    w[:, rows_g] = kg
    w[:, rows_b] = kb
    bias = torch.empty(2 * Cc, dtype=torch.float32, device=wg.device)
    bias[rows_g] = bg
    bias[rows_b] = bb
    return w.contiguous(), bias


def split_bf16(ctx: OpContext, x: torch.Tensor) -> torch.Tensor:
    """fp32 -> split-bf16 words (same shape, float32 storage)."""
    x = x.contiguous()
    out = torch.empty_like(x)
    rc = ctx.lib.msr_op_split_bf16(ctx.h, x.data_ptr(), out.data_ptr(), x.numel(),
                                   torch.cuda.current_stream(x.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_split_bf16")
    return out


def split_f16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> split-fp16 words: every aligned group of 32 values becomes [32 x hi f16 | 32 x lo f16] with
    hi = f16_rn(v), lo = f16_rn(v - hi) (the operand format of the 2-term gamma|beta mode); float32 storage."""
    x = x.contiguous()
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    hl = torch.stack([hi.reshape(-1, 32), lo.reshape(-1, 32)], 1).contiguous()     # [chunks][2][32]
    return hl.view(torch.int16).reshape(-1).view(torch.float32).reshape(x.shape)


def split_bf16_host(x: torch.Tensor) -> torch.Tensor:
    """Host restatement of the split-bf16 chunk image (kernels.h msr_store_split4): every aligned group of 32 values becomes
    [32 x hi bf16 | 32 x lo bf16] with hi = bf16_rn(v), lo = bf16_rn(v - hi); float32 storage, same shape."""
    x = x.contiguous()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    hl = torch.stack([hi.reshape(-1, 32), lo.reshape(-1, 32)], 1).contiguous()
    return hl.view(torch.int16).reshape(-1).view(torch.float32).reshape(x.shape)


def weights_bf16x3(w_kl: torch.Tensor) -> torch.Tensor:
    """Kernel-layout weights [taps][N][Cin] (fp32) -> the MFMA-fragment order conv_igemm_bf16x3 reads:
    [tap][chunk][n-tile][kg][hi|lo][lane = 32*h + j][8 bf16], returned as float32 storage of the same size."""
    taps, N, Cin = w_kl.shape
    hi = w_kl.to(torch.bfloat16)
    lo = (w_kl - hi.float()).to(torch.bfloat16)
    hl = torch.stack([hi, lo], 0)                                        # [2][tap][N][Cin]
    hl = hl.reshape(2, taps, N // 32, 32, Cin // 32, 2, 2, 8)            # [hl][tap][nt][j][cc][kg][h][e]
    hl = hl.permute(1, 4, 2, 5, 0, 6, 3, 7).contiguous()                 # [tap][cc][nt][kg][hl][h][j][e]
    return hl.view(torch.int16).reshape(-1).view(torch.float32).reshape(taps, N, Cin)


def conv3x3(ctx: OpContext, x_padded: torch.Tensor, w_kl: torch.Tensor, bias: torch.Tensor, rout: int, stride: int = 1,
            epilogue: int = EPI_BIAS, aux: Optional[torch.Tensor] = None, aux_shift: int = 0,
            mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, out_padded: bool = False,
            tile: int = -1, out: Optional[torch.Tensor] = None, precision: str = "fp32",
            out_split: bool = False) -> torch.Tensor:
    """One conv_igemm launch on torch's current stream.  x_padded [B, rout*stride+2, ., Cin].
    precision="bf16x3": x_padded must hold the split-bf16 chunk image (``split_bf16``); w_kl either the
    split-bf16 image of the kernel layout (``split_bf16(kernel_layout(w))``; tiles 0, 1, 3 = halo and 4 = halo on the 16x16x32 MFMA) or, with
    tile | TILE_FRAG, the fragment-order weights (``weights_bf16x3``; tiles 0 and 1, weights kept in VGPRs)."""
    B, Cin = x_padded.shape[0], x_padded.shape[3]
    N = w_kl.shape[1]
    Cout = N // 2 if epilogue == EPI_SPADE else N
    if out is None:
        shape = (B, rout + 2, rout + 2, Cout) if out_padded else (B, rout, rout, Cout)
        out = (torch.zeros if out_padded else torch.empty)(shape, dtype=torch.float32, device=x_padded.device)
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    stream = torch.cuda.current_stream(x_padded.device).cuda_stream
    if precision == "bf16x3":
        rc = ctx.lib.msr_op_conv3x3_bf16x3(ctx.h, x_padded.data_ptr(), w_kl.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                           B, rout, Cin, N, stride, epilogue, p(aux), aux_shift, p(mean), p(std),
                                           1 if out_padded else 0, 1 if out_split else 0, tile, stream)
    else:
        rc = ctx.lib.msr_op_conv3x3(ctx.h, x_padded.data_ptr(), w_kl.data_ptr(), bias.data_ptr(), out.data_ptr(), B,
                                    rout, Cin, N, stride, epilogue, p(aux), aux_shift, p(mean), p(std),
                                    1 if out_padded else 0, tile, stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_conv3x3")
    return out


def conv_affine(ctx: Optional[OpContext], x, in_off: int, in_pitch, w_kl, scale, shift, out, out_off: int, out_pitch,
                B: int, rout: int, cin: int, n: int, k: int, stride: int, act: int = 0, slope: float = 0.0, tile: int = -1):
    """One msr_op_conv_affine launch on torch's current stream (include/moonsr.h): out = act(conv * scale + shift) with explicit
    geometry.  ``x`` and ``out`` are the whole buffers; the kernel reads from element ``in_off`` of x with pitches ``in_pitch`` =
    (px, py, pb) and writes from element ``out_off`` of out with ``out_pitch``, all in floats.  w_kl [k * k][n][cin]; scale may be
    None.  Tensors may also be plain integer addresses, and ``ctx`` None: the entry validates before it looks at either, which is
    how the argument checks are tested without a device."""
    lib = ctx.lib if ctx is not None else _lib.load()
    h = ctx.h if ctx is not None else None
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()   # noqa: E731
    stream = torch.cuda.current_stream(x.device).cuda_stream if isinstance(x, torch.Tensor) and x.is_cuda else None
    rc = lib.msr_op_conv_affine(h, ptr(x) + 4 * in_off, in_pitch[0], in_pitch[1], in_pitch[2], ptr(w_kl), ptr(scale), ptr(shift),
                                ptr(out), out_off, out_pitch[0], out_pitch[1], out_pitch[2], B, rout, cin, n, k, k, stride, act,
                                slope, tile, stream)
    _lib.raise_for(lib, h, rc, "msr_op_conv_affine")
    return out


def fp8_weight_image(w_kl: torch.Tensor):
    """Kernel-layout weights [taps][N][Cin] (fp32) -> (e4m3 bytes [taps][N][Cpad] uint8, wexp [N] int32, dequantised
    fp32 weights) exactly as msr_load_weight quantises them for the fp8 mode: a power-of-two scale per output channel
    that puts the channel's largest |w| into e4m3's top binade."""
    taps, N, Cin = w_kl.shape
    cpad = 128 if Cin <= 128 else (Cin + 255) // 256 * 256
    amax = w_kl.abs().amax(dim=(0, 2)).double().cpu()
    e = torch.zeros(N, dtype=torch.int64)
    nz = amax > 0
    e[nz] = torch.frexp((amax[nz] / 448.0).float())[1].to(torch.int64)
    scale = torch.pow(2.0, e.double()).float().to(w_kl.device)
    q = (w_kl / scale[None, :, None]).to(torch.float8_e4m3fn)
    img = torch.zeros((taps, N, cpad), dtype=torch.uint8, device=w_kl.device)
    img[:, :, :Cin] = q.view(torch.uint8)
    b = (127 + e).to(torch.int64)
    wexp = (b | (b << 8) | (b << 16) | (b << 24)).to(torch.int32).to(w_kl.device)
    return img.contiguous(), wexp.contiguous(), q.float() * scale[None, :, None]


def bf8_activation_image(x_padded: torch.Tensor):
    """[B, r+2, r+2, C] fp32 -> (bf8 e5m2 bytes [B, r+2, r+2, Cpad] uint8, dequantised fp32 values)."""
    C_ = x_padded.shape[-1]
    cpad = 128 if C_ <= 128 else (C_ + 255) // 256 * 256
    q = x_padded.to(torch.float8_e5m2)
    img = torch.zeros(x_padded.shape[:-1] + (cpad,), dtype=torch.uint8, device=x_padded.device)
    img[..., :C_] = q.view(torch.uint8)
    return img.contiguous(), q.float()


def conv3x3_fp8(ctx: OpContext, x_bytes: torch.Tensor, w_bytes: torch.Tensor, wexp: torch.Tensor, bias: torch.Tensor,
                rout: int, epilogue: int = EPI_BIAS, aux: Optional[torch.Tensor] = None, aux_shift: int = 0,
                mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, out_padded: bool = False,
                out_mode: int = 0) -> torch.Tensor:
    """One launch of the fp8 form of the persistent ping-pong conv (msr_op_conv3x3_fp8)."""
    B, cpad = x_bytes.shape[0], x_bytes.shape[3]
    N = w_bytes.shape[1]
    Cout = N // 2 if epilogue == EPI_SPADE else N
    if out_mode == 3:
        opad = 128 if Cout <= 128 else (Cout + 255) // 256 * 256
        shape = (B, rout + 2, rout + 2, opad) if out_padded else (B, rout, rout, opad)
        out = torch.zeros(shape, dtype=torch.uint8, device=x_bytes.device)
    else:
        shape = (B, rout + 2, rout + 2, Cout) if out_padded else (B, rout, rout, Cout)
        out = torch.zeros(shape, dtype=torch.float32, device=x_bytes.device)
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = ctx.lib.msr_op_conv3x3_fp8(ctx.h, x_bytes.data_ptr(), w_bytes.data_ptr(), wexp.data_ptr(), bias.data_ptr(),
                                    out.data_ptr(), B, rout, cpad, N, epilogue, p(aux), aux_shift, p(mean), p(std),
                                    1 if out_padded else 0, out_mode, torch.cuda.current_stream(x_bytes.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_conv3x3_fp8")
    return out


def _f16c_pack(hi_f16: torch.Tensor, p_even: torch.Tensor, p_odd: torch.Tensor) -> torch.Tensor:
    """[..., C] f16 + two [..., C] float8 tensors -> the 128-byte chunk image per 32 channels, as float32 storage [..., C]:
    [32 x f16 | 32 bytes of the first float8 tensor | 32 bytes of the second]."""
    shp = hi_f16.shape
    n = shp[-1] // 32
    img = torch.empty(shp[:-1] + (n, 128), dtype=torch.uint8, device=hi_f16.device)
    img[..., 0:64] = hi_f16.contiguous().view(torch.uint8).reshape(shp[:-1] + (n, 64))
    e = p_even.contiguous().view(torch.uint8).reshape(shp[:-1] + (n, 32))
    o = p_odd.contiguous().view(torch.uint8).reshape(shp[:-1] + (n, 32))
    img[..., 64:96], img[..., 96:128] = e, o
    return img.reshape(shp[:-1] + (n * 128,)).view(torch.float32).reshape(shp)


def f16c_activation_image(x: torch.Tensor):
    """fp32 [..., C] (C % 32 == 0) -> (f16c chunk image as float32 storage, (hi, h8, lo8) de-quantised float64 parts):
    hi = f16_rn(v), h8 = e4m3(v), lo8 = e4m3((v - hi) * 2^11) / 2^11 — what the SPADE epilogue / mask embedding write."""
    hi = x.to(torch.float16)
    lo = x - hi.float()
    h8 = x.clamp(-448, 448).to(torch.float8_e4m3fn)
    l8 = (lo * 2048.0).clamp(-448, 448).to(torch.float8_e4m3fn)
    return _f16c_pack(hi, h8, l8), (hi.double(), h8.double(), l8.double() / 2048.0)


def f16c_weight_image(w_kl: torch.Tensor):
    """Kernel-layout weights [taps][N][Cin] -> (f16c image, wexp int32 [N], (hi, h8, lo8) de-quantised): pieces are stored
    lo-first so that piece g of a weight row pairs with piece g of an activation row (w_lo * x_hi, w_hi * x_lo)."""
    hi = w_kl.to(torch.float16)
    lo = w_kl - hi.float()

    def pow2exp(t):
        amax = t.abs().amax(dim=(0, 2)).float().cpu()
        e = torch.zeros(amax.shape, dtype=torch.int64)
        nz = amax > 0
        e[nz] = torch.frexp(amax[nz] / 448.0)[1].to(torch.int64)
        return e
    eh, el = pow2exp(w_kl), pow2exp(lo)
    sh = torch.pow(2.0, eh.double()).float().to(w_kl.device)[None, :, None]
    sl = torch.pow(2.0, el.double()).float().to(w_kl.device)[None, :, None]
    h8 = (w_kl / sh).to(torch.float8_e4m3fn)
    l8 = (lo / sl).to(torch.float8_e4m3fn)
    wexp = ((127 + el) | ((127 + eh) << 8)).to(torch.int32).to(w_kl.device)
    return _f16c_pack(hi, l8, h8), wexp.contiguous(), (hi.double(), h8.double() * sh.double(), l8.double() * sl.double())


# ---- f16c6: fp16 main term + fp6 e2m3 cross pieces with block scales (csrc/kernels.h PREC_F16C6) ------------------------------
_E2M3 = torch.tensor([i / 8 for i in range(8)] + [1 + i / 8 for i in range(8)] + [2 + i / 4 for i in range(8)] +
                     [4 + i / 2 for i in range(8)], dtype=torch.float64)


E2M3_TIE_RULES = ("even", "odd", "away", "zero")


def _e2m3_codes(q: torch.Tensor, ties: str = "even", with_ties: bool = False):
    """|q| <= 7.5 (float64) -> 6-bit codes (uint8), round to nearest.  A quotient that sits exactly on the midpoint of two
    codes goes to the even code (``ties="even"``: msr_f32_to_e2m3, the host side of the weight upload), to the other one
    ("odd": no converter's rule, the opposite of "even" on every tie), to the larger magnitude ("away") or the smaller
    ("zero").  The hardware converter v_cvt_scalef32_2xpk16_fp6_f32 rounds ties to EVEN as well: measured on an MI355X by
    tests/test_gpu_gbr_terms.py::test_tie_rule_of_the_fp6_converter (inputs with 2 % exact midpoints; the isolated cross terms
    of conv_gb_resident meet their rounding bound under "even" and miss it several hundred times over under the other three).
    ``with_ties``: also the bool mask of the tie elements and the distance of their two candidate codes in quotient units
    (float64, zero off the ties)."""
    if ties not in E2M3_TIE_RULES:
        raise ValueError(f"_e2m3_codes: ties is one of {E2M3_TIE_RULES}")
    grid = _E2M3.to(q.device)
    a = q.abs().clamp(max=7.5)
    mid = (grid[1:] + grid[:-1]) / 2
    idx = torch.bucketize(a, mid, right=False)
    # a tie sits exactly on a midpoint: bucketize(right=False) puts it in the lower bucket
    lo = idx.clamp(max=30)
    tie = (idx < 31) & (a == mid[lo])
    up = {"even": idx % 2 == 1, "odd": idx % 2 == 0, "away": torch.ones_like(tie), "zero": torch.zeros_like(tie)}[ties]
    idx = torch.where(tie & up, idx + 1, idx)
    codes = (idx.to(torch.uint8) | ((q < 0) & (a > 0)).to(torch.uint8) * 32).to(torch.uint8)
    if not with_ties:
        return codes
    return codes, tie, torch.where(tie, grid[lo + 1] - grid[lo], torch.zeros_like(a))


def _pack6(codes: torch.Tensor) -> torch.Tensor:
    """[..., 32] 6-bit codes -> [..., 24] bytes, little-endian bit string (element c at bits 6c..6c+5)."""
    c = codes.to(torch.int64).reshape(codes.shape[:-1] + (8, 4))
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)       # 24 bits per 4 codes
    b = torch.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], dim=-1)
    return b.reshape(codes.shape[:-1] + (24,)).to(torch.uint8)


def _f16c6_pack(hi: torch.Tensor, first: torch.Tensor, e_first: torch.Tensor, second: torch.Tensor, e_second: torch.Tensor):
    """hi [..., C] fp16, the two code pieces [..., C] and their e8m0 bytes [..., C // 32] -> float32 storage [..., C]."""
    shp = hi.shape
    n = shp[-1] // 32
    out = torch.zeros(shp[:-1] + (n, 128), dtype=torch.uint8, device=hi.device)
    out[..., 0:64] = hi.contiguous().view(torch.uint8).reshape(shp[:-1] + (n, 64))
    out[..., 64:88] = _pack6(first.reshape(shp[:-1] + (n, 32)))
    out[..., 88] = e_first.to(torch.uint8)
    out[..., 96:120] = _pack6(second.reshape(shp[:-1] + (n, 32)))
    out[..., 120] = e_second.to(torch.uint8)
    return out.reshape(shp[:-1] + (n * 128,)).view(torch.float32).reshape(shp)


def _pow2(E: torch.Tensor) -> torch.Tensor:
    """2^E as float64, built from the exponent bits: exact on every device (a device pow(2.0, E) may be an ulp off, which moves
    quotients that sit on a rounding tie to the other code)."""
    return ((E.to(torch.int64) + 1023) << 52).view(torch.float64)


def _ceil_log2_over(amax: torch.Tensor, top: float) -> torch.Tensor:
    """E = ceil(log2(amax / top)) as int64 (0 where amax == 0)"""
    m, e = torch.frexp((amax.double() / top))
    E = torch.where(m == 0.5, e - 1, e).to(torch.int64)
    return torch.where(amax > 0, E, torch.zeros_like(E))


def f16c6_activation_image(x: torch.Tensor):
    """fp32 [..., C] -> (f16c6 image, (hi, h6, l6) de-quantised float64 parts): one scale 2^E >= max|x| / 7.5 per pixel and
    32-channel chunk, h6 = e2m3(x / 2^E), l6 = e2m3((x - hi) / 2^(E - 11)) — what the SPADE epilogue writes."""
    shp = x.shape
    n = shp[-1] // 32
    hi = x.to(torch.float16)
    lo = (x - hi.float()).double()
    xb = x.double().reshape(shp[:-1] + (n, 32))
    # a NaN element is left out of its block's maximum (as the kernels' fmaxf does): it is NaN in hi, its 6-bit codes are free,
    # and the other 31 channels keep the bytes they would have had beside a zero
    E = _ceil_log2_over(torch.where(xb.isnan(), torch.zeros_like(xb), xb.abs()).amax(-1), 7.5).clamp(-100, 120)
    s = _pow2(E)[..., None]
    ch = _e2m3_codes(xb / s)
    cl = _e2m3_codes(lo.reshape(xb.shape) / (s / 2048.0))
    dec = lambda c: torch.where(c >= 32, -_E2M3.to(c.device)[(c & 31).long()], _E2M3.to(c.device)[(c & 31).long()])   # noqa: E731
    img = _f16c6_pack(hi, ch, 127 + E, cl, 127 + E - 11)
    return img, (hi.double(), (dec(ch) * s).reshape(shp), (dec(cl) * s / 2048.0).reshape(shp))


def block_e8m0(amax: torch.Tensor) -> torch.Tensor:
    """csrc/kernels.h msr_block_e8m0_dev bit for bit: fp32 block maxima -> the e8m0 byte (int64) of the block scale.  The
    device multiplies by float32(1 / 7.5) and lets a non-zero mantissa carry into the exponent; a maximum whose exact
    quotient sits within an ulp of a power of two may land a binade away from _ceil_log2_over's answer."""
    a = amax.to(torch.float32)
    inv = torch.ones((), dtype=torch.float32, device=a.device) / torch.full((), 7.5, dtype=torch.float32, device=a.device)
    bits = (a * inv).contiguous().view(torch.int32).to(torch.int64) + 0x7FFFFF
    eb = (bits >> 23) & 0xFF
    eb = torch.where(a > 0, eb, torch.full_like(eb, 127))
    return eb.clamp(27, 247)


def gbr_embedding_pieces(e: torch.Tensor, ties: str = "even"):
    """What phase 1 of conv_gb_resident (csrc/conv_gbr.hip) leaves in its LDS planes for the fp32 embedding ``e`` [..., 128]
    (already relu'd, zero outside the image): hi = f16_rn(e), and per pixel and 32-channel chunk the scale byte
    eb = block_e8m0(max e), h6 = e2m3(e / 2^(eb - 127)), l6 = e2m3((e - hi) / 2^(eb - 11 - 127)).  Returns a dict of float64
    tensors shaped like ``e``: hi, h6, l6 (pieces multiplied by their scales), tie_h6 / tie_l6 (zero, or at an element whose
    quotient is an exact midpoint the distance of its two candidate values: the tie rule of v_cvt_scalef32_2xpk16_fp6_f32
    decides between them; ``ties`` is the rule used here, see _e2m3_codes), and eb [..., 4] (int64).  The order of a chunk's
    channels (GBR_PERM) does not enter: a chunk shares one scale."""
    shp = e.shape
    n = shp[-1] // 32
    e = e.to(torch.float32)
    hi = e.to(torch.float16)
    lo = (e - hi.float()).double().reshape(shp[:-1] + (n, 32))            # exact in fp32: the kernel's la / lb
    eb = block_e8m0(e.reshape(shp[:-1] + (n, 32)).amax(-1))
    sh, sl = _pow2(eb - 127)[..., None], _pow2(eb - 11 - 127)[..., None]
    ch, th, dh = _e2m3_codes(e.double().reshape(lo.shape) / sh, ties, True)
    cl, tl, dl = _e2m3_codes(lo / sl, ties, True)
    dec = lambda c: torch.where(c >= 32, -_E2M3.to(c.device)[(c & 31).long()], _E2M3.to(c.device)[(c & 31).long()])   # noqa: E731
    return dict(hi=hi.double(), h6=(dec(ch) * sh).reshape(shp), l6=(dec(cl) * sl).reshape(shp), tie_h6=(dh * sh).reshape(shp),
                tie_l6=(dl * sl).reshape(shp), eb=eb)


def f16c6_weight_image(w_kl: torch.Tensor):
    """Kernel-layout weights [taps][N][Cin] -> (f16c6 image, (hi, h6, l6) de-quantised): one scale per output channel and piece;
    the lo piece is stored first so that half g of a weight row pairs with half g of an activation row."""
    hi = w_kl.to(torch.float16)
    lo = (w_kl - hi.float()).double()
    Eh = _ceil_log2_over(w_kl.abs().amax(dim=(0, 2)), 7.5).clamp(-100, 100)
    El = _ceil_log2_over(lo.abs().amax(dim=(0, 2)), 7.5).clamp(-100, 100)
    sh = _pow2(Eh)[None, :, None]
    sl = _pow2(El)[None, :, None]
    ch, cl = _e2m3_codes(w_kl.double() / sh), _e2m3_codes(lo / sl)
    n = w_kl.shape[-1] // 32
    eb = lambda E: (127 + E)[None, :, None].expand(w_kl.shape[0], -1, n)   # noqa: E731
    dec = lambda c: torch.where(c >= 32, -_E2M3.to(c.device)[(c & 31).long()], _E2M3.to(c.device)[(c & 31).long()])   # noqa: E731
    img = _f16c6_pack(hi, cl, eb(El), ch, eb(Eh))
    return img, (hi.double(), dec(ch) * sh, dec(cl) * sl)


def f16c6_decode(img: torch.Tensor):
    """f16c6 activation image -> (hi, h6, l6) float64 tensors [..., C] (pieces multiplied by their block scales)."""
    shp = img.shape
    n = shp[-1] // 32
    b = img.contiguous().view(torch.uint8).reshape(shp[:-1] + (n, 128)).long()
    hi = img.contiguous().view(torch.uint8).reshape(shp[:-1] + (n, 128))[..., 0:64].contiguous().view(torch.float16).reshape(shp).double()

    def piece(off):
        by = b[..., off:off + 24].reshape(shp[:-1] + (n, 8, 3))
        w = by[..., 0] | (by[..., 1] << 8) | (by[..., 2] << 16)
        c = torch.stack([(w >> (6 * k)) & 63 for k in range(4)], dim=-1).reshape(shp[:-1] + (n, 32))
        grid = _E2M3.to(img.device)
        v = torch.where(c >= 32, -grid[c & 31], grid[c & 31])
        s = _pow2(b[..., off + 24] - 127)[..., None]
        return (v * s).reshape(shp)
    return hi, piece(64), piece(96)


# ---- host twins of "the kernel was handed this scale": one output channel's e8m0 bytes moved, the decoded parts rescaled ----
def _check_e8m0(b: torch.Tensor, what: str):
    if int(b.min()) < 1 or int(b.max()) > 254:
        raise ValueError(f"{what}: a shifted scale byte leaves e8m0's finite range [1, 254]")


def _rescale_row(part: torch.Tensor, channel: int, d: int) -> torch.Tensor:
    out = part.clone()
    out[:, channel] = out[:, channel] * 2.0 ** d          # a power of two: exact
    return out


def f16c_weight_decode(w_img: torch.Tensor, wexp: torch.Tensor):
    """f16c weight image [taps][N][Cin] + wexp [N] -> (hi, h8, lo8) float64, as the kernels read them: bytes 64..95 of a chunk
    are the e4m3 codes of the lo piece (scale = byte 0 of wexp[n]), bytes 96..127 of the hi piece (scale = byte 1)."""
    shp = w_img.shape
    n = shp[-1] // 32
    b = w_img.contiguous().view(torch.uint8).reshape(shp[:-1] + (n, 128))
    hi = b[..., 0:64].contiguous().view(torch.float16).reshape(shp).double()
    l8 = b[..., 64:96].contiguous().view(torch.float8_e4m3fn).reshape(shp).double()
    h8 = b[..., 96:128].contiguous().view(torch.float8_e4m3fn).reshape(shp).double()
    e = wexp.to(torch.int64).to(w_img.device)
    sl, sh = _pow2((e & 255) - 127)[None, :, None], _pow2(((e >> 8) & 255) - 127)[None, :, None]
    return hi, h8 * sh, l8 * sl


def f16c_shift_wexp(wexp: torch.Tensor, wparts, channel: int, d_lo: int, d_hi: int):
    """A copy of ``wexp`` (f16c_weight_image) with the two e8m0 bytes of ONE output channel moved by d_lo / d_hi binades (byte 0
    = 127 + el scales the w_lo pieces, byte 1 = 127 + eh the w_h8 pieces), and the de-quantised (hi, h8, lo8) parts rescaled to
    match: what a kernel that is handed these scales must compute."""
    e = wexp.to(torch.int64).clone()
    lo, hi = (e[channel] & 255) + d_lo, ((e[channel] >> 8) & 255) + d_hi
    _check_e8m0(torch.stack([lo, hi]), "f16c_shift_wexp")
    e[channel] = (e[channel] & ~0xFFFF) | lo | (hi << 8)
    wh, w8, wl = wparts
    return e.to(torch.int32), (wh, _rescale_row(w8, channel, d_hi), _rescale_row(wl, channel, d_lo))


def f16c6_weight_decode(w_img: torch.Tensor):
    """f16c6 weight image -> (hi, h6, l6) float64 (the lo piece is stored first: f16c6_weight_image)."""
    hi, first, second = f16c6_decode(w_img)
    return hi, second, first


def f16c6_shift_wscale(w_img: torch.Tensor, wparts, channel: int, d_lo: int, d_hi: int):
    """The same for the f16c6 weight image, whose scales ride inside it: byte 88 (lo piece) and byte 120 (hi piece) of every
    128-byte chunk of weight row ``channel``, all taps.  Returns (image copy, rescaled (hi, h6, l6))."""
    shp = w_img.shape
    b = w_img.contiguous().view(torch.uint8).reshape(shp[0], shp[1], shp[2] // 32, 128).clone()
    lo, hi = b[:, channel, :, 88].to(torch.int64) + d_lo, b[:, channel, :, 120].to(torch.int64) + d_hi
    _check_e8m0(torch.stack([lo, hi]), "f16c6_shift_wscale")
    b[:, channel, :, 88], b[:, channel, :, 120] = lo.to(torch.uint8), hi.to(torch.uint8)
    wh, w6, wl = wparts
    return (b.reshape(shp[0], shp[1], -1).view(torch.float32).reshape(shp),
            (wh, _rescale_row(w6, channel, d_hi), _rescale_row(wl, channel, d_lo)))


def fp8_weight_decode(w_bytes: torch.Tensor, wexp: torch.Tensor, cin: int) -> torch.Tensor:
    """fp8 weight image [taps][N][Cpad] uint8 + wexp [N] -> de-quantised float64 weights [taps][N][cin] (scale = byte 0)."""
    e = wexp.to(torch.int64).to(w_bytes.device)
    return w_bytes[:, :, :cin].contiguous().view(torch.float8_e4m3fn).double() * _pow2((e & 255) - 127)[None, :, None]


def fp8_shift_wexp(wexp: torch.Tensor, wdq: torch.Tensor, channel: int, d: int):
    """The same for fp8_weight_image's wexp: the four equal e8m0 bytes of ONE channel moved by d binades."""
    e = wexp.to(torch.int64).clone() & 0xFFFFFFFF
    b = (e[channel] & 255) + d
    _check_e8m0(b.reshape(1), "fp8_shift_wexp")
    e[channel] = b | (b << 8) | (b << 16) | (b << 24)
    e = torch.where(e >= 2 ** 31, e - 2 ** 32, e)
    return e.to(torch.int32), _rescale_row(wdq, channel, d)


F16C_NO_CROSS = 0x10000     # msr_op_conv3x3_f16c out_mode bit: MSR_FLAG_F16_MAIN's form (x_hi * w_hi only, stream kernel)


def conv3x3_f16c(ctx: OpContext, x_img: torch.Tensor, w_img: torch.Tensor, wexp: torch.Tensor, bias: torch.Tensor, rout: int,
                 epilogue: int = EPI_BIAS, aux: Optional[torch.Tensor] = None, aux_shift: int = 0,
                 mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, out_padded: bool = False,
                 out_mode: int = 0, ksplit: int = 1, no_cross: bool = False) -> torch.Tensor:
    """One launch of the f16c conv (msr_op_conv3x3_f16c; the library sends it to the ping-pong or the stream kernel).
    ``wexp=None``: the operands are f16c6 images (fp6 pieces, stream kernel).  ``ksplit`` > 1: K ranges of the ping-pong kernel
    + the split-K epilogue pass (the planner's form for layers with fewer tiles than CUs); ``no_cross``: the cross terms left
    out (the f16 mode's stream kernel)."""
    B, Cin = x_img.shape[0], x_img.shape[3]
    N = w_img.shape[1]
    Cout = N // 2 if epilogue == EPI_SPADE else N
    shape = (B, rout + 2, rout + 2, Cout) if out_padded else (B, rout, rout, Cout)
    out = torch.zeros(shape, dtype=torch.float32, device=x_img.device)
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = ctx.lib.msr_op_conv3x3_f16c(ctx.h, x_img.data_ptr(), w_img.data_ptr(), p(wexp), bias.data_ptr(),
                                     out.data_ptr(), B, rout, Cin, N, epilogue, p(aux), aux_shift, p(mean), p(std),
                                     1 if out_padded else 0, out_mode | 256 * ksplit | (F16C_NO_CROSS if no_cross else 0),
                                     torch.cuda.current_stream(x_img.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_conv3x3_f16c")
    return out


GBR_PERM = [8 * (e >> 3) + 4 * (e & 1) + ((e >> 1) & 3) for e in range(32)]   # csrc/conv_gbr.hip: position e <- channel


def gbr_channel_order(cin: int = 128, device=None) -> torch.Tensor:
    """Input channel held by every position of the resident kernel's operands: position 32 c + e <- channel 32 c + GBR_PERM[e]."""
    return torch.tensor([32 * c + GBR_PERM[e] for c in range(cin // 32) for e in range(32)], device=device)


def gbr_weight_perm_image(w_kl: torch.Tensor):
    """Step 1 of gbr_weight_image: gamma|beta weights [9][N][128] (kernel layout, spade_layout rows) -> (the f16c6 weight image
    with the input channels of every 32-chunk in the kernel's position order, its de-quantised (hi, h6, l6) parts in that
    order).  This is the image whose fp16 plane, codes and scale bytes (88: l6, 120: h6) a test may edit before step 2."""
    return f16c6_weight_image(w_kl[:, :, gbr_channel_order(w_kl.shape[2], w_kl.device)].contiguous())


def gbr_weight_stream(img: torch.Tensor) -> torch.Tensor:
    """Step 2 of gbr_weight_image: the f16c6 weight image [9][N][128] (float32 storage) re-ordered into the order the waves of
    conv_gb_resident load it: [channel block nt][wave q][tap pair P][column block j][piece][lane] x 16 bytes
    (csrc/conv_gbr.hip, weight_images.hip gbr_weight_stream).  Same shape and byte count."""
    N = img.shape[1]
    rec = img.contiguous().view(torch.uint8).reshape(9, N, 4, 128)                 # [tap][row][chunk][128 bytes]
    dev = img.device
    nt, q, P, j, piece, lane = torch.meshgrid(torch.arange(N // 128), torch.arange(4), torch.arange(18), torch.arange(2),
                                              torch.arange(4), torch.arange(64), indexing="ij")
    px, cg = lane & 15, lane >> 4
    row = 128 * nt + 64 * (q >> 1) + 16 * (q & 1) + 32 * j + px
    T = torch.where(piece < 2, 2 * P + piece, 2 * P + (cg >> 1))
    off = torch.where(piece < 2, 16 * cg, 64 + 32 * (cg & 1) + 16 * (piece - 2))
    tap, chunk = (T % 9).to(dev), (T // 9).to(dev)
    byte = off.to(dev)[..., None] + torch.arange(16, device=dev)
    out = rec[tap[..., None], row.to(dev)[..., None], chunk[..., None], byte]        # [..., 16] bytes
    return out.contiguous().reshape(-1).view(torch.float32).reshape(9, N, 128)


def gbr_weight_image(w_kl: torch.Tensor) -> torch.Tensor:
    """gamma|beta weights [9][N][128] (kernel layout, spade_layout rows) -> the weight STREAM conv_gb_resident reads:
    gbr_weight_stream(gbr_weight_perm_image(w_kl)).  Returned as float32 storage [9][N][128] (same byte count)."""
    return gbr_weight_stream(gbr_weight_perm_image(w_kl)[0])


def f16c6_weight_keep(w_img: torch.Tensor, hi: bool = True, h6: bool = True, l6: bool = True, rows=None, lift: int = 0):
    """A copy of an f16c6 WEIGHT image [taps][N][Cin] with pieces zeroed: the fp16 plane (bytes 0..63 of a chunk), the l6 codes
    (64..87) or the h6 codes (96..119); the scale bytes stay.  ``rows``: bool [N], rows to keep at all (the others lose all
    three pieces).  ``lift``: binades added to both scale bytes (88, 120) of every row, so that a cross term that is handed
    to a kernel alone comes out on the main term's scale (2^lift times the term, exact).  f16c6_weight_decode of the result
    is what the kernel then multiplies."""
    shp = w_img.shape
    b = w_img.contiguous().view(torch.uint8).reshape(shp[0], shp[1], shp[2] // 32, 128).clone()
    if not hi:
        b[..., 0:64] = 0
    if not l6:
        b[..., 64:88] = 0
    if not h6:
        b[..., 96:120] = 0
    if rows is not None:
        drop = ~rows.to(b.device)
        b[:, drop, :, 0:88] = 0
        b[:, drop, :, 96:120] = 0
    if lift:
        s = b[..., [88, 120]].to(torch.int64) + lift
        _check_e8m0(s, "f16c6_weight_keep")
        b[..., 88], b[..., 120] = s[..., 0].to(torch.uint8), s[..., 1].to(torch.uint8)
    return b.reshape(shp[0], shp[1], -1).view(torch.float32).reshape(shp)


def spade_gbr(ctx: OpContext, src: torch.Tensor, we: torch.Tensor, be: torch.Tensor, w_img: torch.Tensor, bias: torch.Tensor,
              r: int, x: torch.Tensor, aux_shift: int, mean: torch.Tensor, std: torch.Tensor, no_cross: bool = False,
              out_mode: int = 4) -> torch.Tensor:
    """One launch of conv_gb_resident (msr_op_spade_gbr; ``no_cross``: msr_op_spade_gbr_f16, the f16 mode's form): resize +
    mask embedding + gamma|beta conv + SPADE epilogue; returns the zero-bordered f16c image [B, r + 2, r + 2, C] (float32
    storage; f16c_decode reads it).  ``out_mode=5`` (msr_op_spade_gbr_f16c6): the f16c6 image instead (f16c6_decode)."""
    if out_mode not in (4, 5) or (out_mode == 5 and no_cross):
        raise ValueError("spade_gbr: out_mode is 4 (f16c image) or 5 (f16c6 image, not with no_cross)")
    B, S = src.shape[0], src.shape[1]
    N = w_img.shape[1]
    out = torch.zeros((B, r + 2, r + 2, N // 2), dtype=torch.float32, device=src.device)
    fn = ctx.lib.msr_op_spade_gbr_f16 if no_cross else (ctx.lib.msr_op_spade_gbr_f16c6 if out_mode == 5 else ctx.lib.msr_op_spade_gbr)
    rc = fn(ctx.h, src.data_ptr(), S, we.data_ptr(), be.data_ptr(), w_img.data_ptr(), bias.data_ptr(), out.data_ptr(), B, r, N,
            x.data_ptr(), aux_shift, mean.data_ptr(), std.data_ptr(), torch.cuda.current_stream(src.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_spade_gbr")
    return out


def gbr_embed_image(we_hwio: torch.Tensor) -> torch.Tensor:
    """Mask-embedding kernel HWIO [3, 3, 2, 128] -> the fp16 A operands of conv_gb_resident's phase 1 (conv_gbr.hip
    conv_gbr_embed_image, uploaded as <kernel>.e16): [channel quarter 4][instruction 4][lane 64] x 8 fp16.  K slot pair
    P = 8 j + 4 (lane >> 5) + u carries term P // 9 (0, 1: w_hi, 2: w_lo = f16_rn(w - w_hi)) of tap P % 9 for both mask
    channels, output channel 32 wq + (lane & 31); P >= 27 is zero.  Returned as float32 storage [4096]."""
    w = we_hwio.reshape(9, 2, 128).float().cpu()
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    wq, j, lane, u, c = torch.meshgrid(torch.arange(4), torch.arange(4), torch.arange(64), torch.arange(4), torch.arange(2),
                                       indexing="ij")
    P = 8 * j + 4 * (lane >> 5) + u
    ch = 32 * wq + (lane & 31)
    tap = (P % 9).clamp(max=8)
    v = torch.where(P // 9 == 2, lo[tap, c, ch], hi[tap, c, ch])
    v = torch.where(P < 27, v, torch.zeros_like(v))
    return v.contiguous().view(torch.int16).reshape(-1).view(torch.float32).clone()


def head_taps_upconv(k44c: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """Head kernel [4, 4, C] (Conv2D(1, 4, 'same') after UpSampling2D(2), networks.py:54-56) -> the effective per-parity taps
    weff[py][px][dy + 1][dx + 1][C] the head kernel reads (weight_images.hip head_weff_upconv, uploaded as gen.head.weff): TF SAME for
    k = 4 pads 1 before / 2 after, so output parity p reads half-resolution offsets {-1, 0, 0, +1} (p = 0) or {0, 0, +1, +1}
    (p = 1) for kh = 0..3; taps that land on the same pixel are added in fp32 (``dtype``: float64 for a reference), in kh, kw
    order."""
    k = k44c.to(dtype).cpu()
    dmap = lambda parity, t: (0 if t == 0 else 2 if t == 3 else 1) if parity == 0 else (1 if t < 2 else 2)   # noqa: E731
    weff = torch.zeros((2, 2, 3, 3, k.shape[2]), dtype=dtype)
    for py in range(2):
        for px in range(2):
            for kh in range(4):
                for kw in range(4):
                    weff[py, px, dmap(py, kh), dmap(px, kw)] += k[kh, kw]
    return weff


def head_slots() -> dict:
    """Slot table of the fused head's partial sums (csrc/kernels.h HEAD_SLOTS): {(py, px, dy, dx): slot} for the 25 live
    entries of ``head_taps_upconv``'s weff[py][px][dy][dx] (dy >= py and dx >= px), counted in py, px, dy, dx order; slots
    25..31 of a line are zero."""
    table, n = {}, 0
    for py in range(2):
        for px in range(2):
            for dy in range(py, 3):
                for dx in range(px, 3):
                    table[(py, px, dy, dx)] = n
                    n += 1
    return table


def head_partials(x: torch.Tensor, k44c: torch.Tensor) -> torch.Tensor:
    """What the head epilogue computes, in the dtype of ``x`` [B, r, r, C] (host): P[b, y, x, slot] = sum_c weff[slot][c] *
    leaky_relu(x[b, y, x, c], 0.2), 32 slots per pixel (``head_slots``), the coinciding taps summed in that dtype too."""
    weff = head_taps_upconv(k44c, x.dtype)
    a = torch.where(x >= 0, x, 0.2 * x)
    P = torch.zeros(tuple(x.shape[:3]) + (32,), dtype=x.dtype)
    for (py, px, dy, dx), s in head_slots().items():
        P[..., s] = a @ weff[py, px, dy, dx]
    return P


def head_from_partials(P: torch.Tensor, bias: float) -> torch.Tensor:
    """The gather of the fused head restated in torch, in the dtype of ``P`` [B, r, r, 32] (float32 or float64, host or
    device): out[b, 2i + py, 2j + px] = bias + sum over the live (dy, dx) of P[b, i + dy - 1, j + dx - 1, slot(py, px, dy, dx)],
    zero outside the image, summed in the kernel's order (dy, then dx, the bias last)."""
    B, r = P.shape[0], P.shape[1]
    pad = torch.zeros((B, r + 2, r + 2, 32), dtype=P.dtype, device=P.device)
    pad[:, 1:-1, 1:-1] = P
    out = torch.zeros((B, 2 * r, 2 * r), dtype=P.dtype, device=P.device)
    slots = head_slots()
    for py in range(2):
        for px in range(2):
            acc = torch.zeros((B, r, r), dtype=P.dtype, device=P.device)
            for dy in range(py, 3):
                for dx in range(px, 3):
                    acc = acc + pad[:, dy:dy + r, dx:dx + r, slots[(py, px, dy, dx)]]
            out[:, py::2, px::2] = acc + bias
    return out


def conv3x3_f16c_head(ctx: OpContext, x_img: torch.Tensor, w_img: torch.Tensor, wexp: torch.Tensor, bias: torch.Tensor, rout: int,
                      aux: torch.Tensor, aux_shift: int, head_kernel: "np.ndarray", head_bias: float, want_partial: bool = False):
    """The fused head at kernel level (msr_op_conv3x3_f16c_head): the f16c residual conv on the stream kernel with the head
    epilogue, then the gather.  ``head_kernel`` [4, 4, 128] float32 (host).  Returns out [B, 2 rout, 2 rout], and with
    ``want_partial`` also the partial sums [B, rout, rout, 32]."""
    import numpy as np
    B, Cin = x_img.shape[0], x_img.shape[3]
    N = w_img.shape[1]
    k = np.ascontiguousarray(head_kernel, dtype=np.float32)
    assert k.shape == (4, 4, 128)
    out = torch.zeros((B, 2 * rout, 2 * rout), dtype=torch.float32, device=x_img.device)
    part = torch.zeros((B, rout, rout, 32), dtype=torch.float32, device=x_img.device) if want_partial else None
    rc = ctx.lib.msr_op_conv3x3_f16c_head(ctx.h, x_img.data_ptr(), w_img.data_ptr(), wexp.data_ptr(), bias.data_ptr(), B, rout, Cin,
                                          N, aux.data_ptr(), aux_shift, k.ctypes.data_as(C.c_void_p), float(head_bias),
                                          out.data_ptr(), part.data_ptr() if want_partial else None,
                                          torch.cuda.current_stream(x_img.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_conv3x3_f16c_head")
    return (out, part) if want_partial else out


def heads_concat(mean: torch.Tensor, variance: torch.Tensor) -> torch.Tensor:
    """The encoder's two heads as msr_load_weight stores them (enc.heads.kernel [K, 2L], enc.heads.bias [2L]): mean | variance
    side by side along the last axis, so that the flattened encoder output is streamed once."""
    return torch.cat([mean, variance], dim=-1).contiguous()


SMALLCIN_STRIDE2, SMALLCIN_EMBED = 0, 1     # msr_op_conv_smallcin index maps: encoder block 1 / SPADE mask embedding


def conv_smallcin(ctx: OpContext, src: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], hout: int, index_map: int,
                  act: int = 0, slope: float = 0.0, out_split: int = 0, out_padded: bool = False) -> torch.Tensor:
    """One launch of conv_smallcin (msr_op_conv_smallcin): src [B, S, S, 2], w HWIO [3, 3, 2, Cout].  Returns float32 storage
    [B, hout (+2), hout (+2), slots] with slots = Cout, or 32 for bf8 bytes (out_split 3); a padded output starts zeroed."""
    B, S, Cout = src.shape[0], src.shape[1], w.shape[3]
    slots = 32 if out_split == 3 else Cout
    shape = (B, hout + 2, hout + 2, slots) if out_padded else (B, hout, hout, slots)
    out = torch.zeros(shape, dtype=torch.float32, device=src.device)
    rc = ctx.lib.msr_op_conv_smallcin(ctx.h, src.contiguous().data_ptr(), S, w.contiguous().data_ptr(),
                                      bias.data_ptr() if bias is not None else None, out.data_ptr(), B, hout, Cout, index_map,
                                      act, float(slope), out_split, 1 if out_padded else 0,
                                      torch.cuda.current_stream(src.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_conv_smallcin")
    return out


def norm_act(ctx: OpContext, x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
             slope: float = 0.2, out_padded: bool = False, out_split: bool = False) -> torch.Tensor:
    """One launch of norm_act (msr_op_norm_act): x dense [B, H, W, C], mean / std [B, C], gamma / beta [C]."""
    B, H, W, Cc = x.shape
    shape = (B, H + 2, W + 2, Cc) if out_padded else (B, H, W, Cc)
    out = torch.zeros(shape, dtype=torch.float32, device=x.device)
    rc = ctx.lib.msr_op_norm_act(ctx.h, x.contiguous().data_ptr(), mean.contiguous().data_ptr(), std.contiguous().data_ptr(),
                                 gamma.contiguous().data_ptr(), beta.contiguous().data_ptr(), out.data_ptr(), B, H, W, Cc,
                                 float(slope), 1 if out_padded else 0, 1 if out_split else 0,
                                 torch.cuda.current_stream(x.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_norm_act")
    return out


def dense(ctx: OpContext, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One dense layer (msr_op_dense, synchronous): x [B, K] (B <= 16), w [K, N] -> [B, N]."""
    B, K = x.shape
    N = w.shape[1]
    y = torch.empty((B, N), dtype=torch.float32, device=x.device)
    rc = ctx.lib.msr_op_dense(ctx.h, x.contiguous().data_ptr(), w.contiguous().data_ptr(),
                              bias.data_ptr() if bias is not None else None, y.data_ptr(), B, K, N,
                              torch.cuda.current_stream(x.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_dense")
    return y


def latent(ctx: OpContext, mv: torch.Tensor, eps: Optional[torch.Tensor], sampler: int) -> torch.Tensor:
    """The latent sampler (msr_op_latent): mv [B, 2L] -> z [B, L] = m + exp(v / 2) * eps (sampler 1) or m + v (sampler 0)."""
    B, L = mv.shape[0], mv.shape[1] // 2
    z = torch.empty((B, L), dtype=torch.float32, device=mv.device)
    rc = ctx.lib.msr_op_latent(ctx.h, mv.contiguous().data_ptr(), eps.contiguous().data_ptr() if eps is not None else None,
                               z.data_ptr(), B, L, sampler, torch.cuda.current_stream(mv.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_latent")
    return z


def f16c_decode(img: torch.Tensor):
    """f16c activation image (float32 storage [..., C]) -> (hi, h8, lo8) as float64 tensors [..., C]."""
    shp = img.shape
    n = shp[-1] // 32
    b = img.contiguous().view(torch.uint8).reshape(shp[:-1] + (n, 128))
    hi = b[..., 0:64].contiguous().view(torch.float16).reshape(shp).double()
    h8 = b[..., 64:96].contiguous().view(torch.float8_e4m3fn).reshape(shp).double()
    l8 = b[..., 96:128].contiguous().view(torch.float8_e4m3fn).reshape(shp).double()
    return hi, h8, l8 / 2048.0


def moments(ctx: OpContext, x: torch.Tensor, eps: float):
    """One run of the moments kernels (msr_op_moments): x [G, P, C] float32 -> (mean, std), each [G, C], with
    std = sqrtf(float(biased variance) + eps) — the moments of every normalisation in the generator."""
    G, P, Cc = x.shape
    x = x.contiguous()
    mean = torch.empty((G, Cc), dtype=torch.float32, device=x.device)
    std = torch.empty_like(mean)
    rc = ctx.lib.msr_op_moments(ctx.h, x.data_ptr(), G, P, Cc, float(eps), mean.data_ptr(), std.data_ptr(),
                                torch.cuda.current_stream(x.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_moments")
    return mean, std


def head(ctx: OpContext, x: torch.Tensor, kernel: "np.ndarray", bias: float, slope: float = 0.2, transpose_tanh: bool = False) -> torch.Tensor:
    """One launch of the head kernel (msr_op_head): x dense [B, r, r, C] -> [B, 2r, 2r].  kernel [4, 4, C] float32 (host):
    the Conv2D(1, 4, 'same') kernel applied after UpSampling2D(2) (networks.py:54-56), or with ``transpose_tanh`` the
    Conv2DTranspose(1, 4, 2, 'same') kernel followed by tanh (pix2pix.py:53-57)."""
    import numpy as np
    B, r, _, Cc = x.shape
    k = np.ascontiguousarray(kernel, dtype=np.float32)
    assert k.shape == (4, 4, Cc)
    out = torch.empty((B, 2 * r, 2 * r), dtype=torch.float32, device=x.device)
    rc = ctx.lib.msr_op_head(ctx.h, x.contiguous().data_ptr(), k.ctypes.data_as(C.c_void_p), float(bias), out.data_ptr(), B, r, Cc,
                             float(slope), 1 if transpose_tanh else 0, torch.cuda.current_stream(x.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_head")
    return out


# ---- activation-range scan (csrc/range_scan.hip, include/moonsr.h msr_range_scan) ---------------------------------------------
RANGE_FORMATS = (2, 3, 4, 5)        # out_split values with a finite range: split-fp16, bf8 bytes, f16c, f16c6
F16_MAX, BF8_MAX = 65504.0, 57344.0


def e4m3_cross_limit() -> float:
    """The largest fp16 value whose e4m3 piece is not changed by the saturation at 448: the largest fp16 that
    round-to-nearest-even takes to 448 (``torch.float8_e4m3fn`` has no 480: above the midpoint the conversion overflows).
    It is 464, the midpoint of 448 and the 480 the grid would continue with; the tie goes to 448, whose mantissa is even."""
    v = torch.arange(448, 513, 0.25, dtype=torch.float32).to(torch.float16)          # every fp16 of [448, 512]: spacing 0.25
    ok = v.float().to(torch.float8_e4m3fn).float() == 448.0
    return float(v[ok].max())


def range_stats(img: torch.Tensor, fmt: int, padded: bool, channels: Optional[int] = None) -> dict:
    """Host twin of the range scan, from the DECODED image: the record msr_op_range_scan / msr_range_scan give for one
    activation image [B, r (+2), r (+2), .] in format ``fmt`` (2 split-fp16, 4 f16c, 5 f16c6: float32 storage, one slot per
    channel; 3: bf8 bytes, ``channels`` real channels in a pixel padded with zero bytes).  The zero border of a padded image and
    the padding channels are left out.  Returns max_abs (np.float32, the largest finite \\|main piece\\|) and the four counts."""
    import numpy as np
    if fmt not in RANGE_FORMATS:
        raise ValueError(f"format {fmt} has fp32's range and is not scanned; expected one of {RANGE_FORMATS}")
    img = img.detach().cpu().contiguous()
    if padded:
        img = img[:, 1:-1, 1:-1].contiguous()
    if fmt == 3:
        b = img.view(torch.uint8) if img.dtype != torch.uint8 else img
        hi = b[..., :channels if channels is not None else b.shape[-1]].contiguous().view(torch.float8_e5m2).double()
        top = BF8_MAX
    elif fmt == 4:
        hi, top = f16c_decode(img)[0], F16_MAX
    elif fmt == 5:
        hi, top = f16c6_decode(img)[0], F16_MAX
    else:
        words = img.view(torch.int16).reshape(-1, 2, 32)                       # [chunk][hi | lo][32]
        hi, top = words[:, 0].contiguous().view(torch.float16).double(), F16_MAX
    mag = hi.abs()
    finite = torch.isfinite(mag)
    cross = int((~(mag <= e4m3_cross_limit())).sum()) if fmt == 4 else 0       # a NaN piece is clipped as well
    return dict(max_abs=np.float32(mag[finite].max()) if bool(finite.any()) else np.float32(0.0), n_total=int(mag.numel()),
                n_cross_clipped=cross, n_clamped=int((mag == top).sum()), n_nonfinite=int((~finite).sum()))


def range_stat_dict(rec) -> dict:
    """An msr_range_stat (``_lib.MsrRangeStat``) as a dict; max_abs stays an np.float32 (compared bit for bit in the tests)."""
    import numpy as np
    return dict(tensor=rec.tensor.decode(), format=int(rec.format), producer=int(rec.producer), max_abs=np.float32(rec.max_abs),
                n_total=int(rec.n_total), n_cross_clipped=int(rec.n_cross_clipped), n_clamped=int(rec.n_clamped),
                n_nonfinite=int(rec.n_nonfinite))


def range_scan(ctx: OpContext, img: torch.Tensor, fmt: int, B: int, r: int, channels: int, padded: bool) -> dict:
    """One synchronous scan of a device image (msr_op_range_scan); the layout is what ``range_stats`` takes."""
    rec = _lib.MsrRangeStat()
    rc = ctx.lib.msr_op_range_scan(ctx.h, img.contiguous().data_ptr(), fmt, B, r, channels, 1 if padded else 0, C.byref(rec),
                                   torch.cuda.current_stream(img.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_op_range_scan")
    return range_stat_dict(rec)


# ---- counter-based sampler noise (csrc/sampler.hip, include/moonsr.h msr_sampler_noise) ---------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 on uint32 arrays: ``counter`` [..., 4], ``key`` [..., 2] (broadcast against each other) -> [..., 4]."""
    import numpy as np
    c = np.asarray(counter).astype(np.uint32)
    k = np.asarray(key).astype(np.uint32)
    if c.shape[-1] != 4 or k.shape[-1] != 2:
        raise ValueError(f"counter must be [..., 4] and key [..., 2], got {c.shape} and {k.shape}")
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).astype(np.uint64) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).astype(np.uint64) for i in range(2))
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2       # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _f32(hexfloat: str):
    import numpy as np
    return np.float32(float.fromhex(hexfloat))        # every constant of the recipe is a float32 written exactly


def _clz32(n):
    """Leading zeros of uint32 values (32 for 0), by binary search with shifts."""
    import numpy as np
    x = n.astype(np.uint32)
    lz = np.zeros(x.shape, np.int32)
    for sh in (16, 8, 4, 2, 1):
        top_clear = (x >> np.uint32(32 - sh)) == 0
        lz += np.where(top_clear, sh, 0).astype(np.int32)
        x = np.where(top_clear, x << np.uint32(sh), x)
    return lz + (x == 0)                              # all 32 shifted out: the value was 0


def _sampler_radius(n):
    """sqrt(-2 ln u), u = (n + 0.5) / 2^32, op for op as csrc/sampler.hip::radius (float32 throughout)."""
    import numpy as np
    one, half = np.float32(1.0), np.float32(0.5)
    lz = _clz32(n)
    t = ((((n.astype(np.uint64) << np.uint64(1)) | np.uint64(1)) << lz.astype(np.uint64)) >> np.uint64(9)).astype(np.uint32)
    m = t.astype(np.float32) * _f32("0x1p-23")
    e = -1 - lz
    big = t >= np.uint32(0xB504F4)
    m = np.where(big, m * half, m)
    e = np.where(big, e + 1, e)
    s = (m - one) / (m + one)
    s2 = s * s
    p = np.full(s.shape, _f32("0x1.c71c72p-4"), np.float32)
    p = p * s2 + _f32("0x1.24924ap-3")
    p = p * s2 + _f32("0x1.99999ap-3")
    p = p * s2 + _f32("0x1.555556p-2")
    p = p * s2 + one
    lnm = (s + s) * p
    ln = e.astype(np.float32) * _f32("0x1.62e43p-1") + lnm
    return np.sqrt(np.float32(-2.0) * ln)


def _sampler_cos_sin(n):
    """(cos, sin) of 2 pi (n + 0.5) / 2^32, op for op as csrc/sampler.hip::cos_sin."""
    import numpy as np
    one, half = np.float32(1.0), np.float32(0.5)
    octant = n >> np.uint32(29)
    f = n & np.uint32(0x1FFFFFFF)
    f = np.where((octant & np.uint32(1)) != 0, np.uint32(0x1FFFFFFF) - f, f)
    a = (((f >> np.uint32(6)) << np.uint32(1)) | np.uint32(1)).astype(np.float32) * _f32("0x1p-24")
    x = a * _f32("0x1.921fb6p-1")
    x2 = x * x
    ps = np.full(x.shape, _f32("0x1.71de3ap-19"), np.float32)
    ps = ps * x2 - _f32("0x1.a01a02p-13")
    ps = ps * x2 + _f32("0x1.111112p-7")
    ps = ps * x2 - _f32("0x1.555556p-3")
    sn = x + x * (x2 * ps)
    pc = np.full(x.shape, _f32("-0x1.27e4fcp-22"), np.float32)
    pc = pc * x2 + _f32("0x1.a01a02p-16")
    pc = pc * x2 - _f32("0x1.6c16c2p-10")
    pc = pc * x2 + _f32("0x1.555556p-5")
    pc = pc * x2 - half
    cs = one + x2 * pc
    swap = (((octant + np.uint32(1)) >> np.uint32(1)) & np.uint32(1)) != 0
    c = np.where(swap, sn, cs)
    s = np.where(swap, cs, sn)
    c = np.where((((octant + np.uint32(2)) >> np.uint32(2)) & np.uint32(1)) != 0, -c, c)
    s = np.where((octant >> np.uint32(2)) != 0, -s, s)
    return c, s


def sampler_noise(seed: int, ids=None, B: Optional[int] = None, L: int = 256, first_row: int = 0):
    """Host twin of msr_sampler_noise, bit for bit: the [B, L] float32 noise of rows whose ids are ``ids`` [B, 3] (any integer
    type; values are taken modulo 2^32, so -1 is 0xFFFFFFFF) or, without ids, (first_row + b, 0, 0) for b < B."""
    import numpy as np
    if L < 4 or L % 4:
        raise ValueError(f"L must be a positive multiple of 4, got {L}")
    if ids is None:
        if B is None:
            raise ValueError("sampler_noise needs ids or B")
        rows = (np.arange(B, dtype=np.uint64) + np.uint64(int(first_row) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
        ids = np.stack([rows, np.zeros_like(rows), np.zeros_like(rows)], axis=1)
    ids = (np.asarray(ids).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    if ids.ndim != 2 or ids.shape[1] != 3 or (B is not None and ids.shape[0] != B):
        raise ValueError(f"ids must be [B, 3], got {ids.shape}")
    B, G = ids.shape[0], L // 4
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    counter = np.empty((B, G, 4), np.uint32)
    counter[..., 0] = np.arange(G, dtype=np.uint32)[None, :]
    counter[..., 1:] = ids[:, None, :]
    w = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))
    c0, s0 = _sampler_cos_sin(w[..., 1])
    c1, s1 = _sampler_cos_sin(w[..., 3])
    r0, r1 = _sampler_radius(w[..., 0]), _sampler_radius(w[..., 2])
    return np.stack([r0 * c0, r0 * s0, r1 * c1, r1 * s1], axis=-1).reshape(B, L).astype(np.float32)


def sampler_noise_device(ctx: OpContext, seed: int, B: int, L: int, ids: Optional[torch.Tensor] = None, first_row: int = 0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch of msr_sampler_noise on the current stream: ``ids`` int32 / uint32 [B, 3] on the device or None (then rows
    first_row + b); fills and returns ``out`` (the first B * L floats of it) or a new [B, L] tensor."""
    if out is None:
        out = torch.empty((B, L), dtype=torch.float32, device=ctx.device)
    rc = ctx.lib.msr_sampler_noise(ctx.h, int(seed), None if ids is None else ids.contiguous().data_ptr(), int(first_row),
                                   out.data_ptr(), B, L, torch.cuda.current_stream(ctx.device).cuda_stream)
    _lib.raise_for(ctx.lib, ctx.h, rc, "msr_sampler_noise")
    return out

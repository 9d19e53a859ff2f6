// The finishing pass of the split-K conv launches, and the fp64 combine of the fused epilogues' moment slabs.
#include "conv_common.h"

namespace msr {

// ------------------------------------------------------------------------------------------------------
// splitk_epilogue: sums the ksplit partial accumulators in a fixed order (deterministic) and applies the same
// epilogue the fused kernel would have applied.  One thread per (pixel, 4 channels).
// ------------------------------------------------------------------------------------------------------
template <int EPI>
__global__ void __launch_bounds__(256) splitk_epilogue_kernel(const ConvParams p) {
    MSR_SATURATING_CONVERSIONS();
    const int Cout = EPI == EPI_SPADE ? p.N / 2 : p.N;
    const int quads = Cout / 4;
    const long M = (long)p.B * p.Hout * p.Wout;
    const long total = M * quads;
    const size_t pstride = (size_t)M * p.N;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int q = (int)(i % quads);
        const long pix = i / quads;
        const int x = (int)(pix % p.Wout);
        const int y = (int)((pix / p.Wout) % p.Hout);
        const int b = (int)(pix / ((long)p.Wout * p.Hout));
        const int c = q * 4;
        const int col = EPI == EPI_SPADE ? (c / 32) * 64 + (c % 32) : c;
        const float* pp = p.partial + (size_t)pix * p.N + col;
        float4 a = *reinterpret_cast<const float4*>(pp);
        float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (EPI == EPI_SPADE) bsum = *reinterpret_cast<const float4*>(pp + 32);
#pragma unroll 8      // the K ranges' loads in flight together, the additions in range order
        for (int k = 1; k < p.ksplit; ++k) {
            const float4 t = *reinterpret_cast<const float4*>(pp + k * pstride);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
            if constexpr (EPI == EPI_SPADE) {
                const float4 u = *reinterpret_cast<const float4*>(pp + k * pstride + 32);
                bsum.x += u.x; bsum.y += u.y; bsum.z += u.z; bsum.w += u.w;
            }
        }
        const float4 b0v = *reinterpret_cast<const float4*>(p.bias + col);
        float4 v = make_float4(a.x + b0v.x, a.y + b0v.y, a.z + b0v.z, a.w + b0v.w);
        if constexpr (EPI == EPI_AFFINE) {
            float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
            if (p.scale) sc = *reinterpret_cast<const float4*>(p.scale + col);
            v = make_float4(a.x * sc.x + b0v.x, a.y * sc.y + b0v.y, a.z * sc.z + b0v.z, a.w * sc.w + b0v.w);
            if (p.act == 1) {
                v.x = v.x <= 0.f ? 0.f : v.x; v.y = v.y <= 0.f ? 0.f : v.y; v.z = v.z <= 0.f ? 0.f : v.z; v.w = v.w <= 0.f ? 0.f : v.w;   // keeps NaN (fmaxf drops it)
            } else if (p.act == 2) {
                v.x = v.x >= 0.f ? v.x : v.x * p.slope; v.y = v.y >= 0.f ? v.y : v.y * p.slope;
                v.z = v.z >= 0.f ? v.z : v.z * p.slope; v.w = v.w >= 0.f ? v.w : v.w * p.slope;
            }
        }
        if constexpr (EPI == EPI_RES || EPI == EPI_SPADE) {
            const float4 xv = *reinterpret_cast<const float4*>(p.aux + (size_t)b * p.aux_pb +
                                                               (size_t)(y >> p.aux_shift) * p.aux_py +
                                                               (size_t)(x >> p.aux_shift) * p.aux_px + c);
            if constexpr (EPI == EPI_RES) {
                v.x += xv.x; v.y += xv.y; v.z += xv.z; v.w += xv.w;
            } else {
                const float4 b1v = *reinterpret_cast<const float4*>(p.bias + col + 32);
                const float4 mu = *reinterpret_cast<const float4*>(p.mean + c);
                const float4 sd = *reinterpret_cast<const float4*>(p.stdv + c);
                v.x = v.x * ((xv.x - mu.x) / sd.x) + (bsum.x + b1v.x);
                v.y = v.y * ((xv.y - mu.y) / sd.y) + (bsum.y + b1v.y);
                v.z = v.z * ((xv.z - mu.z) / sd.z) + (bsum.z + b1v.z);
                v.w = v.w * ((xv.w - mu.w) / sd.w) + (bsum.w + b1v.w);
                v.x = v.x >= 0.f ? v.x : v.x * p.slope; v.y = v.y >= 0.f ? v.y : v.y * p.slope;
                v.z = v.z >= 0.f ? v.z : v.z * p.slope; v.w = v.w >= 0.f ? v.w : v.w * p.slope;
            }
        }
        float* opix = p.out + (size_t)p.out_off + (size_t)b * p.out_pb + (size_t)y * p.out_py + (size_t)x * p.out_px;
        if (EPI == EPI_SPADE && p.out_split == OUT_F16C) msr_store_f16c4_dev(opix, c, v.x, v.y, v.z, v.w);
        else if (EPI == EPI_SPADE && p.out_split) msr_store_split4_dev(opix, c, v.x, v.y, v.z, v.w);
        else *reinterpret_cast<float4*>(opix + c) = v;
    }
}

// The finishing pass of every split-K launch: sums the K ranges of p.partial and applies epilogue `epi` (bias, residual,
// SPADE or affine), with the output's moments in the same launch when the plan asked for them (p.mom_mean).
hipError_t finish_splitk(const ConvParams& p, int epi, hipStream_t s) {
    if (p.mom_mean) return launch_splitk_epilogue_mom(p, epi, s);      // epilogue + the output's moments, one launch
    const int Cout = epi == EPI_SPADE ? p.N / 2 : p.N;
    long eb = ((long)p.B * p.Hout * p.Wout * (Cout / 4) + 255) / 256;
    if (eb > 4096) eb = 4096;
    switch (epi) {
        case EPI_BIAS: splitk_epilogue_kernel<EPI_BIAS><<<(int)eb, 256, 0, s>>>(p); break;
        case EPI_RES: splitk_epilogue_kernel<EPI_RES><<<(int)eb, 256, 0, s>>>(p); break;
        case EPI_SPADE: splitk_epilogue_kernel<EPI_SPADE><<<(int)eb, 256, 0, s>>>(p); break;
        case EPI_AFFINE: splitk_epilogue_kernel<EPI_AFFINE><<<(int)eb, 256, 0, s>>>(p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// Stage 1: grid (C/32, groups): 32 slab slots x 32 channels per workgroup, sequential Chan per slot over the
// group's slab range, fixed-order combine of the 32 slots -> one (count, mean, M2) triple per (group, channel).
// Stage 2: the same kernel over the stage-1 triples with one group and final = 1.  fp64, deterministic order.
template <typename T>
__global__ void __launch_bounds__(1024) moments_from_slabs_kernel(const T* __restrict__ partial, int P, int C,
                                                                  int final_stage, float eps,
                                                                  double* __restrict__ group_out,
                                                                  float* __restrict__ mean, float* __restrict__ stdv) {
    __shared__ double red[32][32][3];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const int slot = threadIdx.x >> 5;
    const int groups = gridDim.y, grp = blockIdx.y;
    const int per = (P + groups - 1) / groups;
    const int k0 = grp * per, k1 = min(P, k0 + per);
    double n = 0, mu = 0, m2 = 0;
    for (int k = k0 + slot; k < k1; k += 32) {
        const T* o = partial + (size_t)k * 3 * C + c;
        const double bn = (double)o[0], bmu = (double)o[C], bm2 = (double)o[2 * C];
        if (bn > 0) {
            const double tot = n + bn, delta = bmu - mu;
            m2 += bm2 + delta * delta * (n * bn / tot);
            mu += delta * (bn / tot);
            n = tot;
        }
    }
    red[slot][threadIdx.x & 31][0] = n; red[slot][threadIdx.x & 31][1] = mu; red[slot][threadIdx.x & 31][2] = m2;
    __syncthreads();
    if (slot == 0) {
        for (int k = 1; k < 32; ++k) {
            const double bn = red[k][threadIdx.x][0], bmu = red[k][threadIdx.x][1], bm2 = red[k][threadIdx.x][2];
            if (bn > 0) {
                const double tot = n + bn, delta = bmu - mu;
                m2 += bm2 + delta * delta * (n * bn / tot);
                mu += delta * (bn / tot);
                n = tot;
            }
        }
        if (final_stage) {
            const double var = n > 0 ? m2 / n : 0.0;
            mean[c] = (float)mu;
            stdv[c] = sqrtf((float)var + eps);
        } else {
            double* o = group_out + (size_t)grp * 3 * C + c;
            o[0] = n; o[C] = mu; o[2 * C] = m2;
        }
    }
}

hipError_t launch_moments_from_slabs(const float* partial, int P, int C, float eps, double* group_ws, float* mean,
                                     float* stdv, hipStream_t s) {
    if (C % 32 || P <= 0) return hipErrorInvalidValue;
    int groups = P < 512 ? 1 : P / 64;       // up to a few hundred slabs one launch is faster than two (5-8 us each); 512 slabs in
                                             // one launch were 16 sequential fp64 Chan updates per thread: 18 us
    if (groups > 128) groups = 128;          // 512 workgroups at C = 128 (32 groups = 128 workgroups pulled 12.6 MB of slabs in 17 us)
    if (groups <= 1) {
        moments_from_slabs_kernel<float><<<dim3(C / 32, 1), 1024, 0, s>>>(partial, P, C, 1, eps, nullptr, mean, stdv);
    } else {
        moments_from_slabs_kernel<float><<<dim3(C / 32, groups), 1024, 0, s>>>(partial, P, C, 0, eps, group_ws, mean, stdv);
        moments_from_slabs_kernel<double><<<dim3(C / 32, 1), 1024, 0, s>>>(group_ws, groups, C, 1, eps, nullptr, mean, stdv);
    }
    return hipGetLastError();
}

}  // namespace msr

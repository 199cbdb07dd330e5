// 'choice' decode on the device: Dense(H -> N) + tempered softmax + inverse-CDF draw per (t, b) row of a softmax head.
// Replaces sample_vector(v, 'choice') of the decode path (reference vae_definition.py:1048-1067: p / sum(p), log(p) / temperature,
// softmax of that, np.random.choice, number_of_tries / cutoff_sample_threshold) for rows that never leave the device.
//
// The logits are computed exactly as head_k does (heads.hip): one wave = 16 rows, A = rows of h, B = W^T (the head's own packed
// copy), f32 accumulation on the matrix cores; a row's columns sit across the 16 lanes of a lane group, column n*16 + r in tile n.
// softmax(log(softmax(lg)) / tau) = softmax(lg / tau), so e_j = exp2((lg_j - max) * log2e / tau) comes straight from the logits and
// p is never formed.  np.random.choice's rule - cdf = cumsum(q); cdf /= cdf[-1]; searchsorted(cdf, u, side='right') - is
// idx = #{j < N : cdf_j <= u * S} with cdf the inclusive prefix sum of e in column order and S its last element: a 16-lane scan
// per tile (DPP row shifts), the tile totals carried forward, a count per lane and one 16-lane sum.  Pad columns add 0; a
// zero-probability column repeats the cdf of its predecessor and can never be drawn.
//
// Forward only: writes one uint8 per row and nothing else (no loss scalars, no probabilities).
#include "common.h"

namespace {

constexpr int MAX_TRIES = 4;
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;
constexpr int DPP_ROW_BCAST15 = 0x15F;          // every lane of a 16-lane row reads the row's lane 15

// inclusive prefix sum over the 16 lanes of a DPP row (lanes shifted in from outside the row read 0)
__device__ __forceinline__ float group16_scan(float v) {
    v += dpp_f<DPP_ROW_SHR1>(v);
    v += dpp_f<DPP_ROW_SHR2>(v);
    v += dpp_f<DPP_ROW_SHR4>(v);
    v += dpp_f<DPP_ROW_SHR8>(v);
    return v;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// row tiles per wave and pass: as head_k (the weight fragments are shared by both row tiles)
template <typename WT, int NTL>
__host__ __device__ constexpr int sample_rb() { return (sizeof(WT) == 2 && NTL <= 4) ? 2 : 1; }

template <typename WT, int NTL>
__global__ __launch_bounds__(256) void head_sample_k(const mvae_head_sample_args a) {
    constexpr int KG = op<WT>::KG, FE = op<WT>::FRAG_ELEMS;
    typedef typename op<WT>::frag frag;
    constexpr int RB = sample_rb<WT, NTL>();
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, q = l >> 4, r = l & 15;
    const int R = a.R, H = a.H, N = a.N;
    const WT* __restrict__ hs = reinterpret_cast<const WT*>(a.hs);
    const WT* __restrict__ wt = reinterpret_cast<const WT*>(a.wt);
    // the per-call values: from the device-resident control block when there is one (a recorded launch is then replayable
    // whatever the seed), else from the argument struct
    const mvae_sample_ctl c = a.ctl ? *a.ctl : a.host;
    int tries = c.tries < 1 ? 1 : (c.tries > MAX_TRIES ? MAX_TRIES : c.tries);
    if (a.uniforms && tries > a.u_stride) tries = a.u_stride;
    const float kscale = 1.4426950408889634f / c.temperature;
    const float cutoff = c.cutoff;
    const long long window0 = (long long)(((unsigned long long)c.window0_hi << 32) | c.window0_lo);
    float bias[NTL];
#pragma unroll
    for (int n = 0; n < NTL; ++n) bias[n] = (n * 16 + r < N) ? a.bias[n * 16 + r] : 0.0f;

    for (int row00 = (blockIdx.x * 4 + w) * 16 * RB; row00 < R; row00 += gridDim.x * 64 * RB) {
        f32x4 acc_[RB][NTL];
#pragma unroll
        for (int b = 0; b < RB; ++b)
#pragma unroll
            for (int n = 0; n < NTL; ++n) acc_[b][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < H / KG; ++s) {
            frag fa[RB];
#pragma unroll
            for (int b = 0; b < RB; ++b)
                fa[b] = *reinterpret_cast<const frag*>(hs + (size_t)min(row00 + b * 16 + r, R - 1) * H + s * KG + q * FE);
#pragma unroll
            for (int n = 0; n < NTL; ++n) {
                const frag fb = *reinterpret_cast<const frag*>(wt + (size_t)(n * 16 + r) * H + s * KG + q * FE);
#pragma unroll
                for (int b = 0; b < RB; ++b) acc_[b][n] = op<WT>::mma(fa[b], fb, acc_[b][n]);     // C[row = q*4+i][col = n*16 + r]
            }
        }
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const f32x4 (&acc)[NTL] = acc_[b];
            const int rowq = row00 + b * 16 + q * 4;          // first of this lane group's 4 rows
            // position of that row in the caller's order: device rows are (t, b) time-major with b_stride windows a step
            long long g = (long long)a.row0 + rowq;
            long long tt = 0, bb = g;
            if (a.b_stride > 0) {
                tt = g / a.b_stride;
                bb = g % a.b_stride;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rowq + i;
                const bool rv = row < R;
                const int rc = rv ? row : R - 1;
                float e[NTL], mx = -INFINITY;
#pragma unroll
                for (int n = 0; n < NTL; ++n) {
                    e[n] = (n * 16 + r < N) ? acc[n][i] + bias[n] : -INFINITY;
                    mx = fmaxf(mx, e[n]);
                }
                mx = group16_max(mx);
                float cdf[NTL], carry = 0.0f;
#pragma unroll
                for (int n = 0; n < NTL; ++n) {
                    e[n] = (n * 16 + r < N) ? __builtin_amdgcn_exp2f((e[n] - mx) * kscale) : 0.0f;     // v_exp_f32 (rel. error ~1e-6)
                    cdf[n] = carry + group16_scan(e[n]);
                    carry = dpp_f<DPP_ROW_BCAST15>(cdf[n]);
                }
                const float S = carry;
                uint32_t words[4] = {0u, 0u, 0u, 0u};
                if (!a.uniforms) {
                    const unsigned long long grow = (unsigned long long)(a.b_stride > 0 ? (window0 + bb) * a.T + tt : window0 * a.T + bb);
                    philox4x32_10((uint32_t)grow, (uint32_t)(grow >> 32), (uint32_t)a.head_id, 0u, c.seed_lo, c.seed_hi, words);
                }
                int idx = 0;
                bool done = false;
#pragma unroll
                for (int t = 0; t < MAX_TRIES; ++t) {
                    if (t < tries) {
                        const float u = a.uniforms ? a.uniforms[(size_t)rc * a.u_stride + t] : (float)(words[t] >> 8) * 0x1p-24f;
                        const float thr = u * S;
                        float cnt = 0.0f;
#pragma unroll
                        for (int n = 0; n < NTL; ++n) cnt += (n * 16 + r < N && cdf[n] <= thr) ? 1.0f : 0.0f;
                        const int k = min((int)group16_sum(cnt), N - 1);          // (<= 192 ones: exact in f32)
                        if (!done) idx = k;
                        if (tries > 1) {
                            float ek = 0.0f;
#pragma unroll
                            for (int n = 0; n < NTL; ++n) ek += (n * 16 + r == k) ? e[n] : 0.0f;
                            ek = group16_sum(ek);
                            done = done || ek > cutoff * S;
                        }
                    }
                }
                if (rv && r == 0) a.out[row] = (uint8_t)idx;
                // the next row of the lane group
                if (a.b_stride > 0) {
                    if (++bb == a.b_stride) {
                        bb = 0;
                        ++tt;
                    }
                } else {
                    ++bb;
                }
            }
        }
    }
}

template <typename WT>
int launch(const mvae_head_sample_args& a, hipStream_t s) {
    const int ntl = (a.N + 15) / 16;
    const dim3 block(256);
    auto grid = [&](int rb) {
        const int need = (a.R + 64 * rb - 1) / (64 * rb);
        const int cap = rb == 2 ? 512 : 1024;
        return dim3(need < cap ? need : cap);
    };
    // the tile counts of mvae_head_np: wt has that many rows
    switch (ntl) {
        case 1: hipLaunchKernelGGL((head_sample_k<WT, 1>), grid(sample_rb<WT, 1>()), block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((head_sample_k<WT, 2>), grid(sample_rb<WT, 2>()), block, 0, s, a); break;
        case 3:
        case 4: hipLaunchKernelGGL((head_sample_k<WT, 4>), grid(sample_rb<WT, 4>()), block, 0, s, a); break;
        case 5: case 6: case 7:
        case 8: hipLaunchKernelGGL((head_sample_k<WT, 8>), grid(1), block, 0, s, a); break;
        case 9: hipLaunchKernelGGL((head_sample_k<WT, 9>), grid(1), block, 0, s, a); break;
        case 10: hipLaunchKernelGGL((head_sample_k<WT, 10>), grid(1), block, 0, s, a); break;
        case 11: hipLaunchKernelGGL((head_sample_k<WT, 11>), grid(1), block, 0, s, a); break;
        case 12: hipLaunchKernelGGL((head_sample_k<WT, 12>), grid(1), block, 0, s, a); break;
        default: return MVAE_E_UNSUPPORTED;
    }
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

}  // namespace

extern "C" int mvae_head_sample(const mvae_head_sample_args* a, void* stream) {
    if (!a || !a->hs || !a->wt || !a->bias || !a->out || a->R <= 0 || a->N <= 0 || a->H <= 0) return MVAE_E_ARG;
    if (a->row0 < 0 || a->T < 0 || a->b_stride < 0 || (a->b_stride > 0 && a->T <= 0)) return MVAE_E_ARG;
    if (a->uniforms && (a->u_stride < 1 || a->u_stride > MAX_TRIES)) return MVAE_E_ARG;
    if (!a->ctl) {          // (a device-resident control block is the caller's to validate)
        if (!(a->host.temperature > 0.0f) || a->host.tries < 1 || !(a->host.cutoff >= 0.0f)) return MVAE_E_ARG;
        if (a->host.tries > MAX_TRIES) return MVAE_E_UNSUPPORTED;
        if (a->uniforms && a->u_stride < a->host.tries) return MVAE_E_ARG;
    }
    if (a->N > 192) return MVAE_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (a->dtype == MVAE_F32) {
        if (a->H % 16) return MVAE_E_UNSUPPORTED;
        return launch<float>(*a, s);
    }
    if (a->dtype == MVAE_BF16) {
        if (a->H % 32) return MVAE_E_UNSUPPORTED;
        return launch<bf16_t>(*a, s);
    }
    return MVAE_E_ARG;
}

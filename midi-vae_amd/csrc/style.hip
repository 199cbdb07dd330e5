// Style-transfer scoring on the device: the pitch, velocity and instrument style judges and their weighted ensemble per window,
// accuracy and confidence per group of windows, and the confusion counts (reference vae_evaluation.py:110-117 and the per-song
// counters of :2096-2172, :2471-2604), from the probability tables the classifiers leave in HBM.  C ABI: include/midivae_style.h.
//
// Mapping: ONE WORKGROUP OF 256 LANES PER GROUP.  Lane l walks the windows first + l, first + l + 256, .. of its group in ascending
// order; a window is one loop over its C <= 64 columns that reads the three probabilities of a column, forms the ensemble's value
// and carries the four running argmaxes and the four probabilities of the window's class in registers - nothing a lane indexes
// dynamically.  The confidences are summed in double per lane and reduced by the fixed tree the header states; the hits and the
// count are integers.  Up to CONF_LDS_C classes the confusion counts of a group are gathered in LDS and flushed once; above that
// they go to memory directly.  A group longer than 256 windows loops; no workgroup waits for another.
#include "common.h"

#include "../../include/midivae_style.h"

namespace {

constexpr int LANES = MVAE_STYLE_LANES, JUDGES = MVAE_STYLE_JUDGES, MAXC = MVAE_STYLE_MAX_CLASSES;
constexpr int CONF_LDS_C = 16;          // 4 x 16 x 16 counters = 4 KiB of LDS
constexpr int NONE = 255;

// np.argmax one element at a time: a later element wins only if it is larger or the first NaN
struct ArgMax {
    float v;
    int at;
    __device__ __forceinline__ void first(float x) {
        v = x;
        at = 0;
    }
    __device__ __forceinline__ void next(float x, int c) {
        if (!(v != v) && (x > v || x != x)) {
            v = x;
            at = c;
        }
    }
};

// the reference's expression on float32 arrays: every product, sum and the division rounded on its own
__device__ __forceinline__ float ensemble_value(float p, float i, float v, float wp, float wi, float wv, float den) {
#pragma clang fp contract(off)
    const float a = p * wp;
    const float b = i * wi;
    const float ab = a + b;
    const float c = v * wv;
    const float s = ab + c;
    return s / den;
}

__global__ __launch_bounds__(LANES) void style_scores_k(const mvae_style_args a) {
    __shared__ double sum[JUDGES][LANES];
    __shared__ int hit[JUDGES][LANES];
    __shared__ int cnt[LANES];
    __shared__ int conf[JUDGES * CONF_LDS_C * CONF_LDS_C];
    const int l = threadIdx.x, g = blockIdx.x, C = a.C, n = a.n;
    const bool ens = a.p_pitch && a.p_vel && a.p_instr;
    const bool conf_lds = a.confusion_out && C <= CONF_LDS_C;
    const float wp = (float)a.weights[0], wi = (float)a.weights[1], wv = (float)a.weights[2];
    const float den = (float)(a.weights[0] + a.weights[1] + a.weights[2]);
    const float nan32 = __builtin_nanf("");

    int first = a.group_off[g], last = a.group_off[g + 1];
    first = min(max(first, 0), n);
    last = min(max(last, 0), n);

    if (conf_lds) {
        for (int i = l; i < JUDGES * C * C; i += LANES) conf[i] = 0;
        __syncthreads();
    }

    double s_p = 0.0, s_v = 0.0, s_i = 0.0, s_e = 0.0;
    int h_p = 0, h_v = 0, h_i = 0, h_e = 0, counted = 0;
    for (int w = first + l; w < last; w += LANES) {
        const int k = a.cls[w];
        const bool count = k < C;          // 255 and every other class that does not exist
        int r = a.instr_row ? a.instr_row[w] : w;
        const bool have_i = a.p_instr && r >= 0 && r < a.n_instr_rows;
        const float* pp = a.p_pitch ? a.p_pitch + (size_t)w * a.ld_pitch : nullptr;
        const float* pv = a.p_vel ? a.p_vel + (size_t)w * a.ld_vel : nullptr;
        const float* pi = have_i ? a.p_instr + (size_t)r * a.ld_instr : nullptr;
        float* eo = a.ens_out ? a.ens_out + (size_t)w * a.ld_ens : nullptr;
        const bool have_e = ens && have_i;
        ArgMax m_p, m_v, m_i, m_e;
        m_p.first(0.0f), m_v.first(0.0f), m_i.first(0.0f), m_e.first(0.0f);
        float c_p = nan32, c_v = nan32, c_i = nan32, c_e = nan32;          // the probabilities of class k
        for (int c = 0; c < C; ++c) {
            const float x_p = pp ? pp[c] : 0.0f, x_v = pv ? pv[c] : 0.0f, x_i = pi ? pi[c] : 0.0f;
            const float x_e = have_e ? ensemble_value(x_p, x_i, x_v, wp, wi, wv, den) : nan32;
            if (c == 0) {
                m_p.first(x_p), m_v.first(x_v), m_i.first(x_i), m_e.first(x_e);
            } else {
                m_p.next(x_p, c), m_v.next(x_v, c), m_i.next(x_i, c), m_e.next(x_e, c);
            }
            if (c == k) c_p = x_p, c_v = x_v, c_i = x_i, c_e = x_e;
            if (eo) eo[c] = x_e;
        }
        const int a_p = pp ? m_p.at : NONE, a_v = pv ? m_v.at : NONE, a_i = pi ? m_i.at : NONE, a_e = have_e ? m_e.at : NONE;
        if (a.pred_out) {
            uint8_t* po = a.pred_out + (size_t)w * JUDGES;
            po[0] = (uint8_t)a_p, po[1] = (uint8_t)a_v, po[2] = (uint8_t)a_i, po[3] = (uint8_t)a_e;
        }
        if (!count) continue;
        ++counted;
        s_p += (double)c_p, s_v += (double)c_v, s_i += (double)(pi ? c_i : nan32), s_e += (double)(have_e ? c_e : nan32);
        h_p += a_p == k, h_v += a_v == k, h_i += a_i == k, h_e += a_e == k;
        if (a.confusion_out) {
            const int am[JUDGES] = {a_p, a_v, a_i, a_e};          // (unrolled: registers)
#pragma unroll
            for (int j = 0; j < JUDGES; ++j) {
                if (am[j] == NONE) continue;
                const int at = (j * C + k) * C + am[j];
                if (conf_lds)
                    atomicAdd(&conf[at], 1);
                else
                    atomicAdd(&a.confusion_out[at], 1);
            }
        }
    }

    if (conf_lds) {
        __syncthreads();
        for (int i = l; i < JUDGES * C * C; i += LANES)
            if (conf[i]) atomicAdd(&a.confusion_out[i], conf[i]);
    }
    if (!a.table_out) return;

    sum[0][l] = s_p, sum[1][l] = s_v, sum[2][l] = s_i, sum[3][l] = s_e;
    hit[0][l] = h_p, hit[1][l] = h_v, hit[2][l] = h_i, hit[3][l] = h_e;
    cnt[l] = counted;
    __syncthreads();
    for (int s = LANES / 2; s > 0; s >>= 1) {
        if (l < s) {
#pragma unroll
            for (int j = 0; j < JUDGES; ++j) {
                sum[j][l] += sum[j][l + s];
                hit[j][l] += hit[j][l + s];
            }
            cnt[l] += cnt[l + s];
        }
        __syncthreads();
    }
    if (l < MVAE_STYLE_COLUMNS) {
        const unsigned have = (a.p_pitch ? 1u : 0u) | (a.p_vel ? 2u : 0u) | (a.p_instr ? 4u : 0u) | (ens ? 8u : 0u);
        const int total = cnt[0];
        double out = (double)total;
        if (l > 0) {
            const int j = (l - 1) >> 1;
            if (total == 0 || !((have >> j) & 1u))
                out = __builtin_nan("");
            else
                out = ((l & 1) ? (double)hit[j][0] : sum[j][0]) / (double)total;
        }
        a.table_out[(size_t)g * a.ld_table + l] = out;
    }
}

bool is_finite(double x) { return x == x && x - x == 0.0; }

}  // namespace

extern "C" int mvae_style_abi_version(void) { return 1; }

extern "C" int mvae_style_scores(const mvae_style_args* a, void* stream) {
    if (!a) return MVAE_E_ARG;
    if (!a->p_pitch && !a->p_vel && !a->p_instr) return MVAE_E_ARG;
    if (!a->ens_out && !a->pred_out && !a->table_out && !a->confusion_out) return MVAE_E_ARG;
    if (a->ens_out && !(a->p_pitch && a->p_vel && a->p_instr)) return MVAE_E_ARG;
    if (a->n <= 0 || a->n_groups <= 0 || !a->cls || !a->group_off) return MVAE_E_ARG;
    for (int i = 0; i < 3; ++i)
        if (!is_finite(a->weights[i])) return MVAE_E_ARG;
    const double wsum = a->weights[0] + a->weights[1] + a->weights[2];
    if (!is_finite(wsum) || !(wsum > 0.0)) return MVAE_E_ARG;
    if (a->C < MVAE_STYLE_MIN_CLASSES || a->C > MAXC) return MVAE_E_UNSUPPORTED;
    if ((a->p_pitch && a->ld_pitch < a->C) || (a->p_vel && a->ld_vel < a->C) || (a->p_instr && a->ld_instr < a->C)) return MVAE_E_ARG;
    if (a->ens_out && a->ld_ens < a->C) return MVAE_E_ARG;
    if (a->table_out && a->ld_table < MVAE_STYLE_COLUMNS) return MVAE_E_ARG;
    if (a->p_instr && a->n_instr_rows <= 0) return MVAE_E_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(style_scores_k, dim3(a->n_groups), dim3(LANES), 0, s, *a);
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

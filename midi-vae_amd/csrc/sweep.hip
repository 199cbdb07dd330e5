// Latent-sweep statistics on the device: the velocity post-rules of a decoded window (reference vae_definition.py:1153-1190) and
// the pitch / velocity / note-start statistics the sweep ranks latent dimensions by (vae_evaluation.py:1018-1096), from the index
// and the float velocity per row that a decode leaves in HBM.  C ABI: include/midivae_sweep.h.
//
// Mapping as in descriptors.hip: ONE LANE PER WINDOW, one wave per workgroup, loops over the ticks (any T up to MAX_T).  What a lane
// indexes dynamically - the tick's note set, the voices' previous pitch and velocity, a pitch histogram, the radix bins of the
// velocity selection - lives in LDS laid out [slot][lane]; nothing lands in scratch (the Makefile checks it).
//
// Reading the rows: Rows of rolls.h in chunks of CHUNK_TICKS ticks, indices and velocities side by side.
//
// A window is walked several times; every walk re-runs the rule automaton, so nothing of size T is kept per lane:
//   walk 1   pitch list (exact integer sums, a histogram for the median and the two counted columns), velocities after the rules
//            (vel_out), count / sum / min / max of the note starts and the integer sums of their positions;
//   walk 2   squared deviations from the mean (two-pass std), the position median (the positions ascend: a counting walk meets the
//            middle one or two), and the first digit of the velocity selection;
//   walks 3..8  the other digits.  The velocity median is an exact selection on the floats' bit patterns, mapped to keys whose
//            unsigned order is the floats' order: 5 bits a walk from the top, counting the keys that share the prefix found so far;
//   walk 9   only where a lane's count is even and its two middle elements differ: the smallest key above the lower one.
// Walks 3..9 are skipped by a workgroup none of whose lanes needs them.
#include "rolls.h"

#include "../../include/midivae_sweep.h"

namespace {

constexpr int MAXV = MVAE_SWEEP_MAX_VOICES, MAXP = MVAE_SWEEP_MAX_PITCH;
constexpr int CHUNK_TICKS = 8;
constexpr int MAX_T = MVAE_SWEEP_MAX_T;    // ticks <= 2^15 fit the 16-bit histogram; c * sum(t^2) < 2^16 * 2^48 / 3 stays inside int64
constexpr int DIGIT_BITS = 5, DIGITS = 1 << DIGIT_BITS;
static_assert(MAXV == ROLL_MAX_VOICES, "rolls.h sizes its tiles for the headers' voice limit");

template <bool STAGED>
using SweepRows = Rows<mvae_sweep_args, STAGED, true, CHUNK_TICKS>;          // index and velocity side by side

// the floats' order as the unsigned order of 32-bit keys, and back
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

struct Lds {
    int (*cur)[LANES];
    int (*pp)[LANES];
    float (*pv)[LANES];
};

// One walk over the window of this lane: note(x) for every distinct sounding index of a tick (only with PITCH), row(t, v) for every
// row with its velocity after the rules.  Every lane of the workgroup calls it; lanes that are not live only help staging.
template <bool STAGED, bool PITCH, class NoteF, class RowF>
__device__ __forceinline__ void walk(const mvae_sweep_args& a, SweepRows<STAGED>& rows, const Lds& m, bool live, NoteF&& note, RowF&& row) {
    const int l = threadIdx.x, V = a.voices, ticks = a.T / V;
    const bool rules = a.vel != nullptr && a.override_rules != 0;
    if (rules)
        for (int v = 0; v < V; ++v) {
            m.pp[v][l] = -1;
            m.pv[v][l] = 0.0f;
        }
    for (int tick0 = 0; tick0 < ticks; tick0 += CHUNK_TICKS) {
        const int nt = min(CHUNK_TICKS, ticks - tick0);
        rows.open(tick0, nt);
        if (!live) continue;
        for (int k = 0; k < nt; ++k) {
            int nc = 0;
            for (int v = 0; v < V; ++v) {
                const int r = k * V + v;
                const int x = rows.idx(tick0, r);
                const bool snd = roll_sounding(a.silent, a.n_pitch, x);
                if (PITCH && snd) {          // the k-hot fold: a pitch doubled across voices counts once
                    bool dup = false;
                    for (int j = 0; j < nc; ++j) dup = dup || m.cur[j][l] == x;
                    if (!dup) {
                        m.cur[nc++][l] = x;
                        note(x);
                    }
                }
                double vel = a.default_velocity;
                if (a.vel) {
                    const float v0 = snd ? rows.vel(tick0, r) : 0.0f;
                    // the voice's state stays in its LDS slots; the rule's float is widened afterwards, which is exact
                    vel = (double)(rules ? velocity_rule_step(snd, x, v0, a.threshold, m.pp[v][l], m.pv[v][l]) : v0);
                }
                row((tick0 + k) * V + v, vel);
            }
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(LANES) void sweep_windows_k(const mvae_sweep_args a) {
    __shared__ int cur[MAXV][LANES], pp[MAXV][LANES];
    __shared__ float pv[MAXV][LANES];
    __shared__ uint16_t hist[MAXP][LANES];
    __shared__ uint32_t bins[DIGITS][LANES];
    __shared__ uint8_t ti[SweepRows<STAGED>::TILE];
    __shared__ float tv[SweepRows<STAGED>::TILE];
    __shared__ int more;
    const int l = threadIdx.x, T = a.T;
    const int w = blockIdx.x * LANES + l;
    const bool live = w < a.n;
    const double thr = a.threshold;
    SweepRows<STAGED> rows(a, ti, tv);
    const Lds m{cur, pp, pv};

    // ---- walk 1 ----
    for (int b = 0; b < a.n_pitch; ++b) hist[b][l] = 0;
    Stats pitches, starts;
    double vsum = 0.0, vmin = 0.0, vmax = 0.0;
    float* vel_out = a.vel_out && live ? a.vel_out + (size_t)w * T : nullptr;
    walk<STAGED, true>(
        a, rows, m, live,
        [&](int x) {
            pitches.push(x);
            ++hist[x][l];
        },
        [&](int t, double v) {
            if (vel_out) vel_out[t] = (float)v;
            if (v > thr) {
                if (starts.c == 0) vmin = vmax = v;
                vmin = v < vmin ? v : vmin;
                vmax = v > vmax ? v : vmax;
                vsum += v;
                starts.push(t);
            }
        });
    if (!a.stats_out) return;
    double* out = a.stats_out + (size_t)(live ? w : 0) * a.ld_out;
    const long long c = live ? starts.c : 0;
    const double vmean = c ? vsum / (double)c : 0.0;
    if (live) {
        double median = 0.0;
        if (pitches.c) {
            const long long r_lo = (pitches.c - 1) / 2, r_hi = pitches.c / 2;
            long long cum = 0;
            int m_lo = -1, m_hi = -1;
            for (int b = pitches.lo; b <= pitches.hi; ++b) {
                cum += hist[b][l];
                if (m_lo < 0 && cum > r_lo) m_lo = b;
                if (m_hi < 0 && cum > r_hi) m_hi = b;
            }
            median = (double)(m_lo + m_hi) / 2.0;
        }
        out[0] = (double)pitches.c;
        pitches.store_six(out + 1, median);
        out[7] = a.count_a < a.n_pitch ? (double)hist[a.count_a][l] : 0.0;
        out[8] = a.count_b < a.n_pitch ? (double)hist[a.count_b][l] : 0.0;
        out[9] = (double)c;
    }

    // ---- walk 2 ----
    const bool select = a.vel != nullptr && c > 0;          // (without vel every velocity is default_velocity: so is the median)
    const long long r_lo = (c - 1) / 2, r_hi = c / 2;
    uint32_t prefix = 0, known = 0;
    long long rank = r_lo, seen = 0;
    int p_lo = 0, p_hi = 0;
    double dev = 0.0;
    for (int d = 0; d < DIGITS; ++d) bins[d][l] = 0;
    auto nop = [](int) {};
    walk<STAGED, false>(a, rows, m, live, nop, [&](int t, double v) {
        if (!(v > thr)) return;
        const double e = v - vmean;
        dev += e * e;
        if (seen == r_lo) p_lo = t;
        if (seen == r_hi) p_hi = t;
        ++seen;
        if (select) ++bins[key_of((float)v) >> (32 - DIGIT_BITS)][l];
    });
    if (live) {
        starts.store_six(out + 16, (double)(p_lo + p_hi) / 2.0);
        if (c == 0) {
            for (int i = 10; i < 16; ++i) out[i] = __builtin_nan("");
        } else {
            out[10] = vmean;
            out[12] = vmin;
            out[13] = vmax;
            out[14] = vmax - vmin;
            out[15] = sqrt(dev / (double)c);
            if (!select) out[11] = a.default_velocity;
        }
    }
    // does any lane of the workgroup select?  (uniform: the walks hold barriers)
    if (l == 0) more = 0;
    __syncthreads();
    if (select) more = 1;
    __syncthreads();
    if (!more) return;

    // ---- walks 3..8: the other digits, top down ----
    long long equal = 0;          // keys that share the prefix, after the last digit: the copies of the lower median
    for (int shift = 32 - DIGIT_BITS, bits = DIGIT_BITS;;) {
        if (select) {
            long long cum = 0;
            int d = 0;
            for (; d < DIGITS - 1; ++d) {
                const long long here = bins[d][l];
                if (cum + here > rank) break;
                cum += here;
            }
            rank -= cum;
            equal = bins[d][l];
            prefix |= (uint32_t)d << shift;
            known |= ((1u << bits) - 1u) << shift;
        }
        if (shift == 0) break;
        bits = min(DIGIT_BITS, shift);          // 27, 22, .., 2, then the last two bits
        shift -= bits;
        const uint32_t mask = (1u << bits) - 1u;
        for (int d = 0; d < DIGITS; ++d) bins[d][l] = 0;
        walk<STAGED, false>(a, rows, m, live, nop, [&](int t, double v) {
            if (!select || !(v > thr)) return;
            const uint32_t k = key_of((float)v);
            if ((k & known) == prefix) ++bins[(k >> shift) & mask][l];
        });
    }
    // ---- walk 9: the upper median where it is another value ----
    const bool upper = select && r_hi != r_lo && rank + 1 >= equal;
    __syncthreads();
    if (l == 0) more = 0;
    __syncthreads();
    if (upper) more = 1;
    __syncthreads();
    uint32_t next = 0xffffffffu;
    if (more)
        walk<STAGED, false>(a, rows, m, live, nop, [&](int t, double v) {
            if (!upper || !(v > thr)) return;
            const uint32_t k = key_of((float)v);
            if (k > prefix && k < next) next = k;
        });
    if (select) out[11] = ((double)float_of(prefix) + (double)float_of(upper ? next : prefix)) / 2.0;
}

}  // namespace

extern "C" int mvae_sweep_abi_version(void) { return 1; }

extern "C" int mvae_sweep_windows(const mvae_sweep_args* a, void* stream) {
    if (roll_args_refused(a) || rule_args_refused(a) || (!a->stats_out && !a->vel_out)) return MVAE_E_ARG;
    if (a->count_a < 0 || a->count_a > 255 || a->count_b < 0 || a->count_b > 255) return MVAE_E_ARG;
    if (a->stats_out && a->ld_out < MVAE_SWEEP_COLUMNS) return MVAE_E_ARG;
    if (a->n_pitch > MAXP || a->T > MAX_T) return MVAE_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((a->n + LANES - 1) / LANES), block(LANES);
    if (a->stride_w != 1)
        hipLaunchKernelGGL(sweep_windows_k<true>, grid, block, 0, s, *a);
    else
        hipLaunchKernelGGL(sweep_windows_k<false>, grid, block, 0, s, *a);
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

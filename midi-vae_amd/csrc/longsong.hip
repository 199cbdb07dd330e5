// Long songs on the device (reference vae_evaluation.py:1821-1896): the nearest-code search and pull of one iteration for S songs in
// lockstep, and the decoded batch turned into the encoder's next input.  C ABI: include/midivae_longsong.h.
//
// walk_search_k: a workgroup takes ONE chunk of ROW_CHUNK rows of all_z and ONE group of SONG_GROUP songs.  Rows travel through an LDS
// tile [row][column] in pieces of JCH columns, fetched with adjacent lanes on adjacent columns; the codes of the group sit beside it as
// doubles.  A lane owns one row of the tile and SONGS_PER_LANE songs: it adds the squares in ascending column order into one double
// per song - the sum of a (row, song) pair is formed by one lane in one order, whatever N, S or the grid.  The four waves of a workgroup
// hold the four song pairs of the group, so the codes are LDS broadcasts.  Whether a row has been picked is looked up only for a row
// that would otherwise become the lane's best.  The workgroup leaves the minimal (d2, index) per song in the workspace; (smaller d2,
// then smaller index) is a total order, so the partial minima combine to the same winner in any order.
// walk_pull_k: one workgroup per song reduces the chunks' minima, appends the winner and pulls the code, one lane per column; each
// statement of the pull is one rounding under fp contract(off).
//
// feedback_rows_k: ONE LANE PER (WINDOW, VOICE) as recon.hip, rows through the LDS tiles of rolls.h [tick][lane]; the rule state of a
// voice is two registers and starts afresh in every window.  The time-major outputs are written with adjacent lanes on adjacent
// windows; the workgroup that holds the last window also writes the padding columns.
#include "rolls.h"

#include "../../include/midivae_longsong.h"

namespace {

// ---- nearest walk ------------------------------------------------------------------------------------------------------------------
constexpr int WB = 256;                                   // lanes of both walk kernels
constexpr int TILE_ROWS = 64, JCH = 128, TZ_LD = JCH + 1;  // the all_z tile: a row is 129 floats from the next
constexpr int ROW_CHUNK = MVAE_WALK_ROW_CHUNK, SONG_GROUP = MVAE_WALK_SONG_GROUP;
constexpr int SONGS_PER_LANE = SONG_GROUP / (WB / TILE_ROWS);
static_assert(SONGS_PER_LANE * (WB / TILE_ROWS) == SONG_GROUP && ROW_CHUNK % TILE_ROWS == 0, "a wave holds whole songs, a chunk whole tiles");
constexpr int NO_ROW = 0x7fffffff;

__host__ __device__ inline long long walk_chunks(long long N) { return (N + ROW_CHUNK - 1) / ROW_CHUNK; }

// the workspace: the chunks' minimal d2 (S, nch) doubles, d2 of row 0 (S) doubles, the chunks' indices (S, nch) int32
struct WalkSpace {
    double* d2;
    double* d0;
    int* idx;
    __device__ WalkSpace(void* ws, int S, long long nch)
        : d2(static_cast<double*>(ws)), d0(d2 + (size_t)S * nch), idx(reinterpret_cast<int*>(d0 + S)) {}
};

// (d, i) beats (bd, bi): a smaller distance, or the same at a smaller index; a NaN beats nothing
__device__ __forceinline__ bool walk_better(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

template <class F>
__global__ __launch_bounds__(WB) void walk_search_k(const mvae_walk_args a, const int groups) {
#pragma clang fp contract(off)
    __shared__ float tz[TILE_ROWS * TZ_LD];
    __shared__ double cz[SONG_GROUP * JCH];
    __shared__ double rd[SONG_GROUP * TILE_ROWS];
    __shared__ int ri[SONG_GROUP * TILE_ROWS];
    const int l = threadIdx.x, r = l & (TILE_ROWS - 1), q = l / TILE_ROWS;
    const long long nch = walk_chunks(a.N);
    const long long chunk = blockIdx.x / groups;
    const int s0 = (int)(blockIdx.x - chunk * groups) * SONG_GROUP;
    const long long row_lo = chunk * ROW_CHUNK;
    const int rows = (int)min((long long)ROW_CHUNK, (long long)a.N - row_lo);
    const F* R = static_cast<const F*>(a.r_in);
    const WalkSpace ws(a.workspace, a.S, nch);

    double bd[SONGS_PER_LANE];
    int bi[SONGS_PER_LANE];
#pragma unroll
    for (int k = 0; k < SONGS_PER_LANE; ++k) {
        bd[k] = __builtin_inf();
        bi[k] = NO_ROW;
    }
    for (int tile0 = 0; tile0 < rows; tile0 += TILE_ROWS) {
        double acc[SONGS_PER_LANE];
#pragma unroll
        for (int k = 0; k < SONGS_PER_LANE; ++k) acc[k] = 0.0;
        for (int j0 = 0; j0 < a.Z; j0 += JCH) {
            const int jn = min(JCH, a.Z - j0);
            __syncthreads();          // the previous piece has been read
            for (int i = l; i < TILE_ROWS * JCH; i += WB) {
                const int rr = i / JCH, c = i - rr * JCH;
                const long long row = row_lo + tile0 + rr;
                tz[rr * TZ_LD + c] = (row < a.N && c < jn) ? a.all_z[(size_t)row * (size_t)a.ld_all + j0 + c] : 0.0f;
            }
            if (tile0 == 0 || a.Z > JCH)          // (a code of at most JCH columns stays where the first tile put it)
                for (int i = l; i < SONG_GROUP * JCH; i += WB) {
                    const int g = i / JCH, c = i - g * JCH;
                    cz[i] = (s0 + g < a.S && c < jn) ? (double)R[(size_t)(s0 + g) * (size_t)a.ld_r + j0 + c] : 0.0;
                }
            __syncthreads();
            const float* zr = tz + r * TZ_LD;
            const double* cr = cz + q * SONGS_PER_LANE * JCH;
            for (int j = 0; j < jn; ++j) {
                const double z = (double)zr[j];
#pragma unroll
                for (int k = 0; k < SONGS_PER_LANE; ++k) {
                    const double d = z - cr[k * JCH + j];
                    const double sq = d * d;
                    acc[k] = acc[k] + sq;
                }
            }
        }
        const long long row = row_lo + tile0 + r;
        if (row < a.N) {
#pragma unroll
            for (int k = 0; k < SONGS_PER_LANE; ++k) {
                const int s = s0 + q * SONGS_PER_LANE + k;
                if (s >= a.S) continue;
                if (row == 0) ws.d0[s] = acc[k];
                if (!walk_better(acc[k], (int)row, bd[k], bi[k])) continue;
                int taken = 0;          // (no early exit: every lane makes the same n_picked comparisons; row 0 is a candidate anyway)
                const int* mine = a.picked + (size_t)s * (size_t)a.cap;
                for (int m = 0; m < a.n_picked; ++m) taken |= (int)(mine[m] == (int)row);
                if (row == 0 || !taken) {
                    bd[k] = acc[k];
                    bi[k] = (int)row;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < SONGS_PER_LANE; ++k) {
        rd[(q * SONGS_PER_LANE + k) * TILE_ROWS + r] = bd[k];
        ri[(q * SONGS_PER_LANE + k) * TILE_ROWS + r] = bi[k];
    }
    __syncthreads();
    if (l < SONG_GROUP && s0 + l < a.S) {
        double d = rd[l * TILE_ROWS];
        int i = ri[l * TILE_ROWS];
        for (int m = 1; m < TILE_ROWS; ++m)
            if (walk_better(rd[l * TILE_ROWS + m], ri[l * TILE_ROWS + m], d, i)) {
                d = rd[l * TILE_ROWS + m];
                i = ri[l * TILE_ROWS + m];
            }
        ws.d2[(size_t)(s0 + l) * nch + chunk] = d;
        ws.idx[(size_t)(s0 + l) * nch + chunk] = i;
    }
}

template <class F>
__global__ __launch_bounds__(WB) void walk_pull_k(const mvae_walk_args a) {
#pragma clang fp contract(off)
    __shared__ double sd[WB];
    __shared__ int si[WB];
    const int l = threadIdx.x, s = blockIdx.x;
    const long long nch = walk_chunks(a.N);
    const WalkSpace ws(a.workspace, a.S, nch);
    double d = __builtin_inf();
    int i = NO_ROW;
    for (long long c = l; c < nch; c += WB) {
        const double cd = ws.d2[(size_t)s * nch + c];
        const int ci = ws.idx[(size_t)s * nch + c];
        if (walk_better(cd, ci, d, i)) {
            d = cd;
            i = ci;
        }
    }
    sd[l] = d;
    si[l] = i;
    __syncthreads();
    for (int half = WB / 2; half > 0; half /= 2) {
        if (l < half && walk_better(sd[l + half], si[l + half], sd[l], si[l])) {
            sd[l] = sd[l + half];
            si[l] = si[l + half];
        }
        __syncthreads();
    }
    if (l == 0) {
        const double d0 = ws.d0[s];
        if (d0 != d0 || si[0] == NO_ROW) {          // nothing compares below a NaN: the reference's loop never leaves index 0
            sd[0] = d0;
            si[0] = 0;
        }
        a.picked[(size_t)s * (size_t)a.cap + a.n_picked] = si[0];
        a.best_out[s] = si[0];
        a.dist_out[s] = __builtin_sqrt(sd[0]);
    }
    __syncthreads();
    const float* zw = a.all_z + (size_t)si[0] * (size_t)a.ld_all;
    const F* rin = static_cast<const F*>(a.r_in) + (size_t)s * (size_t)a.ld_r;
    F* rout = static_cast<F*>(a.r_out) + (size_t)s * (size_t)a.ld_rout;
    float* zout = a.z_out + (size_t)s * (size_t)a.ld_z;
    const float ef = (float)a.e;
    const F den = (F)a.den;
    for (int j = l; j < a.Z; j += WB) {
        const F r = rin[j];
        const float p = zw[j] * ef;
        const F sum = r + (F)p;
        const F pulled = sum / den;
        zout[j] = (float)pulled;
        rout[j] = pulled;
        if (a.hist_out) {
            float h = 0.0f;
            if (a.hist_in) {
                const size_t at = (size_t)s * (size_t)a.ld_hist_in + j;
                h = a.hist_f64 ? (float)static_cast<const double*>(a.hist_in)[at] : static_cast<const float*>(a.hist_in)[at];
            }
            a.hist_out[(size_t)s * (size_t)a.ld_hist + j] = h;
        }
    }
}

// ---- feedback ----------------------------------------------------------------------------------------------------------------------
constexpr int BLOCK = VOICE_BLOCK;
static_assert(MVAE_FEEDBACK_MAX_VOICES == ROLL_MAX_VOICES, "rolls.h refuses more voices than the header's limit");
constexpr int CHUNK_TICKS = 8;

// a chunk of a tile -> rows of a time-major (T, ld) output, row t at T - 1 - t if ``reverse``; the workgroup of the last window also
// zeroes the columns n .. ld - 1 of its rows
template <class E>
__device__ __forceinline__ void unstage_tm(const Place& p, const E* tile, int n, int T, int ld, int tick0, int nt, bool reverse, E* dst) {
    const int width = (p.w0 + p.nw == n) ? ld - p.w0 : p.nw;
    const int rows = nt * p.V, total = rows * width;
    for (int i = threadIdx.x; i < total; i += BLOCK) {
        const int r = i / width, c = i - r * width;
        const int t = tick0 * p.V + r;
        const E v = c < p.nw ? tile[(r / p.V) * BLOCK + c * p.V + r % p.V] : (E)0;
        dst[(size_t)(reverse ? T - 1 - t : t) * (size_t)ld + p.w0 + c] = v;
    }
}

__global__ __launch_bounds__(BLOCK) void feedback_rows_k(const mvae_feedback_args a) {
    __shared__ uint8_t ti[CHUNK_TICKS * BLOCK], th[CHUNK_TICKS * BLOCK];
    __shared__ float tv[CHUNK_TICKS * BLOCK];
    const Place p(a);
    const int l = threadIdx.x;
    const int w = p.w0 + p.wl;
    const double thr = a.threshold;
    const bool rules = a.vel != nullptr && a.override_rules != 0;
    const float fallback = (float)(thr + (1.0 - thr) * 0.5);          // every row's velocity without the head
    const bool want_vel = a.vel_out != nullptr, want_held = a.held_out != nullptr;

    if (a.instr && a.instr_out) {
        if (p.live) a.instr_out[(size_t)p.v * (size_t)a.ld_out + w] = a.instr[(size_t)p.v * (size_t)a.instr_stride_v + (size_t)w * (size_t)a.instr_stride_w];
        if (p.w0 + p.nw == a.n) {
            const int pad = a.ld_out - a.n;
            for (int i = l; i < pad * p.V; i += BLOCK) a.instr_out[(size_t)(i / pad) * (size_t)a.ld_out + a.n + i % pad] = 0;
        }
    }

    int pp = -1;
    float pv = 0.0f;
    for (int tick0 = 0; tick0 < p.ticks; tick0 += CHUNK_TICKS) {
        const int nt = min(CHUNK_TICKS, p.ticks - tick0);
        __syncthreads();          // the previous chunk has been written out
        stage(p, a.idx, a.stride_t, a.stride_w, tick0, nt, ti);
        if (a.vel && (want_vel || want_held)) stage(p, a.vel, a.stride_t, a.stride_w, tick0, nt, tv);
        if (a.held_idx && want_held) stage(p, a.held_idx, a.stride_t, a.stride_w, tick0, nt, th);
        __syncthreads();
        if (p.live && (want_vel || want_held))
            for (int k = 0; k < nt; ++k) {
                const int at = k * BLOCK + l;
                const int x = ti[at];
                const bool snd = roll_sounding(a.silent, a.n_pitch, x);
                float out = fallback;
                if (a.vel) {
                    const float v0 = snd ? tv[at] : 0.0f;
                    out = rules ? velocity_rule_step(snd, x, v0, thr, pp, pv) : v0;
                }
                tv[at] = out;
                if (!a.held_idx) th[at] = a.vel ? ((double)out > thr ? 0 : 1) : 1;
            }
        __syncthreads();
        if (a.x_out) unstage_tm(p, ti, a.n, a.T, a.ld_out, tick0, nt, false, a.x_out);
        if (a.x_rev_out) unstage_tm(p, ti, a.n, a.T, a.ld_out, tick0, nt, true, a.x_rev_out);
        if (want_vel) unstage_tm(p, tv, a.n, a.T, a.ld_out, tick0, nt, false, a.vel_out);
        if (want_held) unstage_tm(p, th, a.n, a.T, a.ld_out, tick0, nt, false, a.held_out);
    }
}

bool is_finite(double x) { return x - x == 0.0; }

}  // namespace

extern "C" int mvae_longsong_abi_version(void) { return 1; }

extern "C" size_t mvae_nearest_walk_workspace(int32_t N, int32_t S, int32_t Z) {
    if (N <= 0 || S <= 0 || Z <= 0) return 0;
    return (size_t)S * (size_t)walk_chunks(N) * 16 + (size_t)S * 8;
}

extern "C" int mvae_nearest_walk(const mvae_walk_args* a, void* stream) {
    if (!a || !a->all_z || !a->r_in || !a->picked || !a->workspace || !a->best_out || !a->dist_out || !a->z_out || !a->r_out) return MVAE_E_ARG;
    if (a->N <= 0 || a->S <= 0 || a->Z <= 0 || a->cap <= 0) return MVAE_E_ARG;
    if (a->n_picked < 0 || a->n_picked >= a->cap) return MVAE_E_ARG;
    if (a->r_f64 < 0 || a->r_f64 > 1 || a->hist_f64 < 0 || a->hist_f64 > 1) return MVAE_E_ARG;
    if (!is_finite(a->e) || !is_finite(a->den) || a->den == 0.0) return MVAE_E_ARG;
    if (a->Z > MVAE_WALK_MAX_Z) return MVAE_E_UNSUPPORTED;
    if (a->ld_all < a->Z || a->ld_r < a->Z || a->ld_z < a->Z || a->ld_rout < a->Z) return MVAE_E_ARG;
    if (a->hist_out && (a->ld_hist < a->Z || (a->hist_in && a->ld_hist_in < a->Z))) return MVAE_E_ARG;
    const long long groups = ((long long)a->S + SONG_GROUP - 1) / SONG_GROUP;
    const long long blocks = walk_chunks(a->N) * groups;
    if (blocks > 0x7fffffffLL) return MVAE_E_UNSUPPORTED;          // (N * S beyond 2^42: more workgroups than a grid holds)
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (a->r_f64) {
        hipLaunchKernelGGL(walk_search_k<double>, dim3((unsigned)blocks), dim3(WB), 0, s, *a, (int)groups);
        MVAE_CHECK_LAUNCH();
        hipLaunchKernelGGL(walk_pull_k<double>, dim3((unsigned)a->S), dim3(WB), 0, s, *a);
    } else {
        hipLaunchKernelGGL(walk_search_k<float>, dim3((unsigned)blocks), dim3(WB), 0, s, *a, (int)groups);
        MVAE_CHECK_LAUNCH();
        hipLaunchKernelGGL(walk_pull_k<float>, dim3((unsigned)a->S), dim3(WB), 0, s, *a);
    }
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

extern "C" int mvae_feedback_rows(const mvae_feedback_args* a, void* stream) {
    if (roll_args_refused(a) || rule_args_refused(a)) return MVAE_E_ARG;
    if (!a->x_out && !a->x_rev_out && !a->vel_out && !a->held_out && !a->instr_out) return MVAE_E_ARG;
    if (a->instr && (a->instr_stride_v <= 0 || a->instr_stride_w <= 0)) return MVAE_E_ARG;
    if (a->T > MVAE_FEEDBACK_MAX_T) return MVAE_E_UNSUPPORTED;
    if (a->ld_out < a->n) return MVAE_E_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int wpb = BLOCK / a->voices;
    const dim3 grid((unsigned)(((long long)a->n + wpb - 1) / wpb)), block(BLOCK);
    hipLaunchKernelGGL(feedback_rows_k, grid, block, 0, s, *a);
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

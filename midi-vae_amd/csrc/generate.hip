// Generated songs on the device: the decoder's latent rows of interpolation songs and medleys from a few anchor codes and a
// four-column recipe (reference vae_evaluation.py:578-584, :705-887), and the piano-roll image of decoded songs (prepare_for_drawing,
// :619-642, followed by data_class.monophonic_to_khot_pianoroll).  C ABI: include/midivae_generate.h.
//
// latent_paths_k: ONE LANE PER ELEMENT of the (count, Z) block, adjacent lanes adjacent columns.  A lane forms the value of its window
// and, where a history is wanted, the value of the window before it from that window's own table row - two anchors more to read,
// nobody to wait for.  The blend is written one operation a statement under fp contract(off): the products are rounded before the sum.
//
// pianoroll_k: ONE LANE PER (WINDOW, VOICE) as recon.hip, the voices of a window in adjacent lanes; rows come through LDS tiles
// [tick][lane] in chunks of CHUNK_TICKS ticks.  What a row displays depends on the row one tick earlier only through two registers
// (pitch or -1, level), so a lane walks its window forwards.  What the window inherits it finds by walking the voice's rows back from
// the window's first row until a struck row or a break of the chain - as long as the held run that reaches the window.  The image
// rows of a chunk are then summed by all lanes of the workgroup, one lane per (window, tick, column), contiguous doubles.
#include "rolls.h"

#include "../../include/midivae_generate.h"

namespace {

constexpr int BLOCK = VOICE_BLOCK;
static_assert(MVAE_PIANOROLL_MAX_VOICES == ROLL_MAX_VOICES, "rolls.h refuses more voices than the header's limit");
constexpr int CHUNK_TICKS = 8;
constexpr int PATH_LANES = 256, PATH_MAX_BLOCKS = 1 << 20;

// ---- latent paths ----------------------------------------------------------------------------------------------------------------
template <class F>
__device__ __forceinline__ float path_value(const mvae_paths_args& a, int w, int j) {
#pragma clang fp contract(off)
    const int i0 = a.a0[w], i1 = a.a1[w];
    if (i0 < 0 || i0 >= a.n_anchors || i1 >= a.n_anchors) return __builtin_nanf("");
    const F* A = static_cast<const F*>(a.anchors);
    const F x = A[(size_t)i0 * a.ld_anchor + j];
    if (i1 < 0) return (float)x;
    const F y = A[(size_t)i1 * a.ld_anchor + j];
    const F k0 = (F)a.c0[w], k1 = (F)a.c1[w];
    const F p = x * k0;
    const F q = y * k1;
    const F s = p + q;
    return (float)s;
}

template <class F>
__global__ __launch_bounds__(PATH_LANES) void latent_paths_k(const mvae_paths_args a) {
    const long long total = (long long)a.count * a.Z;
    for (long long i = (long long)blockIdx.x * PATH_LANES + threadIdx.x; i < total; i += (long long)gridDim.x * PATH_LANES) {
        const int r = (int)(i / a.Z), j = (int)(i - (long long)r * a.Z);
        const int w = a.lo + r;
        a.z_out[(size_t)r * a.ld_z + j] = path_value<F>(a, w, j);
        if (a.hist_out) {
            const bool carried = w > 0 && a.first_window != nullptr && a.first_window[w] < w;
            a.hist_out[(size_t)r * a.ld_hist + j] = carried ? path_value<F>(a, w - 1, j) : 0.0f;
        }
    }
}

// ---- piano-roll image ------------------------------------------------------------------------------------------------------------
// what the row (w, t) of a voice displays, found by walking the voice's rows back through the song that starts at window fw
__device__ __forceinline__ void display_of(const mvae_pianoroll_args& a, int fw, int w, int t, int& pitch, double& level) {
    pitch = -1;
    level = 0.0;
    int chain = -2;          // the cur every row of the chain shares; -2: not yet known
    for (;;) {
        const size_t at = (size_t)t * (size_t)a.stride_t + (size_t)w * (size_t)a.stride_w;
        const int x = a.idx[at];
        const bool snd = roll_sounding(a.silent, a.n_pitch, x);
        const int cur = snd ? x : 0;
        if (chain != -2 && cur != chain) return;          // the later row does not continue what this one displays
        chain = cur;
        const double v = (double)a.vel[at];
        if (v > a.threshold) {
            if (snd) {
                pitch = x;
                level = (v - a.threshold) * a.max_velocity;
            }
            return;
        }
        const long long step = (long long)(w - fw) * a.T + t;
        if (step <= a.voices) return;                      // (the rows at step == voices never inherit)
        t -= a.voices;
        if (t < 0) {
            t += a.T;
            --w;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void pianoroll_k(const mvae_pianoroll_args a) {
    __shared__ uint8_t ti[CHUNK_TICKS * BLOCK];
    __shared__ float tv[CHUNK_TICKS * BLOCK];
    __shared__ short dp[CHUNK_TICKS * BLOCK];
    __shared__ double dl[CHUNK_TICKS * BLOCK];
    const Place p(a);
    const int l = threadIdx.x, V = p.V;
    const int w = p.w0 + p.wl;
    const bool drawn = a.vel != nullptr;
    const double thr = a.threshold, scale = a.max_velocity;

    int fw = w, pitch = -1;
    double level = 0.0;
    if (p.live && drawn) {
        if (a.first_window) fw = min(max(a.first_window[w], 0), w);
        if (w > fw) display_of(a, fw, w - 1, a.T - V + p.v, pitch, level);
    }
    const long long step0 = (long long)(w - fw) * a.T + p.v;

    for (int tick0 = 0; tick0 < p.ticks; tick0 += CHUNK_TICKS) {
        const int nt = min(CHUNK_TICKS, p.ticks - tick0);
        __syncthreads();          // the previous chunk's image rows have been written
        stage(p, a.idx, a.stride_t, a.stride_w, tick0, nt, ti);
        if (drawn) stage(p, a.vel, a.stride_t, a.stride_w, tick0, nt, tv);
        __syncthreads();
        if (p.live)
            for (int k = 0; k < nt; ++k) {
                const int at = k * BLOCK + l;
                const int x = ti[at];
                const bool snd = roll_sounding(a.silent, a.n_pitch, x);
                if (!drawn) {
                    pitch = snd ? x : -1;
                    level = 1.0;
                } else {
                    const double v = (double)tv[at];
                    if (v > thr) {
                        pitch = snd ? x : -1;
                        level = (v - thr) * scale;
                    } else {
                        const long long step = step0 + (long long)(tick0 + k) * V;
                        const int cur = snd ? x : 0;
                        if (!(step > V && pitch == cur)) pitch = -1;
                    }
                }
                dp[at] = (short)pitch;
                dl[at] = level;
            }
        __syncthreads();
        // tick (w0 + wl) * ticks + tick0 + k of the run, column c: the voices of the tick in ascending order
        const int per_window = nt * a.n_pitch, total = per_window * p.nw;
        for (int i = l; i < total; i += BLOCK) {
            const int wl = i / per_window, r = i - wl * per_window;
            const int k = r / a.n_pitch, c = r - k * a.n_pitch;
            double sum = 0.0;
            for (int v = 0; v < V; ++v) {
                const int at = k * BLOCK + wl * V + v;
                if (dp[at] == c) sum = drawn ? sum + dl[at] : 1.0;
            }
            a.img_out[((size_t)(p.w0 + wl) * p.ticks + tick0 + k) * (size_t)a.ld_img + c] = sum;
        }
    }
}

bool is_finite(double x) { return x - x == 0.0; }

}  // namespace

extern "C" int mvae_generate_abi_version(void) { return 1; }

extern "C" int mvae_latent_paths(const mvae_paths_args* a, void* stream) {
    if (!a || !a->anchors || !a->a0 || !a->a1 || !a->c0 || !a->c1 || !a->z_out) return MVAE_E_ARG;
    if (a->n <= 0 || a->count <= 0 || a->Z <= 0 || a->n_anchors <= 0 || a->lo < 0) return MVAE_E_ARG;
    if ((long long)a->lo + a->count > a->n) return MVAE_E_ARG;
    if (a->anchor_f64 < 0 || a->anchor_f64 > 1) return MVAE_E_ARG;
    if (a->Z > MVAE_PATHS_MAX_Z) return MVAE_E_UNSUPPORTED;
    if (a->ld_anchor < a->Z || a->ld_z < a->Z || (a->hist_out && a->ld_hist < a->Z)) return MVAE_E_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long total = (long long)a->count * a->Z;
    const long long blocks = (total + PATH_LANES - 1) / PATH_LANES;
    const dim3 grid((unsigned)(blocks < PATH_MAX_BLOCKS ? blocks : PATH_MAX_BLOCKS)), block(PATH_LANES);
    if (a->anchor_f64)
        hipLaunchKernelGGL(latent_paths_k<double>, grid, block, 0, s, *a);
    else
        hipLaunchKernelGGL(latent_paths_k<float>, grid, block, 0, s, *a);
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

extern "C" int mvae_pianoroll(const mvae_pianoroll_args* a, void* stream) {
    if (roll_args_refused(a) || !a->img_out) return MVAE_E_ARG;
    if (!is_finite(a->threshold) || !is_finite(a->max_velocity)) return MVAE_E_ARG;
    if (a->n_pitch > MVAE_PIANOROLL_MAX_PITCH || a->T > MVAE_PIANOROLL_MAX_T) return MVAE_E_UNSUPPORTED;
    if (a->ld_img < a->n_pitch) return MVAE_E_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int wpb = BLOCK / a->voices;
    const dim3 grid((unsigned)(((long long)a->n + wpb - 1) / wpb)), block(BLOCK);
    hipLaunchKernelGGL(pianoroll_k, grid, block, 0, s, *a);
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

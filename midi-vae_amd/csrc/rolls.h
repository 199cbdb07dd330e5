// What the kernels over decoded piano-roll windows share (descriptors.hip, sweep.hip, recon.hip, events.hip): which row sounds, the exact
// integer statistics of a list, the rows of a chunk of ticks with one lane per window, one row of the velocity post-rule, and the
// refusals common to the three entry points.  Row t of a window is voice t % V of tick t // V.
#pragma once
#include "common.h"

namespace {

constexpr int LANES = 64;                  // the one-lane-per-window kernels: one wave per workgroup
constexpr int TILE_LD = LANES + 1;         // a staged row is 65 elements from the next: the 64 stores of a fetch spread over the banks
constexpr int ROLL_MAX_VOICES = 8;         // = MVAE_DESC_MAX_VOICES = MVAE_SWEEP_MAX_VOICES = MVAE_RECON_MAX_VOICES

// an index is a note unless it is the silent index, 255 ("no target") or past the pitch range
__device__ __forceinline__ bool roll_sounding(int silent, int n_pitch, int x) { return x != silent && x != 255 && x < n_pitch; }

// count, max, min and the exact sums of a list of non-negative integers
struct Stats {
    long long c = 0, s = 0, q = 0;
    int hi = 0, lo = 0x7fffffff;
    __device__ void push(int x) {
        ++c;
        s += x;
        q += (long long)x * x;
        hi = max(hi, x);
        lo = min(lo, x);
    }
    __device__ double mean() const { return (double)s / (double)c; }
    __device__ double std() const { return sqrt((double)(c * q - s * s) / (double)(c * c)); }
    // max, min, mean, std over ``scale``; zeros for an empty list (the signature vector)
    __device__ void store_scaled(double* out, double scale) const {
        if (c == 0) {
            out[0] = out[1] = out[2] = out[3] = 0.0;
            return;
        }
        out[0] = (double)hi / scale;
        out[1] = (double)lo / scale;
        out[2] = mean() / scale;
        out[3] = std() / scale;
    }
    // mean, median, min, max, range, std; NaN for an empty list (the sweep's table)
    __device__ void store_six(double* out, double median) const {
        if (c == 0) {
            for (int i = 0; i < 6; ++i) out[i] = __builtin_nan("");
            return;
        }
        out[0] = mean();
        out[1] = median;
        out[2] = (double)lo;
        out[3] = (double)hi;
        out[4] = (double)(hi - lo);
        out[5] = std();
    }
};

// The rows of CHUNK_TICKS ticks of a workgroup's 64 windows, one lane per window: the index and, WITH_VEL, the float velocity (a.vel,
// NULL allowed).  Time-major buffers (stride_w == 1, !STAGED) are read straight from memory, adjacent lanes adjacent elements; any
// other layout is STAGED through LDS tiles of TILE elements: consecutive lanes fetch consecutive rows of ONE window (contiguous when
// stride_t == 1) and the tile is read back [row][lane].
template <class Args, bool STAGED, bool WITH_VEL, int CHUNK_TICKS>
struct Rows {
    static constexpr int TILE = STAGED ? CHUNK_TICKS * ROLL_MAX_VOICES * TILE_LD : 1;
    const Args& a;
    uint8_t* ti;
    float* tv;
    const int lane, w0;
    __device__ Rows(const Args& a_, uint8_t* ti_, float* tv_ = nullptr) : a(a_), ti(ti_), tv(tv_), lane(threadIdx.x), w0(blockIdx.x * LANES) {}

    // before the ticks [tick0, tick0 + nt) are read (every lane of the workgroup calls it)
    __device__ void open(int tick0, int nt) {
        if (!STAGED) return;
        const int rows = nt * a.voices;
        const int nw = min(LANES, a.n - w0);
        __syncthreads();          // the previous chunk has been read
        for (int i = lane; i < nw * rows; i += LANES) {
            const int wl = i / rows, r = i - wl * rows;
            const size_t at = (size_t)(tick0 * a.voices + r) * a.stride_t + (size_t)(w0 + wl) * a.stride_w;
            ti[r * TILE_LD + wl] = a.idx[at];
            if constexpr (WITH_VEL)
                if (a.vel) tv[r * TILE_LD + wl] = a.vel[at];
        }
        __syncthreads();
    }
    __device__ size_t at(int tick0, int r) const { return (size_t)(tick0 * a.voices + r) * a.stride_t + (size_t)(w0 + lane) * a.stride_w; }
    // row r of the open chunk, window w0 + lane (< n)
    __device__ int idx(int tick0, int r) const { return STAGED ? ti[r * TILE_LD + lane] : a.idx[at(tick0, r)]; }
    __device__ float vel(int tick0, int r) const { return STAGED ? tv[r * TILE_LD + lane] : a.vel[at(tick0, r)]; }
};

// The kernels with ONE LANE PER (WINDOW, VOICE) (recon.hip, events.hip): the voices of a window in adjacent lanes, VOICE_BLOCK lanes a
// workgroup hold VOICE_BLOCK / voices windows; rows travel through LDS tiles [tick][lane].
constexpr int VOICE_BLOCK = 256;

// the workgroup's windows and this lane's place among them
struct Place {
    int V, wpb, w0, nw, wl, v, ticks;
    bool live;
    template <class Args>
    __device__ Place(const Args& a) {
        V = a.voices;
        wpb = VOICE_BLOCK / V;
        const long long first = (long long)blockIdx.x * wpb;
        w0 = (int)first;
        nw = (int)min((long long)wpb, (long long)a.n - first);
        wl = threadIdx.x / V;
        v = threadIdx.x - wl * V;
        ticks = a.T / V;
        live = wl < nw;
    }
};

// rows [tick0 * V, (tick0 + nt) * V) of the workgroup's windows -> tile[tick][wl * V + voice]; every lane of the workgroup calls it
template <class E>
__device__ __forceinline__ void stage(const Place& p, const E* src, int64_t stride_t, int64_t stride_w, int tick0, int nt, E* tile) {
    const int rows = nt * p.V, total = rows * p.nw;
    const size_t base = (size_t)tick0 * p.V * (size_t)stride_t + (size_t)p.w0 * (size_t)stride_w;
    if (stride_w == 1) {          // time-major: adjacent lanes, adjacent windows
        for (int i = threadIdx.x; i < total; i += VOICE_BLOCK) {
            const int r = i / p.nw, wl = i - r * p.nw;
            tile[(r / p.V) * VOICE_BLOCK + wl * p.V + r % p.V] = src[base + (size_t)r * (size_t)stride_t + (size_t)wl];
        }
    } else {                      // adjacent lanes, adjacent rows of a window
        for (int i = threadIdx.x; i < total; i += VOICE_BLOCK) {
            const int wl = i / rows, r = i - wl * rows;
            tile[(r / p.V) * VOICE_BLOCK + wl * p.V + r % p.V] = src[base + (size_t)r * (size_t)stride_t + (size_t)wl * (size_t)stride_w];
        }
    }
}

// One row of the velocity post-rule (reference vae_definition.py:1156-1190) for one voice: ``snd`` whether the row sounds, ``x`` its
// index, ``v0`` its velocity (0 on a row that does not sound); ``pp`` / ``pv`` the voice's previous pitch (-1: none) and the last
// velocity that was not silent, updated in place (LDS slots or registers).  The comparison with the threshold is a double's, the
// value stays the float it was: an input or a zero.
__device__ __forceinline__ float velocity_rule_step(bool snd, int x, float v0, double thr, int& pp, float& pv) {
    const int pitch = snd ? x : -1;
    const bool vel_silent = (double)v0 < thr;
    float out = v0;
    if (vel_silent) {
        if (snd && pp > 0 && pp != pitch) out = pv;          // (> 0, not >= 0: the reference's own test)
    } else if (!snd) {
        out = 0.0f;
    }
    pp = pitch;
    if (!vel_silent) pv = v0;                                // (the value before the rule)
    return out;
}

// the MVAE_E_ARG refusals every entry point over rolls makes first: ``a`` is a mvae_desc_args, mvae_sweep_args or mvae_recon_args
template <class Args>
static inline bool roll_args_refused(const Args* a) {
    if (!a || !a->idx) return true;
    if (a->n <= 0 || a->T <= 0 || a->n_pitch <= 0 || a->stride_t <= 0 || a->stride_w <= 0) return true;
    if (a->voices < 2 || a->voices > ROLL_MAX_VOICES || a->T % a->voices) return true;
    return a->silent < -1 || a->silent > 255;
}
// ... and of the two that apply the velocity rule: the switch is 0 or 1, the threshold finite
template <class Args>
static inline bool rule_args_refused(const Args* a) {
    return a->override_rules < 0 || a->override_rules > 1 || !(a->threshold - a->threshold == 0.0);
}

}  // namespace

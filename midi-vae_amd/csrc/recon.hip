// Song-level decode on the device: the velocity post-rules of the reference (vae_definition.py:1156-1190) with the per-voice state
// carried from one window of a song into the next, the note starts and the counts of the reconstruction report
// (vae_evaluation.py:2211-2236, :2380-2397).  C ABI: include/midivae_recon.h.
//
// Mapping: ONE LANE PER (WINDOW, VOICE), the voices of a window in adjacent lanes; 256 lanes a workgroup hold 256 / voices windows.
// A lane walks the T / voices rows of its voice, so its whole state is two registers (previous pitch, previous velocity) - nothing a
// lane indexes dynamically, nothing in scratch (the Makefile checks it).
//
// The rule has no serial chain through a song.  What window w inherits is the pitch of the last row of window w - 1 and the velocity
// of the nearest earlier row whose velocity was not silent, so the order between windows comes from three launches and from nothing
// else - no lane waits for a flag of another workgroup:
//   recon_carry_k   every lane walks its rows and leaves an 8-byte record: the pitch of its last row, whether any row's velocity was
//                   not silent, and the last such velocity;
//   recon_apply_k   every lane takes previous_pitch from the record of window w - 1 (-1 at the song's first window) and walks the
//                   records back from w - 1 to first_window[w] until one holds a velocity (as long as the song only for a voice that
//                   never plays), then applies the rule, writes velocities and note starts and counts; the counts of a window are
//                   summed over its voices' lanes through LDS - integers, one writer per window, no atomics.
// recon_carry_k is launched only where a state is carried: with vel, override_rules and first_window.
//
// Rows travel through LDS both ways, in chunks of CHUNK_TICKS ticks laid out [tick][lane]: a lane's byte and its neighbours' share a
// dword (reads of one dword by several lanes are a broadcast, not a bank conflict), and the global side of every copy is contiguous
// - along a window's rows for window-major arrays and for the two outputs, along the windows for time-major (T, Bp) buffers.
#include "rolls.h"

#include "../../include/midivae_recon.h"

namespace {

constexpr int BLOCK = VOICE_BLOCK;
static_assert(MVAE_RECON_MAX_VOICES == ROLL_MAX_VOICES, "rolls.h refuses more voices than the header's limit");
constexpr int MAXP = MVAE_RECON_MAX_PITCH, MAX_T = MVAE_RECON_MAX_T;
constexpr int CHUNK_TICKS = 8;
constexpr int NCOUNT = 6;          // what a lane counts: columns 0, 1, 2, 5, 6, 7

// the same chunk of a tile -> a window-major (n, T) output
template <class E>
__device__ __forceinline__ void unstage(const Place& p, const E* tile, int T, int tick0, int nt, E* dst) {
    const int rows = nt * p.V, total = rows * p.nw;
    E* out = dst + (size_t)p.w0 * T + (size_t)tick0 * p.V;
    for (int i = threadIdx.x; i < total; i += BLOCK) {
        const int wl = i / rows, r = i - wl * rows;
        out[(size_t)wl * T + r] = tile[(r / p.V) * BLOCK + wl * p.V + r % p.V];
    }
}

// the record a (window, voice) leaves: x = the bits of the last velocity that was not silent, y = (one exists) << 16 | last pitch + 1
__device__ __forceinline__ uint2 record(int pitch, bool has, float last) {
    return make_uint2(__float_as_uint(last), ((uint32_t)has << 16) | (uint32_t)(pitch + 1));
}

__global__ __launch_bounds__(BLOCK) void recon_carry_k(const mvae_recon_args a) {
    __shared__ uint8_t ti[CHUNK_TICKS * BLOCK];
    __shared__ float tv[CHUNK_TICKS * BLOCK];
    const Place p(a);
    const int l = threadIdx.x;
    const double thr = a.threshold;
    int pitch = -1;
    bool has = false;
    float last = 0.0f;
    for (int tick0 = 0; tick0 < p.ticks; tick0 += CHUNK_TICKS) {
        const int nt = min(CHUNK_TICKS, p.ticks - tick0);
        __syncthreads();          // the previous chunk has been read
        stage(p, a.idx, a.stride_t, a.stride_w, tick0, nt, ti);
        stage(p, a.vel, a.stride_t, a.stride_w, tick0, nt, tv);
        __syncthreads();
        if (!p.live) continue;
        for (int k = 0; k < nt; ++k) {
            const int x = ti[k * BLOCK + l];
            const bool snd = roll_sounding(a.silent, a.n_pitch, x);
            const float v0 = snd ? tv[k * BLOCK + l] : 0.0f;
            pitch = snd ? x : -1;
            if (!((double)v0 < thr)) {
                has = true;
                last = v0;
            }
        }
    }
    if (p.live) reinterpret_cast<uint2*>(a.carry)[(size_t)(p.w0 + p.wl) * p.V + p.v] = record(pitch, has, last);
}

__global__ __launch_bounds__(BLOCK) void recon_apply_k(const mvae_recon_args a) {
    __shared__ uint8_t ti[CHUNK_TICKS * BLOCK], th[CHUNK_TICKS * BLOCK], to[CHUNK_TICKS * BLOCK];
    __shared__ float tv[CHUNK_TICKS * BLOCK];
    __shared__ int red[NCOUNT][BLOCK];
    const Place p(a);
    const int l = threadIdx.x, T = a.T;
    const int w = p.w0 + p.wl;
    const double thr = a.threshold;
    const bool rules = a.vel != nullptr && a.override_rules != 0;
    const float fallback = (float)(thr + (1.0 - thr) * 0.5);          // every row's velocity without the head

    // ---- what the song hands this (window, voice): a.carry is NULL where nothing is carried ----
    int pp0 = -1;
    float pv0 = 0.0f;
    if (a.carry && p.live) {
        const uint2* rec = reinterpret_cast<const uint2*>(a.carry);
        const int fw = min(max(a.first_window[w], 0), w);
        if (w > fw) {
            pp0 = (int)(rec[(size_t)(w - 1) * p.V + p.v].y & 0xffffu) - 1;
            for (int u = w - 1; u >= fw; --u) {
                const uint2 r = rec[(size_t)u * p.V + p.v];
                if (r.y >> 16) {
                    pv0 = __uint_as_float(r.x);
                    break;
                }
            }
        }
    }
    // the voice's state through this window, variables of its own: velocity_rule_step takes references, and with references to what the
    // look-back loop assigns hipcc hoists that loop's velocity load behind it at a fifth more time per record
    int pp = pp0;
    float pv = pv0;

    int c_orig = 0, c_pred = 0, c_both = 0, c_start = 0, c_start_pred = 0, c_start_orig = 0;
    for (int tick0 = 0; tick0 < p.ticks; tick0 += CHUNK_TICKS) {
        const int nt = min(CHUNK_TICKS, p.ticks - tick0);
        __syncthreads();          // the previous chunk has been written out
        stage(p, a.idx, a.stride_t, a.stride_w, tick0, nt, ti);
        if (a.vel) stage(p, a.vel, a.stride_t, a.stride_w, tick0, nt, tv);
        if (a.held) stage(p, a.held, a.stride_t, a.stride_w, tick0, nt, th);
        if (a.orig) stage(p, a.orig, a.orig_stride_t, a.orig_stride_w, tick0, nt, to);
        __syncthreads();
        if (p.live)
            for (int k = 0; k < nt; ++k) {
                const int at = k * BLOCK + l;
                const int x = ti[at];
                const bool snd = roll_sounding(a.silent, a.n_pitch, x);
                float out = fallback;
                if (a.vel) {
                    const float v0 = snd ? tv[at] : 0.0f;
                    out = v0;
                    out = rules ? velocity_rule_step(snd, x, v0, thr, pp, pv) : v0;
                }
                tv[at] = out;
                int start = 1;
                if (a.held)
                    start = th[at];
                else if (a.vel)
                    start = (double)out > thr ? 0 : 1;
                th[at] = (uint8_t)start;
                const bool osnd = a.orig != nullptr && roll_sounding(a.silent, a.n_pitch, to[at]);
                c_orig += osnd;
                c_pred += snd;
                c_both += osnd && snd && to[at] == x;
                c_start += start == 0;
                c_start_pred += start == 0 && !snd;
                c_start_orig += a.orig != nullptr && start == 0 && !osnd;
            }
        if (a.vel_out || a.start_out) {
            __syncthreads();
            if (a.vel_out) unstage(p, tv, T, tick0, nt, a.vel_out);
            if (a.start_out) unstage(p, th, T, tick0, nt, a.start_out);
        }
    }
    if (!a.counts_out) return;
    red[0][l] = c_orig;
    red[1][l] = c_pred;
    red[2][l] = c_both;
    red[3][l] = c_start;
    red[4][l] = c_start_pred;
    red[5][l] = c_start_orig;
    __syncthreads();
    if (p.live && p.v == 0) {
        int s[NCOUNT];
#pragma unroll
        for (int c = 0; c < NCOUNT; ++c) {
            s[c] = 0;
            for (int j = 0; j < p.V; ++j) s[c] += red[c][l + j];
        }
        int* out = a.counts_out + (size_t)w * a.ld_counts;
        out[0] = s[0];
        out[1] = s[1];
        out[2] = s[2];
        out[3] = s[0] - s[2];
        out[4] = s[1] - s[2];
        out[5] = s[3];
        out[6] = s[4];
        out[7] = s[5];
    }
}

}  // namespace

extern "C" int mvae_recon_abi_version(void) { return 1; }

extern "C" int mvae_recon_songs(const mvae_recon_args* a, void* stream) {
    if (roll_args_refused(a) || rule_args_refused(a) || (!a->vel_out && !a->start_out && !a->counts_out)) return MVAE_E_ARG;
    if (a->orig && (a->orig_stride_t <= 0 || a->orig_stride_w <= 0)) return MVAE_E_ARG;
    if (a->counts_out && a->ld_counts < MVAE_RECON_COUNTS) return MVAE_E_ARG;
    const bool carried = a->vel && a->override_rules && a->first_window;
    if (carried && !a->carry) return MVAE_E_ARG;
    if (a->n_pitch > MAXP || a->T > MAX_T) return MVAE_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int wpb = BLOCK / a->voices;
    const dim3 grid((unsigned)(((long long)a->n + wpb - 1) / wpb)), block(BLOCK);
    mvae_recon_args k = *a;
    if (!carried) k.carry = nullptr;
    if (carried) {
        hipLaunchKernelGGL(recon_carry_k, grid, block, 0, s, k);
        MVAE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(recon_apply_k, grid, block, 0, s, k);
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

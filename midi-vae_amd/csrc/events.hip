// Note events on the device: what the reference's rolls_to_midi (midi_functions.py:57-137) makes of a decoded song's rolls, without
// its row-by-row tracker.  C ABI and semantics: include/midivae_events.h.
//
// For the one-hot rows of a decode the tracker holds, after row i, the voice's pitch of row i or nothing, so whether a note ends or
// starts on tick i is a function of ticks i - 1 and i alone, starts and ends alternate per voice, and the k-th start pairs with the
// k-th end: two flag passes, a prefix sum and a compaction.
//
// Mapping as in recon.hip: ONE LANE PER (WINDOW, VOICE), 256 lanes a workgroup hold 256 / voices windows, rows staged through LDS
// tiles [tick][lane]; a lane's state is a handful of registers, nothing in scratch (the Makefile checks it).  A lane reads the last
// row of its voice in the previous window of its song for p_{i-1} of its first tick, so a note may span windows, workgroups and
// engine batches.  Order comes from four launches on the stream and from nothing else - no workgroup waits for another:
//   events_first_k        the first and the last window of every song (one writer each);
//   events_walk_k<false>  every lane counts the starts and the ends that fall on its ticks;
//   events_scan_k         ONE workgroup, looping: the counts become exclusive ranks within (song, voice) by a segmented scan over the
//                         windows, a song's last window leaves the totals, and a scan over (song, voice) gives `offsets` and `total`;
//   events_walk_k<true>   the same walk writes: a start's fields at base + rank(start) while that rank is below the notes of its
//                         (song, voice), an end's tick at base + rank(end).  The two are different dwords of a record.
// Every record position is compared with `capacity` before it is written, whatever the song ordinals hold.
#include "rolls.h"

#include "../../include/midivae_events.h"

namespace {

constexpr int BLOCK = VOICE_BLOCK;
static_assert(MVAE_EVENTS_MAX_VOICES == ROLL_MAX_VOICES, "rolls.h refuses more voices than the header's limit");
constexpr int CHUNK_TICKS = 8;
constexpr int SCAN_BLOCK = 1024;
static_assert(sizeof(mvae_note_event) == 12, "a record is three dwords");

// the workspace: MVAE_EVENTS_WORKSPACE_BYTES
struct Work {
    int *rank_s, *rank_e;          // [n * V]         counts of (window, voice), then their exclusive ranks within (song, voice)
    int *tot_s, *tot_e;            // [n_songs * V]   starts and ends of (song, voice)
    int *first, *last;             // [n_songs]       the song's first and last window
    __device__ Work(const mvae_events_args& a) {
        const size_t nv = (size_t)a.n * a.voices, m = (size_t)a.n_songs * a.voices;
        rank_s = static_cast<int*>(a.workspace);
        rank_e = rank_s + nv;
        tot_s = rank_e + nv;
        tot_e = tot_s + m;
        first = tot_e + m;
        last = first + a.n_songs;
    }
};

__global__ __launch_bounds__(BLOCK) void events_first_k(const mvae_events_args a) {
    const Work ws(a);
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (at >= a.n) return;
    const int w = (int)at, s = a.song[w];
    if (s < 0 || s >= a.n_songs) return;
    if (w == 0 || a.song[w - 1] != s) ws.first[s] = w;
    if (w == a.n - 1 || a.song[w + 1] != s) ws.last[s] = w;
}

// the velocity of a note that starts on a row of velocity x (reference :78-81, :117-118, :134), in double, in the reference's order
__device__ __forceinline__ int note_velocity(float x32, double thr) {
    double x = (double)x32;
    if (x < thr) x = 0.0;
    if (x >= thr) x -= 0.5;
    const double y = (x / (1.0 - thr)) * 127.0;
    if (!(y == y)) return 0;
    if (y > 127.0) return 127;
    if (y < -32768.0) return -32768;
    return (int)y;
}

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void events_walk_k(const mvae_events_args a) {
    __shared__ uint8_t ti[CHUNK_TICKS * BLOCK], th[CHUNK_TICKS * BLOCK];
    __shared__ float tv[WRITE ? CHUNK_TICKS * BLOCK : 1];
    const Place p(a);
    const Work ws(a);
    const int l = threadIdx.x, V = p.V, w = p.w0 + p.wl, sn = a.smallest_note;
    const double thr = a.threshold;

    // ---- what the song hands this (window, voice): its tick in the song and the voice's pitch on the tick before ----
    int s = 0, prev = -1, tick = 0, phase = 0;
    bool in_song = false;
    if (p.live) {
        s = a.song[w];
        in_song = s >= 0 && s < a.n_songs;
        const int first = in_song ? min(max(ws.first[s], 0), w) : w;
        tick = (w - first) * p.ticks;
        phase = tick % sn;
        if (w > first) {
            const int x = a.idx[(size_t)(a.T - V + p.v) * (size_t)a.stride_t + (size_t)(w - 1) * (size_t)a.stride_w];
            prev = roll_sounding(a.silent, a.n_pitch, x) ? x : -1;
        }
    }
    // starts and ends so far: counted from 0, or (WRITE) from the lane's ranks within its (song, voice)
    int rs = 0, re = 0, ends = 0, notes = 0, song_ticks = 0;
    unsigned base = 0;
    if (WRITE && in_song) {
        const int slot = s * V + p.v;
        rs = ws.rank_s[w * V + p.v];
        re = ws.rank_e[w * V + p.v];
        ends = ws.tot_e[slot];
        notes = ends + (a.close_at_end && ws.tot_s[slot] > ends ? 1 : 0);
        base = (unsigned)a.offsets[slot];
        song_ticks = (ws.last[s] - ws.first[s] + 1) * p.ticks;
    }
    int32_t* rec = reinterpret_cast<int32_t*>(a.records);
    const unsigned cap = (unsigned)a.capacity;

    for (int tick0 = 0; tick0 < p.ticks; tick0 += CHUNK_TICKS) {
        const int nt = min(CHUNK_TICKS, p.ticks - tick0);
        __syncthreads();          // the previous chunk has been read
        stage(p, a.idx, a.stride_t, a.stride_w, tick0, nt, ti);
        if (a.held) stage(p, a.held, a.stride_t, a.stride_w, tick0, nt, th);
        if (WRITE && a.vel) stage(p, a.vel, a.stride_t, a.stride_w, tick0, nt, tv);
        __syncthreads();
        if (!p.live) continue;
        for (int k = 0; k < nt; ++k) {
            const int at = k * BLOCK + l;
            const int x = ti[at];
            const bool snd = roll_sounding(a.silent, a.n_pitch, x);
            const int pitch = snd ? x : -1;
            const bool cont = prev >= 0 && pitch == prev && (a.held ? th[at] != 0 : phase != 0);
            const bool end = prev >= 0 && !cont, start = snd && !cont;
            if (WRITE && in_song) {
                if (end) {
                    const unsigned pos = base + (unsigned)re;
                    if (pos < cap) rec[3 * (size_t)pos + 1] = tick;
                }
                if (start && rs < notes) {
                    const unsigned pos = base + (unsigned)rs;
                    if (pos < cap) {
                        const int vel = a.vel ? note_velocity(tv[at], thr) : (int)MVAE_EVENTS_DEFAULT_VELOCITY;
                        rec[3 * (size_t)pos] = tick;
                        if (rs == ends) rec[3 * (size_t)pos + 1] = song_ticks;          // (close_at_end: no end will come)
                        rec[3 * (size_t)pos + 2] =
                            (int32_t)((uint32_t)(pitch + a.pitch_base) | ((uint32_t)p.v << 8) | ((uint32_t)(vel & 0xffff) << 16));
                    }
                }
            }
            re += end;
            rs += start;
            prev = pitch;
            ++tick;
            if (++phase == sn) phase = 0;
        }
    }
    if (!WRITE && p.live) {
        ws.rank_s[w * V + p.v] = in_song ? rs : 0;
        ws.rank_e[w * V + p.v] = in_song ? re : 0;
    }
}

__global__ __launch_bounds__(SCAN_BLOCK) void events_scan_k(const mvae_events_args a) {
    __shared__ int xs[SCAN_BLOCK], xe[SCAN_BLOCK], fl[SCAN_BLOCK], carry[2][ROLL_MAX_VOICES];
    const Work ws(a);
    const int t = threadIdx.x, V = a.voices, M = a.n_songs * V;
    for (int j = t; j < M; j += SCAN_BLOCK) ws.tot_s[j] = ws.tot_e[j] = 0;          // (a song without windows: empty ranges)
    if (t < ROLL_MAX_VOICES) carry[0][t] = carry[1][t] = 0;
    __syncthreads();

    // ---- ranks within (song, voice): an inclusive scan over the windows, per voice, restarted at every song's first window ----
    const int wps = SCAN_BLOCK / V, wl = t / V, v = t - wl * V;
    for (int w0 = 0; w0 < a.n; w0 += wps) {
        const int w = w0 + wl;
        const bool live = wl < wps && w < a.n;
        int s = -1, own_s = 0, own_e = 0;
        bool head = false;
        if (live) {
            s = a.song[w];
            head = w == 0 || a.song[w - 1] != s;
            own_s = ws.rank_s[w * V + v];
            own_e = ws.rank_e[w * V + v];
        }
        const bool inherits = live && wl == 0 && !head;
        xs[t] = own_s + (inherits ? carry[0][v] : 0);
        xe[t] = own_e + (inherits ? carry[1][v] : 0);
        fl[t] = head;
        __syncthreads();
        for (int d = 1; d < wps; d <<= 1) {
            const bool take = live && wl >= d && !fl[t];
            int add_s = 0, add_e = 0, f = 0;
            if (take) {
                add_s = xs[t - d * V];
                add_e = xe[t - d * V];
                f = fl[t - d * V];
            }
            __syncthreads();
            if (take) {
                xs[t] += add_s;
                xe[t] += add_e;
                fl[t] = f;
            }
            __syncthreads();
        }
        if (live) {
            ws.rank_s[w * V + v] = xs[t] - own_s;
            ws.rank_e[w * V + v] = xe[t] - own_e;
            if ((w == a.n - 1 || a.song[w + 1] != s) && s >= 0 && s < a.n_songs) {
                ws.tot_s[s * V + v] = xs[t];
                ws.tot_e[s * V + v] = xe[t];
            }
            if (wl == wps - 1) {
                carry[0][v] = xs[t];
                carry[1][v] = xe[t];
            }
        }
        __syncthreads();          // the carry, and (after the last pass) the totals, are there
    }

    // ---- notes per (song, voice) -> offsets: an exclusive scan over the n_songs * V slots ----
    int run = 0;
    for (int j0 = 0; j0 < M; j0 += SCAN_BLOCK) {
        const int j = j0 + t;
        int val = 0;
        if (j < M) {
            const int ends = ws.tot_e[j];
            val = ends + (a.close_at_end && ws.tot_s[j] > ends ? 1 : 0);
        }
        xs[t] = val;
        __syncthreads();
        for (int d = 1; d < SCAN_BLOCK; d <<= 1) {
            const int add = t >= d ? xs[t - d] : 0;
            __syncthreads();
            xs[t] += add;
            __syncthreads();
        }
        if (j < M) a.offsets[j] = run + xs[t] - val;
        run += xs[SCAN_BLOCK - 1];
        __syncthreads();          // xs has been read
    }
    if (t == 0) {
        a.offsets[M] = run;
        *a.total = run;
    }
}

}  // namespace

extern "C" int mvae_events_abi_version(void) { return 1; }

extern "C" int mvae_note_events(const mvae_events_args* a, void* stream) {
    if (roll_args_refused(a) || !a->song || !a->workspace || !a->offsets || !a->total) return MVAE_E_ARG;
    if (a->n_songs <= 0 || a->n_songs > a->n || a->smallest_note <= 0 || !(a->threshold - a->threshold == 0.0)) return MVAE_E_ARG;
    if (a->pitch_base < 0 || (long long)a->pitch_base + a->n_pitch > 256 || a->close_at_end < 0 || a->close_at_end > 1) return MVAE_E_ARG;
    if (a->capacity < 0 || (a->capacity > 0 && !a->records)) return MVAE_E_ARG;
    if (a->T > MVAE_EVENTS_MAX_T || (long long)a->n * a->T > 0x7fffffffLL) return MVAE_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int wpb = BLOCK / a->voices;
    const dim3 windows((unsigned)(((long long)a->n + BLOCK - 1) / BLOCK)), lanes((unsigned)(((long long)a->n + wpb - 1) / wpb));
    hipLaunchKernelGGL(events_first_k, windows, dim3(BLOCK), 0, s, *a);
    MVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(events_walk_k<false>, lanes, dim3(BLOCK), 0, s, *a);
    MVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(events_scan_k, dim3(1), dim3(SCAN_BLOCK), 0, s, *a);
    MVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(events_walk_k<true>, lanes, dim3(BLOCK), 0, s, *a);
    MVAE_CHECK_LAUNCH();
    return MVAE_OK;
}

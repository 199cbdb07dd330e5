// Rolls from notes on the device: what the reference's load_rolls (import_midi.py:94-286) makes of a song's tick-quantised notes,
// without its Python loops over every tick of every track - the inverse of events.hip.  C ABI and semantics: include/midivae_import.h.
//
// The state of a (track, tick) is nine dwords of the workspace: which of the 128 pitches sound, which of them start there (the keys),
// and how many notes cover the tick.  Order comes from seven launches on the stream and from nothing else - no workgroup waits for
// another:
//   import_plan_k         ONE workgroup, looping: the first cell of every song, an exclusive scan of tracks * ticks over the songs;
//   import_clear_k        the masks and counts are zeroed;
//   import_paint_k        one lane per record: atomicOr into the pitch and key masks, atomicAdd into the count - integers, so the
//                         result does not depend on the order in which the lanes arrive;
//   import_concurrent_k   one workgroup per track, looping over its ticks: the maximum of the count;
//   import_allot_k        one lane per song: the reference's voice allotment (:161-231);
//   import_rows_k         one lane per output row: the (k+1)-th highest set bit of the tick's mask, in registers; idx, held, and
//                         zeros in the velocities;
//   import_velocity_k     one lane per record: the last record of a key finds its rank on its tick and its output voice and writes
//                         the velocity.
// Offsets and tick counts are device data nobody has checked: every index is compared with the totals the host passed (n_notes,
// n_tracks, n_windows, cells) before it is used, so a call never leaves the buffers those totals size.
#include "common.h"

#include "../../include/midivae_import.h"

namespace {

constexpr int BLOCK = 256;
constexpr int SCAN_BLOCK = 1024;
constexpr int MAX_V = MVAE_IMPORT_MAX_VOICES;
static_assert(sizeof(mvae_import_note) == 12, "a record is three dwords");

// the workspace: MVAE_IMPORT_WORKSPACE_BYTES
struct Work {
    unsigned *pm, *km;          // [cells][4]      painted pitches, keys
    int* count;                 // [cells]         notes that cover the tick
    int* first;                 // [n_songs + 1]   the song's first cell
    __device__ Work(const mvae_import_args& a) {
        pm = static_cast<unsigned*>(a.workspace);
        km = pm + 4 * (size_t)a.cells;
        count = reinterpret_cast<int*>(km + 4 * (size_t)a.cells);
        first = count + (size_t)a.cells;
    }
};

// the song that owns position x of a list whose songs start at off[0 .. n]: the last s with off[s] <= x, if x < off[s + 1]; else -1
__device__ __forceinline__ int owner(const int32_t* off, int n, int x) {
    int lo = 0, hi = n;          // invariant: off[lo] <= x or lo == 0
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return off[lo] <= x && x < off[lo + 1] ? lo : -1;
}

// what a song gives its lanes: tracks, ticks, first track, first cell; `ok` only if all its cells and tracks lie inside the totals
struct Song {
    int tracks, ticks, track0;
    long long cell0;
    bool ok;
    __device__ Song(const mvae_import_args& a, const Work& ws, int s) {
        track0 = a.track_off[s];
        tracks = a.track_off[s + 1] - track0;
        ticks = a.ticks[s];
        cell0 = ws.first[s];
        ok = track0 >= 0 && tracks >= 0 && (long long)track0 + tracks <= a.n_tracks && ticks >= 0 && cell0 >= 0 &&
             cell0 + (long long)tracks * ticks <= a.cells;
    }
    __device__ size_t cell(int track, int tick) const { return (size_t)(cell0 + (long long)track * ticks + tick); }
};

__global__ __launch_bounds__(SCAN_BLOCK) void import_plan_k(const mvae_import_args a) {
    __shared__ long long xs[SCAN_BLOCK];
    const Work ws(a);
    const int t = threadIdx.x;
    long long run = 0;
    for (int s0 = 0; s0 < a.n_songs; s0 += SCAN_BLOCK) {
        const int s = s0 + t;
        long long val = 0;
        if (s < a.n_songs) {
            const long long tracks = (long long)a.track_off[s + 1] - a.track_off[s], ticks = a.ticks[s];
            if (tracks > 0 && ticks > 0) val = tracks * ticks;
        }
        xs[t] = val;
        __syncthreads();
        for (int d = 1; d < SCAN_BLOCK; d <<= 1) {
            const long long add = t >= d ? xs[t - d] : 0;
            __syncthreads();
            xs[t] += add;
            __syncthreads();
        }
        // (a sum past the int32 the cells were promised to fit: the songs from there on fail Song::ok and yield silence)
        if (s < a.n_songs) ws.first[s] = (int)min(run + xs[t] - val, (long long)0x7fffffff);
        run += xs[SCAN_BLOCK - 1];
        __syncthreads();          // xs has been read
    }
    if (t == 0) ws.first[a.n_songs] = (int)min(run, (long long)0x7fffffff);
}

__global__ __launch_bounds__(BLOCK) void import_clear_k(const mvae_import_args a) {
    const Work ws(a);
    const size_t words = 9 * (size_t)a.cells, step = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < words; i += step) ws.pm[i] = 0u;          // (pm, km, count: one run)
}

// record i of the call: its song, and whether the kernels take it at all
struct Record {
    int s, start, end, pitch, velocity, track;
    bool ok;
    __device__ Record(const mvae_import_args& a, int i) {
        const int32_t* raw = reinterpret_cast<const int32_t*>(a.notes) + 3 * (size_t)i;
        start = raw[0];
        end = raw[1];
        const unsigned tail = (unsigned)raw[2];
        pitch = tail & 0xff;
        velocity = (tail >> 8) & 0xff;
        track = tail >> 16;
        s = owner(a.note_off, a.n_songs, i);
        ok = s >= 0 && pitch < MVAE_IMPORT_PITCHES;
    }
};

__global__ __launch_bounds__(BLOCK) void import_paint_k(const mvae_import_args a) {
    const Work ws(a);
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (at >= a.n_notes) return;
    const Record r(a, (int)at);
    if (!r.ok) return;
    const Song song(a, ws, r.s);
    if (!song.ok || r.track >= song.tracks) return;
    const unsigned bit = 1u << (r.pitch & 31);
    const int word = r.pitch >> 5;
    if (r.start >= 0 && r.start < song.ticks) atomicOr(&ws.km[4 * song.cell(r.track, r.start) + word], bit);
    const int hi = min(r.end, song.ticks);
    for (int tick = max(r.start, 0); tick < hi; ++tick) {
        const size_t c = song.cell(r.track, tick);
        atomicOr(&ws.pm[4 * c + word], bit);
        atomicAdd(&ws.count[c], 1);
    }
}

__global__ __launch_bounds__(BLOCK) void import_concurrent_k(const mvae_import_args a) {
    __shared__ int part[BLOCK];
    const Work ws(a);
    const int g = blockIdx.x, t = threadIdx.x;          // g < n_tracks: the grid
    const int s = owner(a.track_off, a.n_songs, g);
    int best = 0;
    if (s >= 0) {          // (uniform over the workgroup)
        const Song song(a, ws, s);
        if (song.ok)
            for (int tick = t; tick < song.ticks; tick += BLOCK) best = max(best, ws.count[song.cell(g - song.track0, tick)]);
    }
    part[t] = best;
    __syncthreads();
    for (int d = BLOCK / 2; d > 0; d >>= 1) {
        if (t < d) part[t] = max(part[t], part[t + d]);
        __syncthreads();
    }
    if (t == 0) a.concurrent[g] = part[0];
}

__global__ __launch_bounds__(BLOCK) void import_allot_k(const mvae_import_args a) {
    const Work ws(a);
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (at >= a.n_songs) return;
    const int s = (int)at, V = a.voices, M = a.max_per_track;
    const Song song(a, ws, s);
    const int tracks = song.ok ? song.tracks : 0;
    const int32_t* c = a.concurrent + song.track0;          // (read only below `tracks`)
    const int head = min(V, tracks);
    int free_voices = V;
    for (int k = 0; k < head; ++k) free_voices -= c[k] > 0 ? min(M, c[k]) : 0;
    int filled = 0;
    for (int k = 0; k < tracks && filled < V; ++k) {
        int cap = M;
        if (k < head && free_voices > 0 && c[k] > M) {
            const int add = min(free_voices, c[k] - M);
            cap += add;
            free_voices -= add;
        }
        if (c[k] <= 0) continue;
        const int give = min(c[k], cap);
        for (int voice = 0; voice < give && filled < V; ++voice, ++filled) {
            a.slots[(size_t)s * V + filled] = k;
            a.slot_voice[(size_t)s * V + filled] = voice;
        }
    }
    for (; filled < V; ++filled) {
        a.slots[(size_t)s * V + filled] = -1;
        a.slot_voice[(size_t)s * V + filled] = 0;
    }
}

// the (k+1)-th highest set bit of a 128-bit mask, or -1
__device__ __forceinline__ int kth_highest(const unsigned m[4], int k) {
    for (int w = 3; w >= 0; --w) {
        unsigned x = m[w];
        const int c = __popc(x);
        if (k >= c) {
            k -= c;
            continue;
        }
        for (; k > 0; --k) x &= ~(0x80000000u >> __clz(x));
        return 32 * w + 31 - __clz(x);
    }
    return -1;
}

__global__ __launch_bounds__(BLOCK) void import_rows_k(const mvae_import_args a) {
    const Work ws(a);
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x;          // < 2^31: the entry point
    if (at >= (long long)a.n_windows * a.T) return;
    const int w = (int)(at / a.T), t = (int)(at - (long long)w * a.T), V = a.voices;
    int idx = a.silent, held = 0;
    const int s = owner(a.win_off, a.n_songs, w);
    if (s >= 0) {
        const Song song(a, ws, s);
        const long long row = (long long)(w - a.win_off[s]) * a.T + t;
        const long long tick = row / V;
        const int slot = (int)(row - tick * V);
        const int track = a.slots[(size_t)s * V + slot], voice = a.slot_voice[(size_t)s * V + slot];
        if (song.ok && tick < song.ticks && track >= 0 && track < song.tracks && voice >= 0) {
            const size_t c = 4 * song.cell(track, (int)tick);
            const unsigned m[4] = {ws.pm[c], ws.pm[c + 1], ws.pm[c + 2], ws.pm[c + 3]};
            const int pitch = kth_highest(m, voice);
            if (pitch >= 0) {
                held = (ws.km[c + (pitch >> 5)] >> (pitch & 31)) & 1u ? 0 : 1;
                if (pitch >= a.pitch_base && pitch < a.pitch_base + a.n_pitch) idx = pitch - a.pitch_base;
            }
        }
    }
    const size_t out = (size_t)t * (size_t)a.stride_t + (size_t)w * (size_t)a.stride_w;
    a.idx[out] = (uint8_t)idx;
    a.held[out] = (uint8_t)held;
    if (a.vel_raw) a.vel_raw[out] = 0;
    if (a.vel) a.vel[out] = 0.0f;
}

__global__ __launch_bounds__(BLOCK) void import_velocity_k(const mvae_import_args a) {
    const Work ws(a);
    const long long at = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (at >= a.n_notes) return;
    const int i = (int)at, V = a.voices;
    const Record r(a, i);
    if (!r.ok) return;
    const Song song(a, ws, r.s);
    if (!song.ok || r.track >= song.tracks || r.start < 0 || r.start >= song.ticks) return;
    if (i + 1 < a.n_notes && i + 1 < a.note_off[r.s + 1]) {          // a later record of the same key gives the velocity
        const Record next(a, i + 1);
        if (next.track == r.track && next.start == r.start && next.pitch == r.pitch) return;
    }
    const size_t c = 4 * song.cell(r.track, r.start);
    const int word = r.pitch >> 5, b = r.pitch & 31;
    const unsigned own = ws.pm[c + word];
    if (!((own >> b) & 1u)) return;          // a key nothing paints: no row shows it
    int rank = b == 31 ? 0 : __popc(own >> (b + 1));
    for (int k = word + 1; k < 4; ++k) rank += __popc(ws.pm[c + k]);
    for (int slot = 0; slot < V; ++slot) {
        if (a.slots[(size_t)r.s * V + slot] != r.track || a.slot_voice[(size_t)r.s * V + slot] != rank) continue;
        const long long row = (long long)r.start * V + slot;
        const long long w = (long long)a.win_off[r.s] + row / a.T;
        if (w < 0 || w >= a.win_off[r.s + 1] || w >= a.n_windows) return;
        const size_t out = (size_t)(row % a.T) * (size_t)a.stride_t + (size_t)w * (size_t)a.stride_w;
        if (a.vel_raw) a.vel_raw[out] = (uint8_t)r.velocity;
        // the reference's expression (:273) in double, in its order, the product and the sum rounded separately
        if (a.vel && r.velocity > 0)
            a.vel[out] = (float)__dadd_rn(a.threshold, __dmul_rn((double)r.velocity / 127.0, 1.0 - a.threshold));
        return;
    }
}

}  // namespace

extern "C" int mvae_import_abi_version(void) { return 1; }

extern "C" int mvae_rolls_from_notes(const mvae_import_args* a, void* stream) {
    if (!a || !a->note_off || !a->track_off || !a->ticks || !a->win_off || !a->workspace) return MVAE_E_ARG;
    if (!a->idx || !a->held || !a->slots || !a->slot_voice) return MVAE_E_ARG;
    if (a->n_songs <= 0 || a->n_windows <= 0 || a->T <= 0 || a->max_per_track <= 0 || a->stride_t <= 0 || a->stride_w <= 0) return MVAE_E_ARG;
    if (a->n_notes < 0 || a->n_tracks < 0 || a->cells < 0 || (a->n_notes > 0 && !a->notes) || (a->n_tracks > 0 && !a->concurrent)) return MVAE_E_ARG;
    if (a->voices < 1 || a->voices > MAX_V || a->T % a->voices) return MVAE_E_ARG;
    if (a->pitch_base < 0 || a->n_pitch <= 0 || (long long)a->pitch_base + a->n_pitch > MVAE_IMPORT_PITCHES) return MVAE_E_ARG;
    if (a->silent < 0 || a->silent > 255 || !(a->threshold >= 0.0 && a->threshold < 1.0)) return MVAE_E_ARG;
    if (a->n_tracks > MVAE_IMPORT_MAX_TRACKS || (long long)a->n_windows * a->T > 0x7fffffffLL || a->cells > 0x7fffffffLL) return MVAE_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const auto blocks = [](long long lanes) { return dim3((unsigned)((lanes + BLOCK - 1) / BLOCK)); };
    hipLaunchKernelGGL(import_plan_k, dim3(1), dim3(SCAN_BLOCK), 0, s, *a);
    MVAE_CHECK_LAUNCH();
    if (a->cells > 0) {
        const long long want = (9 * (long long)a->cells + BLOCK - 1) / BLOCK;          // (a grid-stride loop: 65536 workgroups at most)
        hipLaunchKernelGGL(import_clear_k, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(BLOCK), 0, s, *a);
        MVAE_CHECK_LAUNCH();
    }
    if (a->n_notes > 0) {
        hipLaunchKernelGGL(import_paint_k, blocks(a->n_notes), dim3(BLOCK), 0, s, *a);
        MVAE_CHECK_LAUNCH();
    }
    if (a->n_tracks > 0) {
        hipLaunchKernelGGL(import_concurrent_k, dim3((unsigned)a->n_tracks), dim3(BLOCK), 0, s, *a);
        MVAE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(import_allot_k, blocks(a->n_songs), dim3(BLOCK), 0, s, *a);
    MVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(import_rows_k, blocks((long long)a->n_windows * a->T), dim3(BLOCK), 0, s, *a);
    MVAE_CHECK_LAUNCH();
    if (a->n_notes > 0) {
        hipLaunchKernelGGL(import_velocity_k, blocks(a->n_notes), dim3(BLOCK), 0, s, *a);
        MVAE_CHECK_LAUNCH();
    }
    return MVAE_OK;
}

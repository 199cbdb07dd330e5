// Window descriptors on the device: the 15-entry signature vector (reference data_class.py:96-215) and the voice-by-voice
// harmonicity (:25-88) of piano-roll windows, from the one-byte index per row that the staging and the fused decode leave in HBM.
// C ABI: include/midivae_descriptors.h.
//
// Both descriptors are serial automata over the ticks of a window with a few dozen bytes of state, so the mapping is ONE LANE PER
// WINDOW, one wave per workgroup, a loop over the ticks (any T: nothing is unrolled to a fixed count).  What a lane indexes
// dynamically - the held notes and their ages, the note sets of this and the previous tick, the voices' centroids - lives in LDS
// laid out [slot][lane]: lane l of a 4-byte array is on bank l % 32 of its 32-lane half whatever slot it is at (a row is 256 bytes),
// an 8-byte one on banks 2l, 2l + 1 of 64 - conflict-free - and nothing lands in scratch (the Makefile checks it).  The rest
// (counts, exact integer sums) stays in registers.
//
// Reading the rows: Rows of rolls.h, in chunks of CHUNK_TICKS ticks - straight from memory in a time-major (T, Bp) buffer, staged
// through LDS in any other layout, window-major (n, T) first of all.
//
// Arithmetic: counts, sums and sums of squares are integers (exact); max, min, mean and the ratios are one or two double divisions
// in the reference's order (sum / count) / scale and so bit-equal to NumPy's; std = sqrt((c * sum(x^2) - sum(x)^2) / c^2).
#include "rolls.h"

#include "../../include/midivae_descriptors.h"

namespace {

constexpr int MAXV = MVAE_DESC_MAX_VOICES;
constexpr int MAXHELD = 2 * MAXV;          // the held list keeps skipped notes: it settles below 2 * voices (see held update)
constexpr int CHUNK_TICKS = 16;
constexpr int MAX_T = 1 << 20, MAX_LOW_CROP = 1023;      // c * sum(x^2) stays inside int64
static_assert(MAXV == ROLL_MAX_VOICES, "rolls.h sizes its tiles for the headers' voice limit");

template <bool STAGED>
using DescRows = Rows<mvae_desc_args, STAGED, false, CHUNK_TICKS>;          // no velocity tile

template <bool STAGED>
__global__ __launch_bounds__(LANES) void desc_signature_k(const mvae_desc_args a) {
    __shared__ int held[MAXHELD][LANES], age[MAXHELD][LANES], cur[MAXV][LANES], prev[MAXV][LANES], dist[MAXV][LANES];
    __shared__ uint8_t tile[DescRows<STAGED>::TILE];
    const int l = threadIdx.x, V = a.voices, ticks = a.T / V;
    const bool live = blockIdx.x * LANES + l < a.n;
    DescRows<STAGED> rows(a, tile);
    Stats pitches, intervals, durations;
    int nheld = 0, nprev = 0, poly = 0;

    for (int tick0 = 0; tick0 < ticks; tick0 += CHUNK_TICKS) {
        const int nt = min(CHUNK_TICKS, ticks - tick0);
        rows.open(tick0, nt);
        if (!live) continue;
        for (int k = 0; k < nt; ++k) {
            // the note set of the tick: the distinct sounding indices of the voices, ascending (the k-hot fold)
            int nc = 0;
            for (int v = 0; v < V; ++v) {
                const int x = rows.idx(tick0, k * V + v);
                if (!roll_sounding(a.silent, a.n_pitch, x)) continue;
                int p = 0;
                while (p < nc && cur[p][l] < x) ++p;
                if (p < nc && cur[p][l] == x) continue;          // a pitch doubled across voices counts once
                for (int j = nc; j > p; --j) cur[j][l] = cur[j - 1][l];
                cur[p][l] = x;
                ++nc;
            }
            // held notes that ended: the reference deletes from the list it iterates, so the element after a deleted one is
            // skipped and stays held.  At most every second note leaves, at most V join: nheld <= V + nheld / 2 < 2 V.
            for (int i = 0; i < nheld; ++i) {
                const int h = held[i][l];
                bool in = false;
                for (int j = 0; j < nc; ++j) in = in || cur[j][l] == h;
                if (in) continue;
                durations.push(age[i][l]);
                --nheld;
                for (int j = i; j < nheld; ++j) {
                    held[j][l] = held[j + 1][l];
                    age[j][l] = age[j + 1][l];
                }
            }
            for (int j = 0; j < nc; ++j) {
                const int x = cur[j][l];
                pitches.push(x + a.low_crop);
                int i = 0;
                while (i < nheld && held[i][l] != x) ++i;
                if (i < nheld) {
                    ++age[i][l];
                } else if (nheld < MAXHELD) {
                    held[nheld][l] = x;
                    age[nheld][l] = 1;
                    ++nheld;
                }
            }
            // intervals to the previous non-silent tick
            if (nc == nprev) {
                for (int j = 0; j < nc; ++j) intervals.push(abs(cur[j][l] - prev[j][l]));
            } else if (nc != 0 && nprev != 0) {
                // of the longer set keep the len(shorter) notes nearest to the shorter one (ties: the earlier); both sets ascend,
                // so the kept notes are met in ascending order and pair off with the shorter set as they come
                const bool cur_longer = nc > nprev;
                int (*lng)[LANES] = cur_longer ? cur : prev;
                int (*sht)[LANES] = cur_longer ? prev : cur;
                const int nl = max(nc, nprev), ns = min(nc, nprev);
                for (int i = 0; i < nl; ++i) {
                    int d = 9999;
                    for (int j = 0; j < ns; ++j) d = min(d, abs(lng[i][l] - sht[j][l]));
                    dist[i][l] = d;
                }
                int taken = 0;
                for (int i = 0; i < nl; ++i) {
                    const int d = dist[i][l];
                    int rank = 0;
                    for (int j = 0; j < nl; ++j) rank += (dist[j][l] < d || (dist[j][l] == d && j < i)) ? 1 : 0;
                    if (rank < ns) intervals.push(abs(lng[i][l] - sht[taken++][l]));
                }
            }
            poly += nc > 1 ? 1 : 0;
            if (nc > 0) {
                for (int j = 0; j < nc; ++j) prev[j][l] = cur[j][l];
                nprev = nc;
            } else {          // silence ends every held note; the previous note set stays
                for (int i = 0; i < nheld; ++i) durations.push(age[i][l]);
                nheld = 0;
            }
        }
    }
    if (!live) return;
    double* out = a.sig_out + (size_t)(blockIdx.x * LANES + l) * a.ld_sig;
    out[0] = (double)durations.c / (double)ticks;          // (notes still held at the window's end are not counted)
    out[1] = (double)pitches.c / (double)ticks;
    out[2] = (double)poly / (double)ticks;
    pitches.store_scaled(out + 3, 127.0);
    intervals.store_scaled(out + 7, 127.0);
    durations.store_scaled(out + 11, 1.0);
}

template <bool STAGED>
__global__ __launch_bounds__(LANES) void desc_harmonicity_k(const mvae_desc_args a) {
    constexpr int PAIRS = MAXV * (MAXV - 1) / 2;
    __shared__ double cent[MAXV * 6][LANES], psum[PAIRS][LANES], tonal[72];
    __shared__ int cnt[MAXV][LANES], pcnt[PAIRS][LANES];
    __shared__ uint8_t tile[DescRows<STAGED>::TILE];
    const int l = threadIdx.x, V = a.voices, ticks = a.T / V, res = a.resolution;
    const int used = ticks / res * res, per = a.n_pitch / 12, pairs = V * (V - 1) / 2;
    const bool live = blockIdx.x * LANES + l < a.n;
    DescRows<STAGED> rows(a, tile);
    for (int i = l; i < 72; i += LANES) tonal[i] = (double)a.tonal[i];
    for (int p = 0; p < pairs; ++p) {
        psum[p][l] = 0.0;
        pcnt[p][l] = 0;
    }
    __syncthreads();

    int in_seg = 0;
    for (int tick0 = 0; tick0 < used; tick0 += CHUNK_TICKS) {
        const int nt = min(CHUNK_TICKS, used - tick0);
        rows.open(tick0, nt);
        if (!live) continue;
        for (int k = 0; k < nt; ++k) {
            if (in_seg == 0)
                for (int v = 0; v < V; ++v) {
                    cnt[v][l] = 0;
                    for (int j = 0; j < 6; ++j) cent[v * 6 + j][l] = 0.0;
                }
            // a voice's chroma over the segment, times the tonal matrix: the sum of the columns of its sounding ticks
            for (int v = 0; v < V; ++v) {
                const int x = rows.idx(tick0, k * V + v);
                if (!roll_sounding(a.silent, a.n_pitch, x)) continue;
                const int bin = x / per;
                ++cnt[v][l];
                for (int j = 0; j < 6; ++j) cent[v * 6 + j][l] += tonal[j * 12 + bin];
            }
            if (++in_seg < res) continue;
            in_seg = 0;
            for (int v = 0; v < V; ++v) {
                const int c = cnt[v][l];
                if (c > 0)
                    for (int j = 0; j < 6; ++j) cent[v * 6 + j][l] /= (double)c;
            }
            for (int v1 = 1, p = 0; v1 < V; ++v1)
                for (int v2 = 0; v2 < v1; ++v2, ++p) {
                    if (cnt[v1][l] == 0 || cnt[v2][l] == 0) continue;          // the segment's distance is NaN: left out of the mean
                    double ss = 0.0;
                    for (int j = 0; j < 6; ++j) {
                        const double d = cent[v1 * 6 + j][l] - cent[v2 * 6 + j][l];
                        ss += d * d;
                    }
                    psum[p][l] += sqrt(ss);
                    ++pcnt[p][l];
                }
        }
    }
    if (!live) return;
    double* out = a.harm_out + (size_t)(blockIdx.x * LANES + l) * V * V;
    for (int v = 0; v < V; ++v) out[v * V + v] = 0.0;
    for (int v1 = 1, p = 0; v1 < V; ++v1)
        for (int v2 = 0; v2 < v1; ++v2, ++p) {
            const int c = pcnt[p][l];
            const double m = c > 0 ? psum[p][l] / (double)c : __builtin_nan("");
            out[v1 * V + v2] = m;
            out[v2 * V + v1] = m;
        }
}

}  // namespace

extern "C" int mvae_desc_abi_version(void) { return 1; }

extern "C" int mvae_desc_windows(const mvae_desc_args* a, void* stream) {
    if (roll_args_refused(a) || (!a->sig_out && !a->harm_out)) return MVAE_E_ARG;
    if (a->resolution <= 0 || a->low_crop < 0) return MVAE_E_ARG;
    if (a->sig_out && a->ld_sig < MVAE_DESC_SIGNATURE_LENGTH) return MVAE_E_ARG;
    if (a->harm_out && (!a->tonal || a->n_pitch % 12)) return MVAE_E_ARG;
    if (a->n_pitch > MVAE_DESC_MAX_PITCH || a->T > MAX_T || a->low_crop > MAX_LOW_CROP) return MVAE_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((a->n + LANES - 1) / LANES), block(LANES);
    const bool staged = a->stride_w != 1;
    if (a->sig_out) {
        if (staged)
            hipLaunchKernelGGL(desc_signature_k<true>, grid, block, 0, s, *a);
        else
            hipLaunchKernelGGL(desc_signature_k<false>, grid, block, 0, s, *a);
        MVAE_CHECK_LAUNCH();
    }
    if (a->harm_out) {
        if (staged)
            hipLaunchKernelGGL(desc_harmonicity_k<true>, grid, block, 0, s, *a);
        else
            hipLaunchKernelGGL(desc_harmonicity_k<false>, grid, block, 0, s, *a);
        MVAE_CHECK_LAUNCH();
    }
    return MVAE_OK;
}

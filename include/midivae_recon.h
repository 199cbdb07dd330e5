/* midivae_recon.h - song-level decode of libmidivae_hip.so: the velocity post-rules carried across the windows of a song (reference
 * vae_definition.py:1156-1190, run over a whole song), the note starts (the reference's D) and the counts of the reconstruction
 * report (vae_evaluation.py:2211-2236 and :2380-2397), from the one-byte index, the float velocity and the held-notes index per row
 * that a decode leaves on the device.
 *
 * A fourth header of the same library; the conventions are those of midivae_sweep.h (this file includes midivae_hip.h for MVAE_E_*):
 *   - pointers are DEVICE pointers, `stream` is a hipStream_t; nothing allocates, nothing synchronises;
 *   - return value: 0 = enqueued, negative = rejected, nothing enqueued.  Every limit below is checked before the first launch:
 *     MVAE_E_ARG for a NULL `a` or a NULL idx, all three outputs NULL, an extent (n, T, n_pitch) or a stride <= 0 (the strides of
 *     orig only with orig), voices outside 2..8, T % voices != 0, ld_counts < 8 (with counts_out), silent outside -1..255,
 *     override_rules outside 0..1, a threshold that is not finite, a NULL carry when vel, override_rules and first_window are all
 *     given; MVAE_E_UNSUPPORTED for n_pitch > 192 or T > 65536 = MVAE_RECON_MAX_T; MVAE_E_LAUNCH if HIP refuses a launch.
 *   - versioned on its own: mvae_recon_abi_version(); the other three versions do not move with this file.
 *
 * Semantics.  Row t of a window belongs to voice t % voices of tick t / voices.  An index SOUNDS unless it equals `silent`, is 255,
 * or is >= n_pitch (as in midivae_sweep.h).  The windows first_window[w] .. w are the song of window w so far; the windows of a song
 * are contiguous and first_window[w] <= w (a value outside 0..w is read as the nearer end of that range).  first_window == NULL:
 * every window is a song of its own, and vel_out is what mvae_sweep_windows writes for the same inputs.
 *   Velocity.  v0 of a row = the float32 of `vel` widened to double, 0 on a row that does not sound.  With override_rules, per voice
 *   over the rows of the SONG: previous_pitch = the index of the voice's previous row if that row sounds, else -1, and -1 at the
 *   song's first tick; previous_velocity = v0 of the nearest earlier row of the voice for which `v0 < threshold` is false, 0.0 if
 *   there is none.  The result is previous_velocity if v0 < threshold, the row sounds, previous_pitch > 0 (not >= 0) and
 *   previous_pitch differs from the row's index; 0 if v0 < threshold is false and the row does not sound; v0 otherwise.  With
 *   vel == NULL every row's velocity is threshold + (1 - threshold) * 0.5, nothing is zeroed and no rule runs.
 *   Note starts.  start_out is the held index where `held` is given; else, with vel, 0 where the velocity after the rules is
 *   > threshold and 1 elsewhere; with neither, 1 everywhere.
 *   counts_out[w][0..7] (columns [8, ld_counts) are not touched), over the T rows of window w:
 *      0  original rows that sound                 4  column 1 - column 2 (new)
 *      1  predicted rows that sound                5  note starts (start == 0)
 *      2  rows where both sound, the same index    6  note starts on a row whose prediction does not sound
 *      3  column 0 - column 2 (not predicted)      7  note starts on a row whose original does not sound
 *   With orig == NULL columns 0, 2, 3 and 7 are 0.
 *   carry: workspace of n * voices * 8 bytes (8-byte aligned), read and written only when vel, override_rules and first_window are
 *   all given.  Three launches at most, ordered by the stream; no workgroup waits for another.
 */
#ifndef MIDIVAE_RECON_H
#define MIDIVAE_RECON_H

#include "midivae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MVAE_RECON_COUNTS = 8, MVAE_RECON_MAX_VOICES = 8, MVAE_RECON_MAX_PITCH = 192, MVAE_RECON_MAX_T = 65536 };

typedef struct {
    const uint8_t* idx;          /* the decoded index of row t of window w is idx[t * stride_t + w * stride_w]                    */
    int64_t stride_t;            /* > 0, in elements, shared by idx, vel and held.  Time-major (T, Bp) buffers: stride_t = Bp,     */
    int64_t stride_w;            /* > 0.  stride_w = 1; window-major (n, T): stride_t = 1, stride_w = T                           */
    const float* vel;            /* the velocity head's value at the same offset, or NULL                                         */
    const uint8_t* held;         /* the held-notes head's index at the same offset, or NULL                                       */
    const uint8_t* orig;         /* the original target index of the row at orig[t * orig_stride_t + w * orig_stride_w], 255 = no  */
    int64_t orig_stride_t;       /* target; or NULL (the strides are then not read)                                               */
    int64_t orig_stride_w;
    const int32_t* first_window; /* n values, or NULL: every window is its own song                                               */
    int32_t n;                   /* windows, > 0                                                                                  */
    int32_t T;                   /* rows per window, 1..65536, a multiple of voices                                               */
    int32_t voices;              /* 2..8                                                                                          */
    int32_t silent;              /* the index that means "no note", or -1 for none                                                */
    int32_t n_pitch;             /* 1..192 pitch columns                                                                          */
    int32_t override_rules;      /* 0 or 1: run the per-voice velocity rule                                                       */
    double threshold;            /* finite: a velocity > threshold starts a note, one < threshold is silent                       */
    void* carry;                 /* n * voices * 8 bytes of workspace, see above                                                  */
    float* vel_out;              /* (n, T) window-major velocities after the rules, or NULL                                       */
    uint8_t* start_out;          /* (n, T) window-major, 0 = a note starts on the row, or NULL                                    */
    int32_t* counts_out;         /* (n, ld_counts), columns 0..7 written, or NULL; at least one output is given                   */
    int32_t ld_counts;           /* >= 8 with counts_out                                                                          */
    int32_t reserved;            /* not read                                                                                      */
} mvae_recon_args;

int mvae_recon_abi_version(void); /* 1 */
int mvae_recon_songs(const mvae_recon_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIDIVAE_RECON_H */

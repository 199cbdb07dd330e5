/* midivae_sweep.h - latent-sweep statistics of libmidivae_hip.so: per-window pitch, velocity and note-start statistics and the
 * velocity post-rules of a decoded window (reference vae_evaluation.py:1018-1096 on top of vae_definition.py:1153-1190), computed
 * from the one-byte index per row and the float velocity per row that a decode leaves on the device.
 *
 * A third header of the same library; the conventions are those of midivae_hip.h (which this file includes for MVAE_E_*):
 *   - pointers are DEVICE pointers, `stream` is a hipStream_t; nothing allocates, nothing synchronises;
 *   - return value: 0 = enqueued, negative = rejected, nothing enqueued.  Every limit below is checked before the first launch:
 *     MVAE_E_ARG for a NULL `a` or a NULL idx, both outputs NULL, an extent (n, T, n_pitch) or stride <= 0, voices outside 2..8,
 *     T % voices != 0, ld_out < 22 (with stats_out), silent outside -1..255, count_a or count_b outside 0..255, override_rules
 *     outside 0..1, a threshold that is not finite; MVAE_E_UNSUPPORTED for n_pitch > 192 or T > 65536 = MVAE_SWEEP_MAX_T (the
 *     per-lane pitch histogram counts ticks in 16 bits, the integer sums of the row positions stay inside int64);
 *     MVAE_E_LAUNCH if HIP refuses the launch.
 *   - versioned on its own: mvae_sweep_abi_version(); mvae_abi_version() and mvae_desc_abi_version() do not move with this file.
 *
 * Semantics.  Row t of a window belongs to voice t % voices of tick t / voices.  An index is a sounding note unless it equals
 * `silent`, is 255, or is >= n_pitch.  Windows are independent.
 *   Velocity of a row: the float32 of `vel` widened to double; 0 on a row that does not sound; with override_rules, per voice and
 *   starting every window from previous_pitch = -1, previous_velocity = 0: "velocity is silent" means velocity < threshold; a
 *   silent velocity on a sounding row whose voice's previous pitch is > 0 (not >= 0) and differs from this pitch becomes the
 *   previous velocity; a velocity that is not silent on a row that does not sound becomes 0; then previous_pitch = pitch (-1 for
 *   none) and, if the velocity was not silent, previous_velocity = the velocity before the rule.  With vel == NULL every row's
 *   velocity is default_velocity, nothing is zeroed and no rule runs.  vel_out[w][t] receives the result as float32.
 *   stats_out[w][0..21] (columns [22, ld_out) are not touched); every group is count, mean, median, min, max, range, std:
 *      0..6   the pitch list: the distinct sounding indices of every tick, as column indices (nothing is added to them);
 *      7, 8   the number of ticks in which column count_a, respectively count_b, sounds;
 *      9..15  the velocities of the note starts: the rows whose velocity after the rules is > threshold;
 *      16..21 mean, median, min, max, range, std of the note starts' row positions 0..T-1 (their count is column 9).
 *   An empty list has count 0 and NaN statistics.  Pitch and position statistics come from exact integer sums: the mean is one
 *   double division, std = sqrt((c * sum(x^2) - sum(x)^2) / c^2).  Medians follow np.median: the middle element, or (a + b) / 2
 *   of the two middle ones.  Velocities are summed in double in row order; their std is the two-pass form.
 */
#ifndef MIDIVAE_SWEEP_H
#define MIDIVAE_SWEEP_H

#include "midivae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MVAE_SWEEP_COLUMNS = 22, MVAE_SWEEP_MAX_VOICES = 8, MVAE_SWEEP_MAX_PITCH = 192, MVAE_SWEEP_MAX_T = 65536 };

typedef struct {
    const uint8_t* idx;       /* the index of row t of window w is idx[t * stride_t + w * stride_w]                            */
    int64_t stride_t;         /* > 0, in elements, shared by idx and vel.  Time-major (T, Bp) buffers: stride_t = Bp,           */
    int64_t stride_w;         /* > 0.  stride_w = 1 (read directly); window-major (n, T): stride_t = 1, stride_w = T (staged)   */
    const float* vel;         /* the velocity head's value of row t of window w at the same offset, or NULL                     */
    int32_t n;                /* windows, > 0                                                                                  */
    int32_t T;                /* rows per window, 1..65536, a multiple of voices                                                */
    int32_t voices;           /* 2..8                                                                                          */
    int32_t silent;           /* the index that means "no note", or -1 for none (255 and indices >= n_pitch are silent too)    */
    int32_t n_pitch;          /* 1..192 pitch columns                                                                          */
    int32_t count_a;          /* 0..255: the two columns whose ticks are counted (the reference counts 35 and 39)              */
    int32_t count_b;
    int32_t override_rules;   /* 0 or 1: run the per-voice velocity rule                                                       */
    double threshold;         /* finite: a velocity > threshold starts a note, one < threshold is silent                       */
    double default_velocity;  /* every row's velocity when vel is NULL                                                         */
    int32_t ld_out;           /* >= 22 with stats_out, doubles between two rows of stats_out                                   */
    int32_t reserved;         /* not read                                                                                      */
    double* stats_out;        /* (n, ld_out), columns 0..21 written, or NULL                                                   */
    float* vel_out;           /* (n, T) window-major velocities after the rules, or NULL; at least one output is given         */
} mvae_sweep_args;

int mvae_sweep_abi_version(void); /* 1 */
int mvae_sweep_windows(const mvae_sweep_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIDIVAE_SWEEP_H */

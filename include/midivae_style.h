/* midivae_style.h - style-transfer scoring of libmidivae_hip.so: the pitch, velocity and instrument style judges and their weighted
 * ensemble over the windows of songs (reference vae_evaluation.py:110-117, :2075-2172, :2248-2340, :2448-2604), from the
 * probability tables the three classifiers leave on the device.
 *
 * A seventh header of the same library; the conventions are those of midivae_sweep.h (this file includes midivae_hip.h for MVAE_E_*):
 *   - pointers are DEVICE pointers, `stream` is a hipStream_t; nothing allocates, nothing synchronises;
 *   - return value: 0 = enqueued, negative = rejected, nothing enqueued.  Every limit below is checked before the first launch:
 *     MVAE_E_ARG for a NULL `a`, all three tables NULL, all four outputs NULL, ens_out given while a table is missing, n <= 0 or
 *     n_groups <= 0, a NULL cls or group_off, the ld of a given table or of ens_out < C, ld_table < 9 (with table_out),
 *     n_instr_rows <= 0 (with p_instr), a weight that is not finite, a weight sum that is not > 0;
 *     MVAE_E_UNSUPPORTED for C outside 2..64; MVAE_E_LAUNCH if HIP refuses the launch.
 *   - versioned on its own: mvae_style_abi_version(); mvae_abi_version() and the other side headers' versions do not move with it.
 *
 * Semantics.  Window w is judged by row w of p_pitch and of p_vel and by row r(w) of p_instr, r(w) = instr_row[w], or w when
 * instr_row is NULL.  A NULL table is an absent judge.  r(w) outside [0, n_instr_rows) is never read: the window's instrument and
 * ensemble judges then have no argmax (255), its ens_out row is NaN, it adds NaN to the two confidences and a miss to the two
 * accuracies of its group, and it is left out of their confusion counts.
 *   Ensemble (only when all three tables are given), in float32, every operation rounded on its own - no fused multiply-add, a
 *   correctly rounded division - which is what NumPy does to float32 arrays with Python-float weights:
 *       wp = (float)weights[0], wi = (float)weights[1], wv = (float)weights[2], den = (float)(weights[0] + weights[1] + weights[2])
 *       e[c] = ((p_pitch[c] * wp + p_instr[c] * wi) + p_vel[c] * wv) / den
 *   weights are in the order pitch, instrument, velocity.
 *   Argmax follows np.argmax: the first maximum wins, the first NaN wins.
 *   Groups.  Group g holds the windows group_off[g] .. group_off[g + 1] - 1 (a song, or a (song, target class) pair); group_off
 *   ascends from 0 to n, empty groups are allowed.  group_off lives on the device and cannot be validated before the launch: the
 *   kernel clamps both ends of every group to [0, n] and treats a descending pair as empty.  ens_out and pred_out are written for
 *   the windows some group holds (all of them when group_off is as described).  A window is COUNTED in its group unless cls[w] is
 *   255 or >= C (its row of ens_out and pred_out is written all the same).
 *   table_out[g][0..8] (columns [9, ld_table) are not touched): [0] the number of counted windows, then accuracy and confidence of
 *   the pitch [1, 2], velocity [3, 4], instrument [5, 6] and ensemble [7, 8] judges.  Accuracy: the number of counted windows whose
 *   argmax equals cls[w], an exact integer, divided once by [0] in double.  Confidence: the judge's float32 probability of class
 *   cls[w], widened to double, summed over the counted windows and divided once by [0].  An absent judge and an empty group: NaN.
 *   confusion_out[judge][cls[w]][argmax] (4 x C x C int32, judges in the order of pred_out, zeroed by the caller) is incremented
 *   with integer atomics for every counted window and every judge that has an argmax: exact, whatever the order.
 *
 * Order of the sums (the bound of the confidence means in tests/test_style_scores_gpu.py is derived from it).  One workgroup of 256
 * lanes per group.  Lane l adds the windows first + l, first + l + 256, .. of its group in ascending order into a double partial sum
 * that starts from 0; the 256 partial sums are reduced in LDS by the fixed binary tree  for (s = 128; s > 0; s /= 2) if (l < s)
 * sum[l] += sum[l + s].  No workgroup waits for another.
 */
#ifndef MIDIVAE_STYLE_H
#define MIDIVAE_STYLE_H

#include "midivae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MVAE_STYLE_COLUMNS = 9, MVAE_STYLE_JUDGES = 4, MVAE_STYLE_MIN_CLASSES = 2, MVAE_STYLE_MAX_CLASSES = 64, MVAE_STYLE_LANES = 256 };

typedef struct {
    const float* p_pitch;     /* (n, ld_pitch) probabilities of the pitch judge, or NULL                                         */
    const float* p_vel;       /* (n, ld_vel) of the velocity judge, or NULL                                                      */
    const float* p_instr;     /* (n_instr_rows, ld_instr) of the instrument judge, or NULL                                       */
    const int32_t* instr_row; /* (n) the row of p_instr that judges window w, or NULL for row w                                  */
    const uint8_t* cls;       /* (n) the class a window is scored against; 255 (or >= C): not counted                            */
    const int32_t* group_off; /* (n_groups + 1) ascending from 0 to n                                                            */
    int32_t n;                /* windows, > 0                                                                                    */
    int32_t C;                /* classes, 2..64                                                                                  */
    int32_t n_groups;         /* > 0                                                                                             */
    int32_t n_instr_rows;     /* > 0 with p_instr                                                                                */
    int32_t ld_pitch;         /* floats between two rows, >= C for a table that is given                                         */
    int32_t ld_vel;
    int32_t ld_instr;
    int32_t ld_ens;           /* >= C with ens_out                                                                               */
    int32_t ld_table;         /* >= 9 with table_out, doubles between two rows of table_out                                      */
    int32_t reserved;         /* not read                                                                                        */
    double weights[3];        /* pitch, instrument, velocity: finite, their sum > 0                                              */
    float* ens_out;           /* (n, ld_ens), columns 0..C-1 written, or NULL; needs all three tables                            */
    uint8_t* pred_out;        /* (n, 4) argmax of the pitch, velocity, instrument and ensemble judges, 255 = none, or NULL       */
    double* table_out;        /* (n_groups, ld_table), columns 0..8 written, or NULL                                             */
    int32_t* confusion_out;   /* (4, C, C) counts added to what the caller left there, or NULL; at least one output is given     */
} mvae_style_args;

int mvae_style_abi_version(void); /* 1 */
int mvae_style_scores(const mvae_style_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIDIVAE_STYLE_H */

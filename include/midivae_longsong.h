/* midivae_longsong.h - long songs of libmidivae_hip.so: the reference's long-song generator (vae_evaluation.py:1821-1896) walks from
 * a random code towards the nearest training code it has not picked yet, decodes a window, turns the window back into encoder input and
 * encodes it - the next code.  Two entry points keep that loop on the device: the search and pull of one iteration for S songs at once,
 * and the decoded batch as the encoder's next input.
 *
 * A ninth header of the same library; the conventions are those of midivae_generate.h (this file includes midivae_hip.h for MVAE_E_*):
 *   - pointers are DEVICE pointers, `stream` is a hipStream_t; nothing allocates, nothing synchronises;
 *   - return value: 0 = enqueued, negative = rejected, nothing enqueued.  Every limit below is checked before the first launch;
 *     MVAE_E_LAUNCH if HIP refuses a launch;
 *   - versioned on its own: mvae_longsong_abi_version(); mvae_abi_version() and the other side headers' versions do not move with it.
 *
 * mvae_nearest_walk.  all_z is (N, ld_all) float32, r_in (S, ld_r) float32 (r_f64 = 0) or double (1), picked (S, cap) int32 of which
 * the first n_picked entries of every row are valid (the songs run in lockstep).
 *   Search (:1847-1853).  For song s and row i, d2(i) = sum_j ((double)all_z[i][j] - (double)r_in[s][j])^2: the difference, its square and
 *   the sum are doubles, each rounded on its own (no fused multiply-add), added in ascending j from 0.0 by ONE lane - the value does not
 *   depend on N, S or how the launch is cut.  The CANDIDATES of song s are index 0 - always, even when it has been picked before: the
 *   reference's loop starts from it - and every i that is not among picked[s][0 .. n_picked-1].  The winner is the smallest index among
 *   the candidates whose d2 is minimal (the reference compares strictly: an equal later distance never replaces an earlier one).
 *   NaN: a candidate whose d2 is NaN never wins against another one, and if d2(0) is NaN the winner is index 0 and dist_out NaN (nothing
 *   compares below a NaN, so the reference's loop never leaves index 0).  Infinite distances compare as numbers.
 *   Outputs.  picked[s][n_picked] = winner; best_out[s] = winner; dist_out[s] = sqrt(d2(winner)), a double.
 *   Pull (:1862), R' = (R + z_w * e) / den with z_w = all_z[winner]; every operation rounded on its own, no fused multiply-add:
 *       r_f64 == 0:  fl32(fl32(r + fl32(z_w * (float)e)) / (float)den)                     r_out = z_out = that float
 *       r_f64 == 1:  fl64(fl64(r + (double)fl32(z_w * (float)e)) / den)                    r_out = that double, z_out = its float32 cast
 *   which is NumPy's `(R + closest_z * e) / (1 + e)` for a float32 all_z and an np.float32 e on a float64 R (np.random.normal) or a
 *   float32 R (encoder.predict).  The value of `1 + e` depends on NumPy's promotion rules, so the HOST passes den as it forms it.
 *   Row s of z_out (ld_z floats between rows) and of r_out (ld_rout elements of r_in's type) get columns 0..Z-1, the rest is not touched.
 *   z_out and r_out may alias r_in (a lane reads an element before it writes it).  Unless hist_out is NULL, row s of hist_out gets the
 *   float32 cast of row s of hist_in (float32 with hist_f64 = 0, double with 1; ld_hist_in elements between rows) - zeros where hist_in
 *   is NULL: the decoder's history, the r_out of the iteration before.
 *   workspace: mvae_nearest_walk_workspace(N, S, Z) bytes, 8-byte aligned (0 for extents <= 0):
 *       S * ceil(N / 256) * 16 + S * 8.
 *   Two launches.  The first leaves per (song, chunk of MVAE_WALK_ROW_CHUNK = 256 rows) the minimal (d2, index) among the chunk's
 *   candidates in the workspace - a workgroup holds the codes of MVAE_WALK_SONG_GROUP = 8 songs in LDS and reads its rows of all_z ONCE
 *   for all of them.  The second runs one workgroup per song: the reduction over the chunks, the append to picked, the pull, the stores.
 *   The order between them is the stream's; no workgroup waits for another.
 *   Refusals.  MVAE_E_ARG: a NULL `a`, all_z, r_in, picked, workspace, best_out, dist_out, z_out or r_out; N, S, Z or cap <= 0;
 *   ld_all, ld_r, ld_z or ld_rout < Z; ld_hist < Z with hist_out; ld_hist_in < Z with hist_out and hist_in; n_picked < 0 or
 *   n_picked >= cap; r_f64 or hist_f64 outside 0..1; an e that is not finite; a den that is not finite or is 0.
 *   MVAE_E_UNSUPPORTED: Z > 4096 = MVAE_WALK_MAX_Z.
 *
 * mvae_feedback_rows.  process_decoder_outputs (vae_definition.py:1131-1225) of ONE window per call, :1878-1887 and
 * prepare_encoder_input_list (:770-808) on the wire formats.  idx, stride_t, stride_w, vel, n, T, voices, silent, n_pitch, threshold and
 * override_rules are named and read exactly as in mvae_recon_args, held_idx as its `held`: row t of window w is voice t % voices of tick
 * t / voices and lies at idx[t * stride_t + w * stride_w], vel and held_idx at the same offset; an index SOUNDS unless it equals
 * `silent`, is 255, or is >= n_pitch.  instr holds the instrument byte of voice v of window w at instr[v * instr_stride_v +
 * w * instr_stride_w] (NULL allowed).  The outputs are TIME-MAJOR with ld_out >= n elements between rows; NULL: not written.
 *   x_out (T, ld_out) uint8      the index byte unchanged (a silent row keeps the silent index: the reference appends a silent column
 *                                and sets it where the row is empty);
 *   x_rev_out (T, ld_out) uint8  the same with the rows in reverse order: row T-1-t holds row t (the bidirectional encoder);
 *   vel_out (T, ld_out) float32  the velocity of mvae_recon_args with first_window == NULL: 0 on a row that does not sound; with
 *                                override_rules the per-voice rule, RESTARTED IN EVERY WINDOW (previous_pitch -1, previous_velocity 0 at
 *                                the window's first tick); with vel == NULL threshold + (1 - threshold) * 0.5 on every row;
 *   held_out (T, ld_out) uint8   1 = held: held_idx's byte where it is given; else, with vel, 1 unless the velocity after the rule,
 *                                widened to double, is > threshold (:1214-1221); with neither, 1;
 *   instr_out (voices, ld_out)   a copy of the instrument bytes (not written without instr).
 *   Columns n .. ld_out-1 of every output are written too, with 0 - what the engine's host staging puts into the padding windows.
 *   One launch, one lane per (window, voice) as mvae_recon_songs; no workgroup waits for another.
 *   Refusals.  MVAE_E_ARG: a NULL `a` or idx; all five outputs NULL; an extent (n, T, n_pitch) or a stride <= 0 (the strides of instr
 *   only with instr); voices outside 2..8; T % voices != 0; silent outside -1..255; override_rules outside 0..1; a threshold that is not
 *   finite; ld_out < n.  MVAE_E_UNSUPPORTED: T > 65536 = MVAE_FEEDBACK_MAX_T.
 */
#ifndef MIDIVAE_LONGSONG_H
#define MIDIVAE_LONGSONG_H

#include <stddef.h>

#include "midivae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MVAE_WALK_MAX_Z = 4096, MVAE_WALK_ROW_CHUNK = 256, MVAE_WALK_SONG_GROUP = 8, MVAE_FEEDBACK_MAX_VOICES = 8, MVAE_FEEDBACK_MAX_T = 65536 };

typedef struct {
    const float* all_z;          /* (N, ld_all) the training codes                                                                */
    const void* r_in;            /* (S, ld_r) float32 (r_f64 = 0) or double (1): the songs' current codes                         */
    const void* hist_in;         /* (S, ld_hist_in) float32 (hist_f64 = 0) or double (1), or NULL: zeros                          */
    int32_t* picked;             /* (S, cap): entries 0..n_picked-1 of every row are read, entry n_picked is written              */
    void* workspace;             /* mvae_nearest_walk_workspace(N, S, Z) bytes, 8-byte aligned                                    */
    int32_t N;                   /* training codes, > 0                                                                           */
    int32_t S;                   /* songs, > 0                                                                                    */
    int32_t Z;                   /* latent columns, 1..4096                                                                       */
    int32_t ld_all;              /* floats between two rows of all_z, >= Z                                                        */
    int32_t ld_r;                /* elements between two rows of r_in, >= Z                                                       */
    int32_t r_f64;               /* 0 or 1                                                                                        */
    int32_t ld_hist_in;          /* elements between two rows of hist_in, >= Z with hist_in and hist_out                          */
    int32_t hist_f64;            /* 0 or 1                                                                                        */
    int32_t cap;                 /* int32s between two rows of picked, > n_picked                                                 */
    int32_t n_picked;            /* >= 0: the iteration                                                                           */
    int32_t ld_z;                /* floats between two rows of z_out, >= Z                                                        */
    int32_t ld_rout;             /* elements between two rows of r_out, >= Z                                                      */
    int32_t ld_hist;             /* floats between two rows of hist_out, >= Z with hist_out                                       */
    int32_t reserved;            /* not read                                                                                      */
    double e;                    /* finite: the pull's weight, the reference's z_std_train                                        */
    double den;                  /* finite, not 0: 1 + e as the host's NumPy forms it                                             */
    int32_t* best_out;           /* (S) the winning index                                                                         */
    double* dist_out;            /* (S) its distance                                                                              */
    float* z_out;                /* (S, ld_z), columns 0..Z-1 written: the pulled code as the decoder reads it                    */
    void* r_out;                 /* (S, ld_rout) of r_in's type, columns 0..Z-1 written: the pulled code, unrounded               */
    float* hist_out;             /* (S, ld_hist), columns 0..Z-1 written, or NULL                                                 */
} mvae_walk_args;

typedef struct {
    const uint8_t* idx;          /* the decoded index of row t of window w is idx[t * stride_t + w * stride_w]                    */
    int64_t stride_t;            /* > 0, in elements, shared by idx, vel and held_idx                                             */
    int64_t stride_w;            /* > 0                                                                                           */
    const float* vel;            /* the velocity head's value at the same offset, or NULL                                         */
    const uint8_t* held_idx;     /* the held-notes head's index at the same offset, or NULL                                       */
    const uint8_t* instr;        /* the instrument byte of voice v of window w is instr[v * instr_stride_v + w * instr_stride_w],  */
    int64_t instr_stride_v;      /* or NULL (the strides are then not read)                                                       */
    int64_t instr_stride_w;
    int32_t n;                   /* windows, > 0                                                                                  */
    int32_t T;                   /* rows per window, 1..65536, a multiple of voices                                               */
    int32_t voices;              /* 2..8                                                                                          */
    int32_t silent;              /* the index that means "no note", or -1 for none                                                */
    int32_t n_pitch;             /* > 0 pitch columns                                                                             */
    int32_t override_rules;      /* 0 or 1: run the per-voice velocity rule, restarted in every window                            */
    double threshold;            /* finite                                                                                        */
    int32_t ld_out;              /* elements between two rows of every output, >= n                                               */
    int32_t reserved;            /* not read                                                                                      */
    uint8_t* x_out;              /* (T, ld_out) or NULL                                                                           */
    uint8_t* x_rev_out;          /* (T, ld_out) or NULL                                                                           */
    float* vel_out;              /* (T, ld_out) or NULL                                                                           */
    uint8_t* held_out;           /* (T, ld_out) or NULL                                                                           */
    uint8_t* instr_out;          /* (voices, ld_out) or NULL; written only with instr                                             */
} mvae_feedback_args;

int mvae_longsong_abi_version(void); /* 1 */
size_t mvae_nearest_walk_workspace(int32_t N, int32_t S, int32_t Z);
int mvae_nearest_walk(const mvae_walk_args* a, void* stream);
int mvae_feedback_rows(const mvae_feedback_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIDIVAE_LONGSONG_H */

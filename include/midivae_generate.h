/* midivae_generate.h - generated songs of libmidivae_hip.so: the decoder's latent rows of interpolation songs and medleys
 * (reference vae_evaluation.py:578-584, :705-887) written in place from a few anchor codes and a four-column recipe, and the
 * piano-roll image of decoded songs (prepare_for_drawing, :619-642, followed by data_class.monophonic_to_khot_pianoroll).
 *
 * An eighth header of the same library; the conventions are those of midivae_recon.h (this file includes midivae_hip.h for MVAE_E_*):
 *   - pointers are DEVICE pointers, `stream` is a hipStream_t; nothing allocates, nothing synchronises;
 *   - return value: 0 = enqueued, negative = rejected, nothing enqueued.  Every limit below is checked before the first launch;
 *     MVAE_E_LAUNCH if HIP refuses a launch;
 *   - versioned on its own: mvae_generate_abi_version(); mvae_abi_version() and the other side headers' versions do not move with it.
 *
 * mvae_latent_paths.  A run holds n windows; window w is described by a0[w], a1[w], c0[w], c1[w] and first_window[w] (the convention
 * of midivae_recon.h: the first window of w's song; NULL: every window is a song of its own).  The call fills the windows
 * lo .. lo + count - 1: the value of window w into row w - lo of z_out (ld_z floats between two rows, columns 0..Z-1 written, the
 * rest not touched) and, unless hist_out is NULL, its history into row w - lo of hist_out (ld_hist).
 *   Value of window w, column j, with A = anchors (n_anchors rows, ld_anchor elements between two rows); every operation is rounded
 *   on its own, no fused multiply-add:
 *       anchor_f64 == 0:  fl32(fl32(A[a0][j] * (float)c0) + fl32(A[a1][j] * (float)c1))                       in float32
 *       anchor_f64 == 1:  (float)(fl64(fl64(A[a0][j] * c0) + fl64(A[a1][j] * c1)))   in double, rounded once to float32 at the end
 *   which is NumPy's `p0 * (1.0 - t) + p1 * t` with a Python float t on float32 / float64 arrays, followed by the float32 cast of the
 *   decoder's input.  a1[w] < 0: the row is a copy of A[a0[w]] (rounded to float32 for float64 anchors); c0[w], c1[w] are not read.
 *   A blend at c1 = 0 is NOT that copy: it turns -0.0 into +0.0.  An a0[w], or a non-negative a1[w], outside [0, n_anchors) is
 *   never read: the row is NaN.
 *   History of window w: zeros when w == 0 or first_window[w] >= w (or first_window is NULL); else the VALUE of window w - 1,
 *   computed again from its own table row, so that no lane waits for another (window w - 1 may lie before lo).
 *   Refusals.  MVAE_E_ARG: a NULL `a`, anchors, a0, a1, c0, c1 or z_out; n, count, Z or n_anchors <= 0; lo < 0; lo + count > n;
 *   ld_anchor < Z, ld_z < Z, ld_hist < Z (with hist_out); anchor_f64 outside 0..1.  MVAE_E_UNSUPPORTED: Z > 4096 = MVAE_PATHS_MAX_Z.
 *   One launch; one lane per element, no workgroup waits for another.
 *
 * mvae_pianoroll.  idx, stride_t, stride_w, vel, first_window, n, T, voices, silent and n_pitch are named and read exactly as in
 * mvae_recon_args: row t of window w is voice t % voices of tick t / voices and lies at idx[t * stride_t + w * stride_w], vel at the
 * same offset; an index SOUNDS unless it equals `silent`, is 255, or is >= n_pitch; first_window[w] outside 0..w is read as the nearer
 * end of that range; NULL: every window is a song of its own.
 *   img_out is (n * T / voices, ld_img) doubles, tick-major: tick w * T / voices + t / voices of the run is row t of window w.
 *   Columns 0..n_pitch-1 of every tick are written, zeros included; columns [n_pitch, ld_img) are not touched.
 *   Let `step` be the row's number within its SONG, counted from the first row of the song's first window, and `cur` the row's index
 *   if it sounds, else 0.  Per voice, in song order, a row DISPLAYS a pair (pitch, level) or nothing:
 *     struck (the float32 vel widened to double is > threshold): (index, ((double)vel - threshold) * max_velocity) if the row sounds,
 *       nothing if it does not;
 *     not struck: what row step - voices displays, if all three hold: step > voices (strictly), that row displays something, and its
 *       pitch equals cur.  Otherwise nothing.
 *   So silence after a struck note of pitch index 0 continues that note, and the rows at step == voices never inherit: the
 *   reference's own behaviour.  img[tick][p] is the sum of the levels the tick's voices display at p, added in ascending voice order
 *   starting from 0.0.  With vel == NULL (the reference's V=None): 1.0 where any voice of the tick sounds p, else 0.0; threshold and
 *   max_velocity are still checked.
 *   Refusals.  MVAE_E_ARG: a NULL `a`, idx or img_out; an extent (n, T, n_pitch) or a stride <= 0; voices outside 2..8;
 *   T % voices != 0; silent outside -1..255; ld_img < n_pitch; a threshold or max_velocity that is not finite.
 *   MVAE_E_UNSUPPORTED: n_pitch > 192 or T > 65536 = MVAE_PIANOROLL_MAX_T.
 *   One launch, one lane per (window, voice).  What a window inherits from the song before it is found by walking the voice's rows
 *   back from the window's first row - as long as the held run that reaches it, and no longer; no workgroup waits for another.
 */
#ifndef MIDIVAE_GENERATE_H
#define MIDIVAE_GENERATE_H

#include "midivae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MVAE_PATHS_MAX_Z = 4096, MVAE_PIANOROLL_MAX_VOICES = 8, MVAE_PIANOROLL_MAX_PITCH = 192, MVAE_PIANOROLL_MAX_T = 65536 };

typedef struct {
    const void* anchors;         /* (n_anchors, ld_anchor) float32 (anchor_f64 = 0) or float64 (1)                                */
    const int32_t* a0;           /* (n) the first anchor of window w                                                              */
    const int32_t* a1;           /* (n) the second anchor, or < 0: the window is a copy of anchor a0                              */
    const double* c0;            /* (n) the coefficient of anchor a0                                                              */
    const double* c1;            /* (n) the coefficient of anchor a1                                                              */
    const int32_t* first_window; /* (n) or NULL: every window is its own song                                                     */
    int32_t n;                   /* windows of the run, > 0                                                                       */
    int32_t lo;                  /* the first window this call fills, >= 0                                                        */
    int32_t count;               /* how many it fills, > 0, lo + count <= n                                                       */
    int32_t Z;                   /* latent columns, 1..4096                                                                       */
    int32_t n_anchors;           /* > 0                                                                                           */
    int32_t ld_anchor;           /* elements between two anchors, >= Z                                                            */
    int32_t anchor_f64;          /* 0 or 1                                                                                        */
    int32_t ld_z;                /* floats between two rows of z_out, >= Z                                                        */
    int32_t ld_hist;             /* floats between two rows of hist_out, >= Z with hist_out                                       */
    int32_t reserved;            /* not read                                                                                      */
    float* z_out;                /* (count, ld_z), columns 0..Z-1 written                                                         */
    float* hist_out;             /* (count, ld_hist), columns 0..Z-1 written, or NULL                                             */
} mvae_paths_args;

typedef struct {
    const uint8_t* idx;          /* the decoded index of row t of window w is idx[t * stride_t + w * stride_w]                    */
    int64_t stride_t;            /* > 0, in elements, shared by idx and vel                                                       */
    int64_t stride_w;            /* > 0                                                                                           */
    const float* vel;            /* the velocity of the row at the same offset, or NULL                                           */
    const int32_t* first_window; /* n values, or NULL: every window is its own song                                               */
    int32_t n;                   /* windows, > 0                                                                                  */
    int32_t T;                   /* rows per window, 1..65536, a multiple of voices                                               */
    int32_t voices;              /* 2..8                                                                                          */
    int32_t silent;              /* the index that means "no note", or -1 for none                                                */
    int32_t n_pitch;             /* 1..192 pitch columns                                                                          */
    int32_t ld_img;              /* doubles between two ticks of img_out, >= n_pitch                                              */
    double threshold;            /* finite: a velocity > threshold strikes a note                                                 */
    double max_velocity;         /* finite: the factor of a struck note's level                                                   */
    double* img_out;             /* (n * T / voices, ld_img), columns 0..n_pitch-1 written                                        */
} mvae_pianoroll_args;

int mvae_generate_abi_version(void); /* 1 */
int mvae_latent_paths(const mvae_paths_args* a, void* stream);
int mvae_pianoroll(const mvae_pianoroll_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIDIVAE_GENERATE_H */

/* midivae_descriptors.h - window descriptors of libmidivae_hip.so: the 15-entry signature vector and the voice-by-voice
 * harmonicity (tonal distance) of piano-roll windows, computed from the one-byte index per row the engine stages and decodes.
 *
 * A second header of the same library; the conventions are those of midivae_hip.h (which this file includes for MVAE_E_*):
 *   - pointers are DEVICE pointers, `stream` is a hipStream_t; nothing allocates, nothing synchronises;
 *   - return value: 0 = enqueued, negative = rejected, nothing enqueued.  Every limit below is checked before the first launch:
 *     MVAE_E_ARG for a NULL required pointer, an extent or stride <= 0, voices outside 2..8, T % voices != 0, ld_sig < 15,
 *     silent outside -1..255, low_crop < 0, n_pitch % 12 != 0 with harm_out; MVAE_E_UNSUPPORTED for n_pitch > 192,
 *     T > 2^20 or low_crop > 1023 (the exact integer sums are sized for these); MVAE_E_LAUNCH if HIP refuses the launch.
 *   - versioned on its own: mvae_desc_abi_version(); mvae_abi_version() does not move when this file changes.
 *
 * Semantics (reference data_class.py:25-88 harmonicity, :96-215 signature; the quirks are kept):
 *   Row t of a window belongs to voice t % voices of tick t / voices; ticks = T / voices.  An index is a sounding note unless
 *   it equals `silent`, is 255, or is >= n_pitch; its pitch is index + low_crop.
 *   sig_out[w][0..14] = notes ended / ticks, notes sounded / ticks, polyphonic ticks / ticks, then [max, min, mean, std] of the
 *   pitches / 127, of the intervals between consecutive note sets / 127, and of the note durations (an empty list: four zeros).
 *   harm_out[w][v1 * voices + v2] = mean over the segments of `resolution` ticks (T / voices / resolution of them, a remainder
 *   is ignored) of the 2-norm between the two voices' tonal centroids, over the segments in which both voices sound; NaN when
 *   there is no such segment; 0 on the diagonal.  The chroma bin of an index is index / (n_pitch / 12).
 */
#ifndef MIDIVAE_DESCRIPTORS_H
#define MIDIVAE_DESCRIPTORS_H

#include "midivae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MVAE_DESC_SIGNATURE_LENGTH = 15, MVAE_DESC_MAX_VOICES = 8, MVAE_DESC_MAX_PITCH = 192 };

typedef struct {
    const uint8_t* idx;     /* the index of row t of window w is idx[t * stride_t + w * stride_w]                              */
    int64_t stride_t;       /* > 0.  Time-major (T, Bp) buffers: stride_t = Bp, stride_w = 1 (adjacent lanes read adjacent     */
    int64_t stride_w;       /* > 0.  bytes); window-major (n, T) arrays: stride_t = 1, stride_w = T (staged through LDS)       */
    int32_t n;              /* windows, > 0                                                                                    */
    int32_t T;              /* rows per window, 1..2^20, a multiple of voices                                                   */
    int32_t voices;         /* 2..8                                                                                            */
    int32_t silent;         /* the index that means "no note", or -1 for none (255 and indices >= n_pitch are silent too)      */
    int32_t n_pitch;        /* 1..192 pitch columns; with harm_out a multiple of 12                                            */
    int32_t low_crop;       /* 0..1023, added to an index to make it a pitch                                                    */
    int32_t resolution;     /* > 0, ticks per harmonicity segment                                                              */
    int32_t ld_sig;         /* >= 15, doubles between two rows of sig_out                                                      */
    const float* tonal;     /* (6, 12) tonal matrix, row-major; required with harm_out (the device widens it to double)        */
    double* sig_out;        /* (n, ld_sig), columns 0..14 written, or NULL                                                     */
    double* harm_out;       /* (n, voices * voices), or NULL; at least one of the two outputs is given                         */
} mvae_desc_args;

int mvae_desc_abi_version(void); /* 1 */
int mvae_desc_windows(const mvae_desc_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIDIVAE_DESCRIPTORS_H */

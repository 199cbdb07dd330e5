/* midivae_events.h - note events of libmidivae_hip.so: what the reference's rolls_to_midi (midi_functions.py:57-137) turns the rolls
 * of a decoded song into - one note per (start, end, pitch, velocity, voice) - from the one-byte index, the float velocity and the
 * held-notes byte per row that a decode (and mvae_recon_songs behind it) leaves on the device.
 *
 * A fifth header of the same library; the conventions are those of midivae_recon.h (this file includes midivae_hip.h for MVAE_E_*):
 *   - pointers are DEVICE pointers, `stream` is a hipStream_t; nothing allocates, nothing synchronises;
 *   - return value: 0 = enqueued, negative = rejected, nothing enqueued.  Every limit below is checked before the first launch:
 *     MVAE_E_ARG for a NULL `a`, a NULL idx, song, workspace, offsets or total, NULL records with capacity > 0, an extent (n, T,
 *     n_pitch, n_songs) or a stride <= 0, n_songs > n, voices outside 2..8, T % voices != 0, silent outside -1..255, smallest_note <= 0, a
 *     threshold that is not finite, pitch_base < 0, pitch_base + n_pitch > 256, close_at_end outside 0..1, capacity < 0;
 *     MVAE_E_UNSUPPORTED for T > 65536 = MVAE_EVENTS_MAX_T or n * T > 2^31 - 1 (ticks, ranks and record counts are int32);
 *     MVAE_E_LAUNCH if HIP refuses a launch.
 *   - versioned on its own: mvae_events_abi_version(); the other four versions do not move with this file.
 *
 * Semantics.  Row t of a window belongs to voice t % voices of tick t / voices.  An index SOUNDS unless it equals `silent`, is 255,
 * or is >= n_pitch (as in midivae_recon.h).  song[w] is the ordinal 0..n_songs-1 of window w's song: non-decreasing, the windows of
 * a song contiguous (an ordinal outside 0..n_songs-1 yields no records for that window; an ordinal no window carries is an empty
 * song).  Tick i of voice v of a song is row i * voices + v of the song's concatenated rows; p_i is its index if the row sounds.
 *   For i >= 1 with p_{i-1} sounding the note CONTINUES on tick i
 *     with held:     if held_i != 0 and p_i == p_{i-1}   (the reference's held roll > 0.5, and "note not in notes" releases);
 *     without held:  if p_i == p_{i-1} and i % smallest_note != 0   (i: the tick in the SONG, not in the window).
 *   An END falls on tick i when p_{i-1} sounds and the note does not continue; a START falls on tick i when p_i sounds and no note
 *   continues there.  At a song's first tick there is no p_{i-1}.  Starts and ends alternate per voice; the k-th start of a (song,
 *   voice) pairs with its k-th end and every end yields one note.  A start without an end - the note still sounds on the song's last
 *   row - is dropped, as the reference drops it (it never flushes its tracker); with close_at_end it is closed at the song's tick
 *   count instead.
 *   Velocity of a note, with vel: from x = the float32 at the start row widened to double, in double and in the reference's order
 *   (:78-81): x' = 0 if x < threshold, else x;  x' = x' - 0.5 if x' >= threshold (the 0.5 is the reference's literal; for a
 *   threshold > 0 a zeroed value stays 0);  y = (x' / (1.0 - threshold)) * 127.0, truncated toward zero; above 127 it becomes 127;
 *   negative values are kept (the field is signed; below -32768 it becomes -32768; a NaN becomes 0).  Without vel: 80.
 *
 * Outputs.  records: packed 12-byte mvae_note_event, sorted by (song, voice, start); the notes of (song s, voice v) are
 * records[offsets[s * voices + v] .. offsets[s * voices + v + 1]).  offsets: n_songs * voices + 1 int32.  total: one int32, the
 * number of notes, always written - also when it exceeds capacity.  Records at positions >= capacity are not written and nothing past
 * capacity records is ever touched: a call with capacity 0 (records may be NULL) only counts.  n * T records always suffice.
 *   workspace: MVAE_EVENTS_WORKSPACE_BYTES(n, n_songs, voices) bytes, 4-byte aligned, read and written by every call.
 * Four launches, ordered by the stream; no workgroup waits for another: the first and last window of every song; starts and ends per
 * (window, voice); their ranks per (song, voice), the notes per (song, voice) and `offsets` (one workgroup, looping); the records.
 */
#ifndef MIDIVAE_EVENTS_H
#define MIDIVAE_EVENTS_H

#include "midivae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MVAE_EVENTS_MAX_VOICES = 8, MVAE_EVENTS_MAX_T = 65536, MVAE_EVENTS_DEFAULT_VELOCITY = 80 };

#define MVAE_EVENTS_WORKSPACE_BYTES(n, n_songs, voices) \
    (4 * (2 * (size_t)(n) * (size_t)(voices) + 2 * (size_t)(n_songs) * ((size_t)(voices) + 1)))

typedef struct {
    int32_t start;               /* tick of the song on which the note starts                                                     */
    int32_t end;                 /* tick on which it ends (> start); the song's tick count for a note closed by close_at_end      */
    uint8_t pitch;               /* index + pitch_base                                                                            */
    uint8_t voice;
    int16_t velocity;            /* see above: <= 127, negative values kept                                                       */
} mvae_note_event;

typedef struct {
    const uint8_t* idx;          /* the decoded index of row t of window w is idx[t * stride_t + w * stride_w]                    */
    int64_t stride_t;            /* > 0, in elements, shared by idx, vel and held.  Time-major (T, Bp) buffers: stride_t = Bp,     */
    int64_t stride_w;            /* > 0.  stride_w = 1; window-major (n, T): stride_t = 1, stride_w = T                           */
    const float* vel;            /* the velocity of the row at the same offset, or NULL                                           */
    const uint8_t* held;         /* != 0: the row holds the voice's note; at the same offset, or NULL: the tick rule              */
    const int32_t* song;         /* n song ordinals, see above                                                                    */
    int32_t n;                   /* windows, > 0                                                                                  */
    int32_t T;                   /* rows per window, 1..65536, a multiple of voices                                               */
    int32_t voices;              /* 2..8                                                                                          */
    int32_t silent;              /* the index that means "no note", or -1 for none                                                */
    int32_t n_pitch;             /* pitch columns, 1..256 - pitch_base                                                            */
    int32_t n_songs;             /* 1..n                                                                                          */
    int32_t smallest_note;       /* > 0: without held a note is struck again every smallest_note ticks of the song                */
    int32_t pitch_base;          /* >= 0: the MIDI pitch of column 0 (the reference's low_crop)                                   */
    int32_t close_at_end;        /* 0 or 1                                                                                        */
    int32_t capacity;            /* >= 0: the records `records` has room for                                                      */
    double threshold;            /* finite                                                                                        */
    void* workspace;             /* MVAE_EVENTS_WORKSPACE_BYTES(n, n_songs, voices) bytes                                         */
    mvae_note_event* records;    /* capacity records, 4-byte aligned; may be NULL with capacity 0                                 */
    int32_t* offsets;            /* n_songs * voices + 1 values                                                                   */
    int32_t* total;              /* one value                                                                                     */
} mvae_events_args;

int mvae_events_abi_version(void); /* 1 */
int mvae_note_events(const mvae_events_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIDIVAE_EVENTS_H */

/* midivae_import.h - rolls from notes in libmidivae_hip.so: what the reference's load_rolls (import_midi.py:94-286, with
 * include_only_monophonic_instruments False) makes of the tick-quantised notes of whole songs - the inverse of midivae_events.h.  The
 * product is the engine's wire: one index byte, one float velocity and one held byte per row, in windows of T rows.
 *
 * A sixth header of the same library; the conventions are those of midivae_events.h (this file includes midivae_hip.h for MVAE_E_*):
 *   - pointers are DEVICE pointers, `stream` is a hipStream_t; nothing allocates, nothing synchronises;
 *   - return value: 0 = enqueued, negative = rejected, nothing enqueued.  Every limit below is checked before the first launch:
 *     MVAE_E_ARG for a NULL `a`, a NULL note_off, track_off, ticks, win_off, workspace, idx, held, slots or slot_voice, NULL notes with
 *     n_notes > 0, NULL concurrent with n_tracks > 0, n_songs, n_windows, T, max_per_track or a stride <= 0, n_notes, n_tracks or cells
 *     < 0, voices outside 1..8, T % voices != 0, pitch_base < 0, n_pitch <= 0, pitch_base + n_pitch > 128, silent outside 0..255, a
 *     threshold that is not finite or lies outside [0, 1);
 *     MVAE_E_UNSUPPORTED for n_tracks > 65535 = MVAE_IMPORT_MAX_TRACKS, n_windows * T > 2^31 - 1 or cells > 2^31 - 1;
 *     MVAE_E_LAUNCH if HIP refuses a launch.
 *   - versioned on its own: mvae_import_abi_version(); the other five versions do not move with this file.
 *
 * Inputs.  The offsets and `ticks` live on the device, so the entry point cannot read them: note_off, track_off and win_off are
 * non-decreasing and start at 0, ticks[s] >= 0, and the host-side totals n_notes = note_off[n_songs], n_tracks = track_off[n_songs],
 * n_windows = win_off[n_songs] and cells = the sum over the songs of tracks(s) * ticks[s] are the CALLER'S CONTRACT, as is
 * win_off[s + 1] - win_off[s] >= ceil(ticks[s] * voices / T).  The kernels compare every index they form with n_notes, n_tracks,
 * n_windows and cells: whatever the arrays hold, nothing outside the buffers sized by those four totals is read or written.
 *   The records of song s are notes[note_off[s] .. note_off[s + 1]), its tracks are track_off[s] .. track_off[s + 1] and a record's
 * `track` counts WITHIN ITS SONG (concurrent[] is indexed by track_off[s] + track).  Records of one (track, start, pitch) are
 * adjacent and the last of them gives the key's velocity.  A record whose track is not one of its song's, or whose pitch is > 127,
 * is ignored.
 *
 * Semantics (reference :94-286).
 *   1. A record with end > start paints (tick, pitch) for start <= tick < min(end, ticks[s]) and adds 1 to its track's count on those
 *      ticks - per note: two overlapping notes of one pitch count 2.  concurrent[track] is the maximum of the count over the ticks.
 *   2. Every record, also one with end == start, makes (start, pitch) a KEY of its track, with the velocity of its last record.
 *   3. Voices per song (:161-231): cap[track] = max_per_track; free = voices - sum over the first `voices` tracks of
 *      (c > 0 ? min(max_per_track, c) : 0); for each of the first min(voices, tracks) tracks with c > max_per_track and free > 0, in
 *      order: add = min(free, c - max_per_track), cap += add, free -= add.  Then the tracks with c > 0, in order, each give their
 *      voices 0 .. min(c, cap) - 1 until `voices` slots are full: slots[s * voices + j] is the track of output voice j (-1: none),
 *      slot_voice[s * voices + j] its voice within that track (0 where there is none).
 *   4. Output row r of a song is tick r / voices of slot r % voices; row r is row r % T of window win_off[s] + r / T.
 *   5. Voice k of a track on a tick is its (k+1)-th highest painted pitch among all 128 - the rank is taken before the crop.
 *   6. idx = pitch - pitch_base for a pitch in [pitch_base, pitch_base + n_pitch), else `silent`.
 *   7. held = 1 iff the voice has a painted pitch on the tick whose (tick, pitch) is not a key.
 *   8. vel_raw = the key's velocity if (tick, pitch) is a key, else 0;  vel = (float)(threshold + (v / 127.) * (1.0 - threshold)) for
 *      v > 0, in double and in that order (no fused multiply-add), else 0.
 *   9. held and the velocities follow the UNCROPPED pitch: a row whose pitch the crop removes is silent in idx and keeps them.
 *  10. Rows past ticks[s] * voices, slots without a track and ticks without a k-th pitch: `silent`, velocity 0, held 0.  EVERY row of
 *      every window 0 .. n_windows is written, in idx, held and (where given) vel_raw and vel; nothing else of those buffers is.
 *
 * workspace: MVAE_IMPORT_WORKSPACE_BYTES(cells, n_songs) bytes, 4-byte aligned, read and written by every call: a 128-bit pitch mask,
 * a 128-bit key mask and an int32 count per (track, tick), and the songs' first cells.
 * Seven launches, ordered by the stream; no workgroup waits for another: the songs' first cells (one workgroup, looping); the masks
 * cleared; one lane per record paints (integer atomicOr / atomicAdd: the result does not depend on the order of arrival); one
 * workgroup per track, looping, reduces the count; one lane per song allots the voices; one lane per output row selects its pitch and
 * writes idx, held and zero velocities; one lane per record writes the velocity of its key.
 */
#ifndef MIDIVAE_IMPORT_H
#define MIDIVAE_IMPORT_H

#include "midivae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MVAE_IMPORT_MAX_VOICES = 8, MVAE_IMPORT_MAX_TRACKS = 65535, MVAE_IMPORT_PITCHES = 128 };

#define MVAE_IMPORT_WORKSPACE_BYTES(cells, n_songs) (4 * (9 * (size_t)(cells) + (size_t)(n_songs) + 1))

typedef struct {
    int32_t start;               /* tick of the song on which the note starts                                                     */
    int32_t end;                 /* tick on which it ends, >= start                                                               */
    uint8_t pitch;               /* MIDI pitch 0..127                                                                             */
    uint8_t velocity;            /* 0..127                                                                                        */
    uint16_t track;              /* the track within the song                                                                     */
} mvae_import_note;

typedef struct {
    const mvae_import_note* notes; /* n_notes records sorted by (song, track, start, pitch); may be NULL with n_notes 0           */
    const int32_t* note_off;     /* n_songs + 1                                                                                   */
    const int32_t* track_off;    /* n_songs + 1                                                                                   */
    const int32_t* ticks;        /* n_songs                                                                                       */
    const int32_t* win_off;      /* n_songs + 1                                                                                   */
    int32_t n_songs;             /* > 0                                                                                           */
    int32_t n_notes;             /* >= 0: note_off[n_songs]                                                                       */
    int32_t n_tracks;            /* 0..65535: track_off[n_songs]                                                                  */
    int32_t n_windows;           /* > 0: win_off[n_songs]                                                                         */
    int32_t T;                   /* rows per window, a multiple of voices                                                         */
    int32_t voices;              /* 1..8                                                                                          */
    int32_t max_per_track;       /* >= 1: the reference's MAXIMAL_NUMBER_OF_VOICES_PER_TRACK                                      */
    int32_t pitch_base;          /* >= 0: the MIDI pitch of column 0 (the reference's low_crop)                                   */
    int32_t n_pitch;             /* 1..128 - pitch_base: high_crop - low_crop                                                     */
    int32_t silent;              /* 0..255: the index written for "no note"                                                       */
    int64_t cells;               /* >= 0: the sum over the songs of tracks * ticks                                                */
    int64_t stride_t;            /* > 0, in elements, shared by idx, held, vel_raw and vel: row t of window w is at               */
    int64_t stride_w;            /* > 0.  t * stride_t + w * stride_w; window-major (n, T): stride_t = 1, stride_w = T            */
    double threshold;            /* in [0, 1)                                                                                     */
    void* workspace;             /* MVAE_IMPORT_WORKSPACE_BYTES(cells, n_songs) bytes                                             */
    uint8_t* idx;
    uint8_t* held;
    uint8_t* vel_raw;            /* may be NULL                                                                                   */
    float* vel;                  /* may be NULL                                                                                   */
    int32_t* concurrent;         /* n_tracks values; may be NULL with n_tracks 0                                                  */
    int32_t* slots;              /* n_songs * voices                                                                              */
    int32_t* slot_voice;         /* n_songs * voices                                                                              */
} mvae_import_args;

int mvae_import_abi_version(void); /* 1 */
int mvae_rolls_from_notes(const mvae_import_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIDIVAE_IMPORT_H */

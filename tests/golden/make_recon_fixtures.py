#!/usr/bin/env python3
"""Generate tests/golden/recon.npz: song-level velocities, note starts and reconstruction counts from the reference's own functions.

Runs ONLY where the reference is present (make_fixtures.REF).  vae_definition is imported with the stub modules of make_fixtures.py
and its process_decoder_outputs is called on the one-hot rows of a WHOLE song, as the reference's evaluation calls it
(vae_evaluation.py:2196-2201): V and D of the fixture are its results.  The counts are the reference's own arithmetic
(vae_evaluation.py:2211-2236 and :2380-2397), restated here in NumPy on the same one-hot matrices: np.unique(song * 2 + Y_pred),
np.count_nonzero and the note-start loop - per window for the (n, 8) table and per song for the metric rows.  Only data is written.

  python tests/golden/make_recon_fixtures.py

Songs: the shipped shape (T = 64 rows = 16 ticks x 4 voices, 60 pitch columns + the silent one, threshold 0.5, rules on).  Six songs of
1..12 windows from each of the four random-walk generators of the descriptor fixture, then four hand-made songs: every window
silent (originals too: no original note, accuracy NaN - the reference itself divides two Python ints there and stops); a one-window
song; a voice that stays under the threshold for three whole windows and then changes pitch (the inherited velocity comes from four
windows back); and a voice whose last row of a window is pitch column 0 and whose next window opens on another pitch with a quiet
velocity (``previous_pitch > 0`` at a window boundary) beside a voice that does inherit there.  Velocities are float32 in [0, 1], a
third of them multiples of 1/8.  Originals: the predicted song with about a third of the rows replaced by a random column (the
silent one included).  A second pass gives the model a held-notes head (``held``: random
0 / 1 per row, D is then that index): without one a note start never falls on a row whose prediction does not sound - such a row has
velocity 0 after the rules - so column 6 of the counts is 0 by construction; ``counts_held`` is the table of that pass.  Assertions
keep the fixture from going soft: in at least a quarter of the multi-window songs the song-level velocities differ from the
per-window ones, every counts column is non-zero somewhere (column 6 in the held pass), even and odd song lengths both occur.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mfx  # noqa: E402
from make_descriptor_fixtures import GENERATORS, random_walk_windows  # noqa: E402

SONGS_PER_GENERATOR = 6
METRICS = ("total_original_notes", "total_predicted_notes", "pitch_reconstruction_accuracy", "not_predicted_notes",
           "new_predicted_notes", "predicted_note_start_to_original_errors", "predicted_note_start_to_predicted_errors")


def reference_counts(song, Y_pred, Y, D_pred, include_silent_note):
    """the eight numbers of the reference's report for the rows given: ``song`` / ``Y_pred`` (rows, n_pitch) one-hot rolls without the
    silent column, ``Y`` (rows, output_dim) the original with it, ``D_pred`` (rows,)"""
    difference_song = song * 2 + Y_pred
    unique, counts = np.unique(difference_song, return_counts=True)
    difference_statistics = dict(zip(unique, counts))
    total_original_notes = np.count_nonzero(song)
    total_predicted_notes = np.count_nonzero(Y_pred)
    correct_predicted_notes = difference_statistics.get(3, 0)
    not_predicted_notes = difference_statistics.get(2, 0)
    new_predicted_notes = difference_statistics.get(1, 0)
    note_starts = to_predicted = to_original = 0
    for row in range(Y_pred.shape[0]):
        note_vector_predicted_is_silent = np.sum(Y_pred[row]) == 0
        if include_silent_note:
            note_vector_original_is_silent = Y[row][-1] == 1
        else:
            note_vector_original_is_silent = np.sum(Y[row]) == 0
        predicted_duration_is_note_start = D_pred[row] == 0
        note_starts += int(predicted_duration_is_note_start)
        if note_vector_predicted_is_silent and predicted_duration_is_note_start:
            to_predicted += 1
        if note_vector_original_is_silent and predicted_duration_is_note_start:
            to_original += 1
    return [int(total_original_notes), int(total_predicted_notes), int(correct_predicted_notes), int(not_predicted_notes),
            int(new_predicted_notes), note_starts, to_predicted, to_original]


def main():
    if not os.path.isdir(mfx.REF):
        raise SystemExit("reference not present; fixtures can only be regenerated where it is")
    mfx._stub_modules()
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp(prefix="mvae_fixture_"))          # the reference's settings module makes folders where it is imported
    sys.path.insert(0, mfx.REF)
    import settings
    import vae_definition as vd
    os.chdir(cwd)
    for name in ("settings", "data_class", "midi_functions", "vae_definition"):
        sys.modules.pop(name, None)
    sys.path.remove(mfx.REF)
    process = vd.process_decoder_outputs          # the one function this fixture pins

    V, T, D, ID = int(settings.max_voices), int(settings.output_length), int(settings.output_dim), int(settings.meta_instrument_dim)
    thr = float(settings.velocity_threshold_such_that_it_is_a_played_note)
    s = dict(max_voices=V, low_crop=int(settings.low_crop), high_crop=int(settings.high_crop),
             include_silent_note=bool(settings.include_silent_note), velocity_threshold_such_that_it_is_a_played_note=thr,
             override_sampled_pitches_based_on_velocity_info=bool(settings.override_sampled_pitches_based_on_velocity_info),
             meta_velocity=bool(settings.meta_velocity), meta_held_notes=bool(settings.meta_held_notes))
    n_pitch = s["high_crop"] - s["low_crop"]
    assert (T, V, D, n_pitch, thr, s["include_silent_note"], s["override_sampled_pitches_based_on_velocity_info"]) == \
        (64, 4, 61, 60, 0.5, True, True)
    assert settings.meta_instrument and settings.meta_velocity and not settings.meta_held_notes and not settings.meta_next_notes

    rng = np.random.default_rng(20261021)

    def velocities(n):
        v = rng.random((n, T))
        v = np.where(rng.random((n, T)) < 1 / 3, np.round(v * 8) / 8, v)
        return v.astype(np.float32)

    songs = []          # (idx, vel, orig or None: derived below)
    for ps, ph in GENERATORS:
        for _ in range(SONGS_PER_GENERATOR):
            n = int(rng.integers(1, 13))
            songs.append([random_walk_windows(rng, n, T, V, n_pitch, ps, ph), velocities(n), None])
    # every window silent, the originals too
    songs.append([np.full((3, T), n_pitch, np.uint8), velocities(3), np.full((3, T), n_pitch, np.uint8)])
    # a one-window song
    songs.append([random_walk_windows(rng, 1, T, V, n_pitch, 0.3, 0.3), velocities(1), None])
    # voice 0: loud on column 10 to the end of window 0, three whole windows under the threshold on the same column, then window 4
    # opens on column 14 with a quiet velocity: it inherits 0.875 from four windows back
    far_idx, far_vel = random_walk_windows(rng, 5, T, V, n_pitch, 0.3, 0.3), velocities(5)
    far_idx[:, 0::V] = 10
    far_vel[0, 0::V] = 0.625
    far_vel[0, T - V] = 0.875
    far_vel[1:4, 0::V] = 0.25
    far_idx[4, 0], far_vel[4, 0] = 14, 0.125
    songs.append([far_idx, far_vel, None])
    # the window boundary: voice 0 ends window 0 on column 0 (loud) and opens window 1 on column 5, quiet: `previous_pitch > 0` leaves
    # it; voice 1 ends on column 3 (0.8125) and opens on column 7, quiet: it inherits
    edge_idx, edge_vel = random_walk_windows(rng, 2, T, V, n_pitch, 0.3, 0.3), velocities(2)
    edge_idx[0, T - V:T - V + 2], edge_vel[0, T - V:T - V + 2] = [0, 3], [0.9375, 0.8125]
    edge_idx[1, 0:2], edge_vel[1, 0:2] = [5, 7], [0.125, 0.1875]
    songs.append([edge_idx, edge_vel, None])
    for song in songs:
        if song[2] is None:
            replace = rng.random(song[0].shape) < 1 / 3
            song[2] = np.where(replace, rng.integers(0, n_pitch + 1, song[0].shape), song[0]).astype(np.uint8)

    def onehot(idx, width):
        out = np.zeros(idx.shape + (width,))
        np.put_along_axis(out, idx[..., None].astype(np.int64), 1, axis=-1)
        return out

    def decode(idx, vel, held=None):
        """the reference on the windows given as ONE song: Y (rows, n_pitch), V (rows,), D (rows,); with ``held`` the model has the
        held-notes head and D is its index"""
        n = idx.shape[0]
        I = np.zeros((n, V, ID))
        I[:, :, 0] = 1
        outputs = [onehot(idx, D), I, vel.astype(np.float64).reshape(n, T, 1)]
        vd.meta_held_notes = held is not None
        if held is not None:
            outputs.append(onehot(held, 2))
        Y, _, V_pred, D_pred, _ = process(outputs, "argmax")
        vd.meta_held_notes = s["meta_held_notes"]
        return np.asarray(Y), np.asarray(V_pred, np.float64), np.asarray(D_pred)

    lengths = np.array([song[0].shape[0] for song in songs], np.int64)
    idx, vel, orig = (np.concatenate([song[k] for song in songs], 0) for k in range(3))
    n = idx.shape[0]
    held = (rng.random((n, T)) < 0.6).astype(np.uint8)          # what a held-notes head might say: unrelated to the notes
    velocity, per_window = np.zeros((n, T)), np.zeros((n, T))
    starts = np.zeros((n, T), np.uint8)
    counts, counts_held = np.zeros((n, 8), np.int64), np.zeros((n, 8), np.int64)
    metrics = np.zeros((len(songs), len(METRICS)))
    differs = []
    lo = 0
    for i, (song_idx, song_vel, song_orig) in enumerate(songs):
        m = song_idx.shape[0]
        Y_pred, V_pred, D_pred = decode(song_idx, song_vel)
        velocity[lo:lo + m] = V_pred.reshape(m, T)
        starts[lo:lo + m] = D_pred.reshape(m, T)
        Y_held, V_held, D_held = decode(song_idx, song_vel, held[lo:lo + m])
        assert np.array_equal(Y_held, Y_pred) and np.array_equal(V_held, V_pred) and np.array_equal(D_held.reshape(m, T), held[lo:lo + m])
        Y = onehot(song_orig, D).reshape(m * T, D)
        song = Y[:, :n_pitch]
        for w in range(m):
            rows = slice(w * T, (w + 1) * T)
            counts[lo + w] = reference_counts(song[rows], Y_pred[rows], Y[rows], D_pred[rows], s["include_silent_note"])
            counts_held[lo + w] = reference_counts(song[rows], Y_pred[rows], Y[rows], D_held[rows], s["include_silent_note"])
            per_window[lo + w] = decode(song_idx[w:w + 1], song_vel[w:w + 1])[1]
        c = reference_counts(song, Y_pred, Y, D_pred, s["include_silent_note"])
        assert c == counts[lo:lo + m].sum(0).tolist()
        # (0 / 0 on Python ints: the reference stops there; the report says NaN)
        metrics[i] = [c[0], c[1], c[2] / c[0] if c[0] else np.nan, c[3], c[4], c[7] / (m * T), c[6] / (m * T)]
        if m > 1:
            differs.append(bool(np.any(velocity[lo:lo + m] != per_window[lo:lo + m])))
        lo += m

    assert np.array_equal(velocity.astype(np.float32).astype(np.float64), velocity)          # input values and zeros: nothing rounds
    print("multi-window songs whose velocities differ from the per-window rule: %d of %d" % (sum(differs), len(differs)))
    assert np.mean(differs) >= 0.25, "the fixture no longer needs the state carried across windows"
    # (without a held-notes head column 6 is 0 by construction: a row that does not sound has velocity 0 after the rules)
    assert np.all(np.delete(counts.sum(0), 6) > 0) and counts[:, 6].sum() == 0, "a counts column is zero everywhere: %r" % (counts.sum(0),)
    assert np.all(counts_held.sum(0) > 0), "a counts column is zero everywhere with the held head: %r" % (counts_held.sum(0),)
    assert np.array_equal(counts_held[:, :5], counts[:, :5])
    assert np.any(lengths % 2 == 0) and np.any(lengths % 2 == 1) and lengths.min() == 1 and lengths.max() <= 12
    first = np.cumsum(lengths) - lengths
    far, edge = first[-2], first[-1]
    assert velocity[far + 4, 0] == 0.875 and per_window[far + 4, 0] == 0.125, "the four-windows-back song lost its point"
    assert velocity[edge + 1, 0] == 0.125 and velocity[edge + 1, 1] == 0.8125 and per_window[edge + 1, 1] == 0.1875, \
        "the window-boundary song lost its point"
    assert np.isnan(metrics[-4, 2]) and not np.isnan(np.delete(metrics[:, 2], len(songs) - 4)).any()

    out = dict(idx=idx, vel=vel, orig=orig, lengths=lengths, velocity=velocity.astype(np.float32), starts=starts,
               counts=counts.astype(np.int32), held=held, counts_held=counts_held.astype(np.int32), metrics=metrics, metric_names=np.array(METRICS),
               **{"s_" + k: np.asarray(v) for k, v in s.items()})
    path = os.path.join(HERE, "recon.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "songs:", len(songs), "windows:", n, "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()

"""Drop-in for the reference's ``midi_functions`` module (reference midi_functions.py:14-137), bound to the flat ``settings``
namespace at call time like ``data_class``.  ``rolls_to_midi`` takes one song's host rolls, as the reference's callers pass them
(vae_evaluation.py:837, :885, :2204, :2442, :2625), runs the NumPy mirror of ``midi_vae_amd.events`` and writes the file with
``midi_vae_amd.midifile`` - no pretty_midi.  Songs that are already on the device go through ``decoder.predict_songs(...,
note_events=True)`` or ``events.note_events`` instead."""
import os

import numpy as np

import midi_vae_amd  # noqa: F401
import settings as _settings
from midi_vae_amd import events as _ev
from midi_vae_amd import midifile as _mf
from midi_vae_amd import packers as _pk


def programs_to_instrument_matrix(programs, instrument_attach_method, max_voices):
    return _pk.programs_to_instrument_matrix(programs, instrument_attach_method, max_voices)


def rolls_to_midi(pianoroll, programs, save_folder, filename, bpm, velocity_roll=None, held_notes_roll=None):
    """Write ``save_folder + filename + '.mid'`` (the reference's own concatenation) and return that path.  ``pianoroll``: (rows,
    high_crop - low_crop) with at most one 1 per row, row r being voice r % len(programs) of tick r // len(programs);
    ``velocity_roll`` / ``held_notes_roll``: (rows,) or None.  A row with several notes - the reference's tracker handles those - gets
    a NotImplementedError: a decode produces none.  Velocities outside 0..127 are clamped on writing (midifile.write_midi)."""
    s = dict(vars(_settings), max_voices=len(programs))
    pianoroll = np.asarray(pianoroll)
    V, width = len(programs), int(s["high_crop"]) - int(s["low_crop"])
    if pianoroll.ndim != 2 or pianoroll.shape[1] != width or pianoroll.shape[0] % V:
        raise ValueError("the pianoroll must be (rows, %d) with rows a multiple of the %d programs, got %r" % (width, V, pianoroll.shape))
    per_row = np.count_nonzero(pianoroll, axis=1)
    if np.any(per_row > 1):
        raise NotImplementedError("polyphonic rows: row %d holds %d notes; rolls_to_midi takes the rolls of a decode, one note per "
                                  "row at most" % (int(np.argmax(per_row > 1)), int(per_row.max())))
    # every tick a window of its own: a song of any length
    idx = np.where(per_row == 1, np.argmax(pianoroll != 0, axis=1), 255).astype(np.uint8).reshape(-1, V)
    vel = None if velocity_roll is None else np.asarray(velocity_roll, np.float32).reshape(-1, V)
    held = None if held_notes_roll is None else (np.asarray(held_notes_roll).reshape(-1, V) > 0.5).astype(np.uint8)
    records, offsets = _ev.event_table(idx, vel, held, [idx.shape[0]], s, device=False)
    if not os.path.exists(save_folder):
        os.makedirs(save_folder)
    path = save_folder + filename + ".mid"
    _mf.write_midi(path, [records[offsets[v]:offsets[v + 1]] for v in range(V)], programs, bpm, int(s["SMALLEST_NOTE"]))
    return path

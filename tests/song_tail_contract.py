"""The rolls the song-tail tests share (test_song_tail_cpu.py, test_song_tail_gpu.py): random voice walks with the rows planted on
which mvae_sweep_windows' ``vel_out`` and mvae_recon_songs without a song structure could part - both state the velocity post-rule
with every window starting afresh."""
import numpy as np

THRESHOLD, N_PITCH = 0.5, 60
# (n, T, V).  A sweep workgroup is 64 windows, a recon workgroup 256 / V windows: 130 windows of 2 voices are three of the one and two
# of the other (70, the first thought, would stay inside one recon workgroup at V = 2); 5 windows of 4 voices stay inside one of each.
SHAPES = ((5, 16, 4), (130, 8, 2))


def settings(V, override):
    return dict(max_voices=V, low_crop=24, high_crop=24 + N_PITCH, include_silent_note=True,
                velocity_threshold_such_that_it_is_a_played_note=THRESHOLD, override_sampled_pitches_based_on_velocity_info=override)


def planted_rolls(n, T, V):
    """(idx (n, T) uint8, vel (n, T) float32, plants): ``plants`` lists (window, row, what the row must become with the rules on) -
    None: the NaN it holds"""
    rng = np.random.default_rng(1000 * n + T)
    ticks = T // V
    assert ticks >= 4 and n >= 3
    rest = rng.random((n, ticks, V)) < 0.3
    idx = np.where(rest, N_PITCH, rng.integers(0, N_PITCH, (n, ticks, V))).astype(np.uint8).reshape(n, T)
    vel = rng.random((n, T)).astype(np.float32)
    row = lambda tick, voice: tick * V + voice
    plants = []
    for w in (0, n - 1):          # (the last window too: it lies in the last workgroup of both kernels)
        # a silent velocity behind a pitch change inherits the loud one before it
        idx[w, row(0, 0)], idx[w, row(1, 0)] = 10, 12
        vel[w, row(0, 0)], vel[w, row(1, 0)] = 0.875, 0.125
        plants.append((w, row(1, 0), np.float32(0.875)))
    # behind previous pitch 0 it does not (the reference tests previous_pitch > 0)
    idx[1, row(0, 0)], idx[1, row(1, 0)] = 0, 5
    vel[1, row(0, 0)], vel[1, row(1, 0)] = 0.875, 0.125
    plants.append((1, row(1, 0), np.float32(0.125)))
    # a loud velocity on a silent row becomes 0
    idx[2, row(1, 1)], vel[2, row(1, 1)] = N_PITCH, 0.75
    plants.append((2, row(1, 1), np.float32(0)))
    # a NaN velocity on a sounding row: neither silent nor replaced
    idx[2, row(2, 1)], vel[2, row(2, 1)] = 7, np.nan
    plants.append((2, row(2, 1), None))
    # index 255 does not sound
    idx[2, row(3, 1)], vel[2, row(3, 1)] = 255, 0.75
    plants.append((2, row(3, 1), np.float32(0)))
    return idx, vel, plants

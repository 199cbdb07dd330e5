"""ctypes binding of libmidivae_hip.so (C ABI declared in include/midivae_hip.h).

The library is built in-tree by ``make -C midi-vae_amd/csrc`` (or ``__graft_entry__.build()``).  Loading fails
LOUDLY when it is missing: there is no CPU fallback anywhere in the product path.

Device pointers are plain integers here (``tensor.data_ptr()``); streams are the raw ``hipStream_t`` value
(``torch.cuda.current_stream().cuda_stream``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVAE_LIB", os.path.join(_HERE, "libmidivae_hip.so"))   # MVAE_LIB: experiment builds

GRU, LSTM, RNN = 0, 1, 2
F32, BF16, ONEHOT = 0, 1, 2
X_DENSE, X_INDEX, X_SCALAR, X_CONST = 0, 1, 2, 3
ACT_NONE, ACT_TANH = 0, 1
ROWMAJOR, TILE16, TILE16P, TILE16Q = 0, 1, 2, 3
TABLE_ROWMAJOR, TABLE_PAIRED, TABLE_PAIRED8 = 0, 1, 2
CELL_CODE = {"GRU": GRU, "LSTM": LSTM, "SimpleRNN": RNN}
GATES = {GRU: 3, LSTM: 4, RNN: 1}
E_ARG, E_UNSUPPORTED, E_LAUNCH, E_FORMAT = -1, -2, -3, -4
HOST_F64, HOST_F32, HOST_U8 = 0, 1, 2
ABI_VERSION = 9
ERRORS = {-1: "MVAE_E_ARG (bad argument)", -2: "MVAE_E_UNSUPPORTED (shape/dtype not built)",
          -3: "MVAE_E_LAUNCH (HIP launch failed)", -4: "MVAE_E_FORMAT (a row is not one-hot)"}

_i32, _f32, _vp, _sz, _i64 = C.c_int32, C.c_float, C.c_void_p, C.c_size_t, C.c_int64


class RnnFwdArgs(C.Structure):
    _fields_ = [("cell", _i32), ("dtype", _i32), ("xmode", _i32), ("T", _i32), ("B", _i32), ("H", _i32),
                ("u_pack", _vp), ("xp", _vp), ("idx", _vp), ("table", _vp), ("xs", _vp), ("w_row", _vp),
                ("bias", _vp), ("xp0", _vp), ("h0", _vp), ("c0", _vp), ("hs", _vp), ("cs", _vp), ("acts", _vp),
                ("h_last", _vp), ("c_last", _vp), ("h0_ld", _i32), ("h_last_ld", _i32),
                ("chunk_steps", _i32), ("wait_ready", _vp), ("wait_value", C.c_uint32), ("signal_done", _vp), ("status", _vp),
                ("seq_layout", _i32), ("table_layout", _i32)]


class RnnBwdArgs(C.Structure):
    _fields_ = [("cell", _i32), ("dtype", _i32), ("T", _i32), ("B", _i32), ("H", _i32),
                ("ut_pack", _vp), ("hs", _vp), ("cs", _vp), ("acts", _vp), ("dhs_ext", _vp), ("dh_last", _vp),
                ("dc_last", _vp), ("da", _vp), ("rh", _vp), ("dh0", _vp), ("dc0", _vp), ("dh_last_ld", _i32), ("dh0_ld", _i32),
                ("chunk_steps", _i32), ("wait_ready", _vp), ("wait_value", C.c_uint32), ("signal_done", _vp), ("status", _vp),
                ("seq_layout", _i32)]


class GemmArgs(C.Structure):
    _fields_ = [("M", _i32), ("N", _i32), ("K", _i32), ("trans_a", _i32), ("trans_b", _i32),
                ("a_kind", _i32), ("b_kind", _i32), ("c_kind", _i32), ("lda", _i32), ("ldb", _i32), ("ldc", _i32),
                ("accumulate", _i32), ("act", _i32), ("split_k", _i32), ("alpha", _f32),
                ("A", _vp), ("B", _vp), ("C", _vp), ("bias", _vp), ("c_layout", _i32), ("max_blocks", _i32),
                ("sys_release", _i32), ("chunk_rows", _i32), ("chunk_reverse", _i32), ("chunk_wait", _vp),
                ("chunk_wait_value", C.c_uint32), ("chunk_done", _vp), ("chunk_status", _vp), ("colsum_b", _vp),
                ("k_wait", _vp), ("k_wait_value", C.c_uint32), ("k_chunk_rows", C.c_int32), ("k_reverse", C.c_int32)]


class XpandArgs(C.Structure):
    _fields_ = [("xs", _vp), ("w", _vp), ("bias", _vp), ("out", _vp), ("out_kind", _i32), ("R", _i32), ("N", _i32),
                ("chunk_rows", _i32), ("chunk_done", _vp), ("blocks", _i32), ("reserved", _i32), ("idx", _vp), ("table", _vp)]


class PrepJob(C.Structure):
    _fields_ = [("op", _i32), ("kind", _i32), ("a", _i32), ("b", _i32), ("c", _i32), ("reserved", _i32),
                ("src", _vp), ("src2", _vp), ("dst", _vp)]


PREP_PACK_RECURRENT, PREP_MAKE_TABLE, PREP_TRANSPOSE_CONVERT, PREP_CONVERT, PREP_ZERO, PREP_CONVERT_PAD = 0, 1, 2, 3, 4, 5
PREP_ADD_I32, PREP_BROADCAST_ROWS = 6, 7
ADAM_ZERO_GRAD, ADAM_KEEP_COUNT = 1, 2


class HeadArgs(C.Structure):
    _fields_ = [("kind", _i32), ("dtype", _i32), ("R", _i32), ("H", _i32), ("N", _i32), ("want_grad", _i32),
                ("hs", _vp), ("wt", _vp), ("bias", _vp), ("target_idx", _vp), ("target_val", _vp),
                ("row_weight", _vp), ("grad_scale", _f32), ("probs", _vp), ("argmax", _vp), ("dlogits", _vp),
                ("scalars", _vp), ("b_stride", _i32), ("b_valid", _i32), ("wc", _vp), ("dhs", _vp), ("target_idx2", _vp),
                ("row_out", _vp)]


class SampleCtl(C.Structure):
    """per-call values of mvae_head_sample: in device memory (8 words, ``sampling.control_words``) or inside HeadSampleArgs"""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("window0_lo", C.c_uint32), ("window0_hi", C.c_uint32),
                ("temperature", _f32), ("cutoff", _f32), ("tries", _i32), ("reserved", _i32)]


class HeadSampleArgs(C.Structure):
    _fields_ = [("dtype", _i32), ("R", _i32), ("H", _i32), ("N", _i32), ("hs", _vp), ("wt", _vp), ("bias", _vp),
                ("uniforms", _vp), ("ctl", _vp), ("out", _vp), ("b_stride", _i32), ("b_valid", _i32), ("T", _i32), ("row0", _i32),
                ("head_id", _i32), ("u_stride", _i32), ("host", SampleCtl)]


SAMPLE_MAX_TRIES = 4


class LatentFwdArgs(C.Structure):
    _fields_ = [("B", _i32), ("Z", _i32), ("C", _i32), ("beta", _f32), ("prior_mean", _f32), ("prior_std", _f32),
                ("inv_batch", _f32), ("mu", _vp), ("logvar", _vp), ("eps", _vp), ("style_target", _vp),
                ("style_row_weight", _vp), ("z", _vp), ("style_probs", _vp), ("scalars", _vp), ("ldz", _i32),
                ("kl_rows", _vp), ("style_rows", _vp)]


class LatentBwdArgs(C.Structure):
    _fields_ = [("B", _i32), ("Z", _i32), ("C", _i32), ("beta", _f32), ("prior_mean", _f32), ("prior_std", _f32),
                ("style_weight", _f32), ("inv_batch", _f32), ("mu", _vp), ("logvar", _vp), ("eps", _vp), ("dz", _vp),
                ("style_probs", _vp), ("style_target", _vp), ("style_row_weight", _vp), ("dmu", _vp),
                ("dlogvar", _vp), ("lddz", _i32)]


class LatentChainFwdArgs(C.Structure):
    _fields_ = ([(n, _i32) for n in ("B", "B_valid", "H", "Z", "C", "ncat", "zin", "n_init", "split")] +
                [(n, _f32) for n in ("beta", "prior_mean", "prior_std", "inv_batch")] +
                [(n, _vp) for n in ("cat", "w_pack", "b_pack", "w_extra", "b_extra", "w_mu", "b_mu", "w_lv", "b_lv", "w_init",
                                    "b_init", "eps", "style_target", "style_row_weight", "pack", "extra", "mu", "logvar", "zh",
                                    "style_probs", "scalars", "S", "kl_rows", "style_rows")])


class LatentChainBwdArgs(C.Structure):
    _fields_ = ([(n, _i32) for n in ("B", "B_valid", "H", "Z", "C", "ncat", "zin", "n_init", "split")] +
                [(n, _f32) for n in ("beta", "prior_mean", "prior_std", "style_weight", "inv_batch")] +
                [(n, _vp) for n in ("wt_pack", "wt_extra", "wt_mu", "wt_lv", "wt_init", "S", "pack", "extra", "mu", "logvar", "eps",
                                    "style_probs", "style_target", "style_row_weight", "dS", "dzh", "dmu", "dlogvar",
                                    "d_extra", "d_pack", "dcat")])


class DescArgs(C.Structure):
    """mvae_desc_args of include/midivae_descriptors.h"""
    _fields_ = [("idx", _vp), ("stride_t", _i64), ("stride_w", _i64), ("n", _i32), ("T", _i32), ("voices", _i32), ("silent", _i32),
                ("n_pitch", _i32), ("low_crop", _i32), ("resolution", _i32), ("ld_sig", _i32), ("tonal", _vp), ("sig_out", _vp),
                ("harm_out", _vp)]


DESC_ABI_VERSION = 1
# the second header, include/midivae_descriptors.h (versioned on its own: SIGNATURES and ABI_VERSION do not move with it)
DESC_SIGNATURES = {
    "mvae_desc_abi_version": (_i32, []),
    "mvae_desc_windows": (_i32, [C.POINTER(DescArgs), _vp]),
}


class SweepArgs(C.Structure):
    """mvae_sweep_args of include/midivae_sweep.h"""
    _fields_ = [("idx", _vp), ("stride_t", _i64), ("stride_w", _i64), ("vel", _vp), ("n", _i32), ("T", _i32), ("voices", _i32),
                ("silent", _i32), ("n_pitch", _i32), ("count_a", _i32), ("count_b", _i32), ("override_rules", _i32),
                ("threshold", C.c_double), ("default_velocity", C.c_double), ("ld_out", _i32), ("reserved", _i32),
                ("stats_out", _vp), ("vel_out", _vp)]


SWEEP_ABI_VERSION = 1
# the third header, include/midivae_sweep.h (versioned on its own, like the second)
SWEEP_SIGNATURES = {
    "mvae_sweep_abi_version": (_i32, []),
    "mvae_sweep_windows": (_i32, [C.POINTER(SweepArgs), _vp]),
}

class ReconArgs(C.Structure):
    """mvae_recon_args of include/midivae_recon.h"""
    _fields_ = [("idx", _vp), ("stride_t", _i64), ("stride_w", _i64), ("vel", _vp), ("held", _vp), ("orig", _vp),
                ("orig_stride_t", _i64), ("orig_stride_w", _i64), ("first_window", _vp), ("n", _i32), ("T", _i32), ("voices", _i32),
                ("silent", _i32), ("n_pitch", _i32), ("override_rules", _i32), ("threshold", C.c_double), ("carry", _vp),
                ("vel_out", _vp), ("start_out", _vp), ("counts_out", _vp), ("ld_counts", _i32), ("reserved", _i32)]


RECON_ABI_VERSION = 1
# the fourth header, include/midivae_recon.h (versioned on its own, like the second and third)
RECON_SIGNATURES = {
    "mvae_recon_abi_version": (_i32, []),
    "mvae_recon_songs": (_i32, [C.POINTER(ReconArgs), _vp]),
}


class EventsArgs(C.Structure):
    """mvae_events_args of include/midivae_events.h"""
    _fields_ = [("idx", _vp), ("stride_t", _i64), ("stride_w", _i64), ("vel", _vp), ("held", _vp), ("song", _vp), ("n", _i32), ("T", _i32),
                ("voices", _i32), ("silent", _i32), ("n_pitch", _i32), ("n_songs", _i32), ("smallest_note", _i32), ("pitch_base", _i32),
                ("close_at_end", _i32), ("capacity", _i32), ("threshold", C.c_double), ("workspace", _vp), ("records", _vp),
                ("offsets", _vp), ("total", _vp)]


EVENTS_ABI_VERSION = 1
# the fifth header, include/midivae_events.h (versioned on its own, like the second, third and fourth)
EVENTS_SIGNATURES = {
    "mvae_events_abi_version": (_i32, []),
    "mvae_note_events": (_i32, [C.POINTER(EventsArgs), _vp]),
}

class ImportArgs(C.Structure):
    """mvae_import_args of include/midivae_import.h"""
    _fields_ = [("notes", _vp), ("note_off", _vp), ("track_off", _vp), ("ticks", _vp), ("win_off", _vp), ("n_songs", _i32),
                ("n_notes", _i32), ("n_tracks", _i32), ("n_windows", _i32), ("T", _i32), ("voices", _i32), ("max_per_track", _i32),
                ("pitch_base", _i32), ("n_pitch", _i32), ("silent", _i32), ("cells", _i64), ("stride_t", _i64), ("stride_w", _i64),
                ("threshold", C.c_double), ("workspace", _vp), ("idx", _vp), ("held", _vp), ("vel_raw", _vp), ("vel", _vp),
                ("concurrent", _vp), ("slots", _vp), ("slot_voice", _vp)]


IMPORT_ABI_VERSION = 1
# the sixth header, include/midivae_import.h (versioned on its own, like the second to fifth)
IMPORT_SIGNATURES = {
    "mvae_import_abi_version": (_i32, []),
    "mvae_rolls_from_notes": (_i32, [C.POINTER(ImportArgs), _vp]),
}


class StyleArgs(C.Structure):
    """mvae_style_args of include/midivae_style.h"""
    _fields_ = [("p_pitch", _vp), ("p_vel", _vp), ("p_instr", _vp), ("instr_row", _vp), ("cls", _vp), ("group_off", _vp), ("n", _i32),
                ("C", _i32), ("n_groups", _i32), ("n_instr_rows", _i32), ("ld_pitch", _i32), ("ld_vel", _i32), ("ld_instr", _i32),
                ("ld_ens", _i32), ("ld_table", _i32), ("reserved", _i32), ("weights", C.c_double * 3), ("ens_out", _vp),
                ("pred_out", _vp), ("table_out", _vp), ("confusion_out", _vp)]


STYLE_ABI_VERSION = 1
# the seventh header, include/midivae_style.h (versioned on its own, like the second to sixth)
STYLE_SIGNATURES = {
    "mvae_style_abi_version": (_i32, []),
    "mvae_style_scores": (_i32, [C.POINTER(StyleArgs), _vp]),
}


class PathsArgs(C.Structure):
    """mvae_paths_args of include/midivae_generate.h"""
    _fields_ = [("anchors", _vp), ("a0", _vp), ("a1", _vp), ("c0", _vp), ("c1", _vp), ("first_window", _vp), ("n", _i32), ("lo", _i32),
                ("count", _i32), ("Z", _i32), ("n_anchors", _i32), ("ld_anchor", _i32), ("anchor_f64", _i32), ("ld_z", _i32),
                ("ld_hist", _i32), ("reserved", _i32), ("z_out", _vp), ("hist_out", _vp)]


class PianorollArgs(C.Structure):
    """mvae_pianoroll_args of include/midivae_generate.h"""
    _fields_ = [("idx", _vp), ("stride_t", _i64), ("stride_w", _i64), ("vel", _vp), ("first_window", _vp), ("n", _i32), ("T", _i32),
                ("voices", _i32), ("silent", _i32), ("n_pitch", _i32), ("ld_img", _i32), ("threshold", C.c_double),
                ("max_velocity", C.c_double), ("img_out", _vp)]


GENERATE_ABI_VERSION = 1
# the eighth header, include/midivae_generate.h (versioned on its own, like the second to seventh)
GENERATE_SIGNATURES = {
    "mvae_generate_abi_version": (_i32, []),
    "mvae_latent_paths": (_i32, [C.POINTER(PathsArgs), _vp]),
    "mvae_pianoroll": (_i32, [C.POINTER(PianorollArgs), _vp]),
}

class WalkArgs(C.Structure):
    """mvae_walk_args of include/midivae_longsong.h"""
    _fields_ = [("all_z", _vp), ("r_in", _vp), ("hist_in", _vp), ("picked", _vp), ("workspace", _vp), ("N", _i32), ("S", _i32), ("Z", _i32),
                ("ld_all", _i32), ("ld_r", _i32), ("r_f64", _i32), ("ld_hist_in", _i32), ("hist_f64", _i32), ("cap", _i32),
                ("n_picked", _i32), ("ld_z", _i32), ("ld_rout", _i32), ("ld_hist", _i32), ("reserved", _i32), ("e", C.c_double),
                ("den", C.c_double), ("best_out", _vp), ("dist_out", _vp), ("z_out", _vp), ("r_out", _vp), ("hist_out", _vp)]


class FeedbackArgs(C.Structure):
    """mvae_feedback_args of include/midivae_longsong.h"""
    _fields_ = [("idx", _vp), ("stride_t", _i64), ("stride_w", _i64), ("vel", _vp), ("held_idx", _vp), ("instr", _vp),
                ("instr_stride_v", _i64), ("instr_stride_w", _i64), ("n", _i32), ("T", _i32), ("voices", _i32), ("silent", _i32),
                ("n_pitch", _i32), ("override_rules", _i32), ("threshold", C.c_double), ("ld_out", _i32), ("reserved", _i32),
                ("x_out", _vp), ("x_rev_out", _vp), ("vel_out", _vp), ("held_out", _vp), ("instr_out", _vp)]


LONGSONG_ABI_VERSION = 1
# the ninth header, include/midivae_longsong.h (versioned on its own, like the second to eighth)
LONGSONG_SIGNATURES = {
    "mvae_longsong_abi_version": (_i32, []),
    "mvae_nearest_walk_workspace": (_sz, [_i32, _i32, _i32]),
    "mvae_nearest_walk": (_i32, [C.POINTER(WalkArgs), _vp]),
    "mvae_feedback_rows": (_i32, [C.POINTER(FeedbackArgs), _vp]),
}

# name -> (restype, argtypes); every symbol include/midivae_hip.h declares
SIGNATURES = {
    "mvae_abi_version": (_i32, []),
    "mvae_rnn_producer_waves": (_i32, [_i32]),
    "mvae_build_info": (C.c_char_p, []),
    "mvae_rnn_fwd": (_i32, [C.POINTER(RnnFwdArgs), _vp]),
    "mvae_rnn_bwd": (_i32, [C.POINTER(RnnBwdArgs), _vp]),
    "mvae_rnn_fwd_multi": (_i32, [C.POINTER(RnnFwdArgs), _i32, C.POINTER(XpandArgs), _i32, _vp]),
    "mvae_rnn_bwd_multi": (_i32, [C.POINTER(RnnBwdArgs), _i32, _vp]),
    "mvae_pack_recurrent": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "mvae_gemm": (_i32, [C.POINTER(GemmArgs), _vp]),
    "mvae_gemm_kstream_multi": (_i32, [C.POINTER(GemmArgs), _i32, _vp]),
    "mvae_gemm_multi": (_i32, [C.POINTER(GemmArgs), _i32, _vp]),
    "mvae_colsum": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mvae_stream_wait_value32": (_i32, [_vp, _vp, C.c_uint32]),
    "mvae_stream_write_value32": (_i32, [_vp, _vp, C.c_uint32]),
    "mvae_occupancy": (_i32, [_i32]),
    "mvae_streams_alias": (_i32, [_vp, _vp, _vp, C.c_uint32]),
    "mvae_prepare_batch": (_i32, [_vp, _i32, _vp]),
    "mvae_outer_bias_tile16": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "mvae_gather2_tile16": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "mvae_colsum_weighted": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "mvae_sum_over_time": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _vp]),
    "mvae_head": (_i32, [C.POINTER(HeadArgs), _vp]),
    "mvae_head_np": (_i32, [_i32]),
    "mvae_head_sample": (_i32, [C.POINTER(HeadSampleArgs), _vp]),
    "mvae_latent_fwd": (_i32, [C.POINTER(LatentFwdArgs), _vp]),
    "mvae_latent_bwd": (_i32, [C.POINTER(LatentBwdArgs), _vp]),
    "mvae_latent_chain_fwd": (_i32, [C.POINTER(LatentChainFwdArgs), _vp]),
    "mvae_latent_chain_bwd": (_i32, [C.POINTER(LatentChainBwdArgs), _vp]),
    "mvae_relayout": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "mvae_tanh_bwd": (_i32, [_vp, _vp, _vp, _sz, _vp]),
    "mvae_convert": (_i32, [_vp, _i32, _vp, _i32, _sz, _vp]),
    "mvae_make_table": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "mvae_transpose_convert": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "mvae_adam_step": (_i32, [_vp, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _i32, _f32, _vp]),
    "mvae_adam_step_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _vp, _f32, _i32, _vp, _vp]),
    "mvae_rmsprop_step": (_i32, [_vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _i32, _vp, _vp]),
    "mvae_scalars_accumulate": (_i32, [_vp, _vp, _i32, _f32, C.c_uint32, _vp]),
    "mvae_copy2d_f32": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "mvae_history_from_latent": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp]),
    "mvae_signature_head_fwd": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mvae_signature_head_bwd": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _vp]),
    "mvae_softmax_bwd_add": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "mvae_bi_concat": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "mvae_add_time_reversed": (_i32, [_vp, _vp, _vp, _i32, _i32, _sz, _vp]),
    "mvae_event_create": (_i32, [C.POINTER(_vp)]),
    "mvae_event_create_timed": (_i32, [C.POINTER(_vp)]),
    "mvae_event_elapsed_ms": (_i32, [_vp, _vp, C.POINTER(C.c_float)]),
    "mvae_event_destroy": (_i32, [_vp]),
    "mvae_event_record": (_i32, [_vp, _vp]),
    "mvae_event_synchronize": (_i32, [_vp]),
    "mvae_stream_wait_event": (_i32, [_vp, _vp]),
    "mvae_plan_create": (_i32, [C.POINTER(_vp)]),
    "mvae_plan_destroy": (_i32, [_vp]),
    "mvae_plan_add_call": (_i32, [_vp, C.c_char_p, C.POINTER(C.c_uint64), _i32]),
    "mvae_plan_set_blob": (_i32, [_vp, _i32, _i32, _vp, _sz]),
    "mvae_plan_add_patch": (_i32, [_vp, _i32, _i32, _i64, _i32, _i64]),
    "mvae_plan_run": (_i32, [_vp, _i32, _i32, C.POINTER(C.c_uint64), _i32]),
    "mvae_plan_size": (_i32, [_vp]),
    "mvae_plan_failed_call": (_i32, [_vp]),
    "mvae_host_threads": (_i32, [_i32]),
    "mvae_host_onehot_to_index_tm": (_i32, [_vp, _i32, _i64, _i32, _i32, _i64, _i64, _vp, _i32, C.c_uint8, C.POINTER(_i64)]),
    "mvae_host_index_to_tm": (_i32, [_vp, _i64, _i32, _i64, _i64, _vp, _i32, C.c_uint8]),
    "mvae_host_twohot_to_index_tm": (_i32, [_vp, _i32, _i64, _i32, _i32, _i32, _i64, _i64, _vp, _vp, _i32, C.c_uint8, C.POINTER(_i64)]),
    "mvae_host_rows_to_tm_f32": (_i32, [_vp, _i32, _i64, _i32, _i64, _i64, _f32, _vp, _i32]),
}

# the seven headers under include/: (what its message calls it, version symbol, version constant, signatures)
HEADERS = (("", "mvae_abi_version", ABI_VERSION, SIGNATURES),
           ("descriptor ", "mvae_desc_abi_version", DESC_ABI_VERSION, DESC_SIGNATURES),
           ("sweep ", "mvae_sweep_abi_version", SWEEP_ABI_VERSION, SWEEP_SIGNATURES),
           ("reconstruction ", "mvae_recon_abi_version", RECON_ABI_VERSION, RECON_SIGNATURES),
           ("note events ", "mvae_events_abi_version", EVENTS_ABI_VERSION, EVENTS_SIGNATURES),
           ("import ", "mvae_import_abi_version", IMPORT_ABI_VERSION, IMPORT_SIGNATURES),
           ("style ", "mvae_style_abi_version", STYLE_ABI_VERSION, STYLE_SIGNATURES))
# the headers after the seventh, checked by load() right behind HEADERS in the same way
LATER_HEADERS = (("generate ", "mvae_generate_abi_version", GENERATE_ABI_VERSION, GENERATE_SIGNATURES),)
# ... and the ninth (a tuple of its own: LATER_HEADERS stays what the eighth header's tests pin)
LONGSONG_HEADERS = (("long song ", "mvae_longsong_abi_version", LONGSONG_ABI_VERSION, LONGSONG_SIGNATURES),)

_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def load():
    """Load the C-ABI library once; raise HipLibraryMissing (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            "%s not found - build it with `make -C midi-vae_amd/csrc` (or __graft_entry__.build()); "
            "the MIDI-VAE engine has no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for what, version, want, signatures in HEADERS + LATER_HEADERS + LONGSONG_HEADERS:
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)      # AttributeError here = ABI drift between header and library
            fn.restype = res
            fn.argtypes = args
        have = getattr(lib, version)()
        if have != want:
            raise HipLibraryMissing("%sABI version mismatch: library %d, binding %d - rebuild with `make -C midi-vae_amd/csrc`"
                                    % (what, have, want))
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        raise RuntimeError("%s failed: %s" % (what, ERRORS.get(code, code)))


def ptr(t):
    """Device pointer of a torch tensor (or None -> NULL)."""
    return None if t is None else t.data_ptr()

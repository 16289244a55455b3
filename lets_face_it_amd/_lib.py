"""ctypes binding of liblfi_hip.so (the C ABI declared in include/lfi.h).

There is no CPU or PyTorch fallback: if the shared library is missing the import of
the compute path fails loudly, and every entry point raises on a non-zero status.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LFI_LIB_PATH") or os.path.join(_HERE, "liblfi_hip.so")  # override: kernel A/B experiments

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)


class GemmDesc(C.Structure):
    _fields_ = [
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("A", C.c_void_p), ("lda", C.c_long), ("a_kcontig", C.c_int),
        ("B", C.c_void_p), ("ldb", C.c_long), ("b_kcontig", C.c_int),
        ("C", C.c_void_p), ("ldc", C.c_long),
        ("bias", C.c_void_p),
        ("G", C.c_void_p), ("ldg", C.c_long),
        ("batch", C.c_int), ("strideA", C.c_long), ("strideB", C.c_long), ("strideC", C.c_long),
        ("strideBias", C.c_long), ("strideG", C.c_long),
        ("accumulate", C.c_int),
        ("act", C.c_int), ("slope", C.c_float),
        ("splitk", C.c_int), ("work", C.c_void_p),
        ("precision", C.c_int), ("a_bf16", C.c_int),
        ("colsum_part", C.c_void_p), ("ld_part", C.c_long),
    ]


class PGemmDesc(C.Structure):
    _fields_ = [
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("Ap", C.c_void_p), ("a_nkt", C.c_int), ("a_stride", C.c_long),
        ("Bp", C.c_void_p), ("b_nkt", C.c_int), ("b_stride", C.c_long),
        ("C", C.c_void_p), ("ldc", C.c_long),
        ("bias", C.c_void_p), ("G", C.c_void_p), ("ldg", C.c_long),
        ("batch", C.c_int), ("strideC", C.c_long), ("strideBias", C.c_long), ("strideG", C.c_long),
        ("accumulate", C.c_int), ("act", C.c_int), ("slope", C.c_float), ("skip", C.c_int),
        ("a_fmt", C.c_int), ("b_fmt", C.c_int),
        ("splitk", C.c_int), ("work", C.c_void_p),
        ("store_f32", C.c_int),
        ("Cr", C.c_void_p), ("cr_nkt", C.c_int), ("cr_col0", C.c_long),
        ("Gr", C.c_void_p), ("gr_nkt", C.c_int), ("gr_col0", C.c_long),
        ("colsum_part", C.c_void_p), ("ld_part", C.c_long),
        ("out_hi_only", C.c_int), ("tile", C.c_int),
        ("sign_out", C.c_void_p), ("sign_in", C.c_void_p),
    ]


class EncDesc(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("N", C.c_int), ("start", C.c_int),
                ("hist", C.c_int), ("hid", C.c_int), ("ldcond", C.c_int), ("col", C.c_int), ("precision", C.c_int),
                ("dup", C.c_int), ("lstm", C.c_int), ("bwd_two_products", C.c_int), ("stash_f16", C.c_int)]


class FlowDims(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("C", C.c_int), ("H", C.c_int), ("D", C.c_int), ("Ks", C.c_int),
                ("affine", C.c_int), ("lstm", C.c_int), ("scale_eps", C.c_float), ("gemm_precision", C.c_int)]


_FLOW_PARAM_FIELDS = ["an_bias", "an_logs", "inv_l", "inv_u", "inv_logs", "inv_p", "inv_sign", "inv_w",
                      "w_ih", "w_hh", "b_ih", "b_hh", "w_fl", "b_fl", "l_fl"]
_FLOW_GRAD_FIELDS = ["an_bias", "an_logs", "inv_l", "inv_u", "inv_logs", "inv_w",
                     "w_ih", "w_hh", "b_ih", "b_hh", "w_fl", "b_fl", "l_fl"]


class P1Enc(C.Structure):
    _fields_ = [("kind", C.c_int), ("hid", C.c_int), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w_ih", C.c_void_p),
                ("w_hh", C.c_void_p), ("b_ih", C.c_void_p), ("b_hh", C.c_void_p), ("col", C.c_int)]


class FlowParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _FLOW_PARAM_FIELDS]


class FlowGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _FLOW_GRAD_FIELDS]


class LfiError(RuntimeError):
    pass


_lib = None


def lib():
    """The loaded library; raises if liblfi_hip.so has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LfiError(
            "liblfi_hip.so not found at %s: build it with `make -C lets_face_it_amd/csrc` "
            "(there is no fallback path)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i, l, f, d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double
    P = C.POINTER
    sig = {
        "lfi_last_error": (C.c_char_p, []),
        "lfi_version": (i, []),
        "lfi_gemm_work_floats": (l, [P(GemmDesc)]),
        "lfi_gemm_f32": (i, [P(GemmDesc), vp]),
        "lfi_gemm_colpart_rows": (l, [P(GemmDesc)]),
        "lfi_planes_elems": (l, [l, i]),
        "lfi_planes_from_f32": (i, [vp, l, l, i, vp, vp]),
        "lfi_gemm_planes": (i, [P(PGemmDesc), vp]),
        "lfi_flow_bwd_emits_planes": (i, [P(FlowDims)]),
        "lfi_flow_walk_variant": (i, [P(FlowDims), i]),
        "lfi_flow_seq_bwd_planes": (i, [P(FlowDims), P(FlowParams), vp, vp, f, vp, vp, i, vp]),
        "lfi_encode_windows_grad_stash_bf16": (i, [P(EncDesc)]),
        "lfi_encode_windows_stash_f16_ok": (i, [P(EncDesc)]),
        "lfi_encode_windows_fwd_variant": (i, [P(EncDesc), i, i]),
        "lfi_gemm_planes_work_floats": (l, [P(PGemmDesc)]),
        "lfi_gemm_planes_colpart_rows": (l, [P(PGemmDesc)]),
        "lfi_planes_sign_words": (l, [l, l]),
        "lfi_gemm_planes_signs_ok": (i, [P(PGemmDesc)]),
        "lfi_gemm_planes_persist_grid": (l, [P(PGemmDesc)]),
        "lfi_colsum_work_floats": (l, [i, i, i]),
        "lfi_colsum_f32": (i, [vp, l, l, i, i, i, vp, l, f, i, vp, vp]),
        "lfi_cols_fold": (i, [vp, l, l, vp, vp, i, vp, l, vp]),
        "lfi_encode_windows_work_floats": (l, [P(EncDesc)]),
        "lfi_encode_windows_fwd": (i, [P(EncDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "lfi_encode_windows_bwd": (i, [P(EncDesc), vp, i, vp, vp, vp, vp, vp, vp, vp, vp]),
        "lfi_encode_windows_bias_rows": (l, [P(EncDesc)]),
        "lfi_encode_windows_bias_grads": (i, [vp, l, i, vp, vp, vp]),
        "lfi_encode_windows_compact_dgi": (i, [P(EncDesc)]),
        "lfi_encode_windows_scatter": (i, [P(EncDesc), vp, vp, vp, vp, vp]),
        "lfi_gather_windows": (i, [vp, i, i, i, i, i, i, i, vp, vp, i, i, vp]),
        "lfi_pad_rows": (i, [vp, l, i, l, vp, l, vp]),
        "lfi_dropout_masks": (i, [i, P(vp), P(l), P(f), C.c_ulonglong, C.c_ulonglong, vp]),
        "lfi_dropout_masks_dev": (i, [i, P(vp), P(l), P(f), vp, vp]),
        "lfi_set_step_params": (i, [vp, C.c_ulonglong, C.c_ulonglong, f, f, vp]),
        "lfi_adam_clip_step_dev": (i, [vp, vp, vp, vp, l, vp, f, f, f, f, f, vp, vp]),
        "lfi_leaky_grad": (i, [vp, l, vp, l, i, i, f, vp]),
        "lfi_fill_frame_nb": (i, [vp, f, i, i, vp, i, i, vp]),
        "lfi_flow_prep_floats": (l, [P(FlowDims)]),
        "lfi_flow_prep": (i, [P(FlowDims), P(FlowParams), vp, i, vp]),
        "lfi_flow_stash_floats": (l, [P(FlowDims)]),
        "lfi_flow_bstash_floats": (l, [P(FlowDims)]),
        "lfi_flow_stash_ptr": (vp, [P(FlowDims), vp, i]),
        "lfi_flow_bstash_ptr": (vp, [P(FlowDims), vp, i]),
        "lfi_flow_seq_fwd": (i, [P(FlowDims), P(FlowParams), vp, vp, i, i, vp, vp, vp, vp, vp]),
        "lfi_flow_seq_bwd": (i, [P(FlowDims), P(FlowParams), vp, vp, f, vp, vp]),
        "lfi_flow_param_grads_work_floats": (l, [P(FlowDims)]),
        "lfi_flow_param_grads": (i, [P(FlowDims), P(FlowParams), vp, vp, vp, vp, l, f, P(FlowGrads), i, vp, vp, vp]),
        "lfi_actnorm_init_stats": (i, [vp, i, i, vp, vp]),
        "lfi_actnorm_init_apply": (i, [vp, d, i, f, vp, vp, vp]),
        "lfi_flow_step": (i, [P(FlowDims), P(FlowParams), vp, i, i, vp, l, vp, vp, vp, vp, l, vp, vp, vp, i, vp]),
        "lfi_flow_seq_rev_ok": (i, [P(FlowDims)]),
        "lfi_flow_seq_rev_work_floats": (l, [P(FlowDims)]),
        "lfi_flow_seq_rev": (i, [P(FlowDims), P(FlowParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "lfi_flow_sample_work_floats": (l, [P(FlowDims)]),
        "lfi_flow_sample_p1_work_floats": (l, [P(FlowDims), P(P1Enc), i]),
        "lfi_flow_sample_seq": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, vp, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                    vp]),
        "lfi_flow_sample_seq_from": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                         vp]),
        "lfi_flow_sample_nll_work_floats": (l, [P(FlowDims)]),
        "lfi_flow_sample_seq_nll": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                        vp, vp, vp]),
        "lfi_flow_score_work_floats": (l, [P(FlowDims)]),
        "lfi_flow_score_seq_from": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                        vp, vp, vp, vp]),
        "lfi_flow_score_chunk_work_floats": (l, [P(FlowDims), P(P1Enc), i]),
        "lfi_flow_score_chunk_ok": (i, [P(FlowDims)]),
        "lfi_flow_frame_plan": (i, [P(FlowDims)]),
        "lfi_flow_score_seq_chunk": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                         vp, vp, vp, vp]),
        "lfi_flow_score_seq_chunk_rows": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                              vp, vp, vp, vp, vp]),
        "lfi_flow_step_rows_work_floats": (l, [P(FlowDims)]),
        "lfi_flow_step_rows_from": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                        vp, vp, vp, vp, vp]),
        "lfi_flow_step_rows_seq": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                       vp, vp, vp, vp, vp]),
        "lfi_flow_sample_cand_work_floats": (l, [P(FlowDims), i]),
        "lfi_flow_sample_cand_from": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                          vp, vp, i, vp, vp, vp, vp, vp, vp]),
        "lfi_stream_commit_cand": (i, [i, i, i, i, i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp]),
        "lfi_flow_sample_cand_seq_work_floats": (l, [P(FlowDims), i]),
        "lfi_flow_sample_cand_seq": (i, [P(FlowDims), P(FlowParams), vp, vp, l, i, vp, vp, vp, i, i, i, i, vp, vp, P(P1Enc), vp, vp,
                                         vp, vp, i, vp]),
        "lfi_stream_cand_seq_in": (i, [i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp]),
        "lfi_stream_commit_cand_seq": (i, [i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]),
        "lfi_absmax_f32": (i, [i, P(vp), P(l), vp, vp]),
        "lfi_stream_advance": (i, [i, i, P(vp), P(vp), P(i), P(i), vp, vp, i, vp, vp, vp]),
        "lfi_stream_advance_rows": (i, [i, i, P(vp), P(vp), P(i), P(i), i, vp, vp, i, vp, vp, vp, vp, vp]),
        "lfi_stream_chunk_in": (i, [i, i, i, i, P(vp), P(vp), P(vp), P(i), P(i), P(i), vp, vp]),
        "lfi_stream_chunk_out": (i, [i, i, i, i, P(vp), P(vp), P(i), P(i), P(i), vp, vp]),
        "lfi_stream_chunk_in_rows": (i, [i, i, i, i, P(vp), P(vp), P(vp), P(i), P(i), P(i), vp, vp, vp]),
        "lfi_stream_chunk_out_rows": (i, [i, i, i, i, P(vp), P(vp), P(i), P(i), P(i), vp, vp, vp]),
        "lfi_stream_chunk_gen_in": (i, [i, i, i, i, P(vp), P(vp), P(vp), P(i), P(i), P(i), i, vp, i, vp, vp]),
        "lfi_stream_chunk_gen_out": (i, [i, i, i, i, P(vp), P(vp), P(i), P(i), P(i), i, vp, l, vp, vp, vp]),
        "lfi_stream_chunk_roles_in": (i, [i, i, i, i, P(vp), P(vp), P(vp), P(i), P(i), P(i), i, vp, i, vp, vp, vp]),
        "lfi_stream_reset_rows": (i, [i, i, P(i), i, P(vp), P(vp), P(l), P(i), P(i), P(i), vp, vp, i, i, vp, vp, vp]),
        "lfi_stream_row_floats": (l, [i, P(i), P(i), i, i, i, i]),
        "lfi_stream_save_rows": (i, [i, i, P(i), i, P(vp), P(i), P(i), vp, vp, i, i, vp, i, vp, l, vp]),
        "lfi_stream_load_rows": (i, [i, i, P(i), P(i), i, i, P(vp), P(i), P(i), vp, vp, i, i, vp, vp, l, vp, vp]),
        "lfi_stream_create_partial": (i, [i, P(vp)]),
        "lfi_stream_destroy": (i, [vp]),
        "lfi_grad_sumsq": (i, [vp, l, vp, vp, vp]),
        "lfi_adam_clip_step": (i, [vp, vp, vp, vp, l, vp, f, f, f, f, f, f, i, vp]),
        "lfi_adam_clip_step_ex": (i, [vp, vp, vp, vp, vp, l, vp, f, f, f, f, f, f, f, i, vp, vp]),
        "lfi_sgd_clip_step": (i, [vp, vp, vp, l, vp, f, f, f, f, f, f, i, i, vp]),
        "lfi_rmsprop_clip_step": (i, [vp, vp, vp, vp, vp, l, vp, f, f, f, f, f, f, f, vp]),
        "lfi_ema_update": (i, [vp, vp, l, f, vp]),
        "lfi_grad_guard": (i, [vp, l, vp, vp, vp, f, i, f, f, f, f, C.c_ulonglong, vp]),
        "lfi_grad_guard_dev": (i, [vp, l, vp, vp, vp, f, i, f, f, vp, vp]),
        "lfi_adam_clip_step_guard": (i, [vp, vp, vp, vp, vp, l, vp, f, f, f, f, f, f, vp, vp]),
        "lfi_sgd_clip_step_guard": (i, [vp, vp, vp, l, vp, f, f, f, f, f, f, i, vp, vp]),
        "lfi_rmsprop_clip_step_guard": (i, [vp, vp, vp, vp, vp, l, vp, f, f, f, f, f, f, f, vp, vp]),
        "lfi_ema_update_guard": (i, [vp, vp, l, f, vp, vp]),
        "lfi_set_step_params_t": (i, [vp, C.c_ulonglong, C.c_ulonglong, f, f, C.c_ulonglong, vp]),
        "lfi_segment_stats_chunk": (l, []),
        "lfi_segment_stats_work_floats": (l, [l, i, i, P(l)]),
        "lfi_segment_stats": (i, [vp, l, vp, i, i, P(vp), P(l), vp, vp, vp]),
        "lfi_segment_stats_guard": (i, [vp, l, vp, i, i, P(vp), P(l), vp, vp, vp, vp]),
        "lfi_actnorm_forward": (i, [vp, i, i, vp, vp, i, vp, vp, vp]),
        "lfi_invconv_work_floats": (l, [i]),
        "lfi_invconv_weights": (i, [i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp]),
        "lfi_row_noise": (i, [vp, i, i, i, i, f, vp, l, l, l, i, vp]),
        "lfi_row_rng_advance": (i, [vp, i, l, vp, vp]),
        "lfi_row_rng_seed_rows": (i, [vp, i, i, P(i), P(C.c_ulonglong), P(C.c_ulonglong), vp]),
        "lfi_row_rng_save_rows": (i, [vp, i, i, P(i), vp, vp]),
        "lfi_row_rng_load_rows": (i, [vp, i, i, P(i), P(i), i, vp, P(C.c_ulonglong), vp]),
        "lfi_gather_sequences": (i, [vp, l, i, vp, i, i, vp, vp]),
        "lfi_jerk_mean": (i, [vp, i, i, i, vp, vp, vp]),
        "lfi_selftest_mfma": (i, [vp, vp]),
        "lfi_debug_set_stamps": (i, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = header and library out of sync
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTS = [
    "lfi_last_error", "lfi_version", "lfi_gemm_work_floats", "lfi_gemm_f32", "lfi_gemm_colpart_rows", "lfi_planes_elems", "lfi_planes_from_f32",
    "lfi_gemm_planes", "lfi_gemm_planes_work_floats", "lfi_gemm_planes_colpart_rows", "lfi_planes_sign_words", "lfi_gemm_planes_signs_ok", "lfi_gemm_planes_persist_grid",
    "lfi_flow_bwd_emits_planes", "lfi_flow_walk_variant", "lfi_flow_seq_bwd_planes", "lfi_encode_windows_grad_stash_bf16", "lfi_encode_windows_stash_f16_ok", "lfi_encode_windows_fwd_variant", "lfi_colsum_work_floats",
    "lfi_colsum_f32", "lfi_cols_fold", "lfi_encode_windows_work_floats", "lfi_encode_windows_fwd", "lfi_encode_windows_bwd",
    "lfi_encode_windows_bias_rows", "lfi_encode_windows_bias_grads",
    "lfi_encode_windows_scatter", "lfi_encode_windows_compact_dgi", "lfi_gather_windows", "lfi_pad_rows", "lfi_dropout_masks", "lfi_leaky_grad", "lfi_fill_frame_nb", "lfi_flow_prep_floats", "lfi_flow_prep",
    "lfi_flow_stash_floats", "lfi_flow_bstash_floats", "lfi_flow_stash_ptr", "lfi_flow_bstash_ptr",
    "lfi_flow_seq_fwd", "lfi_flow_seq_bwd", "lfi_flow_param_grads_work_floats", "lfi_flow_param_grads",
    "lfi_actnorm_init_stats", "lfi_actnorm_init_apply", "lfi_flow_step", "lfi_flow_seq_rev_ok", "lfi_flow_seq_rev_work_floats",
    "lfi_flow_seq_rev", "lfi_flow_sample_work_floats",
    "lfi_flow_sample_p1_work_floats", "lfi_flow_sample_seq", "lfi_flow_sample_seq_from", "lfi_flow_sample_nll_work_floats", "lfi_flow_sample_seq_nll", "lfi_flow_score_work_floats", "lfi_flow_score_seq_from",
    "lfi_flow_score_chunk_work_floats", "lfi_flow_score_chunk_ok", "lfi_flow_frame_plan", "lfi_flow_score_seq_chunk", "lfi_stream_chunk_in", "lfi_stream_chunk_out",
    "lfi_stream_chunk_gen_in", "lfi_stream_chunk_gen_out",
    "lfi_flow_score_seq_chunk_rows", "lfi_stream_chunk_in_rows", "lfi_stream_chunk_out_rows",
    "lfi_flow_step_rows_seq", "lfi_stream_chunk_roles_in",
    "lfi_flow_sample_cand_work_floats", "lfi_flow_sample_cand_from", "lfi_stream_commit_cand",
    "lfi_flow_sample_cand_seq_work_floats", "lfi_flow_sample_cand_seq", "lfi_stream_cand_seq_in", "lfi_stream_commit_cand_seq",
    "lfi_flow_step_rows_work_floats", "lfi_flow_step_rows_from", "lfi_absmax_f32", "lfi_stream_advance", "lfi_stream_advance_rows", "lfi_stream_reset_rows", "lfi_stream_row_floats",
    "lfi_stream_save_rows", "lfi_stream_load_rows", "lfi_stream_create_partial", "lfi_stream_destroy", "lfi_grad_sumsq", "lfi_adam_clip_step", "lfi_adam_clip_step_ex",
    "lfi_sgd_clip_step", "lfi_rmsprop_clip_step", "lfi_ema_update", "lfi_set_step_params", "lfi_dropout_masks_dev", "lfi_adam_clip_step_dev", "lfi_selftest_mfma", "lfi_debug_set_stamps",
    "lfi_gather_sequences", "lfi_jerk_mean", "lfi_actnorm_forward", "lfi_invconv_work_floats", "lfi_invconv_weights",
    "lfi_grad_guard", "lfi_grad_guard_dev", "lfi_adam_clip_step_guard", "lfi_sgd_clip_step_guard", "lfi_rmsprop_clip_step_guard",
    "lfi_ema_update_guard", "lfi_set_step_params_t",
    "lfi_segment_stats_chunk", "lfi_segment_stats_work_floats", "lfi_segment_stats", "lfi_segment_stats_guard",
    "lfi_row_noise", "lfi_row_rng_advance", "lfi_row_rng_seed_rows", "lfi_row_rng_save_rows", "lfi_row_rng_load_rows",
]

# slots of the non-finite step guard's device record (include/lfi.h, LFI_GUARD_*): 8 bytes each
GUARD_SKIPPED, GUARD_CONSECUTIVE, GUARD_APPLIED, GUARD_LAST_NORM, GUARD_MAX_NORM = 0, 1, 2, 3, 4
GUARD_APPLY, GUARD_STEP_FLOATS, GUARD_MOMENTUM_LIVE, GUARD_AVERAGE_LIVE, GUARD_SLOTS = 5, 6, 7, 8, 9
# slots of one per-array record of lfi_segment_stats (LFI_SEG_*) and of the blame record's header in front of them (LFI_BLAME_*)
SEG_SUMSQ, SEG_NAN, SEG_INF, SEG_FIRST, SEG_SLOTS = 0, 1, 2, 3, 4
BLAME_FILLED, BLAME_STEP, BLAME_HEAD = 0, 1, 2
SEG_NONE = 2 ** 64 - 1      # FIRST of an array without a non-finite element
SEG_MAX_EXTRA = 8


def translate_oom(fn):
    """Decorator for the engine's entry points. The reference's Optuna harness halves the batch size when a trial dies with
    a RuntimeError whose text starts with "CUDA out of memory" (hparams_tuning.py:162-166,194-199); PyTorch-ROCm words
    its allocator error "HIP out of memory...", which that test would silently miss. Re-raise it in the expected wording
    (torch.OutOfMemoryError is a RuntimeError subclass, and so is this)."""
    import functools

    import torch

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        try:
            return fn(*args, **kwargs)
        except torch.OutOfMemoryError as e:
            msg = str(e)
            if msg.startswith("CUDA out of memory"):
                raise
            raise torch.OutOfMemoryError("CUDA out of memory. [ROCm: " + msg + "]") from e

    return wrapper


def check(rc, what=""):
    if rc != 0:
        msg = lib().lfi_last_error()
        raise LfiError("%s failed (%d): %s" % (what or "lfi call", rc, msg.decode() if msg else ""))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()

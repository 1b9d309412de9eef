"""ctypes binding of libhual_seqpan.so (include/hual_seqpan.h).  No fallback: a missing or stale
library raises - the product path never routes through a CPU implementation."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HUAL_LIB_PATH: an experiment build of the library (scripts/exp/tl_variant.sh) - the in-tree file is never overwritten
LIB_PATH = os.environ.get('HUAL_LIB_PATH') or os.path.join(_HERE, 'libhual_seqpan.so')
ABI_VERSION = 9

_lib = None


class HualError(RuntimeError):
    pass


class hual_cfg(ctypes.Structure):
    _fields_ = [('vdim', ctypes.c_int32), ('dim', ctypes.c_int32), ('num_heads', ctypes.c_int32),
                ('word_dim', ctypes.c_int32), ('char_dim', ctypes.c_int32), ('max_vlen', ctypes.c_int32),
                ('attn_layer', ctypes.c_int32), ('num_chars', ctypes.c_int32), ('num_words', ctypes.c_int32),
                ('no_gumbel', ctypes.c_int32), ('match_lambda', ctypes.c_float), ('tau', ctypes.c_float),
                ('clip_norm', ctypes.c_float), ('finetune_word_emb', ctypes.c_int32)]


class hual_param_entry(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char * 112), ('offset', ctypes.c_uint64), ('size', ctypes.c_uint64),
                ('ndim', ctypes.c_int32), ('shape', ctypes.c_int32 * 4), ('decay', ctypes.c_int32)]


class hual_batch(ctypes.Structure):
    _fields_ = [('video', ctypes.c_void_p), ('video_seq_len', ctypes.c_void_p), ('word_ids', ctypes.c_void_p),
                ('char_ids', ctypes.c_void_p), ('B', ctypes.c_int32), ('T', ctypes.c_int32), ('L', ctypes.c_int32),
                ('C', ctypes.c_int32), ('video_dtype', ctypes.c_int32)]


class hual_labels(ctypes.Structure):
    _fields_ = [('y1', ctypes.c_void_p), ('y2', ctypes.c_void_p), ('match_labels', ctypes.c_void_p),
                ('inner_labels', ctypes.c_void_p)]


class hual_outputs(ctypes.Structure):
    _fields_ = [('start_logits', ctypes.c_void_p), ('end_logits', ctypes.c_void_p), ('match_scores', ctypes.c_void_p),
                ('start_index', ctypes.c_void_p), ('end_index', ctypes.c_void_p), ('loss_terms', ctypes.c_void_p)]


class hual_run_opts(ctypes.Structure):
    _fields_ = [('drop_rate', ctypes.c_float), ('rng_state', ctypes.c_void_p), ('match_denom_override', ctypes.c_float),
                ('align_external', ctypes.c_int32), ('static_tables', ctypes.c_int32),
                ('match_denom_dev', ctypes.c_void_p), ('debug_taps', ctypes.c_int32), ('grads_prezero', ctypes.c_void_p),
                ('prezero_token', ctypes.c_void_p), ('deferred_loss_terms', ctypes.c_void_p),
                ('dw_table', ctypes.c_void_p), ('dw_table_bytes', ctypes.c_uint64)]


class hual_al_set(ctypes.Structure):
    _fields_ = [('N', ctypes.c_int32), ('ld', ctypes.c_int32), ('vlen', ctypes.c_void_p), ('tlen', ctypes.c_void_p),
                ('ap_off', ctypes.c_void_p), ('ap_idx', ctypes.c_void_p), ('ap_pos', ctypes.c_void_p)]


class hual_al_bank(ctypes.Structure):
    _fields_ = [('N', ctypes.c_int32), ('ld', ctypes.c_int32), ('tlen', ctypes.c_void_p), ('s0', ctypes.c_void_p), ('e0', ctypes.c_void_p),
                ('lo_s', ctypes.c_void_p), ('hi_s', ctypes.c_void_p), ('mean_s', ctypes.c_void_p), ('m2_s', ctypes.c_void_p),
                ('lo_e', ctypes.c_void_p), ('hi_e', ctypes.c_void_p), ('mean_e', ctypes.c_void_p), ('m2_e', ctypes.c_void_p)]


class hual_al_info(ctypes.Structure):
    _fields_ = [('ent_s', ctypes.c_void_p), ('ent_e', ctypes.c_void_p)]


AL_STAT = {'range': 0, 'std': 1}      # HUAL_AL_STAT_RANGE / HUAL_AL_STAT_STD: hual_al_score_mc
# HUAL_AL_STAT_BALD / _ENTROPY / _EXPECTED_ENTROPY: hual_al_score_info, from a bank that also folds the passes' entropy (hual_al_info)
AL_STAT_INFO = {'bald': 2, 'entropy': 3, 'expected_entropy': 4}


class hual_dataset(ctypes.Structure):
    _fields_ = [('feat_bank', ctypes.c_void_p), ('feat_off', ctypes.c_void_p), ('vdim', ctypes.c_int32),
                ('sample_vid', ctypes.c_void_p), ('word_off', ctypes.c_void_p), ('word_bank', ctypes.c_void_p),
                ('char_off', ctypes.c_void_p), ('char_bank', ctypes.c_void_p), ('s_ind', ctypes.c_void_p),
                ('e_ind', ctypes.c_void_p)]


class hual_soft_labels(ctypes.Structure):
    _fields_ = [('y1', ctypes.c_void_p), ('y2', ctypes.c_void_p), ('w', ctypes.c_void_p), ('ld', ctypes.c_int32)]


class hual_ws_entry(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char * 48), ('offset', ctypes.c_uint64), ('rows', ctypes.c_uint64),
                ('cols', ctypes.c_uint64)]


def load():
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its wheel bundles its own libamdhip64, and a process must end up with ONE HIP runtime - if this library
    # were loaded before torch it would bind /opt/rocm's copy and its launches would not see torch's device context
    # ("no ROCm-capable device is detected")
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise HualError('%s not found: build it with `python -m hual_amd.build` (or __graft_entry__.build())' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.hual_abi_version.restype = ctypes.c_int
    lib.hual_last_error.restype = ctypes.c_char_p
    v = lib.hual_abi_version()
    if v != ABI_VERSION:
        raise HualError('libhual_seqpan.so ABI %d != python binding %d: rebuild' % (v, ABI_VERSION))
    lib.hual_cfg_bytes.restype = ctypes.c_uint64
    if lib.hual_cfg_bytes() != ctypes.sizeof(hual_cfg):
        raise HualError('libhual_seqpan.so hual_cfg is %d bytes, python binding %d: rebuild' % (lib.hual_cfg_bytes(), ctypes.sizeof(hual_cfg)))
    lib.hual_seqpan_dw_table_bytes.restype = ctypes.c_uint64
    vp, i32, u64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_float
    P = ctypes.POINTER
    lib.hual_seqpan_validate.argtypes = [P(hual_cfg)]
    lib.hual_seqpan_param_count.argtypes = [P(hual_cfg), P(u64), P(u64)]
    lib.hual_seqpan_param_table.argtypes = [P(hual_cfg), P(hual_param_entry), i32]
    lib.hual_seqpan_query_workspace.argtypes = [P(hual_cfg), i32, i32, i32, i32, P(u64)]
    lib.hual_seqpan_ws_table.argtypes = [P(hual_cfg), i32, i32, i32, i32, P(hual_ws_entry), i32]
    lib.hual_seqpan_forward.argtypes = [P(hual_cfg), vp, vp, P(hual_batch), P(hual_labels), P(hual_outputs),
                                        P(hual_run_opts), vp, u64, vp]
    lib.hual_seqpan_backward.argtypes = [P(hual_cfg), vp, vp, P(hual_batch), P(hual_labels), P(hual_run_opts), vp, vp,
                                         u64, vp]
    lib.hual_adamw_clip_step.argtypes = [vp, vp, vp, vp, vp, u64, vp, f32, f32, vp, vp]
    lib.hual_adamw_clip_step_rng.argtypes = [vp, vp, vp, vp, vp, u64, vp, f32, f32, vp, vp, vp]
    lib.hual_adamw_clip_step_loop.argtypes = [vp, vp, vp, vp, vp, u64, vp, f32, f32, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.hual_adamw_clip_step_ema.argtypes = [vp, vp, vp, vp, vp, u64, vp, f32, f32, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, f32, i32, vp]
    lib.hual_assemble_batch_cursor.argtypes = [P(hual_dataset), vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.hual_xgmi_flags_bytes.restype = ctypes.c_uint64
    lib.hual_xgmi_flags_alloc.argtypes = [P(vp)]
    lib.hual_xgmi_flags_free.argtypes = [vp]
    lib.hual_xgmi_ipc_export.argtypes = [vp, vp, P(u64)]
    lib.hual_xgmi_ipc_open.argtypes = [vp, P(vp)]
    lib.hual_xgmi_ipc_close.argtypes = [vp]
    lib.hual_xgmi_allreduce.argtypes = [i32, i32, P(vp), P(vp), P(vp), vp, vp, u64, u64, vp]
    lib.hual_align_loss.argtypes = [vp, vp, i32, vp, vp, vp, vp, f32, vp]
    lib.hual_align_loss_rows.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, f32, vp]
    blk = [P(hual_cfg), vp, P(hual_batch), P(hual_run_opts)]
    lib.hual_video_proj_ln_fwd.argtypes = [P(hual_cfg), vp, vp, P(hual_batch), P(hual_run_opts), vp, vp, u64, vp]
    lib.hual_input_bwd.argtypes = [P(hual_cfg), vp, vp, P(hual_batch), P(hual_run_opts), vp, vp, vp, u64, vp]
    lib.hual_conv_block_fwd.argtypes = blk + [vp, vp, vp, u64, vp]
    lib.hual_conv_block_bwd.argtypes = blk + [vp, vp, vp, vp, u64, vp]
    lib.hual_dual_attn_fwd.argtypes = blk + [i32, vp, vp, vp, u64, vp]
    lib.hual_dual_attn_bwd.argtypes = blk + [i32, vp, vp, vp, vp, u64, vp]
    lib.hual_cq_attn_fwd.argtypes = blk + [vp, vp, vp, u64, vp]
    lib.hual_cq_attn_bwd.argtypes = blk + [vp, vp, vp, vp, u64, vp]
    lib.hual_fuse_fwd.argtypes = blk + [P(hual_labels), vp, vp, vp, vp, vp, vp, u64, vp]
    lib.hual_fuse_bwd.argtypes = blk + [P(hual_labels), vp, vp, vp, vp, vp, u64, vp]
    lib.hual_localizing_loss.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    lib.hual_predictor_fwd.argtypes = blk + [vp, vp, vp, vp, vp, vp, u64, vp]
    lib.hual_predictor_bwd.argtypes = blk + [vp, vp, vp, vp, vp, u64, vp]
    lib.hual_prof_get.argtypes = [i32, ctypes.c_char_p, i32, P(ctypes.c_int64), P(ctypes.c_double), P(ctypes.c_double),
                                  P(ctypes.c_double)]
    lib.hual_prof_kernel_pipe.argtypes = [ctypes.c_char_p, P(i32), P(i32)]
    lib.hual_linear_bf16x3.argtypes = [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, u64, vp]
    lib.hual_layer_norm_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp]
    lib.hual_attention_fwd.argtypes = [vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.hual_attention_fwd_save.argtypes = [vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, f32, i32, vp]
    lib.hual_attention_bwd.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp,
                                       vp, f32, i32, vp]
    lib.hual_attention_keep_row_bytes.argtypes = [i32]
    lib.hual_span_argmax.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    lib.hual_span_topk.argtypes = [vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp]
    lib.hual_span_expected_iou.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.hual_span_hit_prob.argtypes = [vp, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.hual_span_hit_cover.argtypes = [vp, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, i32, f32, vp, vp, vp, vp]
    lib.hual_linear_dw.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, vp, u64, vp]
    lib.hual_al_score.argtypes = [P(hual_al_set), vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp]
    lib.hual_al_mc_fold.argtypes = [P(hual_al_bank), vp, vp, vp, vp, i32, i32, i32, vp]
    lib.hual_al_score_mc.argtypes = [P(hual_al_set), vp, vp, P(hual_al_bank), i32, i32, f32, vp, vp, vp, vp, vp, vp, vp]
    lib.hual_al_mc_fold_info.argtypes = [P(hual_al_bank), P(hual_al_info), vp, vp, vp, vp, i32, i32, i32, vp]
    lib.hual_al_score_info.argtypes = [P(hual_al_set), vp, vp, P(hual_al_bank), P(hual_al_info), i32, i32, f32, vp, vp, vp, vp, vp, vp, vp]
    lib.hual_al_renew.argtypes = [P(hual_al_set), vp, i32, vp, vp, vp, P(ctypes.c_double), vp, vp]
    lib.hual_al_query.argtypes = [P(hual_al_set), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.hual_al_mbr_label.argtypes = [P(hual_al_set), vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.hual_al_label_gain.argtypes = [P(hual_al_set), vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.hual_al_hit_label.argtypes = [P(hual_al_set), vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.hual_assemble_batch.argtypes = [P(hual_dataset), vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.hual_assemble_batch_carry.argtypes = [P(hual_dataset), vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.hual_al_span_marginals.argtypes = [P(hual_al_set), vp, vp, vp, vp, vp, vp]
    lib.hual_al_noisy_tilt.argtypes = [P(hual_al_set), vp, vp, f32, vp, vp, vp, vp]
    lib.hual_al_label_gain_noisy.argtypes = [P(hual_al_set), vp, vp, f32, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.hual_al_session.argtypes = [P(hual_al_set), vp, vp, vp, vp, i32, i32, vp, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.hual_al_session_label.argtypes = ([P(hual_al_set), vp, vp, vp, vp, i32, i32, vp, f32, f32, f32, vp, vp, i32, i32, f32] + [vp] * 10
                                          + [vp])
    lib.hual_al_design.argtypes = [P(hual_al_set), vp, vp, vp, i32, i32, vp, f32, f32, vp, vp, vp, vp, vp, vp]
    lib.hual_al_evidence_grid.argtypes = [P(hual_al_set), vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.hual_al_ensemble_query.argtypes = [P(hual_al_set), vp, vp, i32, vp] + [vp] * 12 + [vp]
    lib.hual_al_ensemble_label.argtypes = [P(hual_al_set), vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.hual_assemble_batch_soft.argtypes = lib.hual_assemble_batch_carry.argtypes[:-1] + [P(hual_soft_labels), vp]
    lib.hual_assemble_batch_cursor_soft.argtypes = lib.hual_assemble_batch_cursor.argtypes[:-1] + [P(hual_soft_labels), vp]
    lib.hual_clip_mean_features.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp]
    lib.hual_kcenter_workspace_bytes.restype = ctypes.c_uint64
    lib.hual_kcenter_workspace_bytes.argtypes = [i32]
    lib.hual_kcenter_greedy.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, u64, vp]
    lib.hual_kcenter_sample.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, u64, ctypes.c_uint32, i32, i32, vp, vp, vp, vp, vp, u64, vp]
    lib.hual_al_grad_embed.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp]
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise HualError('libhual_seqpan: %s (code %d)' % (load().hual_last_error().decode(), code))


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _addr(t):
    return None if t is None else t.data_ptr()


def batch_struct(video, video_seq_len, word_ids, char_ids):
    """hual_batch over device tensors: video [B,T,V] float32 or bfloat16 (-> video_dtype), word_ids [B,L], char_ids [B,L,C]"""
    import torch
    (B, T), L, C = video.shape[:2], word_ids.shape[1], char_ids.shape[2]
    return hual_batch(_addr(video), _addr(video_seq_len), _addr(word_ids), _addr(char_ids), B, T, L, C,
                      1 if video.dtype == torch.bfloat16 else 0)


def labels_struct(y1, y2, match_labels, inner_labels):
    return hual_labels(_addr(y1), _addr(y2), _addr(match_labels), _addr(inner_labels))


def outputs_struct(start_logits, end_logits, match_scores, start_index, end_index, loss_terms=None):
    """hual_outputs over device tensors (loss_terms None: a forward without labels)"""
    return hual_outputs(_addr(start_logits), _addr(end_logits), _addr(match_scores), _addr(start_index), _addr(end_index),
                        _addr(loss_terms))


def stream_ptr(stream=None):
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    return ctypes.c_void_p(s.cuda_stream)


# ---------------------------------------------------------------- host-only queries (no GPU needed)
def make_cfg(**kw):
    c = hual_cfg()
    d = dict(vdim=1024, dim=128, num_heads=8, word_dim=300, char_dim=50, max_vlen=64, attn_layer=2, num_chars=40,
             num_words=500, no_gumbel=1, match_lambda=1.0, tau=0.3, clip_norm=1.0, finetune_word_emb=0)
    d.update(kw)
    for k, v in d.items():
        setattr(c, k, v)
    return c


def param_table(cfg):
    lib = load()
    n = lib.hual_seqpan_param_table(ctypes.byref(cfg), None, 0)
    if n < 0:
        check(n)
    arr = (hual_param_entry * n)()
    n2 = lib.hual_seqpan_param_table(ctypes.byref(cfg), arr, n)
    assert n2 == n
    total, count = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.hual_seqpan_param_count(ctypes.byref(cfg), ctypes.byref(total), ctypes.byref(count)))
    ents = [dict(name=e.name.decode(), offset=int(e.offset), size=int(e.size), shape=list(e.shape[:e.ndim]),
                 decay=bool(e.decay)) for e in arr]
    return ents, int(total.value), int(count.value)


def query_workspace(cfg, B, T, L, C):
    b = ctypes.c_uint64()
    check(load().hual_seqpan_query_workspace(ctypes.byref(cfg), B, T, L, C, ctypes.byref(b)))
    return int(b.value)


def ws_table(cfg, B, T, L, C):
    lib = load()
    n = lib.hual_seqpan_ws_table(ctypes.byref(cfg), B, T, L, C, None, 0)
    if n < 0:
        check(n)
    arr = (hual_ws_entry * n)()
    lib.hual_seqpan_ws_table(ctypes.byref(cfg), B, T, L, C, arr, n)
    return {e.name.decode(): (int(e.offset), int(e.rows), int(e.cols)) for e in arr}


# ---------------------------------------------------------------- per-kernel entry points
def linear_bf16x3(A, W, bias=None, act=0, trans_w=False):
    """split-bf16 dense: W [K,128] (trans_w False) or [N,128] used transposed (dX)"""
    import torch
    M, K = A.shape
    N = W.shape[0] if trans_w else W.shape[1]
    Y = torch.empty(M, N, device=A.device, dtype=torch.float32)
    nbytes = ((N + 127) // 128) * 65536 if trans_w else ((K + 127) // 128) * 65536
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=A.device)
    check(load().hual_linear_bf16x3(ptr(A), A.stride(0), ptr(W), int(trans_w), ptr(bias), ptr(Y), Y.stride(0), M, K, N, act,
                                    ptr(scratch), nbytes, stream_ptr()))
    return Y


def linear_dw(A, dY, dW, db=None, workgroups=0):
    M, K = A.shape
    N = dY.shape[1]
    import torch
    scratch = torch.empty(256, dtype=torch.float32, device=A.device)
    check(load().hual_linear_dw(ptr(A), A.stride(0), ptr(dY), dY.stride(0), ptr(dW), dW.stride(0), ptr(db), M, K, N,
                                workgroups, ptr(scratch), 1024, stream_ptr()))


def _clip_logits(who, start_logits, end_logits):
    import torch
    if start_logits.dtype != torch.float32 or end_logits.dtype != torch.float32:
        raise HualError(who + ': float32 logits required')
    if start_logits.dim() != 2 or end_logits.shape != start_logits.shape:
        raise HualError(who + ': start / end logits must both be [B,T]')


def _clip_lengths(who, start_logits, end_logits, video_seq_len):
    import torch
    s, e = start_logits.contiguous(), end_logits.contiguous()
    B, T = s.shape
    vl = video_seq_len.to(device=s.device, dtype=torch.int32).contiguous()
    if vl.numel() != B:
        raise HualError(who + ': video_seq_len must hold B = %d lengths' % B)
    return s, e, vl, B, T


def _clip_inputs(who, start_logits, end_logits, video_seq_len):
    """the gate of every per-clip span launch -> (s, e, vl, B, T), the logits contiguous, the lengths int32 on their device"""
    _clip_logits(who, start_logits, end_logits)
    return _clip_lengths(who, start_logits, end_logits, video_seq_len)


def _clip_slots(who, starts, ends, score, B, dev):
    """the gate of the proposal slots starts / ends int64 [B,k] and score float32 [B,k] or None -> k.  No .contiguous() here: a
    reorder writes them in place, and a copy would take the permutation with it"""
    import torch
    if starts.dim() != 2 or starts.shape[0] != B:
        raise HualError(who + ': starts / ends must be [B,k] with B = %d' % B)
    k = int(starts.shape[1])
    for x, dt, what in ((starts, torch.int64, 'starts'), (ends, torch.int64, 'ends'), (score, torch.float32, 'score')):
        if x is not None and (x.dtype != dt or tuple(x.shape) != (B, k) or not x.is_contiguous() or x.device != dev):
            raise HualError(who + ': %s must be a contiguous [B,k] %s tensor on the logits\' device' % (what, str(dt).replace('torch.', '')))
    return k


def span_topk(start_logits, end_logits, video_seq_len, k, max_len=0, nms_iou=1.0, out=None):
    """the k best spans of each clip after greedy temporal NMS (hual_span_topk): start_logits / end_logits f32 [B,T] and
    video_seq_len [B] on the device -> (start [B,k] int64, end [B,k] int64, score [B,k] float32), enqueued on the current stream.
    Slots no candidate fills are -1 (score -1.0).  out: three contiguous device tensors of those shapes to write into instead."""
    import torch
    s, e, vl, B, T = _clip_inputs('span_topk', start_logits, end_logits, video_seq_len)
    k = int(k)
    if out is None:
        out = (torch.empty(B, k, dtype=torch.int64, device=s.device), torch.empty(B, k, dtype=torch.int64, device=s.device),
               torch.empty(B, k, dtype=torch.float32, device=s.device))
    else:
        for o, dt in zip(out, (torch.int64, torch.int64, torch.float32)):
            if o.dtype != dt or tuple(o.shape) != (B, k) or not o.is_contiguous():
                raise HualError('span_topk: out tensors must be contiguous [B,k] int64, int64, float32')
    check(load().hual_span_topk(ptr(s), ptr(e), ptr(vl), B, T, k, int(max_len), ctypes.c_float(nms_iou), ptr(out[0]), ptr(out[1]),
                                ptr(out[2]), stream_ptr()))
    return out


def span_expected_iou(start_logits, end_logits, video_seq_len, starts, ends, score=None, reorder=False, entropy=True, out=None):
    """expected temporal IoU of the proposals starts / ends (int64 [B,k] on the device, k <= 16; -1 = no proposal) under the span
    distribution of start_logits / end_logits f32 [B,T] and video_seq_len [B], and that distribution's entropy in bits
    (hual_span_expected_iou) -> (expected_iou [B,k] float32, span_entropy [B] float32 or None with entropy=False), enqueued on the
    current stream.  Invalid slots, empty clips and rows with a NaN logit give -1.0.  reorder=True sorts every row's slots by expected
    IoU, best first, stable: starts, ends and score (float32 [B,k] or None) are permuted in place along with the result.
    out: (expected_iou, span_entropy) contiguous device tensors of those shapes to write into instead (span_entropy may be None)."""
    import torch
    who = 'span_expected_iou'
    s, e, vl, B, T = _clip_inputs(who, start_logits, end_logits, video_seq_len)
    k = _clip_slots(who, starts, ends, score, B, s.device)
    if out is None:
        out = (torch.empty(B, k, dtype=torch.float32, device=s.device), torch.empty(B, dtype=torch.float32, device=s.device) if entropy else None)
    else:
        if len(out) != 2 or out[0] is None:
            raise HualError(who + ': out is (expected_iou [B,k], span_entropy [B] or None)')
        for o, shape in zip(out, ((B, k), (B,))):
            if o is not None and (o.dtype != torch.float32 or tuple(o.shape) != shape or not o.is_contiguous() or o.device != s.device):
                raise HualError(who + ': out tensors must be contiguous float32 [B,k] and [B] on the logits\' device')
    check(load().hual_span_expected_iou(ptr(s), ptr(e), ptr(vl), B, T, k, ptr(starts), ptr(ends), ptr(score), ptr(out[0]), ptr(out[1]),
                                        1 if reorder else 0, stream_ptr()))
    return out[0], out[1]


def hit_thresholds(thresholds):
    """IoU thresholds as the exact rationals hual_span_hit_prob takes: each a float (through fractions.Fraction(x).limit_denominator(1024);
    an error when that moves the value by more than 1e-9) or a (num, den) pair -> [(num, den), ...] in lowest terms, 1 <= num <= den <= 1024"""
    import fractions
    out = []
    try:
        items = list(thresholds)
    except TypeError:
        raise HualError('span_hit_prob: thresholds is a sequence of floats or (num, den) pairs')
    if not 1 <= len(items) <= 4:
        raise HualError('span_hit_prob: 1 to 4 thresholds, got %d' % len(items))
    for x in items:
        if isinstance(x, (tuple, list)):
            if len(x) != 2 or any(int(y) != y for y in x) or int(x[1]) < 1:
                raise HualError('span_hit_prob: a threshold pair is (num, den) in integers, got %r' % (x,))
            f = fractions.Fraction(int(x[0]), int(x[1]))
        else:
            f = fractions.Fraction(float(x)).limit_denominator(1024)
            if abs(float(f) - float(x)) > 1e-9:
                raise HualError('span_hit_prob: threshold %r is no fraction with a denominator <= 1024 (nearest: %s)' % (x, f))
        if not (1 <= f.numerator <= f.denominator <= 1024):
            raise HualError('span_hit_prob: a threshold lies in (0, 1] with a denominator <= 1024, got %r' % (x,))
        out.append((f.numerator, f.denominator))
    return out


def span_hit_prob(start_logits, end_logits, video_seq_len, thresholds=(0.3, 0.5, 0.7), starts=None, ends=None, score=None, reorder_by=None,
                  best=False, out=None):
    """hit probability P(IoU(span, truth) >= m) under the span distribution of start_logits / end_logits f32 [B,T] and video_seq_len [B]
    for M <= 4 IoU thresholds (hit_thresholds), enqueued on the current stream (hual_span_hit_prob) -> (hit_prob, best):
    hit_prob float32 [B,k,M] of the proposals starts / ends (int64 [B,k] on the device, k <= 16; -1 = no proposal), or None without
    proposals; best = (best_start int64 [B,M], best_end int64 [B,M], best_prob float32 [B,M]), each threshold's span of maximal hit
    probability over the whole triangle, with best=True, else None.  Invalid slots, empty clips and rows with a NaN logit give -1.
    reorder_by=m sorts every row's slots by column m, best first, stable: starts, ends and score (float32 [B,k] or None) are permuted in
    place along with all columns of the result.  out: (hit_prob or None, (best_start, best_end, best_prob) or None) contiguous device
    tensors of those shapes to write into instead."""
    import torch
    who = 'span_hit_prob'
    _clip_logits(who, start_logits, end_logits)      # (_clip_inputs in its two parts: the thresholds' faults are reported between them, as always)
    thr = hit_thresholds(thresholds)
    s, e, vl, B, T = _clip_lengths(who, start_logits, end_logits, video_seq_len)
    M = len(thr)
    if (starts is None) != (ends is None):
        raise HualError(who + ': starts and ends are given together')
    k = 0
    if starts is not None:
        k = _clip_slots(who, starts, ends, score, B, s.device)
    elif score is not None or reorder_by is not None:
        raise HualError(who + ': score and reorder_by need proposals (starts, ends)')
    if not k and not best:
        raise HualError(who + ': nothing to do (no proposals and best=False)')
    rb = -1 if reorder_by is None else int(reorder_by)
    if reorder_by is not None and not 0 <= rb < M:
        raise HualError(who + ': reorder_by is None or a threshold\'s column, 0 <= reorder_by < %d' % M)
    if out is None:
        out = (torch.empty(B, k, M, dtype=torch.float32, device=s.device) if k else None,
               (torch.empty(B, M, dtype=torch.int64, device=s.device), torch.empty(B, M, dtype=torch.int64, device=s.device),
                torch.empty(B, M, dtype=torch.float32, device=s.device)) if best else None)
    else:
        if len(out) != 2 or (out[0] is None) != (k == 0) or (out[1] is None) != (not best) or (best and len(out[1]) != 3):
            raise HualError(who + ': out is (hit_prob [B,k,M] or None, (best_start, best_end, best_prob) [B,M] or None)')
        for o, dt, shape in ((out[0], torch.float32, (B, k, M)),) + (tuple(zip(out[1], (torch.int64, torch.int64, torch.float32), ((B, M),) * 3))
                                                                     if best else ()):
            if o is not None and (o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous() or o.device != s.device):
                raise HualError(who + ': out tensors must be contiguous float32 [B,k,M] and int64, int64, float32 [B,M] on the logits\' device')
    bst = out[1] if best else (None, None, None)
    cthr = (ctypes.c_int32 * (2 * M))(*[x for nd in thr for x in nd])
    check(load().hual_span_hit_prob(ptr(s), ptr(e), ptr(vl), B, T, cthr, M, k, ptr(starts), ptr(ends), ptr(score), ptr(out[0]), rb,
                                    ptr(bst[0]), ptr(bst[1]), ptr(bst[2]), stream_ptr()))
    return out[0], (tuple(out[1]) if best else None)


def span_hit_cover(start_logits, end_logits, video_seq_len, thresholds=(0.3, 0.5, 0.7), starts=None, ends=None, K=0, min_gain=1e-6, out=None):
    """coverage P(some span of a set hits the truth at IoU >= m) under the span distribution of start_logits / end_logits f32 [B,T] and
    video_seq_len [B] for M <= 4 IoU thresholds (hit_thresholds), enqueued on the current stream (hual_span_hit_cover) ->
    (set_prob, cover): set_prob float32 [B,k,M], column q the coverage of the valid slots among slots 0..q of the proposals starts /
    ends (int64 [B,k] on the device, k <= 16; -1 = no proposal; only read) - the chance that the clip counts for R@(q+1) - or None
    without proposals; cover = (cover_start int64 [B,M,K], cover_end int64 [B,M,K], cover_prob float32 [B,M,K]), each threshold's greedy
    set of K <= 16 spans of the whole triangle, every step the span that adds the most mass not yet covered, with the cumulative
    coverage after it, or None with K == 0.  The set stops when the best gain is <= min_gain: later slots are -1, -1 and repeat the
    last coverage.  Empty clips and rows with a NaN logit give -1.  out: (set_prob or None, (cover_start, cover_end, cover_prob) or
    None) contiguous device tensors of those shapes to write into instead."""
    import torch
    who = 'span_hit_cover'
    _clip_logits(who, start_logits, end_logits)
    thr = hit_thresholds(thresholds)
    s, e, vl, B, T = _clip_lengths(who, start_logits, end_logits, video_seq_len)
    M, K = len(thr), int(K)
    if (starts is None) != (ends is None):
        raise HualError(who + ': starts and ends are given together')
    k = _clip_slots(who, starts, ends, None, B, s.device) if starts is not None else 0
    if not 0 <= K <= 16:
        raise HualError(who + ': 0 <= K <= 16, got %d' % K)
    if not k and not K:
        raise HualError(who + ': nothing to do (no proposals and K == 0)')
    if not 0.0 <= float(min_gain) < 1.0:
        raise HualError(who + ': 0 <= min_gain < 1, got %r' % (min_gain,))
    if out is None:
        out = (torch.empty(B, k, M, dtype=torch.float32, device=s.device) if k else None,
               (torch.empty(B, M, K, dtype=torch.int64, device=s.device), torch.empty(B, M, K, dtype=torch.int64, device=s.device),
                torch.empty(B, M, K, dtype=torch.float32, device=s.device)) if K else None)
    else:
        if len(out) != 2 or (out[0] is None) != (k == 0) or (out[1] is None) != (K == 0) or (K and len(out[1]) != 3):
            raise HualError(who + ': out is (set_prob [B,k,M] or None, (cover_start, cover_end, cover_prob) [B,M,K] or None)')
        for o, dt, shape in ((out[0], torch.float32, (B, k, M)),) + (tuple(zip(out[1], (torch.int64, torch.int64, torch.float32), ((B, M, K),) * 3))
                                                                     if K else ()):
            if o is not None and (o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous() or o.device != s.device):
                raise HualError(who + ': out tensors must be contiguous float32 [B,k,M] and int64, int64, float32 [B,M,K] on the logits\' device')
    cov = out[1] if K else (None, None, None)
    cthr = (ctypes.c_int32 * (2 * M))(*[x for nd in thr for x in nd])
    check(load().hual_span_hit_cover(ptr(s), ptr(e), ptr(vl), B, T, cthr, M, k, ptr(starts), ptr(ends), ptr(out[0]), K, float(min_gain),
                                     ptr(cov[0]), ptr(cov[1]), ptr(cov[2]), stream_ptr()))
    return out[0], (tuple(out[1]) if K else None)


def al_score(aset, s0, e0, coff_uncert, out, pair=None, bank=None, info=None, K=2, stat='range', uncert_model=None):
    """one scoring launch over the hual_al_set `aset`, the model-uncertainty term from one source: pair = (s1, e1, s2, e2), the two
    stochastic passes' logits (hual_al_score); else the hual_al_bank `bank` of K folded passes, read as `stat` in AL_STAT
    (hual_al_score_mc) or, with the hual_al_info `info` beside it, in AL_STAT_INFO (hual_al_score_info).  s0 / e0: the deterministic
    logits; out = (sprob, eprob, uncert_frame, uncert_video, observe); uncert_model (bank forms): the term itself.  All device tensors
    f32 [N, ld] but uncert_frame f64, uncert_video f32 [N], observe i32 [N]; enqueued on the current stream."""
    l, ref = load(), ctypes.byref
    head = [ref(aset), ptr(s0), ptr(e0)]
    tail = [float(coff_uncert)] + [ptr(t) for t in out]
    if pair is not None:
        rc = l.hual_al_score(*head, *[ptr(t) for t in pair], *tail, stream_ptr())
    elif stat in AL_STAT_INFO:
        rc = l.hual_al_score_info(*head, ref(bank), ref(info) if info is not None else None, int(K), AL_STAT_INFO[stat], *tail,
                                  ptr(uncert_model), stream_ptr())
    else:
        rc = l.hual_al_score_mc(*head, ref(bank), int(K), AL_STAT[stat], *tail, ptr(uncert_model), stream_ptr())
    check(rc)


AL_QUERY_MAX_T = 256      # the span kernels' row length (csrc/spanprob.h)


def _span_inputs(who, aset, s0, e0, tlen):
    """the gate of every span-posterior launch: tlen, the set's row lengths on the HOST, none above AL_QUERY_MAX_T; s0 / e0, the
    deterministic logits, contiguous f32 [N, ld] on one device -> (N, ld, that device)"""
    import numpy as np
    import torch
    N, ld = int(aset.N), int(aset.ld)
    tl = np.asarray(tlen)
    if tl.size != N:
        raise HualError('%s: tlen must hold N = %d row lengths' % (who, N))
    if int(tl.max()) > AL_QUERY_MAX_T:
        raise HualError('%s: a row of %d frames - the span posterior handles at most %d' % (who, int(tl.max()), AL_QUERY_MAX_T))
    for x in (s0, e0):
        if x.dtype != torch.float32 or tuple(x.shape) != (N, ld) or not x.is_contiguous() or x.device != s0.device:
            raise HualError('%s: s0 / e0 must be contiguous float32 [N, ld] = [%d, %d] on one device' % (who, N, ld))
    return N, ld, s0.device


def _span_index(who, name, x, shape, dev, required=False, text=None):
    """the gate of every int32 device argument of the span-posterior launches (sel, cand, old_idx, gt, budget, flip): None - unless
    `required` -, or a contiguous int32 tensor on the logits' device of `shape`, an entry of which is an extent or a range of extents;
    text: how the message words the shape (default: its numbers)"""
    import torch
    if x is None and not required:
        return
    ok = x is not None and x.dtype == torch.int32 and x.is_contiguous() and x.device == dev and (
        tuple(x.shape) == shape or x.dim() == len(shape) and all(d == w or isinstance(w, range) and d in w for d, w in zip(x.shape, shape)))
    if not ok:
        raise HualError('%s: %s must be a contiguous int32 %s on the logits\' device' % (who, name, text or list(shape)))


def _span_sel(who, sel, N, dev):
    """sel: device i32 [nsel] sample ids or None -> nsel, N without a list"""
    _span_index(who, 'sel', sel, (range(1, 2 ** 31),), dev, text='[nsel], nsel >= 1,')
    return N if sel is None else int(sel.numel())


AL_GAIN_MAX_CAND = 256      # candidate frames per sample of hual_al_label_gain
AL_ENS_MAX_K = 16           # passes per hual_al_ensemble_query / hual_al_ensemble_label launch
AL_GRID_MAX_TAU = 32        # temperatures per hual_al_evidence_grid launch
AL_GRID_MAX_EPS = 16        # error rates per launch (csrc/spancalib.h)
AL_SESSION_MAX_Q = 16           # question slots per sample of hual_al_session
AL_SESSION_MAX_POINTS = 64      # active points of one sample, the set's and the session's, that hual_al_session holds
AL_DESIGN_MAX_M = 16            # frames per sample of hual_al_design
AL_STOP_REASONS = ('budget', 'entropy', 'gain', 'contradictory', 'poisoned', 'overflow', 'reliable')      # HUAL_AL_STOP_*, by value

# The outputs of every span-posterior launch, in the order the C entry point takes them: (name, shape, dtype, fill, optional).
# shape: extents by name - N, ld, K (passes), Q (question slots), Q1 = Q + 1, M (design slots), AB (grid cells) - or as numbers; fill: what a tensor
# allocated here holds before the launch writes its part (None: left uninitialised, the launch writes all of it); optional: the caller
# may leave it out (None) - a switch of the wrapper (frames=, marginals=, old_idx=) does so for tensors allocated here.
_NAN = float('nan')
_LABEL_OUT = (('new_idx', ('N', 2), 'int32', -1, False), ('conf', ('N',), 'float32', -1, False), ('old_conf', ('N',), 'float32', -1, True))
_GAIN_OUT = (('gain', ('N', 'ld'), 'float32', 0, True), ('ask_point', ('N',), 'int32', -1, False), ('ask_gain', ('N',), 'float32', -1, False),
             ('value', ('N',), 'float32', -1, False))
_SESSION_OUT = (('asked', ('N', 'Q'), 'int32', -1, False), ('answer', ('N', 'Q'), 'int8', -1, False), ('q_asked', ('N', 'Q'), 'float32', -1, False),
                ('gain', ('N', 'Q'), 'float32', -1, False), ('entropy', ('N', 'Q1'), 'float32', -1, False), ('n_asked', ('N',), 'int32', -1, False),
                ('stop_reason', ('N',), 'int32', -1, False))
_SPAN_OUT = {
    'al_query': (('incl', ('N', 'ld'), 'float32', 0, True), ('gain', ('N', 'ld'), 'float32', 0, True), ('query_point', ('N',), 'int32', None, False),
                 ('query_gain', ('N',), 'float32', None, False), ('post_entropy', ('N',), 'float32', None, False),
                 ('agree', ('N',), 'float32', None, False)),
    'al_mbr_label': _LABEL_OUT,
    'al_ensemble_label': _LABEL_OUT,
    'al_label_gain': _GAIN_OUT,
    'al_label_gain_noisy': _GAIN_OUT,
    'al_span_marginals': (('y_start', ('N', 'ld'), 'float32', 0, False), ('y_end', ('N', 'ld'), 'float32', 0, False),
                          ('status', ('N',), 'int32', 0, False)),
    'al_noisy_tilt': (('s_t', ('N', 'ld'), 'float32', 0, False), ('e_t', ('N', 'ld'), 'float32', 0, False),
                      ('log_evidence', ('N',), 'float32', None, False)),
    'al_ensemble_query': (('weight', ('N', 'K'), 'float32', None, False), ('log_evidence', ('N',), 'float32', None, False),
                          ('incl', ('N', 'ld'), 'float32', 0, True), ('gain', ('N', 'ld'), 'float32', 0, True),
                          ('query_point', ('N',), 'int32', None, False), ('query_gain', ('N',), 'float32', None, False),
                          ('y_start', ('N', 'ld'), 'float32', 0, True), ('y_end', ('N', 'ld'), 'float32', 0, True),
                          ('post_entropy', ('N',), 'float32', None, False), ('expected_entropy', ('N',), 'float32', None, False),
                          ('span_bald', ('N',), 'float32', None, False), ('status', ('N',), 'int32', None, False)),
    'al_evidence_grid': (('table', ('N', 'AB'), 'float64', _NAN, False), ('status', ('N',), 'int32', -1, False),
                         ('total', ('AB',), 'float64', None, False), ('counts', (4,), 'int32', None, False)),
    'al_session': _SESSION_OUT,
    'al_session_label': _SESSION_OUT + (('label', ('N', 'Q1', 2), 'int32', -1, False), ('label_conf', ('N', 'Q1'), 'float32', -1, False),
                                        ('label_hit', ('N', 'Q1', 'M'), 'float32', -1, False)),
    'al_design': (('frames', ('N', 'M'), 'int32', -1, False), ('info', ('N', 'M'), 'float32', -1, False), ('post_entropy', ('N',), 'float32', -1, False),
                  ('n_design', ('N',), 'int32', -1, False), ('stop_reason', ('N',), 'int32', -1, False)),
}
AL_ENS_QUERY_OUT = tuple(name for name, _, _, _, _ in _SPAN_OUT['al_ensemble_query'])


def _span_out(who, out, dev, off=(), tied=None, both=(), **extent):
    """the output tuple of the launch `who` (its row of _SPAN_OUT) at the extents given by name.  out None: allocated here with the
    spec's fills, the outputs named in `off` left out.  Else the caller's tuple of tensors to write into, checked: only optional
    outputs may be None; tied = (output, argument): that output is None exactly when it is named in `off` (when that argument is
    None); both: two outputs that are given or left out together."""
    import torch
    if out is None:
        return tuple([None if name in off else torch.full([extent.get(d, d) for d in shape], fill, dtype=getattr(torch, dt), device=dev) if fill
                      else (torch.empty if fill is None else torch.zeros)(*[extent.get(d, d) for d in shape], dtype=getattr(torch, dt), device=dev)
                      for name, shape, dt, fill, _ in _SPAN_OUT[who]])
    spec = [(name, tuple(extent.get(d, d) for d in shape), getattr(torch, dt)) for name, shape, dt, _, _ in _SPAN_OUT[who]]
    names = [name for name, _, _ in spec]
    optional = [name for name, _, _, _, opt in _SPAN_OUT[who] if opt]
    given = {name: o is not None for o, name in zip(out, names)}
    if len(out) != len(spec) or not all(given[name] or name in optional for name in names) or (tied and given[tied[0]] == (tied[0] in off)):
        rule = '%s is None exactly when %s is' % tied if tied else 'only %s may be None' % ' / '.join(optional) if optional else ''
        raise HualError('%s: out is (%s)%s' % (who, ', '.join(names), '; ' + rule if rule else ''))
    if both and given[both[0]] != given[both[1]]:
        raise HualError('%s: %s and %s are both given or both None' % (who, both[0], both[1]))
    for o, (name, shape, dt) in zip(out, spec):
        if o is not None and (o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous() or o.device != dev):
            raise HualError('%s: %s must be a contiguous %s %s on the logits\' device' % (who, name, str(dt).replace('torch.', ''), list(shape)))
    return tuple(out)


def _launch(entry, aset, *args):
    """one C entry point of the family on the hual_al_set `aset`: tensors go as their device pointers, the current stream last"""
    check(getattr(load(), entry)(ctypes.byref(aset), *[ptr(a) if a is None or hasattr(a, 'data_ptr') else a for a in args], stream_ptr()))


def al_query(aset, s0, e0, tlen, frames=True, out=None):
    """the posterior over spans of every sample of the hual_al_set `aset` given its answered active points, and the frame whose answer
    carries most information about the span (hual_al_query), one launch enqueued on the current stream.  s0 / e0: the deterministic
    logits f32 [N, ld] on the device; tlen: the set's row lengths on the HOST (array or list) - the kernel handles rows of at most 256
    frames, and a longer one is refused here, before the launch.
    -> (incl, gain, query_point, query_gain, post_entropy, agree): f32 [N, ld] twice (None with frames=False: only the per-sample outputs
    are written), i32 [N], f32 [N] three times.  out: such a tuple of contiguous device tensors to write into instead (incl / gain may be
    None); columns beyond a row's tlen keep what they held (0 in tensors allocated here)."""
    N, ld, dev = _span_inputs('al_query', aset, s0, e0, tlen)
    out = _span_out('al_query', out, dev, off=() if frames else ('incl', 'gain'), N=N, ld=ld)
    _launch('hual_al_query', aset, s0, e0, *out)
    return out


def _label(who, entry, head, N, dev, sel, old_idx, out):
    """al_mbr_label and al_ensemble_label behind their input gates; head: the entry point's arguments before sel"""
    nsel = _span_sel(who, sel, N, dev)
    _span_index(who, 'old_idx', old_idx, (N, 2), dev)
    out = _span_out(who, out, dev, off=('old_conf',) if old_idx is None else (), tied=('old_conf', 'old_idx'), N=N)
    _launch(entry, *head, sel, nsel, old_idx, *out)
    return out


def al_mbr_label(aset, s0, e0, tlen, sel=None, old_idx=None, out=None):
    """the pseudo-label by minimum Bayes risk of the selected samples of the hual_al_set `aset`: the span of the consistent set of
    maximal expected temporal IoU under the span posterior given the answered active points (hual_al_mbr_label), one launch enqueued
    on the current stream.  s0 / e0: the deterministic logits f32 [N, ld] on the device; tlen: the set's row lengths on the HOST - a row
    above AL_QUERY_MAX_T frames is refused here, before the launch, as in al_query; sel: device i32 [nsel] sample ids (None: all);
    old_idx: device i32 [N, 2], the old spans to score beside the label (None: not scored).
    -> (new_idx i32 [N, 2], conf f32 [N], old_conf f32 [N] or None).  out: such a tuple of contiguous device tensors to write into
    instead (old_conf None exactly when old_idx is).  Only the rows of selected samples are written: the others keep what they held
    (-1 in tensors allocated here, the value of a row that gives no label)."""
    N, ld, dev = _span_inputs('al_mbr_label', aset, s0, e0, tlen)
    return _label('al_mbr_label', 'hual_al_mbr_label', (aset, s0, e0), N, dev, sel, old_idx, out)


AL_HIT_MAX_CAND = 16        # candidate spans per sample of hual_al_hit_label


def al_hit_label(aset, s0, e0, tlen, thresholds=(0.3, 0.5, 0.7), sel=None, cand=None, best=True, out=None):
    """label reliability: the hit probability P(IoU(span, truth) >= m | the answers) of spans under the span posterior of the selected
    samples of the hual_al_set `aset` given the answered active points, for M <= 4 IoU thresholds (hit_thresholds), and per threshold
    the member of the consistent set that maximises it (hual_al_hit_label), one launch enqueued on the current stream.  s0 / e0: the
    deterministic logits f32 [N, ld] on the device; tlen: the set's row lengths on the HOST - a row above AL_QUERY_MAX_T frames is
    refused here, before the launch, as in al_mbr_label; sel: device i32 [nsel] sample ids (None: all); cand: device i32 [N, k, 2],
    1 <= k <= 16, the spans to score - members of the consistent set or not; a slot that is no span of the clip gives -1 (None: none).
    -> (cand_hit f32 [N, k, M] or None without cand, (best_idx i32 [N, M, 2], best_prob f32 [N, M]) with best=True, else None - the
    launch then does not search).  out: such a pair of contiguous device tensors to write into instead.  Only the entries of selected
    samples are written: the others keep what they held (-1 in tensors allocated here, the value of a row that gives no probability)."""
    import torch
    who = 'al_hit_label'
    N, ld, dev = _span_inputs(who, aset, s0, e0, tlen)
    thr = hit_thresholds(thresholds)
    M = len(thr)
    nsel = _span_sel(who, sel, N, dev)
    _span_index(who, 'cand', cand, (N, range(1, AL_HIT_MAX_CAND + 1), 2), dev, text='[N, k, 2], 1 <= k <= %d,' % AL_HIT_MAX_CAND)
    k = 0 if cand is None else int(cand.shape[1])
    if not k and not best:
        raise HualError(who + ': nothing to do (no candidates and best=False)')
    if out is None:
        out = (torch.full((N, k, M), -1.0, dtype=torch.float32, device=dev) if k else None,
               (torch.full((N, M, 2), -1, dtype=torch.int32, device=dev), torch.full((N, M), -1.0, dtype=torch.float32, device=dev)) if best else None)
    else:
        if len(out) != 2 or (out[0] is None) != (k == 0) or (out[1] is None) != (not best) or (best and len(out[1]) != 2):
            raise HualError(who + ': out is (cand_hit [N,k,M] or None, (best_idx [N,M,2], best_prob [N,M]) or None)')
        for o, dt, shape in ((out[0], torch.float32, (N, k, M)),) + (tuple(zip(out[1], (torch.int32, torch.float32), ((N, M, 2), (N, M))))
                                                                     if best else ()):
            if o is not None and (o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous() or o.device != dev):
                raise HualError(who + ': out tensors must be contiguous float32 [N,k,M] and int32 [N,M,2], float32 [N,M] on the logits\' device')
    bst = out[1] if best else (None, None)
    cthr = (ctypes.c_int32 * (2 * M))(*[x for nd in thr for x in nd])
    _launch('hual_al_hit_label', aset, s0, e0, sel, nsel, cthr, M, cand, k, out[0], bst[0], bst[1])
    return out[0], (tuple(out[1]) if best else None)


def _label_gain(who, entry, head, N, ld, dev, sel, cand, frames, out):
    """al_label_gain and al_label_gain_noisy behind their input gate; head: the entry point's arguments before sel"""
    nsel = _span_sel(who, sel, N, dev)
    _span_index(who, 'cand', cand, (N, range(1, AL_GAIN_MAX_CAND + 1)), dev, text='[N, M], 1 <= M <= %d,' % AL_GAIN_MAX_CAND)
    out = _span_out(who, out, dev, off=() if frames else ('gain',), N=N, ld=ld)
    _launch(entry, *head, sel, nsel, cand, 0 if cand is None else int(cand.shape[1]), *out)
    return out


def al_label_gain(aset, s0, e0, tlen, sel=None, cand=None, frames=True, out=None):
    """per frame, the temporal IoU the minimum-Bayes-risk label of the selected samples of the hual_al_set `aset` is expected to gain
    from the annotator's answer at that frame, under the span posterior given the answered active points (hual_al_label_gain), one
    launch enqueued on the current stream.  s0 / e0: the deterministic logits f32 [N, ld] on the device; tlen: the set's row lengths on
    the HOST - a row above AL_QUERY_MAX_T frames is refused here, before the launch, as in al_mbr_label; sel: device i32 [nsel] sample
    ids (None: all); cand: device i32 [N, M], 1 <= M <= 256, the frames to evaluate in that order, entries outside the clip skipped
    (None: every frame of the clip).
    -> (gain f32 [N, ld] or None with frames=False, ask_point i32 [N], ask_gain f32 [N], value f32 [N]): the gain per frame, the first
    evaluated frame of maximal gain, that gain, and the expected tIoU of today's label (al_mbr_label's conf).  out: such a tuple of
    contiguous device tensors to write into instead (gain may be None).  Only the rows of selected samples are written, and of gain only
    the columns below a row's tlen: the rest keeps what it held (gain 0, ask_point -1, ask_gain and value -1 in tensors allocated here -
    the values of a row that has no answer to give)."""
    N, ld, dev = _span_inputs('al_label_gain', aset, s0, e0, tlen)
    return _label_gain('al_label_gain', 'hual_al_label_gain', (aset, s0, e0), N, ld, dev, sel, cand, frames, out)


def al_span_marginals(aset, s0, e0, tlen, out=None):
    """the start and end marginals of the span posterior of every sample of the hual_al_set `aset` given its answered active points
    (hual_al_span_marginals), one launch enqueued on the current stream: the soft labels DeviceDataset.set_soft_labels takes.  s0 / e0:
    the deterministic logits f32 [N, ld] on the device; tlen: the set's row lengths on the HOST - a row above AL_QUERY_MAX_T frames is
    refused here, before the launch, as in al_query.
    -> (y_start f32 [N, ld], y_end f32 [N, ld], status i32 [N]): status 1 = a live row, 0 = a poisoned or contradictory one, whose
    columns are 0.  out: such a tuple of contiguous device tensors to write into instead; columns beyond a row's tlen keep what they
    held (0 in tensors allocated here)."""
    N, ld, dev = _span_inputs('al_span_marginals', aset, s0, e0, tlen)
    out = _span_out('al_span_marginals', out, dev, N=N, ld=ld)
    _launch('hual_al_span_marginals', aset, s0, e0, *out)
    return out


def al_noisy_tilt(aset, s0, e0, tlen, eps, out=None):
    """the answers of the hual_al_set `aset` folded into its logits under an annotator who errs with probability eps in (0, 0.5]
    (hual_al_noisy_tilt), one launch enqueued on the current stream: the span posterior given noisy answers is the product form of the
    tilted rows on the whole triangle, so al_query, al_mbr_label, al_span_marginals (and al_label_gain_noisy) read it from them and a set
    WITHOUT answers.  s0 / e0: the deterministic logits f32 [N, ld] on the device; tlen: the set's row lengths on the HOST - a row above
    AL_QUERY_MAX_T frames is refused here, before the launch, as in al_query.
    -> (s_t f32 [N, ld], e_t f32 [N, ld], log_evidence f32 [N]): the tilted logits and ln P(the answers | the model, eps), NaN on a
    poisoned row (whose columns are raw copies).  out: such a tuple of contiguous device tensors to write into instead; columns beyond
    a row's tlen keep what they held (0 in tensors allocated here)."""
    N, ld, dev = _span_inputs('al_noisy_tilt', aset, s0, e0, tlen)
    out = _span_out('al_noisy_tilt', out, dev, N=N, ld=ld)
    _launch('hual_al_noisy_tilt', aset, s0, e0, float(eps), *out)
    return out


def al_label_gain_noisy(aset, s_t, e_t, tlen, eps, sel=None, cand=None, frames=True, out=None):
    """al_label_gain under an annotator who errs with probability eps in (0, 0.5] (hual_al_label_gain_noisy), one launch enqueued on
    the current stream: per frame, the temporal IoU the minimum-Bayes-risk label is expected to gain from a NOISY answer at that frame -
    the answer re-weights the posterior instead of cutting it, and the label after it may be any span.  s_t / e_t: the TILTED logits of
    al_noisy_tilt, f32 [N, ld] on the device; of `aset` only N, ld, vlen and tlen are read (the answers are in the rows); tlen, sel,
    cand, frames, out and the returned (gain, ask_point, ask_gain, value) are al_label_gain's; value is al_mbr_label's conf on the same
    rows and a set without answers."""
    N, ld, dev = _span_inputs('al_label_gain_noisy', aset, s_t, e_t, tlen)
    return _label_gain('al_label_gain_noisy', 'hual_al_label_gain_noisy', (aset, s_t, e_t, float(eps)), N, ld, dev, sel, cand, frames, out)


def _ens_inputs(who, aset, pass_s, pass_e, tlen, logw):
    """the gate of the two ensemble launches: _span_inputs' on every plane of pass_s / pass_e, contiguous f32 [K, N, ld] on one device,
    1 <= K <= AL_ENS_MAX_K; logw None or contiguous f32 [K, N] there -> (K, N, ld, that device)"""
    import torch
    if pass_s.dim() != 3 or pass_e.shape != pass_s.shape or not 1 <= pass_s.shape[0] <= AL_ENS_MAX_K:
        raise HualError('%s: pass_s / pass_e must both be [K, N, ld] with 1 <= K <= %d' % (who, AL_ENS_MAX_K))
    if not pass_s.is_contiguous() or not pass_e.is_contiguous():
        raise HualError('%s: pass_s / pass_e must be contiguous (plane stride N * ld)' % who)
    K = int(pass_s.shape[0])
    N, ld, dev = _span_inputs(who, aset, pass_s[0], pass_e[0], tlen)
    if pass_e.device != dev:
        raise HualError('%s: pass_s / pass_e must lie on one device' % who)
    if logw is not None and (logw.dtype != torch.float32 or tuple(logw.shape) != (K, N) or not logw.is_contiguous() or logw.device != dev):
        raise HualError('%s: logw must be a contiguous float32 [K, N] = [%d, %d] on the logits\' device' % (who, K, N))
    return K, N, ld, dev


def al_ensemble_query(aset, pass_s, pass_e, tlen, logw=None, frames=True, marginals=True, out=None):
    """the span posterior of every sample of the hual_al_set `aset` as the Bayesian model average over K stochastic passes, each
    weighted by its evidence of the answered active points (hual_al_ensemble_query), one launch enqueued on the current stream.
    pass_s / pass_e: the passes' logits f32 [K, N, ld] on the device, 1 <= K <= 16; tlen: the set's row lengths on the HOST - a row above
    AL_QUERY_MAX_T frames is refused here, before the launch, as in al_query; logw: None or device f32 [K, N], a log prior weight per
    pass and row (the K log_evidence rows of al_noisy_tilt, with the tilted planes and a set without answers: the noisy ensemble).
    -> the tuple AL_ENS_QUERY_OUT names: weight f32 [N, K], log_evidence f32 [N], incl, gain f32 [N, ld] (None with frames=False),
    query_point i32 [N], query_gain f32 [N], y_start, y_end f32 [N, ld] (None with marginals=False), post_entropy (of the mixture),
    expected_entropy (the weighted mean of the passes') and span_bald (their difference: the mutual information between the span and
    the dropout mask, bits) f32 [N], status i32 [N] (1 = live).  out: such a tuple of contiguous device tensors to write into instead
    (incl / gain may be None, y_start / y_end both or neither); columns beyond a row's tlen keep what they held (0 in tensors allocated
    here)."""
    K, N, ld, dev = _ens_inputs('al_ensemble_query', aset, pass_s, pass_e, tlen, logw)
    off = (() if frames else ('incl', 'gain')) + (() if marginals else ('y_start', 'y_end'))
    out = _span_out('al_ensemble_query', out, dev, off=off, both=('y_start', 'y_end'), N=N, ld=ld, K=K)
    _launch('hual_al_ensemble_query', aset, pass_s, pass_e, K, logw, *out)
    return out


def al_ensemble_label(aset, pass_s, pass_e, tlen, logw=None, sel=None, old_idx=None, out=None):
    """al_mbr_label under the same model average (hual_al_ensemble_label), one launch enqueued on the current stream: the span of
    the consistent set of maximal expected temporal IoU R(a, e) = sum_k w_k R_k(a, e), the passes' values weighted as in
    al_ensemble_query.  pass_s / pass_e, tlen and logw are al_ensemble_query's; sel, old_idx, out and the returned (new_idx i32 [N, 2],
    conf f32 [N], old_conf f32 [N] or None) are al_mbr_label's."""
    K, N, ld, dev = _ens_inputs('al_ensemble_label', aset, pass_s, pass_e, tlen, logw)
    return _label('al_ensemble_label', 'hual_al_ensemble_label', (aset, pass_s, pass_e, K, logw), N, dev, sel, old_idx, out)


def al_evidence_grid(aset, s0, e0, tlen, inv_tau, eps, sel=None, out=None):
    """ln P(the answers | softmax(s0 * inv_tau[a]), softmax(e0 * inv_tau[a]), eps[b]) of every selected sample of the hual_al_set `aset`
    on the grid of A reciprocal temperatures x B error rates, and its sum over the set per cell (hual_al_evidence_grid), enqueued on the
    current stream: the likelihood that calibrates the span posterior.  s0 / e0: the UNTILTED deterministic logits f32 [N, ld] on the
    device; tlen: the set's row lengths on the HOST - a row above AL_QUERY_MAX_T frames is refused here, before the launch, as in
    al_query; inv_tau: 1 to 32 host floats, finite and > 0 (read as float32: the row is the float32 product s0 * inv_tau[a]); eps: 1 to
    16 host floats in (0, 0.5] (read as float32); sel: device i32 [nsel] sample ids (None: all).
    -> (table f64 [N, A * B], status i32 [N], total f64 [A * B], counts i32 [4]): cell c = a * B + b; a poisoned cell is NaN; status 1 = every
    cell of the row is finite; total sums the selected rows of status 1; counts = rows summed, answers summed, rows left out, the first
    cell of maximal total (-1: no row was summed).  out: such a tuple of contiguous device tensors to write into instead.  Only the rows
    of selected samples are written in table and status: the others keep what they held (NaN and -1 in tensors allocated here)."""
    import numpy as np
    N, ld, dev = _span_inputs('al_evidence_grid', aset, s0, e0, tlen)
    nsel = _span_sel('al_evidence_grid', sel, N, dev)
    it = np.ascontiguousarray(np.asarray(inv_tau, dtype=np.float32).reshape(-1))
    ep = np.ascontiguousarray(np.asarray(eps, dtype=np.float32).reshape(-1))
    A, B = int(it.size), int(ep.size)
    if not 1 <= A <= AL_GRID_MAX_TAU or not 1 <= B <= AL_GRID_MAX_EPS:
        raise HualError('al_evidence_grid: 1 to %d temperatures and 1 to %d error rates per launch' % (AL_GRID_MAX_TAU, AL_GRID_MAX_EPS))
    out = _span_out('al_evidence_grid', out, dev, N=N, AB=A * B)
    _launch('hual_al_evidence_grid', aset, s0, e0, sel, nsel, it.ctypes.data_as(ctypes.c_void_p), A, ep.ctypes.data_as(ctypes.c_void_p), B, *out)
    return out


def al_session(aset, s0, e0, tlen, gt, qmax, sel=None, budget=None, stop_entropy=-1.0, min_gain=0.0, eps=0.0, flip=None, out=None):
    """an annotation session per selected sample of the hual_al_set `aset` (hual_al_session), one launch enqueued on the current
    stream: up to qmax questions, each the frame of most expected information gain under the span posterior given every answer so far,
    answered from the ground-truth span, until a stop condition holds.  s0 / e0: the UNTILTED deterministic logits f32 [N, ld] on the
    device; tlen: the set's row lengths on the HOST - a row above AL_QUERY_MAX_T frames is refused here, before the launch, as in
    al_query; gt: device i32 [N, 2], the ground-truth frame spans; qmax in [1, 16]; sel: device i32 [nsel] sample ids (None: all);
    budget: device i32 [N] per-sample caps (None: qmax); stop_entropy: bits, negative = off; min_gain: bits, >= 0; eps: 0 = the hard
    rule, (0, 0.5] = the noisy annotator; flip: device i32 [N] (read as u32), bit k flips the session's k-th answer (None: no flip).
    -> (asked i32 [N, qmax], answer i8 [N, qmax], q_asked f32 [N, qmax], gain f32 [N, qmax], entropy f32 [N, qmax + 1], n_asked i32 [N],
    stop_reason i32 [N]; AL_STOP_REASONS names its values).  out: such a tuple of contiguous device tensors to write into instead.
    Only the rows of selected samples are written: the others keep what they held (-1 in tensors allocated here, the value of an unused
    slot)."""
    N, ld, dev = _span_inputs('al_session', aset, s0, e0, tlen)
    nsel = _span_sel('al_session', sel, N, dev)
    qmax = int(qmax)
    if not 1 <= qmax <= AL_SESSION_MAX_Q:
        raise HualError('al_session: qmax must lie in [1, %d]' % AL_SESSION_MAX_Q)
    _span_index('al_session', 'gt', gt, (N, 2), dev, required=True)
    _span_index('al_session', 'budget', budget, (N,), dev)
    _span_index('al_session', 'flip', flip, (N,), dev)
    out = _span_out('al_session', out, dev, N=N, Q=qmax, Q1=qmax + 1)
    _launch('hual_al_session', aset, s0, e0, gt, sel, nsel, qmax, budget, float(stop_entropy), float(min_gain), float(eps), flip, *out)
    return out


def al_session_label(aset, s0, e0, tlen, gt, qmax, thresholds=(0.3, 0.5, 0.7), stop_m=0, stop_hit=-1.0, sel=None, budget=None,
                     stop_entropy=-1.0, min_gain=0.0, eps=0.0, flip=None, out=None):
    """al_session with a label trail and a stop rule on the label's reliability (hual_al_session_label), one launch enqueued on the
    current stream: after every pass of the session the minimum-Bayes-risk label of the list so far (al_mbr_label's) and its hit
    probability at the M <= 4 IoU thresholds `thresholds` (hit_thresholds; al_hit_label's cand_hit of that one span), and the session
    stops as 'reliable' once the stored float32 hit probability at thresholds[stop_m] reaches stop_hit - a probability in (0, 1];
    negative: the rule is off and the session is al_session's bit for bit.  aset, s0 / e0, tlen, gt, qmax, sel, budget, stop_entropy,
    min_gain, eps and flip are al_session's.
    -> al_session's seven tensors, then label i32 [N, qmax + 1, 2], label_conf f32 [N, qmax + 1], label_hit f32 [N, qmax + 1, M]: slot k
    is the pass before question k, slot n_asked the final label.  out: such a tuple of ten contiguous device tensors to write into
    instead.  Only the rows of selected samples are written: the others keep what they held (-1 in tensors allocated here, the value
    of an unused slot and of a pass that was not live)."""
    who = 'al_session_label'
    N, ld, dev = _span_inputs(who, aset, s0, e0, tlen)
    thr = hit_thresholds(thresholds)
    M = len(thr)
    nsel = _span_sel(who, sel, N, dev)
    qmax = int(qmax)
    if not 1 <= qmax <= AL_SESSION_MAX_Q:
        raise HualError(who + ': qmax must lie in [1, %d]' % AL_SESSION_MAX_Q)
    if isinstance(stop_m, bool) or int(stop_m) != stop_m or not 0 <= int(stop_m) < M:
        raise HualError(who + ': stop_m is the index of one of the %d thresholds' % M)
    stop_hit = float(stop_hit)
    if not (stop_hit < 0.0 or 0.0 < stop_hit <= 1.0):
        raise HualError(who + ': stop_hit is negative (off) or a probability in (0, 1]')
    _span_index(who, 'gt', gt, (N, 2), dev, required=True)
    _span_index(who, 'budget', budget, (N,), dev)
    _span_index(who, 'flip', flip, (N,), dev)
    out = _span_out(who, out, dev, N=N, Q=qmax, Q1=qmax + 1, M=M)
    cthr = (ctypes.c_int32 * (2 * M))(*[x for nd in thr for x in nd])
    _launch('hual_al_session_label', aset, s0, e0, gt, sel, nsel, qmax, budget, float(stop_entropy), float(min_gain), float(eps), flip,
            cthr, M, int(stop_m), stop_hit, *out)
    return out


def al_design(aset, s0, e0, tlen, mmax, sel=None, forced=None, min_gain=0.0, stop_entropy=-1.0, out=None):
    """the frames to ask TOGETHER about every selected sample of the hual_al_set `aset` (hual_al_design), one launch enqueued on the
    current stream: a greedy design of up to mmax frames under the span posterior given the answered active points - step m takes the
    first frame of maximal I(D + t), the entropy of the answer vector of the frames so far and t - for an annotator who answers the
    frames of a clip at once.  s0 / e0: the deterministic logits f32 [N, ld] on the device; tlen: the set's row lengths on the HOST - a
    row above AL_QUERY_MAX_T frames is refused here, before the launch, as in al_query; mmax in [1, 16]; sel: device i32 [nsel] sample
    ids (None: all); forced: device i32 [N, mmax] (None: none) - a row's leading entries >= 0 are the first frames of its design,
    placed without a stop test (-1 ends them; an entry beyond the clip is ignored); min_gain: bits, >= 0; stop_entropy: bits of
    expected entropy left at which the design stops, negative = off.
    -> (frames i32 [N, mmax], info f32 [N, mmax], post_entropy f32 [N], n_design i32 [N], stop_reason i32 [N]; AL_STOP_REASONS names
    its values): info[n, m] is the information of the first m + 1 frames in bits.  out: such a tuple of contiguous device tensors to
    write into instead.  Only the rows of selected samples are written: the others keep what they held (-1 in tensors allocated here,
    the value of an unused slot)."""
    N, ld, dev = _span_inputs('al_design', aset, s0, e0, tlen)
    nsel = _span_sel('al_design', sel, N, dev)
    mmax = int(mmax)
    if not 1 <= mmax <= AL_DESIGN_MAX_M:
        raise HualError('al_design: mmax must lie in [1, %d]' % AL_DESIGN_MAX_M)
    _span_index('al_design', 'forced', forced, (N, mmax), dev)
    out = _span_out('al_design', out, dev, N=N, M=mmax)
    _launch('hual_al_design', aset, s0, e0, sel, nsel, mmax, forced, float(min_gain), float(stop_entropy), *out)
    return out


# ---------------------------------------------------------------- core-set clip selection
KCENTER_MAX_D = 4096        # columns of hual_kcenter_greedy's x and of hual_clip_mean_features' bank


def clip_mean_features(feat_bank, feat_off, normalize=True, out=None):
    """one descriptor per video of a resident feature bank (hual_clip_mean_features), one launch enqueued on the current stream.
    feat_bank: device f32 [frames, vdim], contiguous; feat_off: device i64 [V + 1], the frames of video v are the rows
    feat_off[v] .. feat_off[v + 1] (DeviceDataset.feat_bank / feat_off).  -> f32 [V, vdim]: the mean over the video's frames, with
    normalize divided by its L2 norm (a zero row stays zero).  out: a contiguous device f32 [V, vdim] to write into instead."""
    import torch
    who = 'clip_mean_features'
    if not (torch.is_tensor(feat_bank) and feat_bank.dtype == torch.float32 and feat_bank.dim() == 2 and feat_bank.is_contiguous()):
        raise HualError(who + ': feat_bank must be a contiguous float32 [frames, vdim] tensor')
    dev, vdim = feat_bank.device, int(feat_bank.shape[1])
    if not (torch.is_tensor(feat_off) and feat_off.dtype == torch.int64 and feat_off.dim() == 1 and feat_off.numel() >= 2
            and feat_off.is_contiguous() and feat_off.device == dev):
        raise HualError(who + ': feat_off must be a contiguous int64 [V + 1] tensor on the bank\'s device, V >= 1')
    if not 1 <= vdim <= KCENTER_MAX_D:
        raise HualError(who + ': vdim must lie in [1, %d]' % KCENTER_MAX_D)
    V = int(feat_off.numel()) - 1
    if out is None:
        out = torch.empty(V, vdim, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (V, vdim) and out.is_contiguous() and out.device == dev):
        raise HualError(who + ': out must be a contiguous float32 [%d, %d] tensor on the bank\'s device' % (V, vdim))
    check(load().hual_clip_mean_features(ptr(feat_bank), ptr(feat_off), V, vdim, int(bool(normalize)), ptr(out), vdim, stream_ptr()))
    return out


def kcenter_workspace_bytes(N):
    return int(load().hual_kcenter_workspace_bytes(int(N)))


def kcenter_select(x, n_select, weight=None, init=None, out=None, workspace=None, validate=True):
    """core-set selection: n_select greedy k-center picks among the rows of x, weighted by `weight` (hual_kcenter_greedy: 2 + n_init +
    n_select launches enqueued on the current stream by one call, nothing synchronised).  x: device f32 [N, D], 1 <= D <= 4096, its
    rows contiguous (a row stride above D is taken as it is); weight: device f32 [N] (None: every weight 1; a negative or NaN weight:
    never picked); init: the rows that are centers before the first pick - a HOST sequence or array of ints, checked here (in [0, N),
    no repeats: ValueError) and uploaded, or a device int32 tensor, read back for the same check; n_select in [0, N].
    -> (picked i32 [n_select], pick_dist f32 [n_select], mind f32 [N], assign i32 [N]): step s picks the eligible row of maximal
    (weight * mind, weight, -index), mind the squared distance to the nearest center so far; picked = -1 and pick_dist = -1 once no
    eligible row is left; mind / assign account for every center on return (assign: the row index of the nearest center).  out: such
    a tuple of contiguous device tensors to write into instead.  n_select = 0 launches and writes nothing (tensors allocated here then
    hold +inf in mind and -1 in assign).  workspace: a device uint8 tensor of at least kcenter_workspace_bytes(N) bytes to reuse.
    validate=False: a device int32 init is taken as it is, without the read-back - for a graph capture, where nothing can be read back
    (the kernel range-checks every index itself: a row outside [0, N) is skipped there)."""
    return _kcenter('kcenter_select', None, x, n_select, weight, init, out, workspace, validate)


def kcenter_sample(x, n_select, weight=None, init=None, seed=0, offset=0, sample=True, origin=True, out=None, workspace=None,
                   validate=True):
    """kcenter_select with two switches (hual_kcenter_sample: the same launches, outputs, workspace and eligibility rules).  origin: the
    zero vector is a center before the first pick - mind opens as |x_i|^2 and assign -1 means "the origin".  sample: D^2 sampling -
    step s draws the row with probability proportional to weight * mind (the argmax of (weight * mind) / E over unit exponentials E,
    Philox4x32-7 at (step, row, HUAL_SITE_SELECT, offset) under `seed`), so a second call with the same seed and offset returns equal
    bits; a row with weight * mind == 0 is taken only when nothing else is left.  seed: an int in [0, 2^64); offset: an int in
    [0, 2^32) - ValueError otherwise.  sample=False, origin=False is kcenter_select, bit for bit."""
    who = 'kcenter_sample'
    for name, val, bits in (('seed', seed, 64), ('offset', offset, 32)):
        if isinstance(val, bool) or not isinstance(val, int) or not 0 <= val < (1 << bits):
            raise ValueError('%s: %s must be an integer in [0, 2^%d)' % (who, name, bits))
    return _kcenter(who, (int(seed), int(offset), int(bool(sample)), int(bool(origin))), x, n_select, weight, init, out, workspace, validate)


def _kcenter(who, sampler, x, n_select, weight, init, out, workspace, validate):
    """the argument checks and the call kcenter_select and kcenter_sample share; sampler: None, or (seed, offset, sample, origin)"""
    import numpy as np
    import torch
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and x.shape[1] >= 1 and x.stride(1) == 1
            and x.stride(0) >= x.shape[1]):
        raise HualError(who + ': x must be a float32 [N, D] tensor with contiguous rows, N >= 1')
    N, D, dev = int(x.shape[0]), int(x.shape[1]), x.device
    if D > KCENTER_MAX_D:
        raise HualError(who + ': D must lie in [1, %d]' % KCENTER_MAX_D)
    if isinstance(n_select, bool) or int(n_select) != n_select or not 0 <= int(n_select) <= N:
        raise ValueError(who + ': n_select must be an integer in [0, N] = [0, %d]' % N)
    n_select = int(n_select)
    if weight is not None and not (torch.is_tensor(weight) and weight.dtype == torch.float32 and tuple(weight.shape) == (N,)
                                   and weight.is_contiguous() and weight.device == dev):
        raise HualError(who + ': weight must be a contiguous float32 [N] tensor on x\'s device')
    init_d, n_init = None, 0
    if not validate:                                             # (inside a graph capture nothing can be read back or uploaded)
        if init is not None and not (torch.is_tensor(init) and init.dtype == torch.int32 and init.dim() == 1 and init.is_contiguous()
                                     and init.device == dev and init.numel() <= N):
            raise HualError(who + ': validate=False takes init as a contiguous device int32 [n_init <= N] tensor')
        init_d, n_init = (init, int(init.numel())) if init is not None and init.numel() else (None, 0)
    elif init is not None:
        init_h = init.cpu().numpy() if torch.is_tensor(init) else np.asarray(init)
        if init_h.ndim != 1 or (init_h.size and init_h.dtype.kind not in 'iu'):
            raise ValueError(who + ': init must be a one-dimensional sequence of row indices')
        init_h = init_h.astype(np.int64)
        if init_h.size and (init_h.min() < 0 or init_h.max() >= N):
            raise ValueError(who + ': init holds a row outside [0, N) = [0, %d)' % N)
        if len(np.unique(init_h)) != init_h.size:
            raise ValueError(who + ': init holds a row twice')
        n_init = int(init_h.size)
        if n_init:
            init_d = (init if torch.is_tensor(init) and init.dtype == torch.int32 and init.is_contiguous() and init.device == dev
                      else torch.from_numpy(init_h.astype(np.int32)).to(dev))
    if out is None:
        out = (torch.full((n_select,), -1, dtype=torch.int32, device=dev), torch.full((n_select,), -1.0, dtype=torch.float32, device=dev),
               torch.full((N,), float('inf'), dtype=torch.float32, device=dev), torch.full((N,), -1, dtype=torch.int32, device=dev))
    else:
        spec = (('picked', torch.int32, (n_select,)), ('pick_dist', torch.float32, (n_select,)), ('mind', torch.float32, (N,)),
                ('assign', torch.int32, (N,)))
        if len(out) != 4:
            raise HualError(who + ': out is (picked, pick_dist, mind, assign)')
        for o, (name, dt, shape) in zip(out, spec):
            if not (torch.is_tensor(o) and o.dtype == dt and tuple(o.shape) == shape and o.is_contiguous() and o.device == dev):
                raise HualError('%s: %s must be a contiguous %s %s on x\'s device' % (who, name, str(dt).replace('torch.', ''), list(shape)))
        out = tuple(out)
    need = kcenter_workspace_bytes(N)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= need
              and workspace.device == dev and workspace.data_ptr() % 16 == 0):
        raise HualError(who + ': workspace must be a contiguous 16-byte aligned uint8 tensor of at least %d bytes on x\'s device' % need)
    head = (ptr(x), N, D, int(x.stride(0)), ptr(weight), ptr(init_d), n_init, n_select)
    tail = (ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(workspace), int(workspace.numel()), stream_ptr())
    if sampler is None:
        check(load().hual_kcenter_greedy(*head, *tail))
    else:
        check(load().hual_kcenter_sample(*head, *sampler, *tail))
    return out      # (a workspace allocated here goes back to the caching allocator in stream order: behind the launches)


# ---------------------------------------------------------------- gradient embeddings
GRAD_EMBED_DIM = 256        # columns hual_al_grad_embed writes per row: g_s (0..127), g_e (128..255)
GRAD_EMBED_MAX_T = 256


def al_grad_embed(hs, he, s_logits, e_logits, v_len, hyp, desc, gnorm2, egl, rows=None):
    """the gradient embeddings of the samples of one batch (hual_al_grad_embed), one launch enqueued on the current stream, after a
    label-free forward.  hs / he: device f32 [B * T, 128], contiguous - the forward's head.hs / head.he; s_logits / e_logits: device f32
    [B, ld] with contiguous rows of one stride ld, T <= ld <= 1024, 1 <= T <= 256; v_len: device i32 [B]; hyp: device i32 [B, 2], the
    hypothesised (start, end) frame - an entry outside [0, v) means "no label for this head" (g = the expected feature); rows: device
    i32 [B] or None - the bank row of sample b (None: b), an id outside [0, N) writes nothing.
    Banks, written in place at the rows of the batch's samples: desc f32 [N, >= 256] with contiguous rows (columns 0..127 g_s, 128..255
    g_e), gnorm2 f32 [N] = |g_s|^2 + |g_e|^2, egl f32 [N] = the expected squared gradient length under y ~ p.  A sample without frames
    or with a non-finite logit among its frames gets a NaN descriptor and -1 in gnorm2 / egl.  -> (desc, gnorm2, egl)."""
    import torch
    who = 'al_grad_embed'
    if not (torch.is_tensor(hs) and torch.is_tensor(he) and hs.dtype == he.dtype == torch.float32 and hs.dim() == he.dim() == 2
            and hs.shape == he.shape and hs.shape[1] == 128 and hs.shape[0] >= 1 and hs.is_contiguous() and he.is_contiguous()
            and hs.device == he.device):
        raise HualError(who + ': hs / he must be contiguous float32 [B * T, 128] tensors on one device')
    dev = hs.device
    if not (torch.is_tensor(v_len) and v_len.dtype == torch.int32 and v_len.dim() == 1 and v_len.numel() >= 1 and v_len.is_contiguous()
            and v_len.device == dev):
        raise HualError(who + ': v_len must be a contiguous int32 [B] tensor on the device of hs')
    B = int(v_len.numel())
    if hs.shape[0] % B:
        raise HualError(who + ': hs / he hold %d rows, not a multiple of B = %d' % (hs.shape[0], B))
    T = int(hs.shape[0]) // B
    if not 1 <= T <= GRAD_EMBED_MAX_T:
        raise HualError(who + ': T must lie in [1, %d]' % GRAD_EMBED_MAX_T)
    for name, z in (('s_logits', s_logits), ('e_logits', e_logits)):
        if not (torch.is_tensor(z) and z.dtype == torch.float32 and z.dim() == 2 and z.shape[0] == B and z.stride(1) == 1
                and z.stride(0) >= z.shape[1] and z.device == dev):
            raise HualError('%s: %s must be a float32 [B, ld] tensor with contiguous rows on the device of hs' % (who, name))
    ld = int(s_logits.stride(0)) if B > 1 else int(s_logits.shape[1])
    if B > 1 and int(e_logits.stride(0)) != ld or s_logits.shape[1] != e_logits.shape[1] or s_logits.shape[1] < T:
        raise HualError(who + ': s_logits / e_logits must share one shape [B, >= T] and one row stride')
    if not T <= ld <= 1024:
        raise HualError(who + ': the logits\' row stride must lie in [T, 1024]')
    if not (torch.is_tensor(hyp) and hyp.dtype == torch.int32 and tuple(hyp.shape) == (B, 2) and hyp.is_contiguous() and hyp.device == dev):
        raise HualError(who + ': hyp must be a contiguous int32 [B, 2] tensor on the device of hs')
    if rows is not None and not (torch.is_tensor(rows) and rows.dtype == torch.int32 and tuple(rows.shape) == (B,) and rows.is_contiguous()
                                 and rows.device == dev):
        raise HualError(who + ': rows must be a contiguous int32 [B] tensor on the device of hs')
    if not (torch.is_tensor(desc) and desc.dtype == torch.float32 and desc.dim() == 2 and desc.shape[0] >= 1
            and desc.shape[1] >= GRAD_EMBED_DIM and desc.stride(1) == 1 and desc.stride(0) >= desc.shape[1] and desc.device == dev):
        raise HualError(who + ': desc must be a float32 [N, >= %d] tensor with contiguous rows on the device of hs' % GRAD_EMBED_DIM)
    N = int(desc.shape[0])
    if rows is None and B > N:
        raise HualError(who + ': without rows the bank needs at least B = %d rows' % B)
    for name, o in (('gnorm2', gnorm2), ('egl', egl)):
        if not (torch.is_tensor(o) and o.dtype == torch.float32 and tuple(o.shape) == (N,) and o.is_contiguous() and o.device == dev):
            raise HualError('%s: %s must be a contiguous float32 [N] tensor on the device of hs' % (who, name))
    check(load().hual_al_grad_embed(ptr(hs), ptr(he), ptr(s_logits), ptr(e_logits), ptr(v_len), ptr(hyp), ptr(rows), B, T, ld, N, ptr(desc),
                                    int(desc.stride(0)), ptr(gnorm2), ptr(egl), stream_ptr()))
    return desc, gnorm2, egl

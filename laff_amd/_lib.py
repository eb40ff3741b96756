"""ctypes binding of liblaff_hip.so (include/laff_hip.h).  No fallback: a missing library is an error."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('LAFF_HIP_LIB') or os.path.join(_HERE, 'lib', 'liblaff_hip.so')   # env override: debug builds

# enums of include/laff_hip.h
ACT = {None: 0, False: 0, '': 0, 'none': 0, 'tanh': 1, 'relu': 2, 'sigmoid': 3}
ATT_WITH_AVE, ATT_MUL, ATT_L2NORM_EACH_HEAD, ATT_NO_SPLIT_HEAD, ATT_JUST_AVERAGE = 1, 2, 4, 8, 16
GRU_POOLING = {'mean': 0, 'last': 1, 'mean_last': 2}
OPT_KIND = {'adam': 0, 'rmsprop': 1}
PREC = {'fp32': 0, 'fp16': 1, 'bf16': 2, 'fp16x3': 3, 'bf16x3': 4}
ABI_VERSION = 45


class Plane(C.Structure):
    _fields_ = [('src', C.c_void_p), ('ld', C.c_int), ('tile', C.c_int), ('scale', C.c_void_p), ('shift', C.c_void_p), ('act', C.c_int),
                ('indptr', C.c_void_p), ('indices', C.c_void_p), ('values', C.c_void_p), ('wt', C.c_void_p), ('ldwt', C.c_int),
                ('dk', C.c_int), ('bias', C.c_void_p), ('row_scale', C.c_void_p)]


class RankSide(C.Structure):
    _fields_ = [('side', C.c_int), ('gt_col', C.c_void_p), ('col0', C.c_int), ('Ev', C.c_void_p), ('Nv', C.c_int), ('s_gt64', C.c_void_p),
                ('band', C.c_void_p), ('band_v', C.c_void_p), ('count', C.c_void_p), ('pairs', C.c_void_p), ('partials', C.c_void_p),
                ('tickets', C.c_void_p)]


class FcFusedProblem(C.Structure):
    _fields_ = [('X', C.c_void_p), ('ldx', C.c_int), ('x_rscale', C.c_void_p), ('N', C.c_int), ('Dk', C.c_int),
                ('Ws', C.c_void_p), ('w_rscale', C.c_void_p), ('bias', C.c_void_p), ('bn_scale', C.c_void_p),
                ('bn_shift', C.c_void_p), ('D', C.c_int), ('act', C.c_int), ('Y', C.c_void_p), ('ldy', C.c_int)]


class FcStripProblem(C.Structure):
    _fields_ = [('X', C.c_void_p), ('ldx', C.c_int), ('N', C.c_int), ('img', C.c_void_p), ('D', C.c_int), ('act', C.c_int),
                ('Y', C.c_void_p), ('ldy', C.c_int)]


class FcProblem(C.Structure):
    _fields_ = [('X', C.c_void_p), ('N', C.c_int), ('Dk', C.c_int), ('ldx', C.c_int), ('W', C.c_void_p), ('ldw', C.c_int),
                ('bias', C.c_void_p), ('bn_scale', C.c_void_p), ('bn_shift', C.c_void_p), ('D', C.c_int), ('act', C.c_int),
                ('Y', C.c_void_p), ('ldy', C.c_int)]


class FcShape(C.Structure):
    _fields_ = [('N', C.c_int), ('Dk', C.c_int), ('D', C.c_int), ('ldx', C.c_int), ('ldw', C.c_int), ('x_aligned', C.c_int),
                ('w_aligned', C.c_int)]


class FcLaunch(C.Structure):
    _fields_ = [('kernel', C.c_int), ('count', C.c_int), ('tiles', C.c_longlong), ('nbig', C.c_int), ('quarters', C.c_longlong)]


class FcConcatSegment(C.Structure):
    _fields_ = [('X', C.c_void_p), ('ldx', C.c_int), ('indptr', C.c_void_p), ('indices', C.c_void_p), ('values', C.c_void_p),
                ('Wt', C.c_void_p), ('ldwt', C.c_int), ('Dk', C.c_int), ('col', C.c_int)]


class FcConcatProblem(C.Structure):
    _fields_ = [('segments', C.POINTER(FcConcatSegment)), ('nseg', C.c_int), ('N', C.c_int), ('W', C.c_void_p), ('K', C.c_int),
                ('ldw', C.c_int), ('bias', C.c_void_p), ('bn_scale', C.c_void_p), ('bn_shift', C.c_void_p), ('D', C.c_int),
                ('act', C.c_int), ('Y', C.c_void_p), ('ldy', C.c_int)]


class FcSplitProblem(C.Structure):
    _fields_ = [('Xs', C.c_void_p), ('x_rscale', C.c_void_p), ('N', C.c_int), ('Dk', C.c_int), ('Ws', C.c_void_p),
                ('w_rscale', C.c_void_p), ('bias', C.c_void_p), ('bn_scale', C.c_void_p), ('bn_shift', C.c_void_p),
                ('D', C.c_int), ('act', C.c_int), ('Y', C.c_void_p), ('ldy', C.c_int)]


class ClipBlock(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('ln_1_weight', 'ln_1_bias', 'in_proj_weight', 'in_proj_bias', 'out_proj_weight', 'out_proj_bias',
                                          'ln_2_weight', 'ln_2_bias', 'c_fc_weight', 'c_fc_bias', 'c_proj_weight', 'c_proj_bias')]


class ClipText(C.Structure):
    _fields_ = [('width', C.c_int), ('layers', C.c_int), ('heads', C.c_int), ('embed_dim', C.c_int), ('context_length', C.c_int),
                ('vocab_size', C.c_int), ('token_embedding', C.c_void_p), ('positional_embedding', C.c_void_p),
                ('blocks', C.POINTER(ClipBlock)), ('ln_final_weight', C.c_void_p), ('ln_final_bias', C.c_void_p),
                ('text_projection', C.c_void_p)]


class ClipVisual(C.Structure):
    _fields_ = [('width', C.c_int), ('layers', C.c_int), ('heads', C.c_int), ('embed_dim', C.c_int), ('input_resolution', C.c_int),
                ('patch_size', C.c_int), ('conv1_weight', C.c_void_p), ('class_embedding', C.c_void_p),
                ('positional_embedding', C.c_void_p), ('ln_pre_weight', C.c_void_p), ('ln_pre_bias', C.c_void_p),
                ('blocks', C.POINTER(ClipBlock)), ('ln_post_weight', C.c_void_p), ('ln_post_bias', C.c_void_p), ('proj', C.c_void_p)]


class BertBlock(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('qkv_weight', 'qkv_bias', 'attn_out_weight', 'attn_out_bias', 'ln_1_weight', 'ln_1_bias',
                                          'inter_weight', 'inter_bias', 'out_weight', 'out_bias', 'ln_2_weight', 'ln_2_bias')]


class BertText(C.Structure):
    _fields_ = [('width', C.c_int), ('layers', C.c_int), ('heads', C.c_int), ('intermediate', C.c_int), ('max_position', C.c_int),
                ('vocab_size', C.c_int), ('layer_norm_eps', C.c_float), ('word_embeddings', C.c_void_p),
                ('position_embeddings', C.c_void_p), ('token_type_embedding', C.c_void_p), ('emb_ln_weight', C.c_void_p),
                ('emb_ln_bias', C.c_void_p), ('blocks', C.POINTER(BertBlock)), ('pooler_weight', C.c_void_p),
                ('pooler_bias', C.c_void_p)]


class OptimTensor(C.Structure):
    _fields_ = [('p', C.c_void_p), ('g', C.c_void_p), ('s1', C.c_void_p), ('s2', C.c_void_p), ('n', C.c_longlong)]


class OptimHyper(C.Structure):
    _fields_ = [('kind', C.c_int), ('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double),
                ('weight_decay', C.c_double), ('step', C.c_longlong)]


class FrameDesc(C.Structure):
    _fields_ = [('offset', C.c_int64), ('height', C.c_int32), ('width', C.c_int32), ('htab', C.c_int32), ('vtab', C.c_int32),
                ('reserved', C.c_int32 * 2)]


class RerankProblem(C.Structure):
    _fields_ = [('qq', C.c_void_p), ('ldqq', C.c_longlong), ('qg', C.c_void_p), ('ldqg', C.c_longlong), ('gg', C.c_void_p),
                ('ldgg', C.c_longlong), ('out', C.c_void_p), ('ldo', C.c_longlong), ('Q', C.c_int), ('G', C.c_int)]


class AssembleJob(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('kind', 'rows_at', 'crow_at', 'w', 'ld_src', 'ld_dst', 'n_src', 'n_items', 'fmax', 'cap_dst')] + \
               [(n, C.c_void_p) for n in ('src', 'off_src', 'col_src', 'dst', 'col_dst', 'mask')]


ASSEMBLE_KIND = {'rows': 0, 'ragged': 1, 'csr': 2}
ASSEMBLE_MAX_JOBS, ASSEMBLE_MAX_BATCH = 16, 4096

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
SIGNATURES = {
    'laff_abi_version': (C.c_int, []),
    'laff_last_error': (C.c_char_p, []),
    'laff_ctx_create': (C.c_int, [_I, _P, C.POINTER(_P)]),
    'laff_ctx_set_stream': (C.c_int, [_P, _P]),
    'laff_ctx_destroy': (C.c_int, [_P]),
    'laff_device_info': (C.c_int, [_P, C.POINTER(_I)]),
    'laff_stamp': (C.c_int, [_P, _P]),
    'laff_wall_clock_khz': (C.c_int, [_P, C.POINTER(_I)]),
    'laff_fc_act_bn': (C.c_int, [_P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _I, _I, _P, _I]),
    'laff_fc_act_bn_grouped': (C.c_int, [_P, C.POINTER(FcProblem), _I]),
    'laff_fc_gather_act_bn': (C.c_int, [_P, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P, _I, _I, _P, _I]),
    'laff_fc_concat_act_bn': (C.c_int, [_P, C.POINTER(FcConcatProblem)]),
    'laff_fc_concat_act_bn_grouped': (C.c_int, [_P, C.POINTER(FcConcatProblem), _I]),
    'laff_margin_loss_workspace_bytes': (C.c_int, [_I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_margin_loss': (C.c_int, [_P, _P, _P, _I, _I, _I, C.c_float, C.c_uint, _P, _P, _P, _P, C.c_size_t]),
    'laff_dsl_loss_workspace_bytes': (C.c_int, [_I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_dsl_loss': (C.c_int, [_P, _P, _P, _I, _I, _I, C.c_float, _P, _P, _P, _P, C.c_size_t]),
    'laff_margin_loss_scores': (C.c_int, [_P, _P, _I, _I, C.c_float, C.c_uint, _P, _P]),
    'laff_row_scales_grouped': (C.c_int, [_P, _I, C.POINTER(C.c_void_p), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I),
                                          C.POINTER(C.c_void_p)]),
    'laff_fc_act_bn_fused_grouped': (C.c_int, [_P, C.POINTER(FcFusedProblem), _I]),
    'laff_fc_route': (C.c_int, [_P, _I, C.POINTER(FcShape), _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(FcLaunch), _I, C.POINTER(_I)]),
    'laff_fc_strip_pack_bytes': (C.c_int, [_I, _I, C.POINTER(C.c_size_t)]),
    'laff_fc_strip_pack': (C.c_int, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _P]),
    'laff_fc_act_bn_strip_grouped': (C.c_int, [_P, C.POINTER(FcStripProblem), _I]),
    'laff_frame_fuse_grouped': (C.c_int, [_P, _I, C.POINTER(C.c_void_p), _P, _I, _I, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), C.c_uint, C.POINTER(C.c_void_p)]),
    'laff_frame_fuse_grouped_mask': (C.c_int, [_P, _I, C.POINTER(C.c_void_p), _P, _I, _I, _I, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_void_p), C.c_uint, C.POINTER(C.c_void_p)]),
    'laff_split_rows_bytes': (C.c_int, [_I, _I, C.POINTER(C.c_size_t)]),
    'laff_split_rows': (C.c_int, [_P, _P, _I, _I, _I, _P, _P]),
    'laff_split_rows_grouped': (C.c_int, [_P, _I, C.POINTER(C.c_void_p), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    'laff_fc_act_bn_split_grouped': (C.c_int, [_P, C.POINTER(FcSplitProblem), _I]),
    'laff_plane_row_norms': (C.c_int, [_P, C.POINTER(Plane), _I, _I, _I, _I, C.c_uint, _P]),
    'laff_fuse': (C.c_int, [_P, C.POINTER(Plane), _I, _I, _I, _I, _P, _P, _P, C.c_uint, _P, _P]),
    'laff_fuse_packed': (C.c_int, [_P, C.POINTER(Plane), _I, _I, _I, _I, _P, _P, _P, C.c_uint, _P, _P, _P, _I, _F]),
    'laff_fuse_packed_rank': (C.c_int, [_P, C.POINTER(Plane), _I, _I, _I, _I, _P, _P, _P, C.c_uint, _P, _P, _P, _I, _F, C.POINTER(RankSide)]),
    'laff_fuse_backward_workspace_bytes': (C.c_int, [_I, _I, _I, _I, C.c_uint, C.POINTER(C.c_size_t)]),
    'laff_fuse_backward': (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(_I), _I, _I, _I, _I, _P, _P, _P, C.c_uint, _P, _I,
                                     C.POINTER(C.c_void_p), C.POINTER(_I), _P, _P, _P, C.c_size_t]),
    'laff_fc_backward_plan': (C.c_int, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    'laff_fc_backward': (C.c_int, [_P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, C.c_size_t]),
    'laff_fc_gather_backward': (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P]),
    'laff_dropout_bn_train_plan': (C.c_int, [_I, _I, _I, C.POINTER(_I)]),
    'laff_dropout_bn_train': (C.c_int, [_P, _P, _I, _I, _I, C.c_double, _P, _P, _P, _P, _P, C.c_double, C.c_double, _P, _I, _P, _P, _P,
                                        C.c_size_t]),
    'laff_dropout_bn_train_backward': (C.c_int, [_P, _P, _I, _P, _I, _I, _I, C.c_double, _P, _P, _P, _P, _P, _I, _P, _P, _P, C.c_size_t]),
    'laff_tile_bn_train_plan': (C.c_int, [_I, _I, _I, C.POINTER(_I)]),
    'laff_tile_bn_train': (C.c_int, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, C.c_double, C.c_double, _P, _I, _P, _P, _P, C.c_size_t]),
    'laff_tile_bn_train_backward': (C.c_int, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, C.c_size_t]),
    'laff_expert_stage_train_plan': (C.c_int, [_I, _I, _I, C.POINTER(_I)]),
    'laff_expert_stage_train': (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(_I), _I, _I, _I, _P, _I, _I, _P, _I, _I, _P]),
    'laff_expert_stage_train_backward': (C.c_int, [_P, _P, _I, _I, C.POINTER(C.c_void_p), C.POINTER(_I), _I, _I, _I, _P, _I, _I, _P,
                                                   C.POINTER(C.c_void_p), C.POINTER(_I), _P, _P, C.c_size_t]),
    'laff_optim_plan': (C.c_int, [_I, C.POINTER(C.c_longlong), C.POINTER(_I)]),
    'laff_optim_last_launches': (C.c_int, [C.POINTER(_I)]),
    'laff_grad_sqnorm': (C.c_int, [_P, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), _P, C.c_size_t]),
    'laff_grad_scale': (C.c_int, [_P, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.c_double, _P, _I, _P]),
    'laff_optim_step': (C.c_int, [_P, C.POINTER(OptimTensor), _I, C.POINTER(OptimHyper), C.c_double, _P, _I, _P]),
    'laff_frame_fuse': (C.c_int, [_P, _P, _P, _I, _I, _I, _P, _P, _P, C.c_uint, _P]),
    'laff_frame_fuse_backward_plan': (C.c_int, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    'laff_frame_fuse_backward': (C.c_int, [_P, _I, C.POINTER(C.c_void_p), _P, _I, _I, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p), C.c_uint, C.POINTER(C.c_void_p), _I, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _P, C.c_size_t]),
    'laff_packed_bytes': (C.c_int, [_I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_pack_rows': (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _F, _F, _I, _P]),
    'laff_sim_gemm': (C.c_int, [_P, _P, _P, _I, _I, _I, _F, _I, _P, _I, _P, _I, _P, _P]),
    'laff_sim_gemm_route': (C.c_int, [_P, _I, _I, _I, _I, _I, _I, C.c_uint, C.POINTER(_I)]),
    'laff_row_dot_gt': (C.c_int, [_P, _P, _P, _I, _I, _I, _F, _I, _P, _I, _P, _P]),
    'laff_rank_prepare': (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _P]),
    'laff_match_ids': (C.c_int, [C.c_char_p, C.c_size_t, _I, C.c_char_p, C.c_size_t, _I, _P]),
    'laff_rank_prepare_part': (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _P]),
    'laff_rank_prepare_emit': (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _P]),
    'laff_rank_export_pairs': (C.c_int, [_P, _P, _P, _P, _I, _I, _P, C.c_uint, _P, _I, _I, _P, C.c_uint, _P]),
    'laff_sim_gemm_banded': (C.c_int, [_P, _P, _P, _I, _I, _I, _F, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, C.c_uint]),
    'laff_rank_resolve': (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, C.c_uint]),
    'laff_rank_resolve_metrics': (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, C.c_uint, _I, _P, _P, _I]),
    'laff_gather_gt': (C.c_int, [_P, _P, _I, _I, _I, _P, _I, _P]),
    'laff_rank_count': (C.c_int, [_P, _P, _I, _I, _I, _P, _I, _P, _P, _I]),
    'laff_topk_rows': (C.c_int, [_P, _P, _I, _I, _I, _I, _P, _P]),
    'laff_v2t_count': (C.c_int, [_P, _P, _I, _I, _I, _P, _P, _I, _P]),
    'laff_comm_unique_id': (C.c_int, [_P]),
    'laff_comm_init': (C.c_int, [_P, _I, _I, _P, C.POINTER(_P)]),
    'laff_comm_set_stream': (C.c_int, [_P, _P]),
    'laff_comm_destroy': (C.c_int, [_P]),
    'laff_allgather_rows': (C.c_int, [_P, _P, _P, C.c_size_t]),
    'laff_allreduce_i32_sum': (C.c_int, [_P, _P, C.c_size_t]),
    'laff_allreduce_f64_max': (C.c_int, [_P, _P, C.c_size_t]),
    'laff_v2t_count_exact': (C.c_int, [_P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P, C.c_uint]),
    'laff_rank_metrics': (C.c_int, [_P, _P, _I, _I, _P, C.POINTER(C.c_double)]),
    'laff_rank_metrics_async': (C.c_int, [_P, _P, _I, _I, _P, _P]),
    'laff_gru_pack_whh': (C.c_int, [_P, _P, _I, _P]),
    'laff_gru_workspace_bytes': (C.c_int, [_I, _I, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_gru_encode': (C.c_int, [_P, _P, _P, _P, C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P,
                                  C.c_size_t]),
    'laff_gru_pack_whh_t': (C.c_int, [_P, _P, _I, _P]),
    'laff_gru_gather_rows': (C.c_int, [_P, _P, _I, _I, _P, _I, _P]),
    'laff_gru_train_reserve_bytes': (C.c_int, [_I, _I, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_gru_encode_train': (C.c_int, [_P, _P, _P, _P, C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P,
                                        C.c_size_t, _P, C.c_size_t]),
    'laff_gru_backward_plan': (C.c_int, [C.POINTER(_I), _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    'laff_gru_backward_workspace_bytes': (C.c_int, [C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_gru_backward': (C.c_int, [_P, _P, _P, C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, C.c_size_t, _P, _P, _P, _P, _P,
                                    _P, _P, _P, _I, _I, _P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _P, C.c_size_t]),
    'laff_clip_pack_weight': (C.c_int, [_P, _P, _I, _I, _I, _I, _P]),
    'laff_clip_workspace_bytes': (C.c_int, [_I, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_clip_encode': (C.c_int, [_P, _P, _P, C.POINTER(_I), _I, _I, C.POINTER(ClipText), _I, _P, _I, _P, C.c_size_t]),
    'laff_clip_pack_weight_padded': (C.c_int, [_P, _P, _I, _I, _I, _I, _P]),
    'laff_clip_image_kpad': (C.c_int, [_I, _I, C.POINTER(_I)]),
    'laff_clip_image_workspace_bytes': (C.c_int, [_I, _I, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_clip_image_encode': (C.c_int, [_P, _P, _I, _P, C.POINTER(_I), _I, C.POINTER(ClipVisual), _I, _P, _I, _P, _I, _P, C.c_size_t]),
    'laff_frame_preprocess_workspace_bytes': (C.c_int, [_I, _I, C.POINTER(C.c_size_t)]),
    'laff_frame_preprocess': (C.c_int, [_P, _P, C.c_size_t, _P, _P, _I, _I, _P, _P, C.c_size_t, C.POINTER(_F), C.POINTER(_F), _P, _P, _P,
                                        C.c_size_t]),
    'laff_bert_workspace_bytes': (C.c_int, [_I, _I, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_bert_encode': (C.c_int, [_P, _P, _P, C.POINTER(_I), _I, _I, C.POINTER(BertText), _I, _P, _I, _P, C.c_size_t]),
    'laff_netvlad_workspace_bytes': (C.c_int, [_I, _I, C.POINTER(C.c_size_t)]),
    'laff_netvlad_encode': (C.c_int, [_P, _P, _I, _I, _P, _P, C.POINTER(_I), _P, _I, _I, _P, _P, _I, _P, _I, _P, C.c_size_t]),
    'laff_netvlad_train_reserve_bytes': (C.c_int, [_I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_netvlad_backward_workspace_bytes': (C.c_int, [_I, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_netvlad_encode_train': (C.c_int, [_P, _P, _I, _I, _P, _P, C.POINTER(_I), _P, _I, _I, _P, _P, _I, _P, _I, _P, C.c_size_t, _P,
                                            C.c_size_t]),
    'laff_netvlad_backward': (C.c_int, [_P, _P, _I, _I, _P, _P, C.POINTER(_I), _P, _I, _I, _P, _P, _I, _P, _I, _P, _I, _P, C.c_size_t,
                                        _P, _P, _P, C.c_size_t]),
    'laff_batch_assemble': (C.c_int, [_P, C.POINTER(AssembleJob), _I, _I, _P, _P, _I]),
    'laff_rerank_workspace_bytes': (C.c_int, [C.POINTER(RerankProblem), _I, _I, _I, C.POINTER(C.c_size_t)]),
    'laff_rerank_run': (C.c_int, [_P, C.POINTER(RerankProblem), _I, _I, _I, _F, _P, C.c_size_t]),
    'laff_rerank_tkb': (C.c_int, [_P, _P, _I, _I, _P, _I, _I, _P, _P, _I]),
    'laff_sim_hist': (C.c_int, [_P, _P, C.c_long, _P, C.c_long, _I, _I, _I, _I, _F, _P, C.c_long]),
}

_lib = None


def load():
    """Load the library once; raises if it has not been built (python -m laff_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('liblaff_hip.so is missing (%s): build it with `python -m laff_amd.build`; '
                               'laff_amd has no CPU fallback' % LIB_PATH)
        # torch bundles its own libamdhip64.so (same SONAME as /opt/rocm's).  It must be in the process BEFORE
        # liblaff_hip.so is loaded so that both resolve to ONE HIP runtime (shared streams / allocations); loaded
        # the other way round the second runtime sees no device.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if lib.laff_abi_version() != ABI_VERSION:
            raise RuntimeError('liblaff_hip.so ABI %d != binding ABI %d: rebuild' % (lib.laff_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError('liblaff_hip: %s (rc=%d)' % (load().laff_last_error().decode(), rc))

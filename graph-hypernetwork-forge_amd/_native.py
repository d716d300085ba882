"""ctypes binding of libghf_hip.so (the C ABI in include/ghf.h).

There is no CPU or eager-PyTorch fallback behind these functions: if the
library cannot be loaded the first call raises, loudly.  torch appears here
only to obtain device pointers and the current HIP stream.
"""

from __future__ import annotations

import ctypes as C
import os
import re
import threading
from typing import List, Optional, Sequence, Tuple

import torch

from . import _build

_lock = threading.Lock()
_lib: Optional[C.CDLL] = None

ABI_VERSION = 15
GHF_FLAG_NO_TAIL = 1
GHF_FLAG_RAW_SUM = 2
GHF_FLAG_ZERO_SRC = 4
GHF_FLAG_ZERO_DST = 8
GHF_FLAG_ADD_H = 16
SRC_MASK = (1 << 28) - 1        # sorted_src of block plans: node id below bit 28, run head above
WLAYOUT_NATURAL = 0
WLAYOUT_FRAG16 = 1
WLAYOUT_SPLIT2H = 3         # fp16 B fragments, 2 pieces per weight scaled by a power of two per relation (+ the scales)
SPLIT_LAYOUTS = (WLAYOUT_SPLIT2H,)   # layouts whose kernels gather pre-split rows (split_rows)

_vp, _i32, _i64, _f32, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t

# name -> (restype, argtypes); must list every function declared in include/ghf.h
SIGNATURES = {
    "ghf_abi_version": (_i32, []),
    "ghf_last_error": (C.c_char_p, []),
    "ghf_host_checksum64": (C.c_uint64, [_vp, _sz, C.c_uint64]),
    "ghf_host_word_ids": (C.c_longlong, [_vp, C.c_longlong, _vp, _vp, C.c_longlong, C.c_int]),
    "ghf_message_config": (_i32, [_i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "ghf_plan_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "ghf_plan_max_chunks": (_i64, [_i64, _i64, _i32, _i32, _i32]),
    "ghf_plan_max_items": (_i64, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "ghf_plan_build": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp]),
    "ghf_subgraph_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_subgraph_hops": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _sz, _vp, _vp]),
    "ghf_subgraph_nodes": (_i32, [_vp, _i64, _i32, _vp, _sz, _vp, _vp, _vp, _vp]),
    "ghf_subgraph_edges": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp]),
    "ghf_subgraph_sample_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_subgraph_sample_hops": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _i32, C.POINTER(_i32), C.c_uint64, _vp, _sz,
                                        _vp, _vp, C.POINTER(_i64), _vp]),
    "ghf_subgraph_sample_edges": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "ghf_subgraph_hops_excl": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _sz, _vp, _vp, _vp, _i64, _i32]),
    "ghf_subgraph_edges_excl": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i64,
                                       _i32]),
    "ghf_subgraph_sample_hops_excl": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _i32, C.POINTER(_i32), C.c_uint64, _vp,
                                             _sz, _vp, _vp, C.POINTER(_i64), _vp, _vp, _i64, _i32]),
    "ghf_weightgen_fwd": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_vp), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp,
                                 _vp, _vp, _vp, _vp, _vp, _vp]),
    "ghf_weightgen_fwd_batched": (_i32, [_i32, _vp, C.POINTER(_vp), C.POINTER(_vp), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp,
                                         C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "ghf_input_proj_fwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp]),
    "ghf_text_encode_fwd": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "ghf_message_layer_fwd": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i32, _i32,
                                     _vp, _vp, _vp, _i32,
                                     _vp, _vp, _f32, _i64, _i64, _vp, _vp, _vp, _i32, _vp]),
    "ghf_message_side_output_supported": (_i32, [_i32, _i32, _i32]),
    "ghf_split_rows": (_i32, [_vp, _i64, _i32, _i64, _i64, _i32, _vp, _vp]),
    "ghf_split_rows_bytes": (_sz, [_i64, _i32, _i32]),
    "ghf_weights_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "ghf_group_workspace_bytes": (_sz, [_i64]),
    "ghf_group_edges": (_i32, [_vp, _i64, _i32, _vp, _sz, _vp, _vp, _vp]),
    "ghf_tail_bwd_workspace_floats": (_sz, [_i64, _i32]),
    "ghf_segment_axpy": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp]),
    "ghf_tail_bwd": (_i32, [_vp, _vp, _vp, _vp, _f32, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ghf_colsum_workspace_floats": (_sz, [_i64, _i32]),
    "ghf_colsum": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp]),
    "ghf_relu_mask": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "ghf_group_outer": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp]),
    "ghf_message_rs_supported": (_i32, [_i32]),
    "ghf_edge_transform_fwd": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "ghf_weights_rs_bytes": (_sz, [_i32, _i32]),
    "ghf_weights_pack_rs": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "ghf_edge_transform_h_fwd": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp]),
    "ghf_run_rows_fwd": (_i32, [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp]),
    "ghf_segment_partial_fwd": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "ghf_segment_tail_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _i64, _i32, _vp, _vp, _i64, _i32, _vp]),
    "ghf_edge_outer_supported": (_i32, [_i32]),
    "ghf_edge_outer": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i64, _vp, _vp, _vp, _vp]),
    "ghf_edge_outer_scaled": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i64, _vp, _vp, _vp, _vp]),
    "ghf_scale_exp": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "ghf_add3": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "ghf_rowscale": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "ghf_dot": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "ghf_weightgen_acts": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ghf_weightgen_bwd_supported": (_i32, [_i32, _i32, _i32]),
    "ghf_weightgen_bwd_workspace_floats": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "ghf_weightgen_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ghf_text_encode_bwd": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ghf_transpose_batched": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "ghf_weights_pack": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "ghf_score_pairs_fwd": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp]),
    "ghf_score_rank_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_score_rank": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_topk_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "ghf_score_topk": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_softmax_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_score_softmax_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_softmax_bwd_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_score_softmax_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_bce_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_score_bce_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _vp, _sz, _vp, _vp]),
    "ghf_score_bce_bwd_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_score_bce_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_rank_sub_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_score_rank_sub": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_topk_sub_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i64]),
    "ghf_score_topk_sub": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_softmax_sub_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_score_softmax_fwd_sub": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _i64, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_softmax_bwd_sub_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_score_softmax_bwd_sub": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _vp, _vp, _i64, _vp, _sz, _vp,
                                         _vp, _vp]),
    "ghf_score_bce_sub_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_score_bce_fwd_sub": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _vp, _i64, _vp, _sz, _vp, _vp]),
    "ghf_score_bce_bwd_sub_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_score_bce_bwd_sub": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _vp, _vp, _vp, _i64, _vp, _sz, _vp,
                                     _vp, _vp]),
    "ghf_score_rank_b_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_rank_b": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_topk_b_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i32, _i64]),
    "ghf_score_topk_b": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ghf_score_softmax_b_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_softmax_fwd_b": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _i64, _vp, _vp, _sz, _vp, _vp,
                                       _vp]),
    "ghf_score_softmax_bwd_b_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_softmax_bwd_b": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _vp, _vp, _i64, _vp, _vp, _sz,
                                       _vp, _vp, _vp, _vp]),
    "ghf_score_bce_b_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_bce_fwd_b": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _vp, _i64, _vp, _vp, _sz, _vp, _vp]),
    "ghf_score_bce_bwd_b_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_bce_bwd_b": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _vp, _vp, _vp, _i64, _vp, _vp, _sz,
                                   _vp, _vp, _vp, _vp]),
    "ghf_score_negsamp_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_negsamp_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _f32, _vp, _i64, _vp, _vp, _sz,
                                     _vp, _vp, _vp]),
    "ghf_score_negsamp_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_negsamp_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _f32, _vp, _vp, _vp, _i64, _vp,
                                     _vp, _sz, _vp, _vp, _vp, _vp]),
    "ghf_relation_rows_workspace_bytes": (_sz, [_i64, _i32]),
    "ghf_relation_rows": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _sz, _vp, _vp]),
    "ghf_relation_scores": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp]),
    "ghf_relation_scores_bwd_rows_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_relation_scores_bwd_rows": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _sz, _vp, _vp]),
    "ghf_relation_scores_bwd_weights_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ghf_relation_scores_bwd_weights": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _sz, _vp, _vp, _vp]),
    "ghf_rows_pack": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "ghf_rows_unpack": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
    "ghf_rows_accumulate": (_i32, [_vp, _vp, _i64, _i64, _vp, _i32, _vp]),
    "ghf_rows_accumulate_any": (_i32, [_vp, _vp, _i64, _i64, _vp, _i32, _vp]),
    "ghf_tail_fwd": (_i32, [_vp, _vp, _vp, _vp, _f32, _i64, _i64, _i32, _vp, _vp, _vp]),
    "ghf_set_range_flag": (_i32, [_vp]),
}

# include/ghf_negatives.h (per-query negative sets, csrc/negatives.hip): a table of its own — SIGNATURES is include/ghf.h's
NEG_SIGNATURES = {
    "ghf_neg_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_neg_rank": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _sz, _vp, _vp, _vp]),
    "ghf_neg_softmax_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _i64, _vp, _vp, _sz, _vp, _vp,
                                   _vp]),
    "ghf_neg_negsamp_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _f32, _vp, _i64, _vp, _vp, _sz,
                                   _vp, _vp, _vp]),
    "ghf_neg_bwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _f32, _vp, _i64, _vp, _vp, _vp,
                           _vp, _sz, _vp, _vp, _vp]),
}
NEG_SOFTMAX, NEG_NEGSAMP = 0, 1          # ghf_neg_bwd's mode

# include/ghf_distance.h (distance scores for per-query negative sets, csrc/distance.hip): the third table
DIST_SIGNATURES = {
    "ghf_dist_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_dist_rank": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _sz, _vp, _vp, _vp]),
    "ghf_dist_softmax_fwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _i64, _vp, _sz, _vp, _vp,
                                    _vp]),
    "ghf_dist_negsamp_fwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _f32, _vp, _i64, _vp, _sz,
                                    _vp, _vp, _vp]),
    "ghf_dist_bwd": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _f32, _vp, _i64, _vp, _vp,
                            _vp, _sz, _vp, _vp, _vp]),
    "ghf_dist_rows_grad": (_i32, [_i32, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp]),
}
DIST_L1, DIST_L2, DIST_COMPLEX = 1, 2, 3  # the metric of the ghf_dist_* calls
DIST_METRICS = {"l1": DIST_L1, "l2": DIST_L2, "complex": DIST_COMPLEX}

# include/ghf_distance_sweep.h (distance scores against every node or a candidate subset, csrc/distance_sweep.hip): the fourth
DSWEEP_SIGNATURES = {
    "ghf_dist_sweep_rank_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_dist_sweep_rank": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _sz, _vp, _vp,
                                   _vp]),
    "ghf_dist_sweep_topk_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i64]),
    "ghf_dist_sweep_topk": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _sz, _vp, _vp,
                                   _vp]),
}


# include/ghf_distance_loss.h (the two losses under a distance against every node or a candidate subset, csrc/distance_loss.hip):
# the fifth
DLOSS_SIGNATURES = {
    "ghf_dist_loss_fwd_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_dist_loss_softmax_fwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _vp, _i64, _vp, _sz, _vp,
                                         _vp, _vp]),
    "ghf_dist_loss_negsamp_fwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _f32, _vp, _i64, _vp,
                                         _sz, _vp, _vp, _vp]),
    "ghf_dist_loss_bwd_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_dist_loss_bwd": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _f32, _vp, _i64, _vp,
                                 _vp, _vp, _sz, _vp, _vp, _vp]),
}


# include/ghf_pairwise.h (pairwise ranking losses on per-query negative sets, csrc/pairwise.hip): the sixth
PAIR_SIGNATURES = {
    "ghf_pair_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_pair_fwd": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _i64, _vp, _vp,
                            _sz, _vp, _vp, _vp, _vp]),
    "ghf_pair_bwd": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _i64, _vp, _vp,
                            _vp, _vp, _sz, _vp, _vp, _vp]),
}
PAIR_DOT = 0                              # the metric of the ghf_pair_* calls: PAIR_DOT or DIST_L1 / DIST_L2 / DIST_COMPLEX
PAIR_HINGE, PAIR_LOGISTIC = 1, 2          # their kind
PAIR_KINDS = {"hinge": PAIR_HINGE, "logistic": PAIR_LOGISTIC}


# include/ghf_pairwise_sweep.h (the pairwise losses under a distance against every node or a candidate subset,
# csrc/pairwise_sweep.hip): the seventh
PAIRSWEEP_SIGNATURES = {
    "ghf_dist_pair_fwd_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_dist_pair_fwd": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _i64, _vp,
                                 _sz, _vp, _vp, _vp, _vp, _vp]),
    "ghf_dist_pair_bwd_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64]),
    "ghf_dist_pair_bwd": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _i64, _vp,
                                 _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
}


# include/ghf_pairwise_dot_sweep.h (the pairwise losses by dot product against every node or a candidate subset,
# csrc/pairwise_dot_sweep.hip + csrc/softmax.hip): the eighth
PAIRDOT_SIGNATURES = {
    "ghf_score_pair_fwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_pair_fwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _i64, _vp, _vp,
                                  _sz, _vp, _vp, _vp, _vp, _vp]),
    "ghf_score_pair_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i64]),
    "ghf_score_pair_bwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _i64, _vp, _vp,
                                  _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
}


def header_symbols() -> List[str]:
    """Function names declared in include/ghf.h (for the export test)."""
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", text)))


def negatives_header_symbols() -> List[str]:
    """Function names declared in include/ghf_negatives.h."""
    with open(os.path.join(_build.INCLUDE, "ghf_negatives.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", text)))


def distance_header_symbols() -> List[str]:
    """Function names declared in include/ghf_distance.h."""
    with open(os.path.join(_build.INCLUDE, "ghf_distance.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", text)))


def distance_sweep_header_symbols() -> List[str]:
    """Function names declared in include/ghf_distance_sweep.h."""
    with open(os.path.join(_build.INCLUDE, "ghf_distance_sweep.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", text)))


def distance_loss_header_symbols() -> List[str]:
    """Function names declared in include/ghf_distance_loss.h."""
    with open(os.path.join(_build.INCLUDE, "ghf_distance_loss.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", text)))


def pairwise_header_symbols() -> List[str]:
    """Function names declared in include/ghf_pairwise.h."""
    with open(os.path.join(_build.INCLUDE, "ghf_pairwise.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(ghf_pair_[a-z_0-9]+)\s*\(", text)))


def pairwise_sweep_header_symbols() -> List[str]:
    """Function names declared in include/ghf_pairwise_sweep.h."""
    with open(os.path.join(_build.INCLUDE, "ghf_pairwise_sweep.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ghf_dist_pair_[a-z_0-9]+)\s*\(", text)))


def pairwise_dot_sweep_header_symbols() -> List[str]:
    """Function names declared in include/ghf_pairwise_dot_sweep.h."""
    with open(os.path.join(_build.INCLUDE, "ghf_pairwise_dot_sweep.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ghf_score_pair_[a-z_0-9]+)\s*\(", text)))


def lib_path() -> str:
    return _build.LIB_PATH


def load() -> C.CDLL:
    """Load libghf_hip.so (building it first if it is absent and hipcc is here)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = _build.LIB_PATH
        if not os.path.exists(path):
            try:
                _build.build()
            except Exception as exc:  # noqa: BLE001
                raise RuntimeError(
                    f"libghf_hip.so is missing at {path} and could not be built ({exc}). "
                    "This package has no CPU/PyTorch fallback: run __graft_entry__.build() first.") from exc
        lib = C.CDLL(path)
        for name, (res, args) in (list(SIGNATURES.items()) + list(NEG_SIGNATURES.items()) + list(DIST_SIGNATURES.items())
                                  + list(DSWEEP_SIGNATURES.items()) + list(DLOSS_SIGNATURES.items()) + list(PAIR_SIGNATURES.items())
                                  + list(PAIRSWEEP_SIGNATURES.items()) + list(PAIRDOT_SIGNATURES.items())):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.ghf_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libghf_hip.so ABI version {lib.ghf_abi_version()} != {ABI_VERSION}")
        if os.environ.get("GHF_TRACE_CALLS") == "1":          # diagnostics: name every C-ABI call on stderr and wait for it
            lib = _Traced(lib)
        _lib = lib
        return lib


class _Traced:
    """GHF_TRACE_CALLS=1: every entry point prints its name before it is enqueued and synchronises the device after — the last
    name on stderr is the call whose kernel faulted."""

    def __init__(self, lib) -> None:
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ghf_") or name in ("ghf_last_error", "ghf_abi_version", "ghf_host_checksum64", "ghf_host_word_ids"):
            return fn

        def call(*args):
            import sys
            print(f"[ghf] {name}", file=sys.stderr, flush=True)
            rc = fn(*args)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            return rc
        return call


class GhfError(RuntimeError):
    pass


def _check(code: int, what: str) -> None:
    if code != 0:
        msg = load().ghf_last_error().decode("utf-8", "replace")
        if code == -1:
            raise ValueError(f"{what}: {msg}")
        raise GhfError(f"{what} failed (code {code}): {msg}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    # the raw getter: torch.cuda.current_stream() without a device index walks through torch.cuda.is_available()
    # (environment lookups, ~40 us per launch on the GPU box — more than most of these kernels' launch cost)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _req(t: torch.Tensor, dtype: torch.dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        # launches go to the CURRENT device's stream (_stream): a tensor elsewhere would be read from the wrong GPU's queue
        raise RuntimeError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}: "
                           "call torch.cuda.set_device(tensor.device) first (one process drives one GPU)")
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------------
# thin wrappers (tensors in, tensors out; all work enqueued on the current stream)
# ---------------------------------------------------------------------------

# ---- range guard of the two-fp16-piece kernels (include/ghf.h: ghf_set_range_flag) -------------------------------
RANGE_ROWS, RANGE_WEIGHTS, RANGE_WEAK_W = 1, 2, 4
_range_flag: Optional[torch.Tensor] = None


def range_guard_enabled() -> bool:
    return os.environ.get("GHF_RANGE_GUARD", "1") != "0"


def range_flag(device) -> torch.Tensor:
    """The int32 device word the cutting kernels OR into (registered once per process)."""
    global _range_flag
    if _range_flag is None or _range_flag.device != torch.device(device):
        _range_flag = torch.zeros(1, dtype=torch.int32, device=device)
        _check(load().ghf_set_range_flag(_range_flag.data_ptr()), "ghf_set_range_flag")
    return _range_flag


class RangeFlagRead:
    """The guard word read EARLY: every bit a forward on the block kernels can raise is raised before its last layer is
    launched (rows are cut by the input projection and by the tails of the layers before the last; weights are packed
    before their layer starts), so the 4-byte copy is enqueued on a side stream behind an event recorded just before that
    launch, and the host waits for the copy while the GPU runs the last layer — it is back in time to enqueue the next
    forward, where a read at the very end left the GPU idle for the host's launch latency (C3: ~0.3 ms per forward)."""
    _host: Optional[torch.Tensor] = None
    _stream = None

    def __init__(self, flag: torch.Tensor) -> None:
        cls = RangeFlagRead
        if cls._host is None:
            cls._host = torch.zeros(1, dtype=torch.int32).pin_memory()
        if cls._stream is None or cls._stream.device != flag.device:
            cls._stream = torch.cuda.Stream(device=flag.device)
        self.flag, self.done = flag, None

    def arm(self) -> None:
        """Call on the forward's stream right before its last layer is enqueued."""
        cls = RangeFlagRead
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.flag.device))
        cls._stream.wait_event(ev)
        with torch.cuda.stream(cls._stream):
            cls._host.copy_(self.flag, non_blocking=True)
            self.done = torch.cuda.Event()
            self.done.record(cls._stream)

    def value(self) -> int:
        if self.done is None:                       # never armed (a path without an early point): a plain read
            return int(self.flag.item())
        self.done.synchronize()
        return int(RangeFlagRead._host[0])


def message_config(d: int, kernel: Optional[str] = None) -> Tuple[int, int, int, int]:
    """(block_nodes, weight layout, chunk_rows, split_chunks) of the message kernel for hidden size d; `kernel` names one
    as GHF_KERNEL would ("pp": the exact fp32-MFMA kernel, "generic", ...)."""
    bn, wl, cr, sc = _i32(0), _i32(0), _i32(0), _i32(0)
    lib = load()                                    # (before taking the lock: load() takes it too)
    with _lock:
        old = os.environ.get("GHF_KERNEL")
        try:
            if kernel is not None:
                os.environ["GHF_KERNEL"] = kernel
            _check(lib.ghf_message_config(int(d), C.byref(bn), C.byref(wl), C.byref(cr), C.byref(sc)), "ghf_message_config")
        finally:
            if kernel is not None:
                if old is None:
                    os.environ.pop("GHF_KERNEL", None)
                else:
                    os.environ["GHF_KERNEL"] = old
    return bn.value, wl.value, cr.value, sc.value


def _exclude_args(exclude, seeds: torch.Tensor):
    """`exclude` = (keys, typed) of subgraph / subgraph_sample as the C arguments (excl, n_excl, typed): keys a sorted int64
    tensor on the seeds' device (include/ghf.h: the key encoding; sorting is the caller's duty), typed a bool."""
    keys, typed = exclude
    keys = _req(keys, torch.int64, "exclude keys")
    if keys.dim() != 1 or keys.device != seeds.device:
        raise ValueError(f"exclude keys must be a 1-D tensor on {seeds.device}, got {tuple(keys.shape)} on {keys.device}")
    return keys, (_ptr(keys) if keys.numel() else None, keys.numel(), 1 if typed else 0)


def subgraph(plan, seeds: torch.Tensor, k: int, exclude=None) -> dict:
    """The k-hop in-neighbourhood of `seeds` (int64, on the plan's device, ids in [0, N)) in `plan`'s graph
    (include/ghf.h: ghf_subgraph_*): dist [N] int32, node_list [m_k] int64 ordered by (dist, id), new_id [N] int64 (-1 beyond
    k hops), m: the host list m_0..m_k (m_j = nodes within j hops: the first m_j entries of node_list), and the induced edges
    edge_index [2, E'] / rel [E'] int64 (destinations within k - 1 hops), renumbered, in the plan's sorted order.  One host
    sync (the counts).  `exclude` = (keys, typed): the edges named by the sorted keys do not exist for the call
    (ghf_subgraph_*_excl); None calls exactly what is called without it."""
    lib = load()
    seeds = _req(seeds, torch.int64, "seeds")
    if exclude is not None:
        excl_keys, excl = _exclude_args(exclude, seeds)             # (excl_keys: alive until the counts are read)
    dev, N, E = seeds.device, plan.N, plan.E
    ws_bytes = lib.ghf_subgraph_workspace_bytes(N, E, k)
    if ws_bytes == 0:
        raise ValueError(f"subgraph: bad sizes N={N} E={E} k={k}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    dist = torch.empty(N, dtype=torch.int32, device=dev)
    node_list = torch.empty(N, dtype=torch.int64, device=dev)
    new_id = torch.empty(N, dtype=torch.int64, device=dev)
    counts = torch.empty(k + 2, dtype=torch.int64, device=dev)           # m_0 .. m_k, E'
    edge_out = torch.empty((2, max(E, 1)), dtype=torch.int64, device=dev)
    rel_out = torch.empty(max(E, 1), dtype=torch.int64, device=dev)
    key, src, st = _ptr(plan.sorted_key), _ptr(plan.sorted_src), _stream()
    hops = (key, src, N, E, plan.R, plan.block_nodes, _ptr(seeds), seeds.numel(), k, _ptr(ws), ws_bytes, _ptr(dist), st)
    if exclude is None:
        _check(lib.ghf_subgraph_hops(*hops), "ghf_subgraph_hops")
    else:
        _check(lib.ghf_subgraph_hops_excl(*hops, *excl), "ghf_subgraph_hops_excl")
    _check(lib.ghf_subgraph_nodes(_ptr(dist), N, k, _ptr(ws), ws_bytes, _ptr(node_list), _ptr(new_id), _ptr(counts), st),
           "ghf_subgraph_nodes")
    edges = (key, src, N, E, plan.R, plan.block_nodes, _ptr(dist), _ptr(new_id), k, _ptr(ws), ws_bytes, _ptr(edge_out),
             _ptr(rel_out), counts.data_ptr() + 8 * (k + 1), st)
    if exclude is None:
        _check(lib.ghf_subgraph_edges(*edges), "ghf_subgraph_edges")
    else:
        _check(lib.ghf_subgraph_edges_excl(*edges, *excl), "ghf_subgraph_edges_excl")
    c = counts.cpu().tolist()
    m, E_sub = c[:k + 1], c[k + 1]
    return dict(dist=dist, node_list=node_list[:m[k]], new_id=new_id, m=m,
                edge_index=edge_out[:, :E_sub] if E else edge_out[:, :0], rel=rel_out[:E_sub])


def subgraph_sample(plan, seeds: torch.Tensor, fanout: Sequence[int], seed: int, exclude=None) -> dict:
    """`subgraph` with per-hop fanout caps (include/ghf.h: ghf_subgraph_sample_*): k = len(fanout) hops, hop j keeping at most
    fanout[j] in-edges (-1: all) of each node first reached at sampled distance j — the ones with the smallest
    (priority(seed, plan position), plan position).  The keys of `subgraph`, plus host_reads: the words read back inside the
    hops stage (at most one per capped hop); one more host sync for the counts.  `exclude` as in `subgraph`: excluded edges
    are no candidates (ghf_subgraph_sample_hops_excl); the priorities stay those of the full plan's positions."""
    lib = load()
    seeds = _req(seeds, torch.int64, "seeds")
    if exclude is not None:
        excl_keys, excl = _exclude_args(exclude, seeds)             # (excl_keys: alive until the counts are read)
    fanout = [int(f) for f in fanout]
    k = len(fanout)
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"subgraph_sample: seed {seed} is not a 64-bit unsigned integer")
    dev, N, E = seeds.device, plan.N, plan.E
    ws_bytes = lib.ghf_subgraph_sample_workspace_bytes(N, E, k)
    if ws_bytes == 0:
        raise ValueError(f"subgraph_sample: bad sizes N={N} E={E} k={k}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    dist = torch.empty(N, dtype=torch.int32, device=dev)
    keep = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    node_list = torch.empty(N, dtype=torch.int64, device=dev)
    new_id = torch.empty(N, dtype=torch.int64, device=dev)
    counts = torch.empty(k + 2, dtype=torch.int64, device=dev)           # m_0 .. m_k, E'
    edge_out = torch.empty((2, max(E, 1)), dtype=torch.int64, device=dev)
    rel_out = torch.empty(max(E, 1), dtype=torch.int64, device=dev)
    key, src, st = _ptr(plan.sorted_key), _ptr(plan.sorted_src), _stream()
    reads = _i64(0)
    hops = (key, src, N, E, plan.R, plan.block_nodes, _ptr(seeds), seeds.numel(), k, (_i32 * k)(*fanout), int(seed), _ptr(ws),
            ws_bytes, _ptr(dist), _ptr(keep), C.byref(reads), st)
    if exclude is None:
        _check(lib.ghf_subgraph_sample_hops(*hops), "ghf_subgraph_sample_hops")
    else:
        _check(lib.ghf_subgraph_sample_hops_excl(*hops, *excl), "ghf_subgraph_sample_hops_excl")
    _check(lib.ghf_subgraph_nodes(_ptr(dist), N, k, _ptr(ws), ws_bytes, _ptr(node_list), _ptr(new_id), _ptr(counts), st),
           "ghf_subgraph_nodes")
    _check(lib.ghf_subgraph_sample_edges(key, src, N, E, plan.R, plan.block_nodes, _ptr(keep), _ptr(new_id), _ptr(ws), ws_bytes,
                                         _ptr(edge_out), _ptr(rel_out), counts.data_ptr() + 8 * (k + 1), st),
           "ghf_subgraph_sample_edges")
    c = counts.cpu().tolist()
    m, E_sub = c[:k + 1], c[k + 1]
    return dict(dist=dist, node_list=node_list[:m[k]], new_id=new_id, m=m,
                edge_index=edge_out[:, :E_sub] if E else edge_out[:, :0], rel=rel_out[:E_sub], host_reads=reads.value)


def exact_config(d: int) -> Tuple[int, int, int, int]:
    """The plan geometry of the exact (fp32 fma chain) kernel for hidden size d: the fp32-MFMA block kernel where one exists
    (d = 64, 128), else a CSR plan (generic kernel; relation-stationary layer on fp32 MFMAs for wide rows)."""
    cfg = message_config(d, "pp")
    return cfg if cfg[1] == WLAYOUT_FRAG16 else (1, WLAYOUT_NATURAL, 0, 0)


def plan_build(edge_index: torch.Tensor, rel_id: torch.Tensor, N: int, R: int, block_nodes: int, chunk_rows: int = 0,
               split_chunks: int = 0):
    """Returns a dict of the plan's device arrays (names as in include/ghf.h: ghf_plan_build) plus `status` [3]."""
    lib = load()
    ei = _req(edge_index, torch.int64, "edge_index")
    rel = _req(rel_id, torch.int64, "rel_id")
    E = ei.size(1)
    dev = ei.device
    nb = (N + block_nodes - 1) // block_nodes
    nseg = N if block_nodes == 1 else nb * R
    ws_bytes = lib.ghf_plan_workspace_bytes(N, E, R, block_nodes, chunk_rows)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)       # noqa: E731
    out = dict(sorted_key=i32(E), sorted_src=i32(E), seg_off=i32(nseg + 1), indeg=i32(N), status=i32(3),
               chunk_tab=None, blk_chunk_off=None, item_tab=None, blk_item_off=None)   # sorted_key: uint32 bit patterns
    if block_nodes > 1:
        out["chunk_tab"] = torch.zeros(2 * lib.ghf_plan_max_chunks(N, E, R, block_nodes, chunk_rows), dtype=torch.int32,
                                       device=dev)
        out["blk_chunk_off"] = i32(nb + 1)
        out["item_tab"] = torch.zeros(4 * lib.ghf_plan_max_items(N, E, R, block_nodes, chunk_rows, split_chunks),
                                      dtype=torch.int32, device=dev)
        out["blk_item_off"] = i32(nb + 1)
    _check(lib.ghf_plan_build(_ptr(ei), _ptr(rel), N, E, R, block_nodes, chunk_rows, split_chunks, _ptr(ws), ws_bytes,
                              _ptr(out["sorted_key"]), _ptr(out["sorted_src"]), _ptr(out["seg_off"]), _ptr(out["indeg"]),
                              _ptr(out["chunk_tab"]), _ptr(out["blk_chunk_off"]), _ptr(out["item_tab"]),
                              _ptr(out["blk_item_off"]), _ptr(out["status"]), _stream()), "ghf_plan_build")
    return out


def weightgen_fwd(text_emb: torch.Tensor, head_params: Sequence[torch.Tensor], log_scales: Sequence[torch.Tensor],
                  T: int, Hh: int, num_hidden: int, d_in: int, d_out: int, layout: int,
                  out: Optional[Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]] = None,
                  hidden_drop: Optional[torch.Tensor] = None, want_acts: bool = False):
    """head_params: flat list [head][layer][weight,bias]; log_scales: the three 1-element tensors (W_msg, W_self, bias),
    read in place; hidden_drop: scaled dropout masks [3, num_hidden, R, Hh] of the hidden activations (training);
    returns (W_msg or Wfrag, W_self or None, bias) — and, with want_acts, a fourth entry: the hidden activations
    [3, num_hidden, R, Hh] the same launch leaves for the backward (weightgen_acts' result; None without hidden layers)."""
    lib = load()
    x = _req(text_emb, torch.float32, "text_emb")
    R = x.size(0)
    dev = x.device
    keep = [_req(p, torch.float32, "weight-generator parameter") for p in head_params]
    arr = (_vp * len(keep))(*[p.data_ptr() for p in keep])
    if isinstance(log_scales, torch.Tensor):                  # a [3] tensor: three views of it
        log_scales = [log_scales[i:i + 1] for i in range(3)]
    ls_keep = [_req(t, torch.float32, "log_scale") for t in log_scales]
    if len(ls_keep) != 3:
        raise ValueError("weightgen_fwd: three log-scale tensors expected (W_msg, W_self, bias)")
    ls = (_vp * 3)(*[t.data_ptr() for t in ls_keep])
    hidden_ws = torch.empty(3 * 2 * R * max(Hh, T, 1), dtype=torch.float32, device=dev)
    if out is None:
        if layout != WLAYOUT_NATURAL:                # one opaque buffer holds [W_msg; W_self] in the kernel's order
            W_msg = torch.empty(lib.ghf_weights_bytes(R, d_in, d_out, layout) // 4, dtype=torch.float32, device=dev)
            W_self = None
        else:
            W_msg = torch.empty(R, d_in, d_out, dtype=torch.float32, device=dev)
            W_self = torch.empty(R, d_in, d_out, dtype=torch.float32, device=dev)
        bias = torch.empty(R, d_out, dtype=torch.float32, device=dev)
    else:
        W_msg, W_self, bias = out
    acts = torch.empty(3, num_hidden, R, Hh, dtype=torch.float32, device=dev) if want_acts and num_hidden > 0 else None
    _check(lib.ghf_weightgen_fwd(_ptr(x), arr, ls, R, T, Hh, num_hidden, d_in, d_out, layout,
                                 _ptr(hidden_ws), _ptr(W_msg), _ptr(W_self), _ptr(bias),
                                 _ptr(None if hidden_drop is None else _req(hidden_drop, torch.float32, "hidden_drop")), _ptr(acts),
                                 _stream()), "ghf_weightgen_fwd")
    return (W_msg, W_self, bias, acts) if want_acts else (W_msg, W_self, bias)


WG_BATCH_MAX = 8       # generators per ghf_weightgen_fwd_batched call: WG_MAX_L in csrc/weightgen.hip (kernel arguments below 4 KB)


def weightgen_fwd_batched(text_emb: torch.Tensor, head_params: Sequence[Sequence[torch.Tensor]], log_scales: Sequence[Sequence[torch.Tensor]],
                          T: int, Hh: int, num_hidden: int, d_in: int, d_out: int, layout: int):
    """All L generators of a model in one launch sequence (include/ghf.h: ghf_weightgen_fwd_batched): head_params[g] /
    log_scales[g] as weightgen_fwd takes them; returns [(W_msg or Wfrag, W_self or None, bias)] per generator."""
    lib = load()
    x = _req(text_emb, torch.float32, "text_emb")
    R, dev, L = x.size(0), x.device, len(head_params)
    keep = [_req(p, torch.float32, "weight-generator parameter") for g in head_params for p in g]
    arr = (_vp * len(keep))(*[p.data_ptr() for p in keep])
    ls_keep = [_req(t, torch.float32, "log_scale") for g in log_scales for t in g]
    if len(ls_keep) != 3 * L:
        raise ValueError("weightgen_fwd_batched: three log-scale tensors per generator expected")
    ls = (_vp * len(ls_keep))(*[t.data_ptr() for t in ls_keep])
    hidden_ws = torch.empty(L * 3 * 2 * R * max(Hh, T, 1), dtype=torch.float32, device=dev)
    outs = []
    for _ in range(L):
        if layout != WLAYOUT_NATURAL:
            W_msg = torch.empty(lib.ghf_weights_bytes(R, d_in, d_out, layout) // 4, dtype=torch.float32, device=dev)
            W_self = None
        else:
            W_msg = torch.empty(R, d_in, d_out, dtype=torch.float32, device=dev)
            W_self = torch.empty(R, d_in, d_out, dtype=torch.float32, device=dev)
        outs.append((W_msg, W_self, torch.empty(R, d_out, dtype=torch.float32, device=dev)))
    wm = (_vp * L)(*[o[0].data_ptr() for o in outs])
    wsf = (_vp * L)(*[(None if o[1] is None else o[1].data_ptr()) for o in outs])
    bs = (_vp * L)(*[o[2].data_ptr() for o in outs])
    _check(lib.ghf_weightgen_fwd_batched(L, _ptr(x), arr, ls, R, T, Hh, num_hidden, d_in, d_out, layout, _ptr(hidden_ws),
                                         wm, wsf, bs, _stream()), "ghf_weightgen_fwd_batched")
    return outs


def text_encode_fwd(ids: torch.Tensor, lens: torch.Tensor, char_emb: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[U, Lmax] int32 ids + [U] lengths -> [U, T] text embeddings (reference TextEncoder, all strings at once)."""
    ids = _req(ids, torch.int32, "ids")
    lens = _req(lens, torch.int32, "lens")
    E, Wt, bt = (_req(t, torch.float32, n) for t, n in ((char_emb, "char_emb.weight"), (W, "proj.weight"), (b, "proj.bias")))
    U, Lmax = ids.shape
    out = torch.empty(U, Wt.size(0), dtype=torch.float32, device=ids.device)
    _check(load().ghf_text_encode_fwd(_ptr(ids), _ptr(lens), U, Lmax, _ptr(E), E.size(0), E.size(1), _ptr(Wt), _ptr(bt),
                                      Wt.size(0), _ptr(out), _stream()), "ghf_text_encode_fwd")
    return out


def input_proj_fwd(x: torch.Tensor, W_in: torch.Tensor, b_in: torch.Tensor, out: Optional[torch.Tensor] = None,
                   h_split: Optional[torch.Tensor] = None, split_layout: int = 0):
    lib = load()
    x = _req(x, torch.float32, "node_features")
    W = _req(W_in, torch.float32, "input_proj.weight")
    b = _req(b_in, torch.float32, "input_proj.bias")
    N, F = x.shape
    d = W.size(0)
    if W.size(1) != F:
        raise ValueError(f"node_features has {F} columns but input_proj expects {W.size(1)}")
    h0 = torch.empty(N, d, dtype=torch.float32, device=x.device) if out is None else out
    _check(lib.ghf_input_proj_fwd(_ptr(x), _ptr(W), _ptr(b), N, F, d, _ptr(h0), _ptr(h_split), split_layout, _stream()),
           "ghf_input_proj_fwd")
    return h0


def alloc_split(N: int, d: int, wlayout: int, device) -> torch.Tensor:
    """Uninitialised buffer for the split form of an [N, d] matrix (ghf_split_rows_bytes)."""
    nbytes = load().ghf_split_rows_bytes(N, d, wlayout)
    if nbytes == 0:
        raise ValueError(f"weight layout {wlayout} gathers h itself")
    return torch.empty((nbytes // 2,), dtype=torch.int16, device=device)


def split_rows(h: torch.Tensor, wlayout: int, out: Optional[torch.Tensor] = None, row0: int = 0,
               rows: Optional[int] = None) -> torch.Tensor:
    """Rows of h in the form the message kernel of `wlayout` gathers (include/ghf.h: ghf_split_rows): an opaque int16
    tensor — SPLIT2H: N*2*d fp16 bit patterns followed by N float scales."""
    lib = load()
    h = _req(h, torch.float32, "h")
    N, d = h.shape
    if out is None:
        out = alloc_split(N, d, wlayout, h.device)
    rows = N - row0 if rows is None else rows
    _check(lib.ghf_split_rows(_ptr(h), N, d, row0, rows, wlayout, _ptr(out), _stream()), "ghf_split_rows")
    return out


def message_layer_fwd(h: torch.Tensor, plan, W_msg: torch.Tensor, W_self: Optional[torch.Tensor],
                      bias: torch.Tensor, wlayout: int, ln_gamma: Optional[torch.Tensor],
                      ln_beta: Optional[torch.Tensor], ln_eps: float, h_out: torch.Tensor,
                      row0: int = 0, rows: Optional[int] = None, flags: int = 0,
                      h_split: Optional[torch.Tensor] = None, h_split_out: Optional[torch.Tensor] = None,
                      agg_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`plan` is a plan.GraphPlan: the device arrays, the host copy of the item offsets and the split-block scratch.
    SPLIT2H plans gather from `h_split` (split_rows(h, wlayout); made here when the caller has none) and can
    emit the split form of the rows they write into `h_split_out` for the next layer; `agg_out` (side_output_supported)
    also receives the aggregate before the tail."""
    lib = load()
    h = _req(h, torch.float32, "h")
    N, d = h.shape
    if rows is None:
        rows = N - row0
    item0, n_items, partial = plan.items_for(row0, rows, d)
    if wlayout in SPLIT_LAYOUTS and h_split is None:
        h_split = split_rows(h, wlayout)
    _check(lib.ghf_message_layer_fwd(_ptr(h), _ptr(h_split), N, d, _ptr(plan.sorted_key), _ptr(plan.sorted_src), _ptr(plan.seg_off),
                                     _ptr(plan.indeg), _ptr(plan.chunk_tab), _ptr(plan.blk_chunk_off), _ptr(plan.item_tab),
                                     _ptr(plan.blk_item_off), item0, n_items, _ptr(partial), plan.E, plan.R,
                                     plan.block_nodes, _ptr(W_msg), _ptr(W_self), _ptr(bias), wlayout, _ptr(ln_gamma),
                                     _ptr(ln_beta), float(ln_eps), row0, rows, _ptr(h_out), _ptr(h_split_out), _ptr(agg_out), flags,
                                     _stream()),
           "ghf_message_layer_fwd")
    return h_out


def side_output_supported(plan, d: int) -> bool:
    """Whether the plan's message kernel can also write the aggregate before the tail (message_layer_fwd's agg_out)."""
    return bool(load().ghf_message_side_output_supported(d, plan.block_nodes, plan.wlayout))


def score_pairs_fwd(a: torch.Tensor, b: torch.Tensor, ia: Optional[torch.Tensor] = None,
                    ib: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scores[i] = a[ia[i]] . b[ib[i]] (indices optional): reference score_triple with its callers' row gathers fused."""
    a = _req(a, torch.float32, "a")
    b = _req(b, torch.float32, "b")
    if a.dim() != 2 or b.dim() != 2 or a.size(1) != b.size(1):
        raise ValueError(f"score_pairs: need two [rows, d] matrices of equal d, got {tuple(a.shape)} and {tuple(b.shape)}")
    ia = None if ia is None else _req(ia, torch.int64, "ia")
    ib = None if ib is None else _req(ib, torch.int64, "ib")
    n = ia.numel() if ia is not None else (ib.numel() if ib is not None else a.size(0))
    if (ia is not None and ib is not None and ia.numel() != ib.numel()) or (ia is None and ib is None and a.size(0) != b.size(0)):
        raise ValueError("score_pairs: the two sides name different numbers of pairs")
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    _check(load().ghf_score_pairs_fwd(_ptr(a), _ptr(b), _ptr(ia), _ptr(ib), a.size(0), b.size(0), n, a.size(1), _ptr(out),
                                      _stream()), "ghf_score_pairs_fwd")
    return out


# ---- link prediction against every node (include/ghf.h: ghf_score_rank / ghf_score_topk, csrc/rank.hip) ----------------
def _rank_args(q: torch.Tensor, c: torch.Tensor, iq: Optional[torch.Tensor], filt_ptr: Optional[torch.Tensor],
               filt_idx: Optional[torch.Tensor], what: str):
    q = _req(q, torch.float32, "q")
    c = _req(c, torch.float32, "c")
    if q.dim() != 2 or c.dim() != 2 or q.size(1) != c.size(1) or q.size(0) == 0 or c.size(0) == 0:
        raise ValueError(f"{what}: need two non-empty [rows, d] matrices of equal d, got {tuple(q.shape)} and {tuple(c.shape)}")
    if q.device != c.device:
        raise RuntimeError(f"{what}: q is on {q.device}, c on {c.device}")
    iq = None if iq is None else _req(iq, torch.int64, "iq")
    if iq is not None and iq.dim() != 1:
        raise ValueError(f"{what}: iq must be 1-D")
    B = iq.numel() if iq is not None else q.size(0)
    if B == 0:
        raise ValueError(f"{what}: no queries")
    if (filt_ptr is None) != (filt_idx is None):
        raise ValueError(f"{what}: filt_ptr and filt_idx come together")
    nnz = 0
    if filt_ptr is not None:
        filt_ptr = _req(filt_ptr, torch.int64, "filt_ptr")
        filt_idx = _req(filt_idx, torch.int64, "filt_idx")
        if filt_ptr.dim() != 1 or filt_idx.dim() != 1 or filt_ptr.numel() != B + 1:
            raise ValueError(f"{what}: filt_ptr must hold B + 1 = {B + 1} offsets, got {tuple(filt_ptr.shape)}")
        nnz = filt_idx.numel()
    for name, t in (("iq", iq), ("filt_ptr", filt_ptr), ("filt_idx", filt_idx)):
        if t is not None and t.device != q.device:
            raise RuntimeError(f"{what}: {name} is on {t.device}, the embeddings on {q.device}")
    return q, c, iq, filt_ptr, filt_idx, B, nnz


def _workspace(workspace: Optional[torch.Tensor], size_fn, device, what: str, **sizes) -> torch.Tensor:
    """The workspace of call `what`: size_fn (its *_workspace_bytes) says how many bytes `sizes` need, 0 meaning the library
    cannot run them; the caller's workspace is checked against that, or a new one allocated."""
    need = size_fn(*sizes.values())
    if need == 0:
        raise ValueError(f"{what}: unsupported sizes " + " ".join(f"{k}={v}" for k, v in sizes.items()))
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    workspace = _req(workspace, torch.uint8, "workspace")
    if workspace.numel() < need:
        raise ValueError(f"{what}: workspace of {workspace.numel()} bytes, need {need}")
    return workspace


def _ic_arg(ic: Optional[torch.Tensor], c: torch.Tensor, what: str) -> Optional[torch.Tensor]:
    """The candidate subset of the ghf_score_*_sub calls (include/ghf.h): int64 [C] node ids on c's device, 1 <= C <= N.  That
    they ascend strictly and stay inside [0, N) is the device's check (a bad list makes every query invalid)."""
    if ic is None:
        return None
    ic = _req(ic, torch.int64, "ic")
    if ic.dim() != 1 or not 1 <= ic.numel() <= c.size(0):
        raise ValueError(f"{what}: ic must hold 1..N = {c.size(0)} candidate ids, got {tuple(ic.shape)}")
    if ic.device != c.device:
        raise RuntimeError(f"{what}: ic is on {ic.device}, the embeddings on {c.device}")
    return ic


def _bias_arg(bias: Optional[torch.Tensor], c: torch.Tensor, what: str) -> Optional[torch.Tensor]:
    """The per-candidate bias of the ghf_score_*_b calls (include/ghf.h): fp32 [N], one entry per row of c, on c's device.  Only
    metadata is looked at; the values are the device's business."""
    if bias is None:
        return None
    N = c.size(0)
    if (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or bias.dim() != 1 or bias.numel() != N
            or bias.device != c.device):
        got = f"{tuple(bias.shape)} {bias.dtype} on {bias.device}" if isinstance(bias, torch.Tensor) else type(bias).__name__
        raise ValueError(f"{what}: the bias must be a float32 tensor of shape [N = {N}] on {c.device}, got {got}")
    return bias.detach().contiguous()


def score_rank_b_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_rank_b_workspace_bytes(B, N, C, d, nnz))


def score_topk_b_workspace_bytes(B: int, N: int, C: int, d: int, k: int, nnz: int) -> int:
    return int(load().ghf_score_topk_b_workspace_bytes(B, N, C, d, k, nnz))


def score_softmax_b_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_softmax_b_workspace_bytes(B, N, C, d, nnz))


def score_softmax_bwd_b_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_softmax_bwd_b_workspace_bytes(B, N, C, d, nnz))


def score_bce_b_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_bce_b_workspace_bytes(B, N, C, d, nnz))


def score_bce_bwd_b_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_bce_bwd_b_workspace_bytes(B, N, C, d, nnz))


def score_rank_workspace_bytes(B: int, N: int, d: int) -> int:
    return int(load().ghf_score_rank_workspace_bytes(B, N, d))


def score_rank_sub_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_rank_sub_workspace_bytes(B, C, d, nnz))


def score_topk_sub_workspace_bytes(B: int, C: int, d: int, k: int, nnz: int) -> int:
    return int(load().ghf_score_topk_sub_workspace_bytes(B, C, d, k, nnz))


def score_topk_workspace_bytes(B: int, N: int, d: int, k: int) -> int:
    return int(load().ghf_score_topk_workspace_bytes(B, N, d, k))


def score_rank(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, iq: Optional[torch.Tensor] = None,
               filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               ic: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
    """(greater, equal) int64 [B]: how many rows of c score above / the same as row target[i] against query q[iq[i]], the
    target and the query's filter list (CSR, each list sorted ascending) left out.  Nothing of size B x N is stored.  With
    `workspace` (uint8, score_rank_workspace_bytes) and `out` given the call allocates nothing (graph capture).  `ic` (int64
    [C], strictly ascending node ids): only those rows of c are counted (ghf_score_rank_sub; the workspace is then
    score_rank_sub_workspace_bytes'); target and lists stay node ids, the target need not be a candidate.  `bias` (fp32 [N], one
    entry per row of c): every score, the target's too, is s + bias[row] (ghf_score_rank_b; workspace:
    score_rank_b_workspace_bytes with C = 0 for every node)."""
    q, c, iq, filt_ptr, filt_idx, B, nnz = _rank_args(q, c, iq, filt_ptr, filt_idx, "score_rank")
    target = _req(target, torch.int64, "target")
    if target.dim() != 1 or target.numel() != B or target.device != q.device:
        raise ValueError(f"score_rank: target must be [B = {B}] on {q.device}, got {tuple(target.shape)} on {target.device}")
    N, d = c.size(0), c.size(1)
    ic = _ic_arg(ic, c, "score_rank")
    bias = _bias_arg(bias, c, "score_rank")
    C = 0 if ic is None else ic.numel()
    if bias is not None:
        ws = _workspace(workspace, score_rank_b_workspace_bytes, q.device, "score_rank", B=B, N=N, C=C, d=d, nnz=nnz)
    elif ic is None:
        ws = _workspace(workspace, score_rank_workspace_bytes, q.device, "score_rank", B=B, N=N, d=d)
    else:
        ws = _workspace(workspace, score_rank_sub_workspace_bytes, q.device, "score_rank", B=B, C=ic.numel(), d=d, nnz=nnz)
    if out is None:
        greater = torch.empty(B, dtype=torch.int64, device=q.device)
        equal = torch.empty(B, dtype=torch.int64, device=q.device)
    else:
        greater, equal = (_req(t, torch.int64, "out") for t in out)
        if greater.numel() != B or equal.numel() != B or not (out[0].is_contiguous() and out[1].is_contiguous()):
            raise ValueError(f"score_rank: out must be two contiguous int64 [{B}] tensors")
    if bias is not None:
        _check(load().ghf_score_rank_b(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B, d,
                                       _ptr(ic), C, _ptr(bias), _ptr(ws), ws.numel(), _ptr(greater), _ptr(equal), _stream()),
               "ghf_score_rank_b")
        return greater, equal
    if ic is not None:
        _check(load().ghf_score_rank_sub(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B,
                                         d, _ptr(ic), ic.numel(), _ptr(ws), ws.numel(), _ptr(greater), _ptr(equal), _stream()),
               "ghf_score_rank_sub")
        return greater, equal
    _check(load().ghf_score_rank(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B, d,
                                 _ptr(ws), ws.numel(), _ptr(greater), _ptr(equal), _stream()), "ghf_score_rank")
    return greater, equal


def score_topk(q: torch.Tensor, c: torch.Tensor, k: int, iq: Optional[torch.Tensor] = None,
               filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               ic: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
    """(scores [B, k] fp32 descending, ids [B, k] int64): the k best rows of c for every query, ties towards the lower id,
    (-inf, -1) where fewer than k candidates remain outside the query's filter list.  `ic` (int64 [C], strictly ascending node
    ids): the k best among those rows only (ghf_score_topk_sub); the ids returned are node ids.  `bias` (fp32 [N]): the scores
    compared and returned are s + bias[row] (ghf_score_topk_b); -inf there means "never this row"."""
    q, c, iq, filt_ptr, filt_idx, B, nnz = _rank_args(q, c, iq, filt_ptr, filt_idx, "score_topk")
    k = int(k)
    if not 1 <= k <= 128:
        raise ValueError(f"score_topk: k = {k} outside 1..128")
    N, d = c.size(0), c.size(1)
    ic = _ic_arg(ic, c, "score_topk")
    bias = _bias_arg(bias, c, "score_topk")
    C = 0 if ic is None else ic.numel()
    if bias is not None:
        ws = _workspace(workspace, score_topk_b_workspace_bytes, q.device, "score_topk", B=B, N=N, C=C, d=d, k=k, nnz=nnz)
    elif ic is None:
        ws = _workspace(workspace, score_topk_workspace_bytes, q.device, "score_topk", B=B, N=N, d=d, k=k)
    else:
        ws = _workspace(workspace, score_topk_sub_workspace_bytes, q.device, "score_topk", B=B, C=ic.numel(), d=d, k=k, nnz=nnz)
    if out is None:
        scores = torch.empty(B, k, dtype=torch.float32, device=q.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=q.device)
    else:
        scores, ids = _req(out[0], torch.float32, "out[0]"), _req(out[1], torch.int64, "out[1]")
        if tuple(scores.shape) != (B, k) or tuple(ids.shape) != (B, k) or not (out[0].is_contiguous() and out[1].is_contiguous()):
            raise ValueError(f"score_topk: out must be contiguous fp32 and int64 [{B}, {k}] tensors")
    if bias is not None:
        _check(load().ghf_score_topk_b(_ptr(q), _ptr(c), _ptr(iq), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B, d, k, _ptr(ic),
                                       C, _ptr(bias), _ptr(ws), ws.numel(), _ptr(scores), _ptr(ids), _stream()), "ghf_score_topk_b")
        return scores, ids
    if ic is not None:
        _check(load().ghf_score_topk_sub(_ptr(q), _ptr(c), _ptr(iq), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B, d, k,
                                         _ptr(ic), ic.numel(), _ptr(ws), ws.numel(), _ptr(scores), _ptr(ids), _stream()),
               "ghf_score_topk_sub")
        return scores, ids
    _check(load().ghf_score_topk(_ptr(q), _ptr(c), _ptr(iq), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B, d, k, _ptr(ws),
                                 ws.numel(), _ptr(scores), _ptr(ids), _stream()), "ghf_score_topk")
    return scores, ids


# ---- 1-vs-all softmax loss against every node (include/ghf.h: ghf_score_softmax_fwd / _bwd, csrc/softmax.hip) ----------
def score_softmax_workspace_bytes(B: int, N: int, d: int) -> int:
    return int(load().ghf_score_softmax_workspace_bytes(B, N, d))


def score_softmax_bwd_workspace_bytes(B: int, N: int, d: int) -> int:
    return int(load().ghf_score_softmax_bwd_workspace_bytes(B, N, d))


def score_softmax_sub_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_softmax_sub_workspace_bytes(B, C, d, nnz))


def score_softmax_bwd_sub_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_softmax_bwd_sub_workspace_bytes(B, C, d, nnz))


def _softmax_args(q, c, target, iq, filt_ptr, filt_idx, scale, what: str):
    q, c, iq, filt_ptr, filt_idx, B, nnz = _rank_args(q, c, iq, filt_ptr, filt_idx, what)
    target = _req(target, torch.int64, "target")
    if target.dim() != 1 or target.numel() != B or target.device != q.device:
        raise ValueError(f"{what}: target must be [B = {B}] on {q.device}, got {tuple(target.shape)} on {target.device}")
    return q, c, target, iq, filt_ptr, filt_idx, B, nnz, _scale_arg(scale, what)


def _f32_out(t: Optional[torch.Tensor], shape: Tuple[int, ...], device, what: str) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    r = _req(t, torch.float32, "out")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: out must be contiguous fp32 tensors of shape {tuple(shape)}")
    return r


def _f32_out_pair(out: Optional[Tuple[torch.Tensor, torch.Tensor]], shape0, shape1, device, what: str):
    first, second = (None, None) if out is None else out
    return _f32_out(first, shape0, device, what), _f32_out(second, shape1, device, what)


def _scale_arg(scale, what: str) -> float:
    scale = float(scale)
    if not (0.0 < scale < float("inf")):
        raise ValueError(f"{what}: scale must be finite and positive, got {scale}")
    return scale


def score_softmax_fwd(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, iq: Optional[torch.Tensor] = None,
                      filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0,
                      workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                      ic: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
    """(loss, lse) fp32 [B]: lse[i] = log sum_j exp(scale q[iq[i]] . c[j]) over every row j of c outside query i's filter
    list (CSR, each list sorted ascending; the target always stays in), loss[i] = lse[i] - scale q[iq[i]] . c[target[i]].
    Nothing of size B x N is stored.  With `workspace` (uint8, score_softmax_workspace_bytes) and `out` given the call
    allocates nothing.  `ic` (int64 [C], strictly ascending node ids): the sum runs over those rows of c only
    (ghf_score_softmax_fwd_sub; workspace: score_softmax_sub_workspace_bytes); a query whose target is not among them gets
    NaN.  `bias` (fp32 [N]): every logit is fmaf(scale, q . c[j], bias[j]), the bias not scaled (ghf_score_softmax_fwd_b;
    workspace: score_softmax_b_workspace_bytes with C = 0 for every node)."""
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale = _softmax_args(q, c, target, iq, filt_ptr, filt_idx, scale, "score_softmax_fwd")
    N, d = c.size(0), c.size(1)
    ic = _ic_arg(ic, c, "score_softmax_fwd")
    loss, lse = _f32_out_pair(out, (B,), (B,), q.device, "score_softmax_fwd")
    bias = _bias_arg(bias, c, "score_softmax_fwd")
    if bias is not None:
        C = 0 if ic is None else ic.numel()
        ws = _workspace(workspace, score_softmax_b_workspace_bytes, q.device, "score_softmax_fwd", B=B, N=N, C=C, d=d, nnz=nnz)
        _check(load().ghf_score_softmax_fwd_b(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0),
                                              N, B, d, scale, _ptr(ic), C, _ptr(bias), _ptr(ws), ws.numel(), _ptr(loss), _ptr(lse),
                                              _stream()), "ghf_score_softmax_fwd_b")
        return loss, lse
    if ic is not None:
        ws = _workspace(workspace, score_softmax_sub_workspace_bytes, q.device, "score_softmax_fwd", B=B, C=ic.numel(), d=d, nnz=nnz)
        _check(load().ghf_score_softmax_fwd_sub(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0),
                                                N, B, d, scale, _ptr(ic), ic.numel(), _ptr(ws), ws.numel(), _ptr(loss), _ptr(lse),
                                                _stream()), "ghf_score_softmax_fwd_sub")
        return loss, lse
    ws = _workspace(workspace, score_softmax_workspace_bytes, q.device, "score_softmax_fwd", B=B, N=N, d=d)
    _check(load().ghf_score_softmax_fwd(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B,
                                        d, scale, _ptr(ws), ws.numel(), _ptr(loss), _ptr(lse), _stream()), "ghf_score_softmax_fwd")
    return loss, lse


def score_softmax_bwd(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, lse: torch.Tensor, grad_loss: torch.Tensor,
                      iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                      filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, workspace: Optional[torch.Tensor] = None,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ic: Optional[torch.Tensor] = None,
                      bias: Optional[torch.Tensor] = None, want_db: bool = True):
    """(dq [B, d], dc [N, d]) fp32 of include/ghf.h: ghf_score_softmax_bwd — dq per query (not scattered through iq), every
    row of dc written.  `lse` is the forward's.  With `ic` (the forward's): ghf_score_softmax_bwd_sub, dc is [C, d], row j the
    gradient of row ic[j] of c.  With `bias` (the forward's): ghf_score_softmax_bwd_b, and the result is (dq, dc, db), db fp32
    [N] ([C] with ic, entry j belonging to node ic[j]) the bias's gradient, None when `want_db` is False."""
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale = _softmax_args(q, c, target, iq, filt_ptr, filt_idx, scale, "score_softmax_bwd")
    lse, grad_loss = _req(lse, torch.float32, "lse"), _req(grad_loss, torch.float32, "grad_loss")
    if lse.numel() != B or grad_loss.numel() != B:
        raise ValueError(f"score_softmax_bwd: lse and grad_loss must hold B = {B} values")
    N, d = c.size(0), c.size(1)
    ic = _ic_arg(ic, c, "score_softmax_bwd")
    bias = _bias_arg(bias, c, "score_softmax_bwd")
    if bias is not None:
        C = 0 if ic is None else ic.numel()
        M = C if C else N
        ws = _workspace(workspace, score_softmax_bwd_b_workspace_bytes, q.device, "score_softmax_bwd", B=B, N=N, C=C, d=d, nnz=nnz)
        dq, dc = _f32_out_pair(out, (B, d), (M, d), q.device, "score_softmax_bwd")
        db = torch.empty(M, dtype=torch.float32, device=q.device) if want_db else None
        _check(load().ghf_score_softmax_bwd_b(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0),
                                              N, B, d, scale, _ptr(lse), _ptr(grad_loss), _ptr(ic), C, _ptr(bias), _ptr(ws),
                                              ws.numel(), _ptr(dq), _ptr(dc), _ptr(db), _stream()), "ghf_score_softmax_bwd_b")
        return dq, dc, db
    if ic is not None:
        C = ic.numel()
        ws = _workspace(workspace, score_softmax_bwd_sub_workspace_bytes, q.device, "score_softmax_bwd", B=B, C=C, d=d, nnz=nnz)
        dq, dc = _f32_out_pair(out, (B, d), (C, d), q.device, "score_softmax_bwd")
        _check(load().ghf_score_softmax_bwd_sub(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0),
                                                N, B, d, scale, _ptr(lse), _ptr(grad_loss), _ptr(ic), C, _ptr(ws), ws.numel(), _ptr(dq),
                                                _ptr(dc), _stream()), "ghf_score_softmax_bwd_sub")
        return dq, dc
    ws = _workspace(workspace, score_softmax_bwd_workspace_bytes, q.device, "score_softmax_bwd", B=B, N=N, d=d)
    dq, dc = _f32_out_pair(out, (B, d), (N, d), q.device, "score_softmax_bwd")
    _check(load().ghf_score_softmax_bwd(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B,
                                        d, scale, _ptr(lse), _ptr(grad_loss), _ptr(ws), ws.numel(), _ptr(dq), _ptr(dc), _stream()),
           "ghf_score_softmax_bwd")
    return dq, dc


# ---- multi-label 1-vs-all BCE loss against every node (include/ghf.h: ghf_score_bce_fwd / _bwd, csrc/bce.hip) ---------
def score_bce_workspace_bytes(B: int, N: int, d: int) -> int:
    return int(load().ghf_score_bce_workspace_bytes(B, N, d))


def score_bce_bwd_workspace_bytes(B: int, N: int, d: int) -> int:
    return int(load().ghf_score_bce_bwd_workspace_bytes(B, N, d))


def score_bce_sub_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_bce_sub_workspace_bytes(B, C, d, nnz))


def score_bce_bwd_sub_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_bce_bwd_sub_workspace_bytes(B, C, d, nnz))


def _bce_args(q, c, iq, pos_ptr, pos_idx, scale, smoothing, what: str):
    q, c, iq, pos_ptr, pos_idx, B, nnz = _rank_args(q, c, iq, pos_ptr, pos_idx, what)
    scale, smoothing = _scale_arg(scale, what), float(smoothing)
    if not (0.0 <= smoothing < 1.0):
        raise ValueError(f"{what}: smoothing must be in [0, 1), got {smoothing}")
    return q, c, iq, pos_ptr, pos_idx, B, nnz, scale, smoothing


def score_bce_fwd(q: torch.Tensor, c: torch.Tensor, iq: Optional[torch.Tensor] = None, pos_ptr: Optional[torch.Tensor] = None,
                  pos_idx: Optional[torch.Tensor] = None, scale: float = 1.0, smoothing: float = 0.0,
                  workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                  ic: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """loss fp32 [B]: binary_cross_entropy_with_logits(scale q[iq[i]] . c[j], y_ij, reduction="sum") over every row j of c, with
    y_ij = (1 - smoothing) [j in query i's list] + smoothing / N (CSR lists, each sorted ascending, a repeated id counting once).
    Nothing of size B x N is stored.  With `workspace` (uint8, score_bce_workspace_bytes) and `out` given the call allocates
    nothing.  `ic` (int64 [C], strictly ascending node ids): the loss over those rows of c alone, smoothing / C, listed ids
    that are no candidates taking no part (ghf_score_bce_fwd_sub; workspace: score_bce_sub_workspace_bytes).  `bias` (fp32 [N],
    finite): every logit is fmaf(scale, q . c[j], bias[j]) (ghf_score_bce_fwd_b; workspace: score_bce_b_workspace_bytes)."""
    q, c, iq, pos_ptr, pos_idx, B, nnz, scale, smoothing = _bce_args(q, c, iq, pos_ptr, pos_idx, scale, smoothing, "score_bce_fwd")
    N, d = c.size(0), c.size(1)
    ic = _ic_arg(ic, c, "score_bce_fwd")
    loss = _f32_out(out, (B,), q.device, "score_bce_fwd")
    bias = _bias_arg(bias, c, "score_bce_fwd")
    if bias is not None:
        C = 0 if ic is None else ic.numel()
        ws = _workspace(workspace, score_bce_b_workspace_bytes, q.device, "score_bce_fwd", B=B, N=N, C=C, d=d, nnz=nnz)
        _check(load().ghf_score_bce_fwd_b(_ptr(q), _ptr(c), _ptr(iq), _ptr(pos_ptr), _ptr(pos_idx), nnz, q.size(0), N, B, d, scale,
                                          smoothing, _ptr(ic), C, _ptr(bias), _ptr(ws), ws.numel(), _ptr(loss), _stream()),
               "ghf_score_bce_fwd_b")
        return loss
    if ic is not None:
        ws = _workspace(workspace, score_bce_sub_workspace_bytes, q.device, "score_bce_fwd", B=B, C=ic.numel(), d=d, nnz=nnz)
        _check(load().ghf_score_bce_fwd_sub(_ptr(q), _ptr(c), _ptr(iq), _ptr(pos_ptr), _ptr(pos_idx), nnz, q.size(0), N, B, d, scale,
                                            smoothing, _ptr(ic), ic.numel(), _ptr(ws), ws.numel(), _ptr(loss), _stream()),
               "ghf_score_bce_fwd_sub")
        return loss
    ws = _workspace(workspace, score_bce_workspace_bytes, q.device, "score_bce_fwd", B=B, N=N, d=d)
    _check(load().ghf_score_bce_fwd(_ptr(q), _ptr(c), _ptr(iq), _ptr(pos_ptr), _ptr(pos_idx), nnz, q.size(0), N, B, d, scale,
                                    smoothing, _ptr(ws), ws.numel(), _ptr(loss), _stream()), "ghf_score_bce_fwd")
    return loss


def score_bce_bwd(q: torch.Tensor, c: torch.Tensor, loss: torch.Tensor, grad_loss: torch.Tensor, iq: Optional[torch.Tensor] = None,
                  pos_ptr: Optional[torch.Tensor] = None, pos_idx: Optional[torch.Tensor] = None, scale: float = 1.0,
                  smoothing: float = 0.0, workspace: Optional[torch.Tensor] = None,
                  out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ic: Optional[torch.Tensor] = None,
                  bias: Optional[torch.Tensor] = None, want_db: bool = True):
    """(dq [B, d], dc [N, d]) fp32 of include/ghf.h: ghf_score_bce_bwd — dq per query (not scattered through iq), every row
    of dc written.  `loss` is the forward's (a NaN entry: that query takes no part).  With `ic` (the forward's):
    ghf_score_bce_bwd_sub, dc is [C, d], row j the gradient of row ic[j] of c.  With `bias` (the forward's): ghf_score_bce_bwd_b,
    and the result is (dq, dc, db) as score_softmax_bwd's."""
    q, c, iq, pos_ptr, pos_idx, B, nnz, scale, smoothing = _bce_args(q, c, iq, pos_ptr, pos_idx, scale, smoothing, "score_bce_bwd")
    loss, grad_loss = _req(loss, torch.float32, "loss"), _req(grad_loss, torch.float32, "grad_loss")
    if loss.numel() != B or grad_loss.numel() != B:
        raise ValueError(f"score_bce_bwd: loss and grad_loss must hold B = {B} values")
    N, d = c.size(0), c.size(1)
    ic = _ic_arg(ic, c, "score_bce_bwd")
    bias = _bias_arg(bias, c, "score_bce_bwd")
    if bias is not None:
        C = 0 if ic is None else ic.numel()
        M = C if C else N
        ws = _workspace(workspace, score_bce_bwd_b_workspace_bytes, q.device, "score_bce_bwd", B=B, N=N, C=C, d=d, nnz=nnz)
        dq, dc = _f32_out_pair(out, (B, d), (M, d), q.device, "score_bce_bwd")
        db = torch.empty(M, dtype=torch.float32, device=q.device) if want_db else None
        _check(load().ghf_score_bce_bwd_b(_ptr(q), _ptr(c), _ptr(iq), _ptr(pos_ptr), _ptr(pos_idx), nnz, q.size(0), N, B, d, scale,
                                          smoothing, _ptr(loss), _ptr(grad_loss), _ptr(ic), C, _ptr(bias), _ptr(ws), ws.numel(),
                                          _ptr(dq), _ptr(dc), _ptr(db), _stream()), "ghf_score_bce_bwd_b")
        return dq, dc, db
    if ic is not None:
        C = ic.numel()
        ws = _workspace(workspace, score_bce_bwd_sub_workspace_bytes, q.device, "score_bce_bwd", B=B, C=C, d=d, nnz=nnz)
        dq, dc = _f32_out_pair(out, (B, d), (C, d), q.device, "score_bce_bwd")
        _check(load().ghf_score_bce_bwd_sub(_ptr(q), _ptr(c), _ptr(iq), _ptr(pos_ptr), _ptr(pos_idx), nnz, q.size(0), N, B, d, scale,
                                            smoothing, _ptr(loss), _ptr(grad_loss), _ptr(ic), C, _ptr(ws), ws.numel(), _ptr(dq),
                                            _ptr(dc), _stream()), "ghf_score_bce_bwd_sub")
        return dq, dc
    ws = _workspace(workspace, score_bce_bwd_workspace_bytes, q.device, "score_bce_bwd", B=B, N=N, d=d)
    dq, dc = _f32_out_pair(out, (B, d), (N, d), q.device, "score_bce_bwd")
    _check(load().ghf_score_bce_bwd(_ptr(q), _ptr(c), _ptr(iq), _ptr(pos_ptr), _ptr(pos_idx), nnz, q.size(0), N, B, d, scale,
                                    smoothing, _ptr(loss), _ptr(grad_loss), _ptr(ws), ws.numel(), _ptr(dq), _ptr(dc), _stream()),
           "ghf_score_bce_bwd")
    return dq, dc


# ---- negative-sampling loss with self-adversarial weighting (include/ghf.h: ghf_score_negsamp_fwd / _bwd, csrc/negsamp.hip) ----
def score_negsamp_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_negsamp_workspace_bytes(B, N, C, d, nnz))


def score_negsamp_bwd_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_negsamp_bwd_workspace_bytes(B, N, C, d, nnz))


def _negsamp_args(q, c, target, iq, filt_ptr, filt_idx, scale, margin, adversarial_temperature, what: str):
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale = _softmax_args(q, c, target, iq, filt_ptr, filt_idx, scale, what)
    margin, alpha = float(margin), float(adversarial_temperature)
    if not (float("-inf") < margin < float("inf")):
        raise ValueError(f"{what}: margin must be finite, got {margin}")
    if not (0.0 <= alpha < float("inf")):
        raise ValueError(f"{what}: adversarial_temperature must be finite and not negative, got {alpha}")
    return q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, alpha


def score_negsamp_fwd(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, iq: Optional[torch.Tensor] = None,
                      filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0,
                      margin: float = 0.0, adversarial_temperature: float = 0.0, workspace: Optional[torch.Tensor] = None,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ic: Optional[torch.Tensor] = None,
                      bias: Optional[torch.Tensor] = None):
    """(loss, lw) fp32 [B] of include/ghf.h: ghf_score_negsamp_fwd.  With z_ij = scale q[iq[i]] . c[j] (+ bias[j]) and J_i the
    rows of c (of c[ic] with `ic`) outside query i's filter list other than target[i]: lw[i] = log sum_{J_i} exp(alpha z_ij)
    (-inf: no negatives), loss[i] = softplus(-(z_it + margin)) + sum_{J_i} exp(alpha z_ij - lw[i]) softplus(z_ij + margin), alpha
    the adversarial temperature.  Nothing of size B x N is stored.  With `workspace` (uint8, score_negsamp_workspace_bytes, C = 0
    for every node) and `out` given the call allocates nothing.  With `ic` a query whose target is not among the candidates
    gets NaN."""
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, alpha = _negsamp_args(
        q, c, target, iq, filt_ptr, filt_idx, scale, margin, adversarial_temperature, "score_negsamp_fwd")
    N, d = c.size(0), c.size(1)
    ic = _ic_arg(ic, c, "score_negsamp_fwd")
    loss, lw = _f32_out_pair(out, (B,), (B,), q.device, "score_negsamp_fwd")
    bias = _bias_arg(bias, c, "score_negsamp_fwd")
    C = 0 if ic is None else ic.numel()
    ws = _workspace(workspace, score_negsamp_workspace_bytes, q.device, "score_negsamp_fwd", B=B, N=N, C=C, d=d, nnz=nnz)
    _check(load().ghf_score_negsamp_fwd(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B,
                                        d, scale, margin, alpha, _ptr(ic), C, _ptr(bias), _ptr(ws), ws.numel(), _ptr(loss), _ptr(lw),
                                        _stream()), "ghf_score_negsamp_fwd")
    return loss, lw


def score_negsamp_bwd(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, lw: torch.Tensor, grad_loss: torch.Tensor,
                      iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                      filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 0.0,
                      adversarial_temperature: float = 0.0, workspace: Optional[torch.Tensor] = None,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ic: Optional[torch.Tensor] = None,
                      bias: Optional[torch.Tensor] = None, want_db: bool = True):
    """(dq [B, d], dc [N, d]) fp32 of include/ghf.h: ghf_score_negsamp_bwd, the weights constants — dq per query (not scattered
    through iq), every row of dc written.  `lw` is the forward's.  With `ic` (the forward's) dc is [C, d], row j the gradient
    of row ic[j] of c.  With `bias` (the forward's) the result is (dq, dc, db) as score_softmax_bwd's."""
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, alpha = _negsamp_args(
        q, c, target, iq, filt_ptr, filt_idx, scale, margin, adversarial_temperature, "score_negsamp_bwd")
    lw, grad_loss = _req(lw, torch.float32, "lw"), _req(grad_loss, torch.float32, "grad_loss")
    if lw.numel() != B or grad_loss.numel() != B:
        raise ValueError(f"score_negsamp_bwd: lw and grad_loss must hold B = {B} values")
    N, d = c.size(0), c.size(1)
    ic = _ic_arg(ic, c, "score_negsamp_bwd")
    bias = _bias_arg(bias, c, "score_negsamp_bwd")
    C = 0 if ic is None else ic.numel()
    M = C if C else N
    ws = _workspace(workspace, score_negsamp_bwd_workspace_bytes, q.device, "score_negsamp_bwd", B=B, N=N, C=C, d=d, nnz=nnz)
    dq, dc = _f32_out_pair(out, (B, d), (M, d), q.device, "score_negsamp_bwd")
    db = torch.empty(M, dtype=torch.float32, device=q.device) if bias is not None and want_db else None
    _check(load().ghf_score_negsamp_bwd(_ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B,
                                        d, scale, margin, alpha, _ptr(lw), _ptr(grad_loss), _ptr(ic), C, _ptr(bias), _ptr(ws),
                                        ws.numel(), _ptr(dq), _ptr(dc), _ptr(db), _stream()), "ghf_score_negsamp_bwd")
    return (dq, dc) if bias is None else (dq, dc, db)


# ---- per-query negative sets (include/ghf_negatives.h, csrc/negatives.hip) ------------------------------------------------
def neg_workspace_bytes(B: int, K: int, d: int, nnz: int) -> int:
    return int(load().ghf_neg_workspace_bytes(B, K, d, nnz))


def _neg_arg(neg: torch.Tensor, B: int, c: torch.Tensor, what: str) -> torch.Tensor:
    """The negatives of the ghf_neg_* calls: int64 [B, K], K >= 1, on c's device.  What the entries are (-1, a node id, or
    neither: that query is invalid) is the device's check."""
    neg = _req(neg, torch.int64, "neg")
    if neg.dim() != 2 or neg.size(0) != B or neg.size(1) < 1:
        raise ValueError(f"{what}: neg must be [B = {B}, K >= 1], got {tuple(neg.shape)}")
    if neg.device != c.device:
        raise RuntimeError(f"{what}: neg is on {neg.device}, the embeddings on {c.device}")
    return neg


def _per_query(symbol: str, what: str, lead, q, c, target, neg, iq, filt_ptr, filt_idx, workspace, ws_fn, out, out_specs,
               out_err: Optional[str] = None, scale=None, margin=None, alpha=None, normalize=None, bias=None, bias_slot: bool = True,
               saved=None):
    """One call of the per-query family (ghf_neg_*, ghf_dist_*, ghf_pair_*): the argument normalisation, the
    workspace, the outputs and _check, for every member.  `lead`: None or d -> the call's leading selectors (it raises what a bad
    one deserves); `scale` None: the call has none (rank); `margin`, `alpha`, `normalize`: the scalars the call takes, in the
    ABI's order; `bias_slot`: whether the ABI has a bias argument; `saved`: None or (tensor, dtype, name, grad_loss) of a
    backward; `out_specs`: (dtype, shape) per output, the shape "B", "Bd" or "BK" ([B], [B, d], [B, K + 1]); `out_err`: the message for a bad
    non-float output."""
    q, c, iq, filt_ptr, filt_idx, B, nnz = _rank_args(q, c, iq, filt_ptr, filt_idx, what)
    target = _req(target, torch.int64, "target")
    if target.dim() != 1 or target.numel() != B or target.device != q.device:
        raise ValueError(f"{what}: target must be [B = {B}] on {q.device}, got {tuple(target.shape)} on {target.device}")
    scalars = [] if scale is None else [_scale_arg(scale, what)]
    if margin is not None:
        margin = float(margin)
        if not (float("-inf") < margin < float("inf")):
            raise ValueError(f"{what}: margin must be finite, got {margin}")
        scalars.append(margin)
    if alpha is not None:
        alpha = float(alpha)
        if not (0.0 <= alpha < float("inf")):
            raise ValueError(f"{what}: adversarial_temperature must be finite and not negative, got {alpha}")
        scalars.append(alpha)
    if normalize is not None:
        if not isinstance(normalize, (bool, int)) or normalize not in (0, 1):
            raise ValueError(f"{what}: normalize must be a bool, got {normalize!r}")
        scalars.append(int(normalize))
    neg = _neg_arg(neg, B, c, what)
    N, d, K = c.size(0), c.size(1), neg.size(1)
    lead = () if lead is None else lead(d)
    tail = [_ptr(_bias_arg(bias, c, what))] if bias_slot else []
    if saved is not None:
        t, dtype, name, grad_loss = saved
        t, grad_loss = _req(t, dtype, name), _req(grad_loss, torch.float32, "grad_loss")
        if t.numel() != B or grad_loss.numel() != B:
            raise ValueError(f"{what}: {name} and grad_loss must hold B = {B} values")
        tail += [_ptr(t), _ptr(grad_loss)]
    ws = _workspace(workspace, ws_fn, q.device, what, B=B, K=K, d=d, nnz=nnz)
    dev, outs = q.device, []
    for k, (dtype, code) in enumerate(out_specs):
        given = None if out is None else out[k]
        shape = (B,) if code == "B" else (B, d) if code == "Bd" else (B, K + 1)
        if given is None:
            outs.append(torch.empty(shape, dtype=dtype, device=dev))
        elif dtype == torch.float32:
            outs.append(_f32_out(given, shape, dev, what))
        else:
            t = _req(given, dtype, "out")
            if t.numel() != B or not given.is_contiguous():           # every non-float output is a [B] vector
                raise ValueError(f"{what}: {out_err.format(B=B)}")
            outs.append(t)
    args = [*lead, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B, d, *scalars,
            _ptr(neg), K, *tail, _ptr(ws), ws.numel()]
    for t in outs:
        args.append(_ptr(t))
    _check(getattr(load(), symbol)(*args, _stream()), symbol)
    return tuple(outs)


_PQ_LOSS = ((torch.float32, "B"), (torch.float32, "B"))
_PQ_COUNTS = ((torch.int64, "B"), (torch.int64, "B"))
_PQ_GRADS = ((torch.float32, "Bd"), (torch.float32, "BK"))
_PQ_COUNTS_ERR = "out must be two contiguous int64 [{B}] tensors"


def score_neg_rank(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor, iq: Optional[torch.Tensor] = None,
                   filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                   bias: Optional[torch.Tensor] = None):
    """(greater, equal) int64 [B] of include/ghf_negatives.h: ghf_neg_rank — how many of query i's OWN negatives neg[i, :]
    (node ids, -1 = no entry, repeats count) score above / the same as row target[i], positions that hold the target or a
    listed id left out.  `bias` (fp32 [N]): every score is s + bias[row].  With `workspace` (uint8, neg_workspace_bytes) and
    `out` given the call allocates nothing."""
    return _per_query("ghf_neg_rank", "score_neg_rank", None, q, c, target, neg, iq, filt_ptr, filt_idx, workspace, neg_workspace_bytes,
                      out, _PQ_COUNTS, _PQ_COUNTS_ERR, bias=bias)


def score_neg_softmax_fwd(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
                          iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                          filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, workspace: Optional[torch.Tensor] = None,
                          out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, bias: Optional[torch.Tensor] = None):
    """(loss, lse) fp32 [B] of include/ghf_negatives.h: ghf_neg_softmax_fwd — lse[i] = log(exp(z_it) + sum over query i's own
    negatives neg[i, :] outside its list other than the target of exp(z_ij)), z = scale q . c[row] (+ bias[row]), loss = lse -
    z_it; exactly 0 for a query without negatives."""
    return _per_query("ghf_neg_softmax_fwd", "score_neg_softmax_fwd", None, q, c, target, neg, iq, filt_ptr, filt_idx, workspace,
                      neg_workspace_bytes, out, _PQ_LOSS, scale=scale, bias=bias)


def score_neg_negsamp_fwd(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
                          iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                          filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 0.0,
                          adversarial_temperature: float = 0.0, workspace: Optional[torch.Tensor] = None,
                          out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, bias: Optional[torch.Tensor] = None):
    """(loss, lw) fp32 [B] of include/ghf_negatives.h: ghf_neg_negsamp_fwd — score_negsamp_fwd's formulas with J_i the positions
    of query i's own negatives neg[i, :] outside its list other than the target; lw = -inf and the positive term alone where
    there are none."""
    return _per_query("ghf_neg_negsamp_fwd", "score_neg_negsamp_fwd", None, q, c, target, neg, iq, filt_ptr, filt_idx, workspace,
                      neg_workspace_bytes, out, _PQ_LOSS, scale=scale, margin=margin, alpha=adversarial_temperature, bias=bias)


def score_neg_bwd(mode: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor, saved: torch.Tensor,
                  grad_loss: torch.Tensor, iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                  filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 0.0,
                  adversarial_temperature: float = 0.0, workspace: Optional[torch.Tensor] = None,
                  out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, bias: Optional[torch.Tensor] = None):
    """(dq [B, d], coef [B, K + 1]) fp32 of include/ghf_negatives.h: ghf_neg_bwd, `mode` NEG_SOFTMAX or NEG_NEGSAMP and `saved`
    that forward's lse / lw.  coef[i, j] is the gradient of the loss sum with respect to the score of position j of query i (0
    where the position takes no part), coef[i, K] the target's; dq[i] = sum_j coef[i, j] c[neg[i, j]] + coef[i, K] c[target[i]],
    per query (not scattered through iq).  The gradient of c is a grouped sum over coef (autograd.PerQueryLossFn)."""
    if mode not in (NEG_SOFTMAX, NEG_NEGSAMP):
        raise ValueError(f"score_neg_bwd: mode must be NEG_SOFTMAX or NEG_NEGSAMP, got {mode}")
    return _per_query("ghf_neg_bwd", "score_neg_bwd", lambda d: (mode,), q, c, target, neg, iq, filt_ptr, filt_idx, workspace,
                      neg_workspace_bytes, out, _PQ_GRADS, scale=scale, margin=margin, alpha=adversarial_temperature, bias=bias,
                      saved=(saved, torch.float32, "saved", grad_loss))


# ---- distance scores for per-query negative sets (include/ghf_distance.h, csrc/distance.hip) ----------------------------
def dist_workspace_bytes(B: int, K: int, d: int, nnz: int) -> int:
    return int(load().ghf_dist_workspace_bytes(B, K, d, nnz))


def _metric_arg(metric: int, d: int, what: str) -> int:
    if metric not in (DIST_L1, DIST_L2, DIST_COMPLEX):
        raise ValueError(f"{what}: metric must be DIST_L1, DIST_L2 or DIST_COMPLEX, got {metric}")
    if metric == DIST_COMPLEX and d % 2:
        raise ValueError(f"{what}: DIST_COMPLEX reads the rows as interleaved re / im pairs and needs an even d, got {d}")
    return int(metric)


def score_dist_rank(metric: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
                    iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                    filt_idx: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                    out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """(greater, equal) int64 [B] of include/ghf_distance.h: ghf_dist_rank — score_neg_rank with the score -D(q_i, c[row]),
    `metric` DIST_L1, DIST_L2 or DIST_COMPLEX: how many of query i's own negatives lie closer to q_i than / exactly as far as
    row target[i]."""
    return _per_query("ghf_dist_rank", "score_dist_rank", lambda d: (_metric_arg(metric, d, "score_dist_rank"),), q, c, target, neg,
                      iq, filt_ptr, filt_idx, workspace, dist_workspace_bytes, out, _PQ_COUNTS, _PQ_COUNTS_ERR, bias_slot=False)


# ---- distance scores against every node or a candidate subset (include/ghf_distance_sweep.h, csrc/distance_sweep.hip) ---
def dist_sweep_rank_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_dist_sweep_rank_workspace_bytes(B, C, d, nnz))


def dist_sweep_topk_workspace_bytes(B: int, C: int, d: int, k: int, nnz: int) -> int:
    return int(load().ghf_dist_sweep_topk_workspace_bytes(B, C, d, k, nnz))


def score_dist_sweep_rank(metric: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, iq: Optional[torch.Tensor] = None,
                          filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                          ic: Optional[torch.Tensor] = None):
    """(greater, equal) int64 [B] of include/ghf_distance_sweep.h: ghf_dist_sweep_rank — score_rank with the score -D(q_i,
    c[row]), `metric` DIST_L1, DIST_L2 or DIST_COMPLEX: how many rows of c (of c[ic] with `ic`, int64 [C] strictly ascending
    node ids) lie closer to query q[iq[i]] than / exactly as far as row target[i], the target and the query's filter list
    left out.  Nothing of size B x N is stored.  With `workspace` (uint8, dist_sweep_rank_workspace_bytes) and `out` given
    the call allocates nothing."""
    q, c, iq, filt_ptr, filt_idx, B, nnz = _rank_args(q, c, iq, filt_ptr, filt_idx, "score_dist_sweep_rank")
    N, d = c.size(0), c.size(1)
    metric = _metric_arg(metric, d, "score_dist_sweep_rank")
    target = _req(target, torch.int64, "target")
    if target.dim() != 1 or target.numel() != B or target.device != q.device:
        raise ValueError(f"score_dist_sweep_rank: target must be [B = {B}] on {q.device}, got {tuple(target.shape)} on {target.device}")
    ic = _ic_arg(ic, c, "score_dist_sweep_rank")
    C = N if ic is None else ic.numel()
    ws = _workspace(workspace, dist_sweep_rank_workspace_bytes, q.device, "score_dist_sweep_rank", B=B, C=C, d=d, nnz=nnz)
    if out is None:
        greater = torch.empty(B, dtype=torch.int64, device=q.device)
        equal = torch.empty(B, dtype=torch.int64, device=q.device)
    else:
        greater, equal = (_req(t, torch.int64, "out") for t in out)
        if greater.numel() != B or equal.numel() != B or not (out[0].is_contiguous() and out[1].is_contiguous()):
            raise ValueError(f"score_dist_sweep_rank: out must be two contiguous int64 [{B}] tensors")
    _check(load().ghf_dist_sweep_rank(metric, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0),
                                      N, B, d, _ptr(ic), C, _ptr(ws), ws.numel(), _ptr(greater), _ptr(equal), _stream()),
           "ghf_dist_sweep_rank")
    return greater, equal


def score_dist_sweep_topk(metric: int, q: torch.Tensor, c: torch.Tensor, k: int, iq: Optional[torch.Tensor] = None,
                          filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                          ic: Optional[torch.Tensor] = None):
    """(scores [B, k] fp32 = -D descending, ids [B, k] int64) of include/ghf_distance_sweep.h: ghf_dist_sweep_topk — score_topk
    with the score -D(q_i, c[row]): the k nearest rows of c (of c[ic] with `ic`; the ids returned are node ids) for every query,
    ties towards the lower id, (-inf, -1) where fewer than k candidates remain outside the query's filter list."""
    q, c, iq, filt_ptr, filt_idx, B, nnz = _rank_args(q, c, iq, filt_ptr, filt_idx, "score_dist_sweep_topk")
    N, d = c.size(0), c.size(1)
    metric = _metric_arg(metric, d, "score_dist_sweep_topk")
    k = int(k)
    if not 1 <= k <= 128:
        raise ValueError(f"score_dist_sweep_topk: k = {k} outside 1..128")
    ic = _ic_arg(ic, c, "score_dist_sweep_topk")
    C = N if ic is None else ic.numel()
    ws = _workspace(workspace, dist_sweep_topk_workspace_bytes, q.device, "score_dist_sweep_topk", B=B, C=C, d=d, k=k, nnz=nnz)
    if out is None:
        scores = torch.empty(B, k, dtype=torch.float32, device=q.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=q.device)
    else:
        scores, ids = _req(out[0], torch.float32, "out[0]"), _req(out[1], torch.int64, "out[1]")
        if tuple(scores.shape) != (B, k) or tuple(ids.shape) != (B, k) or not (out[0].is_contiguous() and out[1].is_contiguous()):
            raise ValueError(f"score_dist_sweep_topk: out must be contiguous fp32 and int64 [{B}, {k}] tensors")
    _check(load().ghf_dist_sweep_topk(metric, _ptr(q), _ptr(c), _ptr(iq), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N, B, d, k,
                                      _ptr(ic), C, _ptr(ws), ws.numel(), _ptr(scores), _ptr(ids), _stream()), "ghf_dist_sweep_topk")
    return scores, ids


# ---- the two losses under a distance against every node or a candidate subset (include/ghf_distance_loss.h) -------------
def dist_loss_fwd_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_dist_loss_fwd_workspace_bytes(B, C, d, nnz))


def dist_loss_bwd_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_dist_loss_bwd_workspace_bytes(B, C, d, nnz))


def score_dist_loss_softmax_fwd(metric: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor,
                                iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                                filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0,
                                workspace: Optional[torch.Tensor] = None,
                                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ic: Optional[torch.Tensor] = None):
    """(loss, lse) fp32 [B] of include/ghf_distance_loss.h: ghf_dist_loss_softmax_fwd — score_softmax_fwd with z = -scale D(q_i,
    c[row]) over every row of c (of c[ic] with `ic`, int64 [C] strictly ascending node ids, which must hold every target).
    Nothing of size B x C is stored; with `workspace` (uint8, dist_loss_fwd_workspace_bytes) and `out` the call allocates
    nothing."""
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale = _softmax_args(q, c, target, iq, filt_ptr, filt_idx, scale,
                                                                        "score_dist_loss_softmax_fwd")
    N, d = c.size(0), c.size(1)
    metric = _metric_arg(metric, d, "score_dist_loss_softmax_fwd")
    ic = _ic_arg(ic, c, "score_dist_loss_softmax_fwd")
    C = N if ic is None else ic.numel()
    loss, lse = _f32_out_pair(out, (B,), (B,), q.device, "score_dist_loss_softmax_fwd")
    ws = _workspace(workspace, dist_loss_fwd_workspace_bytes, q.device, "score_dist_loss_softmax_fwd", B=B, C=C, d=d, nnz=nnz)
    _check(load().ghf_dist_loss_softmax_fwd(metric, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz,
                                            q.size(0), N, B, d, scale, _ptr(ic), C, _ptr(ws), ws.numel(), _ptr(loss), _ptr(lse),
                                            _stream()), "ghf_dist_loss_softmax_fwd")
    return loss, lse


def score_dist_loss_negsamp_fwd(metric: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor,
                                iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                                filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 0.0,
                                adversarial_temperature: float = 0.0, workspace: Optional[torch.Tensor] = None,
                                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ic: Optional[torch.Tensor] = None):
    """(loss, lw) fp32 [B] of include/ghf_distance_loss.h: ghf_dist_loss_negsamp_fwd — score_negsamp_fwd with z = -scale D(q_i,
    c[row]) over every row of c (of c[ic] with `ic`); lw = -inf and the positive term alone where a query has no negatives."""
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, alpha = _negsamp_args(
        q, c, target, iq, filt_ptr, filt_idx, scale, margin, adversarial_temperature, "score_dist_loss_negsamp_fwd")
    N, d = c.size(0), c.size(1)
    metric = _metric_arg(metric, d, "score_dist_loss_negsamp_fwd")
    ic = _ic_arg(ic, c, "score_dist_loss_negsamp_fwd")
    C = N if ic is None else ic.numel()
    loss, lw = _f32_out_pair(out, (B,), (B,), q.device, "score_dist_loss_negsamp_fwd")
    ws = _workspace(workspace, dist_loss_fwd_workspace_bytes, q.device, "score_dist_loss_negsamp_fwd", B=B, C=C, d=d, nnz=nnz)
    _check(load().ghf_dist_loss_negsamp_fwd(metric, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz,
                                            q.size(0), N, B, d, scale, margin, alpha, _ptr(ic), C, _ptr(ws), ws.numel(), _ptr(loss),
                                            _ptr(lw), _stream()), "ghf_dist_loss_negsamp_fwd")
    return loss, lw


def score_dist_loss_bwd(metric: int, mode: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, saved: torch.Tensor,
                        grad_loss: torch.Tensor, iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                        filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 0.0,
                        adversarial_temperature: float = 0.0, workspace: Optional[torch.Tensor] = None,
                        out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ic: Optional[torch.Tensor] = None):
    """(dq [B, d], dc [C, d]) fp32 of include/ghf_distance_loss.h: ghf_dist_loss_bwd, `mode` NEG_SOFTMAX or NEG_NEGSAMP and
    `saved` that forward's lse / lw.  dq[i] = -sum_j G_ij g(i, j) per query (not scattered through iq); dc[j] = +sum_i G_ij
    g(i, j), row j the gradient of c[ic[j]] (of c[j] without `ic`, where C = N); every row written."""
    if mode not in (NEG_SOFTMAX, NEG_NEGSAMP):
        raise ValueError(f"score_dist_loss_bwd: mode must be NEG_SOFTMAX or NEG_NEGSAMP, got {mode}")
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, alpha = _negsamp_args(
        q, c, target, iq, filt_ptr, filt_idx, scale, margin, adversarial_temperature, "score_dist_loss_bwd")
    saved, grad_loss = _req(saved, torch.float32, "saved"), _req(grad_loss, torch.float32, "grad_loss")
    if saved.numel() != B or grad_loss.numel() != B:
        raise ValueError(f"score_dist_loss_bwd: saved and grad_loss must hold B = {B} values")
    N, d = c.size(0), c.size(1)
    metric = _metric_arg(metric, d, "score_dist_loss_bwd")
    ic = _ic_arg(ic, c, "score_dist_loss_bwd")
    C = N if ic is None else ic.numel()
    ws = _workspace(workspace, dist_loss_bwd_workspace_bytes, q.device, "score_dist_loss_bwd", B=B, C=C, d=d, nnz=nnz)
    dq, dc = _f32_out_pair(out, (B, d), (C, d), q.device, "score_dist_loss_bwd")
    _check(load().ghf_dist_loss_bwd(metric, mode, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz,
                                    q.size(0), N, B, d, scale, margin, alpha, _ptr(ic), C, _ptr(saved), _ptr(grad_loss), _ptr(ws),
                                    ws.numel(), _ptr(dq), _ptr(dc), _stream()), "ghf_dist_loss_bwd")
    return dq, dc


def score_dist_softmax_fwd(metric: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
                           iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                           filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, workspace: Optional[torch.Tensor] = None,
                           out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """(loss, lse) fp32 [B] of include/ghf_distance.h: ghf_dist_softmax_fwd — score_neg_softmax_fwd with z = -scale D(q_i,
    c[row])."""
    return _per_query("ghf_dist_softmax_fwd", "score_dist_softmax_fwd", lambda d: (_metric_arg(metric, d, "score_dist_softmax_fwd"),),
                      q, c, target, neg, iq, filt_ptr, filt_idx, workspace, dist_workspace_bytes, out, _PQ_LOSS, scale=scale,
                      bias_slot=False)


def score_dist_negsamp_fwd(metric: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
                           iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                           filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 0.0,
                           adversarial_temperature: float = 0.0, workspace: Optional[torch.Tensor] = None,
                           out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """(loss, lw) fp32 [B] of include/ghf_distance.h: ghf_dist_negsamp_fwd — score_neg_negsamp_fwd with z = -scale D(q_i,
    c[row]); at scale = 1 and margin = gamma the positive term is -log sigmoid(gamma - D_t), RotatE's."""
    return _per_query("ghf_dist_negsamp_fwd", "score_dist_negsamp_fwd", lambda d: (_metric_arg(metric, d, "score_dist_negsamp_fwd"),),
                      q, c, target, neg, iq, filt_ptr, filt_idx, workspace, dist_workspace_bytes, out, _PQ_LOSS, scale=scale,
                      margin=margin, alpha=adversarial_temperature, bias_slot=False)


def score_dist_bwd(metric: int, mode: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
                   saved: torch.Tensor, grad_loss: torch.Tensor, iq: Optional[torch.Tensor] = None,
                   filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0,
                   margin: float = 0.0, adversarial_temperature: float = 0.0, workspace: Optional[torch.Tensor] = None,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """(dq [B, d], coef [B, K + 1]) fp32 of include/ghf_distance.h: ghf_dist_bwd, `mode` NEG_SOFTMAX or NEG_NEGSAMP and `saved`
    that forward's lse / lw.  coef means what score_neg_bwd's means (the gradient with respect to the score s = -D of every
    position, the target's last); dq[i] = -(sum_j coef[i, j] g(i, neg[i, j]) + coef[i, K] g(i, target[i])), g = dD / dq.  The
    gradient of c is dist_rows_grad over coef (autograd.PerQueryLossFn)."""
    if mode not in (NEG_SOFTMAX, NEG_NEGSAMP):
        raise ValueError(f"score_dist_bwd: mode must be NEG_SOFTMAX or NEG_NEGSAMP, got {mode}")
    return _per_query("ghf_dist_bwd", "score_dist_bwd", lambda d: (_metric_arg(metric, d, "score_dist_bwd"), mode), q, c, target, neg,
                      iq, filt_ptr, filt_idx, workspace, dist_workspace_bytes, out, _PQ_GRADS, scale=scale, margin=margin,
                      alpha=adversarial_temperature, bias_slot=False, saved=(saved, torch.float32, "saved", grad_loss))


def dist_rows_grad(metric: int, q: torch.Tensor, c: torch.Tensor, coef: torch.Tensor, perm: torch.Tensor, off: torch.Tensor,
                   iq: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dc [N, d] fp32 of include/ghf_distance.h: ghf_dist_rows_grad — the gradient of the candidate rows under a distance:
    dc[v] = sum_{e in off[v] .. off[v + 1]} coef[perm[e]] g(query perm[e] // (K + 1), v), e ascending, `coef` [B, K + 1]
    score_dist_bwd's and (perm, off) group_edges' for the B (K + 1) node ids [neg | target]; exact zeros for a node nobody
    names."""
    q, c, iq, _, _, B, _ = _rank_args(q, c, iq, None, None, "dist_rows_grad")
    coef = _req(coef, torch.float32, "coef")
    perm, off = _req(perm, torch.int64, "perm"), _req(off, torch.int64, "off")
    N, d = c.size(0), c.size(1)
    metric = _metric_arg(metric, d, "dist_rows_grad")
    if coef.dim() != 2 or coef.size(0) != B or coef.size(1) < 2:
        raise ValueError(f"dist_rows_grad: coef must be [B = {B}, K + 1], got {tuple(coef.shape)}")
    if perm.numel() != coef.numel() or off.numel() != N + 1:
        raise ValueError(f"dist_rows_grad: perm must hold B (K + 1) = {coef.numel()} entries and off N + 1 = {N + 1}, got "
                         f"{perm.numel()} and {off.numel()}")
    dc = _f32_out(out, (N, d), q.device, "dist_rows_grad")
    _check(load().ghf_dist_rows_grad(metric, _ptr(q), _ptr(c), _ptr(iq), q.size(0), N, B, d, coef.size(1) - 1, _ptr(coef), _ptr(perm),
                                     _ptr(off), _ptr(dc), _stream()), "ghf_dist_rows_grad")
    return dc


# ---- pairwise ranking losses on per-query negative sets (include/ghf_pairwise.h, csrc/pairwise.hip) -----------------------
def pair_workspace_bytes(B: int, K: int, d: int, nnz: int) -> int:
    return int(load().ghf_pair_workspace_bytes(B, K, d, nnz))


def _pair_selectors(metric: int, kind: int, d: int, bias, what: str) -> Tuple[int, int]:
    if metric not in (PAIR_DOT, DIST_L1, DIST_L2, DIST_COMPLEX):
        raise ValueError(f"{what}: metric must be PAIR_DOT, DIST_L1, DIST_L2 or DIST_COMPLEX, got {metric}")
    if metric == DIST_COMPLEX and d % 2:
        raise ValueError(f"{what}: DIST_COMPLEX reads the rows as interleaved re / im pairs and needs an even d, got {d}")
    if kind not in (PAIR_HINGE, PAIR_LOGISTIC):
        raise ValueError(f"{what}: kind must be PAIR_HINGE or PAIR_LOGISTIC, got {kind}")
    if bias is not None and metric != PAIR_DOT:
        raise ValueError(f"{what}: no per-candidate bias under a distance")
    return int(metric), int(kind)


def score_pair_fwd(metric: int, kind: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
                   iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                   filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 1.0, normalize: bool = True,
                   workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                   bias: Optional[torch.Tensor] = None):
    """(loss fp32 [B], count int32 [B], active int32 [B]) of include/ghf_pairwise.h: ghf_pair_fwd — the hinge (`kind`
    PAIR_HINGE) or logistic (PAIR_LOGISTIC) pairwise loss of query i's target against ITS OWN negatives neg[i, :]: with u_ij =
    (z_ij - z_it) + margin over the positions J_i outside the query's list other than the target, loss = sum phi(u) (over n_i =
    count[i] with `normalize`), active = #{u_ij > 0}.  `metric` PAIR_DOT: z = scale q . c[row] (+ bias[row]); DIST_L1 / DIST_L2 /
    DIST_COMPLEX: z = -scale D(q_i, c[row]), no bias.  With `workspace` (uint8, pair_workspace_bytes) and `out` given the call
    allocates nothing."""
    return _per_query("ghf_pair_fwd", "score_pair_fwd", lambda d: _pair_selectors(metric, kind, d, bias, "score_pair_fwd"), q, c, target,
                      neg, iq, filt_ptr, filt_idx, workspace, pair_workspace_bytes, out,
                      ((torch.float32, "B"), (torch.int32, "B"), (torch.int32, "B")),
                      "out must be a contiguous fp32 [{B}] and two contiguous int32 [{B}] tensors", scale=scale, margin=margin,
                      normalize=normalize, bias=bias)


def score_pair_bwd(metric: int, kind: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor,
                   count: torch.Tensor, grad_loss: torch.Tensor, iq: Optional[torch.Tensor] = None,
                   filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0,
                   margin: float = 1.0, normalize: bool = True, workspace: Optional[torch.Tensor] = None,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, bias: Optional[torch.Tensor] = None):
    """(dq [B, d], coef [B, K + 1]) fp32 of include/ghf_pairwise.h: ghf_pair_bwd, `count` the forward's.  coef[i, j] is the
    gradient of the loss sum with respect to the score of position j of query i (0 where the position takes no part), coef[i,
    K] the target's: minus the sum of the row's others.  dq is per query (not scattered through iq), formed from coef as
    score_neg_bwd (PAIR_DOT) or score_dist_bwd (a distance) form it.  The gradient of c is a grouped sum over coef
    (autograd.PerQueryLossFn)."""
    return _per_query("ghf_pair_bwd", "score_pair_bwd", lambda d: _pair_selectors(metric, kind, d, bias, "score_pair_bwd"), q, c, target,
                      neg, iq, filt_ptr, filt_idx, workspace, pair_workspace_bytes, out, _PQ_GRADS, scale=scale, margin=margin,
                      normalize=normalize, bias=bias, saved=(count, torch.int32, "count", grad_loss))


# ---- the pairwise losses under a distance against every node or a candidate subset (include/ghf_pairwise_sweep.h) --------
def dist_pair_fwd_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_dist_pair_fwd_workspace_bytes(B, C, d, nnz))


def dist_pair_bwd_workspace_bytes(B: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_dist_pair_bwd_workspace_bytes(B, C, d, nnz))


def _pair_sweep_args(metric, kind, q, c, target, iq, filt_ptr, filt_idx, scale, margin, normalize, ic, what: str):
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale = _softmax_args(q, c, target, iq, filt_ptr, filt_idx, scale, what)
    margin = float(margin)
    if not (float("-inf") < margin < float("inf")):
        raise ValueError(f"{what}: margin must be finite, got {margin}")
    if not isinstance(normalize, bool):
        raise TypeError(f"{what}: normalize must be a bool, got {normalize!r}")
    metric = _metric_arg(metric, c.size(1), what)
    if kind not in (PAIR_HINGE, PAIR_LOGISTIC):
        raise ValueError(f"{what}: kind must be PAIR_HINGE or PAIR_LOGISTIC, got {kind}")
    ic = _ic_arg(ic, c, what)
    return metric, int(kind), q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, ic, (c.size(0) if ic is None else ic.numel())


def score_dist_pair_sweep_fwd(metric: int, kind: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor,
                              iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                              filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 1.0,
                              normalize: bool = True, workspace: Optional[torch.Tensor] = None,
                              out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                              ic: Optional[torch.Tensor] = None):
    """(loss fp32 [B], dsum fp32 [B], count int32 [B], active int32 [B]) of include/ghf_pairwise_sweep.h: ghf_dist_pair_fwd —
    score_pair_fwd under a distance with every row of c (of c[ic] with `ic`, int64 [C] strictly ascending node ids, which must
    hold every target) as the negatives of every query: u_ij = (z_ij - z_it) + margin with z = -scale D over J_i, the
    candidates outside the query's list other than its target; loss = sum phi(u) (over n_i = count[i] with `normalize`), dsum
    = sum phi'(u) (what the backward needs for the target's coefficient), active = #{u_ij > 0}.  Nothing of size B x C is
    stored; with `workspace` (uint8, dist_pair_fwd_workspace_bytes) and `out` the call allocates nothing."""
    what = "score_dist_pair_sweep_fwd"
    metric, kind, q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, ic, C = _pair_sweep_args(
        metric, kind, q, c, target, iq, filt_ptr, filt_idx, scale, margin, normalize, ic, what)
    N, d = c.size(0), c.size(1)
    if out is None:
        loss, dsum = (torch.empty(B, dtype=torch.float32, device=q.device) for _ in range(2))
        count, active = (torch.empty(B, dtype=torch.int32, device=q.device) for _ in range(2))
    else:
        if len(out) != 4:
            raise ValueError(f"{what}: out must be two contiguous fp32 [{B}] and two contiguous int32 [{B}] tensors")
        loss, dsum = _f32_out_pair(out[:2], (B,), (B,), q.device, what)
        count, active = _req(out[2], torch.int32, "out"), _req(out[3], torch.int32, "out")
        if any(tuple(t.shape) != (B,) or not t.is_contiguous() for t in out[2:]):
            raise ValueError(f"{what}: out must be two contiguous fp32 [{B}] and two contiguous int32 [{B}] tensors")
    ws = _workspace(workspace, dist_pair_fwd_workspace_bytes, q.device, what, B=B, C=C, d=d, nnz=nnz)
    _check(load().ghf_dist_pair_fwd(metric, kind, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz,
                                    q.size(0), N, B, d, scale, margin, int(normalize), _ptr(ic), C, _ptr(ws), ws.numel(), _ptr(loss),
                                    _ptr(dsum), _ptr(count), _ptr(active), _stream()), "ghf_dist_pair_fwd")
    return loss, dsum, count, active


def score_dist_pair_sweep_bwd(metric: int, kind: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, dsum: torch.Tensor,
                              count: torch.Tensor, grad_loss: torch.Tensor, iq: Optional[torch.Tensor] = None,
                              filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0,
                              margin: float = 1.0, normalize: bool = True, workspace: Optional[torch.Tensor] = None,
                              out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ic: Optional[torch.Tensor] = None):
    """(dq [B, d], dc [C, d]) fp32 of include/ghf_pairwise_sweep.h: ghf_dist_pair_bwd, `dsum` and `count` the forward's.  dq[i]
    = -sum_j G_ij g(i, j) per query (not scattered through iq); dc[j] = +sum_i G_ij g(i, j), row j the gradient of c[ic[j]] (of
    c[j] without `ic`, where C = N); G_ij = w_i phi'(u_ij) on J_i, -w_i dsum[i] on the target pair; every row written."""
    what = "score_dist_pair_sweep_bwd"
    metric, kind, q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, ic, C = _pair_sweep_args(
        metric, kind, q, c, target, iq, filt_ptr, filt_idx, scale, margin, normalize, ic, what)
    dsum, grad_loss = _req(dsum, torch.float32, "dsum"), _req(grad_loss, torch.float32, "grad_loss")
    count = _req(count, torch.int32, "count")
    if dsum.numel() != B or count.numel() != B or grad_loss.numel() != B:
        raise ValueError(f"{what}: dsum, count and grad_loss must hold B = {B} values")
    N, d = c.size(0), c.size(1)
    ws = _workspace(workspace, dist_pair_bwd_workspace_bytes, q.device, what, B=B, C=C, d=d, nnz=nnz)
    dq, dc = _f32_out_pair(out, (B, d), (C, d), q.device, what)
    _check(load().ghf_dist_pair_bwd(metric, kind, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz,
                                    q.size(0), N, B, d, scale, margin, int(normalize), _ptr(ic), C, _ptr(dsum), _ptr(count),
                                    _ptr(grad_loss), _ptr(ws), ws.numel(), _ptr(dq), _ptr(dc), _stream()), "ghf_dist_pair_bwd")
    return dq, dc


# ---- the pairwise losses by dot product against every node or a candidate subset (include/ghf_pairwise_dot_sweep.h) -------
def score_pair_fwd_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_pair_fwd_workspace_bytes(B, N, C, d, nnz))


def score_pair_bwd_workspace_bytes(B: int, N: int, C: int, d: int, nnz: int) -> int:
    return int(load().ghf_score_pair_bwd_workspace_bytes(B, N, C, d, nnz))


def _pair_dot_sweep_args(kind, q, c, target, iq, filt_ptr, filt_idx, scale, margin, normalize, ic, bias, what: str):
    q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale = _softmax_args(q, c, target, iq, filt_ptr, filt_idx, scale, what)
    margin = float(margin)
    if not (float("-inf") < margin < float("inf")):
        raise ValueError(f"{what}: margin must be finite, got {margin}")
    if not isinstance(normalize, bool):
        raise TypeError(f"{what}: normalize must be a bool, got {normalize!r}")
    if kind not in (PAIR_HINGE, PAIR_LOGISTIC):
        raise ValueError(f"{what}: kind must be PAIR_HINGE or PAIR_LOGISTIC, got {kind}")
    ic = _ic_arg(ic, c, what)
    bias = _bias_arg(bias, c, what)
    return int(kind), q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, ic, (0 if ic is None else ic.numel()), bias


def score_pair_sweep_fwd(kind: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, iq: Optional[torch.Tensor] = None,
                         filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0,
                         margin: float = 1.0, normalize: bool = True, workspace: Optional[torch.Tensor] = None,
                         out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                         ic: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
    """(loss fp32 [B], dsum fp32 [B], count int32 [B], active int32 [B]) of include/ghf_pairwise_dot_sweep.h: ghf_score_pair_fwd
    — the hinge (`kind` PAIR_HINGE) or logistic (PAIR_LOGISTIC) pairwise loss with every row of c (of c[ic] with `ic`, int64 [C]
    strictly ascending node ids, which must hold every target) as the negatives of every query: u_ij = (z_ij - z_it) + margin
    with z = scale q . c[j] (+ bias[j]) over J_i, the candidates outside the query's list other than its target; loss = sum
    phi(u) (over n_i = count[i] with `normalize`), dsum = sum phi'(u) (what the backward needs for the target's coefficient),
    active = #{u_ij > 0}.  Nothing of size B x C is stored; with `workspace` (uint8, score_pair_fwd_workspace_bytes, C = 0 for
    every node) and `out` the call allocates nothing."""
    what = "score_pair_sweep_fwd"
    kind, q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, ic, C, bias = _pair_dot_sweep_args(
        kind, q, c, target, iq, filt_ptr, filt_idx, scale, margin, normalize, ic, bias, what)
    N, d = c.size(0), c.size(1)
    if out is None:
        loss, dsum = (torch.empty(B, dtype=torch.float32, device=q.device) for _ in range(2))
        count, active = (torch.empty(B, dtype=torch.int32, device=q.device) for _ in range(2))
    else:
        if len(out) != 4:
            raise ValueError(f"{what}: out must be two contiguous fp32 [{B}] and two contiguous int32 [{B}] tensors")
        loss, dsum = _f32_out_pair(out[:2], (B,), (B,), q.device, what)
        count, active = _req(out[2], torch.int32, "out"), _req(out[3], torch.int32, "out")
        if any(tuple(t.shape) != (B,) or not t.is_contiguous() for t in out[2:]):
            raise ValueError(f"{what}: out must be two contiguous fp32 [{B}] and two contiguous int32 [{B}] tensors")
    ws = _workspace(workspace, score_pair_fwd_workspace_bytes, q.device, what, B=B, N=N, C=C, d=d, nnz=nnz)
    _check(load().ghf_score_pair_fwd(kind, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N,
                                     B, d, scale, margin, int(normalize), _ptr(ic), C, _ptr(bias), _ptr(ws), ws.numel(), _ptr(loss),
                                     _ptr(dsum), _ptr(count), _ptr(active), _stream()), "ghf_score_pair_fwd")
    return loss, dsum, count, active


def score_pair_sweep_bwd(kind: int, q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, dsum: torch.Tensor, count: torch.Tensor,
                         grad_loss: torch.Tensor, iq: Optional[torch.Tensor] = None, filt_ptr: Optional[torch.Tensor] = None,
                         filt_idx: Optional[torch.Tensor] = None, scale: float = 1.0, margin: float = 1.0, normalize: bool = True,
                         workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                         ic: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, want_db: bool = True):
    """(dq [B, d], dc [N, d]) fp32 of include/ghf_pairwise_dot_sweep.h: ghf_score_pair_bwd, `dsum` and `count` the forward's —
    dq per query (not scattered through iq), every row of dc written; G_ij = w_i phi'(u_ij) on J_i, -w_i dsum[i] on the target
    pair.  With `ic` (the forward's) dc is [C, d], row j the gradient of row ic[j] of c.  With `bias` (the forward's) the result
    is (dq, dc, db) as score_softmax_bwd's."""
    what = "score_pair_sweep_bwd"
    kind, q, c, target, iq, filt_ptr, filt_idx, B, nnz, scale, margin, ic, C, bias = _pair_dot_sweep_args(
        kind, q, c, target, iq, filt_ptr, filt_idx, scale, margin, normalize, ic, bias, what)
    dsum, grad_loss = _req(dsum, torch.float32, "dsum"), _req(grad_loss, torch.float32, "grad_loss")
    count = _req(count, torch.int32, "count")
    if dsum.numel() != B or count.numel() != B or grad_loss.numel() != B:
        raise ValueError(f"{what}: dsum, count and grad_loss must hold B = {B} values")
    N, d = c.size(0), c.size(1)
    M = C if C else N
    ws = _workspace(workspace, score_pair_bwd_workspace_bytes, q.device, what, B=B, N=N, C=C, d=d, nnz=nnz)
    dq, dc = _f32_out_pair(out, (B, d), (M, d), q.device, what)
    db = torch.empty(M, dtype=torch.float32, device=q.device) if bias is not None and want_db else None
    _check(load().ghf_score_pair_bwd(kind, _ptr(q), _ptr(c), _ptr(iq), _ptr(target), _ptr(filt_ptr), _ptr(filt_idx), nnz, q.size(0), N,
                                     B, d, scale, margin, int(normalize), _ptr(ic), C, _ptr(bias), _ptr(dsum), _ptr(count),
                                     _ptr(grad_loss), _ptr(ws), ws.numel(), _ptr(dq), _ptr(dc), _ptr(db), _stream()),
           "ghf_score_pair_bwd")
    return (dq, dc) if bias is None else (dq, dc, db)


# ---- relation-typed query rows (include/ghf.h: ghf_relation_rows, csrc/relation.hip) ------------------------------------
GHF_REL_ADD_X = 1
GHF_REL_TRANSPOSE = 2


def relation_rows_workspace_bytes(B: int, R: int) -> int:
    return int(load().ghf_relation_rows_workspace_bytes(B, R))


def relation_rows(x: torch.Tensor, rel: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  ix: Optional[torch.Tensor] = None, add_x: bool = True, transpose: bool = False,
                  group: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, workspace: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = [x[ix[i]]] + x[ix[i]] @ op(W[rel[i]]) + [bias[rel[i]]], fp32 [B, d], with no matrix gathered per query.
    x [rows_x, d]; rel int64 [B]; W [R, d, d] natural; bias [R, d] or None; ix int64 [B] or None (= the rows in order);
    transpose: multiply by W[r]^T.  group = group_edges(rel, R) when the caller has it (the backward reuses the forward's).
    An id out of range gives a NaN row.  With `group`, `workspace` (uint8, relation_rows_workspace_bytes) and `out` given
    the call allocates nothing."""
    x = _req(x, torch.float32, "x")
    W = _req(W, torch.float32, "W")
    rel = _req(rel, torch.int64, "rel")
    if x.dim() != 2 or W.dim() != 3 or W.size(1) != x.size(1) or W.size(2) != x.size(1) or rel.dim() != 1:
        raise ValueError(f"relation_rows: need x [rows, d], W [R, d, d] and rel [B], got {tuple(x.shape)}, {tuple(W.shape)}, "
                         f"{tuple(rel.shape)}")
    (rows_x, d), R = x.shape, W.size(0)
    ix = None if ix is None else _req(ix, torch.int64, "ix")
    B = rel.numel()
    if ix is not None and (ix.dim() != 1 or ix.numel() != B):
        raise ValueError(f"relation_rows: ix must name one row per entry of rel ({B}), got {tuple(ix.shape)}")
    if bias is not None:
        bias = _req(bias, torch.float32, "bias")
        if tuple(bias.shape) != (R, d):
            raise ValueError(f"relation_rows: bias must be [{R}, {d}], got {tuple(bias.shape)}")
    for name, t in (("W", W), ("rel", rel), ("ix", ix), ("bias", bias)):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"relation_rows: {name} is on {t.device}, x on {x.device}")
    if rows_x == 0 or d == 0:
        raise ValueError(f"relation_rows: unsupported sizes B={B} R={R} rows={rows_x} d={d}")
    ws = _workspace(workspace, relation_rows_workspace_bytes, x.device, "relation_rows", B=B, R=R)
    perm, goff = group_edges(rel, R) if group is None else (_req(group[0], torch.int64, "perm"), _req(group[1], torch.int64, "goff"))
    if perm.numel() != B or goff.numel() != R + 1:
        raise ValueError(f"relation_rows: group must be (perm [{B}], goff [{R + 1}])")
    out = _f32_out(out, (B, d), x.device, "relation_rows")
    flags = (GHF_REL_ADD_X if add_x else 0) | (GHF_REL_TRANSPOSE if transpose else 0)
    _check(load().ghf_relation_rows(_ptr(x), _ptr(ix), _ptr(rel), _ptr(W), _ptr(bias), _ptr(perm), _ptr(goff), rows_x, B, R, d,
                                    flags, _ptr(ws), ws.numel(), _ptr(out), _stream()), "ghf_relation_rows")
    return out


# ---- relation prediction: every relation's score for a pair (include/ghf.h: ghf_relation_scores, csrc/relation_predict.hip) ----
def relation_scores_bwd_rows_workspace_bytes(B: int, U: int, d: int) -> int:
    return int(load().ghf_relation_scores_bwd_rows_workspace_bytes(B, U, d))


def relation_scores_bwd_weights_workspace_bytes(B: int, U: int, d: int) -> int:
    return int(load().ghf_relation_scores_bwd_weights_workspace_bytes(B, U, d))


def _relation_scores_args(x, ia, ib, W, bias, G, what: str):
    x = _req(x, torch.float32, "x")
    ia = _req(ia, torch.int64, "ia")
    ib = None if ib is None else _req(ib, torch.int64, "ib")
    if x.dim() != 2 or x.size(0) == 0 or x.size(1) == 0 or ia.dim() != 1 or ia.numel() == 0:
        raise ValueError(f"{what}: need x [rows, d] and ia [B], got {tuple(x.shape)} and {tuple(ia.shape)}")
    (rows_x, d), B = x.shape, ia.numel()
    if ib is not None and (ib.dim() != 1 or ib.numel() != B):
        raise ValueError(f"{what}: ib must name one row per entry of ia ({B}), got {tuple(ib.shape)}")
    U = None
    if W is not None:
        W = _req(W, torch.float32, "W")
        if W.dim() != 3 or W.size(0) == 0 or W.size(1) != d or W.size(2) != d:
            raise ValueError(f"{what}: W must be [U, {d}, {d}], got {tuple(W.shape)}")
        U = W.size(0)
    if G is not None:
        G = _req(G, torch.float32, "G")
        if G.dim() != 2 or G.size(0) != B or G.size(1) == 0 or (U is not None and G.size(1) != U):
            raise ValueError(f"{what}: G must be [B = {B}, U{'' if U is None else f' = {U}'}], got {tuple(G.shape)}")
        U = G.size(1)
    if bias is not None:
        bias = _req(bias, torch.float32, "bias")
        if tuple(bias.shape) != (U, d):
            raise ValueError(f"{what}: bias must be [{U}, {d}], got {tuple(bias.shape)}")
    for name, t in (("ia", ia), ("ib", ib), ("W", W), ("bias", bias), ("G", G)):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"{what}: {name} is on {t.device}, x on {x.device}")
    return x, ia, ib, W, bias, G, rows_x, B, U, d


def relation_scores(x: torch.Tensor, ia: torch.Tensor, ib: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
                    add_x: bool = True, transpose: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i][u] = q(i, u) . x[ib[i]] with q(i, u) = [x[ia[i]]] + x[ia[i]] @ op(W[u]) + [bias[u]]: every relation's score
    for every pair, fp32 [B, U], in one sweep that stores nothing of size B x U x d.  x [rows, d]; ia, ib int64 [B];
    W [U, d, d]; bias [U, d] or None.  An id out of range gives a NaN row.  With `out` given the call allocates nothing."""
    x, ia, ib, W, bias, _, rows_x, B, U, d = _relation_scores_args(x, ia, ib, W, bias, None, "relation_scores")
    out = _f32_out(out, (B, U), x.device, "relation_scores")
    flags = (GHF_REL_ADD_X if add_x else 0) | (GHF_REL_TRANSPOSE if transpose else 0)
    _check(load().ghf_relation_scores(_ptr(x), _ptr(ia), _ptr(ib), _ptr(W), _ptr(bias), rows_x, B, U, d, flags, _ptr(out),
                                      _stream()), "ghf_relation_scores")
    return out


def relation_scores_bwd_rows(x: torch.Tensor, ia: torch.Tensor, G: torch.Tensor, W: torch.Tensor,
                             bias: Optional[torch.Tensor] = None, add_x: bool = True, transpose: bool = False,
                             workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = sum_u G[i][u] q(i, u), fp32 [B, d], u ascending (q as in relation_scores).  As called: the gradient of
    the b rows; with ia = the forward's ib, `transpose` flipped and no bias: the gradient of the a rows."""
    x, ia, _, W, bias, G, rows_x, B, U, d = _relation_scores_args(x, ia, None, W, bias, G, "relation_scores_bwd_rows")
    ws = _workspace(workspace, relation_scores_bwd_rows_workspace_bytes, x.device, "relation_scores_bwd_rows", B=B, U=U, d=d)
    out = _f32_out(out, (B, d), x.device, "relation_scores_bwd_rows")
    flags = (GHF_REL_ADD_X if add_x else 0) | (GHF_REL_TRANSPOSE if transpose else 0)
    _check(load().ghf_relation_scores_bwd_rows(_ptr(x), _ptr(ia), _ptr(G), _ptr(W), _ptr(bias), rows_x, B, U, d, flags, _ptr(ws),
                                               ws.numel(), _ptr(out), _stream()), "ghf_relation_scores_bwd_rows")
    return out


def relation_scores_bwd_weights(x: torch.Tensor, ia: torch.Tensor, ib: torch.Tensor, G: torch.Tensor, want_bias: bool = True,
                                workspace: Optional[torch.Tensor] = None,
                                out: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None):
    """(dW [U, d, d], dbias [U, d] or None): dW[u] = sum_i G[i][u] x[ia[i]]^T x[ib[i]], dbias[u] = sum_i G[i][u] x[ib[i]],
    i ascending.  A query with an id out of range adds nothing."""
    x, ia, ib, _, _, G, rows_x, B, U, d = _relation_scores_args(x, ia, ib, None, None, G, "relation_scores_bwd_weights")
    if ib is None:
        raise ValueError("relation_scores_bwd_weights: ib is needed")
    ws = _workspace(workspace, relation_scores_bwd_weights_workspace_bytes, x.device, "relation_scores_bwd_weights", B=B, U=U, d=d)
    dW = _f32_out(None if out is None else out[0], (U, d, d), x.device, "relation_scores_bwd_weights")
    db = _f32_out(None if out is None else out[1], (U, d), x.device, "relation_scores_bwd_weights") if want_bias else None
    _check(load().ghf_relation_scores_bwd_weights(_ptr(x), _ptr(ia), _ptr(ib), _ptr(G), rows_x, B, U, d, 0, _ptr(ws), ws.numel(),
                                                  _ptr(dW), _ptr(db), _stream()), "ghf_relation_scores_bwd_weights")
    return dW, db


# ---- wide hidden sizes: relation-stationary layer (include/ghf.h, csrc/message_rs.hip) ---------------------------

def rs_supported(d: int) -> bool:
    return bool(load().ghf_message_rs_supported(d)) and os.environ.get("GHF_KERNEL") != "generic"


RS_MIN_RELATIONS = 160


def prefer_rs(d: int, R: int) -> bool:
    """Whether an inference plan for hidden size d and R relations should be a CSR plan for the relation-stationary layer:
    always where no destination-block kernel exists (d >= 256); at d = 128 from about 160 relations on — the block
    kernel re-streams a relation's weights per (block, relation) chunk, so its time grows with R while the
    relation-stationary layer's does not (tools/relation_sweep_rs.py, C3-sized graph, ms per layer, message_bx / relation-
    stationary: R = 64: 3.5 / 5.8, 96: 4.1 / 5.6, 128: 4.8 / 5.7, 192: 9.2 / 5.9, 256: 11.0 / 5.7)."""
    if not rs_supported(d) or os.environ.get("GHF_KERNEL") in ("bx", "pp"):
        return False
    return d >= 256 or R >= RS_MIN_RELATIONS or os.environ.get("GHF_KERNEL") in ("rs", "rs32")


def rs_exact(plan=None) -> bool:
    """The wide-row layer's pass 1 on fp32 MFMAs (exact fma chain) instead of two fp16 pieces: GHF_KERNEL=rs32, or a plan
    built for the exact kernels (GraphPlan.force_exact: the range guard's fallback) — carried by the plan, passed to
    edge_transform_fwd / segment_tail_fwd explicitly (no process-wide switch)."""
    return bool(plan is not None and getattr(plan, "force_exact", False)) or os.environ.get("GHF_KERNEL") == "rs32"


def edge_transform_fwd(h: torch.Tensor, rs, W_msg: torch.Tensor, W_self: torch.Tensor, bias: torch.Tensor, Y: torch.Tensor,
                       h_split: Optional[torch.Tensor] = None, exact: Optional[bool] = None) -> torch.Tensor:
    """Pass 1: per-edge results into Y [E, d] at the edges' destination-order positions (rs: plan.RsPlan; W_msg / W_self
    natural [R, d, d]).  Cuts the weights and — unless the caller has them (`h_split`, from the previous layer's pass 2) —
    the rows of h into their two fp16 pieces first (or transposes the weights, rs32).  Plans whose rows stand for runs of
    edges (rs.run_start: graphs with hubs) first sum every run's source rows (ghf_run_rows_fwd); the exact kernel has no
    such rows and runs the plan's per-edge twin."""
    lib = load()
    h = _req(h, torch.float32, "h")
    N, d = h.shape
    exact = rs_exact() if exact is None else (exact or rs_exact())
    if exact and rs.run_start is not None:
        rs = rs.per_edge()
        Y = rs.scratch(0, d, h.device)
    R = W_msg.size(0)
    Wm, Ws = _req(W_msg, torch.float32, "W_msg"), _req(W_self, torch.float32, "W_self")
    if exact:
        WmT, WsT = transpose_batched(Wm), transpose_batched(Ws)      # (named: they must outlive the launch's pointer taking)
        _check(lib.ghf_edge_transform_fwd(_ptr(h), N, d, _ptr(rs.src), _ptr(rs.dst), _ptr(rs.ypos), _ptr(rs.slice_tab),
                                          rs.slice_tab.size(0), _ptr(WmT), _ptr(WsT),
                                          _ptr(_req(bias, torch.float32, "bias")), _ptr(Y), _stream()), "ghf_edge_transform_fwd")
    else:
        hs = h_split if h_split is not None else split_rows(h, WLAYOUT_SPLIT2H)
        w2h = torch.empty(lib.ghf_weights_rs_bytes(R, d), dtype=torch.uint8, device=h.device)
        shift = torch.empty(R, dtype=torch.int32, device=h.device)
        _check(lib.ghf_weights_pack_rs(_ptr(Wm), _ptr(Ws), R, d, _ptr(w2h), _ptr(shift), _stream()), "ghf_weights_pack_rs")
        xs, nx = None, 0
        if rs.run_start is not None and rs.run_start.numel() > 1:
            nx = rs.run_start.numel() - 1
            xs = rs.run_scratch(nx, d)
            _check(lib.ghf_run_rows_fwd(_ptr(h), N, d, _ptr(rs.run_src), _ptr(rs.run_start), nx, _ptr(xs), _stream()), "ghf_run_rows_fwd")
        _check(lib.ghf_edge_transform_h_fwd(_ptr(hs), N, d, _ptr(rs.src), _ptr(rs.dst), _ptr(rs.ypos), _ptr(rs.slice_tab),
                                            rs.slice_tab.size(0), _ptr(w2h), R, _ptr(_req(bias, torch.float32, "bias")),
                                            _ptr(xs), nx, _ptr(rs.cnt), _ptr(Y), _stream()), "ghf_edge_transform_h_fwd")
    if rs.hub_of is not None:                       # hubs: their rows in chunks (fixed order); pass 2 adds the chunks' sums
        _check(load().ghf_segment_partial_fwd(_ptr(Y), _ptr(rs.hub_chunks), rs.hub_chunks.size(0), d, _ptr(rs.hub_scratch(d)),
                                              _stream()), "ghf_segment_partial_fwd")
    return Y


def segment_tail_fwd(Y: torch.Tensor, rs, h: Optional[torch.Tensor], ln_gamma, ln_beta, ln_eps: float, h_out: torch.Tensor,
                     row0: int = 0, rows: Optional[int] = None, flags: int = 0,
                     h_split_out: Optional[torch.Tensor] = None, exact: Optional[bool] = None) -> torch.Tensor:
    """Pass 2: destination sums of Y, mean and tail for rows [row0, row0+rows); `h_split_out` (alloc_split(N, d, SPLIT2H))
    also receives the rows in the form the next layer's pass 1 gathers."""
    N, d = h_out.shape
    rows = N - row0 if rows is None else rows
    exact = rs_exact() if exact is None else (exact or rs_exact())
    if exact and rs.run_start is not None:                        # (see edge_transform_fwd)
        rs = rs.per_edge()
        Y = rs.scratch(0, d, h_out.device)
    P = rs.hub_scratch(d) if rs.hub_of is not None else None      # filled by edge_transform_fwd
    _check(load().ghf_segment_tail_fwd(_ptr(Y), _ptr(rs.off), _ptr(rs.deg_of), _ptr(rs.hub_of), _ptr(rs.hub_tab), _ptr(P), _ptr(h), _ptr(ln_gamma),
                                       _ptr(ln_beta), float(ln_eps), row0, rows, d, _ptr(h_out), _ptr(h_split_out), N, flags,
                                       _stream()), "ghf_segment_tail_fwd")
    return h_out


# ---- backward pieces (include/ghf.h: "backward of the path") ----------------------------------------------------

def group_edges(rel_id: torch.Tensor, R: int):
    """(perm [E], goff [R+1]) int64: edge ids grouped stably by relation."""
    lib = load()
    rel = _req(rel_id, torch.int64, "rel_id")
    E = rel.numel()
    ws = torch.empty(lib.ghf_group_workspace_bytes(E), dtype=torch.uint8, device=rel.device)
    perm = torch.empty(E, dtype=torch.int64, device=rel.device)
    goff = torch.empty(R + 1, dtype=torch.int64, device=rel.device)
    _check(lib.ghf_group_edges(_ptr(rel), E, R, _ptr(ws), ws.numel(), _ptr(perm), _ptr(goff), _stream()), "ghf_group_edges")
    return perm, goff


def tail_bwd(grad_out: torch.Tensor, agg: torch.Tensor, h: torch.Tensor, gamma: torch.Tensor, eps: float, indeg: torch.Tensor,
             drop: Optional[torch.Tensor] = None, split_layout: Optional[int] = None):
    """(dpre, G, G_split, dgamma, dbeta) of include/ghf.h: ghf_tail_bwd (drop: the forward's scaled dropout mask, if any;
    split_layout: also return G cut as ``split_rows(G, split_layout)`` would, else G_split is None)."""
    lib = load()
    g = _req(grad_out, torch.float32, "grad_out")
    N, d = h.shape
    dpre, G = torch.empty_like(h), torch.empty_like(h)
    Gs = None if split_layout is None else alloc_split(N, d, split_layout, h.device)
    dgb = torch.empty(2, d, dtype=torch.float32, device=h.device)
    ws = torch.empty(max(int(lib.ghf_tail_bwd_workspace_floats(N, d)), 1), dtype=torch.float32, device=h.device)
    _check(lib.ghf_tail_bwd(_ptr(g), _ptr(_req(agg, torch.float32, "agg")), _ptr(_req(h, torch.float32, "h")),
                            _ptr(_req(gamma, torch.float32, "gamma")), float(eps), _ptr(indeg), N, d, _ptr(dpre), _ptr(G),
                            _ptr(Gs), _ptr(dgb), _ptr(ws), _ptr(None if drop is None else _req(drop, torch.float32, "drop")),
                            _stream()), "ghf_tail_bwd")
    return dpre, G, Gs, dgb[0], dgb[1]


def colsum(X: torch.Tensor, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[o] (+)= sum_v X[v][o] * (mask[v][o] > 0); accumulates when `out` is given."""
    lib = load()
    X = _req(X, torch.float32, "X")
    N, d = X.shape
    ws = torch.empty(lib.ghf_colsum_workspace_floats(N, d), dtype=torch.float32, device=X.device)
    acc = out is not None
    if out is None:
        out = torch.empty(d, dtype=torch.float32, device=X.device)
    _check(lib.ghf_colsum(_ptr(X), _ptr(None if mask is None else _req(mask, torch.float32, "mask")), N, d, _ptr(ws), _ptr(out),
                          1 if acc else 0, _stream()), "ghf_colsum")
    return out


def relu_mask(X: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    X = _req(X, torch.float32, "X")
    out = torch.empty_like(X)
    _check(load().ghf_relu_mask(_ptr(X), _ptr(_req(ref, torch.float32, "ref")), X.numel(), _ptr(out), _stream()), "ghf_relu_mask")
    return out


def group_outer(A: Optional[torch.Tensor], ia: Optional[torch.Tensor], B: torch.Tensor, ib: Optional[torch.Tensor],
                goff: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C[g] (+)= sum_{e in goff[g]..goff[g+1]} A[ia[e]]^T (outer) B[ib[e]]; A None: column sums of the gathered B rows
    ([G, 1, db])."""
    lib = load()
    B = _req(B, torch.float32, "B")
    A = None if A is None else _req(A, torch.float32, "A")
    goff = _req(goff, torch.int64, "goff")
    da, db, ng = (0 if A is None else A.size(1)), B.size(1), goff.numel() - 1
    acc = out is not None
    if out is None:
        out = torch.empty(ng, max(da, 1), db, dtype=torch.float32, device=B.device)
    _check(lib.ghf_group_outer(_ptr(A), _ptr(ia), da, _ptr(B), _ptr(ib), db, goff.data_ptr(), goff.data_ptr() + 8, ng,
                               _ptr(out), 1 if acc else 0, _stream()), "ghf_group_outer")
    return out


def split_row_scales(split: torch.Tensor, N: int, d: int) -> torch.Tensor:
    """The N row scales (float32 view, no copy) behind the N rows of a SPLIT2H split form (split_rows / alloc_split)."""
    return split.view(torch.float32)[N * d:N * d + N]


def edge_outer(h: torch.Tensor, G: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, slice_tab: torch.Tensor,
               slice_off: torch.Tensor, R: int, exact: bool = False, h_scales: Optional[torch.Tensor] = None,
               G_scales: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None):
    """(dW [R, 2d, d] = dW_msg stacked on dW_self, db [R, d]) of include/ghf.h: ghf_edge_outer (exact: the fp32 chain at
    every d — a step that fell back to the exact kernels).  h_scales / G_scales: the row scales of the two tensors' split
    forms (split_row_scales), when the caller holds them: ghf_edge_outer_scaled, same bits without the pass over h and G.
    order [S] int32: the launch order of the slices (ghf.h; the same bits in any order).  workspace: the call's scratch, for a
    caller that reads it afterwards (ghf.h: the range guard's counters) — float32, at least S (2 D D + D) + 64 elements, D =
    min(d, 128); allocated here when absent."""
    lib = load()
    h, G = _req(h, torch.float32, "h"), _req(G, torch.float32, "G")
    d, ns = h.size(1), slice_tab.size(0)
    D = min(d, 128)
    if workspace is None:
        ws = torch.empty(ns * (2 * D * D + D) + 64, dtype=torch.float32, device=h.device)
    else:
        ws = _req(workspace, torch.float32, "workspace")
        if ws.numel() < ns * (2 * D * D + D) + 64 or ws.device != h.device:
            raise ValueError("edge_outer: workspace of at least S (2 D D + D) + 64 floats on the tensors' device expected")
    dW = torch.empty(R, 2 * d, d, dtype=torch.float32, device=h.device)
    db = torch.empty(R, d, dtype=torch.float32, device=h.device)
    tabs = (_ptr(_req(src, torch.int64, "src")), _ptr(_req(dst, torch.int64, "dst")), _ptr(_req(slice_tab, torch.int64, "slice_tab")),
            _ptr(_req(slice_off, torch.int64, "slice_off")), _ptr(_req(order, torch.int32, "order")) if order is not None else None)
    if order is not None and order.numel() != ns:
        raise ValueError("edge_outer: one launch position per slice expected")
    if not exact and h_scales is not None and G_scales is not None and h.size(0) > 0:
        hsc, gsc = _req(h_scales, torch.float32, "h_scales"), _req(G_scales, torch.float32, "G_scales")
        if hsc.numel() != h.size(0) or gsc.numel() != G.size(0):
            raise ValueError("edge_outer: one row scale per row of h and of G expected")
        _check(lib.ghf_edge_outer_scaled(_ptr(h), _ptr(G), _ptr(hsc), _ptr(gsc), *tabs, ns, R, d, h.size(0), _ptr(ws), _ptr(dW),
                                         _ptr(db), _stream()), "ghf_edge_outer_scaled")
    else:
        _check(lib.ghf_edge_outer(_ptr(h), _ptr(G), *tabs, ns, R, d, 0 if exact else h.size(0), _ptr(ws), _ptr(dW), _ptr(db),
                                  _stream()), "ghf_edge_outer")
    return dW, db


_RANGES: dict = {}


def _row_ranges(K: int, step: int, device) -> torch.Tensor:
    """[0, step, 2 step, ..., K] on the device (cached: a handful of distinct sizes per model)."""
    key = (K, step, str(device))
    r = _RANGES.get(key)
    if r is None:
        n = (K + step - 1) // step
        r = torch.tensor([min(i * step, K) for i in range(n + 1)], dtype=torch.int64).to(device)
        if len(_RANGES) >= 64:
            _RANGES.pop(next(iter(_RANGES)))
        _RANGES[key] = r
    return r


def matmul_tn(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """A^T B for row-major A [K, M], B [K, N] -> [M, N] in exact fp32: ghf_group_outer over slices of the K rows (so that
    a tall contraction fills the chip), the slices' partial products summed in order by ghf_colsum."""
    K, M = A.shape
    N = B.size(1)
    tiles = ((M + 15) // 16) * ((N + 127) // 128)
    step = K if K <= 512 else max(256, ((K * tiles + 2047) // 2048 + 3) & ~3)      # aim at ~2000 workgroups
    goff = _row_ranges(K, step, A.device)
    part = group_outer(A, None, B, None, goff)
    if part.size(0) == 1:
        return part[0]
    return colsum(part.view(part.size(0), M * N)).view(M, N)


def matmul_nn(X: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """X W for row-major X [M, K], W [K, N] (the gradient of a Linear with respect to its input)."""
    return matmul_tn(transpose_batched(X.unsqueeze(0))[0], W)


def scale_exp(X: torch.Tensor, log_scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    X = _req(X, torch.float32, "X")
    out = torch.empty_like(X) if out is None else out
    _check(load().ghf_scale_exp(_ptr(X), X.numel(), _ptr(_req(log_scale, torch.float32, "log_scale")), _ptr(out), _stream()),
           "ghf_scale_exp")
    return out


def add3(a: torch.Tensor, b: torch.Tensor, c: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    a, b = _req(a, torch.float32, "a"), _req(b, torch.float32, "b")
    c = None if c is None else _req(c, torch.float32, "c")
    if a.numel() != b.numel() or (c is not None and c.numel() != a.numel()):
        raise ValueError("add3: operands differ in size")
    out = torch.empty_like(a) if out is None else out
    _check(load().ghf_add3(_ptr(a), _ptr(b), _ptr(c), a.numel(), _ptr(out), _stream()), "ghf_add3")
    return out


def rowscale(X: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    X, g = _req(X, torch.float32, "X"), _req(g, torch.float32, "g")
    n, d = X.shape
    if g.numel() != n:
        raise ValueError("rowscale: one factor per row expected")
    out = torch.empty_like(X)
    _check(load().ghf_rowscale(_ptr(X), _ptr(g), n, d, _ptr(out), _stream()), "ghf_rowscale")
    return out


def segment_axpy(w: torch.Tensor, iw: torch.Tensor, X: torch.Tensor, ix: torch.Tensor, off: torch.Tensor) -> torch.Tensor:
    """out[v] = sum_{e in off[v]..off[v+1]} w[iw[e]] * X[ix[e]] (include/ghf.h: ghf_segment_axpy)."""
    w, X = _req(w, torch.float32, "w"), _req(X, torch.float32, "X")
    iw, ix, off = _req(iw, torch.int64, "iw"), _req(ix, torch.int64, "ix"), _req(off, torch.int64, "off")
    if iw.numel() != ix.numel():
        raise ValueError("segment_axpy: one weight index per row index expected")
    nseg, (nx, d) = off.numel() - 1, X.shape
    out = torch.empty(nseg, d, dtype=torch.float32, device=X.device)
    _check(load().ghf_segment_axpy(_ptr(w), _ptr(iw), _ptr(X), _ptr(ix), _ptr(off), nseg, nx, d, _ptr(out), _stream()), "ghf_segment_axpy")
    return out


def dot(X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """[1] tensor: sum of the elementwise product (fixed summation order)."""
    X, Y = _req(X, torch.float32, "X"), _req(Y, torch.float32, "Y")
    n = X.numel()
    if Y.numel() != n:
        raise ValueError("dot: operands differ in size")
    ws = torch.empty((n + 8191) // 8192, dtype=torch.float32, device=X.device)
    out = torch.empty(1, dtype=torch.float32, device=X.device)
    _check(load().ghf_dot(_ptr(X), _ptr(Y), n, _ptr(ws), _ptr(out), _stream()), "ghf_dot")
    return out


def weightgen_acts(text_emb: torch.Tensor, head_params: Sequence[torch.Tensor], T: int, Hh: int, num_hidden: int,
                   hidden_drop: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[3, num_hidden, R, Hh]: the hidden activations of the three generator heads (post-ReLU, and post-dropout when the
    forward's masks are given)."""
    x = _req(text_emb, torch.float32, "text_emb")
    keep = [_req(p, torch.float32, "weight-generator parameter") for p in head_params]
    arr = (_vp * len(keep))(*[p.data_ptr() for p in keep])
    acts = torch.empty(3, num_hidden, x.size(0), Hh, dtype=torch.float32, device=x.device)
    _check(load().ghf_weightgen_acts(_ptr(x), arr, x.size(0), T, Hh, num_hidden, _ptr(acts),
                                     _ptr(None if hidden_drop is None else _req(hidden_drop, torch.float32, "hidden_drop")), _stream()),
           "ghf_weightgen_acts")
    return acts


def weightgen_bwd_supported(T: int, Hh: int, num_hidden: int) -> bool:
    return bool(load().ghf_weightgen_bwd_supported(T, Hh, num_hidden))


def weightgen_bwd(text_emb: torch.Tensor, head_params: Sequence[torch.Tensor], acts: Optional[torch.Tensor],
                  outs: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], log_scales: torch.Tensor, T: int, Hh: int,
                  num_hidden: int, d_in: int, d_out: int, log_keep: Optional[torch.Tensor] = None, want_dx: bool = True):
    """(dparams [one tensor per parameter], dls [3], d text_emb or None): include/ghf.h, ghf_weightgen_bwd — the three heads'
    backward in three launches.  log_scales: [3] float32 on the device."""
    lib = load()
    x = _req(text_emb, torch.float32, "text_emb")
    R, dev = x.size(0), x.device
    keep = [_req(p, torch.float32, "weight-generator parameter") for p in head_params]
    o = [_req(t, torch.float32, "generator output") for t in outs]
    g = [_req(t, torch.float32, "generator output gradient") for t in grads]
    ls = _req(log_scales, torch.float32, "log_scales")
    dparams = [torch.empty_like(p) for p in keep]
    dls = torch.empty(3, dtype=torch.float32, device=dev)
    dx = torch.empty(R, T, dtype=torch.float32, device=dev) if want_dx else None
    ws = torch.empty(lib.ghf_weightgen_bwd_workspace_floats(R, T, Hh, num_hidden, d_in, d_out), dtype=torch.float32, device=dev)
    arr = lambda ts: (_vp * len(ts))(*[t.data_ptr() for t in ts])       # noqa: E731
    ls_ptrs = (_vp * 3)(*[ls.data_ptr() + 4 * k for k in range(3)])
    dls_ptrs = (_vp * 3)(*[dls.data_ptr() + 4 * k for k in range(3)])
    _check(lib.ghf_weightgen_bwd(_ptr(x), arr(keep), _ptr(None if acts is None else _req(acts, torch.float32, "acts")), arr(o), arr(g),
                                 ls_ptrs, R, T, Hh, num_hidden, d_in, d_out,
                                 _ptr(None if log_keep is None else _req(log_keep, torch.float32, "log_keep")), arr(dparams), dls_ptrs,
                                 _ptr(dx), _ptr(ws), _stream()), "ghf_weightgen_bwd")
    return dparams, dls, dx


def text_encode_bwd(ids: torch.Tensor, lens: torch.Tensor, char_emb: torch.Tensor, W: torch.Tensor, te: torch.Tensor,
                    dte: torch.Tensor):
    """(d char_emb [V, C], d W [T, C], d b [T]) of ghf_text_encode_fwd."""
    E, Wt = _req(char_emb, torch.float32, "char_emb.weight"), _req(W, torch.float32, "proj.weight")
    te, dte = _req(te, torch.float32, "te"), _req(dte, torch.float32, "dte")
    U, Lmax = ids.shape
    V, Cd = E.shape
    T = Wt.size(0)
    ws = torch.empty(2 * U * Cd + U * T, dtype=torch.float32, device=E.device)
    dE, dW, db = torch.empty_like(E), torch.empty_like(Wt), torch.empty(T, dtype=torch.float32, device=E.device)
    _check(load().ghf_text_encode_bwd(_ptr(_req(ids, torch.int32, "ids")), _ptr(_req(lens, torch.int32, "lens")), U, Lmax,
                                      _ptr(E), V, Cd, _ptr(Wt), T, _ptr(te), _ptr(dte), _ptr(ws), _ptr(dE), _ptr(dW), _ptr(db),
                                      _stream()), "ghf_text_encode_bwd")
    return dE, dW, db


def transpose_batched(x: torch.Tensor) -> torch.Tensor:
    """[B, r, c] -> [B, c, r] (a copy)."""
    x = _req(x, torch.float32, "x")
    Bn, r, c = x.shape
    out = torch.empty(Bn, c, r, dtype=torch.float32, device=x.device)
    _check(load().ghf_transpose_batched(_ptr(x), Bn, r, c, _ptr(out), _stream()), "ghf_transpose_batched")
    return out


def weights_pack(top: Optional[torch.Tensor], bottom: Optional[torch.Tensor], transpose: bool, R: int, d: int, wlayout: int):
    """[top[r]; bottom[r]] (natural [R, d, d] each, None = zeros, optionally transposed) in the kernel's weight layout."""
    lib = load()
    dev = (top if top is not None else bottom).device
    out = torch.empty(lib.ghf_weights_bytes(R, d, d, wlayout) // 4, dtype=torch.float32, device=dev)
    _check(lib.ghf_weights_pack(_ptr(None if top is None else _req(top, torch.float32, "top")),
                                _ptr(None if bottom is None else _req(bottom, torch.float32, "bottom")), 1 if transpose else 0,
                                R, d, wlayout, _ptr(out), _stream()), "ghf_weights_pack")
    return out


def tail_fwd(agg: torch.Tensor, h: torch.Tensor, ln_gamma: torch.Tensor, ln_beta: torch.Tensor, ln_eps: float,
             h_out: torch.Tensor, row0: int = 0, rows: Optional[int] = None, drop: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = load()
    N, d = h.shape
    if rows is None:
        rows = N - row0
    _check(lib.ghf_tail_fwd(_ptr(agg), _ptr(h), _ptr(ln_gamma), _ptr(ln_beta), float(ln_eps), row0, rows, d,
                            _ptr(h_out), _ptr(None if drop is None else _req(drop, torch.float32, "drop")), _stream()), "ghf_tail_fwd")
    return h_out


def _row_tables(tables):
    """(rows, extra or None, row bytes, extra bytes) of the one or two tables ghf_rows_pack / ghf_rows_unpack take."""
    if not 1 <= len(tables) <= 2:
        raise ValueError(f"rows_pack / rows_unpack take one or two tables, got {len(tables)}")
    rows = tables[0]
    extra = tables[1] if len(tables) > 1 else None
    return rows, extra, rows.size(1) * rows.element_size(), (extra.size(1) * extra.element_size() if extra is not None else 0)


def rows_pack(tables, idx: torch.Tensor) -> torch.Tensor:
    """The rows `idx` (int64, device) of one or two row-indexed byte tables ([N, row_bytes] uint8 views of one allocation each)
    as one contiguous message [n, row_bytes (+ extra_bytes)] uint8 — ghf_rows_pack."""
    rows, extra, rb, xb = _row_tables(tables)
    idx = _req(idx, torch.int64, "idx")
    out = torch.empty(idx.numel(), rb + xb, dtype=torch.uint8, device=rows.device)
    _check(load().ghf_rows_pack(_ptr(rows), rb, _ptr(extra), xb, _ptr(idx), idx.numel(), rows.size(0), _ptr(out), _stream()), "ghf_rows_pack")
    return out


def rows_unpack(tables, idx: torch.Tensor, packed: torch.Tensor) -> None:
    """ghf_rows_unpack: a received message back to the rows' places in the same tables."""
    rows, extra, rb, xb = _row_tables(tables)
    idx = _req(idx, torch.int64, "idx")
    if packed.numel() != idx.numel() * (rb + xb):
        raise ValueError(f"rows_unpack: message of {packed.numel()} bytes for {idx.numel()} rows of {rb + xb}")
    _check(load().ghf_rows_unpack(_ptr(packed), _ptr(idx), idx.numel(), rows.size(0), _ptr(rows), rb, _ptr(extra), xb, _stream()), "ghf_rows_unpack")


def rows_accumulate(rows: torch.Tensor, idx: Optional[torch.Tensor], packed: torch.Tensor, any_width: bool = False) -> torch.Tensor:
    """rows[idx[i]] += packed[i] in place (fp32 [nrows, d] and [n, d]; idx None = rows 0..n-1) — ghf_rows_accumulate, the
    adjoint of rows_unpack.  idx entries must be distinct; entries outside [0, nrows) are skipped.  `any_width`:
    ghf_rows_accumulate_any, which also takes a d that is no multiple of 4 (the same bits where d is one)."""
    if rows.dim() != 2 or not rows.is_contiguous() or rows.dtype != torch.float32:
        raise ValueError(f"rows_accumulate: rows must be a contiguous float32 [nrows, d] tensor, got {rows.dtype} {tuple(rows.shape)}")
    rows = _req(rows, torch.float32, "rows")
    nrows, d = rows.shape
    packed = _req(packed, torch.float32, "packed")
    if idx is not None:
        if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
            raise ValueError(f"rows_accumulate: idx must be a contiguous 1-D int64 tensor, got {idx.dtype} {tuple(idx.shape)}")
        if idx.device != rows.device:
            raise ValueError(f"rows_accumulate: idx lives on {idx.device}, rows on {rows.device}")
    n = idx.numel() if idx is not None else packed.numel() // max(d, 1)
    if packed.device != rows.device or packed.numel() != n * d:
        raise ValueError(f"rows_accumulate: message of {packed.numel()} floats on {packed.device} for {n} rows of {d} on {rows.device}")
    if any_width:
        _check(load().ghf_rows_accumulate_any(_ptr(packed), _ptr(idx), n, nrows, _ptr(rows), d, _stream()), "ghf_rows_accumulate_any")
        return rows
    _check(load().ghf_rows_accumulate(_ptr(packed), _ptr(idx), n, nrows, _ptr(rows), d, _stream()), "ghf_rows_accumulate")
    return rows

"""Torch-tensor front end of the C ABI: pointer extraction, shape checks, stream plumbing.

PyTorch is the memory container here and nothing else: every function hands raw device addresses (``tensor.data_ptr()``)
and the current HIP stream to libselfrec_hip.so.  One submodule per kernel family, all re-exported here: callers outside
the package say ``ops.<name>`` (the layout and the rule for a new model's wrappers)."""
from ._base import (NCE_WIDTHS, ROW_WIDTHS, SPMM_WIDTHS, TABLE_NCE_WIDTHS, LossGradFn, SelfrecHipError, SpmmEpilogue, _lib,
                    check, cut_cols, gpu_available, kernel_width, pad_cols, padded_width, require_gpu, to_width, u64, workspace)
from .au import AlignUniformFn, au_fwd_bwd, au_supported
from .boot import BootstrapLossFn, boot_fwd_bwd, boot_supported, rows_momentum
from .contrastive import (KMEANS_MAX_POINTS_PER_CENTROID, KMEANS_SPLIT_EPS, BatchSoftmaxFn, InfoNceFn, TableCeFn,
                          batch_softmax_fwd_bwd, kmeans, kmeans_assign, kmeans_split, kmeans_update, table_ce_fwd_bwd,
                          table_nce_fwd_bwd, table_nce_ws)
from .duo import DUO_WIDTHS, DuoNceFn, duo_nce_fwd_bwd, duo_supported
from .host import Sampler, find_k_largest_host, find_k_largest_host_f64, unique_first
from .knn import KNN_MAX_K, knn_neighbours, knn_score_topk, knn_score_ws
from .losses import (TRIPLET_MARGIN, KlDivFn, PairCeFn, SelfPairCeFn, TripletFn, kl_div_fwd_bwd, pair_ce_fwd_bwd,
                     triplet_fwd_bwd)
from .mhcn import GATE_MAX, ChanMixFn, GateFn, MimFn, chan_mix_bwd, chan_mix_fwd, gate_bwd, gate_fwd, mim_fwd_bwd
from .mixgcf import MIXUP_MAX_HOPS, MixupFn, mixup_bwd, mixup_fwd, mixup_supported
from .ranking import (gemm_nt, metric_rows, score_mask_topk, score_mask_topk_filtered, topk_hit_flags, topk_rows,
                      topk_trim_mark_ties)
from .rnn import (GRU_MAX_LEN, GRU_WIDTH, GatherLiveRowsFn, GruFn, gru_bwd, gru_fwd, gru_lengths, gru_pad_params,
                  gru_supported)
from .sept import (L2NORM_MAX_WIDTH, TRI_ND_MAX_K, NormPropFn, RowsL2NormFn, TriNdFn, rows_l2norm_bwd, rows_l2norm_fwd,
                   tri_nd_fwd_bwd)
from .seq import (LIVE_SUM_CHUNK, LIVE_SUM_MAX_PROBLEMS, SEQ_ATTN_HEAD_WIDTHS, SEQ_ATTN_MAX_LEN, SEQ_ATTN_MAX_WIDTH,
                  SEQ_EMBED_WIDTHS, GatherRowsFn, SeqAttnFn, SeqAttnFullFn, SeqBceFn, SeqBceLiveFn, SeqEmbedFn, live_plan,
                  live_plan_host, rows_live_sum, rows_segment_sum, scatter_plan, scatter_plan_host, seq_attn_bwd,
                  seq_attn_full_bwd, seq_attn_full_fwd, seq_attn_fwd, seq_attn_supported, seq_bce_fwd_bwd, seq_embed_fwd,
                  seq_embed_supported, SEQ_ATTN_TILED_MAX_LEN, SeqAttnTiledFn, seq_attn_tiled_bwd, seq_attn_tiled_fwd,
                  seq_attn_tiled_supported)
from .sparse import (ADAM_EPILOGUE, DeviceCSR, adj_sym_normalize, column_class_order, gather_floor_probe, make_epilogue,
                     spmm, spmm3, spmm_any, spmm_gather_bound, spmm_plan_run_tasks, spmm_probe, spmm_set_xcd_shares)
from .step import (NCE_DEFAULT, NCE_F32_MAX_N, NCE_PRECISIONS, adam_step, axpby, batch_fetch, batch_fetch_args, batch_lists,
                   batch_pack, batch_scatter, batch_unpack, bpr_bwd, bpr_fwd, bpr_infonce, bpr_l2_fwd_bwd, bpr_ws,
                   cursor_advance, get_infonce_precision, infonce_fwd_bwd, infonce_multi, infonce_plan, infonce_ws,
                   l2_reg_bwd, l2_reg_fwd, scalar_ws, _segments, set_infonce_precision, zero_rows)
from .tower import TOWER_HIDDEN, TOWER_IN, TOWER_OUT, TowerFn, tower_bwd, tower_fwd

__all__ = """
    SelfrecHipError gpu_available pad_cols padded_width LossGradFn Sampler find_k_largest_host find_k_largest_host_f64
    unique_first DeviceCSR column_class_order make_epilogue spmm spmm_any spmm3 spmm_probe spmm_set_xcd_shares
    spmm_plan_run_tasks spmm_gather_bound gather_floor_probe adj_sym_normalize bpr_ws bpr_l2_fwd_bwd scalar_ws bpr_fwd
    bpr_bwd l2_reg_fwd l2_reg_bwd set_infonce_precision get_infonce_precision infonce_plan infonce_ws infonce_fwd_bwd
    infonce_multi bpr_infonce adam_step axpby cursor_advance zero_rows batch_fetch_args batch_fetch batch_lists
    batch_pack batch_unpack batch_scatter score_mask_topk score_mask_topk_filtered topk_trim_mark_ties gemm_nt
    topk_rows topk_hit_flags metric_rows knn_neighbours knn_score_ws knn_score_topk table_nce_ws table_nce_fwd_bwd
    kmeans_assign kmeans_update kmeans_split kmeans batch_softmax_fwd_bwd BatchSoftmaxFn table_ce_fwd_bwd TableCeFn
    InfoNceFn tower_fwd tower_bwd TowerFn scatter_plan scatter_plan_host rows_segment_sum seq_attn_supported
    seq_attn_fwd seq_attn_bwd seq_attn_full_fwd seq_attn_full_bwd SeqAttnFn SeqAttnFullFn seq_bce_fwd_bwd SeqBceFn
    GatherRowsFn seq_embed_supported seq_embed_fwd live_plan_host live_plan rows_live_sum SeqEmbedFn SeqBceLiveFn
    rows_l2norm_fwd rows_l2norm_bwd NormPropFn RowsL2NormFn tri_nd_fwd_bwd TriNdFn gate_fwd gate_bwd GateFn
    chan_mix_fwd chan_mix_bwd ChanMixFn mim_fwd_bwd MimFn mixup_supported mixup_fwd mixup_bwd MixupFn au_supported au_fwd_bwd
    AlignUniformFn boot_supported boot_fwd_bwd BootstrapLossFn rows_momentum pair_ce_fwd_bwd PairCeFn SelfPairCeFn
    triplet_fwd_bwd TripletFn kl_div_fwd_bwd KlDivFn SEQ_ATTN_TILED_MAX_LEN seq_attn_tiled_supported seq_attn_tiled_fwd
    seq_attn_tiled_bwd SeqAttnTiledFn duo_supported duo_nce_fwd_bwd DuoNceFn GRU_WIDTH GRU_MAX_LEN gru_supported
    gru_lengths gru_fwd gru_bwd gru_pad_params GruFn GatherLiveRowsFn
""".split()

/*
 * selfrec_hip.h -- C ABI of libselfrec_hip.so, the MI355X (gfx950) engine behind SELFRec's
 * graph-recommender hot path.
 *
 * The reference (Coder-Yu/SELFRec) is pure Python: it has no FFI of its own.  The
 * "operator interface" it does have is a set of Python call sites inside its model
 * files; each entry point below is what a ctypes stub bound at that call site calls
 * (INTEGRATION.md shows the stubs).  Every declaration cites the reference interface it
 * replaces as  <file>:<lines>  relative to the reference checkout.
 *
 * Conventions
 *   - plain C types only; no torch / C++ types cross this boundary.
 *   - pointers named d_*  are raw DEVICE addresses on the current HIP device,
 *     pointers named h_*  are HOST addresses.  All buffers are caller-owned; the library
 *     allocates only the opaque handles it returns (freed by the matching *_destroy).
 *   - every device entry point is asynchronous on the `stream` argument (a hipStream_t
 *     passed as void*); none synchronises, none uses the null stream implicitly.
 *   - return value: SRH_OK (0) or a negative srh_status_t.  Nothing throws, nothing calls
 *     exit().  srh_last_error_string() describes the last failure on the calling thread.
 *   - row-major fp32 matrices with leading dimension == d unless stated.
 *   - handles are not thread-safe; distinct handles may be used from distinct threads.
 */
#ifndef SELFREC_HIP_H
#define SELFREC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t srh_status_t;
enum {
  SRH_OK = 0,
  SRH_ERR_INVALID_ARG = -1,
  SRH_ERR_HIP = -2,
  SRH_ERR_UNSUPPORTED = -3,
  SRH_ERR_NOMEM = -4,
  SRH_ERR_STATE = -5
};

/* ABI version: bumped whenever a signature or struct below changes. */
#define SRH_ABI_VERSION 31
int32_t srh_abi_version(void);
const char* srh_last_error_string(void);
/* Number of visible HIP devices (0 when there is none -- never an error). */
int32_t srh_device_count(void);

/* ------------------------------------------------------------------------------------
 * (a-1) Pairwise sampler -- replaces util/sampler.py:5-28  next_batch_pairwise(data, B, n_negs)
 *
 * Host-side, bit-exact replay of the CPython `random` stream the reference consumes:
 * MT19937 words -> getrandbits(k) -> _randbelow(n) -> shuffle / choice with set rejection.
 * The handle keeps the persistent order of data.training_data across epochs (the
 * reference shuffles that shared list in place, sampler.py:7).
 * ---------------------------------------------------------------------------------- */
typedef struct srh_sampler srh_sampler_t;

/* h_edge_user/h_edge_item: the id columns of training_data in its CURRENT order
 * (ids as assigned by data/ui_graph.py:29-38).  Copied. */
srh_status_t srh_sampler_create(srh_sampler_t** out, int64_t n_users, int64_t n_items,
                                int64_t n_edges, const int32_t* h_edge_user,
                                const int32_t* h_edge_item);
void srh_sampler_destroy(srh_sampler_t* s);
/* MT19937 state exactly as random.getstate()[1]: 624 words followed by the position. */
srh_status_t srh_sampler_set_state(srh_sampler_t* s, const uint32_t* h_mt624, int32_t pos);
srh_status_t srh_sampler_get_state(const srh_sampler_t* s, uint32_t* h_mt624, int32_t* pos);
/* random.seed(int) for 0 <= seed < 2^64 (CPython init_by_array on the 32-bit limbs). */
srh_status_t srh_sampler_seed(srh_sampler_t* s, uint64_t seed);
/* random.shuffle(training_data): one Fisher-Yates pass over the persistent order. */
srh_status_t srh_sampler_shuffle(srh_sampler_t* s);
/* Current order: h_perm[p] = index into the edge arrays given at create time. */
srh_status_t srh_sampler_get_order(const srh_sampler_t* s, int64_t* h_perm);
/* One batch: positions [ptr, ptr+count) of the current order; writes count users, count
 * positives and count*n_negs negatives.  *out_count receives count
 * (= min(batch_size, n_edges-ptr), sampler.py:10-14).  */
srh_status_t srh_sampler_next_batch(srh_sampler_t* s, int64_t ptr, int64_t batch_size,
                                    int32_t n_negs, int32_t* h_u, int32_t* h_i, int32_t* h_j,
                                    int64_t* out_count);
/* A whole epoch = shuffle + every batch, contiguous: h_u/h_i hold n_edges ids, h_j holds
 * n_edges*n_negs.  When h_uniq_u/h_uniq_i are non-NULL they receive, per batch b, the
 * sorted unique user / positive-item ids (torch.unique at XSimGCL.py:46-47) at offset
 * b*batch_size, with the counts in h_n_uniq_u[b] / h_n_uniq_i[b]. */
srh_status_t srh_sampler_epoch(srh_sampler_t* s, int64_t batch_size, int32_t n_negs,
                               int32_t* h_u, int32_t* h_i, int32_t* h_j,
                               int32_t* h_uniq_u, int32_t* h_n_uniq_u,
                               int32_t* h_uniq_i, int32_t* h_n_uniq_i);
/* The row -> slot lists of every batch of an epoch: what lets the batch gradients of XSimGCL.py:30-37 (emb[idx] gathers whose
 * autograd is a scatter-ADD: a user / item that occurs in several pairs of a batch receives several contributions) be summed in
 * ONE FIXED ORDER by one row group each, without float atomics -- a training step is then reproducible bit for bit, like the
 * reference's single-threaded CPU step.  Host only, no draw from the generator; inputs are srh_sampler_epoch's outputs (ids).
 * Per batch b (cnt pairs), the ROW GROUPS are numbered
 *     [0, nuu)                 the sorted unique users                    (h_uniq_u)
 *     [nuu, nuu + nui)         the sorted unique positive items           (h_uniq_i)
 *     [nuu + nui, groups)      the sorted unique negatives that are nobody's positive in this batch (count: h_n_uniq_n[b])
 * h_seg_rows[b 3B + g] = the group's TABLE ROW (id + user_row0 for users, id + item_row0 for items: pass 0, n_users when
 * the items follow the users in one table; -1 for g >= groups), and group g owns entries [h_seg_end[b 3B + g - 1] (0 for
 * g = 0), h_seg_end[b 3B + g]) of the entry arrays at b 3B, slots ascending inside a group:
 *     h_seg[e]   = 4 * slot + role   (role 0: the slot's user, 1: its positive item, 2: its negative item)
 *     h_seg_a[e] = the table row the term needs: the slot's positive item (role 0), its user (roles 1, 2)
 *     h_seg_b[b B + e] = the slot's negative item's table row (role 0 entries: they are the first cnt entries of a batch)
 * Sizes: h_n_uniq_n nb; h_seg_rows / h_seg_end / h_seg / h_seg_a nb * 3 B; h_seg_b nb * B   (nb = ceil(n_edges / B)). */
srh_status_t srh_sampler_epoch_segments(srh_sampler_t* s, int64_t batch_size, const int32_t* h_u, const int32_t* h_i,
                                        const int32_t* h_j, const int32_t* h_uniq_u, const int32_t* h_n_uniq_u,
                                        const int32_t* h_uniq_i, const int32_t* h_n_uniq_i, int32_t user_row0,
                                        int32_t item_row0, int32_t* h_n_uniq_n, int32_t* h_seg_rows, int32_t* h_seg_end,
                                        int32_t* h_seg, int32_t* h_seg_a, int32_t* h_seg_b);
/* random.sample(range(n), k) (data/augmentor.py:35 edge_dropout keep-set; :15-16 node
 * dropout) replayed on the sampler's MT stream.  h_out receives k indices in draw order. */
srh_status_t srh_sampler_sample_range(srh_sampler_t* s, int64_t n, int64_t k, int64_t* h_out);
/* random.getrandbits(32) -- lets tests pin how much of the stream was consumed. */
srh_status_t srh_sampler_next_u32(srh_sampler_t* s, uint32_t* out);

/* find_k_largest(K, candidates) of reference util/algorithm.py:144-156 on the host, with the reference's order among EQUAL
 * scores: python's heapq on (score, position) tuples restated step for step (heapify, heapreplace on a strictly larger score,
 * a stable descending sort of the heap array).  The device ranking orders ties (score desc, id asc); base/graph_recommender.py
 * redoes the rows whose best K + 1 scores hold a tie through this call.  *out_count = min(K, n) entries written. */
srh_status_t srh_find_k_largest_host(int64_t k, const float* h_candidates, int64_t n, int64_t* h_out_ids,
                                     float* h_out_scores, int64_t* out_count);

/* The same walk for float64 candidates (UserKNN / ItemKNN scores: base/graph_recommender.py:47-51 on predict()'s
 * float64 row). */
srh_status_t srh_find_k_largest_host_f64(int64_t k, const double* h_candidates, int64_t n, int64_t* h_out_ids,
                                         double* h_out_scores, int64_t* out_count);

/* `torch.rand(n)` of the CPU generator (ATen: mt19937, one 32-bit word per float32, value = (word & 0xFFFFFF) * 2^-24),
 * replayed on the host from the generator's own words: what model/graph/BUIR.py:118-121 draws per forward pass for its
 * sparse dropout -- `torch.floor(keep_prob + torch.rand(nnz)).type(torch.bool)` -- at 5 M entries per step on the Yelp2018
 * shape, where ATen's serial kernel takes 15 ns per draw.  h_mt624 / *pos are the generator's 624 state words and the
 * index of the next unread word (624: regenerate first), in and out.  h_out (nullable) receives the n uniforms; h_keep
 * (nullable) receives floorf(keep_addend + u) != 0 as bytes, the fp32 arithmetic of the torch expression. */
srh_status_t srh_mt19937_uniform_f32(uint32_t* h_mt624, int32_t* pos, int64_t n, float* h_out,
                                     float keep_addend, uint8_t* h_keep);

/* ------------------------------------------------------------------------------------
 * (a-2) Graph normalisation -- replaces data/graph.py:10-24 normalize_graph_mat and
 * data/ui_graph.py:58-65 convert_to_laplacian_mat on a device-resident CSR.
 *
 * The (N x N) bipartite adjacency keeps ONE structure for the graph and all its
 * edge-dropped views; a view is a value array.  d_edge_id[p] is the position, in the
 * row-major order of the U x I interaction matrix, of the interaction behind non-zero p
 * (both the (u,i) and the (i,u) copies carry the same id), d_weight[p] its weight (NULL =
 * all ones), d_keep[e] != 0 keeps interaction e (NULL = keep all).
 * Output: d_vals[p] = keep ? (dinv[row] * w) * dinv[col] : 0 with
 * dinv[r] = (sum of kept weights in row r)^-1/2, 0 for an empty row -- the reference's
 * inf -> 0 rule (graph.py:15).  d_deg_ws: workspace of n_rows floats.
 * Row-sharded graphs (the CSR holds the rows [row_offset, row_offset + n_rows) of the node table and
 * its columns index the whole table): d_deg_ws covers the whole table, phase 1 only fills this
 * shard's dinv entries, the caller all-gathers d_deg_ws, phase 2 only writes the values.
 * phase 0 = both in one call (row_offset 0 for a whole graph).
 * d_inv_sqrt_table (optional, table_len entries): table[k] = float32(k)^-1/2 as the HOST's
 * numpy computes it; integral degrees below table_len are looked up there, which makes the
 * values bit-identical to the reference's np.power(rowsum, -0.5) (numpy's fp32 pow is not
 * correctly rounded, so no device formula can match it in every last bit).
 * n_rows < 2^31; each kernel is one launch up to 2^25 rows and one per 2^25 rows above (a launch
 * holds fewer than 2^32 work-items at one wave per row).
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_adj_sym_normalize(int64_t n_rows, const int32_t* d_indptr,
                                   const int32_t* d_indices, const int32_t* d_edge_id,
                                   const float* d_weight, const uint8_t* d_keep,
                                   const float* d_inv_sqrt_table, int32_t table_len,
                                   float* d_deg_ws, float* d_vals, int64_t row_offset, int32_t phase,
                                   void* stream);

/* ------------------------------------------------------------------------------------
 * (a-3, a-4) Sparse propagation -- replaces torch.sparse.mm(adj, dense) at
 * LightGCN.py:72, XSimGCL.py:88, SimGCL.py:85, SGL.py:104-108 (adj produced by
 * base/torch_interface.py:8-13), with the per-layer elementwise tail fused in:
 *   PERTURB : y += sign(y) * normalize(noise_row) * eps        XSimGCL.py:90-91
 *   MEAN    : mean_out = (sum_t prev[t] + y) / mean_div         XSimGCL.py:95-96, LightGCN.py:74-75
 *   AXPY    : y = alpha * y + sum_t add_scale[t] * add[t]       (backward accumulation; add[t] may alias y)
 *   FANOUT  : with PERTURB, the SAME product also leaves differently-perturbed copies     SimGCL.py:81-93
 *             (SimGCL's clean pass and its two perturbed views multiply the same A by the same
 *             ego table in their first layer: one gather pass, three outputs)
 *
 * The plan is the row schedule (degree-sorted rows, heavy rows split into segments); it
 * depends only on indptr and is shared by every value array over the same structure.
 * ---------------------------------------------------------------------------------- */
typedef struct srh_spmm_plan srh_spmm_plan_t;

/* xcd_split_row: 0, or the first row of the second node class of a bipartite adjacency (= number
 * of users): rows below it are issued to XCDs 0-3, the rest to XCDs 4-7 (L2 locality only).
 * h_row_mid: NULL, or per row: m >= 0 -- the caller ordered the row's entries [column class 0 | column
 * class 1] and class 1 starts at entry m: the two parts are scheduled as separate segments on different
 * XCDs (each L2 then caches one column class of one row class) and summed in-kernel; -1 - c -- the row
 * stays whole and runs with column class c.  Locality only: the product is the same. */
srh_status_t srh_spmm_plan_create(srh_spmm_plan_t** out, int64_t n_rows, int64_t n_cols,
                                  const int32_t* h_indptr, int32_t split_len /* 0 = default */,
                                  int64_t xcd_split_row, const int32_t* h_row_mid);

/* Unequal XCD shares of a plan's task list (tables of d = 64 / 128 / 256 columns).  A task list binds task k to
 * workgroup k / 4 and the hardware runs workgroup b on XCD b % 8 (observed, performance only), so every XCD gets the same
 * NUMBER of workgroups -- but not the same time over them: at the Yelp2018 shape the XCDs finish a propagation launch
 * 3.5 us apart.  h_blocks_per_xcd[8] (>= 0, adding up to ceil(srh_spmm_plan_run_tasks() / 4) of the canonical list)
 * says how many workgroups of real tasks each XCD runs; queues above their share give up their last workgroups (the
 * shortest rows), the others append them, and empty records pad the list.  NULL restores the canonical list.  Same
 * tasks, same sums bit for bit; locality / balance only.  Synchronises the device: not inside a stream capture, and a
 * captured launch of this plan must be re-captured afterwards.  The engine calibrates the shares once at start-up
 * from srh_spmm_f32_probe (engine.py). */
srh_status_t srh_spmm_plan_set_xcd_shares(srh_spmm_plan_t* plan, int32_t d, const int32_t* h_blocks_per_xcd);
/* records in the list a launch on d-column tables runs now (a multiple of 32 once shares are set); -1: no such list */
int32_t srh_spmm_plan_run_tasks(const srh_spmm_plan_t* plan, int32_t d);
void srh_spmm_plan_destroy(srh_spmm_plan_t* plan);

enum { SRH_EPI_PERTURB = 1, SRH_EPI_MEAN = 2, SRH_EPI_AXPY = 4, SRH_EPI_ADAM = 8 };
#define SRH_MAX_ADAM_CLEAR 4
#define SRH_MAX_PREV 8
#define SRH_MAX_ADD 2
#define SRH_MAX_EXTRA 2

typedef struct srh_spmm_epilogue {
  int32_t flags;               /* OR of SRH_EPI_* ; 0 = plain y = A x                      */
  float eps;                   /* PERTURB magnitude                                          */
  const float* d_noise;        /* PERTURB: U[0,1) noise (n_rows, d) to inject, or NULL       */
  uint64_t rng_seed;        /* PERTURB with d_noise == NULL: in-kernel counter RNG,           */
  uint64_t rng_offset;      /*   counter = (rng_offset + *d_rng_step * rng_stride */
  const int64_t* d_rng_step;/*              + row, lane-quad); d_rng_step may be NULL  */
  uint64_t rng_stride;
  int32_t n_prev;              /* MEAN: number of earlier layer tensors                      */
  int32_t n_add;               /* AXPY: number of addends                                    */
  const float* d_prev[SRH_MAX_PREV];
  float mean_div;              /* MEAN: divisor (number of tensors averaged)                 */
  float alpha;                 /* AXPY: scale of the product (use 1 for a plain add)         */
  float* d_mean_out;           /* MEAN: (n_rows, d) output                                   */
  const float* d_add[SRH_MAX_ADD];
  float add_scale[SRH_MAX_ADD];
  /* Activity marks (any epilogue): a row / column is live iff mark[i] == (int32)*d_mark_stamp.
   * d_row_mark: rows that are not live are skipped entirely (y, mean_out keep their old
   * content).  d_col_mark: entries whose column is not live are treated as zero (the caller
   * guarantees x is zero there).  NULL = everything live. */
  const int32_t* d_row_mark;
  const int32_t* d_col_mark;
  const int64_t* d_mark_stamp;
  /* AXPY: bit t of add_sparse_mask says addend t is zero on every row whose d_add_mark entry is not
   * live, so it is only read on live rows (the batch-row gradients gF / gCL of the backward chain). */
  const int32_t* d_add_mark;
  int32_t add_sparse_mask;
  /* FANOUT (PERTURB only, no MEAN): n_extra further outputs extra_out[k] = perturb_k(product), each
   * with its own injected noise (or NULL) / counter offset; main_clean != 0 leaves the main output y
   * unperturbed. */
  int32_t n_extra;
  int32_t main_clean;
  float* d_extra_out[SRH_MAX_EXTRA];
  const float* d_extra_noise[SRH_MAX_EXTRA];
  uint64_t extra_rng_offset[SRH_MAX_EXTRA];
  /* Column-sharded tables (multi-GPU): y / x / every epilogue tensor hold columns
   * [noise_col0, noise_col0 + d) of rows that are noise_d_full wide on the whole job (any supported d).
   * Only PERTURB cares: its unit vector is normalised over the WHOLE row (XSimGCL.py:90), so d_noise /
   * d_extra_noise are (n_rows, noise_d_full) and the counter RNG regenerates the other ranks' columns.
   * 0 = the rows are d wide (everything above). */
  int32_t noise_d_full;
  int32_t noise_col0;
  /* Row scaling (any epilogue; d = 64 / 128 / 256): with r = d_row_scale[row] (e.g. D^-1/2 of the adjacency),
   *   SRH_SCALE_IN    the product is multiplied by r before everything else  -- with d_vals == NULL (pattern matrix,
   *                   every stored entry = 1) and x = D^-1/2 x' this IS D^-1/2 A D^-1/2 x' (graph.py:10-24) without
   *                   streaming a value per entry;
   *   SRH_SCALE_OUT   y (and the FANOUT outputs) are STORED multiplied by r -- the next layer's pre-scaled input
   *                   (mean_out is not: it holds true values);
   *   bit t of prev_unscale_mask / add_rowscale_mask: MEAN's d_prev[t] is stored pre-scaled (multiply by 1 / r,
   *                   0 where r = 0) / AXPY's d_add[t] is multiplied by r.
   * Lets the engine keep layer outputs in the pre-scaled domain between products. */
  const float* d_row_scale;
  int32_t scale_flags;
  int32_t prev_unscale_mask;
  int32_t add_rowscale_mask;
  /* Any `embedding.size` (base/recommender.py:16): tables of d_valid columns are stored zero-padded to the next width
   * the kernels serve.  Zero columns stay zero through every product, AXPY and MEAN; PERTURB must only know that the
   * noise row (torch.rand_like(h) in XSimGCL.py:90: d_valid columns) ends at noise_d_valid, so that F.normalize runs
   * over those columns alone.  0 = every column of the (whole) row is valid.  Tables of >= 64 columns. */
  int32_t noise_d_valid;
  /* ADAM (d = 64 / 128 / 256, no PERTURB / MEAN / SCALE_OUT, no row marks; the launch is the LAST product of a backward
   * chain, torch.optim.Adam(...).step() of XSimGCL.py:25,37 folded into it): the finished row -- the product after
   * SCALE_IN and AXPY -- is d loss / d param[row].  It is NOT stored (d_y is not written); instead row `row` of
   * d_adam_param / d_adam_m / d_adam_v takes srh_adam_step's update, operation for operation, with this step's
   * {lr / (1 - beta1^t), sqrt(1 - beta2^t)} read from d_adam_coef (float[2]: srh_batch_fetch writes them, see
   * d_adam_coef there).  As in srh_adam_step_reset: rows whose d_adam_clear_mark entry equals (int32)*d_mark_stamp are
   * zeroed in the adam_n_clear tables d_adam_clear[] ((n_rows, d); they may be this launch's addends, they must not be
   * its x), and d_adam_cursor (int64[2], or NULL) is advanced by one batch / one step -- d_mark_stamp must then point at
   * a COPY of the step (srh_batch_fetch's d_now), since the cursor moves while the launch runs. */
  float* d_adam_param;
  float* d_adam_m;
  float* d_adam_v;
  const float* d_adam_coef;
  float adam_beta1, adam_beta2, adam_eps;
  int32_t adam_n_clear;
  const int32_t* d_adam_clear_mark;
  float* d_adam_clear[SRH_MAX_ADAM_CLEAR];
  int64_t* d_adam_cursor;
} srh_spmm_epilogue_t;
enum { SRH_SCALE_IN = 1, SRH_SCALE_OUT = 2 };

/* y (n_rows, d) = A (CSR, fp32 values, int32 structure) * x (n_cols, d); d in {8,16,32,64,128,256}
 * (8 and 16: the thin-table kernel of the column-sharded layout).
 * x and y must not alias.  epi may be NULL.  d_vals may be NULL for d >= 64: A is then the PATTERN of the structure
 * (all stored entries 1) -- no value stream; column marks are not combined with it.
 * A structure with no stored entry (indptr all zero) is served: y is zero rows with the epilogue applied, d_indices and
 * d_vals are never read and may be NULL (a zero-length device array has no address). */
srh_status_t srh_spmm_f32(const srh_spmm_plan_t* plan, const int32_t* d_indptr,
                          const int32_t* d_indices, const float* d_vals, const float* d_x,
                          float* d_y, int32_t d, const srh_spmm_epilogue_t* epi, void* stream);

/* y_v = A_v x for three value arrays over ONE structure in one traversal (the x rows are gathered once):
 * the first layer of SGL.py:104-108, where the full adjacency and its two edge-dropped views
 * (data/augmentor.py:29-40: same indptr / indices, dropped entries = 0) multiply the same ego table.
 * Bit-identical to three srh_spmm_f32 calls, whatever the three arrays hold: an entry may be zero in any of them, the
 * first included.  d = 64 only (SRH_ERR_UNSUPPORTED otherwise).  With no stored entry d_indices / d_vals* may be NULL. */
srh_status_t srh_spmm3_f32(const srh_spmm_plan_t* plan, const int32_t* d_indices, const float* d_vals0,
                           const float* d_vals1, const float* d_vals2, const float* d_x, float* d_y0,
                           float* d_y1, float* d_y2, int32_t d, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-5, a-6, a-7) Row gather + BPR + L2 regulariser, forward and backward in one call --
 * replaces  emb[idx]  (XSimGCL.py:30), util/loss_torch.py:6-10 bpr_loss and :18-22
 * l2_reg_loss, and their autograd.
 *
 * Batch rows b = 0..B-1:  u = U[u_idx[b]], p = I[i_idx[b]], n = I[j_idx[b]].
 *   bpr  = mean_b( -log(1e-5 + sigmoid(<u,p> - <u,n>)) )
 *   reg  = reg_coef * ( ||Ru||_F + ||Rp||_F [+ ||Rn||_F] ) / B_rows     (Frobenius, not squared)
 * where R* are the same gathered rows of the REG source tables (d_reg_user/d_reg_item;
 * pass the propagated tables for XSimGCL/SimGCL/SGL/MF, the ego tables for LightGCN,
 * LightGCN.py:25).  reg_coef already contains any extra /batch_size factor.
 * Gradients (d loss / d table rows, scaled by loss_scale) are ATOMICALLY ACCUMULATED into
 * d_g_user / d_g_item (the gradient w.r.t. d_user/d_item) and d_greg_user / d_greg_item
 * (w.r.t. the REG tables; may alias d_g_*).  d_losses[0] += bpr, d_losses[1] += reg
 * (double, caller zeroes).  d_n_rows: optional device int32 overriding B (graph replay).
 * d_ws: workspace of at least srh_bpr_ws_bytes(B) bytes.
 * (Float atomics make the low bits of a row that several pairs name depend on arrival order.  The struct forms below --
 * srh_bpr_l2_fwd_bwd_p, srh_bpr_infonce_fwd_bwd -- take the batch's row -> slot lists (srh_batch_segments_t) and sum
 * every row's contributions in slot order instead: bit-reproducible, no atomics.)
 * ---------------------------------------------------------------------------------- */
/* The batch's row groups and their slot lists on the DEVICE (srh_sampler_epoch_segments' arrays, uploaded).
 * d_batch_no == NULL: the arrays are this batch's slices and d_n_uniq_n its count.  d_batch_no != NULL (graph replay):
 * they are the EPOCH arrays and batch b = *d_batch_no lives at + b 3B (d_seg_b: + b B), d_n_uniq_n[b] (B = the problem's B). */
typedef struct srh_batch_segments {
  const int32_t* d_n_uniq_u;  /* device-side counts of the batch's unique users / positive items (srh_batch_fetch's d_meta[1], [2]) */
  const int32_t* d_n_uniq_i;
  const int32_t* d_n_uniq_n;
  const int32_t* d_seg_rows;
  const int32_t* d_seg_end;
  const int32_t* d_seg;
  const int32_t* d_seg_a;
  const int32_t* d_seg_b;
  const int32_t* d_batch_no;
  int32_t nce_rows;           /* how the InfoNCE problems of the same call name these rows (srh_bpr_infonce_fwd_bwd):
                                 0 none; 1: problem 0's row i is user group i, problem 1's row i is positive-item group i
                                 (XSimGCL.py:46-49, SimGCL.py:44-49); 2: problem 0's rows are [users ; positive items]
                                 (SGL.py:120-125).  Rows of a problem are then finished by the group that owns them. */
  int32_t rows_are_zero;      /* != 0: the caller guarantees that every row this batch names is ZERO in every gradient table
                                 of the call (the engine clears exactly those rows after every step): rows are stored, not
                                 read-added-stored -- one memory round trip less in a latency-bound launch */
} srh_batch_segments_t;
int64_t srh_bpr_ws_bytes(int64_t B);
srh_status_t srh_bpr_l2_fwd_bwd(const float* d_user, const float* d_item,
                                const float* d_reg_user, const float* d_reg_item,
                                const int32_t* d_u_idx, const int32_t* d_i_idx,
                                const int32_t* d_j_idx, int64_t B, const int32_t* d_n_rows,
                                int32_t d, float reg_coef, int32_t reg_include_neg,
                                float loss_scale, float* d_g_user, float* d_g_item,
                                float* d_greg_user, float* d_greg_item, double* d_losses,
                                void* d_ws, void* stream);

/* Plain (non-gathered) forms behind the op-level tier's loss functions (selfrec_amd/util/loss_torch.py: the signatures of
 * util/loss_torch.py:6-22).  Each call is ONE launch and leaves its scalar on the device as f32, the way the reference's
 * expression would: the last workgroup to finish (a ticket in d_scalar_ws) turns the double accumulators into the result.
 * d_scalar_ws: SRH_SCALAR_WS_BYTES bytes, zero before its first use; every call leaves it zero again (calls that share
 * one must be ordered on a stream).  The upstream gradient d_gout is a DEVICE scalar: no host synchronisation in a
 * backward pass. */
#define SRH_SCALAR_WS_BYTES 64
/* bpr_loss (loss_torch.py:6-10):  *d_loss = mean_b -log(1e-5 + sigmoid(u_b.p_b - u_b.n_b));  d_coef[b] = d loss / d (pos_b - neg_b) */
srh_status_t srh_bpr_fwd(const float* d_u, const float* d_p, const float* d_n, int64_t B,
                         int32_t d, void* d_scalar_ws, float* d_loss, float* d_coef /* B */,
                         void* stream);
srh_status_t srh_bpr_bwd(const float* d_u, const float* d_p, const float* d_n,
                         const float* d_coef, int64_t B, int32_t d, const float* d_gout,
                         float* d_gu, float* d_gp, float* d_gn, void* stream);
/* l2_reg_loss(reg, *embs) (loss_torch.py:18-22):  *d_loss = reg * sum_k ||x_k||_F / rows_k, summed left to right in f32;
 * d_norms[k] = ||x_k||_F (kept for the backward pass).  Backward: d_gx_k = x_k * (((*d_gout * reg) / rows_k) / ||x_k||),
 * zero where the norm is zero (torch.norm's subgradient).  1..4 blocks of rows per call; `blocks` is a HOST array. */
typedef struct srh_l2_block {
  const float* d_x; /* (rows, cols) contiguous f32 */
  int64_t rows;
  int64_t cols;
  float* d_gx;      /* backward only */
} srh_l2_block_t;
srh_status_t srh_l2_reg_fwd(const srh_l2_block_t* blocks, int32_t n_blocks, float reg, void* d_scalar_ws,
                            float* d_norms /* n_blocks */, float* d_loss, void* stream);
srh_status_t srh_l2_reg_bwd(const srh_l2_block_t* blocks, int32_t n_blocks, float reg, const float* d_norms,
                            const float* d_gout, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-8) InfoNCE forward + backward -- replaces util/loss_torch.py:35-50 InfoNCE(view1,
 * view2, temperature, b_cos=True) at XSimGCL.py:48-49, SimGCL.py:48-49, SGL.py:125.
 *
 *   v1 = normalize(V1[idx]), v2 = normalize(V2[idx])   (rows gathered when d_idx != NULL)
 *   S = v1 v2^T / tau ;  loss = -mean_i log_softmax(S, dim=1)[i,i]
 * S (n x n) is never materialised: one flash-style pass over row tiles produces the row
 * log-sum-exp and dL/dv1, a second pass over column tiles produces dL/dv2; the
 * normalisation backward and the scatter to the source rows are fused in the last pass.
 * d_loss[0] += loss_scale * loss (double).  Gradients scaled by loss_scale are ADDED to
 * rows idx of d_g1 / d_g2 (row i when d_idx == NULL; idx must then be unique per call).
 * d_n: optional device int32 overriding n.  d_ws >= srh_infonce_ws_bytes(n, d) bytes.
 * ---------------------------------------------------------------------------------- */
int64_t srh_infonce_ws_bytes(int64_t n, int32_t d);
srh_status_t srh_infonce_fwd_bwd(const float* d_v1, const float* d_v2, const int32_t* d_idx,
                                 int64_t n, const int32_t* d_n, int32_t d, float tau,
                                 float loss_scale, double* d_loss, float* d_g1, float* d_g2,
                                 void* d_ws, void* stream);

/* Several InfoNCE problems in one set of launches (XSimGCL's user side and item side share every
 * kernel: half the launches, twice the resident waves).  d_ws must hold the SUM of
 * srh_infonce_ws_bytes(problems[k].n, d); at most 4 problems per call.  `problems` is a HOST array. */
typedef struct srh_infonce_problem {
  const float* d_v1;
  const float* d_v2;
  const int32_t* d_idx;
  int64_t n;
  const int32_t* d_n;
  float* d_g1;
  float* d_g2;
  int32_t g2_exclusive; /* != 0: the rows of d_g2 this problem names are written by nobody else during the call (e.g. the
                           contrast-layer gradient table of XSimGCL: user-side and item-side problems name disjoint rows):
                           plain read-add-store instead of 4 device-scope atomics per lane */
} srh_infonce_problem_t;
/* precision: SRH_NCE_SPLIT16 / SRH_NCE_F32 for THIS call, or SRH_NCE_DEFAULT (the process default below). */
srh_status_t srh_infonce_fwd_bwd_multi(const srh_infonce_problem_t* problems, int32_t n_problems,
                                       int32_t d, float tau, float loss_scale, double* d_loss,
                                       void* d_ws, int32_t precision, void* stream);

/* Arithmetic of InfoNCE's two n x n x d products (util/loss_torch.py:46-47's matmul and its backward).  The reference
 * computes them in fp32, and so does the DEFAULT here (SRH_NCE_F32): every multiply-add on v_mfma_f32_16x16x4_f32 (exact
 * f32 fma chains), d = 64 / 128 (d = 256 resolves to the split mode).  SRH_NCE_SPLIT16 is the faster opt-in: operands
 * carried as short sums of 16-bit pieces on the 16-bit MFMA pipe with f32 accumulation -- the similarity product on scaled
 * f16 hi + lo (x to 2^-22: logits as accurate as an f32 dot product), the P.V product on bf16 hi + mid (2^-18 per product;
 * gradients within 1e-6 relative of the f64 expression).  The mode is an ARGUMENT of srh_infonce_fwd_bwd_multi /
 * srh_bpr_infonce_fwd_bwd (a trainer carries its own: two models in one process do not share it);
 * srh_infonce_set_precision sets the process DEFAULT that SRH_NCE_DEFAULT and srh_infonce_fwd_bwd resolve to, and the
 * environment variable SRH_NCE_SPLIT16 (set to anything) selects the split mode as its initial value.  (SRH_NCE_SPLIT_BF16:
 * the mode's name in ABI <= 20.) */
#define SRH_NCE_SPLIT16 0
#define SRH_NCE_SPLIT_BF16 SRH_NCE_SPLIT16
#define SRH_NCE_F32 1
#define SRH_NCE_DEFAULT (-1)
srh_status_t srh_infonce_set_precision(int32_t mode);
int32_t srh_infonce_get_precision(void);

/* How the SRH_NCE_F32 passes cut `count` (1..4) problems of n[k] live rows into tasks on `slots` persistent workgroups (one
 * per compute unit in a call).  HOST ONLY: launches nothing, needs no device.  out17 receives the record the passes read,
 * 17 int32: n[4], per[4] (32-key blocks per task), splits[4] (key ranges per 128-row query block), first[5] (running task
 * count; first[4] = tasks in all).  per <= 128 and splits <= 16 for every n <= 65536; larger n: SRH_ERR_UNSUPPORTED. */
srh_status_t srh_infonce_plan(const int32_t* n, int32_t count, int32_t slots, int32_t* out17);

/* The whole batch objective of XSimGCL.py:30-35 / SimGCL.py:33-36 / SGL.py:33-37 --
 *   rec_loss + l2_reg_loss + cl_rate * cl_loss  and its gradients w.r.t. the gathered tables --
 * in one call: exactly srh_bpr_l2_fwd_bwd(bpr...) followed by srh_infonce_fwd_bwd_multi(problems...),
 * with the same outputs, but the two losses' O(batch) kernels share launches (4 instead of 6).
 * `bpr` mirrors the argument list of srh_bpr_l2_fwd_bwd; both structs are HOST memory. */
typedef struct srh_bpr_problem {
  const float* d_user;
  const float* d_item;
  const float* d_reg_user;
  const float* d_reg_item;
  const int32_t* d_u_idx;
  const int32_t* d_i_idx;
  const int32_t* d_j_idx;
  int64_t B;
  const int32_t* d_n_rows;
  float reg_coef;
  int32_t reg_include_neg;
  float loss_scale;
  float* d_g_user;
  float* d_g_item;
  float* d_greg_user;
  float* d_greg_item;
  double* d_losses;
  void* d_ws; /* srh_bpr_ws_bytes(B) */
  const srh_batch_segments_t* seg; /* HOST pointer or NULL.  Given: every touched row of the gradient tables is written by the
                                      ONE row group that owns it -- read, add the row's contributions in slot order (and the
                                      InfoNCE gradients of that row: nce_rows), store -- no float atomics: the same bits on
                                      every run.  The lists hold TABLE ROWS: user rows index d_user / d_reg_user / d_g_user /
                                      d_greg_user, item rows the item tables (two tables with ids, or one table passed for
                                      both with the items offset: user_row0 / item_row0 of srh_sampler_epoch_segments); an
                                      InfoNCE problem's d_idx must name the same rows of ITS tables.  User rows and item rows
                                      must not alias.  NULL: atomic accumulation as srh_bpr_l2_fwd_bwd describes. */
} srh_bpr_problem_t;
/* srh_bpr_l2_fwd_bwd with its arguments in the struct (and the optional fixed-order reduction of `seg`). */
srh_status_t srh_bpr_l2_fwd_bwd_p(const srh_bpr_problem_t* bpr, int32_t d, void* stream);
srh_status_t srh_bpr_infonce_fwd_bwd(const srh_bpr_problem_t* bpr, const srh_infonce_problem_t* problems,
                                     int32_t n_problems, int32_t d, float tau, float cl_scale,
                                     double* d_cl_loss, void* d_nce_ws, int32_t precision, void* stream);
/* The same call for a step whose views were staged by the caller's product (srh_spmm_f32_with_nce_stage on the same
 * problems, d and d_nce_ws, earlier on the stream): one launch fewer.  All-f32 arithmetic (SRH_NCE_F32), d = 64 / 128.  The
 * first InfoNCE pass gathers and normalises its own query rows (the same bits the prep kernel stores) and carries the BPR
 * scores at the end of its grid; losses and gradients are bit for bit those of srh_bpr_infonce_fwd_bwd at SRH_NCE_F32. */
srh_status_t srh_bpr_infonce_fwd_bwd_staged(const srh_bpr_problem_t* bpr, const srh_infonce_problem_t* problems,
                                            int32_t n_problems, int32_t d, float tau, float cl_scale,
                                            double* d_cl_loss, void* d_nce_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-9) Dense Adam -- replaces torch.optim.Adam(...).step() at XSimGCL.py:25,37
 * (betas, eps as given; no weight decay; bias-corrected).  `step` is 1-based; when
 * d_step != NULL the step count is read from that device int64 (graph replay).
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_adam_step(float* d_param, const float* d_grad, float* d_m, float* d_v,
                           int64_t n_elem, int64_t step, const int64_t* d_step, float lr,
                           float beta1, float beta2, float eps, void* stream);
/* The same update of an (n_rows, d) table as the LAST kernel of the engine's step: rows whose activity mark
 * d_row_mark[row] equals *d_step are zeroed in up to SRH_MAX_ADAM_CLEAR other (n_rows, d) tables in the same pass
 * (the batch-sparse gradient buffers: optimizer.zero_grad() of XSimGCL.py:35 for the only rows that are non-zero),
 * and d_cursor_advance (int64[2], optional) is incremented.  d_step must then be srh_batch_fetch's d_now copy, not
 * the cursor itself.  A table to clear may be d_grad (MF: the gradient buffer is the batch-sparse one). */
srh_status_t srh_adam_step_reset(float* d_param, const float* d_grad, float* d_m, float* d_v, int64_t n_rows,
                                 int32_t d, const int64_t* d_step, float lr, float beta1, float beta2, float eps,
                                 const int32_t* d_row_mark, int32_t n_clear, float* const* d_clear_tables,
                                 int64_t* d_cursor_advance, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-10, a-11) Full-catalogue scoring + training-item mask + top-K -- replaces the per
 * user loop of base/graph_recommender.py:46-53 (predict = XSimGCL.py:57-60, mask = -10e8,
 * util/algorithm.py:144-156 find_k_largest).
 *
 *   scores[r, :] = item_emb @ user_emb[user_ids[r]]       fp32 MFMA (exact-f32 fma chain)
 *   scores[r, i] = -1e9 for i in training items of that user (CSR d_r_indptr/d_r_indices)
 *   top-K by (score desc, id asc), written best-first.
 * d_scores_ws: (ws_rows, n_items) fp32 scratch; the queries pass through it ws_rows at a time (size
 * it to stay cache-resident: <= ~96 MB).  d_user_ids may be NULL (rows 0..n_query-1 of d_user_emb).
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_score_mask_topk(const float* d_user_emb, const int32_t* d_user_ids,
                                 int64_t n_query, const float* d_item_emb, int64_t n_items,
                                 int32_t d, const int32_t* d_r_indptr, const int32_t* d_r_indices,
                                 int32_t k, float* d_scores_ws, int64_t ws_rows, int32_t* d_out_ids,
                                 float* d_out_scores, void* stream);
/* The same ranking without ever storing the (users x items) scores.  Per chunk of chunk_rows users:
 *   1. the exact pipeline above on the first `sample_items` items only; its K-th score t_u is a lower
 *      bound of user u's overall K-th score;
 *   2. the scoring GEMM over the whole catalogue with a filter epilogue: a score is kept iff it is
 *      >= t_u -- a few hundred (item, score) pairs per user, appended to a list of `cap` slots;
 *   3. training items of u are dropped from its list (binary search in the mask CSR) and the rest is
 *      put in exact (score desc, id asc) order.
 *   d = 64 / 128: passes 1 and 2 only have to DECIDE, so they run on bf16 operands (one v_mfma_f32_32x32x16_bf16 per 16
 *   dimensions: 16x the f32 MFMA's rate) against rigorous PER-ITEM error bounds: |s~_uj - s_uj| <= delta_uj = 3.94e-3 |u| |i_j|
 *   (both operands rounded to bf16).  Pass 1 ranks LOWER bounds s~ - delta of the sample's scores, so t_u is a lower bound of
 *   the exact K-th best; pass 2 keeps (id, s~) with s~ + delta >= t_u; pass 3 takes tau = the K-th largest s~ - delta of the
 *   unmasked survivors and re-scores exactly -- by the scalar fma chain that is bit-identical to the f32 MFMA's accumulation --
 *   the survivors with s~ + delta >= tau.  (Round 3: three split-bf16 products and one margin 4e-5 |u| max_j|i_j| per user.)
 *   In this path the bound slice of pass 1 is the `sample_items` items of LARGEST NORM, not the first ones: the item image is
 *   built in norm order (norms, one radix sort of (norm, id) pairs, the permutation and its inverse), a user's best scores sit
 *   on the items training has pushed outwards, and the K-th best over such a slice is a far tighter bound: 39 instead of 60
 *   survivors per user on trained tables (tools/sample_choice_probe.py).
 * Scores come from the same fma chain, so ids and scores are identical to srh_score_mask_topk.
 * d_out_counts[q] = number of survivors of row q, training items included: when it exceeds `cap`
 * (tie-heavy rows, users with thousands of training items) that row of the outputs is NOT valid and the caller ranks it with
 * srh_score_mask_topk.  Any k <= cap <= 4096 is served, small ones included: a row is ranked iff its count is <= cap, and a row
 * that is not ranked is not read either.  d_ws: srh_score_mask_topk_filtered_ws_bytes(chunk_rows, ...) bytes.
 * Shape constants measured on the Yelp2018 shape (profiles/r03_m_*): chunk_rows 16384 (larger chunks fill the chip: 4096 ->
 * 16384 users per chunk is +20 %), sample_items 3072 in norm order (2048 .. 4096 are within 3 % of each other on trained
 * tables; round 3, catalogue order: 4096), cap 1024.  In the split path, pass 1 derives t~_u as the K-th largest of 256 disjoint group maxima of
 * the masked sample scores (a lower bound of their K-th largest: K distinct items attain it).
 * The workspace, with A(x) = ceil(x / 256) * 256, rows = chunk_rows, padded = ceil(n_items / 32) * 32:
 *   every d:       A(4 rows sample_items) + 2 A(4 rows k) + 2 A(4 rows cap)      (bound slab, its ranked ids / scores, the survivor lists)
 *   d = 64 / 128:  + A(2 padded d) + A(2 rows d) + A(4 rows) + 6 A(4 padded) + A(the radix sort's scratch for n_items pairs)
 *                  (bf16 item image, bf16 query rows and their norms, item norms and the norm order, the sort library's own scratch)
 * srh_score_mask_topk_filtered_ws_bytes returns 0 if an argument is not positive; it needs no device. */
int64_t srh_score_mask_topk_filtered_ws_bytes(int64_t chunk_rows, int64_t sample_items, int32_t k, int32_t cap,
                                              int64_t n_items, int32_t d);
srh_status_t srh_score_mask_topk_filtered(const float* d_user_emb, const int32_t* d_user_ids, int64_t n_query,
                                          const float* d_item_emb, int64_t n_items, int32_t d,
                                          const int32_t* d_r_indptr, const int32_t* d_r_indices, int32_t k,
                                          int64_t sample_items, int32_t cap, int64_t chunk_rows, void* d_ws,
                                          int32_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts,
                                          void* stream);
/* (n_query, k1) ranked ids / scores (k1 = K + 1) -> their first K columns; a row in which two NEIGHBOURS of the K + 1 scores are
 * EQUAL is marked d_out_ids[row][0] = -1 - id: its order among the equal scores is the reference's heap walk's
 * (util/algorithm.py:144-156), which the caller restores on the host (srh_find_k_largest_host). */
srh_status_t srh_topk_trim_mark_ties(const int32_t* d_ids, const float* d_scores, int64_t n_query, int32_t k1,
                                     int32_t* d_out_ids, float* d_out_scores, void* stream);
/* The scoring GEMM alone: C (m, n) = A (m, d) B (n, d)^T, fp32 MFMA. */
srh_status_t srh_gemm_nt_f32(const float* d_a, const float* d_b, float* d_c, int64_t m,
                             int64_t n, int32_t d, void* stream);
/* Row-wise top-K of a (rows, n) fp32 matrix (ld = n). */
srh_status_t srh_topk_rows(const float* d_scores, int64_t rows, int64_t n, int32_t k,
                           int32_t* d_out_ids, float* d_out_scores, void* stream);

/* (f-3) Metric tail: d_flags[q*k + r] = 1 iff d_ids[q*k + r] is a test item of user d_user_ids[q]
 * (rows 0..n_query-1 when NULL), the membership test of util/evaluation.py:7-16 (hits) and :66-78
 * (NDCG).  d_t_indptr / d_t_indices: the test set as a (users x items) CSR with sorted columns. */
srh_status_t srh_topk_hit_flags(const int32_t* d_ids, int64_t n_query, int32_t k,
                                const int32_t* d_user_ids, const int32_t* d_t_indptr,
                                const int32_t* d_t_indices, uint8_t* d_flags, void* stream);
/* (f-3) Per-user figures of util/evaluation.py:7-16,66-78 from the hit flags, for up to 8 cut-offs N <= k at once:
 *   d_hits[c * n_query + q] = number of hits among the first cuts[c] ranked items of row q                (Metric.hits)
 *   d_ndcg[c * n_query + q] = DCG / IDCG of row q at cuts[c], accumulated exactly as Metric.NDCG does it: float64,
 *                             positions best first, gain table d_gains[pos] = 1 / log2(pos + 2) and ideal prefix sums
 *                             d_ideal[c * (k + 1) + min(|truth_q|, cuts[c])] as the HOST computed them (python's
 *                             math.log: passed in, not recomputed, so the quotients are the reference's bit for bit).
 * d_sizes[q] = |truth_q| (> 0).  cuts: host array.  The cross-user sums stay on the host (31.5 k adds). */
srh_status_t srh_metric_rows(const uint8_t* d_flags, const int32_t* d_sizes, int64_t n_query, int32_t k,
                             const int32_t* cuts, int32_t n_cuts, const double* d_gains, const double* d_ideal,
                             int32_t* d_hits, double* d_ndcg, void* stream);

/* ------------------------------------------------------------------------------------
 * Small device utilities used by the fused engine.
 * ---------------------------------------------------------------------------------- */
/* y = a*x + b*y   (elementwise, n_elem floats; y may be uninitialised when b == 0) */
srh_status_t srh_axpby(float a, const float* d_x, float b, float* d_y, int64_t n_elem, void* stream);
/* Batch cursor for graph replay.  d_cursor: int64[2] = {batch number within the epoch, optimiser
 * step (1-based)} in device memory.  srh_batch_fetch copies batch d_cursor[0] of the per-epoch index
 * arrays into fixed staging buffers and publishes its sizes (d_meta: int32[4] = {rows, n_uniq_u,
 * n_uniq_i, batch_no}); it only READS the cursor.  The cursor is advanced by the last kernel of the
 * step: srh_zero_rows(..., d_cursor_advance, ...) or srh_cursor_advance. */
typedef struct {
  const int32_t* d_epoch_u;        /* the epoch's sampled triples (srh_sampler_epoch, uploaded) */
  const int32_t* d_epoch_i;
  const int32_t* d_epoch_j;
  const int32_t* d_epoch_uniq_u;   /* optional: per-batch sorted unique ids + counts (all five together) */
  const int32_t* d_epoch_uniq_i;
  const int32_t* d_n_uniq_u;
  const int32_t* d_n_uniq_i;
  int64_t n_edges;
  int64_t batch_size;
  const int64_t* d_cursor;         /* [0] = batch no, [1] = adam step */
  int32_t* d_stage_u;
  int32_t* d_stage_i;
  int32_t* d_stage_j;
  int32_t* d_stage_uniq_u;
  int32_t* d_stage_uniq_i;
  int32_t* d_meta;
  int32_t* d_row_mark;             /* optional: mark[u] = mark[off+i] = mark[off+j] = step */
  int32_t mark_item_offset;
  int32_t cat_item_offset;
  double* d_zero4;                 /* optional: 4 loss accumulators cleared for the new step */
  int32_t* d_stage_cat;            /* optional (2*batch_size): [uniq users ; uniq items + cat_item_offset] */
  int32_t* d_n_cat;                /* optional: n_uniq_u + n_uniq_i */
  int64_t* d_now;                  /* optional int64[2]: copy of d_cursor taken by this launch -- what a kernel that runs
                                      CONCURRENTLY with the cursor advance (Adam beside srh_zero_rows) reads its step from */
  int64_t half_batches;            /* 0: the arrays hold one epoch.  nb > 0: they hold TWO epochs back to back, nb batch
                                      slots each (d_epoch_u/i/j and the unique-id lists: 2 nb batch_size entries, the counts:
                                      2 nb) -- batch no b >= nb is batch b - nb of the second: its rows are cut against
                                      n_edges with b - nb, its data sits at b.  The engine fills one half (a copy on its own
                                      stream) while the steps read the other: an epoch boundary costs a cursor write. */
  float* d_adam_coef;              /* optional float[2]: this step's Adam constants {adam_lr / (1 - adam_beta1^t),
                                      sqrt(1 - adam_beta2^t)}, t = d_cursor[1], computed in double as torch does -- what
                                      an SRH_EPI_ADAM product of the step reads (one pow per step, not one per wave) */
  float adam_lr, adam_beta1, adam_beta2;
} srh_batch_fetch_args_t;
srh_status_t srh_batch_fetch(const srh_batch_fetch_args_t* args, void* stream);
/* srh_spmm_f32 for d = 64, 128, 256 (no column marks) that ALSO performs srh_batch_fetch(fetch): eight more workgroups at
 * the head of the same launch.  For a step whose first product does not depend on the batch (every model here: the
 * batch only enters at the last forward layer's row marks and at the losses) this removes a 5 us launch from the
 * step's critical path.  The product must not read anything the fetch writes (row marks, staged ids). */
srh_status_t srh_spmm_f32_with_fetch(const srh_spmm_plan_t* plan, const int32_t* d_indptr, const int32_t* d_indices,
                                     const float* d_vals, const float* d_x, float* d_y, int32_t d,
                                     const srh_spmm_epilogue_t* epi, const srh_batch_fetch_args_t* fetch, void* stream);
/* srh_spmm_f32 for d = 64 / 128 whose launch ALSO stages what the all-f32 InfoNCE passes of `problems` need before their
 * first launch and that depends on nothing later than the key-side tables d_v2: the gathered, normalised key-side view and
 * its norms, the armed arrival counters and loss-partial slots, and the step's task plan (cut from the live counts *d_n) --
 * rider workgroups (a multiple of 8) at the head of the launch, in d_nce_ws as srh_bpr_infonce_fwd_bwd lays it out.
 * problems / n_problems / d / d_nce_ws: exactly what the step later hands to srh_bpr_infonce_fwd_bwd_staged (d_v1, d_g1 and
 * d_g2 are not touched here).  The product must not write a d_v2 table (reading one is fine: the riders only read it), the
 * batch's d_idx / d_n must be staged by an EARLIER launch, and nothing between this launch and the staged loss call may
 * write d_nce_ws.  Not on an SRH_EPI_ADAM launch. */
srh_status_t srh_spmm_f32_with_nce_stage(const srh_spmm_plan_t* plan, const int32_t* d_indptr, const int32_t* d_indices,
                                         const float* d_vals, const float* d_x, float* d_y, int32_t d,
                                         const srh_spmm_epilogue_t* epi, const srh_infonce_problem_t* problems,
                                         int32_t n_problems, void* d_nce_ws, void* stream);

/* srh_spmm_f32 (no column marks, d = 64 / 128 / 256) that also leaves, for task k of the list, d_stamps[3k .. 3k+2] =
 * {begin, end} of its wave on the chip-wide 100 MHz clock and the XCD (0 .. 7) it ran on; records of tasks that do not
 * exist in the list stay untouched.  d_stamps: 3 * srh_spmm_plan_run_tasks(plan, d) uint64 of device memory.  What the
 * calibration of srh_spmm_plan_set_xcd_shares reads; tools/spmm_lab/run.py --probe draws timelines from it. */
srh_status_t srh_spmm_f32_probe(const srh_spmm_plan_t* plan, const int32_t* d_indices, const float* d_vals,
                                const float* d_x, float* d_y, int32_t d, const srh_spmm_epilogue_t* epi,
                                uint64_t* d_stamps, void* stream);
/* The propagation launch's own lower bound, measured (bench.py's roofline.gather_bound_us): the task list of `plan` for d-
 * column tables on its workgroup -> XCD placement, the (col) stream and the eight-in-flight gathers of x rows with their
 * multiply-adds -- and nothing after them: no values (pattern), no cross-group reduction, no split-row hand-off, no epilogue,
 * no y (d_scratch: one (d)-float row, never written for finite sums).  A strict subset of srh_spmm_f32's work on its schedule:
 * it cannot come out slower than the product it bounds.  The XSimGCL_Encoder.forward product it prices:
 * model/graph/XSimGCL.py:83-101.  d = 64 / 128 / 256.  Measurement only. */
srh_status_t srh_spmm_gather_bound(const srh_spmm_plan_t* plan, const int32_t* d_indices, const float* d_x, float* d_scratch,
                                   int32_t d, void* stream);
/* The bare gather stream of a propagation launch, for the roofline block of bench.py (the step's dominant
 * kernel is priced against HBM on ALGORITHMIC bytes; this probe says what the chip's vector-memory path needs for the row
 * fetches alone).  Walks d_indices[0 .. n_idx) -- the live graph's CSR column array, as data/ui_graph.py:47-56 orders it --
 * and fetches row d_indices[k] of the (n_x_rows, d) fp32 table d_x for every k, 8 fetches in flight per row-group, summing
 * into registers: no values, no epilogue, no output (d_sink: 16 bytes, never written for finite tables).  `blocks`
 * workgroups of 256 threads.  d = 64 / 128 / 256.  Replaces nothing in the reference: measurement only. */
srh_status_t srh_gather_floor_probe(const int32_t* d_indices, int64_t n_idx, const float* d_x, int64_t n_x_rows, int32_t d,
                                    int32_t blocks, float* d_sink, void* stream);
/* Zero the listed rows of up to SRH_MAX_ZERO_LISTS (rows, d) tables in one launch: rows
 * d_idx[k][0 .. count_k) + row_offset[k] of d_tables[k], count_k = *d_counts[k] (or n_max[k] when
 * d_counts[k] is NULL).  The sparse counterpart of a memset for gradient buffers that only
 * ever receive O(batch) non-zero rows.  Array arguments are HOST arrays of device pointers. */
#define SRH_MAX_ZERO_LISTS 8
srh_status_t srh_zero_rows(int32_t n_lists, float* const* d_tables, const int32_t* const* d_idx,
                           const int32_t* const* d_counts, const int32_t* n_max,
                           const int32_t* row_offset, int32_t d,
                           int64_t* d_cursor_advance /* optional: {batch, step} += 1 */, void* stream);
srh_status_t srh_cursor_advance(int64_t* d_cursor, void* stream);

/* ------------------------------------------------------------------------------------
 * (e) Column-sharded tables -- the multi-GPU layout for graphs that fit one GPU (DESIGN.md
 * section 6).  Rank r keeps columns [r*dl, (r+1)*dl) of every (N, d) table, dl = d / G.  Propagation
 * (LightGCN.py:72, XSimGCL.py:88) is independent per column: no exchange.  The losses
 * (XSimGCL.py:30-33,45-50; loss_torch.py:6-10,18-22,35-50) read whole rows, but only O(batch) of
 * them: the rows the staged batch lists name.  Those are exchanged by ONE all-gather per step:
 *   srh_batch_pack -> all-gather (host: RCCL) -> srh_batch_unpack -> the loss kernels above on the
 *   "compact" (5B, d) tables with the constant index lists slot -> slot -> srh_batch_scatter.
 * Compact row k = slot k of [u | i | j | unique users | unique items] (B slots each; slots past a
 * list's device-side count are dead: never written, never read).
 * ------------------------------------------------------------------------------------ */
#define SRH_MAX_EXCHANGE 8
typedef struct srh_batch_lists {
  const int32_t* d_idx[5];     /* staged lists of srh_batch_fetch: u, i, j, uniq_u, uniq_i (table rows)  */
  const int32_t* d_count[5];   /* device-side live counts (d_meta[0] for u/i/j, [1], [2]); NULL = B      */
  int32_t B;                   /* slots per list                                                         */
} srh_batch_lists_t;
/* d_send (n_tables, 5B, dl): the listed rows of each local (N, dl) table (dead slots: zeros).
 * d_cat_idx / d_n_cat (optional, 2B / 1): compact slots of [unique users ; unique items] as one list
 * (SGL.py:120-125 concatenates the two sides). */
srh_status_t srh_batch_pack(const srh_batch_lists_t* lists, int32_t n_tables, const float* const* d_tables,
                            int32_t dl, float* d_send, int32_t* d_cat_idx, int32_t* d_n_cat, void* stream);
/* d_recv (world, n_tables, 5B, dl) = all-gather of every rank's d_send -> d_compact[t] (5B, world*dl);
 * the live rows of the n_grads compact gradient tables are zeroed. */
srh_status_t srh_batch_unpack(const srh_batch_lists_t* lists, int32_t n_tables, int32_t world, int32_t dl,
                              const float* d_recv, float* const* d_compact, int32_t n_grads,
                              float* const* d_compact_grads, void* stream);
/* d_local_grads[p][node, :] += d_compact_grads[p][slot, col0 : col0 + dl] for every live slot. */
srh_status_t srh_batch_scatter(const srh_batch_lists_t* lists, int32_t n_pairs, const float* const* d_compact_grads,
                               float* const* d_local_grads, int32_t d_full, int32_t col0, int32_t dl, void* stream);

/* ------------------------------------------------------------------------------------
 * (e) Row-sharded tables -- SURVEY 8e's partition: rank r owns n rows of every (N, d) table (and the CSR rows of its nodes),
 * tables are kept in all-gather order (row = owner * n + local row).  The reference has one implicit device
 * (model/graph/XSimGCL.py:24,73); these are the exchanges its encoder (XSimGCL.py:83-101, one torch.sparse.mm per layer)
 * needs once the rows are dealt over N > 1 GPUs:
 *   forward,  before layer k:  srh_allgather_rows      every rank's (n, d) slice of E^(k-1) -> the whole (world n, d) table
 *   backward, after  layer k:  srh_reducescatter_rows  every rank's partial sums over ALL rows -> the owners' (n, d) slices
 *   (A_hat is symmetric: a backward product written by owners needs only the all-gather; the reduce-scatter serves
 *   formulations that produce partial rows.)  srh_allreduce_sum_f32: the dense gradient of the data-parallel layout.
 * Thin wrappers over RCCL (ncclAllGather / ncclReduceScatter / ncclAllReduce on ncclFloat32), asynchronous on `stream`.
 * `comm` is an ncclComm_t passed as void*: made by srh_comm_init_rank, or the caller's own.  RCCL is not linked -- the
 * symbols are resolved among what the process has loaded (then librccl.so.1), so the caller's copy of RCCL is the one
 * used.  Without RCCL every call returns SRH_ERR_UNSUPPORTED with a message.  In-place is allowed where RCCL allows it
 * (d_rows == d_table + rank * n * d).
 * ---------------------------------------------------------------------------------- */
#define SRH_COMM_ID_BYTES 128
/* rank 0 makes the id (ncclGetUniqueId), hands it to the others by any host channel; then every rank joins. */
srh_status_t srh_comm_unique_id(uint8_t* h_id /* SRH_COMM_ID_BYTES */);
srh_status_t srh_comm_init_rank(void** out_comm, int32_t world, int32_t rank, const uint8_t* h_id);
srh_status_t srh_comm_destroy(void* comm);
srh_status_t srh_comm_world(void* comm, int32_t* out_world);
srh_status_t srh_allgather_rows(const float* d_rows /* (n_rows, d) */, float* d_table /* (world n_rows, d) */,
                                int64_t n_rows, int32_t d, void* comm, void* stream);
srh_status_t srh_reducescatter_rows(const float* d_table /* (world n_rows, d) */, float* d_rows /* (n_rows, d) */,
                                    int64_t n_rows, int32_t d, void* comm, void* stream);
srh_status_t srh_allreduce_sum_f32(float* d_buf, int64_t n_elem, void* comm, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-12) Batch rows against a whole table: InfoNCE forward + backward -- replaces
 * model/graph/NCL.py:57-83 ssl_layer_loss (the user side and the item side, one problem each).
 *
 *   q_b = normalize(Q_b), t_j = normalize(T_j)              (F.normalize: x / max(|x|, 1e-12))
 *   loss = sum_b [ -q_b.t_idx[b] / tau + log sum_j exp(q_b.t_j / tau) ]   (a SUM over b)
 * Q (B x d): the gathered query rows (may repeat); T (N x d): the whole table; idx (B, int32):
 * the positive row of each query in T (may repeat).  The B x N logits are never materialised;
 * exponentials are taken as exp((s - 1) / tau) (unit rows: no running max needed).  Both
 * products of both passes run on the f32 MFMA.  No float atomics: the same bits on every call.
 * ENVELOPE: exp((s - 1) / tau) cannot overflow, but in f32 it is subnormal below cos = 1 - 87 tau
 * and 0 below 1 - 103 tau, where the reference's exp(s / tau) is still accurate.  Any data is safe
 * for tau >= 0.023 (exp(-2 / tau) is normal).  Below that, a query with no key above
 * cos = 1 - 87 tau has no usable row sum: when the sum is under N * 2^-130 (the subnormal terms'
 * errors of 2^-150 each may then exceed 2^-20 of it) that query's loss term is NaN, and so is
 * d_loss[0]; its gradient rows are not meaningful.  An idx outside [0, N) reads nothing and
 * makes the loss NaN as well; the d_gq rows of the other queries are unaffected by either.
 * Rows of norm below 1e-12 (zero rows included) follow F.normalize's clamp: x / 1e-12 forward,
 * g / 1e-12 backward.
 * Outputs are WRITTEN: d_loss[0] = loss_scale * loss (double), d_gq (B x d) = loss_scale *
 * dL/dQ, d_gt (N x d, dense) = loss_scale * dL/dT.  d = 64 or 128 (zero-pad narrower rows).
 * d_ws >= the SUM over problems of srh_table_nce_ws_bytes(B, N, d).  `problems` is a HOST
 * array of 1 or 2 problems.
 * ---------------------------------------------------------------------------------- */
typedef struct srh_table_nce_problem {
  const float* d_q;
  const float* d_t;
  const int32_t* d_idx;
  int64_t B;
  int64_t N;
  float loss_scale;
  double* d_loss;
  float* d_gq;
  float* d_gt;
} srh_table_nce_problem_t;
int64_t srh_table_nce_ws_bytes(int64_t B, int64_t N, int32_t d);
srh_status_t srh_table_nce_fwd_bwd(const srh_table_nce_problem_t* problems, int32_t n_problems,
                                   int32_t d, float tau, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-13) k-means steps on the device -- replace faiss.Kmeans(d, k).train(x) and
 * kmeans.index.search(x, 1) at model/graph/NCL.py:37-40 (run_kmeans, called by e_step).
 *
 * srh_kmeans_assign_f32: for each of the n rows of x (n x d), the nearest of the k centroids
 *   c (k x d) by |c_j|^2 - 2 x.c_j (f32 MFMA product with the argmin fused, no n x k matrix);
 *   ties go to the lowest j.  d_out_ids[i] = j, d_out_dist[i] = max(|x_i|^2 + that, 0).
 *   d = 64 or 128 (zero-pad narrower rows).
 * srh_kmeans_update_f32: per-cluster means and counts of the rows of x under d_ids (rows whose
 *   id is outside [0, k) are ignored).  Each cluster sums its rows in ascending row order
 *   after a stable counting sort, then multiplies by 1/count: the same bits on every call, no
 *   float atomics.  An empty cluster gets a zero centroid and count 0.  Any d >= 1.
 *   d_ws >= srh_kmeans_update_ws_bytes(n, k).
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_kmeans_assign_f32(const float* d_x, int64_t n, const float* d_c, int64_t k,
                                   int32_t d, int32_t* d_out_ids, float* d_out_dist, void* stream);
int64_t srh_kmeans_update_ws_bytes(int64_t n, int64_t k);
srh_status_t srh_kmeans_update_f32(const float* d_x, int64_t n, const int32_t* d_ids, int64_t k,
                                   int32_t d, float* d_out_centroids, int32_t* d_out_counts,
                                   void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-14) UserKNN / ItemKNN -- replace model/graph/UserKNN.py:32-57 / ItemKNN.py:32-56 (train: every row against every
 * other row in python) and :59-81 (predict), ranked as base/graph_recommender.py:44-58 ranks them.
 *
 * srh_knn_neighbours: rows of a binary matrix A (n_rows rows; d_a_* its CSR, d_t_* the transposed CSR with every row's
 *   entries ASCENDING).  For query row q (d_query_rows[i], or row i when NULL) and every other row v sharing n > 0
 *   features with it:
 *       sim = (n / (n + s)) * (n / (norm[q] * norm[v] + 1e-8))     (s = shrinkage, each operation a rounded f64 one)
 *   for any 0 <= s < 2^31: n + s is taken in f64, where it is exact, never in a 32-bit integer.
 *   d_norm[v] = sqrt((double)|A_v|) (np.sqrt of the degree, computed by the caller).  The best k by (sim desc,
 *   d_name_rank desc) -- heapq.nlargest(k, [(sim, name), ...]) when d_name_rank[v] is the rank of v's name in
 *   sorted(names).  Outputs (n_query x k, best first): d_out_ids (-1 padded), d_out_sims (0.0 padded), d_out_len.
 *   1 <= k <= 128.  Integer LDS counters, no float atomics: the same bits on every call.
 * srh_knn_score_topk: for each query user (d_users, n_query), the f64 row of UserKNN.predict (mode 0: d_nbr_* are the
 *   user lists; every training item of every neighbour, in list order) or ItemKNN.predict (mode 1: d_nbr_* are the
 *   item lists; for each training item i of the user in d_r_indices order, every item of i's list):
 *       score = S / (S + 1e-8) where touched (S: the sum of the sims added, in that order), 0.0 elsewhere
 *   with the user's training items at -10e8 when mask_train != 0 (predict() itself does not mask them); then the best
 *   n_top + 1 by (score desc, id asc).  Outputs (n_query x n_top): the first n_top, and rows in which two NEIGHBOURS
 *   of the n_top + 1 are equal marked d_out_ids[row][0] = -1 - id (srh_topk_trim_mark_ties' contract: the caller redoes them with srh_find_k_largest_host_f64).
 *   d_r_indptr / d_r_indices: users x items, each user's items in training-file order.  n_top + 1 <= min(128, n_items).
 *   d_ws >= srh_knn_score_ws_bytes(ws_rows, n_items): ws_rows f64 score rows; the users pass through them ws_rows at a
 *   time.  When n_query <= ws_rows, row q of d_ws holds query q's finished score row after the call.
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_knn_neighbours(const int32_t* d_a_indptr, const int32_t* d_a_indices, const int32_t* d_t_indptr,
                                const int32_t* d_t_indices, const double* d_norm, const int32_t* d_name_rank, int64_t n_rows,
                                const int32_t* d_query_rows, int64_t n_query, int32_t k, int32_t shrinkage,
                                int32_t* d_out_ids, double* d_out_sims, int32_t* d_out_len, void* stream);
int64_t srh_knn_score_ws_bytes(int64_t ws_rows, int64_t n_items);
srh_status_t srh_knn_score_topk(int32_t mode, const int32_t* d_users, int64_t n_query, const int32_t* d_r_indptr,
                                const int32_t* d_r_indices, int64_t n_items, const int32_t* d_nbr_ids,
                                const double* d_nbr_sims, const int32_t* d_nbr_len, int32_t k_nbr, int32_t n_top,
                                int32_t mask_train, void* d_ws, int64_t ws_rows, int32_t* d_out_ids, double* d_out_scores,
                                void* stream);

/* ------------------------------------------------------------------------------------
 * (a-15) SSL4Rec -- replaces the towers and losses of model/graph/SSL4Rec.py:25-46 (DNN_Encoder.user_tower /
 * item_tower: Linear(64, 1024) -> ReLU -> Linear(1024, 128) -> Tanh) and util/loss_torch.py:25-32 (batch_softmax_loss).
 *
 * srh_tower_fwd_f32: out (n x 128) = tanh(W2 relu(W1 x_r + b1) + b2) for rows x_r = d_table[d_idx[r]] (d_table[r] when
 *   d_idx is NULL; an id outside [0, n_table) reads a zero row: exact zeros in d_x_out, masked or not, and the row's output
 *   is the tower's value at zero).  relu is max(z, 0) with relu'(0) = 0, as torch: a unit whose pre-activation is exactly 0
 *   writes 0 to d_hidden and passes no gradient.  Rows r >= mask_row0 take feature dropout: x * m with
 *   m = keep ? 1 / (1 - drop_p) : 0 (nn.Dropout's scaled mask).  keep[r][c] is d_mask_in[(r - mask_row0) * 64 + c] != 0
 *   when d_mask_in is given, else it is drawn from the counter RNG of the SpMM epilogue (tests/counter_rng.py): the word
 *   of column c in float4 c / 4 at counter rng_counter + (r - mask_row0), keep = u01(word) >= drop_p -- a pure function
 *   of (seed, counter, row, column).  d_mask_out (optional) receives keep as 0 / 1 bytes in the same layout; d_x_out
 *   (n x 64, optional) the input after gather and dropout, d_hidden (n x 1024, optional) the post-ReLU hidden layer:
 *   what srh_tower_bwd_f32 reads.  The weights are nn.Linear's: W1 (1024 x 64), W2 (128 x 1024) row-major.
 * srh_tower_bwd_f32: from the forward's x, hidden and out and the upstream d_gy (n x 128): d_gx (n x 64, the gradient
 *   w.r.t. the gathered rows before dropout: already multiplied by the mask of rows >= mask_row0 when d_mask is given),
 *   d_gw1, d_gb1, d_gw2, d_gb2 (written, not added).  A unit is alive where d_hidden > 0 and nowhere else: the rows of
 *   d_gw1 and the entries of d_gb1 of a unit that is dead on every row are exact zeros.  The row of d_gx of an id outside
 *   the table is the gradient w.r.t. the zero row read there (not zero); srh_rows_segment_sum_f32 hands it to no table row.
 *   Reductions over rows in a fixed order, no float atomics: the same bits on every call.  d_ws >= srh_tower_bwd_ws_bytes(n).
 * srh_rows_segment_sum_f32: d_out[d_seg_row[s]] += sum of rows d_order[d_seg_start[s] .. d_seg_start[s + 1]) of d_x
 *   (n_rows x d), in that order: the deterministic scatter-add of gathered-row gradients into a table (the segments are
 *   a stable sort of the row ids; each table row at most once).  Per segment and column the terms are added in float32 from
 *   0 in that order and the sum is then ADDED to what d_out holds; rows of d_out that no segment names are not touched.  A
 *   d_seg_row entry outside [0, n_table) skips its segment, a d_order entry outside [0, n_rows) its term; n_seg = 0 returns
 *   at once.
 * srh_batch_softmax_fwd_bwd: u = normalize(U), v = normalize(V) (B x d each), p_b = exp(u_b.v_b / tau) / sum_j
 *   exp(u_b.v_j / tau);  *d_loss = mean_b -log(p_b + 1e-5) (double), d_gu / d_gv its gradients w.r.t. U and V (written).
 *   The B x B logits are never materialised.  d = 64 or 128; d_ws >= srh_batch_softmax_ws_bytes(B, d).
 *   The same envelope as srh_table_nce_fwd_bwd (a-12): exponentials are exp((s - 1) / tau) in f32; any data is safe for
 *   tau >= 0.023; below that, a row u_b with no v_j above cos = 1 - 87 tau (row sum under B * 2^-130) makes *d_loss NaN.
 * ---------------------------------------------------------------------------------- */
typedef struct srh_tower_weights {
  const float* d_w1; /* (1024, 64) */
  const float* d_b1; /* (1024) */
  const float* d_w2; /* (128, 1024) */
  const float* d_b2; /* (128) */
} srh_tower_weights_t;
srh_status_t srh_tower_fwd_f32(const float* d_table, const int32_t* d_idx, int64_t n, int64_t n_table,
                               const srh_tower_weights_t* w, int64_t mask_row0, const uint8_t* d_mask_in,
                               uint64_t rng_seed, uint64_t rng_counter, float drop_p, uint8_t* d_mask_out,
                               float* d_x_out, float* d_hidden, float* d_out, void* stream);
int64_t srh_tower_bwd_ws_bytes(int64_t n);
srh_status_t srh_tower_bwd_f32(const float* d_x, const float* d_hidden, const float* d_y, const float* d_gy, int64_t n,
                               const srh_tower_weights_t* w, int64_t mask_row0, const uint8_t* d_mask, float drop_p,
                               float* d_gx, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* d_ws,
                               void* stream);
srh_status_t srh_rows_segment_sum_f32(const float* d_x, int64_t n_rows, int32_t d, const int32_t* d_order,
                                      const int32_t* d_seg_start, const int32_t* d_seg_row, int64_t n_seg,
                                      int64_t n_table, float* d_out, void* stream);
int64_t srh_batch_softmax_ws_bytes(int64_t B, int32_t d);
srh_status_t srh_batch_softmax_fwd_bwd(const float* d_u, const float* d_v, int64_t B, int32_t d, float tau,
                                       double* d_loss, float* d_gu, float* d_gv, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-16) SASRec -- replaces the attention core of nn.MultiheadAttention as model/sequential/SASRec.py:107 calls it
 * (causal attn_mask, dropout on the probabilities) and calculate_loss (SASRec.py:44-53).
 *
 * srh_seq_attn_fwd_f32: d_q, d_k, d_v, d_out are (B, L, H * dh) row-major, head h in columns [h dh, (h + 1) dh):
 *   out[b, i, h] = sum_{j <= i} P~[b, h, i, j] v[b, j, h],  P = softmax_j(q_i . k_j / sqrt(dh)) over j <= i,
 *   P~ = P * (keep ? 1 / (1 - drop_p) : 0).  keep[b][h][i][j] is d_keep[((b H + h) L + i) L + j] != 0 when d_keep is
 *   given; else, when drop_p > 0, it is drawn from the counter RNG of the SpMM epilogue (tests/counter_rng.py): the word
 *   j % 4 of float4 j / 4 at counter rng_counter + (b H + h) L + i, keep = u01(word) >= drop_p -- a pure function of
 *   (seed, counter, b, h, row, col).  One call uses the counters [rng_counter, rng_counter + B H L): the caller advances
 *   its counter by B * H * L per call.  d_lse (B, H, L) receives the rows' log-sum-exp; the B x L x L scores are never
 *   written.
 * srh_seq_attn_bwd_f32: from q, k, v, the forward's d_lse, the same dropout arguments and the upstream d_go: d_gq, d_gk,
 *   d_gv (written).  dV = P~^T dO, dP = dO V^T, dS = P (m dP - rowsum(m dP P)), dQ = dS K / sqrt(dh),
 *   dK = dS^T Q / sqrt(dh).
 *   Envelope: 1 <= L <= 64, dh 32 or 64, H dh <= 128, any B >= 1; outside it SRH_ERR_UNSUPPORTED with a message.  One
 *   workgroup produces every element in a fixed order: no float atomics, the same bits on every call.
 * srh_seq_bce_fwd_bwd: for the rows r of d_hidden (R x d) with d_valid[r] != 0: x+ = h_r . table[pos[r]],
 *   x- = h_r . table[neg[r]]; d_loss2[0] = mean BCEWithLogits(x+, 1), d_loss2[1] = mean BCEWithLogits(x-, 0) over the
 *   n_valid valid rows (the caller's count of d_valid; the stable form max(x, 0) - x y + log1p(exp(-|x|)) in double,
 *   summed in a fixed order).  d_gh (R x d): d(loss2[0] + loss2[1]) / dh; d_grows (2R x d): row r the gradient the row
 *   contributes to table[pos[r]], row R + r to table[neg[r]] (zero rows where invalid) -- srh_rows_segment_sum_f32 over
 *   [pos; neg] makes the table gradient.  d_ws >= srh_seq_bce_ws_bytes(R).
 *   Any 1 <= d <= 1024, any R >= 1.  A row with d_valid[r] != 0 whose pos[r] or neg[r] lies outside [0, n_table) is
 *   treated as invalid: the ids are tested before any address is formed, no table row is read for it, it adds nothing to
 *   either loss and takes exact zeros in d_gh and in both of its d_grows rows.  n_valid stays the caller's divisor: to
 *   keep the means over the rows that count, the caller leaves such rows out of it.  n_valid outside [1, R] is refused
 *   (SRH_ERR_INVALID_ARG) before any launch.
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_seq_attn_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t B, int32_t L, int32_t H,
                                  int32_t dh, const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter, float drop_p,
                                  float* d_out, float* d_lse, void* stream);
srh_status_t srh_seq_attn_bwd_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_go,
                                  const float* d_lse, int64_t B, int32_t L, int32_t H, int32_t dh, const uint8_t* d_keep,
                                  uint64_t rng_seed, uint64_t rng_counter, float drop_p, float* d_gq, float* d_gk,
                                  float* d_gv, void* stream);
int64_t srh_seq_bce_ws_bytes(int64_t R);
srh_status_t srh_seq_bce_fwd_bwd(const float* d_hidden, int64_t R, int32_t d, const float* d_table, int64_t n_table,
                                 const int32_t* d_pos, const int32_t* d_neg, const uint8_t* d_valid, int64_t n_valid,
                                 double* d_loss2, float* d_gh, float* d_grows, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-17) BERT4Rec -- replaces the attention core of nn.MultiheadAttention as model/sequential/BERT4Rec.py:123 calls it
 * (attn_mask=None, no key-padding mask) and calculate_loss (BERT4Rec.py:58-62).
 *
 * srh_seq_attn_full_fwd_f32 / srh_seq_attn_full_bwd_f32: the arguments, layouts, dropout contract (keep mask given, or
 *   drawn at counter rng_counter + (b H + h) L + row, float4 col / 4, word col % 4; B H L counters per call), envelope
 *   and repeatability of srh_seq_attn_fwd_f32 / _bwd_f32 of (a-16), with P = softmax_j(q_i . k_j / sqrt(dh)) over ALL
 *   0 <= j < L: out[b, i, h] = sum_{j < L} P~[b, h, i, j] v[b, j, h].  Every position takes part, padded ones included.
 * srh_table_ce_fwd_bwd: softmax cross-entropy of the rows d_h (M x d) against the whole table d_t (N x d), logits
 *   s_mj = h_m . t_j (no normalisation, no temperature), d_labels (M, int32, in [0, N)):
 *     d_loss[0] = loss_scale * sum_m (lse_m - s_{m, label_m}),  lse_m = log sum_j exp(s_mj)   (double, fixed order)
 *     d_gh (M x d)        = loss_scale * (sum_j P_mj t_j - t_{label_m}),  P_mj = exp(s_mj - lse_m)
 *     d_gt (N x d, dense) = loss_scale * sum_m (P_mj - [j == label_m]) h_m
 *   all three WRITTEN.  The M x N logits and probabilities never reach memory; the softmax is max-subtracted (safe for
 *   any finite logits); no float atomics: one producer and one summation order per output element, the same bits on
 *   every call.  d = 64 or 128 (the caller zero-pads narrower rows), else SRH_ERR_UNSUPPORTED with a message; any M >= 1,
 *   N >= 1.  A label outside [0, N) reads nothing and makes the loss NaN; its row has no one-hot: d_gh of that row is
 *   loss_scale * sum_j P_mj t_j, it takes nothing off any row of d_gt, and every other row of d_gh and all of d_gt are
 *   what they are without it.  d_ws >= srh_table_ce_ws_bytes(M, N, d) and may hold anything on entry: every part of it
 *   that is read was written by the same call first.  loss_scale is applied once, as the last float32 multiplication
 *   of each gradient element and the last float64 one of the loss: 0 gives exact zeros, -1 the negated bits.  A
 *   non-finite loss_scale or M, N outside [1, 2^31) is refused (SRH_ERR_INVALID_ARG) before any launch.
 *   F.cross_entropy(h @ t.T, labels) / M (BERT4Rec.py:61) is loss_scale = 1 / M^2.
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_seq_attn_full_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t B, int32_t L,
                                       int32_t H, int32_t dh, const uint8_t* d_keep, uint64_t rng_seed,
                                       uint64_t rng_counter, float drop_p, float* d_out, float* d_lse, void* stream);
srh_status_t srh_seq_attn_full_bwd_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_go,
                                       const float* d_lse, int64_t B, int32_t L, int32_t H, int32_t dh,
                                       const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter, float drop_p,
                                       float* d_gq, float* d_gk, float* d_gv, void* stream);
int64_t srh_table_ce_ws_bytes(int64_t M, int64_t N, int32_t d);
srh_status_t srh_table_ce_fwd_bwd(const float* d_h, int64_t M, const float* d_t, int64_t N, int32_t d,
                                  const int32_t* d_labels, float loss_scale, double* d_loss, float* d_gh, float* d_gt,
                                  void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-25) The attention core of (a-16) and (a-17) for sequences of up to 512 positions (max.len above 64).
 *
 * srh_seq_attn_tiled_fwd_f32 / srh_seq_attn_tiled_bwd_f32: the layouts, formulas, d_lse and dropout contract (keep mask
 *   given, or drawn at counter rng_counter + (b H + h) L + row, float4 col / 4, word col % 4, keep = u01(word) >= drop_p;
 *   B H L counters per call) of srh_seq_attn_fwd_f32 / _bwd_f32 when causal != 0 and of srh_seq_attn_full_fwd_f32 /
 *   _bwd_f32 when causal == 0.  The forward walks 64-key blocks with a running row maximum and sum; only d_out and d_lse
 *   are written.  The backward takes the forward's d_out next to its d_lse (rowsum(m dP P) = dO_i . out_i, dropout
 *   included) and runs two launches: dQ by query block over the key blocks, dK and dV by key block over the query
 *   blocks, both in ascending order.  A query row that sees a single key (row 0 when causal, L = 1 otherwise) has
 *   dS = 0 identically and contributes exact zeros; a query row whose keep mask is empty gives exact zeros in d_out and
 *   d_gq, a key nobody keeps exact zeros in d_gv.
 *   Envelope: 1 <= L <= 512, dh 32 or 64, H dh <= 128, any B >= 1; outside it SRH_ERR_UNSUPPORTED with a message, a
 *   null argument or drop_p outside [0, 1) SRH_ERR_INVALID_ARG, all before any launch.  No float atomics and no
 *   scratch: one producer and one summation order per output element, the same bits on every call.
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_seq_attn_tiled_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t B, int32_t L,
                                        int32_t H, int32_t dh, int32_t causal, const uint8_t* d_keep, uint64_t rng_seed,
                                        uint64_t rng_counter, float drop_p, float* d_out, float* d_lse, void* stream);
srh_status_t srh_seq_attn_tiled_bwd_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_out,
                                        const float* d_go, const float* d_lse, int64_t B, int32_t L, int32_t H, int32_t dh,
                                        int32_t causal, const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter,
                                        float drop_p, float* d_gq, float* d_gk, float* d_gv, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-18) CL4SRec -- the embedding front of SASRec_Model.forward (model/sequential/SASRec.py:70-76: both gathers, the
 * scale, the sum, nn.Dropout, the padding mask) as model/sequential/CL4SRec.py:36-55 calls it three times a step, and the
 * table gradients behind it and behind calculate_loss.
 *
 * srh_seq_embed_fwd_f32: for the R rows of ids d_seq / d_posid (int32): a LIVE row (seq[r] != 0) gets
 *     out[r][c] = (item[seq[r]][c] * scale + pos[posid[r]][c]) * m(r, c)
 *   with the product and the sum rounded separately (no fma: at drop_p = 0 the bits of torch's items * scale + places).
 *   Every other row gets exact zeros and no table row is read for it (row 0 of either table is an ordinary initialised
 *   row).  An id outside its table (seq[r] < 0 or >= n_item, posid[r] < 0 or >= n_pos) makes a zero row, as in
 *   srh_tower_fwd_f32.  m = keep ? 1 / (1 - drop_p) : 0;  keep[r][c] is d_keep[r * d + c] != 0 when d_keep is given, else
 *   (drop_p > 0) drawn under the tower's contract: the word c % 4 of float4 c / 4 at counter rng_counter + r,
 *   keep = u01(word) >= drop_p -- a pure function of (seed, counter, r, c).  One call uses the counters
 *   [rng_counter, rng_counter + R).  d = 32, 64 or 128 (else SRH_ERR_UNSUPPORTED), any R >= 1.
 * srh_rows_live_sum_f32: up to SRH_LIVE_SUM_MAX_PROBLEMS deterministic segment sums in one pair of launches.  A problem's
 *   plan (ops.live_plan_host) lists the rows of d_x (n_rows x d) that matter, sorted stably by their table row:
 *     d_rows (n_live)              the listed rows, segment after segment
 *     d_chunk_start (n_chunk + 1)  every segment cut into chunks of at most SRH_LIVE_SUM_CHUNK entries of d_rows
 *     d_chunk_dst (n_chunk)        the table row when the chunk is its segment's only one, else -1
 *     d_multi_range (2 n_multi)    first chunk and one past the last chunk of every segment of two chunks or more
 *     d_multi_row (n_multi)        those segments' table rows
 *   and  d_out[row] = scale * sum over the segment's rows r, in plan order, of x[r] * m(r)  is WRITTEN for every table
 *   row the plan names; rows it does not name are left as they were (the caller zero-fills), rows of d_x it does not list
 *   are never read.  Launch 1: one lane group per chunk; the only chunk of a segment writes the table row, the others a
 *   partial to d_ws.  Launch 2 (when a problem has a cut segment): one lane group per such segment adds its partials in
 *   chunk order.  No float atomics: one producer and one order per output element, the same bits on every call.  m is the
 *   forward's dropout multiplier of row r (d_keep of n_rows x d bytes, or drawn at rng_counter + r when drop_p > 0, or
 *   1), so a backward pass redraws it instead of storing it.  A problem with n_chunk == 0 writes nothing; d, the widths of
 *   srh_seq_embed_fwd_f32, is shared by the problems of a call.  `problems` is a HOST array;
 *   d_ws >= srh_rows_live_sum_ws_bytes(problems, n_problems, d) (0 when no segment is cut).
 * ---------------------------------------------------------------------------------- */
#define SRH_LIVE_SUM_CHUNK 32
#define SRH_LIVE_SUM_MAX_PROBLEMS 3
srh_status_t srh_seq_embed_fwd_f32(const float* d_item, int64_t n_item, const float* d_pos, int64_t n_pos,
                                   const int32_t* d_seq, const int32_t* d_posid, int64_t R, int32_t d, float scale,
                                   const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter, float drop_p,
                                   float* d_out, void* stream);
typedef struct srh_live_sum_problem {
  const float* d_x;
  int64_t n_rows;
  const int32_t* d_rows;
  const int32_t* d_chunk_start;
  const int32_t* d_chunk_dst;
  const int32_t* d_multi_range;
  const int32_t* d_multi_row;
  int64_t n_live;
  int64_t n_chunk;
  int64_t n_multi;
  float* d_out;
  int64_t n_table;
  float scale;
  float drop_p;
  const uint8_t* d_keep;
  uint64_t rng_seed;
  uint64_t rng_counter;
} srh_live_sum_problem_t;
int64_t srh_rows_live_sum_ws_bytes(const srh_live_sum_problem_t* problems, int32_t n_problems, int32_t d);
srh_status_t srh_rows_live_sum_f32(const srh_live_sum_problem_t* problems, int32_t n_problems, int32_t d, void* d_ws,
                                   void* stream);

/* ------------------------------------------------------------------------------------
 * (a-19) SEPT -- tf.math.l2_normalize(x, axis=1) after every propagation of the four encoders (model/graph/SEPT.py:48-64)
 * and the tri-training step label_prediction -> top_k -> neighbor_discrimination (SEPT.py:98-134).
 *
 * srh_rows_l2norm_fwd_f32: inv_r = rsqrt(max(sum_c y_rc^2, 1e-12)), out_r = y_r * inv_r; d_out (n x d) and d_inv (n) are
 *   WRITTEN.  srh_rows_l2norm_bwd_f32: gy_r = (g_r - out_r (out_r . g_r)) * inv_r where the squared norm was >= 1e-12,
 *   g_r * 1e6 below it (decided from inv_r == 1e6).  Any 1 <= d <= 256 (else SRH_ERR_UNSUPPORTED), any n >= 0; one wave per
 *   row, no atomics, the same bits on every call.
 * srh_tri_nd_fwd_bwd: views V0 (friend), V1 (sharing), V2 (rec) and A (aug), each n x d: the gathered rows of the batch's
 *   unique users, un-normalised.  v = normalize(V), a = normalize(A) under the rule above;
 *     s_v[i][j] = v_i . a_j,  p_v[i][j] = softmax_j(s_v[i][.])            (temperature 1, the diagonal included)
 *     pos_v[i]  = the k largest j of p_a[i][j] + p_b[i][j], (a, b) the two views other than v; value descending, ties
 *                 to the lowest j (tf.math.top_k; the reference's halving of the sum is exact and monotone)
 *     d_loss[v] = loss_scale * sum_i [ log sum_j e_v[i][j] - log sum_{j in pos_v[i]} e_v[i][j] ],  e = exp(s / tau)
 *     dL/ds_v[i][j] = loss_scale / tau * ( e_ij / sum_j e_ij - [j in pos_v[i]] e_ij / sum_{j in pos} e_ij )
 *   The indices carry no gradient.  d_loss (double[3]), d_gview[v] and d_gaug (n x d, the normalisation backward
 *   included) and d_pos (int32, 3 x n x k, best first) are WRITTEN.  No n x n matrix reaches memory (the positives travel
 *   between the passes as n bits per row); exponentials are taken as exp((s - 1) / .); every product runs on the f32
 *   MFMA; no float atomics: the same bits on every call.  The ranking key of (i, j) depends on rows i and j alone, so
 *   identical aug rows tie exactly.  d = 64 or 128 (zero-pad narrower rows), 1 <= k <= 32, n >= k: anything else is
 *   SRH_ERR_UNSUPPORTED with a message.  d_ws >= srh_tri_nd_ws_bytes(n, d, k) (0 for an unsupported shape).
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_rows_l2norm_fwd_f32(const float* d_y, int64_t n, int32_t d, float* d_out, float* d_inv, void* stream);
srh_status_t srh_rows_l2norm_bwd_f32(const float* d_g, const float* d_out, const float* d_inv, int64_t n, int32_t d,
                                     float* d_gy, void* stream);
typedef struct srh_tri_nd_args {
  const float* d_view[3];
  const float* d_aug;
  int64_t n;
  int32_t d;
  int32_t k;
  float tau;
  float loss_scale;
  double* d_loss;
  float* d_gview[3];
  float* d_gaug;
  int32_t* d_pos;
} srh_tri_nd_args_t;
int64_t srh_tri_nd_ws_bytes(int64_t n, int32_t d, int32_t k);
srh_status_t srh_tri_nd_fwd_bwd(const srh_tri_nd_args_t* args, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-21) MixGCF -- the hop mixing of model/graph/MixGCF.py:96-114 (negative_mixup): pick, mix and row gradients.
 * H = n_hops item tables T_k (n_items x d float32, row-major; any 16-byte aligned address, e.g. the item rows of a
 * (users + items) x d table), C = n_negs candidates per pair: pair b owns d_neg[b C .. b C + C - 1].  All arithmetic fp32,
 * no float atomics, nothing waits on the host: a call returns the same bits every time.
 *
 * srh_mixup_fwd_f32: for every pair b < B and hop k < H, with p = T_k[pos[b]] and n_c = T_k[neg[b C + c]]:
 *     m_c = alpha_{k,b,c} (.) p + (1 - alpha_{k,b,c}) (.) n_c   (per element: fma(alpha, p, (1 - alpha) n))
 *     s_c = u_b . m_c,   pick[k][b] = argmax_c s_c
 *   (an exact float32 tie goes to the lowest c; the running maximum starts at -inf).  WRITTEN: d_neg_out[b] =
 *   (sum_k m_pick) / H and d_pos_out[b] = (sum_k T_k[pos[b]]) / H, both B x d and summed in hop order, and d_pick (int32,
 *   H x B).  The mixed candidates, alpha and the scores are never written to memory.
 * alpha: either INJECTED -- d_alpha[k] (B x C x d, values in [0, 1)) for every k < H -- or, with every d_alpha[k] NULL,
 *   DRAWN by the counter RNG of srh_spmm_epilogue (lowbias32 / counter_rng4 / u01): row (k, b, c) uses counter
 *   rng_counter + (k B + b) C + c and float4 number q of the row uses sub = q, so the draws of one call are the
 *   (H B C) x d block of counters [rng_counter, rng_counter + H B C).
 * srh_mixup_bwd_f32: from d_g_neg and d_g_pos (B x d; either may be NULL = zero), the forward's d_pick and the same alpha
 *   source (alpha* = alpha of the picked candidate, recomputed), every d_grad[k] (n_items x d) is WRITTEN whole -- zero
 *   outside the touched rows -- with
 *     row pos[b]                  += (g_pos[b] + alpha*_{k,b} (.) g_neg[b]) / H
 *     row neg[b C + pick[k][b]]   += ((1 - alpha*_{k,b}) (.) g_neg[b]) / H
 *   (per element fma(alpha*, g_neg, g_pos) / H and ((1 - alpha*) g_neg) / H, the division correctly rounded),
 *   summed per (hop, item) row in ascending b, a pair's positive before its negative, by one writer.  u takes no gradient
 *   (the choice is detached).  d_ws >= srh_mixup_bwd_ws_bytes(B, n_hops) (0 for an unsupported shape or B <= 0).
 * Served: d a multiple of 4 in 4..256, 1 <= n_hops <= SRH_MIXUP_MAX_HOPS, n_negs >= 1, any B >= 0 (B == 0: the backward
 *   writes the zero tables, the forward nothing); anything else is SRH_ERR_UNSUPPORTED with a message.  An index outside
 *   [0, n_items) is never dereferenced: such a candidate scores -inf, such a positive reads as a zero row, and neither
 *   takes a gradient.  The forward reads d_table, the backward d_grad; the other array may be left zeroed.
 * ---------------------------------------------------------------------------------- */
#define SRH_MIXUP_MAX_HOPS 8
typedef struct srh_mixup_args {
  const float* d_table[SRH_MIXUP_MAX_HOPS];
  const float* d_alpha[SRH_MIXUP_MAX_HOPS];
  float* d_grad[SRH_MIXUP_MAX_HOPS];
  const int32_t* d_pos;
  const int32_t* d_neg;
  int64_t n_items;
  int64_t B;
  int32_t n_hops;
  int32_t n_negs;
  int32_t d;
  uint64_t rng_seed;
  uint64_t rng_counter;
} srh_mixup_args_t;
srh_status_t srh_mixup_fwd_f32(const srh_mixup_args_t* args, const float* d_u, float* d_pos_out, float* d_neg_out,
                               int32_t* d_pick, void* stream);
int64_t srh_mixup_bwd_ws_bytes(int64_t B, int32_t n_hops);
srh_status_t srh_mixup_bwd_f32(const srh_mixup_args_t* args, const int32_t* d_pick, const float* d_g_pos,
                               const float* d_g_neg, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-22) DirectAU -- the alignment and uniformity losses of model/graph/DirectAU.py:37-48 on the batch's gathered rows,
 * forward and backward in one call, with no n x n matrix (and no list of n (n - 1) / 2 distances) in memory.
 * x and y: n x d float32, row-major, un-normalised.  With xh_i = x_i / max(|x_i|, 1e-12) (F.normalize):
 *     A(x, y) = mean_i |xh_i - yh_i|^2
 *     U(x)    = log( mean_{i<j} exp(-t |xh_i - xh_j|^2) )
 *     loss    = w_align A(x, y) + w_ux U(x) + w_uy U(y)
 *   taken in closed form: q_i = |xh_i|^2 (1 for an ordinary row, below 1 where the norm was clamped), s_ij = xh_i . xh_j,
 *     w_ij = exp(-t max(0, q_i + q_j - 2 s_ij)) for j != i, w_ii = 0;  r_i = sum_j w_ij;  Z = sum_i r_i;
 *     U = log(Z / (n (n - 1)));  dU/dxh_i = (4 t / Z) (sum_j w_ij xh_j - r_i xh_i);  dA/dxh_i = 2 (xh_i - yh_i) / n = -dA/dyh_i
 *   and through the normalisation (G - xh (xh . G)) / |x|, or G 1e12 where the norm was clamped (there the radial part
 *   r_i xh_i stays; on an ordinary row the projection removes it, so it is not formed).  The exponent is never positive:
 *   no running maximum.  Duplicate rows (a batch repeats users) weigh 1 and pull nothing.
 * srh_au_fwd_bwd READS d_x and d_y and WRITES, by plain stores, every element of d_gx and d_gy (n x d, dloss/dx and
 *   dloss/dy), d_parts[0..2] = A, U(x), U(y) unweighted, and d_loss[0] (doubles on the device).  d_y == NULL: U(x) alone --
 *   loss = w_ux U(x); w_align and w_uy are ignored and d_gy, d_parts[0] and d_parts[2] are not touched.  Neither the
 *   outputs nor the workspace need any initialisation by the caller.
 * Launches: prep (both sides: xh, 1 / max(|x|, 1e-12), q, the row's alignment term), the self-Gram pass (64-row tiles
 *   x key chunks x sides on v_mfma_f32_16x16x4_f32: the tile's rows in registers, the SAME matrix streamed through LDS,
 *   the weight taken on the accumulator and fed to the second product; own index and rows >= n weigh exactly 0), a
 *   reduction (r_i over the chunks in chunk order, then Z, A and the parts in a fixed order), the finish (chunk partials
 *   summed in chunk order, both gradients, the normalisation backward, the loss).  No float atomics; every sum has one
 *   order: a call returns the same bits every time.
 * Chunk plan (srh_au_chunk_plan; a function of n alone): tiles = ceil(n / 64), chunks = max(1, min(tiles,
 *   ceil(512 / (2 tiles)))), chunk_len = ceil(ceil(n / chunks) / 64) 64 keys; chunk c holds keys [c chunk_len,
 *   min(n, (c + 1) chunk_len)), which may be empty for trailing chunks (it then writes zeros).
 * Envelope: d = 64 or 128 (zero-pad narrower rows: a padded column changes no result), else SRH_ERR_UNSUPPORTED with a
 *   message; 2 <= n < 2^24 (n < 2 is SRH_ERR_INVALID_ARG: the reference gives nan there); t > 0 and finite, the weights
 *   finite.  All arguments are checked before any launch.  d_ws >= srh_au_ws_bytes(n, d) (0 for a shape the kernels do
 *   not serve): two normalised copies, 3 floats and 1 double per row and side, and per chunk and side n doubles and n x d
 *   floats.
 * ---------------------------------------------------------------------------------- */
int64_t srh_au_ws_bytes(int64_t n, int32_t d);
srh_status_t srh_au_chunk_plan(int64_t n, int64_t* chunks, int64_t* chunk_len);
srh_status_t srh_au_fwd_bwd(const float* d_x, const float* d_y, int64_t n, int32_t d, float t, float w_align, float w_ux,
                            float w_uy, double* d_parts, double* d_loss, float* d_gx, float* d_gy, void* d_ws,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * (a-23) Bootstrap losses -- BUIR (model/graph/BUIR.py:69-95) and SelfCF (model/graph/SelfCF.py:64-91): the predictor,
 * the two cosine terms against momentum-mixed targets, every gradient and the history store in one call; and BUIR's
 * momentum update of the batch's target rows.  All arithmetic fp32, loss and parts leave as doubles, no float atomics.
 * Online rows x_u, x_i (B x d float32, row-major), predictor p(x) = W x + b (nn.Linear: d_w is d x d, out x in), and per
 * side a target table T_side of n_tgt rows read at d_idx[r] (d_idx == NULL: B rows, read at r):
 *     t_side[r] = alpha T_side[idx_side[r]] + beta x_side[r]      (fl(fl(alpha T) + fl(beta x)); no gradient flows through it)
 *     vh = v / max(|v|, eps),   cu_r = ph(x_u[r]) . th(t_i[r]),   ci_r = ph(x_i[r]) . th(t_u[r])
 *     loss = c0 - c1 (mean_r cu_r + mean_r ci_r)
 *   BUIR: alpha = 1, beta = 0, eps = 1e-12 (F.normalize), c0 = 4, c1 = 2, clamp = SRH_BOOT_CLAMP_NORMALIZE, T = the target
 *   encoder's propagated tables.
 *   SelfCF: alpha = m, beta = 1 - m, eps = 1e-8 (F.cosine_similarity: each side over max(norm, eps)), c0 = 1, c1 = 0.5,
 *   clamp = SRH_BOOT_CLAMP_COSINE, T = the history tables, which are also d_store.
 *   Gradients in closed form: dP_r = -(c1 / B) (th - (ph . th) ph) / |p| on an ordinary row;  dX = dP W;
 *   d_gw = dP_u^T X_u + dP_i^T X_i;  d_gb = the column sums of both dP.  Where |p| was clamped the two forward-equal
 *   expressions differentiate differently, and `clamp` says which one the caller's model is:
 *     SRH_BOOT_CLAMP_NORMALIZE  dP_r = -(c1 / B) th / eps, no projection: autograd through x / max(|x|, eps)
 *     SRH_BOOT_CLAMP_COSINE     dP_r = -(c1 / B) (th - (ph . th) p / |p|) / eps (p / |p| = 0 at p = 0): F.cosine_similarity
 *                               clamps the norm in place outside the graph, so the norm's own derivative stays
 * srh_boot_fwd_bwd WRITES, by plain stores, every element of user->d_gx and item->d_gx (B x d), d_gw (d x d), d_gb (d),
 *   d_parts[0..1] = mean cu, mean ci and d_loss[0] (doubles on the device); then, where a side's d_store is given (a table
 *   of n_tgt rows, which may be that side's d_tgt), d_store[d_idx[r]] = x[r] for every slot.  Every target read of the call
 *   happens before any of these stores (they are the last launch): a slot never sees a history row that another slot of the
 *   same call has overwritten -- torch's gather, then index-assign.  Slots of one id are expected to hold the same x row
 *   (rows gathered by that id), so their stores are the same bits.  An id outside [0, n_tgt) reads a zero row and its
 *   store is skipped, as in srh_tower_fwd_f32; its gradients are still per slot.  Neither the outputs nor the workspace
 *   need any initialisation by the caller, and a call returns the same bits every time.
 * Launches: main (side x 64-row tile, 16 rows per wave, on v_mfma_f32_16x16x4_f32: the tile's rows in registers, W
 *   streamed through LDS 64 output rows at a time, P^T = W X^T + b on the accumulator; target mix, norms and the cosine in
 *   the accumulator's layout; dP formed there, written for the weight gradients and fed back as the B operand of
 *   dX^T = W^T dP^T), the loss (row terms of each side in one fixed order), the weight gradients (dP^T X and the column
 *   sums per chunk of 256 rows; the chunk partials summed in chunk order, the user side before the item side), the store.
 * Envelope: d = 64 or 128 (zero-pad narrower rows TOGETHER WITH the rows and columns of W and the entries of b: a padded
 *   column changes no result and takes exactly zero gradient), else SRH_ERR_UNSUPPORTED with a message; 1 <= B < 2^24;
 *   alpha, beta, c0, c1 finite; eps > 0; clamp one of the two above.  All arguments are checked before any launch.  d_ws >= srh_boot_ws_bytes(B, d)
 *   (0 for a shape the kernels do not serve): 2 B d floats, 2 B doubles and per side and chunk d x d + d floats.
 *
 * srh_rows_momentum_f32 (BUIR.py:69-75, update_target): tgt[idx] = tgt[idx] * m + src[idx] * (1 - m) for the n slots of
 *   d_idx (int32) over two tables of n_table rows x d.  Phase 1 computes fl(fl(tgt[id] m) + fl(src[id] one_minus_m)) for
 *   every slot from the values the table held BEFORE the call (no contraction into a fused multiply-add), phase 2, a launch
 *   of its own, stores them: slots of one id compute and store the same bits, so a repeated id is updated once, as torch's
 *   index assignment does.  An id outside [0, n_table) is skipped.  Any d >= 1, n >= 0; the caller passes m and 1 - m as
 *   the two floats torch rounds them to.  d_ws >= srh_rows_momentum_ws_bytes(n, d) = n d floats (0 for n < 1 or d < 1).
 * ---------------------------------------------------------------------------------- */
#define SRH_BOOT_CLAMP_NORMALIZE 0
#define SRH_BOOT_CLAMP_COSINE 1
typedef struct srh_boot_side {
  const float* d_x;       /* B x d, read */
  const float* d_tgt;     /* n_tgt x d (B x d when d_idx is NULL), read */
  const int32_t* d_idx;   /* B, or NULL */
  int64_t n_tgt;
  float* d_store;         /* n_tgt x d, or NULL; may be d_tgt */
  float* d_gx;            /* B x d, written */
} srh_boot_side_t;
int64_t srh_boot_ws_bytes(int64_t B, int32_t d);
srh_status_t srh_boot_fwd_bwd(const srh_boot_side_t* user, const srh_boot_side_t* item, const float* d_w, const float* d_b,
                              int64_t B, int32_t d, float alpha, float beta, float eps, float c0, float c1, int32_t clamp,
                              double* d_parts, double* d_loss, float* d_gw, float* d_gb, void* d_ws, void* stream);
int64_t srh_rows_momentum_ws_bytes(int64_t n, int32_t d);
srh_status_t srh_rows_momentum_f32(float* d_tgt, const float* d_src, const int32_t* d_idx, int64_t n, int64_t n_table,
                                   int32_t d, float m, float one_minus_m, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-24) The rest of util/loss_torch.py -- info_nce (:54-88), InfoNCE with b_cos=False or a low temperature (:35-50),
 * triplet_loss (:12-16) and kl_divergence (:91-94).  DESIGN.md 4.27.
 *
 * srh_pair_ce_fwd_bwd: srh_table_ce_fwd_bwd of (a-17) -- the same kernels, ownership, chunking, workspace layout
 *   (srh_pair_ce_ws_bytes(M, N, d) == srh_table_ce_ws_bytes(M, N, d)), repeatability and label rule -- with scaled logits
 *   s_mj = inv_temp * h_m . t_j and, with exclude_diagonal != 0 (M == N), key j = m left out of row m's softmax:
 *     d_loss[0] = loss_scale * sum_m (lse_m - s_{m, label_m}),  lse_m = log sum_{j (!= m)} exp(s_mj)
 *     d_gh (M x d) = loss_scale * inv_temp * (sum_j P_mj t_j - t_{label_m}),  P_mj = exp(s_mj - lse_m) (0 at j = m if excluded)
 *     d_gt (N x d) = loss_scale * inv_temp * sum_m (P_mj - [j == label_m]) h_m
 *   add_gh_into_gt != 0 (M == N): d_gt receives d_gt + d_gh row by row (d_gh is written as above); a caller whose H and T
 *   are one matrix z reads dL/dz from d_gt.  d_h and d_t may be the same address (both are only read); d_gh and d_gt
 *   may not.  Under exclusion a row can meet a key tile or chunk that holds no key but its own: it contributes nothing.
 *   labels[m] == m under exclusion names a key that is not in the row's softmax: that row's loss term is NaN, as for a
 *   label outside [0, N) (same gradient rule: the row has no one-hot).  exclude_diagonal with N == 1 or M != N,
 *   add_gh_into_gt with M != N, inv_temp not positive and finite, a non-finite loss_scale: SRH_ERR_INVALID_ARG with a
 *   message, before any launch.  d = 64 or 128.
 *   InfoNCE(v1, v2, tau, b_cos=False): labels = 0..n-1, inv_temp = 1/tau, loss_scale = 1/n.  info_nce(z_i, z_j, temp, B):
 *   H = T = cat(z_i, z_j), labels[m] = (m + B) mod 2B, inv_temp = 1/temp, loss_scale = 1/(2B), both flags set.
 * srh_triplet_fwd_bwd: x_b = |u_b - p_b|^2 - |u_b - n_b|^2 + margin over B rows of d columns (32, 64, 128 or 256):
 *     d_loss[0] = mean_b max(x_b, 0) (double);  rows with x_b > 0: d_gu = 2 (n - p) / B, d_gp = -2 (u - p) / B,
 *     d_gn = 2 (u - n) / B;  rows with x_b <= 0: exact zeros.  All four WRITTEN; the three gradient buffers are distinct.
 *   The distances are summed in double; the mean is taken on the device in a fixed order (no float atomics).
 *   d_ws >= srh_triplet_ws_bytes(B), any content.
 * srh_kl_div_fwd_bwd: rows of R x C logits, any R >= 1, C >= 1 (C is a loop bound, nothing is padded):
 *     p = softmax(p_logit_r), q = softmax(q_logit_r), kl_r = sum_c p_c (log p_c - log q_c);  d_loss[0] = mean_r kl_r (double)
 *     d_gp (R x C) = p_rc ((log p_rc - log q_rc) - kl_r) / R,   d_gq (R x C) = (q_rc - p_rc) / R
 *   Both softmaxes max-subtracted; a column with p_c == 0 contributes 0.  d_p_logit may equal d_q_logit (loss 0); d_gp and
 *   d_gq are distinct.  d_ws >= srh_kl_div_ws_bytes(R), any content.
 * ---------------------------------------------------------------------------------- */
int64_t srh_pair_ce_ws_bytes(int64_t M, int64_t N, int32_t d);
srh_status_t srh_pair_ce_fwd_bwd(const float* d_h, int64_t M, const float* d_t, int64_t N, int32_t d,
                                 const int32_t* d_labels, float inv_temp, float loss_scale, int32_t exclude_diagonal,
                                 int32_t add_gh_into_gt, double* d_loss, float* d_gh, float* d_gt, void* d_ws,
                                 void* stream);
int64_t srh_triplet_ws_bytes(int64_t B);
srh_status_t srh_triplet_fwd_bwd(const float* d_u, const float* d_p, const float* d_n, int64_t B, int32_t d, float margin,
                                 double* d_loss, float* d_gu, float* d_gp, float* d_gn, void* d_ws, void* stream);
int64_t srh_kl_div_ws_bytes(int64_t R);
srh_status_t srh_kl_div_fwd_bwd(const float* d_p_logit, const float* d_q_logit, int64_t R, int64_t C, double* d_loss,
                                float* d_gp, float* d_gq, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-25) DuoRec's contrastive section -- two info_nce terms (util/loss_torch.py:54-88) that share their anchor rows,
 * forward and backward in two launches.  DESIGN.md 4.29.
 *
 * srh_duo_nce_fwd_bwd: z = [x[idx_a]; x[idx_p]; x[idx_q]] (3B rows of d columns, B >= 1; all three index vectors NULL: z is
 *   the first 3B rows of x, rows >= 3B), s = inv_temp z z^T.  The u-softmax runs over U = A u P and the s-softmax over
 *   V = A u Q; a row never sees itself, P rows see no Q key and Q rows no P key; partner_u: a_b <-> p_b, partner_s: a_b <-> q_b.
 *     lse^t_m = log sum_{j in keys_t(m)} exp(s_mj)
 *     d_losses[t] = scale_t / 2B * sum_m (lse^t_m - s_{m, partner_t(m)})           (two doubles: u, s)
 *     d_g (3B x d, rows [ga; gp; gq]) = sum_t scale_t inv_temp / 2B * sum_{j in keys_t(r)}
 *                                       (exp(s_rj - lse^t_r) + exp(s_rj - lse^t_j) - 2 [j == partner_t(r)]) z_j
 *   = info_nce(z_a, z_p, 1 / inv_temp, B) * scale_u and info_nce(z_a, z_q, ...) * scale_s with their whole gradients: the
 *   second exponential is the key side of each loss, taken from the same score by symmetry.  Both WRITTEN.  Every row of
 *   d_g has one producer and one summation order: no float atomics, the same bits on every call.  Running maxima make any
 *   finite logits safe.  The caller guarantees 0 <= idx < rows and that the 3B indices are pairwise distinct (a row named
 *   twice would be its own key).  B == 1: each softmax has one key; both losses and d_g are exact zeros.
 *   d = 64 or 128, anything else SRH_ERR_UNSUPPORTED; inv_temp not positive and finite, a non-finite scale, one or two
 *   index vectors: SRH_ERR_INVALID_ARG; all with a message, before any launch.  d_ws >= srh_duo_nce_ws_bytes(B, d) (0 for
 *   an unsupported shape), any content.
 * ---------------------------------------------------------------------------------- */
int64_t srh_duo_nce_ws_bytes(int64_t B, int32_t d);
srh_status_t srh_duo_nce_fwd_bwd(const float* d_x, int64_t rows, const int32_t* d_idx_a, const int32_t* d_idx_p,
                                 const int32_t* d_idx_q, int64_t B, int32_t d, float inv_temp, float scale_u, float scale_s,
                                 double* d_losses, float* d_g, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (a-26) GRU4Rec's recurrence -- the hidden-side half of one torch.nn.GRU layer (gate order r, z, n; both biases) over
 * right-padded sequences, forward and backward in one launch each.  DESIGN.md 4.30.  The input-side product
 * gi = X W_ih^T + b_ih and the weight-gradient products are the caller's GEMMs.
 *
 * srh_gru_fwd_f32: d_gi (B x L x 3H), d_w_hh (3H x H), d_b_hh (3H), d_len (B, int32, 0 <= len_b <= L).  Per sequence b,
 *   t < len_b, h_{-1} = 0:
 *     gh = W_hh h_{t-1} + b_hh;  r = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);  n = tanh(gi_n + r (.) gh_n)
 *     h_t = (1 - z) (.) n + z (.) h_{t-1};   d_out[b,t] = h_t;   d_gates[b,t] = [r, z, n, gh_n]
 *   d_out (B x L x H) and d_gates (B x L x 4H) are WRITTEN whole: their rows at t >= len_b are exact zeros; gi there is
 *   never read.  d_gates == NULL (evaluation): nothing is saved, d_out holds the same bits.
 * srh_gru_bwd_f32: from the upstream gradient d_go (B x L x H) and the forward's d_out and d_gates.  Per sequence b,
 *   carry = 0, t = len_b - 1 .. 0, hp = out[b,t-1] (0 at t = 0):
 *     dh = carry + go[b,t];  dn = dh (1 - z)(1 - n^2);  dz = dh (hp - n) z (1 - z);  dr = dn gh_n r (1 - r)
 *     d_dgi[b,t] = [dr, dz, dn];   d_dghn[b,t] = dn r;   carry = dh z + [dr, dz, dn r] W_hh
 *   d_dgi (B x L x 3H) and d_dghn (B x L x H) are WRITTEN whole, exact zeros at t >= len_b; d_go there is never read (it
 *   may hold anything, NaN included).  The caller finishes with GEMMs on the zero-padded outputs: dX = dgi W_ih,
 *   dW_ih = dgi^T X, db_ih = sum dgi, and with dGH = [dgi_r, dgi_z, dghn]: dW_hh = dGH^T H_prev, db_hh = sum dGH.
 *   One workgroup owns 16 sequences for all their steps; both products run on v_mfma_f32_16x16x4_f32 with W_hh resident
 *   in registers.  One summation order, no float atomics: the same bits on every call.
 *   H == 64 (a narrower layer is zero-padded by the caller: a padded unit stays an exact 0) and 1 <= L <= 512, anything
 *   else SRH_ERR_UNSUPPORTED; B < 1 or a null required pointer SRH_ERR_INVALID_ARG; all with a message, before any launch.
 *   d_gi, d_w_hh and every output must be 16-byte aligned (the kernels read W_hh and write the dead rows as 16-byte
 *   vectors); a misaligned one is SRH_ERR_INVALID_ARG.
 *   The lengths stay on the device, so 0 <= len_b <= L is the caller's contract; the kernels clamp a length into that
 *   range before they use it, so a bad one reads and writes nothing outside the tensors.
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_gru_fwd_f32(const float* d_gi, const float* d_w_hh, const float* d_b_hh, const int32_t* d_len, int64_t B,
                             int32_t L, int32_t H, float* d_out, float* d_gates, void* stream);
srh_status_t srh_gru_bwd_f32(const float* d_go, const float* d_out, const float* d_gates, const float* d_w_hh,
                             const int32_t* d_len, int64_t B, int32_t L, int32_t H, float* d_dgi, float* d_dghn,
                             void* stream);

/* ------------------------------------------------------------------------------------
 * (a-20) MHCN -- the self-gates, the channel attention and the hierarchical mutual-information loss of
 * model/graph/MHCN.py:79-93 and 159-181.  All arithmetic fp32; no float atomics: every reduction over rows runs in fixed
 * chunks whose partials are summed in chunk order, so a call returns the same bits every time.  d = 64 or 128 (zero-pad
 * narrower rows: a padded column has x = 0 and changes no result), anything else is SRH_ERR_UNSUPPORTED with a message;
 * any n >= 0 (n == 0 writes only the weight gradients / the loss, as zeros).
 *
 * srh_gate_fwd_f32: Y_c = X (.) sigmoid(X W_c + b_c), c < n_gates (1..4).  d_x (n x d), d_w (n_gates x d x d, the x @ W
 *   layout), d_b (n_gates x d); d_y (n_gates x n x d) is WRITTEN.  The product runs on v_mfma_f32_16x16x4_f32, every gate
 *   from one read of X.
 * srh_gate_bwd_f32: with dZ_c = dY_c (.) X (.) S_c (1 - S_c) (S is recomputed, not saved):
 *   d_gx = sum_c (dY_c (.) S_c + dZ_c W_c^T), d_gw[c] = X^T dZ_c, d_gb[c] = the column sums of dZ_c; all WRITTEN.
 *   d_ws >= srh_gate_bwd_ws_bytes(n, d, n_gates) (0 for an unsupported shape).
 * srh_chan_mix_fwd_f32: w_c[r] = E_c[r] . q, s[r] = softmax_c w_c[r], out[r] = sum_c s_c[r] E_c[r] + beta X[r] (d_x may be
 *   NULL: no addend).  d_out (n x d) and d_score (n x 3) are WRITTEN.  One wave per row.
 * srh_chan_mix_bwd_f32: from d_gout (n x d) and the forward's d_score: d_ge1..3 (n x d), d_gx = beta d_gout (optional, may
 *   be NULL) and d_gq (d) are WRITTEN.  The scores carry no gradient of their own.  d_ws >= srh_chan_mix_bwd_ws_bytes(n, d).
 * srh_mim_fwd_bwd: em, edge (n x d; edge = H em, made by the caller), row permutations p1, p2, p3 (int32, n) and column
 *   permutations c2, c3 (int32, d; the identity over pad columns).  rcs(E; c, p)[r][j] = E[p[r]][c[j]],
 *   sp(x) = max(x, 0) + log1p(exp(-|x|)), g = the column mean of edge;
 *     pos = em_r . edge_r, n1 = em_{p1[r]} . edge_r, n2 = rcs(edge; c2, p2)_r . em_r, gp = edge_r . g,
 *     gn = rcs(edge; c3, p3)_r . g;   d_loss = loss_scale * sum_r sp(n1 - pos) + sp(n2 - n1) + sp(gn - gp)
 *   (sp(-x) = -log(sigmoid(x)) wherever the latter is finite in float32).  d_loss (one double), d_gem and d_gedge (n x d,
 *   scaled by loss_scale, the gradient through g included) are WRITTEN.  Every scatter of the backward pass is a gather
 *   through the inverse permutation, built on the device in the workspace; an index outside its range contributes nothing.
 *   d_ws >= srh_mim_ws_bytes(n, d).
 * ---------------------------------------------------------------------------------- */
srh_status_t srh_gate_fwd_f32(const float* d_x, const float* d_w, const float* d_b, int64_t n, int32_t d, int32_t n_gates,
                              float* d_y, void* stream);
int64_t srh_gate_bwd_ws_bytes(int64_t n, int32_t d, int32_t n_gates);
srh_status_t srh_gate_bwd_f32(const float* d_x, const float* d_w, const float* d_b, const float* d_gy, int64_t n, int32_t d,
                              int32_t n_gates, float* d_gx, float* d_gw, float* d_gb, void* d_ws, void* stream);
srh_status_t srh_chan_mix_fwd_f32(const float* d_e1, const float* d_e2, const float* d_e3, const float* d_q,
                                  const float* d_x, float beta, int64_t n, int32_t d, float* d_out, float* d_score,
                                  void* stream);
int64_t srh_chan_mix_bwd_ws_bytes(int64_t n, int32_t d);
srh_status_t srh_chan_mix_bwd_f32(const float* d_e1, const float* d_e2, const float* d_e3, const float* d_q,
                                  const float* d_score, const float* d_gout, float beta, int64_t n, int32_t d, float* d_ge1,
                                  float* d_ge2, float* d_ge3, float* d_gx, float* d_gq, void* d_ws, void* stream);
typedef struct srh_mim_args {
  const float* d_em;
  const float* d_edge;
  const int32_t* d_row_perm[3];
  const int32_t* d_col_perm[2];
  int64_t n;
  int32_t d;
  float loss_scale;
  double* d_loss;
  float* d_gem;
  float* d_gedge;
} srh_mim_args_t;
int64_t srh_mim_ws_bytes(int64_t n, int32_t d);
srh_status_t srh_mim_fwd_bwd(const srh_mim_args_t* args, void* d_ws, void* stream);

/* ------------------------------------------------------------------------------------
 * (f-1) Dataset files -> id arrays -- replaces the python loops of data/loader.py:22-33
 * (FileIO.load_data_set: one "user item weight" line per interaction, single-space separated)
 * and data/ui_graph.py:29-45 (ids in first-appearance order of the training file; test pairs kept
 * only when both ends occur in training).  Host only.
 * sizes5 = {n_users, n_items, n_train, n_test_kept, n_test_lines}; names are returned concatenated
 * (offsets has n+1 entries).  which: 0 = users, 1 = items.
 * ---------------------------------------------------------------------------------- */
typedef struct srh_dataset srh_dataset_t;
srh_status_t srh_dataset_load(srh_dataset_t** out, const char* train_path, const char* test_path /* or NULL */);
void srh_dataset_destroy(srh_dataset_t* ds);
srh_status_t srh_dataset_sizes(const srh_dataset_t* ds, int64_t* h_sizes5);
srh_status_t srh_dataset_copy_ids(const srh_dataset_t* ds, int32_t* h_train_u, int32_t* h_train_i,
                                  float* h_train_w, int32_t* h_test_u, int32_t* h_test_i);
int64_t srh_dataset_names_bytes(const srh_dataset_t* ds, int32_t which);
/* h_offsets != NULL: names back to back in h_buf (names_bytes bytes), name k = [h_offsets[k], h_offsets[k+1]); h_offsets
 * == NULL: every name followed by '\n' (names_bytes + count bytes; a name is a token of a line, so it holds no '\n') --
 * one bulk split on the caller's side instead of a slice per name. */
srh_status_t srh_dataset_copy_names(const srh_dataset_t* ds, int32_t which, char* h_buf, int64_t* h_offsets);

#ifdef __cplusplus
}
#endif
#endif /* SELFREC_HIP_H */

// UserKNN / ItemKNN (reference model/graph/UserKNN.py, ItemKNN.py): exact neighbour search and ranking.  DESIGN.md 4.7.
//
// Ratings are all 1 (data/ui_graph.py:39), so the reference's cosine with shrinkage between rows a and b of a binary
// matrix depends on three integers, n = |a & b|, d_a = |a|, d_b = |b| (UserKNN.py:14-30):
//   sim = (n / (n + s)) * (n / (sqrt(d_a) * sqrt(d_b) + 1e-8))
// every operation a separately rounded f64 one.  The whole file is compiled with contraction OFF, so no multiply-add is
// fused and the expression rounds exactly as Python's floats do.
//
// srh_knn_neighbours: one workgroup per query row.  The co-occurrence counts n of the row against every candidate are
// gathered through the row's features and the transposed CSR into int32 counters in LDS (integer LDS atomics: order-free,
// the same counts on every call), 32,768 candidates per chunk.  Per chunk, the best K by (sim desc, name rank desc) --
// heapq.nlargest(K, [(sim, name), ...]) at UserKNN.py:51 -- are merged into a running list in LDS: a lower bound of the
// K-th key from the per-thread maxima, every key at or above it (and the running list) into a buffer, ranks by counting.
// A buffer overflow takes K rounds of "largest key after the previous pick" instead.  Keys are unique (name ranks are).
//
// srh_knn_score_topk: one workgroup per query user, looping over the users; each owns one f64 score row of the workspace.
// Sources are added in the reference's order (UserKNN.py:70-76: neighbours in list order, every item of each;
// ItemKNN.py:69-76: the user's items in training order, the neighbour list of each), one source per barrier-separated
// step, every item touched at most once per step: one f64 accumulator per item, no atomics.  Then score = S / (S + 1e-8)
// (0 where untouched), training items -10e8 (unless the caller wants predict()'s unmasked row), and the best N + 1 by
// (score desc, id asc) with the tie mark of srh_topk_trim_mark_ties: rows whose N + 1 best hold two equal neighbours get
// ids[row][0] = -1 - id.
#pragma clang fp contract(off)

#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int kKnnMaxK = 128;          // neighbours per list / ranked columns (the LDS lists below)
constexpr int kNbThreads = 512;
constexpr int kNbWaves = kNbThreads / 64;
constexpr int kNbChunk = 32768;        // candidate counters per pass (128 KB of LDS)
constexpr int kNbCap = 1024;           // keys at or above the bound that one pass can rank by counting
constexpr size_t kNbLds = (size_t)kNbCap * 16 + (size_t)kKnnMaxK * 16 + (size_t)kNbThreads * 12 + (size_t)kNbChunk * 4;

constexpr int kScThreads = 256;
constexpr int kScCap = 2048;
constexpr double kMasked = -10e8;      // base/graph_recommender.py:50

// n + s is formed in f64 (exact: both are below 2^31), so that a shrinkage near INT_MAX cannot wrap the sum as int would
__device__ __forceinline__ double knn_sim(int n, int s, double norm_a, double norm_b) {
  const double shrink = (double)n / ((double)n + (double)s);
  const double raw = (double)n / (norm_a * norm_b + 1e-8);
  return shrink * raw;
}

// neighbour order: (sim desc, name rank desc); the sentinel (-1, -1) comes after every real key (sims are > 0)
__device__ __forceinline__ bool nb_before(double sa, int ra, double sb, int rb) {
  return sa > sb || (sa == sb && ra > rb);
}
// ranking order: (score desc, id asc); the sentinel (-inf, INT_MAX) comes after every real key
__device__ __forceinline__ bool sc_before(double sa, int ia, double sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

__global__ __launch_bounds__(kNbThreads) void knn_neighbours_kernel(
    const int32_t* __restrict__ a_indptr, const int32_t* __restrict__ a_indices, const int32_t* __restrict__ t_indptr,
    const int32_t* __restrict__ t_indices, const double* __restrict__ norm, const int32_t* __restrict__ name_rank,
    int n_rows, const int32_t* __restrict__ query_rows, int k, int shrinkage, int32_t* __restrict__ out_ids,
    double* __restrict__ out_sims, int32_t* __restrict__ out_len) {
  extern __shared__ __align__(16) unsigned char lds[];
  double* b_sim = reinterpret_cast<double*>(lds);          // kNbCap   candidate buffer
  double* r_sim = b_sim + kNbCap;                          // K        running list, best first
  double* m_sim = r_sim + kKnnMaxK;                        // threads  per-thread maxima
  int* b_id = reinterpret_cast<int*>(m_sim + kNbThreads);
  int* b_rank = b_id + kNbCap;
  int* r_id = b_rank + kNbCap;
  int* r_rank = r_id + kKnnMaxK;
  int* m_rank = r_rank + kKnnMaxK;
  int* cnt = m_rank + kNbThreads;                          // kNbChunk co-occurrence counters
  __shared__ int s_cnt, s_len, s_thr_rank, s_last_rank;
  __shared__ double s_thr_sim, s_last_sim;
  __shared__ double w_sim[kNbWaves];
  __shared__ int w_rank[kNbWaves], w_id[kNbWaves];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = blockIdx.x;
  const int q = query_rows ? query_rows[qi] : qi;
  const int a0 = a_indptr[q], a1 = a_indptr[q + 1];
  const double nq = norm[q];
  if (tid == 0) s_len = 0;

  for (int c0 = 0; c0 < n_rows; c0 += kNbChunk) {
    const int width = min(kNbChunk, n_rows - c0), c1 = c0 + width;
    for (int i = tid; i < width; i += kNbThreads) cnt[i] = 0;
    __syncthreads();
    // gather-count: one wave per feature of the query row, lanes along the feature's (ascending) rows in [c0, c1)
    for (int p = a0 + wave; p < a1; p += kNbWaves) {
      const int f = a_indices[p];
      int lo = t_indptr[f];
      const int hi = t_indptr[f + 1];
      if (c0 > 0) lo = srh::lower_bound_i32(t_indices, lo, hi, c0);
      for (int j = lo + lane; j < hi; j += 64) {
        const int v = t_indices[j];
        if (v >= c1) break;
        atomicAdd(&cnt[v - c0], 1);
      }
    }
    __syncthreads();
    // per-thread best key of this chunk
    double bs = -1.0;
    int br = -1;
    for (int i = tid; i < width; i += kNbThreads) {
      const int n = cnt[i], v = c0 + i;
      if (n > 0 && v != q) {
        const double s = knn_sim(n, shrinkage, nq, norm[v]);
        const int rk = name_rank[v];
        if (nb_before(s, rk, bs, br)) { bs = s; br = rk; }
      }
    }
    m_sim[tid] = bs;
    m_rank[tid] = br;
    if (tid == 0) { s_cnt = 0; s_thr_sim = -1.0; s_thr_rank = -1; }
    __syncthreads();
    // bound: the K-th best of the thread maxima (K distinct candidates reach it), raised to the running list's K-th
    {
      int pos = 0;
      for (int j = 0; j < kNbThreads; ++j) {
        const double os = m_sim[j];
        const int orr = m_rank[j];
        pos += nb_before(os, orr, bs, br) || (os == bs && orr == br && j < tid);
      }
      if (pos == k - 1) {
        const int len = s_len;
        if (len == k && nb_before(r_sim[k - 1], r_rank[k - 1], bs, br)) { s_thr_sim = r_sim[k - 1]; s_thr_rank = r_rank[k - 1]; }
        else { s_thr_sim = bs; s_thr_rank = br; }
      }
    }
    __syncthreads();
    const double ts = s_thr_sim;
    const int tr = s_thr_rank;
    const int len0 = s_len;
    for (int i = tid; i < width; i += kNbThreads) {
      const int n = cnt[i], v = c0 + i;
      if (n > 0 && v != q) {
        const double s = knn_sim(n, shrinkage, nq, norm[v]);
        const int rk = name_rank[v];
        if (!nb_before(ts, tr, s, rk)) {
          const int slot = atomicAdd(&s_cnt, 1);
          if (slot < kNbCap) { b_sim[slot] = s; b_rank[slot] = rk; b_id[slot] = v; }
        }
      }
    }
    for (int t = tid; t < len0; t += kNbThreads) {
      if (!nb_before(ts, tr, r_sim[t], r_rank[t])) {
        const int slot = atomicAdd(&s_cnt, 1);
        if (slot < kNbCap) { b_sim[slot] = r_sim[t]; b_rank[slot] = r_rank[t]; b_id[slot] = r_id[t]; }
      }
    }
    __syncthreads();
    const int total = s_cnt;
    if (total <= kNbCap) {
      for (int c = tid; c < total; c += kNbThreads) {
        const double s = b_sim[c];
        const int rk = b_rank[c];
        int pos = 0;
        for (int j = 0; j < total; ++j) pos += nb_before(b_sim[j], b_rank[j], s, rk);
        if (pos < k) { r_sim[pos] = s; r_rank[pos] = rk; r_id[pos] = b_id[c]; }
      }
      if (tid == 0) s_len = min(k, total);
      __syncthreads();
    } else {
      // too many keys at the bound: K rounds of "best key after the previous pick" over this chunk and the running list
      for (int t = tid; t < len0; t += kNbThreads) { b_sim[t] = r_sim[t]; b_rank[t] = r_rank[t]; b_id[t] = r_id[t]; }
      if (tid == 0) { s_last_sim = INFINITY; s_last_rank = INT_MAX; }
      __syncthreads();
      for (int got = 0; got < k; ++got) {
        const double ls = s_last_sim;
        const int lr = s_last_rank;
        double ps = -1.0;
        int pr = -1, pid = -1;
        for (int i = tid; i < width; i += kNbThreads) {
          const int n = cnt[i], v = c0 + i;
          if (n > 0 && v != q) {
            const double s = knn_sim(n, shrinkage, nq, norm[v]);
            const int rk = name_rank[v];
            if (nb_before(ls, lr, s, rk) && nb_before(s, rk, ps, pr)) { ps = s; pr = rk; pid = v; }
          }
        }
        for (int t = tid; t < len0; t += kNbThreads) {
          if (nb_before(ls, lr, b_sim[t], b_rank[t]) && nb_before(b_sim[t], b_rank[t], ps, pr)) {
            ps = b_sim[t]; pr = b_rank[t]; pid = b_id[t];
          }
        }
        for (int m = 1; m < 64; m <<= 1) {
          const double os = __shfl_xor(ps, m);
          const int orr = __shfl_xor(pr, m), oid = __shfl_xor(pid, m);
          if (nb_before(os, orr, ps, pr)) { ps = os; pr = orr; pid = oid; }
        }
        if (lane == 0) { w_sim[wave] = ps; w_rank[wave] = pr; w_id[wave] = pid; }
        __syncthreads();
        if (tid == 0) {
          for (int w = 1; w < kNbWaves; ++w)
            if (nb_before(w_sim[w], w_rank[w], ps, pr)) { ps = w_sim[w]; pr = w_rank[w]; pid = w_id[w]; }
          r_sim[got] = ps; r_rank[got] = pr; r_id[got] = pid;
          s_last_sim = ps;
          s_last_rank = pr;
        }
        __syncthreads();
      }
      // every round found a key: this branch runs with more than kNbCap distinct keys at hand and k <= kKnnMaxK < kNbCap
      if (tid == 0) s_len = k;
      __syncthreads();
    }
  }
  const int len = s_len;
  for (int t = tid; t < k; t += kNbThreads) {
    out_ids[(size_t)qi * k + t] = t < len ? r_id[t] : -1;
    out_sims[(size_t)qi * k + t] = t < len ? r_sim[t] : 0.0;
  }
  if (tid == 0) out_len[qi] = len;
}

// mode 0 (UserKNN): nbr_* are lists over users; every training item of each neighbour of u receives its sim.
// mode 1 (ItemKNN): nbr_* are lists over items; for each training item i of u in CSR order, every item of i's list.
__global__ __launch_bounds__(kScThreads) void knn_score_topk_kernel(
    int mode, const int32_t* __restrict__ users, int n_query, const int32_t* __restrict__ r_indptr,
    const int32_t* __restrict__ r_indices, int n_items, const int32_t* __restrict__ nbr_ids,
    const double* __restrict__ nbr_sims, const int32_t* __restrict__ nbr_len, int k_nbr, int k1, int mask_train, double* ws,
    int32_t* __restrict__ out_ids, double* __restrict__ out_scores) {
  __shared__ double b_sc[kScCap];
  __shared__ int b_id[kScCap];
  __shared__ double m_sc[kScThreads];
  __shared__ int m_id[kScThreads];
  __shared__ double t_sc[kKnnMaxK];
  __shared__ int t_id[kKnnMaxK];
  __shared__ int s_cnt, s_thr_id, s_last_id;
  __shared__ double s_thr_sc, s_last_sc;
  __shared__ double w_sc[kScThreads / 64];
  __shared__ int w_id[kScThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_top = k1 - 1;
  double* row = ws + (size_t)blockIdx.x * n_items;

  for (int q = blockIdx.x; q < n_query; q += gridDim.x) {
    const int u = users[q];
    const int p0 = r_indptr[u], p1 = r_indptr[u + 1];
    for (int i = tid; i < n_items; i += kScThreads) row[i] = 0.0;
    __syncthreads();
    if (mode == 0) {
      const int len = nbr_len[u];
      for (int t = 0; t < len; ++t) {
        const int v = nbr_ids[(size_t)u * k_nbr + t];
        const double s = nbr_sims[(size_t)u * k_nbr + t];
        for (int p = r_indptr[v] + tid; p < r_indptr[v + 1]; p += kScThreads) row[r_indices[p]] += s;
        __syncthreads();
      }
    } else {
      for (int p = p0; p < p1; ++p) {
        const int i = r_indices[p];
        const int len = nbr_len[i];
        for (int t = tid; t < len; t += kScThreads) row[nbr_ids[(size_t)i * k_nbr + t]] += nbr_sims[(size_t)i * k_nbr + t];
        __syncthreads();
      }
    }
    if (mask_train)
      for (int p = p0 + tid; p < p1; p += kScThreads) row[r_indices[p]] = kMasked;
    __syncthreads();
    // finish the row (S / (S + 1e-8) where touched; 0 and -10e8 stay) and take each thread's best key
    double bs = -INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < n_items; i += kScThreads) {
      double v = row[i];
      if (v > 0.0) { v = v / (v + 1e-8); row[i] = v; }
      if (sc_before(v, i, bs, bi)) { bs = v; bi = i; }
    }
    m_sc[tid] = bs;
    m_id[tid] = bi;
    if (tid == 0) { s_cnt = 0; s_thr_sc = -INFINITY; s_thr_id = INT_MAX; }
    __syncthreads();
    {
      int pos = 0;
      for (int j = 0; j < kScThreads; ++j) {
        const double os = m_sc[j];
        const int oi = m_id[j];
        pos += sc_before(os, oi, bs, bi) || (os == bs && oi == bi && j < tid);
      }
      if (pos == k1 - 1) { s_thr_sc = bs; s_thr_id = bi; }
    }
    __syncthreads();
    const double ts = s_thr_sc;
    const int ti = s_thr_id;
    for (int i = tid; i < n_items; i += kScThreads) {
      const double v = row[i];
      if (!sc_before(ts, ti, v, i)) {
        const int slot = atomicAdd(&s_cnt, 1);
        if (slot < kScCap) { b_sc[slot] = v; b_id[slot] = i; }
      }
    }
    __syncthreads();
    const int total = s_cnt;
    if (total <= kScCap) {
      for (int c = tid; c < total; c += kScThreads) {
        const double v = b_sc[c];
        const int id = b_id[c];
        int pos = 0;
        for (int j = 0; j < total; ++j) pos += sc_before(b_sc[j], b_id[j], v, id);
        if (pos < k1) { t_sc[pos] = v; t_id[pos] = id; }
      }
    } else {
      if (tid == 0) { s_last_sc = INFINITY; s_last_id = -1; }
      __syncthreads();
      for (int r = 0; r < k1; ++r) {
        const double ls = s_last_sc;
        const int li = s_last_id;
        double ps = -INFINITY;
        int pi = INT_MAX;
        for (int i = tid; i < n_items; i += kScThreads) {
          const double v = row[i];
          if (sc_before(ls, li, v, i) && sc_before(v, i, ps, pi)) { ps = v; pi = i; }
        }
        for (int m = 1; m < 64; m <<= 1) {
          const double os = __shfl_xor(ps, m);
          const int oi = __shfl_xor(pi, m);
          if (sc_before(os, oi, ps, pi)) { ps = os; pi = oi; }
        }
        if (lane == 0) { w_sc[wave] = ps; w_id[wave] = pi; }
        __syncthreads();
        if (tid == 0) {
          for (int w = 1; w < kScThreads / 64; ++w)
            if (sc_before(w_sc[w], w_id[w], ps, pi)) { ps = w_sc[w]; pi = w_id[w]; }
          t_sc[r] = ps;
          t_id[r] = pi;
          s_last_sc = ps;
          s_last_id = pi;
        }
        __syncthreads();
      }
    }
    __syncthreads();
    for (int c = tid; c < n_top; c += kScThreads) {
      int id = t_id[c];
      if (c == 0) {
        bool tie = false;
        for (int j = 1; j < k1; ++j) tie |= (t_sc[j] == t_sc[j - 1]);
        if (tie) id = -1 - id;
      }
      out_ids[(size_t)q * n_top + c] = id;
      out_scores[(size_t)q * n_top + c] = t_sc[c];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" {

srh_status_t srh_knn_neighbours(const int32_t* d_a_indptr, const int32_t* d_a_indices, const int32_t* d_t_indptr,
                                const int32_t* d_t_indices, const double* d_norm, const int32_t* d_name_rank, int64_t n_rows,
                                const int32_t* d_query_rows, int64_t n_query, int32_t k, int32_t shrinkage,
                                int32_t* d_out_ids, double* d_out_sims, int32_t* d_out_len, void* stream) {
  SRH_REQUIRE(d_a_indptr && d_a_indices && d_t_indptr && d_t_indices && d_norm && d_name_rank && d_out_ids && d_out_sims &&
                  d_out_len, "knn_neighbours: null argument");
  SRH_REQUIRE(k >= 1 && k <= kKnnMaxK, "knn_neighbours: topK = %d outside [1, %d] (the lists are kept in LDS)", (int)k,
              kKnnMaxK);
  SRH_REQUIRE(shrinkage >= 0, "knn_neighbours: negative shrinkage %d", (int)shrinkage);
  SRH_REQUIRE(n_rows >= 1 && n_rows < INT_MAX, "knn_neighbours: bad row count");
  SRH_REQUIRE(n_query >= 1 && n_query < INT_MAX, "knn_neighbours: bad query count");
  SRH_REQUIRE(d_query_rows || n_query == n_rows, "knn_neighbours: without query rows, n_query must equal n_rows");
  static bool lds_set = false;
  if (!lds_set) {
    SRH_HIP(hipFuncSetAttribute((const void*)knn_neighbours_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNbLds));
    lds_set = true;
  }
  knn_neighbours_kernel<<<(unsigned)n_query, kNbThreads, kNbLds, srh::as_stream(stream)>>>(
      d_a_indptr, d_a_indices, d_t_indptr, d_t_indices, d_norm, d_name_rank, (int)n_rows, d_query_rows, k, shrinkage,
      d_out_ids, d_out_sims, d_out_len);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_knn_score_ws_bytes(int64_t ws_rows, int64_t n_items) {
  return (ws_rows > 0 && n_items > 0) ? ws_rows * n_items * (int64_t)sizeof(double) : 0;
}

srh_status_t srh_knn_score_topk(int32_t mode, const int32_t* d_users, int64_t n_query, const int32_t* d_r_indptr,
                                const int32_t* d_r_indices, int64_t n_items, const int32_t* d_nbr_ids,
                                const double* d_nbr_sims, const int32_t* d_nbr_len, int32_t k_nbr, int32_t n_top,
                                int32_t mask_train, void* d_ws, int64_t ws_rows, int32_t* d_out_ids, double* d_out_scores,
                                void* stream) {
  SRH_REQUIRE(d_users && d_r_indptr && d_r_indices && d_nbr_ids && d_nbr_sims && d_nbr_len && d_ws && d_out_ids &&
                  d_out_scores, "knn_score_topk: null argument");
  SRH_REQUIRE(mode == 0 || mode == 1, "knn_score_topk: mode %d (0: UserKNN, 1: ItemKNN)", (int)mode);
  SRH_REQUIRE(k_nbr >= 1 && k_nbr <= kKnnMaxK, "knn_score_topk: topK = %d outside [1, %d]", (int)k_nbr, kKnnMaxK);
  SRH_REQUIRE(n_items >= 1 && n_items < INT_MAX && n_query >= 1 && n_query < INT_MAX, "knn_score_topk: bad shape");
  SRH_REQUIRE(n_top >= 1 && n_top + 1 <= kKnnMaxK && n_top + 1 <= n_items,
              "knn_score_topk: N = %d needs N + 1 <= min(%d, n_items = %lld)", (int)n_top, kKnnMaxK, (long long)n_items);
  SRH_REQUIRE(ws_rows >= 1, "knn_score_topk: ws_rows must be >= 1");
  const int64_t grid = n_query < ws_rows ? n_query : ws_rows;
  SRH_REQUIRE(grid < INT_MAX, "knn_score_topk: too many workspace rows");
  knn_score_topk_kernel<<<(unsigned)grid, kScThreads, 0, srh::as_stream(stream)>>>(
      mode, d_users, (int)n_query, d_r_indptr, d_r_indices, (int)n_items, d_nbr_ids, d_nbr_sims, d_nbr_len, k_nbr,
      n_top + 1, mask_train != 0, static_cast<double*>(d_ws), d_out_ids, d_out_scores);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // extern "C"

// NCL (reference model/graph/NCL.py): the k-means of the E-step.  DESIGN.md 4.6.  The structure-contrastive loss of
// batch rows against a whole table (srh_table_nce_fwd_bwd) is the shared two-pass kernel of contrastive.hip.
//
// k-means (srh_kmeans_assign_f32 / srh_kmeans_update_f32, NCL.py:29-44 e_step / run_kmeans):
//   assign  argmin_j |c_j|^2 - 2 x.c_j fused into the f32 MFMA product over centroid tiles (lowest j on ties)
//   update  stable counting sort of the rows by cluster, then each cluster sums its rows in ascending row order
#include <cmath>

#include "rowtile.h"

namespace {

using namespace srh;

constexpr int kKmRows = kRtRows;    // rows per assign workgroup (16 per wave)
constexpr int kKmCTile = kRtRows;   // centroids staged in LDS per iteration

// ---- k-means assign ------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void km_assign(const float* __restrict__ x, int64_t n, const float* __restrict__ c,
                                                 int64_t k, int32_t* __restrict__ out_ids, float* __restrict__ out_dist) {
  constexpr int LDS_STRIDE = kRtStride<D>;
  __shared__ float cs[kKmCTile * LDS_STRIDE];
  __shared__ float cn2[kKmCTile];
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int64_t r = (int64_t)blockIdx.x * kKmRows + L.wave * 16 + j16;
  const bool rok = r < n;
  float rf[D / 4];
  float xx = 0.f;
#pragma unroll
  for (int s = 0; s < D / 4; ++s) {
    rf[s] = rok ? x[r * D + 4 * s + g] : 0.f;
    xx = fmaf(rf[s], rf[s], xx);
  }
  xx = sum4(xx);
  float best = INFINITY;
  int32_t best_j = 0x7fffffff;
  for (int64_t c0 = 0; c0 < k; c0 += kKmCTile) {
    __syncthreads();
    stage_tile<D>(cs, c, c0, k);
    __syncthreads();
    if (threadIdx.x < kKmCTile) {
      float s2 = 0.f;
      for (int v = 0; v < D; ++v) s2 = fmaf(cs[threadIdx.x * LDS_STRIDE + v], cs[threadIdx.x * LDS_STRIDE + v], s2);
      cn2[threadIdx.x] = c0 + threadIdx.x < k ? s2 : INFINITY;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kKmCTile / 16; ++sub) {
      const f32x4 s = score16<D>(cs, sub, j16, g, rf);
      // this lane's centroids come in ascending j: a strict < keeps the lowest j of equal distances
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ci = sub * 16 + 4 * g + reg;
        const float dist = fmaf(-2.f, s[reg], cn2[ci]);
        if (dist < best) {
          best = dist;
          best_j = (int32_t)(c0 + ci);
        }
      }
    }
  }
#pragma unroll
  for (int m = 16; m <= 32; m <<= 1) {
    const float ob = __shfl_xor(best, m);
    const int32_t oj = __shfl_xor(best_j, m);
    if (ob < best || (ob == best && oj < best_j)) {
      best = ob;
      best_j = oj;
    }
  }
  if (rok && g == 0) {
    out_ids[r] = best_j;
    out_dist[r] = fmaxf(xx + best, 0.f);
  }
}

// ---- k-means update: stable counting sort by cluster, then ascending-row sums ---------------------------------------
constexpr int kKmChunk = 256;

struct KmWs {
  int32_t* chunk_cnt;  // chunks x k: rows of cluster j in chunk c, then the exclusive prefix over chunks
  int32_t* rank;       // n: rank of the row among the earlier rows of its cluster in its chunk
  int32_t* start;      // k: first slot of cluster j in `order`
  int32_t* order;      // n: row ids sorted by cluster, ascending within a cluster
};

constexpr int64_t km_chunks(int64_t n) { return ceil_div(n, kKmChunk); }

// null ws measures, a workspace carves; returns the bytes
int64_t km_layout(KmWs& w, void* ws, int64_t n, int64_t k) {
  Carver c(ws);
  c.take(w.chunk_cnt, km_chunks(n) * k);
  c.take(w.rank, n);
  c.take(w.start, k);
  c.take(w.order, n);
  return c.used;
}

__device__ __forceinline__ bool km_valid(int32_t id, int64_t k) { return id >= 0 && (int64_t)id < k; }

__global__ __launch_bounds__(kKmChunk) void km_rank(const int32_t* __restrict__ ids, int64_t n, int64_t k, KmWs w) {
  __shared__ int32_t sid[kKmChunk];
  const int64_t row = (int64_t)blockIdx.x * kKmChunk + threadIdx.x;
  const int32_t my = row < n ? ids[row] : -1;
  sid[threadIdx.x] = my;
  __syncthreads();
  if (row >= n || !km_valid(my, k)) return;
  int32_t before = 0, after = 0;
  for (int i = 0; i < kKmChunk; ++i) {
    const int32_t o = sid[i];
    before += (i < (int)threadIdx.x) & (o == my);
    after += (i > (int)threadIdx.x) & (o == my);
  }
  w.rank[row] = before;
  if (after == 0) w.chunk_cnt[(int64_t)blockIdx.x * k + my] = before + 1;  // (the last row of its cluster in the chunk)
}

__global__ __launch_bounds__(256) void km_prefix(int64_t n, int64_t k, KmWs w, int32_t* __restrict__ counts) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= k) return;
  const int64_t chunks = km_chunks(n);
  int32_t run = 0;
  for (int64_t c = 0; c < chunks; ++c) {
    const int32_t v = w.chunk_cnt[c * k + j];
    w.chunk_cnt[c * k + j] = run;
    run += v;
  }
  counts[j] = run;
}

__global__ __launch_bounds__(1024) void km_scan(int64_t k, KmWs w, const int32_t* __restrict__ counts) {
  __shared__ int32_t part[1024];
  const int64_t per = (k + 1023) / 1024;
  const int64_t lo = threadIdx.x * per, hi = lo + per < k ? lo + per : k;
  int32_t s = 0;
  for (int64_t j = lo; j < hi; ++j) s += counts[j];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int32_t v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int32_t run = part[threadIdx.x] - s;
  for (int64_t j = lo; j < hi; ++j) {
    w.start[j] = run;
    run += counts[j];
  }
}

__global__ __launch_bounds__(256) void km_place(const int32_t* __restrict__ ids, int64_t n, int64_t k, KmWs w) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const int32_t id = ids[row];
  if (!km_valid(id, k)) return;
  const int64_t chunk = row / kKmChunk;
  w.order[w.start[id] + w.chunk_cnt[chunk * k + id] + w.rank[row]] = (int32_t)row;
}

// one wave per cluster, a column per lane: the rows of the cluster in ascending order, 8 loads in flight
__global__ __launch_bounds__(256) void km_sum(const float* __restrict__ x, int64_t k, int32_t d, KmWs w,
                                              const int32_t* __restrict__ counts, float* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= k) return;
  const int32_t cnt = counts[j];
  const int32_t* rows = w.order + w.start[j];
  const float inv = cnt > 0 ? 1.f / (float)cnt : 0.f;
  for (int col = lane; col < d; col += 64) {
    float s = 0.f;
    int32_t p = 0;
    for (; p + 8 <= cnt; p += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = x[(int64_t)rows[p + u] * d + col];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; p < cnt; ++p) s += x[(int64_t)rows[p] * d + col];
    out[j * d + col] = s * inv;
  }
}

}  // namespace

extern "C" {

srh_status_t srh_kmeans_assign_f32(const float* d_x, int64_t n, const float* d_c, int64_t k, int32_t d, int32_t* d_out_ids,
                                   float* d_out_dist, void* stream) {
  SRH_REQUIRE(d_x && d_c && d_out_ids && d_out_dist, "kmeans_assign: null argument");
  SRH_REQUIRE(n > 0 && k > 0 && k < (int64_t(1) << 31), "kmeans_assign: bad n / k");
  SRH_REQUIRE(d == 64 || d == 128, "kmeans_assign: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  hipStream_t st = srh::as_stream(stream);
  const unsigned grid = (unsigned)((n + kKmRows - 1) / kKmRows);
  if (d == 64) km_assign<64><<<grid, 256, 0, st>>>(d_x, n, d_c, k, d_out_ids, d_out_dist);
  else km_assign<128><<<grid, 256, 0, st>>>(d_x, n, d_c, k, d_out_ids, d_out_dist);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_kmeans_update_ws_bytes(int64_t n, int64_t k) {
  if (n <= 0 || k <= 0) return 0;
  KmWs w;
  return km_layout(w, nullptr, n, k);
}

srh_status_t srh_kmeans_update_f32(const float* d_x, int64_t n, const int32_t* d_ids, int64_t k, int32_t d,
                                   float* d_out_centroids, int32_t* d_out_counts, void* d_ws, void* stream) {
  SRH_REQUIRE(d_x && d_ids && d_out_centroids && d_out_counts && d_ws, "kmeans_update: null argument");
  SRH_REQUIRE(n > 0 && n < (int64_t(1) << 31) && k > 0 && k < (int64_t(1) << 31) && d > 0, "kmeans_update: bad n / k / d");
  hipStream_t st = srh::as_stream(stream);
  KmWs w;
  km_layout(w, d_ws, n, k);
  SRH_HIP(hipMemsetAsync(w.chunk_cnt, 0, 4 * km_chunks(n) * k, st));
  km_rank<<<(unsigned)km_chunks(n), kKmChunk, 0, st>>>(d_ids, n, k, w);
  SRH_LAUNCH_CHECK();
  km_prefix<<<(unsigned)((k + 255) / 256), 256, 0, st>>>(n, k, w, d_out_counts);
  SRH_LAUNCH_CHECK();
  km_scan<<<1, 1024, 0, st>>>(k, w, d_out_counts);
  SRH_LAUNCH_CHECK();
  km_place<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_ids, n, k, w);
  SRH_LAUNCH_CHECK();
  km_sum<<<(unsigned)((k + 3) / 4), 256, 0, st>>>(d_x, k, d, w, d_out_counts, d_out_centroids);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // extern "C"

// NCL (reference model/graph/NCL.py): the structure-contrastive loss of batch rows against a whole table, and the
// k-means of the E-step.  DESIGN.md 4.6.
//
// Table InfoNCE (srh_table_nce_fwd_bwd, NCL.py:57-83 ssl_layer_loss).  Per problem: queries Q (B x D), table T (N x D),
// idx (B, the positive row of each query in T).  q = normalize(Q_b), t = normalize(T_j) (F.normalize: x / max(|x|, 1e-12))
//   loss = sum_b [ -q_b.t_idx[b] / tau + log sum_j exp(q_b.t_j / tau) ]
// The B x N logits are never materialised.  The rows are unit vectors, so every logit is <= 1/tau and the exponentials
// are taken as exp((s - 1) / tau): no running max.
//   prep    normalise Q and T into the workspace (rows and their norms)
//   pass 1  query tiles x key chunks: per query and chunk, sum_j e_bj and sum_j e_bj t_j (e = exp((s - 1)/tau))
//   finish  per query: the chunk partials in chunk order -> row sum, loss term, dL/dQ (normalisation backward fused)
//   pass 2  key tiles x all queries: dT_j = (1/tau) sum_b (P_bj - [idx_b == j]) q_b, P = e / rowsum (normalisation
//           backward fused); each key tile owns its rows of dT
//   sum     the per-query loss terms in a fixed order
// All four products run on v_mfma_f32_16x16x4_f32.  No float atomics anywhere: every output element is produced by one
// lane in a fixed order, so a call returns the same bits every time.
//
// Both passes are one kernel: a workgroup holds 64 "R" rows (16 per wave) in registers and streams "C" rows through LDS.
//   S^T[c][r] = Cn_c . Rn_r                       (MFMA 1: A = C tile from LDS, B = R rows from registers)
//   W[c][r]   = weight(S^T[c][r])                 (on the accumulator, in place)
//   O^T[:, r] += sum_c Cn_c W[c][r]               (MFMA 2: the accumulator of MFMA 1 is its B operand, no lane movement;
//                                                  the c order inside a k-step is 4*(lane>>4) + reg, matched by A)
// pass 1: R = queries, C = keys,    W = e             -> O = sum_j e_bj t_j, and the row sums of W
// pass 2: R = keys,    C = queries, W = e/rowsum - [idx == key]  -> O = tau * dL/dt
//
// k-means (srh_kmeans_assign_f32 / srh_kmeans_update_f32, NCL.py:29-44 e_step / run_kmeans):
//   assign  argmin_j |c_j|^2 - 2 x.c_j fused into the f32 MFMA product over centroid tiles (lowest j on ties)
//   update  stable counting sort of the rows by cluster, then each cluster sums its rows in ascending row order
#include <algorithm>
#include <cmath>

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTnWaves = 4;                 // waves per workgroup; each owns 16 R rows
constexpr int kTnRows = 16 * kTnWaves;      // R rows per workgroup
constexpr int kTnCTile = 64;                // C rows staged in LDS per iteration
constexpr int kTnMaxProblems = 2;
constexpr int kTnPass1Target = 512;         // pass-1 workgroups aimed for per problem (query tiles x key chunks)
constexpr float kNormEps = 1e-12f;

inline int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

struct TnProblem {
  const float* q;
  const float* t;
  const int32_t* idx;
  int64_t B, N;
  float scale;
  double* loss;
  float* gq;
  float* gt;
  // workspace
  float* qn;        // B x D  normalised queries
  float* qnorm;     // B      |Q_b|
  float* tn;        // N x D  normalised table
  float* tnorm;     // N      |T_j|
  float* part_o;    // chunks x B x D  sum_j e_bj t_j per key chunk
  double* part_rs;  // chunks x B      sum_j e_bj per key chunk
  float* inv_rs;    // B      1 / rowsum
  double* row_loss; // B
  int64_t chunks, chunk_len;
};

struct TnArgs {
  TnProblem p[kTnMaxProblems];
  float inv_tau;
};

// pass-1 key chunks of a problem: a pure function of (B, N), so the workspace query and the launch agree and every
// call sums in the same order
inline int64_t tn_chunks(int64_t B, int64_t N) {
  const int64_t rtiles = (B + kTnRows - 1) / kTnRows;
  const int64_t ctiles = (N + kTnCTile - 1) / kTnCTile;
  int64_t c = (kTnPass1Target + rtiles - 1) / rtiles;
  if (c > ctiles) c = ctiles;
  return c < 1 ? 1 : c;
}
inline int64_t tn_chunk_len(int64_t B, int64_t N) {
  const int64_t c = tn_chunks(B, N);
  const int64_t per = (N + c - 1) / c;
  return (per + kTnCTile - 1) / kTnCTile * kTnCTile;
}

inline int64_t tn_ws_bytes(int64_t B, int64_t N, int D) {
  const int64_t c = tn_chunks(B, N);
  return align256(4 * B * D) + align256(4 * B) + align256(4 * N * D) + align256(4 * N) + align256(4 * c * B * D) +
         align256(8 * c * B) + align256(4 * B) + align256(8 * B);
}

void tn_carve(TnProblem& p, char* ws, int D) {
  char* cur = ws;
  auto take = [&](int64_t bytes) { char* r = cur; cur += align256(bytes); return r; };
  p.chunks = tn_chunks(p.B, p.N);
  p.chunk_len = tn_chunk_len(p.B, p.N);
  p.qn = (float*)take(4 * p.B * D);
  p.qnorm = (float*)take(4 * p.B);
  p.tn = (float*)take(4 * p.N * D);
  p.tnorm = (float*)take(4 * p.N);
  p.part_o = (float*)take(4 * p.chunks * p.B * D);
  p.part_rs = (double*)take(8 * p.chunks * p.B);
  p.inv_rs = (float*)take(4 * p.B);
  p.row_loss = (double*)take(8 * p.B);
}

// d(normalize(x))/dx applied to g: (g - y (y.g)) / |x| where |x| >= eps, g / eps below it (F.normalize's clamp_min)
__device__ __forceinline__ float norm_bwd_scale(float nrm) { return 1.f / fmaxf(nrm, kNormEps); }

// ---- prep: normalise rows (LPR = D/4 lanes per row, one float4 each) ------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void tn_prep(TnArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const TnProblem& P = a.p[blockIdx.y >> 1];
  const bool table = blockIdx.y & 1;
  const int64_t rows = table ? P.N : P.B;
  const float* src = table ? P.t : P.q;
  float* dst = table ? P.tn : P.qn;
  float* nrm_out = table ? P.tnorm : P.qnorm;
  const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  const bool ok = row < rows;
  const float4 v = ok ? reinterpret_cast<const float4*>(src + row * D)[lane] : srh::f4_zero();
  const float ss = srh::group_sum<LPR>(srh::f4_dot(v, v));
  const float nrm = sqrtf(ss);
  const float den = fmaxf(nrm, kNormEps);
  if (ok) {
    reinterpret_cast<float4*>(dst + row * D)[lane] = make_float4(v.x / den, v.y / den, v.z / den, v.w / den);
    if (lane == 0) nrm_out[row] = nrm;
  }
}

// ---- the two passes ------------------------------------------------------------------------------------------------
template <int D, bool PASS2>
__global__ __launch_bounds__(256) void tn_pass(TnArgs a) {
  constexpr int LDS_STRIDE = D + 4;  // rows 4 floats apart in bank space: both LDS read patterns are conflict-free
  __shared__ float cs[kTnCTile * LDS_STRIDE];
  __shared__ float cw[kTnCTile];
  __shared__ int32_t cid[kTnCTile];
  const TnProblem& P = a.p[blockIdx.y];
  const int64_t nR = PASS2 ? P.N : P.B;
  const float* Rn = PASS2 ? P.tn : P.qn;
  const float* Cn = PASS2 ? P.qn : P.tn;
  const int64_t rtiles = (nR + kTnRows - 1) / kTnRows;
  const int64_t rtile = PASS2 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x / P.chunks;
  const int64_t chunk = PASS2 ? 0 : (int64_t)blockIdx.x % P.chunks;
  if (rtile >= rtiles) return;
  int64_t cbeg = 0, cend = P.B;
  if (!PASS2) {
    cbeg = chunk * P.chunk_len;
    cend = cbeg + P.chunk_len < P.N ? cbeg + P.chunk_len : P.N;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int64_t r = rtile * kTnRows + wave * 16 + j16;
  const bool rok = r < nR;
  const float inv_tau = a.inv_tau;

  float rf[D / 4];  // B operand of MFMA 1: Rn[r][4s + g]
#pragma unroll
  for (int s = 0; s < D / 4; ++s) rf[s] = rok ? Rn[r * D + 4 * s + g] : 0.f;
  f32x4 o[D / 16];
#pragma unroll
  for (int b = 0; b < D / 16; ++b) o[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  double rs = 0.0;

  for (int64_t c0 = cbeg; c0 < cend; c0 += kTnCTile) {
    __syncthreads();
    for (int e = threadIdx.x; e < kTnCTile * (D / 4); e += 256) {
      const int i = e / (D / 4), v = e % (D / 4);
      const int64_t c = c0 + i;
      const float4 x = c < cend ? reinterpret_cast<const float4*>(Cn + c * D)[v] : srh::f4_zero();
      *reinterpret_cast<float4*>(&cs[i * LDS_STRIDE + 4 * v]) = x;
    }
    if (threadIdx.x < kTnCTile) {
      const int64_t c = c0 + threadIdx.x;
      const bool cok = c < cend;
      if (PASS2) {
        cw[threadIdx.x] = cok ? P.inv_rs[c] : 0.f;
        cid[threadIdx.x] = cok ? P.idx[c] : -1;
      } else {
        cw[threadIdx.x] = cok ? 1.f : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kTnCTile / 16; ++sub) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      const float* arow = &cs[(sub * 16 + j16) * LDS_STRIDE + g];
#pragma unroll
      for (int k = 0; k < D / 4; ++k) s = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * k], rf[k], s, 0, 0, 0);
      // s[reg] = S^T[c = sub*16 + 4g + reg][r]
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ci = sub * 16 + 4 * g + reg;
        float w = expf((s[reg] - 1.f) * inv_tau) * cw[ci];
        if (PASS2) {
          if ((int64_t)cid[ci] == r) w -= 1.f;
        } else {
          rs += (double)w;
        }
        s[reg] = w;
      }
#pragma unroll
      for (int b = 0; b < D / 16; ++b) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          o[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(cs[(sub * 16 + 4 * g + reg) * LDS_STRIDE + 16 * b + j16], s[reg], o[b],
                                                      0, 0, 0);
      }
    }
  }
  // o[b][reg] = O[r][16b + 4g + reg]
  if (!PASS2) {
    rs += __shfl_xor(rs, 16);
    rs += __shfl_xor(rs, 32);
    if (!rok) return;
    const int64_t row = chunk * P.B + r;
    if (g == 0) P.part_rs[row] = rs;
#pragma unroll
    for (int b = 0; b < D / 16; ++b)
      reinterpret_cast<float4*>(P.part_o + row * D + 16 * b + 4 * g)[0] = make_float4(o[b][0], o[b][1], o[b][2], o[b][3]);
  } else {
    // dL/dt_j = scale / tau * O_j; then the normalisation backward of row j
    const float k = P.scale * inv_tau;
    float4 tv[D / 16];
    float dot = 0.f;
#pragma unroll
    for (int b = 0; b < D / 16; ++b) {
      tv[b] = rok ? reinterpret_cast<const float4*>(P.tn + r * D + 16 * b + 4 * g)[0] : srh::f4_zero();
      o[b] *= k;
      dot = fmaf(tv[b].x, o[b][0], fmaf(tv[b].y, o[b][1], fmaf(tv[b].z, o[b][2], fmaf(tv[b].w, o[b][3], dot))));
    }
    dot += __shfl_xor(dot, 16);
    dot += __shfl_xor(dot, 32);
    if (!rok) return;
    const float nrm = P.tnorm[r];
    const float inv = norm_bwd_scale(nrm);
    const bool clamped = !(nrm > kNormEps);
#pragma unroll
    for (int b = 0; b < D / 16; ++b) {
      float4 out;
      if (clamped) {
        out = make_float4(o[b][0] * inv, o[b][1] * inv, o[b][2] * inv, o[b][3] * inv);
      } else {
        out = make_float4((o[b][0] - tv[b].x * dot) * inv, (o[b][1] - tv[b].y * dot) * inv,
                          (o[b][2] - tv[b].z * dot) * inv, (o[b][3] - tv[b].w * dot) * inv);
      }
      reinterpret_cast<float4*>(P.gt + r * D + 16 * b + 4 * g)[0] = out;
    }
  }
}

// ---- per-query finish: chunk partials in chunk order -> row sum, loss term, dL/dQ -----------------------------------
template <int D>
__global__ __launch_bounds__(256) void tn_finish(TnArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const TnProblem& P = a.p[blockIdx.y];
  const int64_t b = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  if (b >= P.B) return;  // (whole row groups leave together: group_sum stays within live lanes)
  double rs = 0.0;
  float4 o = srh::f4_zero();
  for (int64_t c = 0; c < P.chunks; ++c) {
    rs += P.part_rs[c * P.B + b];
    o = srh::f4_add(o, reinterpret_cast<const float4*>(P.part_o + (c * P.B + b) * D)[lane]);
  }
  const int32_t j = P.idx[b];
  const bool jok = j >= 0 && (int64_t)j < P.N;  // (an index outside the table reads nothing and makes the loss NaN)
  const float4 q = reinterpret_cast<const float4*>(P.qn + b * D)[lane];
  const float4 t = jok ? reinterpret_cast<const float4*>(P.tn + (int64_t)j * D)[lane] : srh::f4_zero();
  const float spos = srh::group_sum<LPR>(srh::f4_dot(q, t));
  const float inv_rs = (float)(1.0 / rs);
  const float inv_tau = a.inv_tau;
  if (lane == 0) {
    P.inv_rs[b] = inv_rs;
    P.row_loss[b] = jok ? (double)inv_tau * (1.0 - (double)spos) + log(rs) : (double)NAN;
  }
  // dL/dq_b = scale / tau * (O_b / rowsum - t_idx[b])
  const float k = P.scale * inv_tau;
  float4 gq = make_float4(k * (o.x * inv_rs - t.x), k * (o.y * inv_rs - t.y), k * (o.z * inv_rs - t.z),
                          k * (o.w * inv_rs - t.w));
  const float dot = srh::group_sum<LPR>(srh::f4_dot(q, gq));
  const float nrm = P.qnorm[b];
  const float inv = norm_bwd_scale(nrm);
  if (nrm > kNormEps) gq = make_float4(gq.x - q.x * dot, gq.y - q.y * dot, gq.z - q.z * dot, gq.w - q.w * dot);
  reinterpret_cast<float4*>(P.gq + b * D)[lane] = srh::f4_scale(gq, inv);
}

// ---- the loss: per-query terms summed in a fixed order, one workgroup per problem ----------------------------------
__global__ __launch_bounds__(256) void tn_loss(TnArgs a) {
  __shared__ double part[256];
  const TnProblem& P = a.p[blockIdx.x];
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < P.B; b += 256) s += P.row_loss[b];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) P.loss[0] = (double)P.scale * part[0];
}

template <int D>
srh_status_t launch_table_nce(TnArgs& a, int np, hipStream_t st) {
  int64_t max_prep = 0, max_p1 = 0, max_fin = 0, max_p2 = 0;
  constexpr int RPB = 256 / (D / 4);
  for (int k = 0; k < np; ++k) {
    const TnProblem& p = a.p[k];
    const int64_t big = p.N > p.B ? p.N : p.B;
    max_prep = std::max(max_prep, (big + RPB - 1) / RPB);
    max_p1 = std::max(max_p1, (p.B + kTnRows - 1) / kTnRows * p.chunks);
    max_fin = std::max(max_fin, (p.B + RPB - 1) / RPB);
    max_p2 = std::max(max_p2, (p.N + kTnRows - 1) / kTnRows);
  }
  tn_prep<D><<<dim3((unsigned)max_prep, 2 * np), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_pass<D, false><<<dim3((unsigned)max_p1, np), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_finish<D><<<dim3((unsigned)max_fin, np), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_pass<D, true><<<dim3((unsigned)max_p2, np), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_loss<<<np, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

// ---- k-means assign ------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void km_assign(const float* __restrict__ x, int64_t n, const float* __restrict__ c,
                                                 int64_t k, int32_t* __restrict__ out_ids, float* __restrict__ out_dist) {
  constexpr int LDS_STRIDE = D + 4;
  __shared__ float cs[kTnCTile * LDS_STRIDE];
  __shared__ float cn2[kTnCTile];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int64_t r = (int64_t)blockIdx.x * kTnRows + wave * 16 + j16;
  const bool rok = r < n;
  float rf[D / 4];
  float xx = 0.f;
#pragma unroll
  for (int s = 0; s < D / 4; ++s) {
    rf[s] = rok ? x[r * D + 4 * s + g] : 0.f;
    xx = fmaf(rf[s], rf[s], xx);
  }
  xx += __shfl_xor(xx, 16);
  xx += __shfl_xor(xx, 32);
  float best = INFINITY;
  int32_t best_j = 0x7fffffff;
  for (int64_t c0 = 0; c0 < k; c0 += kTnCTile) {
    __syncthreads();
    for (int e = threadIdx.x; e < kTnCTile * (D / 4); e += 256) {
      const int i = e / (D / 4), v = e % (D / 4);
      const int64_t cj = c0 + i;
      const float4 y = cj < k ? reinterpret_cast<const float4*>(c + cj * D)[v] : srh::f4_zero();
      *reinterpret_cast<float4*>(&cs[i * LDS_STRIDE + 4 * v]) = y;
    }
    __syncthreads();
    if (threadIdx.x < kTnCTile) {
      float s2 = 0.f;
      for (int v = 0; v < D; ++v) s2 = fmaf(cs[threadIdx.x * LDS_STRIDE + v], cs[threadIdx.x * LDS_STRIDE + v], s2);
      cn2[threadIdx.x] = c0 + threadIdx.x < k ? s2 : INFINITY;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kTnCTile / 16; ++sub) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      const float* arow = &cs[(sub * 16 + j16) * LDS_STRIDE + g];
#pragma unroll
      for (int q = 0; q < D / 4; ++q) s = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * q], rf[q], s, 0, 0, 0);
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

__host__ __device__ inline int64_t km_chunks(int64_t n) { return (n + kKmChunk - 1) / kKmChunk; }

inline int64_t km_ws_bytes(int64_t n, int64_t k) {
  return align256(4 * km_chunks(n) * k) + align256(4 * n) + align256(4 * k) + align256(4 * n);
}

KmWs km_carve(char* ws, int64_t n, int64_t k) {
  KmWs w;
  char* cur = ws;
  auto take = [&](int64_t bytes) { char* r = cur; cur += align256(bytes); return r; };
  w.chunk_cnt = (int32_t*)take(4 * km_chunks(n) * k);
  w.rank = (int32_t*)take(4 * n);
  w.start = (int32_t*)take(4 * k);
  w.order = (int32_t*)take(4 * n);
  return w;
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

int64_t srh_table_nce_ws_bytes(int64_t B, int64_t N, int32_t d) {
  if (B <= 0 || N <= 0 || (d != 64 && d != 128)) return 0;
  return tn_ws_bytes(B, N, d);
}

srh_status_t srh_table_nce_fwd_bwd(const srh_table_nce_problem_t* problems, int32_t n_problems, int32_t d, float tau,
                                   void* d_ws, void* stream) {
  SRH_REQUIRE(problems && d_ws, "table_nce_fwd_bwd: null argument");
  SRH_REQUIRE(n_problems >= 1 && n_problems <= kTnMaxProblems, "table_nce_fwd_bwd: 1..%d problems per call",
              kTnMaxProblems);
  SRH_REQUIRE(d == 64 || d == 128, "table_nce_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(tau > 0.f && std::isfinite(tau), "table_nce_fwd_bwd: temperature must be positive");
  TnArgs a{};
  a.inv_tau = 1.f / tau;
  char* ws = static_cast<char*>(d_ws);
  for (int k = 0; k < n_problems; ++k) {
    const srh_table_nce_problem_t& s = problems[k];
    SRH_REQUIRE(s.d_q && s.d_t && s.d_idx && s.d_loss && s.d_gq && s.d_gt, "table_nce_fwd_bwd: null tensor in problem %d", k);
    SRH_REQUIRE(s.B > 0 && s.B < (int64_t(1) << 31) && s.N > 0 && s.N < (int64_t(1) << 31),
                "table_nce_fwd_bwd: bad B / N in problem %d", k);
    TnProblem& p = a.p[k];
    p.q = s.d_q; p.t = s.d_t; p.idx = s.d_idx; p.B = s.B; p.N = s.N; p.scale = s.loss_scale;
    p.loss = s.d_loss; p.gq = s.d_gq; p.gt = s.d_gt;
    tn_carve(p, ws, d);
    ws += tn_ws_bytes(s.B, s.N, d);
  }
  hipStream_t st = srh::as_stream(stream);
  return d == 64 ? launch_table_nce<64>(a, n_problems, st) : launch_table_nce<128>(a, n_problems, st);
}

srh_status_t srh_kmeans_assign_f32(const float* d_x, int64_t n, const float* d_c, int64_t k, int32_t d, int32_t* d_out_ids,
                                   float* d_out_dist, void* stream) {
  SRH_REQUIRE(d_x && d_c && d_out_ids && d_out_dist, "kmeans_assign: null argument");
  SRH_REQUIRE(n > 0 && k > 0 && k < (int64_t(1) << 31), "kmeans_assign: bad n / k");
  SRH_REQUIRE(d == 64 || d == 128, "kmeans_assign: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  hipStream_t st = srh::as_stream(stream);
  const unsigned grid = (unsigned)((n + kTnRows - 1) / kTnRows);
  if (d == 64) km_assign<64><<<grid, 256, 0, st>>>(d_x, n, d_c, k, d_out_ids, d_out_dist);
  else km_assign<128><<<grid, 256, 0, st>>>(d_x, n, d_c, k, d_out_ids, d_out_dist);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_kmeans_update_ws_bytes(int64_t n, int64_t k) {
  if (n <= 0 || k <= 0) return 0;
  return km_ws_bytes(n, k);
}

srh_status_t srh_kmeans_update_f32(const float* d_x, int64_t n, const int32_t* d_ids, int64_t k, int32_t d,
                                   float* d_out_centroids, int32_t* d_out_counts, void* d_ws, void* stream) {
  SRH_REQUIRE(d_x && d_ids && d_out_centroids && d_out_counts && d_ws, "kmeans_update: null argument");
  SRH_REQUIRE(n > 0 && n < (int64_t(1) << 31) && k > 0 && k < (int64_t(1) << 31) && d > 0, "kmeans_update: bad n / k / d");
  hipStream_t st = srh::as_stream(stream);
  KmWs w = km_carve(static_cast<char*>(d_ws), n, k);
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

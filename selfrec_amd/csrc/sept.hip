// SEPT (model/graph/SEPT.py of the reference): the row L2-normalise behind every propagation of its four encoders, and
// the tri-training neighbour discrimination of a step (label_prediction -> top_k -> neighbor_discrimination,
// SEPT.py:98-134) with no n x n matrix in memory and no float atomics.  DESIGN.md 4.14.
//
// Views V0 (friend), V1 (sharing), V2 (rec) and A (aug), each n x D; v = normalize(V), a = normalize(A) under
// x * rsqrt(max(sum x^2, 1e-12)) (tf.nn.l2_normalize).
//   s_v[i][j] = v_i . a_j,  p_v[i][j] = softmax_j(s_v[i][.])  (temperature 1, diagonal included)
//   pos_v[i]  = top-k over j of p_a[i][j] + p_b[i][j], (a, b) the two views other than v; value descending, ties to the
//               lowest j.  (The reference halves the sum: exact and monotone, so the sum ranks.)
//   loss_v    = scale sum_i [ log sum_j e_v[i][j] - log sum_{j in pos_v[i]} e_v[i][j] ],  e = exp(s / tau)
// Unit rows: every exponential is taken as exp((s - 1) / .), no running max (contrastive.hip's convention).
//   prep     normalise the four matrices into the workspace (rows and 1/norm)
//   pass 1   view-row tiles x key chunks: per view, row and chunk, sum_j exp(s - 1) and sum_j exp((s - 1) / tau)
//   rowsum   the chunk partials in chunk order
//   select   per target view and row tile: the scores of the two OTHER views against every key tile, the key
//            exp(s_a - 1) / rs_a[i] + exp(s_b - 1) / rs_b[i], a top-k list per row kept in LDS -> pos and a membership
//            bitmask of n bits per row.  The key of (i, j) is a function of rows i and j and of row i's two sums only,
//            never of the tile, so identical aug rows tie exactly and the scan (ascending j, strict >) keeps the lower j.
//   rowgrad  per view and row tile: Oout_i = sum_{j not in pos} e_ij a_j, Opos_i = sum_{j in pos} e_ij a_j and
//            sum_{j in pos} e_ij in one sweep (the two products of rowtile.h); with g = scale / tau,
//            dL/dv_i = g ((Oout_i + Opos_i) / sum_j e - Opos_i / sum_pos e), taken as
//            g (Oout_i / sum_j e - Opos_i (sum_j e - sum_pos e) / (sum_j e sum_pos e)) with the factor in double;
//            then the normalisation backward; the row's loss term and its two key-side weights
//   keygrad  key tiles x (3 views x all rows): dL/da_j = g sum_v sum_i e_ij (1 / sum_j e - [j in pos_v[i]] / sum_pos e) v_i,
//            each key tile owns its rows of dL/dA; then the normalisation backward
//   sum      the row loss terms of each view in a fixed order
// All products run on v_mfma_f32_16x16x4_f32.  Every output element has one producer and one summation order: a call
// returns the same bits every time.
#include <algorithm>
#include <cmath>

#include "rowtile.h"

namespace {

using namespace srh;

constexpr int kRows = kRtRows;         // R rows per workgroup (16 per wave, in registers)
constexpr int kCTile = kRtRows;        // C rows staged in LDS per iteration
constexpr int kMaxK = 32;
constexpr int kPass1Target = 512;      // pass-1 workgroups aimed for (3 views x row tiles x key chunks)
constexpr float kSsEps = 1e-12f;       // tf.nn.l2_normalize's epsilon, on the squared norm
constexpr float kInvClamp = 1e6f;      // rsqrt(1e-12)

__device__ __forceinline__ float inv_norm(float ss) { return ss >= kSsEps ? 1.f / sqrtf(ss) : kInvClamp; }

// ---- rows_l2norm: one wave per row, lane c owns columns c, c + 64, c + 128, c + 192 ----------------------------------
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* __restrict__ y, int64_t n, int d,
                                                         float* __restrict__ out, float* __restrict__ inv_out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;  // (whole waves leave together)
  float x[4];
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = lane + 64 * q;
    x[q] = c < d ? y[row * d + c] : 0.f;
    ss = fmaf(x[q], x[q], ss);
  }
  ss = srh::wave_sum_f(ss);
  const float inv = inv_norm(ss);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = lane + 64 * q;
    if (c < d) out[row * d + c] = x[q] * inv;
  }
  if (lane == 0) inv_out[row] = inv;
}

__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                         const float* __restrict__ inv_in, int64_t n, int d,
                                                         float* __restrict__ gy) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  float gv[4], ov[4];
  float dot = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = lane + 64 * q;
    gv[q] = c < d ? g[row * d + c] : 0.f;
    ov[q] = c < d ? out[row * d + c] : 0.f;
    dot = fmaf(gv[q], ov[q], dot);
  }
  dot = srh::wave_sum_f(dot);
  const float inv = inv_in[row];
  const bool clamped = inv == kInvClamp;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = lane + 64 * q;
    if (c < d) gy[row * d + c] = clamped ? gv[q] * inv : (gv[q] - ov[q] * dot) * inv;
  }
}

// ---- tri-training neighbour discrimination ---------------------------------------------------------------------------
struct TnArgs {
  const float* v[3];
  const float* a;
  int64_t n;
  int k;
  float inv_tau, gscale, scale;
  double* loss;
  float* gv[3];
  float* ga;
  int32_t* pos;
  // workspace
  float* vn[3];      // n x D   normalised views
  float* an;         // n x D   normalised aug
  float* vinv[3];    // n       1 / norm (1e6 where clamped)
  float* ainv;       // n
  double* part1;     // chunks x 3 x n   sum_j exp(s - 1) per key chunk
  double* partT;     // chunks x 3 x n   sum_j exp((s - 1) / tau) per key chunk
  float* inv1;       // 3 x n   1 / sum_j exp(s - 1)
  double* rsT;       // 3 x n   sum_j exp((s - 1) / tau)
  float* cw;         // 3 x n   1 / rsT
  float* cp;         // 3 x n   1 / sum_{j in pos} exp((s - 1) / tau)
  double* row_loss;  // 3 x n
  uint32_t* mask;    // 3 x n x words   bit j of row (v, i): j in pos_v[i]
  int64_t words, chunks, chunk_len;
};

// pass-1 key chunks: a pure function of n, so the workspace query and the launch agree and every call sums alike
inline int64_t tn_chunks(int64_t n) {
  const int64_t tiles = (n + kRows - 1) / kRows;
  int64_t c = (kPass1Target + 3 * tiles - 1) / (3 * tiles);
  if (c > tiles) c = tiles;
  return c < 1 ? 1 : c;
}
inline int64_t tn_chunk_len(int64_t n) {
  const int64_t c = tn_chunks(n);
  const int64_t per = (n + c - 1) / c;
  return (per + kCTile - 1) / kCTile * kCTile;
}
inline int64_t tn_words(int64_t n) { return (n + 31) / 32; }

// the workspace of p.n rows: null ws measures, a workspace carves; returns the bytes
int64_t tn_layout(TnArgs& p, void* ws, int D) {
  Carver w(ws);
  const int64_t n = p.n;
  p.chunks = tn_chunks(n);
  p.chunk_len = tn_chunk_len(n);
  p.words = tn_words(n);
  for (int v = 0; v < 3; ++v) w.take(p.vn[v], n * D);
  w.take(p.an, n * D);
  for (int v = 0; v < 3; ++v) w.take(p.vinv[v], n);
  w.take(p.ainv, n);
  w.take(p.part1, p.chunks * 3 * n);
  w.take(p.partT, p.chunks * 3 * n);
  w.take(p.inv1, 3 * n);
  w.take(p.rsT, 3 * n);
  w.take(p.cw, 3 * n);
  w.take(p.cp, 3 * n);
  w.take(p.row_loss, 3 * n);
  w.take(p.mask, 3 * n * p.words);
  return w.used;
}

// prep: LPR = D/4 lanes per row, one float4 each; blockIdx.y = matrix (views 0..2, then aug)
template <int D>
__global__ __launch_bounds__(256) void tn_prep(TnArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const int m = blockIdx.y;
  const float* src = m < 3 ? a.v[m] : a.a;
  float* dst = m < 3 ? a.vn[m] : a.an;
  float* inv_out = m < 3 ? a.vinv[m] : a.ainv;
  const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  const bool ok = row < a.n;
  const float4 x = ok ? reinterpret_cast<const float4*>(src + row * D)[lane] : srh::f4_zero();
  const float ss = srh::group_sum<LPR>(srh::f4_dot(x, x));
  const float inv = inv_norm(ss);
  if (ok) {
    reinterpret_cast<float4*>(dst + row * D)[lane] = srh::f4_scale(x, inv);
    if (lane == 0) inv_out[row] = inv;
  }
}

template <int D>
__global__ __launch_bounds__(256) void tn_pass1(TnArgs a) {
  __shared__ float cs[kCTile * kRtStride<D>];
  const int v = blockIdx.y;
  const int64_t rtile = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x % a.chunks;
  const int64_t cbeg = chunk * a.chunk_len;
  const int64_t cend = cbeg + a.chunk_len < a.n ? cbeg + a.chunk_len : a.n;
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int64_t r = rtile * kRows + L.wave * 16 + j16;
  const bool rok = r < a.n;
  const float inv_tau = a.inv_tau;
  float rf[D / 4];
  load_rf<D>(rf, a.vn[v], r, rok, g);
  double s1 = 0.0, sT = 0.0;
  for (int64_t c0 = cbeg; c0 < cend; c0 += kCTile) {
    __syncthreads();
    stage_tile<D>(cs, a.an, c0, cend);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kCTile / 16; ++sub) {
      const f32x4 s = score16<D>(cs, sub, j16, g, rf);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        if (c0 + sub * 16 + 4 * g + reg < cend) {
          s1 += (double)expf(s[reg] - 1.f);
          sT += (double)expf((s[reg] - 1.f) * inv_tau);
        }
      }
    }
  }
  s1 = sum4(s1);
  sT = sum4(sT);
  if (rok && g == 0) {
    a.part1[(chunk * 3 + v) * a.n + r] = s1;
    a.partT[(chunk * 3 + v) * a.n + r] = sT;
  }
}

__global__ __launch_bounds__(256) void tn_rowsum(TnArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= 3 * a.n) return;
  double s1 = 0.0, sT = 0.0;
  for (int64_t c = 0; c < a.chunks; ++c) {
    s1 += a.part1[c * 3 * a.n + e];
    sT += a.partT[c * 3 * a.n + e];
  }
  a.inv1[e] = (float)(1.0 / s1);
  a.rsT[e] = sT;
  a.cw[e] = (float)(1.0 / sT);
}

template <int D>
__global__ __launch_bounds__(256) void tn_select(TnArgs a) {
  constexpr int DS = 17, LS = kMaxK + 1;
  __shared__ float cs[kCTile * kRtStride<D>];
  __shared__ float dump[kRows * DS];
  __shared__ float lk[kRows * LS];
  __shared__ int32_t li[kRows * LS];
  const int t = blockIdx.y;
  const int va = t == 0 ? 1 : 0, vb = t == 2 ? 1 : 2;
  const int64_t n = a.n;
  const int64_t rtile = blockIdx.x;
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int64_t r = rtile * kRows + L.wave * 16 + j16;
  const bool rok = r < n;
  float rfa[D / 4], rfb[D / 4];
  load_rf<D>(rfa, a.vn[va], r, rok, g);
  load_rf<D>(rfb, a.vn[vb], r, rok, g);
  const float ia = rok ? a.inv1[va * n + r] : 0.f, ib = rok ? a.inv1[vb * n + r] : 0.f;
  // the scanning thread of a row: tid < 64 owns row rtile*64 + tid
  const int k = a.k;
  const int lb = threadIdx.x * LS;
  int cnt = 0;
  for (int64_t c0 = 0; c0 < n; c0 += kCTile) {
    __syncthreads();
    stage_tile<D>(cs, a.an, c0, n);
    __syncthreads();
    for (int sub = 0; sub < kCTile / 16; ++sub) {
      if (c0 + sub * 16 >= n) break;  // (uniform)
      const f32x4 sa = score16<D>(cs, sub, j16, g, rfa);
      const f32x4 sb = score16<D>(cs, sub, j16, g, rfb);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        dump[(L.wave * 16 + j16) * DS + 4 * g + reg] = fmaf(expf(sa[reg] - 1.f), ia, expf(sb[reg] - 1.f) * ib);
      __syncthreads();
      if (threadIdx.x < kRows) {
        const int64_t j0 = c0 + sub * 16;
        for (int cc = 0; cc < 16 && j0 + cc < n; ++cc) {
          const float key = dump[threadIdx.x * DS + cc];
          // ascending j and a strict >: of equal keys the lower j stays ahead
          int p;
          if (cnt < k) {
            p = cnt++;
          } else if (key > lk[lb + k - 1]) {
            p = k - 1;
          } else {
            continue;
          }
          while (p > 0 && key > lk[lb + p - 1]) {
            lk[lb + p] = lk[lb + p - 1];
            li[lb + p] = li[lb + p - 1];
            --p;
          }
          lk[lb + p] = key;
          li[lb + p] = (int32_t)(j0 + cc);
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x < kRows) {
    const int64_t row = rtile * kRows + threadIdx.x;
    if (row < n) {
      int32_t* pos = a.pos + ((int64_t)t * n + row) * k;
      uint32_t* m = a.mask + ((int64_t)t * n + row) * a.words;
      for (int64_t w = 0; w < a.words; ++w) m[w] = 0u;
      for (int p = 0; p < k; ++p) {
        const int32_t j = li[lb + p];
        pos[p] = j;
        m[j >> 5] |= 1u << (j & 31);
      }
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void tn_rowgrad(TnArgs a) {
  __shared__ float cs[kCTile * kRtStride<D>];
  const int v = blockIdx.y;
  const int64_t n = a.n;
  const int64_t rtile = blockIdx.x;
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int64_t r = rtile * kRows + L.wave * 16 + j16;
  const bool rok = r < n;
  const float inv_tau = a.inv_tau;
  float rf[D / 4];
  load_rf<D>(rf, a.vn[v], r, rok, g);
  const uint32_t* mrow = a.mask + ((int64_t)v * n + (rok ? r : 0)) * a.words;
  f32x4 o1[D / 16], o2[D / 16];
  zero_acc(o1);
  zero_acc(o2);
  double sp = 0.0;
  for (int64_t c0 = 0; c0 < n; c0 += kCTile) {
    __syncthreads();
    stage_tile<D>(cs, a.an, c0, n);
    __syncthreads();
    const int64_t w = c0 >> 5;
    const uint32_t m0 = rok ? mrow[w] : 0u;
    const uint32_t m1 = (rok && w + 1 < a.words) ? mrow[w + 1] : 0u;
#pragma unroll
    for (int sub = 0; sub < kCTile / 16; ++sub) {
      f32x4 s = score16<D>(cs, sub, j16, g, rf);
      const uint32_t mw = (sub < 2 ? m0 : m1) >> ((sub & 1) * 16 + 4 * g);
      f32x4 sm;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const bool cok = c0 + sub * 16 + 4 * g + reg < n;
        const float e = cok ? expf((s[reg] - 1.f) * inv_tau) : 0.f;
        const bool in = (mw >> reg) & 1u;
        sp += (double)(in ? e : 0.f);
        s[reg] = in ? 0.f : e;   // o1: the keys off the list; o2: the positives
        sm[reg] = in ? e : 0.f;
      }
      // (accum16 for both sums at once, spelled out so that the two accumulator chains alternate; two accum16 calls give
      // the same bits and measured level at d = 64 and 0.2 % over the limit at d = 128: profiles/NOTES_rowtile.md)
#pragma unroll
      for (int b = 0; b < D / 16; ++b) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float x = cs[(sub * 16 + 4 * g + reg) * kRtStride<D> + 16 * b + j16];
          o1[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, s[reg], o1[b], 0, 0, 0);
          o2[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, sm[reg], o2[b], 0, 0, 0);
        }
      }
    }
  }
  sp = sum4(sp);
  const int64_t e = (int64_t)v * n + (rok ? r : 0);
  const double rsT = rok ? a.rsT[e] : 1.0;
  const float cw = (float)(1.0 / rsT);
  // (Oout + Opos) / sum_j e - Opos / sum_pos e = Oout / sum_j e - Opos (sum_j e - sum_pos e) / (sum_j e sum_pos e): where
  // the positives hold nearly all of the sum both terms are small, and the two large ones never meet in float32
  const float cd = rok ? (float)((rsT - sp) / (rsT * sp)) : 0.f;
  const float gs = a.gscale;
#pragma unroll
  for (int b = 0; b < D / 16; ++b)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) o1[b][reg] = gs * (o1[b][reg] * cw - o2[b][reg] * cd);
  if (rok && g == 0) {
    a.cp[e] = (float)(1.0 / sp);
    a.row_loss[e] = log(rsT) - log(sp);
  }
  const float inv = rok ? a.vinv[v][r] : 1.f;
  norm_bwd_store<D>(o1, a.vn[v], inv, inv == kInvClamp, r, rok, g, a.gv[v]);
}

template <int D>
__global__ __launch_bounds__(256) void tn_keygrad(TnArgs a) {
  __shared__ float cs[kCTile * kRtStride<D>];
  __shared__ float cwl[kCTile];
  __shared__ float cpl[kCTile];
  __shared__ uint32_t ml[kCTile * 2];
  const int64_t n = a.n;
  const int64_t rtile = blockIdx.x;
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int lr = L.wave * 16 + j16;          // this lane's key within the tile
  const int64_t r = rtile * kRows + lr;
  const bool rok = r < n;
  const float inv_tau = a.inv_tau;
  float rf[D / 4];
  load_rf<D>(rf, a.an, r, rok, g);
  f32x4 o[D / 16];
  zero_acc(o);
  const int64_t wbase = rtile * (kRows / 32);  // the two mask words that hold this tile's keys
  for (int v = 0; v < 3; ++v) {
    for (int64_t c0 = 0; c0 < n; c0 += kCTile) {
      __syncthreads();
      stage_tile<D>(cs, a.vn[v], c0, n);
      if (threadIdx.x < kCTile) {
        const int64_t c = c0 + threadIdx.x;
        const bool cok = c < n;
        cwl[threadIdx.x] = cok ? a.cw[(int64_t)v * n + c] : 0.f;
        cpl[threadIdx.x] = cok ? a.cp[(int64_t)v * n + c] : 0.f;
      } else if (threadIdx.x < 3 * kCTile) {
        const int i = (threadIdx.x - kCTile) >> 1, h = (threadIdx.x - kCTile) & 1;
        const int64_t c = c0 + i;
        ml[i * 2 + h] = (c < n && wbase + h < a.words) ? a.mask[((int64_t)v * n + c) * a.words + wbase + h] : 0u;
      }
      __syncthreads();
#pragma unroll
      for (int sub = 0; sub < kCTile / 16; ++sub) {
        f32x4 s = score16<D>(cs, sub, j16, g, rf);
        // s[reg] = S[i = c0 + sub*16 + 4g + reg][j = r]
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int ci = sub * 16 + 4 * g + reg;
          const float e = expf((s[reg] - 1.f) * inv_tau);
          const bool in = (ml[ci * 2 + (lr >> 5)] >> (lr & 31)) & 1u;
          const float wp = e * cpl[ci];
          s[reg] = e * cwl[ci] - (in ? wp : 0.f);
        }
        // (accum16's product, spelled out: through the helper this kernel's code is reordered and the step measured
        // 2 % slower, profiles/NOTES_rowtile.md)
#pragma unroll
        for (int b = 0; b < D / 16; ++b) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            o[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(cs[(sub * 16 + 4 * g + reg) * kRtStride<D> + 16 * b + j16], s[reg], o[b],
                                                        0, 0, 0);
        }
      }
    }
  }
  const float gs = a.gscale;
#pragma unroll
  for (int b = 0; b < D / 16; ++b) o[b] *= gs;
  const float inv = rok ? a.ainv[r] : 1.f;
  norm_bwd_store<D>(o, a.an, inv, inv == kInvClamp, r, rok, g, a.ga);
}

// the loss of view blockIdx.x: its row terms in a fixed order, times the scale
__global__ __launch_bounds__(256) void tn_loss(TnArgs a) {
  const int v = blockIdx.x;
  const double s = block_sum_d(a.row_loss + (int64_t)v * a.n, a.n);
  if (threadIdx.x == 0) a.loss[v] = (double)a.scale * s;
}

template <int D>
srh_status_t launch_tn(const TnArgs& a, hipStream_t st) {
  constexpr int RPB = 256 / (D / 4);
  const unsigned tiles = (unsigned)((a.n + kRows - 1) / kRows);
  tn_prep<D><<<dim3((unsigned)((a.n + RPB - 1) / RPB), 4), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_pass1<D><<<dim3(tiles * (unsigned)a.chunks, 3), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_rowsum<<<(unsigned)((3 * a.n + 255) / 256), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_select<D><<<dim3(tiles, 3), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_rowgrad<D><<<dim3(tiles, 3), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_keygrad<D><<<tiles, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  tn_loss<<<3, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // namespace

extern "C" {

srh_status_t srh_rows_l2norm_fwd_f32(const float* d_y, int64_t n, int32_t d, float* d_out, float* d_inv, void* stream) {
  SRH_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "rows_l2norm_fwd: bad n");
  SRH_SUPPORTED(d >= 1 && d <= 256, "rows_l2norm_fwd: d=%d unsupported (1..256)", d);
  if (n == 0) return SRH_OK;
  SRH_REQUIRE(d_y && d_out && d_inv, "rows_l2norm_fwd: null argument");
  l2norm_fwd_kernel<<<(unsigned)((n + 3) / 4), 256, 0, srh::as_stream(stream)>>>(d_y, n, d, d_out, d_inv);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

srh_status_t srh_rows_l2norm_bwd_f32(const float* d_g, const float* d_out, const float* d_inv, int64_t n, int32_t d,
                                     float* d_gy, void* stream) {
  SRH_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "rows_l2norm_bwd: bad n");
  SRH_SUPPORTED(d >= 1 && d <= 256, "rows_l2norm_bwd: d=%d unsupported (1..256)", d);
  if (n == 0) return SRH_OK;
  SRH_REQUIRE(d_g && d_out && d_inv && d_gy, "rows_l2norm_bwd: null argument");
  l2norm_bwd_kernel<<<(unsigned)((n + 3) / 4), 256, 0, srh::as_stream(stream)>>>(d_g, d_out, d_inv, n, d, d_gy);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_tri_nd_ws_bytes(int64_t n, int32_t d, int32_t k) {
  if (n <= 0 || n >= (int64_t(1) << 24) || (d != 64 && d != 128) || k < 1 || k > kMaxK || n < k) return 0;
  TnArgs a{};
  a.n = n;
  return tn_layout(a, nullptr, d);
}

srh_status_t srh_tri_nd_fwd_bwd(const srh_tri_nd_args_t* args, void* d_ws, void* stream) {
  SRH_REQUIRE(args && d_ws, "tri_nd_fwd_bwd: null argument");
  const srh_tri_nd_args_t& s = *args;
  SRH_SUPPORTED(s.d == 64 || s.d == 128, "tri_nd_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)",
                s.d);
  SRH_SUPPORTED(s.k >= 1 && s.k <= kMaxK, "tri_nd_fwd_bwd: k=%d unsupported (1..%d)", s.k, kMaxK);
  SRH_REQUIRE(s.n >= 1 && s.n < (int64_t(1) << 24), "tri_nd_fwd_bwd: bad n");
  SRH_SUPPORTED(s.n >= s.k, "tri_nd_fwd_bwd: n=%lld rows cannot give k=%d positives (ins_cnt)", (long long)s.n, s.k);
  SRH_REQUIRE(s.tau > 0.f && std::isfinite(s.tau), "tri_nd_fwd_bwd: temperature must be positive");
  SRH_REQUIRE(std::isfinite(s.loss_scale), "tri_nd_fwd_bwd: the loss scale must be finite");
  SRH_REQUIRE(s.d_aug && s.d_loss && s.d_gaug && s.d_pos, "tri_nd_fwd_bwd: null tensor");
  TnArgs a{};
  for (int v = 0; v < 3; ++v) {
    SRH_REQUIRE(s.d_view[v] && s.d_gview[v], "tri_nd_fwd_bwd: null tensor of view %d", v);
    a.v[v] = s.d_view[v];
    a.gv[v] = s.d_gview[v];
  }
  a.a = s.d_aug; a.n = s.n; a.k = s.k;
  a.inv_tau = 1.f / s.tau;
  a.scale = s.loss_scale;
  a.gscale = s.loss_scale * a.inv_tau;
  a.loss = s.d_loss; a.ga = s.d_gaug; a.pos = s.d_pos;
  tn_layout(a, d_ws, s.d);
  hipStream_t st = srh::as_stream(stream);
  return s.d == 64 ? launch_tn<64>(a, st) : launch_tn<128>(a, st);
}

}  // extern "C"

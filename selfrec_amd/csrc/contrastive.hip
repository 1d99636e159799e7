// Unit-row InfoNCE by two MFMA passes, with no logits matrix and no float atomics: NCL's table loss and SSL4Rec's
// batch_softmax_loss.  DESIGN.md 4.6 and 4.8.
//
// Per problem: queries Q (B x D), keys T (N x D) and the positive key of each query, pos(b) = idx[b], or b itself when
// idx is null (then N = B).  q = normalize(Q_b), t = normalize(T_j) (F.normalize: x / max(|x|, 1e-12)),
// e_bj = exp(q_b.t_j / tau), P_bj = e_bj / sum_j e_bj.
//   table InfoNCE (srh_table_nce_fwd_bwd, NCL.py:57-83 ssl_layer_loss; one or two problems, each with a loss scale s)
//     loss = s sum_b [ -q_b.t_idx[b] / tau + log sum_j e_bj ]          dL/ds_bj = s (P_bj - [j == idx_b]) / tau
//   batch softmax (srh_batch_softmax_fwd_bwd, util/loss_torch.py:25-32; one problem, T = V, the identity as positives)
//     loss = mean_b -log(p_b + 1e-5), p_b = P_bb                      dL/ds_bj = w_b (P_bj - [j == b]) / (B tau)
//     with w_b = p_b / (p_b + 1e-5): InfoNCE's row gradient scaled by w_b.
// The B x N logits are never materialised.  The rows are unit vectors, so every logit is <= 1/tau and the exponentials
// are taken as exp((s - 1) / tau): no running max.  That cannot overflow, but it underflows where the reference's exp(s / tau)
// does not: a query with no key above cos = 1 - 87 tau has a row sum of subnormal terms (0 below 1 - 103 tau), and the finish
// makes its loss term NaN (rowsum < N 2^-130).  For tau >= 0.023 no data can get there.
//   prep    normalise Q and T into the workspace (rows and their norms)
//   pass 1  query tiles x key chunks: per query and chunk, sum_j e_bj and sum_j e_bj t_j (e = exp((s - 1)/tau))
//   finish  per query: the chunk partials in chunk order -> row sum, loss term, dL/dQ (normalisation backward fused),
//           and the query's weights for pass 2: cw_b (1 / rowsum; w_b / rowsum) and cd_b (1; w_b)
//   pass 2  key tiles x all queries: dT_j = g sum_b (e_bj cw_b - [pos(b) == j] cd_b) q_b with the problem's gradient
//           scale g (s / tau; 1 / (B tau)), normalisation backward fused; each key tile owns its rows of dT
//   sum     the per-query loss terms in a fixed order
// Only the finish's loss term and weights, the rounding of pass 2's positive term and the scaling of the sum depend on
// the loss (the SOFTMAX template flag); everything else is data.  All four products run on v_mfma_f32_16x16x4_f32.  Every
// output element is produced by one lane in a fixed order, so a call returns the same bits every time.
//
// Both passes are one kernel on the row tile of rowtile.h: a workgroup holds 64 "R" rows (16 per wave) in registers and
// streams "C" rows through LDS.
//   S^T[c][r] = Cn_c . Rn_r                       (MFMA 1: A = C tile from LDS, B = R rows from registers)
//   W[c][r]   = weight(S^T[c][r])                 (on the accumulator, in place)
//   O^T[:, r] += sum_c Cn_c W[c][r]               (MFMA 2: the accumulator of MFMA 1 is its B operand, no lane movement;
//                                                  the c order inside a k-step is 4*(lane>>4) + reg, matched by A)
// pass 1: R = queries, C = keys,    W = e                               -> O = sum_j e_bj t_j, and the row sums of W
// pass 2: R = keys,    C = queries, W = e cw_c - [pos(c) == key] cd_c   -> O = dL/dt / g
//
// Softmax cross-entropy of rows against a whole table (srh_table_ce_fwd_bwd, BERT4Rec.py:58-62) is a
// sibling on the same ownership, seam, chunking and staging: logits s_mj = H_m . T_j with no normalisation and no
// temperature, so they have no bound and the softmax is max-subtracted.  Pass 1 keeps a running max per row, rescales its
// sums when a key tile raises it (e = exp(s - max)) and writes (max, sum e, sum e T_j) per key chunk; the finish takes the
// row's largest chunk max, merges the partials in chunk order with exp(max_c - max), and fixes lse_m; pass 2 weighs with
// exp(s - lse_m) - [j == label_m] <= 1 and sums each 64-row tile from zero before adding it to the key's total (DESIGN.md
// 4.20).  No prep launch: the rows are used as they are.
//
// The pair cross-entropy (srh_pair_ce_fwd_bwd, util/loss_torch.py:35-50 with b_cos=False and :54-88) is
// the same three kernels under the PAIR template flag: the logits carry a scale, s_mj = inv_temp H_m . T_j, and a call may
// leave key j = m out of row m's softmax (exclude_diagonal, M = N).  A row can then meet a tile or a chunk whose only key
// is its own: such a tile has no finite logit, contributes nothing and leaves the running max at -inf, and the finish
// gives a chunk whose max is -inf the weight 0.  Pass 2 can add the finished dL/dH row r into the dL/dT row r it owns
// (add_gh_into_gt, M = N): a caller that passes one matrix as H and T gets its whole gradient without another launch.
#include <algorithm>
#include <cmath>

#include "rowtile.h"

namespace {

using namespace srh;

constexpr int kCtRows = kRtRows;            // R rows per workgroup (16 per wave)
constexpr int kCtCTile = kRtRows;           // C rows staged in LDS per iteration
constexpr int kCtMaxProblems = 2;
constexpr int kCtPass1Target = 512;         // pass-1 workgroups aimed for per problem (query tiles x key chunks)
constexpr float kNormEps = 1e-12f;
constexpr double kBsEps = 1e-5;             // loss_torch.py:31 (10e-6)

struct CtProblem {
  const float* q;
  const float* t;
  const int32_t* idx;  // null: the positive key of query b is row b
  int64_t B, N;
  float scale;         // table loss: the loss scale
  float gscale;        // dL/dt_j = gscale * O_j (then the normalisation backward)
  double* loss;
  float* gq;
  float* gt;
  // workspace
  float* qn;        // B x D  normalised queries
  float* qnorm;     // B      |Q_b|
  float* tn;        // N x D  normalised keys
  float* tnorm;     // N      |T_j|
  float* part_o;    // chunks x B x D  sum_j e_bj t_j per key chunk
  double* part_rs;  // chunks x B      sum_j e_bj per key chunk
  float* cw;        // B      pass-2 weight of query b
  float* cd;        // B      pass-2 weight of query b's positive term
  double* row_loss; // B
  int64_t chunks, chunk_len;
};

struct CtArgs {
  CtProblem p[kCtMaxProblems];
  float inv_tau;
};

// pass-1 key chunks of a problem: a pure function of (B, N), so the workspace query and the launch agree and every
// call sums in the same order
inline int64_t ct_chunks(int64_t B, int64_t N) {
  const int64_t rtiles = (B + kCtRows - 1) / kCtRows;
  const int64_t ctiles = (N + kCtCTile - 1) / kCtCTile;
  int64_t c = (kCtPass1Target + rtiles - 1) / rtiles;
  if (c > ctiles) c = ctiles;
  return c < 1 ? 1 : c;
}
inline int64_t ct_chunk_len(int64_t B, int64_t N) {
  const int64_t c = ct_chunks(B, N);
  const int64_t per = (N + c - 1) / c;
  return (per + kCtCTile - 1) / kCtCTile * kCtCTile;
}

// the workspace of a problem of (p.B, p.N): null ws measures, a workspace carves; returns the bytes
int64_t ct_layout(CtProblem& p, void* ws, int D) {
  Carver w(ws);
  p.chunks = ct_chunks(p.B, p.N);
  p.chunk_len = ct_chunk_len(p.B, p.N);
  w.take(p.qn, p.B * D);
  w.take(p.qnorm, p.B);
  w.take(p.tn, p.N * D);
  w.take(p.tnorm, p.N);
  w.take(p.part_o, p.chunks * p.B * D);
  w.take(p.part_rs, p.chunks * p.B);
  w.take(p.cw, p.B);
  w.take(p.cd, p.B);
  w.take(p.row_loss, p.B);
  return w.used;
}
inline int64_t ct_ws_bytes(int64_t B, int64_t N, int D) {
  CtProblem p{};
  p.B = B; p.N = N;
  return ct_layout(p, nullptr, D);
}

// d(normalize(x))/dx applied to g: (g - y (y.g)) / |x| where |x| >= eps, g / eps below it (F.normalize's clamp_min)
__device__ __forceinline__ float norm_bwd_scale(float nrm) { return 1.f / fmaxf(nrm, kNormEps); }

// pass 2's weight of a query's positive term, rounded as each loss has always rounded it: the table loss in one fused
// multiply-add (e cw - 1), batch softmax after the product (e cw rounded, then - w_b)
template <bool SOFTMAX>
__device__ __forceinline__ float pos_weight(float e, float cw, float cd) {
  if (SOFTMAX) {
#pragma clang fp contract(off)
    return e * cw - cd;
  }
  return fmaf(e, cw, -cd);
}

// ---- prep: normalise rows (LPR = D/4 lanes per row, one float4 each) ------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void ct_prep(CtArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const CtProblem& P = a.p[blockIdx.y >> 1];
  const bool keys = blockIdx.y & 1;
  const int64_t rows = keys ? P.N : P.B;
  const float* src = keys ? P.t : P.q;
  float* dst = keys ? P.tn : P.qn;
  float* nrm_out = keys ? P.tnorm : P.qnorm;
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

// ---- the two passes (SOFTMAX: pass 2's positive-term rounding only) -------------------------------------------------
template <int D, bool PASS2, bool SOFTMAX>
__global__ __launch_bounds__(256) void ct_pass(CtArgs a) {
  __shared__ float cs[kCtCTile * kRtStride<D>];
  __shared__ float cw[kCtCTile];
  __shared__ float cd[kCtCTile];
  __shared__ int32_t cid[kCtCTile];
  const CtProblem& P = a.p[blockIdx.y];
  const int64_t nR = PASS2 ? P.N : P.B;
  const float* Rn = PASS2 ? P.tn : P.qn;
  const float* Cn = PASS2 ? P.qn : P.tn;
  const int64_t rtiles = (nR + kCtRows - 1) / kCtRows;
  const int64_t rtile = PASS2 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x / P.chunks;
  const int64_t chunk = PASS2 ? 0 : (int64_t)blockIdx.x % P.chunks;
  if (rtile >= rtiles) return;
  int64_t cbeg = 0, cend = P.B;
  if (!PASS2) {
    cbeg = chunk * P.chunk_len;
    cend = cbeg + P.chunk_len < P.N ? cbeg + P.chunk_len : P.N;
  }
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int64_t r = rtile * kCtRows + L.wave * 16 + j16;
  const bool rok = r < nR;
  const float inv_tau = a.inv_tau;

  float rf[D / 4];
#pragma unroll
  for (int s = 0; s < D / 4; ++s) rf[s] = rok ? Rn[r * D + 4 * s + g] : 0.f;
  f32x4 o[D / 16];
  zero_acc(o);
  double rs = 0.0;

  for (int64_t c0 = cbeg; c0 < cend; c0 += kCtCTile) {
    __syncthreads();
    stage_tile<D>(cs, Cn, c0, cend);
    if (threadIdx.x < kCtCTile) {
      const int64_t c = c0 + threadIdx.x;
      const bool cok = c < cend;
      if (PASS2) {
        cw[threadIdx.x] = cok ? P.cw[c] : 0.f;
        cd[threadIdx.x] = cok ? P.cd[c] : 0.f;
        cid[threadIdx.x] = !cok ? -1 : P.idx ? P.idx[c] : (int32_t)c;
      } else {
        cw[threadIdx.x] = cok ? 1.f : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kCtCTile / 16; ++sub) {
      f32x4 s = score16<D>(cs, sub, j16, g, rf);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ci = sub * 16 + 4 * g + reg;
        const float e = expf((s[reg] - 1.f) * inv_tau);
        float w = e * cw[ci];
        if (PASS2) {
          // (computed for every column: a select, not a branch, keeps the LDS reads of a k-step in one 16-byte read each)
          const float wpos = pos_weight<SOFTMAX>(e, cw[ci], cd[ci]);
          if ((int64_t)cid[ci] == r) w = wpos;
        } else {
          rs += (double)w;
        }
        s[reg] = w;
      }
      accum16<D>(o, cs, sub, j16, g, s);
    }
  }
  if (!PASS2) {
    rs = sum4(rs);
    if (!rok) return;
    const int64_t row = chunk * P.B + r;
    if (g == 0) P.part_rs[row] = rs;
    store_acc<D>(o, P.part_o, row, g);
  } else {
    // dL/dt_j = gscale * O_j; then the normalisation backward of row j
    const float k = P.gscale;
#pragma unroll
    for (int b = 0; b < D / 16; ++b) o[b] *= k;
    const float nrm = rok ? P.tnorm[r] : 1.f;
    norm_bwd_store<D>(o, P.tn, norm_bwd_scale(nrm), !(nrm > kNormEps), r, rok, g, P.gt);
  }
}

// ---- per-query finish: chunk partials in chunk order -> row sum, loss term, pass-2 weights, dL/dQ -------------------
template <int D, bool SOFTMAX>
__global__ __launch_bounds__(256) void ct_finish(CtArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const CtProblem& P = a.p[blockIdx.y];
  const int64_t b = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  if (b >= P.B) return;  // (whole row groups leave together: group_sum stays within live lanes)
  double rs = 0.0;
  float4 o = srh::f4_zero();
  for (int64_t c = 0; c < P.chunks; ++c) {
    rs += P.part_rs[c * P.B + b];
    o = srh::f4_add(o, reinterpret_cast<const float4*>(P.part_o + (c * P.B + b) * D)[lane]);
  }
  const int64_t j = P.idx ? (int64_t)P.idx[b] : b;
  const bool jok = j >= 0 && j < P.N;  // (an index outside the table reads nothing and makes the loss NaN)
  const float4 q = reinterpret_cast<const float4*>(P.qn + b * D)[lane];
  const float4 t = jok ? reinterpret_cast<const float4*>(P.tn + j * D)[lane] : srh::f4_zero();
  const float spos = srh::group_sum<LPR>(srh::f4_dot(q, t));
  const float inv_rs = (float)(1.0 / rs);
  const float inv_tau = a.inv_tau;
  // The terms are exp((s - 1)/tau) in f32: below cos = 1 - 87 tau they are subnormal, each off by up to 2^-150, and below
  // 1 - 103 tau they are 0.  Under N 2^-130 the N terms' errors may be more than 2^-20 of the row sum (or all of it, at
  // rowsum = 0): such a row's loss term is NaN, like that of an index outside the table.  No data reaches this for
  // tau >= 0.023 (exp(-2/tau) is normal).
  const bool rs_ok = !(rs < (double)P.N * 0x1p-130);
  // dL/dq_b = k (O_b / rowsum - t_pos(b))
  float k = P.gscale;
  if (SOFTMAX) {
    const double p = exp(((double)spos - 1.0) * (double)inv_tau) / rs;
    const double w = p / (p + kBsEps);
    if (lane == 0) {
      P.row_loss[b] = rs_ok ? -log(p + kBsEps) : (double)NAN;
      P.cw[b] = (float)(w / rs);
      P.cd[b] = (float)w;
    }
    k = (float)w * inv_tau / (float)P.B;
  } else if (lane == 0) {
    P.row_loss[b] = jok && rs_ok ? (double)inv_tau * (1.0 - (double)spos) + log(rs) : (double)NAN;
    P.cw[b] = inv_rs;
    P.cd[b] = 1.f;
  }
  float4 gq = make_float4(k * (o.x * inv_rs - t.x), k * (o.y * inv_rs - t.y), k * (o.z * inv_rs - t.z),
                          k * (o.w * inv_rs - t.w));
  const float dot = srh::group_sum<LPR>(srh::f4_dot(q, gq));
  const float nrm = P.qnorm[b];
  const float inv = norm_bwd_scale(nrm);
  if (nrm > kNormEps) gq = make_float4(gq.x - q.x * dot, gq.y - q.y * dot, gq.z - q.z * dot, gq.w - q.w * dot);
  reinterpret_cast<float4*>(P.gq + b * D)[lane] = srh::f4_scale(gq, inv);
}

// ---- the loss: per-query terms summed in a fixed order, one workgroup per problem; scale s, or the mean ------------
template <bool SOFTMAX>
__global__ __launch_bounds__(256) void ct_loss(CtArgs a) {
  const CtProblem& P = a.p[blockIdx.x];
  const double s = block_sum_d(P.row_loss, P.B);
  if (threadIdx.x == 0) P.loss[0] = SOFTMAX ? s / (double)P.B : (double)P.scale * s;
}

template <int D, bool SOFTMAX>
srh_status_t launch_ct(CtArgs& a, int np, hipStream_t st) {
  int64_t max_prep = 0, max_p1 = 0, max_fin = 0, max_p2 = 0;
  constexpr int RPB = 256 / (D / 4);
  for (int k = 0; k < np; ++k) {
    const CtProblem& p = a.p[k];
    const int64_t big = p.N > p.B ? p.N : p.B;
    max_prep = std::max(max_prep, (big + RPB - 1) / RPB);
    max_p1 = std::max(max_p1, (p.B + kCtRows - 1) / kCtRows * p.chunks);
    max_fin = std::max(max_fin, (p.B + RPB - 1) / RPB);
    max_p2 = std::max(max_p2, (p.N + kCtRows - 1) / kCtRows);
  }
  ct_prep<D><<<dim3((unsigned)max_prep, 2 * np), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  ct_pass<D, false, false><<<dim3((unsigned)max_p1, np), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  ct_finish<D, SOFTMAX><<<dim3((unsigned)max_fin, np), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  ct_pass<D, true, SOFTMAX><<<dim3((unsigned)max_p2, np), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  ct_loss<SOFTMAX><<<np, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

// ---- softmax cross-entropy of M rows against the whole table: unbounded logits, running max --------------------------
struct CeArgs {
  const float* h;        // M x D
  const float* t;        // N x D
  const int32_t* label;  // M
  int64_t M, N;
  float scale;
  // the pair cross-entropy only (PAIR): s = inv_temp H.T, gradients times gscale = scale inv_temp
  float inv_temp, gscale;
  int32_t exclude;   // key j = m is left out of row m's softmax (M == N)
  int32_t add_gh;    // pass 2 stores gt_r + gh_r (M == N)
  double* loss;
  float* gh;
  float* gt;
  // workspace
  float* part_o;     // chunks x M x D  sum_j e_mj T_j per key chunk, e = exp(s - part_m)
  double* part_rs;   // chunks x M      sum_j e_mj per key chunk
  float* part_m;     // chunks x M      the chunk's largest logit of row m
  float* lse;        // M               log sum_j exp(s_mj)
  double* row_loss;  // M               lse_m - s_{m, label_m}
  int64_t chunks, chunk_len;
};

int64_t ce_layout(CeArgs& a, void* ws, int D) {
  Carver w(ws);
  a.chunks = ct_chunks(a.M, a.N);
  a.chunk_len = ct_chunk_len(a.M, a.N);
  w.take(a.part_o, a.chunks * a.M * D);
  w.take(a.part_rs, a.chunks * a.M);
  w.take(a.part_m, a.chunks * a.M);
  w.take(a.lse, a.M);
  w.take(a.row_loss, a.M);
  return w.used;
}
inline int64_t ce_ws_bytes(int64_t M, int64_t N, int D) {
  CeArgs a{};
  a.M = M; a.N = N;
  return ce_layout(a, nullptr, D);
}

// max over the four lanes (lane >> 4 = 0..3) that share an R row: the same bits in all four
__device__ __forceinline__ float ce_row_max4(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  v = fmaxf(v, __shfl_xor(v, 32));
  return v;
}

// pass 1: R = the rows of H, C = a key chunk of T, W = exp(s - running max)  -> per chunk (max, sum W, sum W T_j)
// pass 2: R = the rows of T, C = all rows of H,    W = exp(s - lse_c) - [label_c == r]  -> dL/dT_r / scale
// PAIR: s is inv_temp times the product; with P.exclude the pair (row m, key m) has s = -inf in pass 1 and W = 0 in pass 2
template <int D, bool PASS2, bool PAIR>
__global__ __launch_bounds__(256) void ce_pass(CeArgs P) {
  __shared__ float cs[kCtCTile * kRtStride<D>];
  __shared__ float clse[kCtCTile];
  __shared__ int32_t clab[kCtCTile];
  const int64_t nR = PASS2 ? P.N : P.M;
  const float* Rn = PASS2 ? P.t : P.h;
  const float* Cn = PASS2 ? P.h : P.t;
  const int64_t rtile = PASS2 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x / P.chunks;
  const int64_t chunk = PASS2 ? 0 : (int64_t)blockIdx.x % P.chunks;
  int64_t cbeg = 0, cend = P.M;
  if (!PASS2) {
    cbeg = chunk * P.chunk_len;
    cend = cbeg + P.chunk_len < P.N ? cbeg + P.chunk_len : P.N;
  }
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int64_t r = rtile * kCtRows + L.wave * 16 + j16;
  const bool rok = r < nR;
  const bool excl = PAIR && P.exclude != 0;

  float rf[D / 4];
#pragma unroll
  for (int s = 0; s < D / 4; ++s) rf[s] = rok ? Rn[r * D + 4 * s + g] : 0.f;
  f32x4 o[D / 16];
  zero_acc(o);
  // pass 2 sums every 64-row tile from zero and adds the tile's sum here: a key that many rows name builds up a sum of
  // -H_m thousands of times the size of the P_mj H_m terms of all other rows, which a single running sum would then drop
  f32x4 tot[PASS2 ? D / 16 : 1];
  if (PASS2) zero_acc(tot);
  double rs = 0.0;
  float m = -INFINITY;

  for (int64_t c0 = cbeg; c0 < cend; c0 += kCtCTile) {
    __syncthreads();
    stage_tile<D>(cs, Cn, c0, cend);
    if (PASS2 && threadIdx.x < kCtCTile) {
      const int64_t c = c0 + threadIdx.x;
      clse[threadIdx.x] = c < cend ? P.lse[c] : INFINITY;      // (a row past M weighs exp(-inf) = 0)
      clab[threadIdx.x] = c < cend ? P.label[c] : -1;
    }
    __syncthreads();
    f32x4 s[kCtCTile / 16];
#pragma unroll
    for (int sub = 0; sub < kCtCTile / 16; ++sub) s[sub] = score16<D>(cs, sub, j16, g, rf);
    if (PAIR) {
#pragma unroll
      for (int sub = 0; sub < kCtCTile / 16; ++sub) s[sub] *= P.inv_temp;
    }
    if (!PASS2) {
      // the keys past the chunk's end are -inf before the max; a tile holds at least one key, so the max is finite
      // (PAIR with exclusion: the row's own key is -inf too, and a tile may hold no other -- see m_sub below)
      float mx = -INFINITY;
#pragma unroll
      for (int sub = 0; sub < kCtCTile / 16; ++sub)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t c = c0 + sub * 16 + 4 * g + reg;
          if (c >= cend || (excl && c == r)) s[sub][reg] = -INFINITY;
          mx = fmaxf(mx, s[sub][reg]);
        }
      const float m_new = fmaxf(m, ce_row_max4(mx));
      // 0 on the first tile (m = -inf), 1 while the max stands.  PAIR: while the row has met no key, m and m_new are both
      // -inf and m - m_new is NaN: nothing is held yet, so the factor is 0, and the tile's weights exp(-inf - 0) are 0
      const float alpha = PAIR && m == -INFINITY ? 0.f : expf(m - m_new);
      rs *= (double)alpha;
#pragma unroll
      for (int b = 0; b < D / 16; ++b) o[b] *= alpha;
      m = m_new;
      const float m_sub = PAIR && m == -INFINITY ? 0.f : m;
#pragma unroll
      for (int sub = 0; sub < kCtCTile / 16; ++sub)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float w = expf(s[sub][reg] - m_sub);
          rs += (double)w;
          s[sub][reg] = w;
        }
    } else {
#pragma unroll
      for (int sub = 0; sub < kCtCTile / 16; ++sub)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int ci = sub * 16 + 4 * g + reg;
          float w = expf(s[sub][reg] - clse[ci]);
          if ((int64_t)clab[ci] == r) w -= 1.f;
          // (after the one-hot: a row that names its own excluded key has none, here as in the finish)
          if (excl && c0 + ci == r) w = 0.f;
          s[sub][reg] = w;
        }
    }
#pragma unroll
    for (int sub = 0; sub < kCtCTile / 16; ++sub) accum16<D>(o, cs, sub, j16, g, s[sub]);
    if (PASS2) {
#pragma unroll
      for (int b = 0; b < D / 16; ++b) tot[b] += o[b];
      zero_acc(o);
    }
  }
  if (PASS2) {
#pragma unroll
    for (int b = 0; b < D / 16; ++b) o[b] = tot[b];
  }
  if (!PASS2) {
    rs = sum4(rs);
    if (!rok) return;
    const int64_t row = chunk * P.M + r;
    if (g == 0) {
      P.part_rs[row] = rs;
      P.part_m[row] = m;
    }
    store_acc<D>(o, P.part_o, row, g);
  } else {
    if (!rok) return;
    const float k = PAIR ? P.gscale : P.scale;
#pragma unroll
    for (int b = 0; b < D / 16; ++b) o[b] *= k;
    if (PAIR && P.add_gh) {
      // (M == N: row r of dL/dH exists, and the finish that wrote it ran before this launch on the same stream)
#pragma unroll
      for (int b = 0; b < D / 16; ++b) {
        const float4 h = reinterpret_cast<const float4*>(P.gh + r * D + 16 * b + 4 * g)[0];
        o[b] += f32x4{h.x, h.y, h.z, h.w};
      }
    }
    store_acc<D>(o, P.gt, r, g);
  }
}

// per row: the chunk partials merged in chunk order under the row's largest max -> lse, loss term, dL/dH
template <int D, bool PAIR>
__global__ __launch_bounds__(256) void ce_finish(CeArgs P) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const int64_t b = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  if (b >= P.M) return;  // (whole row groups leave together)
  float mm = -INFINITY;
  for (int64_t c = 0; c < P.chunks; ++c) mm = fmaxf(mm, P.part_m[c * P.M + b]);
  double rs = 0.0;
  float4 o = srh::f4_zero();
  for (int64_t c = 0; c < P.chunks; ++c) {
    const float pm = P.part_m[c * P.M + b];
    const float a = PAIR && pm == -INFINITY ? 0.f : expf(pm - mm);  // (PAIR: a chunk that held only the row's own key)
    rs += P.part_rs[c * P.M + b] * (double)a;
    o = srh::f4_fma(a, reinterpret_cast<const float4*>(P.part_o + (c * P.M + b) * D)[lane], o);
  }
  const int64_t j = P.label[b];
  // (a label outside the table reads nothing and makes the loss NaN; so does the row's own key when it is excluded)
  const bool jok = j >= 0 && j < P.N && !(PAIR && P.exclude && j == b);
  const float4 h = reinterpret_cast<const float4*>(P.h + b * D)[lane];
  const float4 t = jok ? reinterpret_cast<const float4*>(P.t + j * D)[lane] : srh::f4_zero();
  double spos = (double)h.x * (double)t.x + (double)h.y * (double)t.y + (double)h.z * (double)t.z + (double)h.w * (double)t.w;
#pragma unroll
  for (int w = 1; w < LPR; w <<= 1) spos += __shfl_xor(spos, w);
  if (PAIR) spos *= (double)P.inv_temp;
  const double lse = (double)mm + log(rs);
  if (lane == 0) {
    P.row_loss[b] = jok ? lse - spos : (double)NAN;
    P.lse[b] = (float)lse;
  }
  const float inv_rs = (float)(1.0 / rs), k = PAIR ? P.gscale : P.scale;
  reinterpret_cast<float4*>(P.gh + b * D)[lane] = make_float4(k * (o.x * inv_rs - t.x), k * (o.y * inv_rs - t.y),
                                                               k * (o.z * inv_rs - t.z), k * (o.w * inv_rs - t.w));
}

// the loss: the row terms summed in a fixed order by one workgroup, times the scale
__global__ __launch_bounds__(256) void ce_loss(CeArgs P) {
  const double s = block_sum_d(P.row_loss, P.M);
  if (threadIdx.x == 0) P.loss[0] = (double)P.scale * s;
}

template <int D, bool PAIR>
srh_status_t launch_ce(const CeArgs& a, hipStream_t st) {
  constexpr int RPB = 256 / (D / 4);
  const int64_t p1 = (a.M + kCtRows - 1) / kCtRows * a.chunks, p2 = (a.N + kCtRows - 1) / kCtRows;
  ce_pass<D, false, PAIR><<<(unsigned)p1, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  ce_finish<D, PAIR><<<(unsigned)((a.M + RPB - 1) / RPB), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  ce_pass<D, true, PAIR><<<(unsigned)p2, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  ce_loss<<<1, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // namespace

extern "C" {

int64_t srh_table_nce_ws_bytes(int64_t B, int64_t N, int32_t d) {
  if (B <= 0 || N <= 0 || (d != 64 && d != 128)) return 0;
  return ct_ws_bytes(B, N, d);
}

srh_status_t srh_table_nce_fwd_bwd(const srh_table_nce_problem_t* problems, int32_t n_problems, int32_t d, float tau,
                                   void* d_ws, void* stream) {
  SRH_REQUIRE(problems && d_ws, "table_nce_fwd_bwd: null argument");
  SRH_REQUIRE(n_problems >= 1 && n_problems <= kCtMaxProblems, "table_nce_fwd_bwd: 1..%d problems per call",
              kCtMaxProblems);
  SRH_REQUIRE(d == 64 || d == 128, "table_nce_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(tau > 0.f && std::isfinite(tau), "table_nce_fwd_bwd: temperature must be positive");
  CtArgs a{};
  a.inv_tau = 1.f / tau;
  char* ws = static_cast<char*>(d_ws);
  for (int k = 0; k < n_problems; ++k) {
    const srh_table_nce_problem_t& s = problems[k];
    SRH_REQUIRE(s.d_q && s.d_t && s.d_idx && s.d_loss && s.d_gq && s.d_gt, "table_nce_fwd_bwd: null tensor in problem %d", k);
    SRH_REQUIRE(s.B > 0 && s.B < (int64_t(1) << 31) && s.N > 0 && s.N < (int64_t(1) << 31),
                "table_nce_fwd_bwd: bad B / N in problem %d", k);
    CtProblem& p = a.p[k];
    p.q = s.d_q; p.t = s.d_t; p.idx = s.d_idx; p.B = s.B; p.N = s.N; p.scale = s.loss_scale;
    p.gscale = s.loss_scale * a.inv_tau;
    p.loss = s.d_loss; p.gq = s.d_gq; p.gt = s.d_gt;
    ws += ct_layout(p, ws, d);
  }
  hipStream_t st = srh::as_stream(stream);
  return d == 64 ? launch_ct<64, false>(a, n_problems, st) : launch_ct<128, false>(a, n_problems, st);
}

int64_t srh_batch_softmax_ws_bytes(int64_t B, int32_t d) {
  if (B <= 0 || (d != 64 && d != 128)) return 0;
  return ct_ws_bytes(B, B, d);
}

srh_status_t srh_batch_softmax_fwd_bwd(const float* d_u, const float* d_v, int64_t B, int32_t d, float tau,
                                       double* d_loss, float* d_gu, float* d_gv, void* d_ws, void* stream) {
  SRH_REQUIRE(d_u && d_v && d_loss && d_gu && d_gv && d_ws, "batch_softmax: null argument");
  SRH_REQUIRE(B > 0 && B < (int64_t(1) << 31), "batch_softmax: bad B");
  SRH_REQUIRE(d == 64 || d == 128, "batch_softmax: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(tau > 0.f && std::isfinite(tau), "batch_softmax: temperature must be positive");
  CtArgs a{};
  a.inv_tau = 1.f / tau;
  CtProblem& p = a.p[0];
  p.q = d_u; p.t = d_v; p.idx = nullptr; p.B = B; p.N = B;
  p.gscale = a.inv_tau / (float)B;
  p.loss = d_loss; p.gq = d_gu; p.gt = d_gv;
  ct_layout(p, d_ws, d);
  hipStream_t st = srh::as_stream(stream);
  return d == 64 ? launch_ct<64, true>(a, 1, st) : launch_ct<128, true>(a, 1, st);
}

int64_t srh_table_ce_ws_bytes(int64_t M, int64_t N, int32_t d) {
  if (M <= 0 || N <= 0 || (d != 64 && d != 128)) return 0;
  return ce_ws_bytes(M, N, d);
}

srh_status_t srh_table_ce_fwd_bwd(const float* d_h, int64_t M, const float* d_t, int64_t N, int32_t d,
                                  const int32_t* d_labels, float loss_scale, double* d_loss, float* d_gh, float* d_gt,
                                  void* d_ws, void* stream) {
  SRH_REQUIRE(M > 0 && M < (int64_t(1) << 31) && N > 0 && N < (int64_t(1) << 31), "table_ce_fwd_bwd: bad M / N");
  SRH_SUPPORTED(d == 64 || d == 128, "table_ce_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(d_h && d_t && d_labels && d_loss && d_gh && d_gt && d_ws, "table_ce_fwd_bwd: null argument");
  SRH_REQUIRE(std::isfinite(loss_scale), "table_ce_fwd_bwd: the loss scale must be finite");
  CeArgs a{};
  a.h = d_h; a.t = d_t; a.label = d_labels; a.M = M; a.N = N; a.scale = loss_scale;
  a.loss = d_loss; a.gh = d_gh; a.gt = d_gt;
  ce_layout(a, d_ws, d);
  hipStream_t st = srh::as_stream(stream);
  return d == 64 ? launch_ce<64, false>(a, st) : launch_ce<128, false>(a, st);
}

int64_t srh_pair_ce_ws_bytes(int64_t M, int64_t N, int32_t d) {
  if (M <= 0 || N <= 0 || (d != 64 && d != 128)) return 0;
  return ce_ws_bytes(M, N, d);
}

srh_status_t srh_pair_ce_fwd_bwd(const float* d_h, int64_t M, const float* d_t, int64_t N, int32_t d,
                                 const int32_t* d_labels, float inv_temp, float loss_scale, int32_t exclude_diagonal,
                                 int32_t add_gh_into_gt, double* d_loss, float* d_gh, float* d_gt, void* d_ws,
                                 void* stream) {
  SRH_REQUIRE(M > 0 && M < (int64_t(1) << 31) && N > 0 && N < (int64_t(1) << 31), "pair_ce_fwd_bwd: bad M / N");
  SRH_SUPPORTED(d == 64 || d == 128, "pair_ce_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(d_h && d_t && d_labels && d_loss && d_gh && d_gt && d_ws, "pair_ce_fwd_bwd: null argument");
  SRH_REQUIRE(std::isfinite(loss_scale), "pair_ce_fwd_bwd: the loss scale must be finite");
  SRH_REQUIRE(std::isfinite(inv_temp) && inv_temp > 0.f, "pair_ce_fwd_bwd: inv_temp must be positive and finite");
  SRH_REQUIRE(!exclude_diagonal || M == N, "pair_ce_fwd_bwd: exclude_diagonal needs M == N (got %lld x %lld)",
              (long long)M, (long long)N);
  SRH_REQUIRE(!exclude_diagonal || N > 1, "pair_ce_fwd_bwd: exclude_diagonal with N = 1 leaves no key in any row");
  SRH_REQUIRE(!add_gh_into_gt || M == N, "pair_ce_fwd_bwd: add_gh_into_gt needs M == N (got %lld x %lld)", (long long)M,
              (long long)N);
  SRH_REQUIRE(d_gh != d_gt, "pair_ce_fwd_bwd: d_gh and d_gt must be two buffers");
  CeArgs a{};
  a.h = d_h; a.t = d_t; a.label = d_labels; a.M = M; a.N = N; a.scale = loss_scale;
  a.inv_temp = inv_temp; a.gscale = loss_scale * inv_temp;
  a.exclude = exclude_diagonal ? 1 : 0; a.add_gh = add_gh_into_gt ? 1 : 0;
  a.loss = d_loss; a.gh = d_gh; a.gt = d_gt;
  ce_layout(a, d_ws, d);
  hipStream_t st = srh::as_stream(stream);
  return d == 64 ? launch_ce<64, true>(a, st) : launch_ce<128, true>(a, st);
}

}  // extern "C"

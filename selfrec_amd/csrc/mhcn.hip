// MHCN (model/graph/MHCN.py of the reference): the three pieces of its step that no other kernel here serves.
// DESIGN.md 4.21.  All arithmetic fp32, losses leave as float64, no float atomics: every reduction over rows runs in fixed
// chunks whose partials are summed in chunk order (chunked.hip), so a call returns the same bits every time.
//
// Gate (self_gating / self_supervised_gating, MHCN.py:79-83):  Y_c = X (.) sigmoid(X W_c + b_c), c < C <= 4, X (n x D),
//   W_c (D x D, the x @ W layout), b_c (D).
//   gate_fwd   a workgroup owns 64 rows (16 per wave) and holds them as the B operand of v_mfma_f32_16x16x4_f32; per gate
//              and 64 output columns the weight chunk W_c[:, j0 : j0 + 64] is staged in LDS (tw_fwd's scheme),
//              Z^T = W_c^T X^T comes out of the MFMA and takes bias, sigmoid and the multiply on the accumulator: every
//              gate of the call from one read of X.
//   gate_bwd   S is RECOMPUTED (the same product), not saved: dZ_c = dY_c (.) X (.) S_c (1 - S_c) is formed on the
//              accumulator, written for the weight gradient, and fed straight back as the B operand of
//              dX^T += W_c dZ_c^T from the SAME staged chunk (the accumulator layout is the B layout with the k order
//              4 * (lane >> 4) + reg); dY_c (.) S_c lands on the accumulator element of the same (row, column).
//   gate_wgrad dW_c = X^T dZ_c per chunk of kRowChunk rows on the MFMA; db_c the column sums per chunk; both summed in
//              chunk order (chunked.hip).
// Channel mix (channel_attention, MHCN.py:85-93): w_c[r] = E_c[r] . q, s[r] = softmax_c w_c[r],
//   out[r] = sum_c s_c[r] E_c[r] + beta X[r].  One wave per row, forward and backward; dq is a chunk-ordered reduction.
// MIM (hierarchical_self_supervision, MHCN.py:159-181), forward and backward in one call: see srh_mim_fwd_bwd below.
#include <algorithm>
#include <cmath>

#include "rowtile.h"

namespace {

using namespace srh;

constexpr int kMaxGates = 4;
constexpr int kJc = 64;                 // output columns per staged weight chunk
constexpr int kLds = kJc + 4;           // LDS row stride (floats) of the staged chunk
constexpr int kRowChunk = 256;          // rows per partial of the gate's weight-gradient reductions
constexpr int kMixChunk = 64;           // rows per partial of the mix / MIM reductions (16 per wave, ascending)

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
// softplus, finite for every finite x
__device__ __forceinline__ float softplusf_(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// ---- gate --------------------------------------------------------------------------------------------------------------
struct GateArgs {
  const float* x;
  const float* w;     // C x D x D
  const float* b;     // C x D
  int64_t n;
  int C;
  float* y;           // fwd: C x n x D
  const float* gy;    // bwd: C x n x D
  float* gx;          // bwd: n x D
  float* dz;          // bwd workspace: C x n x D
};

// W_c[:, j0 : j0 + 64] into wn[k][j] (row stride kLds)
template <int D>
__device__ __forceinline__ void stage_w(float* wn, const float* __restrict__ wc, int j0) {
  for (int e = threadIdx.x; e < D * (kJc / 4); e += 256) {
    const int k = e / (kJc / 4), q = e % (kJc / 4);
    *reinterpret_cast<float4*>(&wn[k * kLds + 4 * q]) = reinterpret_cast<const float4*>(wc + (int64_t)k * D + j0)[q];
  }
}

// acc[reg] = (X W_c)[row j16][j0 + 16 s + 4 g + reg]: A = the staged chunk read down its columns, B = the row's registers
template <int D>
__device__ __forceinline__ f32x4 gate_z(const float* wn, int s, int j16, int g, const float (&rf)[D / 4]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* acol = &wn[g * kLds + 16 * s + j16];
#pragma unroll
  for (int k = 0; k < D / 4; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(acol[4 * k * kLds], rf[k], acc, 0, 0, 0);
  return acc;
}

template <int D, bool BWD>
__global__ __launch_bounds__(256) void gate_kernel(GateArgs a) {
  __shared__ float wn[D * kLds];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int64_t r = (int64_t)blockIdx.x * 64 + wave * 16 + j16;
  const bool rok = r < a.n;
  float rf[D / 4];
#pragma unroll
  for (int s = 0; s < D / 4; ++s) rf[s] = rok ? a.x[r * D + 4 * s + g] : 0.f;
  f32x4 dxt[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t) dxt[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < a.C; ++c) {
    const float* wc = a.w + (int64_t)c * D * D;
    const float* bc = a.b + (int64_t)c * D;
#pragma unroll
    for (int jc = 0; jc < D / kJc; ++jc) {
      const int j0 = jc * kJc;
      __syncthreads();
      stage_w<D>(wn, wc, j0);
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kJc / 16; ++s) {
        const f32x4 z = gate_z<D>(wn, s, j16, g, rf);
        const int col = j0 + 16 * s + 4 * g;
        const float4 bv = *reinterpret_cast<const float4*>(bc + col);
        const float4 xv = rok ? *reinterpret_cast<const float4*>(a.x + r * D + col) : f4_zero();
        const float sg[4] = {sigmoidf_(z[0] + bv.x), sigmoidf_(z[1] + bv.y), sigmoidf_(z[2] + bv.z), sigmoidf_(z[3] + bv.w)};
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
        if constexpr (!BWD) {
          if (rok)
            *reinterpret_cast<float4*>(a.y + ((int64_t)c * a.n + r) * D + col) =
                make_float4(xs[0] * sg[0], xs[1] * sg[1], xs[2] * sg[2], xs[3] * sg[3]);
        } else {
          const float4 gv = rok ? *reinterpret_cast<const float4*>(a.gy + ((int64_t)c * a.n + r) * D + col) : f4_zero();
          const float gs[4] = {gv.x, gv.y, gv.z, gv.w};
          float dz[4];
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            dz[reg] = gs[reg] * xs[reg] * (sg[reg] * (1.f - sg[reg]));
            dxt[jc * (kJc / 16) + s][reg] = fmaf(gs[reg], sg[reg], dxt[jc * (kJc / 16) + s][reg]);
          }
          if (rok) *reinterpret_cast<float4*>(a.dz + ((int64_t)c * a.n + r) * D + col) = make_float4(dz[0], dz[1], dz[2], dz[3]);
          // dX^T[k][row] += sum_j W_c[k][j0 + 16 s + j] dZ^T[j][row], j = 4 g + reg
#pragma unroll
          for (int t = 0; t < D / 16; ++t) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
              dxt[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wn[(16 * t + j16) * kLds + 16 * s + 4 * g + reg], dz[reg], dxt[t],
                                                            0, 0, 0);
          }
        }
      }
    }
  }
  if constexpr (BWD) {
    // dxt[t][reg] = dX[row j16][16 t + 4 g + reg]
    if (!rok) return;
#pragma unroll
    for (int t = 0; t < D / 16; ++t)
      *reinterpret_cast<float4*>(a.gx + r * D + 16 * t + 4 * g) = make_float4(dxt[t][0], dxt[t][1], dxt[t][2], dxt[t][3]);
  }
}

// part[(z * C + c)][k][j] = sum over rows r of chunk z, ascending in steps of 16, of X[r][k] dZ_c[r][j]
// grid (D / 64 column tiles, D / 64 row tiles, chunks * C); 64 x 64 tile per workgroup, 16 rows of it per wave.  The staging
// and MFMA order of chunked.hip's gemm64 with D at compile time and no bounds checks: that one measured 15 % slower on
// the gate backward (profiles/NOTES_rowtile.md).
template <int D>
__global__ __launch_bounds__(256) void gate_wgrad(const float* __restrict__ x, const float* __restrict__ dz, int64_t n, int C,
                                                  float* __restrict__ part) {
  __shared__ float as[64 * 17];   // as[k][r]
  __shared__ float bs[16 * 68];   // bs[r][j]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int k0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int64_t z = blockIdx.z / C;
  const int c = blockIdx.z % C;
  const float* dzc = dz + (int64_t)c * n * D;
  const int64_t rb = z * kRowChunk, re = std::min<int64_t>(rb + kRowChunk, n);
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = rb; r0 < re; r0 += 16) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = threadIdx.x + 256 * u;
      const int rr = e / 64, cc = e % 64;
      const int64_t gr = r0 + rr;
      const bool ok = gr < re;
      as[cc * 17 + rr] = ok ? x[gr * D + k0 + cc] : 0.f;
      bs[rr * 68 + cc] = ok ? dzc[gr * D + j0 + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float av = as[(16 * wave + j16) * 17 + 4 * q + g];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bs[(4 * q + g) * 68 + 16 * t + j16], acc[t], 0, 0, 0);
    }
  }
  float* out = part + (int64_t)blockIdx.z * D * D;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + 16 * t + j16;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) out[(int64_t)(k0 + 16 * wave + 4 * g + reg) * D + j] = acc[t][reg];
  }
}

struct GateBwdWs {
  float* dz;       // C x n x D
  float* part_w;   // chunks x C x D x D
  float* part_b;   // chunks x C x D
};
// null ws measures, a workspace carves; returns the bytes
int64_t gate_bwd_layout(GateBwdWs& w, void* ws, int64_t n, int D, int C) {
  Carver cv(ws);
  const int64_t z = ceil_div(n, kRowChunk);
  cv.take(w.dz, (int64_t)C * n * D);
  cv.take(w.part_w, z * C * D * D);
  cv.take(w.part_b, z * C * D);
  return cv.used;
}

template <int D>
srh_status_t launch_gate_fwd(const GateArgs& a, hipStream_t st) {
  gate_kernel<D, false><<<(unsigned)ceil_div(a.n, 64), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

template <int D>
srh_status_t launch_gate_bwd(GateArgs a, float* gw, float* gb, void* ws, hipStream_t st) {
  const int64_t z = ceil_div(a.n, kRowChunk);
  const int C = a.C;
  GateBwdWs w;
  gate_bwd_layout(w, ws, a.n, D, C);
  a.dz = w.dz;
  gate_kernel<D, true><<<(unsigned)ceil_div(a.n, 64), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  gate_wgrad<D><<<dim3(D / 64, D / 64, (unsigned)(z * C)), 256, 0, st>>>(a.x, w.dz, a.n, C, w.part_w);
  SRH_LAUNCH_CHECK();
  srh_status_t s;
  if ((s = colsum_chunks(w.dz, a.n, D, C, kRowChunk, w.part_b, st)) != SRH_OK) return s;
  if ((s = reduce_chunks(w.part_w, z, (int64_t)C * D * D, 1.f, gw, st)) != SRH_OK) return s;
  return reduce_chunks(w.part_b, z, (int64_t)C * D, 1.f, gb, st);
}

// ---- channel mix -------------------------------------------------------------------------------------------------------
// wp[wave][e]: the four waves' partials of a chunk's D column sums, added in wave order into row blockIdx.x of part
template <int D>
__device__ __forceinline__ void wave_partials_store(const float* wp, float* __restrict__ part) {
  if (threadIdx.x < D) {
    const int e = threadIdx.x;
    part[(int64_t)blockIdx.x * D + e] = ((wp[e] + wp[D + e]) + wp[2 * D + e]) + wp[3 * D + e];
  }
}

struct MixArgs {
  const float* e[3];
  const float* q;
  const float* x;      // optional addend
  float beta;
  int64_t n;
  float* out;          // fwd
  float* score;        // fwd: written; bwd: read   (n x 3)
  const float* gout;   // bwd
  float* ge[3];
  float* gx;           // optional
  float* part;         // bwd workspace: chunks x D
};

// one wave per row; lane l owns columns l (and l + 64 at D = 128)
template <int D>
__global__ __launch_bounds__(256) void mix_fwd(MixArgs a) {
  constexpr int Q = D / 64;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= a.n) return;  // (whole waves leave together)
  float ev[3][Q], w[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      ev[c][k] = a.e[c][r * D + lane + 64 * k];
      s = fmaf(ev[c][k], a.q[lane + 64 * k], s);
    }
    w[c] = wave_sum_f(s);
  }
  const float m = fmaxf(w[0], fmaxf(w[1], w[2]));
  const float e0 = expf(w[0] - m), e1 = expf(w[1] - m), e2 = expf(w[2] - m);
  const float inv = 1.f / (e0 + e1 + e2);
  const float s0 = e0 * inv, s1 = e1 * inv, s2 = e2 * inv;
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    float o = fmaf(s2, ev[2][k], fmaf(s1, ev[1][k], s0 * ev[0][k]));
    if (a.x) o = fmaf(a.beta, a.x[r * D + lane + 64 * k], o);
    a.out[r * D + lane + 64 * k] = o;
  }
  if (lane < 3) a.score[r * 3 + lane] = lane == 0 ? s0 : lane == 1 ? s1 : s2;
}

// a workgroup owns one chunk of kMixChunk rows; wave v takes rows v, v + 4, ... of it in ascending order and keeps its own
// partial of dq; the four partials are added in wave order
template <int D>
__global__ __launch_bounds__(256) void mix_bwd(MixArgs a) {
  constexpr int Q = D / 64;
  __shared__ float wp[4 * D];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t rb = (int64_t)blockIdx.x * kMixChunk;
  const int64_t re = std::min<int64_t>(rb + kMixChunk, a.n);
  float dq[Q], qv[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    dq[k] = 0.f;
    qv[k] = a.q[lane + 64 * k];
  }
  for (int64_t r = rb + wave; r < re; r += 4) {
    float ev[3][Q], gv[Q], dots[3];
#pragma unroll
    for (int k = 0; k < Q; ++k) gv[k] = a.gout[r * D + lane + 64 * k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < Q; ++k) {
        ev[c][k] = a.e[c][r * D + lane + 64 * k];
        s = fmaf(ev[c][k], gv[k], s);
      }
      dots[c] = wave_sum_f(s);
    }
    const float s0 = a.score[r * 3], s1 = a.score[r * 3 + 1], s2 = a.score[r * 3 + 2];
    const float mean = fmaf(s2, dots[2], fmaf(s1, dots[1], s0 * dots[0]));
    const float dw[3] = {s0 * (dots[0] - mean), s1 * (dots[1] - mean), s2 * (dots[2] - mean)};
    const float sc[3] = {s0, s1, s2};
#pragma unroll
    for (int k = 0; k < Q; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a.ge[c][r * D + lane + 64 * k] = fmaf(dw[c], qv[k], sc[c] * gv[k]);
        dq[k] = fmaf(dw[c], ev[c][k], dq[k]);
      }
      if (a.gx) a.gx[r * D + lane + 64 * k] = a.beta * gv[k];
    }
  }
#pragma unroll
  for (int k = 0; k < Q; ++k) wp[wave * D + lane + 64 * k] = dq[k];
  __syncthreads();
  wave_partials_store<D>(wp, a.part);
}

// ---- MIM ---------------------------------------------------------------------------------------------------------------
struct MimArgs {
  const float* em;
  const float* edge;
  const int32_t* p[3];   // p1, p2, p3
  const int32_t* c[2];   // c2, c3
  int64_t n;
  float scale, inv_n;
  double* loss;
  float* gem;
  float* gedge;
  // workspace
  int32_t* ip[3];        // inverse row permutations (-1: no such row)
  int32_t* ic[2];        // inverse column permutations
  float* kk;             // 3 x n   scale * sigmoid(difference) per row: k1, k2, k3
  float* gpart;          // chunks x D   column sums of edge per chunk, then of the gradient of g
  float* g;              // D   column mean of edge
  float* dg;             // D   dL/dg / n
  double* lpart;         // chunks
  int64_t chunks;
};

// the workspace of a.n rows: null ws measures, a workspace carves; returns the bytes.  The ORDER of the first three
// lines matters: launch_mim sets ip[0] .. kk to -1 with one memset, so the five inverse maps lie back to back with kk
// right behind them.
int64_t mim_layout(MimArgs& a, void* ws, int D) {
  Carver w(ws);
  a.chunks = ceil_div(a.n, kMixChunk);
  for (int i = 0; i < 3; ++i) w.take(a.ip[i], a.n);
  for (int i = 0; i < 2; ++i) w.take(a.ic[i], D);
  w.take(a.kk, 3 * a.n);
  w.take(a.gpart, a.chunks * D);
  w.take(a.g, D);
  w.take(a.dg, D);
  w.take(a.lpart, a.chunks);
  return w.used;
}

// the inverse permutations (the workspace holds -1 everywhere before); an entry outside its range is left out
template <int D>
__global__ __launch_bounds__(256) void mim_inverse(MimArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int32_t t = a.p[k][i];
      if (t >= 0 && t < a.n) a.ip[k][t] = (int32_t)i;
    }
  }
  if (i < D) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int32_t t = a.c[k][i];
      if (t >= 0 && t < D) a.ic[k][t] = (int32_t)i;
    }
  }
}

__device__ __forceinline__ bool in_range(int32_t t, int64_t n) { return t >= 0 && t < n; }

// the row terms: a workgroup owns one chunk of kMixChunk rows, wave v its rows v, v + 4, ...; per row the six inner
// products, the three loss terms and the three gradient factors; per chunk the loss and the gradient of g, the four waves'
// partials added in wave order
template <int D>
__global__ __launch_bounds__(256) void mim_rows(MimArgs a) {
  constexpr int Q = D / 64;
  __shared__ float wp[4 * D];
  __shared__ double lp[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t n = a.n;
  const int64_t rb = (int64_t)blockIdx.x * kMixChunk;
  const int64_t re = std::min<int64_t>(rb + kMixChunk, n);
  float gv[Q], dgp[Q];
  int32_t c2[Q], c3[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    gv[k] = a.g[lane + 64 * k];
    dgp[k] = 0.f;
    c2[k] = a.c[0][lane + 64 * k];
    c3[k] = a.c[1][lane + 64 * k];
    if (!in_range(c2[k], D)) c2[k] = -1;
    if (!in_range(c3[k], D)) c3[k] = -1;
  }
  double lsum = 0.0;
  for (int64_t r = rb + wave; r < re; r += 4) {
    const int32_t r1 = a.p[0][r], r2 = a.p[1][r], r3 = a.p[2][r];
    const bool ok1 = in_range(r1, n), ok2 = in_range(r2, n), ok3 = in_range(r3, n);
    float pos = 0.f, n1 = 0.f, n2 = 0.f, gp = 0.f, gn = 0.f;
    float e3[Q], ed[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      const int col = lane + 64 * k;
      const float em = a.em[r * D + col];
      ed[k] = a.edge[r * D + col];
      const float em1 = ok1 ? a.em[(int64_t)r1 * D + col] : 0.f;
      const float e2 = (ok2 && c2[k] >= 0) ? a.edge[(int64_t)r2 * D + c2[k]] : 0.f;
      e3[k] = (ok3 && c3[k] >= 0) ? a.edge[(int64_t)r3 * D + c3[k]] : 0.f;
      pos = fmaf(em, ed[k], pos);
      n1 = fmaf(em1, ed[k], n1);
      n2 = fmaf(em, e2, n2);
      gp = fmaf(gv[k], ed[k], gp);
      gn = fmaf(gv[k], e3[k], gn);
    }
    pos = wave_sum_f(pos); n1 = wave_sum_f(n1); n2 = wave_sum_f(n2); gp = wave_sum_f(gp); gn = wave_sum_f(gn);
    const float x1 = n1 - pos, x2 = n2 - n1, x3 = gn - gp;
    lsum += (double)softplusf_(x1) + (double)softplusf_(x2) + (double)softplusf_(x3);
    const float k3 = a.scale * sigmoidf_(x3);
    if (lane == 0) {
      a.kk[r] = a.scale * sigmoidf_(x1);
      a.kk[n + r] = a.scale * sigmoidf_(x2);
      a.kk[2 * n + r] = k3;
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) dgp[k] = fmaf(k3, e3[k] - ed[k], dgp[k]);
  }
#pragma unroll
  for (int k = 0; k < Q; ++k) wp[wave * D + lane + 64 * k] = dgp[k];
  if (lane == 0) lp[wave] = lsum;
  __syncthreads();
  wave_partials_store<D>(wp, a.gpart);
  if (threadIdx.x == 0) a.lpart[blockIdx.x] = ((lp[0] + lp[1]) + lp[2]) + lp[3];
}

// dg = (sum of the chunk partials in order) / n; the loss = scale * (its chunk partials in order).  One workgroup.
template <int D>
__global__ __launch_bounds__(256) void mim_finish(MimArgs a) {
  if (threadIdx.x < D) {
    float s = 0.f;
    for (int64_t z = 0; z < a.chunks; ++z) s += a.gpart[z * D + threadIdx.x];
    a.dg[threadIdx.x] = s * a.inv_n;
  }
  if (threadIdx.x == 255) {
    double s = 0.0;
    for (int64_t z = 0; z < a.chunks; ++z) s += a.lpart[z];
    a.loss[0] = (double)a.scale * s;
  }
}

// the gradients: one wave per row t, every scatter of the forward taken as a gather through the inverse permutation
//   dEm[t]      = -k1_t edge_t + (k1 - k2)_a edge_a [a = ip1[t]] + k2_t edge[p2[t]][c2[.]]
//   dEdge[t][m] = -k1_t em_t[m] + (k1 - k2)_t em_{p1[t]}[m] + k2_b em_b[ic2[m]] [b = ip2[t]] - k3_t g[m] + k3_e g[ic3[m]]
//                 [e = ip3[t]] + dg[m]
template <int D>
__global__ __launch_bounds__(256) void mim_grads(MimArgs a) {
  constexpr int Q = D / 64;
  const int64_t n = a.n;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= n) return;
  const float k1 = a.kk[t], k2 = a.kk[n + t], k3 = a.kk[2 * n + t];
  const int32_t r1 = a.p[0][t], r2 = a.p[1][t];
  const bool ok1 = in_range(r1, n), ok2 = in_range(r2, n);
  const int32_t ia = a.ip[0][t], ib = a.ip[1][t], ie = a.ip[2][t];
  const float ka = ia >= 0 ? a.kk[ia] - a.kk[n + ia] : 0.f;
  const float kb = ib >= 0 ? a.kk[n + ib] : 0.f;
  const float ke = ie >= 0 ? a.kk[2 * n + ie] : 0.f;
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int col = lane + 64 * k;
    const int32_t c2 = a.c[0][col];
    const int32_t j2 = a.ic[0][col], j3 = a.ic[1][col];
    const float edge_t = a.edge[t * D + col];
    const float edge_a = ia >= 0 ? a.edge[(int64_t)ia * D + col] : 0.f;
    const float e2 = (ok2 && in_range(c2, D)) ? a.edge[(int64_t)r2 * D + c2] : 0.f;
    a.gem[t * D + col] = fmaf(k2, e2, fmaf(ka, edge_a, -k1 * edge_t));
    const float em_t = a.em[t * D + col];
    const float em_1 = ok1 ? a.em[(int64_t)r1 * D + col] : 0.f;
    const float em_b = (ib >= 0 && j2 >= 0) ? a.em[(int64_t)ib * D + j2] : 0.f;
    const float g_m = a.g[col];
    const float g_3 = j3 >= 0 ? a.g[j3] : 0.f;
    float v = fmaf(k1 - k2, em_1, -k1 * em_t);
    v = fmaf(kb, em_b, v);
    v = fmaf(-k3, g_m, v);
    v = fmaf(ke, g_3, v);
    a.gedge[t * D + col] = v + a.dg[col];
  }
}

template <int D>
srh_status_t launch_mim(MimArgs& a, void* ws, hipStream_t st) {
  mim_layout(a, ws, D);
  // the inverse maps start at -1
  SRH_HIP(hipMemsetAsync(a.ip[0], 0xFF, (size_t)((char*)a.kk - (char*)a.ip[0]), st));
  mim_inverse<D><<<(unsigned)ceil_div(std::max<int64_t>(a.n, D), 256), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  srh_status_t s;
  if ((s = colsum_chunks(a.edge, a.n, D, 1, kMixChunk, a.gpart, st)) != SRH_OK) return s;
  if ((s = reduce_chunks(a.gpart, a.chunks, D, a.inv_n, a.g, st)) != SRH_OK) return s;
  mim_rows<D><<<(unsigned)a.chunks, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  mim_finish<D><<<1, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  mim_grads<D><<<(unsigned)ceil_div(a.n, 4), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

inline bool bad_n(int64_t n) { return n < 0 || n >= (int64_t(1) << 31) / 128; }

}  // namespace

extern "C" {

srh_status_t srh_gate_fwd_f32(const float* d_x, const float* d_w, const float* d_b, int64_t n, int32_t d, int32_t n_gates,
                              float* d_y, void* stream) {
  SRH_SUPPORTED(d == 64 || d == 128, "gate_fwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_SUPPORTED(n_gates >= 1 && n_gates <= kMaxGates, "gate_fwd: %d gates unsupported (1..%d)", n_gates, kMaxGates);
  SRH_REQUIRE(!bad_n(n), "gate_fwd: bad n");
  if (n == 0) return SRH_OK;
  SRH_REQUIRE(d_x && d_w && d_b && d_y, "gate_fwd: null argument");
  GateArgs a{};
  a.x = d_x; a.w = d_w; a.b = d_b; a.n = n; a.C = n_gates; a.y = d_y;
  hipStream_t st = as_stream(stream);
  return d == 64 ? launch_gate_fwd<64>(a, st) : launch_gate_fwd<128>(a, st);
}

int64_t srh_gate_bwd_ws_bytes(int64_t n, int32_t d, int32_t n_gates) {
  if (n <= 0 || bad_n(n) || (d != 64 && d != 128) || n_gates < 1 || n_gates > kMaxGates) return 0;
  GateBwdWs w;
  return gate_bwd_layout(w, nullptr, n, d, n_gates);
}

srh_status_t srh_gate_bwd_f32(const float* d_x, const float* d_w, const float* d_b, const float* d_gy, int64_t n, int32_t d,
                              int32_t n_gates, float* d_gx, float* d_gw, float* d_gb, void* d_ws, void* stream) {
  SRH_SUPPORTED(d == 64 || d == 128, "gate_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_SUPPORTED(n_gates >= 1 && n_gates <= kMaxGates, "gate_bwd: %d gates unsupported (1..%d)", n_gates, kMaxGates);
  SRH_REQUIRE(!bad_n(n), "gate_bwd: bad n");
  SRH_REQUIRE(d_gw && d_gb, "gate_bwd: null argument");
  hipStream_t st = as_stream(stream);
  if (n == 0) {   // no rows: the weight gradients are zero
    SRH_HIP(hipMemsetAsync(d_gw, 0, sizeof(float) * (size_t)n_gates * d * d, st));
    SRH_HIP(hipMemsetAsync(d_gb, 0, sizeof(float) * (size_t)n_gates * d, st));
    return SRH_OK;
  }
  SRH_REQUIRE(d_x && d_w && d_b && d_gy && d_gx && d_ws, "gate_bwd: null argument");
  GateArgs a{};
  a.x = d_x; a.w = d_w; a.b = d_b; a.n = n; a.C = n_gates; a.gy = d_gy; a.gx = d_gx;
  return d == 64 ? launch_gate_bwd<64>(a, d_gw, d_gb, d_ws, st) : launch_gate_bwd<128>(a, d_gw, d_gb, d_ws, st);
}

srh_status_t srh_chan_mix_fwd_f32(const float* d_e1, const float* d_e2, const float* d_e3, const float* d_q,
                                  const float* d_x, float beta, int64_t n, int32_t d, float* d_out, float* d_score,
                                  void* stream) {
  SRH_SUPPORTED(d == 64 || d == 128, "chan_mix_fwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(!bad_n(n), "chan_mix_fwd: bad n");
  SRH_REQUIRE(std::isfinite(beta), "chan_mix_fwd: beta must be finite");
  if (n == 0) return SRH_OK;
  SRH_REQUIRE(d_e1 && d_e2 && d_e3 && d_q && d_out && d_score, "chan_mix_fwd: null argument");
  MixArgs a{};
  a.e[0] = d_e1; a.e[1] = d_e2; a.e[2] = d_e3; a.q = d_q; a.x = d_x; a.beta = beta; a.n = n; a.out = d_out; a.score = d_score;
  hipStream_t st = as_stream(stream);
  if (d == 64) mix_fwd<64><<<(unsigned)ceil_div(n, 4), 256, 0, st>>>(a);
  else mix_fwd<128><<<(unsigned)ceil_div(n, 4), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_chan_mix_bwd_ws_bytes(int64_t n, int32_t d) {
  if (n <= 0 || bad_n(n) || (d != 64 && d != 128)) return 0;
  return align256(4 * ceil_div(n, kMixChunk) * d);
}

srh_status_t srh_chan_mix_bwd_f32(const float* d_e1, const float* d_e2, const float* d_e3, const float* d_q,
                                  const float* d_score, const float* d_gout, float beta, int64_t n, int32_t d, float* d_ge1,
                                  float* d_ge2, float* d_ge3, float* d_gx, float* d_gq, void* d_ws, void* stream) {
  SRH_SUPPORTED(d == 64 || d == 128, "chan_mix_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(!bad_n(n), "chan_mix_bwd: bad n");
  SRH_REQUIRE(std::isfinite(beta), "chan_mix_bwd: beta must be finite");
  SRH_REQUIRE(d_gq, "chan_mix_bwd: null argument");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    SRH_HIP(hipMemsetAsync(d_gq, 0, sizeof(float) * (size_t)d, st));
    return SRH_OK;
  }
  SRH_REQUIRE(d_e1 && d_e2 && d_e3 && d_q && d_score && d_gout && d_ge1 && d_ge2 && d_ge3 && d_ws,
              "chan_mix_bwd: null argument");
  MixArgs a{};
  a.e[0] = d_e1; a.e[1] = d_e2; a.e[2] = d_e3; a.q = d_q; a.beta = beta; a.n = n; a.score = const_cast<float*>(d_score);
  a.gout = d_gout; a.ge[0] = d_ge1; a.ge[1] = d_ge2; a.ge[2] = d_ge3; a.gx = d_gx; a.part = static_cast<float*>(d_ws);
  const int64_t z = ceil_div(n, kMixChunk);
  if (d == 64) mix_bwd<64><<<(unsigned)z, 256, 0, st>>>(a);
  else mix_bwd<128><<<(unsigned)z, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return reduce_chunks(a.part, z, d, 1.f, d_gq, st);
}

int64_t srh_mim_ws_bytes(int64_t n, int32_t d) {
  if (n <= 0 || bad_n(n) || (d != 64 && d != 128)) return 0;
  MimArgs a{};
  a.n = n;
  return mim_layout(a, nullptr, d);
}

srh_status_t srh_mim_fwd_bwd(const srh_mim_args_t* args, void* d_ws, void* stream) {
  SRH_REQUIRE(args, "mim_fwd_bwd: null argument");
  const srh_mim_args_t& s = *args;
  SRH_SUPPORTED(s.d == 64 || s.d == 128, "mim_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", s.d);
  SRH_REQUIRE(!bad_n(s.n), "mim_fwd_bwd: bad n");
  SRH_REQUIRE(std::isfinite(s.loss_scale), "mim_fwd_bwd: the loss scale must be finite");
  SRH_REQUIRE(s.d_loss, "mim_fwd_bwd: null loss");
  hipStream_t st = as_stream(stream);
  if (s.n == 0) {
    SRH_HIP(hipMemsetAsync(s.d_loss, 0, sizeof(double), st));
    return SRH_OK;
  }
  SRH_REQUIRE(d_ws && s.d_em && s.d_edge && s.d_gem && s.d_gedge, "mim_fwd_bwd: null tensor");
  MimArgs a{};
  for (int i = 0; i < 3; ++i) {
    SRH_REQUIRE(s.d_row_perm[i], "mim_fwd_bwd: null row permutation %d", i);
    a.p[i] = s.d_row_perm[i];
  }
  for (int i = 0; i < 2; ++i) {
    SRH_REQUIRE(s.d_col_perm[i], "mim_fwd_bwd: null column permutation %d", i);
    a.c[i] = s.d_col_perm[i];
  }
  a.em = s.d_em; a.edge = s.d_edge; a.n = s.n; a.scale = s.loss_scale; a.inv_n = (float)(1.0 / (double)s.n);
  a.loss = s.d_loss; a.gem = s.d_gem; a.gedge = s.d_gedge;
  return s.d == 64 ? launch_mim<64>(a, d_ws, st) : launch_mim<128>(a, d_ws, st);
}

}  // extern "C"

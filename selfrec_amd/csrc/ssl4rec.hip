// SSL4Rec (reference model/graph/SSL4Rec.py): the two MLP towers and batch_softmax_loss.  DESIGN.md 4.8.
//
// Tower (DNN_Encoder.user_tower / item_tower):  Y = tanh(W2 relu(W1 X + b1) + b2),  X (n x 64), W1 (1024 x 64),
// W2 (128 x 1024), the nn.Linear layouts.
//   srh_tower_fwd_f32   one launch.  A workgroup owns 64 rows (16 per wave) and walks the hidden layer in chunks of 64
//                       units: the chunk's W1 rows and W2 columns are staged in LDS, H^T = W1c X^T comes out of the f32
//                       MFMA, takes bias + ReLU on the accumulator and is fed straight back as the B operand of
//                       Y^T += W2c H^T (the accumulator layout of v_mfma_f32_16x16x4_f32 is its B layout with the k order
//                       4 * (lane >> 4) + reg, matched by the A operand): the GEMM -> GEMM seam never leaves registers.
//                       The rows are gathered from an embedding table (optional) and take a feature-dropout mask
//                       (optional): injected, or drawn from the counter RNG of the SpMM epilogue (common.h).  H and the
//                       effective input are written for the backward pass.
//   srh_tower_bwd_f32   dZ2 = dY (1 - Y^2); dZ1 = (dZ2 W2) [H > 0]; dX = (dZ1 W1) m  (m: the dropout multiplier);
//                       dW2 = dZ2^T H, dW1 = dZ1^T X, db2 / db1 the column sums.  The products run on one strided MFMA
//                       GEMM kernel; the reductions over rows are cut into fixed chunks of kRowChunk rows whose partials
//                       are summed in chunk order: no float atomics, the same bits on every call.
//   srh_rows_segment_sum_f32  the deterministic scatter of dX into the embedding-table gradient: rows grouped by the
//                       host's stable sort of the ids, each table row sums its rows in that order.
//
// batch_softmax_loss (util/loss_torch.py:25-32):  u = normalize(U), v = normalize(V), p_b = e_bb / sum_j e_bj with
// e = exp(u.v / tau);  loss = mean_b -log(p_b + 1e-5).  With w_b = p_b / (p_b + 1e-5) the gradient is InfoNCE's row
// gradient scaled by w_b:  dL/ds_bj = w_b (P_bj - [b == j]) / (B tau).  The B x B logits are never materialised: the
// two-pass structure of the table InfoNCE kernel (ncl.hip), with w_b carried into the column pass.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace {

using namespace srh;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kIn = 64, kHid = 1024, kOut = 128;
constexpr int kHc = 64;                 // hidden units per chunk of the forward walk
constexpr int kLds = kHc + 4;           // LDS row stride (floats) of the staged chunk
constexpr int kRowChunk = 256;          // rows per partial of the weight-gradient reductions
constexpr double kBsEps = 1e-5;         // loss_torch.py:31 (10e-6)
constexpr float kNormEps = 1e-12f;

inline int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }
__host__ __device__ inline int64_t row_chunks(int64_t n) { return (n + kRowChunk - 1) / kRowChunk; }

struct FwdArgs {
  const float* table;
  const int32_t* idx;
  int64_t n, n_table, mask_row0;
  const float *w1, *b1, *w2, *b2;
  const uint8_t* mask_in;
  uint8_t* mask_out;
  uint32_t seed_lo, seed_hi;
  uint64_t ctr;
  float drop_p, drop_scale;
  float* x_out;
  float* hidden;
  float* out;
};

// ---- tower forward ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tw_fwd(FwdArgs a) {
  __shared__ float w1c[kHc * kLds];   // w1c[h][k]  = W1[h0 + h][k]
  __shared__ float w2c[kOut * kLds];  // w2c[o][h]  = W2[o][h0 + h]
  __shared__ float b1c[kHc];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int64_t r = (int64_t)blockIdx.x * 64 + wave * 16 + j16;
  const bool rok = r < a.n;
  int64_t src = r;
  if (a.idx) src = rok ? (int64_t)a.idx[r] : -1;
  const bool sok = rok && src >= 0 && src < a.n_table;  // (an id outside the table reads nothing: a zero row)
  const bool masked = rok && r >= a.mask_row0;
  const int64_t mr = r - a.mask_row0;

  // B operand of the first product: X[r][4s + g]
  float rf[kIn / 4];
#pragma unroll
  for (int s = 0; s < kIn / 4; ++s) {
    const int c = 4 * s + g;
    float x = sok ? a.table[src * kIn + c] : 0.f;
    if (masked) {
      bool keep;
      if (a.mask_in) {
        keep = a.mask_in[mr * kIn + c] != 0;
      } else {
        const uint4 w = counter_rng4(a.ctr + (uint64_t)mr, (uint32_t)s, a.seed_lo, a.seed_hi);
        const uint32_t word = g == 0 ? w.x : g == 1 ? w.y : g == 2 ? w.z : w.w;
        keep = u01(word) >= a.drop_p;
      }
      if (a.mask_out) a.mask_out[mr * kIn + c] = keep ? 1 : 0;
      x = x * (keep ? a.drop_scale : 0.f);
    }
    if (rok && a.x_out) a.x_out[r * kIn + c] = x;
    rf[s] = x;
  }

  f32x4 yt[kOut / 16];
#pragma unroll
  for (int t = 0; t < kOut / 16; ++t) yt[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int h0 = 0; h0 < kHid; h0 += kHc) {
    __syncthreads();
    for (int e = threadIdx.x; e < kHc * (kIn / 4); e += 256) {
      const int h = e / (kIn / 4), v = e % (kIn / 4);
      *reinterpret_cast<float4*>(&w1c[h * kLds + 4 * v]) = reinterpret_cast<const float4*>(a.w1 + (int64_t)(h0 + h) * kIn)[v];
    }
    for (int e = threadIdx.x; e < kOut * (kHc / 4); e += 256) {
      const int o = e / (kHc / 4), v = e % (kHc / 4);
      *reinterpret_cast<float4*>(&w2c[o * kLds + 4 * v]) =
          reinterpret_cast<const float4*>(a.w2 + (int64_t)o * kHid + h0)[v];
    }
    if (threadIdx.x < kHc) b1c[threadIdx.x] = a.b1[h0 + threadIdx.x];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kHc / 16; ++s) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* arow = &w1c[(16 * s + j16) * kLds + g];
#pragma unroll
      for (int k = 0; k < kIn / 4; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * k], rf[k], acc, 0, 0, 0);
      // acc[reg] = (W1 X^T)[hidden h0 + 16s + 4g + reg][row j16]
      float hv[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int hl = 16 * s + 4 * g + reg;
        hv[reg] = fmaxf(acc[reg] + b1c[hl], 0.f);
      }
      if (rok && a.hidden)
        *reinterpret_cast<float4*>(a.hidden + r * kHid + h0 + 16 * s + 4 * g) = make_float4(hv[0], hv[1], hv[2], hv[3]);
#pragma unroll
      for (int t = 0; t < kOut / 16; ++t) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          yt[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2c[(16 * t + j16) * kLds + 16 * s + 4 * g + reg], hv[reg], yt[t],
                                                       0, 0, 0);
      }
    }
  }
  // yt[t][reg] = (W2 H^T)[out 16t + 4g + reg][row j16]
  if (!rok) return;
#pragma unroll
  for (int t = 0; t < kOut / 16; ++t) {
    float y[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) y[reg] = tanhf(yt[t][reg] + a.b2[16 * t + 4 * g + reg]);
    *reinterpret_cast<float4*>(a.out + r * kOut + 16 * t + 4 * g) = make_float4(y[0], y[1], y[2], y[3]);
  }
}

// ---- tower backward ----------------------------------------------------------------------------------------------------
enum { EPI_STORE = 0, EPI_RELU = 1, EPI_MASK = 2 };

// C (M x N) = A (M x K) B (K x N) with element strides; blockIdx.z takes rows [z kchunk, (z + 1) kchunk) of K and writes
// its own slab C + z c_zstride.  64 x 64 tile per workgroup, 16 rows of it per wave, K staged 16 at a time.
struct GemmArgs {
  const float* A;
  int64_t sam, sak;
  const float* B;
  int64_t sbk, sbn;
  float* C;
  int64_t ldc, c_zstride;
  int64_t M, N, K, kchunk;
  const float* aux;      // EPI_RELU: C *= (aux[m ldc + n] > 0)
  const uint8_t* mask;   // EPI_MASK: rows m >= mask_row0: C *= mask[(m - mask_row0) N + n] ? mask_scale : 0
  int64_t mask_row0;
  float mask_scale;
};

template <int EPI>
__global__ __launch_bounds__(256) void tw_gemm(GemmArgs a) {
  __shared__ float as[64 * 17];   // as[m][k]
  __shared__ float bs[16 * 68];   // bs[k][n]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int64_t m0 = (int64_t)blockIdx.y * 64, n0 = (int64_t)blockIdx.x * 64;
  const int64_t kb = (int64_t)blockIdx.z * a.kchunk;
  const int64_t ke = std::min(kb + a.kchunk, a.K);
  const bool a_krow = a.sak == 1, b_nrow = a.sbn == 1;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t k0 = kb; k0 < ke; k0 += 16) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = threadIdx.x + 256 * u;
      int m, k;
      if (a_krow) { m = e / 16; k = e % 16; } else { m = e % 64; k = e / 64; }
      const int64_t gm = m0 + m, gk = k0 + k;
      as[m * 17 + k] = (gm < a.M && gk < ke) ? a.A[gm * a.sam + gk * a.sak] : 0.f;
      int n;
      if (b_nrow) { k = e / 64; n = e % 64; } else { n = e / 16; k = e % 16; }
      const int64_t gk2 = k0 + k, gn = n0 + n;
      bs[k * 68 + n] = (gk2 < ke && gn < a.N) ? a.B[gk2 * a.sbk + gn * a.sbn] : 0.f;
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
  float* C = a.C + (int64_t)blockIdx.z * a.c_zstride;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int64_t n = n0 + 16 * t + j16;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t m = m0 + 16 * wave + 4 * g + reg;
      if (m >= a.M || n >= a.N) continue;
      float v = acc[t][reg];
      if (EPI == EPI_RELU) v = a.aux[m * a.ldc + n] > 0.f ? v : 0.f;
      if (EPI == EPI_MASK && m >= a.mask_row0) v = v * (a.mask[(m - a.mask_row0) * a.N + n] ? a.mask_scale : 0.f);
      C[m * a.ldc + n] = v;
    }
  }
}

// dZ2 = dY (1 - Y^2) (torch's tanh_backward)
__global__ __launch_bounds__(256) void tw_tanh_bwd(const float* __restrict__ gy, const float* __restrict__ y, int64_t len,
                                                   float* __restrict__ dz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < len) dz[i] = gy[i] * (1.f - y[i] * y[i]);
}

// part[c][e] = sum over rows r of chunk c, ascending, of x[r][e]  (x: n x len)
__global__ __launch_bounds__(256) void tw_colsum_part(const float* __restrict__ x, int64_t n, int64_t len,
                                                      float* __restrict__ part) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = blockIdx.y;
  if (e >= len) return;
  const int64_t r1 = std::min((c + 1) * kRowChunk, n);
  float s = 0.f;
  for (int64_t r = c * kRowChunk; r < r1; ++r) s += x[r * len + e];
  part[c * len + e] = s;
}

// out[e] = sum over c, ascending, of part[c][e]
__global__ __launch_bounds__(256) void tw_reduce(const float* __restrict__ part, int64_t chunks, int64_t len,
                                                 float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  float s = 0.f;
  for (int64_t c = 0; c < chunks; ++c) s += part[c * len + e];
  out[e] = s;
}

// one wave per segment: table row seg_row[s] += sum of rows order[seg_start[s] .. seg_start[s + 1]) of x, in that order
__global__ __launch_bounds__(256) void seg_sum(const float* __restrict__ x, int32_t d, const int32_t* __restrict__ order,
                                               const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_row,
                                               int64_t n_seg, int64_t n_rows, int64_t n_table, float* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (s >= n_seg) return;
  const int64_t row = seg_row[s];
  if (row < 0 || row >= n_table) return;
  const int32_t p0 = seg_start[s], p1 = seg_start[s + 1];
  for (int col = lane; col < d; col += 64) {
    float acc = 0.f;
    for (int32_t p = p0; p < p1; ++p) {
      const int64_t r = order[p];
      if (r >= 0 && r < n_rows) acc += x[r * d + col];
    }
    out[row * d + col] += acc;
  }
}

template <int EPI>
srh_status_t gemm(const GemmArgs& a, int64_t zchunks, hipStream_t st) {
  const dim3 grid((unsigned)((a.N + 63) / 64), (unsigned)((a.M + 63) / 64), (unsigned)zchunks);
  tw_gemm<EPI><<<grid, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

struct BwdWs {
  float* dz2;     // n x 128
  float* dz1;     // n x 1024
  float* part_w;  // chunks x (1024 x 64 + 128 x 1024)  (dW1 partials, then dW2 partials)
  float* part_b;  // chunks x (1024 + 128)
};

inline int64_t bwd_ws_bytes(int64_t n) {
  const int64_t c = row_chunks(n);
  return align256(4 * n * kOut) + align256(4 * n * kHid) + align256(4 * c * (kHid * kIn + kOut * kHid)) +
         align256(4 * c * (kHid + kOut));
}

BwdWs bwd_carve(char* ws, int64_t n) {
  BwdWs w;
  char* cur = ws;
  auto take = [&](int64_t bytes) { char* r = cur; cur += align256(bytes); return r; };
  const int64_t c = row_chunks(n);
  w.dz2 = (float*)take(4 * n * kOut);
  w.dz1 = (float*)take(4 * n * kHid);
  w.part_w = (float*)take(4 * c * (kHid * kIn + kOut * kHid));
  w.part_b = (float*)take(4 * c * (kHid + kOut));
  return w;
}

// ---- batch softmax ---------------------------------------------------------------------------------------------------
constexpr int kBsRows = 64;           // R rows per workgroup (16 per wave)
constexpr int kBsCTile = 64;          // C rows staged in LDS per iteration
constexpr int kBsPass1Target = 512;   // pass-1 workgroups aimed for (row tiles x column chunks)

struct BsArgs {
  const float *u, *v;
  int64_t B;
  float inv_tau;
  double* loss;
  float *gu, *gv;
  float *un, *unorm, *vn, *vnorm;
  float* part_o;    // chunks x B x D
  double* part_rs;  // chunks x B
  float* cw;        // B  w_b / rowsum_b
  float* wv;        // B  w_b
  double* row_loss; // B
  int64_t chunks, chunk_len;
};

inline int64_t bs_chunks(int64_t B) {
  const int64_t rtiles = (B + kBsRows - 1) / kBsRows;
  const int64_t ctiles = (B + kBsCTile - 1) / kBsCTile;
  int64_t c = (kBsPass1Target + rtiles - 1) / rtiles;
  if (c > ctiles) c = ctiles;
  return c < 1 ? 1 : c;
}
inline int64_t bs_chunk_len(int64_t B) {
  const int64_t c = bs_chunks(B);
  const int64_t per = (B + c - 1) / c;
  return (per + kBsCTile - 1) / kBsCTile * kBsCTile;
}
inline int64_t bs_ws_bytes(int64_t B, int D) {
  const int64_t c = bs_chunks(B);
  return 2 * align256(4 * B * D) + 2 * align256(4 * B) + align256(4 * c * B * D) + align256(8 * c * B) +
         2 * align256(4 * B) + align256(8 * B);
}
void bs_carve(BsArgs& a, char* ws, int D) {
  char* cur = ws;
  auto take = [&](int64_t bytes) { char* r = cur; cur += align256(bytes); return r; };
  a.chunks = bs_chunks(a.B);
  a.chunk_len = bs_chunk_len(a.B);
  a.un = (float*)take(4 * a.B * D);
  a.vn = (float*)take(4 * a.B * D);
  a.unorm = (float*)take(4 * a.B);
  a.vnorm = (float*)take(4 * a.B);
  a.part_o = (float*)take(4 * a.chunks * a.B * D);
  a.part_rs = (double*)take(8 * a.chunks * a.B);
  a.cw = (float*)take(4 * a.B);
  a.wv = (float*)take(4 * a.B);
  a.row_loss = (double*)take(8 * a.B);
}

// F.normalize(x, dim=1): x / max(|x|, 1e-12); blockIdx.y: 0 users, 1 items
template <int D>
__global__ __launch_bounds__(256) void bs_prep(BsArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const bool item = blockIdx.y & 1;
  const float* src = item ? a.v : a.u;
  float* dst = item ? a.vn : a.un;
  float* nrm_out = item ? a.vnorm : a.unorm;
  const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  const bool ok = row < a.B;
  const float4 x = ok ? reinterpret_cast<const float4*>(src + row * D)[lane] : f4_zero();
  const float nrm = sqrtf(group_sum<LPR>(f4_dot(x, x)));
  const float den = fmaxf(nrm, kNormEps);
  if (ok) {
    reinterpret_cast<float4*>(dst + row * D)[lane] = make_float4(x.x / den, x.y / den, x.z / den, x.w / den);
    if (lane == 0) nrm_out[row] = nrm;
  }
}

// pass 1: R = users, C = a chunk of items, weight e = exp((s - 1) / tau)  -> per (chunk, user): sum e, sum e v_j
// pass 2: R = items, C = all users, weight e cw_b - [b == j] w_b        -> dL/dv_j (normalisation backward fused)
// (the rows are unit vectors: every logit is <= 1/tau and exp((s - 1)/tau) needs no running max)
template <int D, bool PASS2>
__global__ __launch_bounds__(256) void bs_pass(BsArgs a) {
  constexpr int LDS_STRIDE = D + 4;
  __shared__ float cs[kBsCTile * LDS_STRIDE];
  __shared__ float cwt[kBsCTile];
  __shared__ float cwd[kBsCTile];
  const float* Rn = PASS2 ? a.vn : a.un;
  const float* Cn = PASS2 ? a.un : a.vn;
  const int64_t rtile = PASS2 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x / a.chunks;
  const int64_t chunk = PASS2 ? 0 : (int64_t)blockIdx.x % a.chunks;
  int64_t cbeg = 0, cend = a.B;
  if (!PASS2) {
    cbeg = chunk * a.chunk_len;
    cend = std::min(cbeg + a.chunk_len, a.B);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int64_t r = rtile * kBsRows + wave * 16 + j16;
  const bool rok = r < a.B;
  const float inv_tau = a.inv_tau;
  float rf[D / 4];
#pragma unroll
  for (int s = 0; s < D / 4; ++s) rf[s] = rok ? Rn[r * D + 4 * s + g] : 0.f;
  f32x4 o[D / 16];
#pragma unroll
  for (int b = 0; b < D / 16; ++b) o[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  double rs = 0.0;

  for (int64_t c0 = cbeg; c0 < cend; c0 += kBsCTile) {
    __syncthreads();
    for (int e = threadIdx.x; e < kBsCTile * (D / 4); e += 256) {
      const int i = e / (D / 4), q = e % (D / 4);
      const int64_t c = c0 + i;
      *reinterpret_cast<float4*>(&cs[i * LDS_STRIDE + 4 * q]) =
          c < cend ? reinterpret_cast<const float4*>(Cn + c * D)[q] : f4_zero();
    }
    if (threadIdx.x < kBsCTile) {
      const int64_t c = c0 + threadIdx.x;
      const bool cok = c < cend;
      cwt[threadIdx.x] = cok ? (PASS2 ? a.cw[c] : 1.f) : 0.f;
      cwd[threadIdx.x] = (PASS2 && cok) ? a.wv[c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kBsCTile / 16; ++sub) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      const float* arow = &cs[(sub * 16 + j16) * LDS_STRIDE + g];
#pragma unroll
      for (int k = 0; k < D / 4; ++k) s = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * k], rf[k], s, 0, 0, 0);
      // s[reg] = S^T[c = c0 + sub*16 + 4g + reg][r]
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ci = sub * 16 + 4 * g + reg;
        float w = expf((s[reg] - 1.f) * inv_tau) * cwt[ci];
        if (PASS2) {
          if (c0 + ci == r) w -= cwd[ci];
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
    const int64_t row = chunk * a.B + r;
    if (g == 0) a.part_rs[row] = rs;
#pragma unroll
    for (int b = 0; b < D / 16; ++b)
      reinterpret_cast<float4*>(a.part_o + row * D + 16 * b + 4 * g)[0] = make_float4(o[b][0], o[b][1], o[b][2], o[b][3]);
  } else {
    const float k = inv_tau / (float)a.B;
    float4 tv[D / 16];
    float dot = 0.f;
#pragma unroll
    for (int b = 0; b < D / 16; ++b) {
      tv[b] = rok ? reinterpret_cast<const float4*>(a.vn + r * D + 16 * b + 4 * g)[0] : f4_zero();
      o[b] *= k;
      dot = fmaf(tv[b].x, o[b][0], fmaf(tv[b].y, o[b][1], fmaf(tv[b].z, o[b][2], fmaf(tv[b].w, o[b][3], dot))));
    }
    dot += __shfl_xor(dot, 16);
    dot += __shfl_xor(dot, 32);
    if (!rok) return;
    const float nrm = a.vnorm[r];
    const float inv = 1.f / fmaxf(nrm, kNormEps);
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
      reinterpret_cast<float4*>(a.gv + r * D + 16 * b + 4 * g)[0] = out;
    }
  }
}

// per user b: the chunk partials in chunk order -> row sum, p_b, loss term, w_b, dL/du_b
template <int D>
__global__ __launch_bounds__(256) void bs_finish(BsArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const int64_t b = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  if (b >= a.B) return;  // (whole row groups leave together)
  double rs = 0.0;
  float4 o = f4_zero();
  for (int64_t c = 0; c < a.chunks; ++c) {
    rs += a.part_rs[c * a.B + b];
    o = f4_add(o, reinterpret_cast<const float4*>(a.part_o + (c * a.B + b) * D)[lane]);
  }
  const float4 q = reinterpret_cast<const float4*>(a.un + b * D)[lane];
  const float4 t = reinterpret_cast<const float4*>(a.vn + b * D)[lane];
  const float spos = group_sum<LPR>(f4_dot(q, t));
  const double p = exp(((double)spos - 1.0) * (double)a.inv_tau) / rs;
  const double w = p / (p + kBsEps);
  const float inv_rs = (float)(1.0 / rs);
  if (lane == 0) {
    a.row_loss[b] = -log(p + kBsEps);
    a.cw[b] = (float)(w / rs);
    a.wv[b] = (float)w;
  }
  // dL/du_b = w_b / (B tau) (O_b / rowsum - v_b), then the normalisation backward
  const float k = (float)w * a.inv_tau / (float)a.B;
  float4 gq = make_float4(k * (o.x * inv_rs - t.x), k * (o.y * inv_rs - t.y), k * (o.z * inv_rs - t.z),
                          k * (o.w * inv_rs - t.w));
  const float dot = group_sum<LPR>(f4_dot(q, gq));
  const float nrm = a.unorm[b];
  const float inv = 1.f / fmaxf(nrm, kNormEps);
  if (nrm > kNormEps) gq = make_float4(gq.x - q.x * dot, gq.y - q.y * dot, gq.z - q.z * dot, gq.w - q.w * dot);
  reinterpret_cast<float4*>(a.gu + b * D)[lane] = f4_scale(gq, inv);
}

// the mean of the per-row terms, summed in a fixed order
__global__ __launch_bounds__(256) void bs_loss(BsArgs a) {
  __shared__ double part[256];
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < a.B; b += 256) s += a.row_loss[b];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.loss[0] = part[0] / (double)a.B;
}

template <int D>
srh_status_t launch_batch_softmax(BsArgs& a, hipStream_t st) {
  constexpr int RPB = 256 / (D / 4);
  const int64_t rtiles = (a.B + kBsRows - 1) / kBsRows;
  bs_prep<D><<<dim3((unsigned)((a.B + RPB - 1) / RPB), 2), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  bs_pass<D, false><<<(unsigned)(rtiles * a.chunks), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  bs_finish<D><<<(unsigned)((a.B + RPB - 1) / RPB), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  bs_pass<D, true><<<(unsigned)rtiles, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  bs_loss<<<1, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

srh_status_t check_weights(const srh_tower_weights_t* w) {
  SRH_REQUIRE(w && w->d_w1 && w->d_b1 && w->d_w2 && w->d_b2, "tower: null weight tensor");
  return SRH_OK;
}

}  // namespace

extern "C" {

srh_status_t srh_tower_fwd_f32(const float* d_table, const int32_t* d_idx, int64_t n, int64_t n_table,
                               const srh_tower_weights_t* w, int64_t mask_row0, const uint8_t* d_mask_in,
                               uint64_t rng_seed, uint64_t rng_counter, float drop_p, uint8_t* d_mask_out,
                               float* d_x_out, float* d_hidden, float* d_out, void* stream) {
  SRH_REQUIRE(d_table && d_out, "tower_fwd: null argument");
  SRH_REQUIRE(n > 0 && n < (int64_t(1) << 31) && n_table > 0, "tower_fwd: bad n / n_table");
  SRH_REQUIRE(d_idx || n <= n_table, "tower_fwd: without ids the table must hold n rows");
  SRH_REQUIRE(mask_row0 >= 0, "tower_fwd: bad mask_row0");
  SRH_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "tower_fwd: drop probability must be in [0, 1)");
  const srh_status_t ws = check_weights(w);
  if (ws != SRH_OK) return ws;
  FwdArgs a{};
  a.table = d_table; a.idx = d_idx; a.n = n; a.n_table = n_table; a.mask_row0 = mask_row0 < n ? mask_row0 : n;
  a.w1 = w->d_w1; a.b1 = w->d_b1; a.w2 = w->d_w2; a.b2 = w->d_b2;
  a.mask_in = d_mask_in; a.mask_out = d_mask_out;
  a.seed_lo = (uint32_t)rng_seed; a.seed_hi = (uint32_t)(rng_seed >> 32); a.ctr = rng_counter;
  a.drop_p = drop_p;
  a.drop_scale = 1.f / (1.f - drop_p);
  a.x_out = d_x_out; a.hidden = d_hidden; a.out = d_out;
  tw_fwd<<<(unsigned)((n + 63) / 64), 256, 0, as_stream(stream)>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_tower_bwd_ws_bytes(int64_t n) {
  if (n <= 0) return 0;
  return bwd_ws_bytes(n);
}

srh_status_t srh_tower_bwd_f32(const float* d_x, const float* d_hidden, const float* d_y, const float* d_gy, int64_t n,
                               const srh_tower_weights_t* w, int64_t mask_row0, const uint8_t* d_mask, float drop_p,
                               float* d_gx, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* d_ws,
                               void* stream) {
  SRH_REQUIRE(d_x && d_hidden && d_y && d_gy && d_gx && d_gw1 && d_gb1 && d_gw2 && d_gb2 && d_ws,
              "tower_bwd: null argument");
  SRH_REQUIRE(n > 0 && n < (int64_t(1) << 31), "tower_bwd: bad n");
  SRH_REQUIRE(mask_row0 >= 0, "tower_bwd: bad mask_row0");
  SRH_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "tower_bwd: drop probability must be in [0, 1)");
  const srh_status_t wst = check_weights(w);
  if (wst != SRH_OK) return wst;
  hipStream_t st = as_stream(stream);
  BwdWs ws = bwd_carve(static_cast<char*>(d_ws), n);
  const int64_t chunks = row_chunks(n);
  srh_status_t s;
  // dZ2
  tw_tanh_bwd<<<(unsigned)((n * kOut + 255) / 256), 256, 0, st>>>(d_gy, d_y, n * kOut, ws.dz2);
  SRH_LAUNCH_CHECK();
  // dZ1 = (dZ2 W2) [H > 0]         (n x 128) (128 x 1024)
  GemmArgs g{};
  g.A = ws.dz2; g.sam = kOut; g.sak = 1; g.B = w->d_w2; g.sbk = kHid; g.sbn = 1; g.C = ws.dz1; g.ldc = kHid; g.M = n; g.N = kHid; g.K = kOut; g.kchunk = kOut;
  g.aux = d_hidden;
  if ((s = gemm<EPI_RELU>(g, 1, st)) != SRH_OK) return s;
  // dX = (dZ1 W1) m                (n x 1024) (1024 x 64)
  g = GemmArgs{};
  g.A = ws.dz1; g.sam = kHid; g.sak = 1; g.B = w->d_w1; g.sbk = kIn; g.sbn = 1; g.C = d_gx; g.ldc = kIn;
  g.M = n; g.N = kIn; g.K = kHid; g.kchunk = kHid;
  g.mask = d_mask; g.mask_row0 = d_mask ? mask_row0 : n; g.mask_scale = 1.f / (1.f - drop_p);
  if ((s = d_mask ? gemm<EPI_MASK>(g, 1, st) : gemm<EPI_STORE>(g, 1, st)) != SRH_OK) return s;
  // dW1 partials = dZ1^T X per chunk of rows     (1024 x n) (n x 64)
  float* part_w1 = ws.part_w;
  float* part_w2 = ws.part_w + chunks * kHid * kIn;
  g = GemmArgs{};
  g.A = ws.dz1; g.sam = 1; g.sak = kHid; g.B = d_x; g.sbk = kIn; g.sbn = 1; g.C = part_w1; g.ldc = kIn;
  g.c_zstride = kHid * kIn; g.M = kHid; g.N = kIn; g.K = n; g.kchunk = kRowChunk;
  if ((s = gemm<EPI_STORE>(g, chunks, st)) != SRH_OK) return s;
  // dW2 partials = dZ2^T H per chunk of rows     (128 x n) (n x 1024)
  g = GemmArgs{};
  g.A = ws.dz2; g.sam = 1; g.sak = kOut; g.B = d_hidden; g.sbk = kHid; g.sbn = 1; g.C = part_w2; g.ldc = kHid;
  g.c_zstride = kOut * kHid; g.M = kOut; g.N = kHid; g.K = n; g.kchunk = kRowChunk;
  if ((s = gemm<EPI_STORE>(g, chunks, st)) != SRH_OK) return s;
  // bias partials
  float* part_b1 = ws.part_b;
  float* part_b2 = ws.part_b + chunks * kHid;
  tw_colsum_part<<<dim3(kHid / 256, (unsigned)chunks), 256, 0, st>>>(ws.dz1, n, kHid, part_b1);
  SRH_LAUNCH_CHECK();
  tw_colsum_part<<<dim3(1, (unsigned)chunks), 256, 0, st>>>(ws.dz2, n, kOut, part_b2);
  SRH_LAUNCH_CHECK();
  // the partials in chunk order
  tw_reduce<<<(unsigned)((kHid * kIn + 255) / 256), 256, 0, st>>>(part_w1, chunks, kHid * kIn, d_gw1);
  SRH_LAUNCH_CHECK();
  tw_reduce<<<(unsigned)((kOut * kHid + 255) / 256), 256, 0, st>>>(part_w2, chunks, kOut * kHid, d_gw2);
  SRH_LAUNCH_CHECK();
  tw_reduce<<<(unsigned)(kHid / 256), 256, 0, st>>>(part_b1, chunks, kHid, d_gb1);
  SRH_LAUNCH_CHECK();
  tw_reduce<<<1, 256, 0, st>>>(part_b2, chunks, kOut, d_gb2);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

srh_status_t srh_rows_segment_sum_f32(const float* d_x, int64_t n_rows, int32_t d, const int32_t* d_order,
                                      const int32_t* d_seg_start, const int32_t* d_seg_row, int64_t n_seg,
                                      int64_t n_table, float* d_out, void* stream) {
  SRH_REQUIRE(d_x && d_order && d_seg_start && d_seg_row && d_out, "rows_segment_sum: null argument");
  SRH_REQUIRE(n_rows > 0 && n_rows < (int64_t(1) << 31) && d > 0 && n_seg >= 0 && n_seg <= n_rows && n_table > 0,
              "rows_segment_sum: bad sizes");
  if (n_seg == 0) return SRH_OK;
  seg_sum<<<(unsigned)((n_seg + 3) / 4), 256, 0, as_stream(stream)>>>(d_x, d, d_order, d_seg_start, d_seg_row, n_seg,
                                                                      n_rows, n_table, d_out);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_batch_softmax_ws_bytes(int64_t B, int32_t d) {
  if (B <= 0 || (d != 64 && d != 128)) return 0;
  return bs_ws_bytes(B, d);
}

srh_status_t srh_batch_softmax_fwd_bwd(const float* d_u, const float* d_v, int64_t B, int32_t d, float tau,
                                       double* d_loss, float* d_gu, float* d_gv, void* d_ws, void* stream) {
  SRH_REQUIRE(d_u && d_v && d_loss && d_gu && d_gv && d_ws, "batch_softmax: null argument");
  SRH_REQUIRE(B > 0 && B < (int64_t(1) << 31), "batch_softmax: bad B");
  SRH_REQUIRE(d == 64 || d == 128, "batch_softmax: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(tau > 0.f && std::isfinite(tau), "batch_softmax: temperature must be positive");
  BsArgs a{};
  a.u = d_u; a.v = d_v; a.B = B; a.inv_tau = 1.f / tau; a.loss = d_loss; a.gu = d_gu; a.gv = d_gv;
  bs_carve(a, static_cast<char*>(d_ws), d);
  hipStream_t st = as_stream(stream);
  return d == 64 ? launch_batch_softmax<64>(a, st) : launch_batch_softmax<128>(a, st);
}

}  // extern "C"

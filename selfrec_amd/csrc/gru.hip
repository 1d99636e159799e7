// GRU4Rec's recurrence (header (a-26)): the hidden-side half of a GRU layer, forward and backward, one
// launch each.  The input-side product GI = X W_ih^T + b_ih and the four weight-gradient products are the caller's GEMMs.
//   forward, per sequence b, t < len_b, h_{-1} = 0:
//     gh = W_hh h_{t-1} + b_hh;  r = sig(gi_r + gh_r);  z = sig(gi_z + gh_z);  n = tanh(gi_n + r gh_n)
//     h_t = (1 - z) n + z h_{t-1};  out[b,t] = h_t;  gates[b,t] = [r, z, n, gh_n]
//   backward, carry = 0, t = len_b - 1 .. 0:
//     dh = carry + go[b,t];  dn = dh (1 - z)(1 - n^2);  dz = dh (h_{t-1} - n) z (1 - z);  dr = dn gh_n r (1 - r)
//     dgi[b,t] = [dr, dz, dn];  dghn[b,t] = dn r;  carry = dh z + [dr, dz, dn r] W_hh
//   every row of out / gates / dgi / dghn at t >= len_b is written as exact zeros; go there is never read.
// One workgroup of four waves owns a tile of 16 sequences for all its steps.  Lane (g, j16) of wave w owns hidden unit
// u = 16 w + j16 of the four sequences 4 g + reg: it forms r, z and n of that unit itself (the wave takes the column tiles
// w, 4 + w, 8 + w of the 12 of W_hh), so the gate arithmetic crosses no lane, and the backward pass hands out its work the
// same way.  Both products run on v_mfma_f32_16x16x4_f32 with the sequences as the A operand from LDS (the h tile 16 x 64,
// the [dr, dz, dn r] tile 16 x 192; two buffers each, so a step has ONE barrier) and the wave's share of W_hh resident in
// 48 B-operand registers per lane, loaded once.  Lane g takes the contiguous k range [K/4 g, K/4 (g + 1)) of the product
// (16-byte LDS reads): a fixed summation order, no float atomics, the same bits on every call.  A tile runs to the longest
// length among its rows; a row past its own length neither updates nor stores.  H = 64.
#include <cmath>

#include "../../include/selfrec_hip.h"
#include "rowtile.h"

namespace {
using namespace srh;

constexpr int kH = 64;                  // hidden width
constexpr int kSeqTile = 16;            // sequences per workgroup
constexpr int kHStride = kH + 4;        // floats between two sequences of the h tile
constexpr int kGStride = 3 * kH + 4;    // ... of the [dr, dz, dn r] tile
constexpr int kMaxLen = 512;

struct GruArgs {
  const float* gi;       // B x L x 3H
  const float* w_hh;     // 3H x H
  const float* b_hh;     // 3H
  const int32_t* len;    // B
  int64_t B;
  int32_t L;
  float* out;            // B x L x H
  float* gates;          // B x L x 4H, or null
};

struct GruBwdArgs {
  const float* go;       // B x L x H
  const float* out;      // B x L x H
  const float* gates;    // B x L x 4H
  const float* w_hh;     // 3H x H
  const int32_t* len;
  int64_t B;
  int32_t L;
  float* dgi;            // B x L x 3H
  float* dghn;           // B x L x H
};

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// the tile's lengths (clamped to [0, L]; 0 for a sequence past B) into LDS -> the longest of them
__device__ __forceinline__ int tile_lengths(int* lens, const int32_t* __restrict__ len, int64_t b0, int64_t B, int L) {
  if (threadIdx.x < kSeqTile) {
    const int64_t b = b0 + threadIdx.x;
    lens[threadIdx.x] = b < B ? min(max((int)len[b], 0), L) : 0;
  }
  __syncthreads();
  int tmax = 0;
#pragma unroll
  for (int i = 0; i < kSeqTile; ++i) tmax = max(tmax, lens[i]);
  return tmax;
}

// rows [len_s, L) of every sequence of the tile, `width` floats each, as zeros: one contiguous block per sequence
__device__ __forceinline__ void zero_tails(float* __restrict__ dst, int width, const int* lens, int64_t b0, int64_t B, int L) {
  for (int s = 0; s < kSeqTile; ++s) {
    const int64_t b = b0 + s;
    if (b >= B) break;
    float4* p = reinterpret_cast<float4*>(dst + (b * L + lens[s]) * (int64_t)width);
    const int n4 = (L - lens[s]) * (width / 4);
    for (int e = threadIdx.x; e < n4; e += 256) p[e] = f4_zero();
  }
}

__global__ __launch_bounds__(256) void gru_fwd(GruArgs P) {
  __shared__ __attribute__((aligned(16))) float hs[2][kSeqTile * kHStride];
  __shared__ int lens[kSeqTile];
  const RtLane T = rt_lane();
  const int g = T.g, j16 = T.j16;
  const int u = 16 * T.wave + j16;
  const int64_t b0 = (int64_t)blockIdx.x * kSeqTile;
  const int L = P.L;
  for (int e = threadIdx.x; e < 2 * kSeqTile * kHStride; e += 256) (&hs[0][0])[e] = 0.f;
  const int tmax = tile_lengths(lens, P.len, b0, P.B, L);   // (its barrier covers the zeroed tiles too)

  // B operand: wreg[gate][k] = W_hh[gate H + u][16 g + k]; the lane's k range is [16 g, 16 g + 16)
  float wreg[3][16], bias[3];
#pragma unroll
  for (int gate = 0; gate < 3; ++gate) {
    bias[gate] = P.b_hh[gate * kH + u];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 w4 = reinterpret_cast<const float4*>(P.w_hh + (int64_t)(gate * kH + u) * kH + 16 * g)[q];
      wreg[gate][4 * q] = w4.x; wreg[gate][4 * q + 1] = w4.y; wreg[gate][4 * q + 2] = w4.z; wreg[gate][4 * q + 3] = w4.w;
    }
  }
  int mylen[4];
  int64_t row0[4];                       // b L of the lane's four sequences
  float hprev[4], gin[3][4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    mylen[reg] = lens[4 * g + reg];
    row0[reg] = (b0 + 4 * g + reg) * L;
    hprev[reg] = 0.f;
#pragma unroll
    for (int gate = 0; gate < 3; ++gate)
      gin[gate][reg] = 0 < mylen[reg] ? P.gi[row0[reg] * (3 * kH) + gate * kH + u] : 0.f;
  }

  for (int t = 0; t < tmax; ++t) {
    const float* hcur = hs[t & 1];
    float* hnext = hs[(t + 1) & 1];
    float gic[3][4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
#pragma unroll
      for (int gate = 0; gate < 3; ++gate) {
        gic[gate][reg] = gin[gate][reg];
        // the next step's inputs travel while this step's product runs
        gin[gate][reg] = t + 1 < mylen[reg] ? P.gi[(row0[reg] + t + 1) * (3 * kH) + gate * kH + u] : 0.f;
      }
    f32x4 acc[3];
    zero_acc(acc);
    const float4* arow = reinterpret_cast<const float4*>(&hcur[j16 * kHStride + 16 * g]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 a4 = arow[q];
      const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int gate = 0; gate < 3; ++gate)
          acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wreg[gate][4 * q + e], acc[gate], 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      if (t < mylen[reg]) {
        const float ghn = acc[2][reg] + bias[2];
        const float r = gru_sigmoid(gic[0][reg] + (acc[0][reg] + bias[0]));
        const float z = gru_sigmoid(gic[1][reg] + (acc[1][reg] + bias[1]));
        const float n = tanhf(gic[2][reg] + r * ghn);
        const float h = (1.f - z) * n + z * hprev[reg];
        hprev[reg] = h;
        const int64_t row = row0[reg] + t;
        P.out[row * kH + u] = h;
        if (P.gates) {
          float* gp = P.gates + row * (4 * kH) + u;
          gp[0] = r; gp[kH] = z; gp[2 * kH] = n; gp[3 * kH] = ghn;
        }
      }
      hnext[(4 * g + reg) * kHStride + u] = hprev[reg];
    }
    __syncthreads();
  }
  zero_tails(P.out, kH, lens, b0, P.B, L);
  if (P.gates) zero_tails(P.gates, 4 * kH, lens, b0, P.B, L);
}

__global__ __launch_bounds__(256) void gru_bwd(GruBwdArgs P) {
  __shared__ __attribute__((aligned(16))) float ds[2][kSeqTile * kGStride];
  __shared__ int lens[kSeqTile];
  const RtLane T = rt_lane();
  const int g = T.g, j16 = T.j16;
  const int u = 16 * T.wave + j16;
  const int64_t b0 = (int64_t)blockIdx.x * kSeqTile;
  const int L = P.L;
  const int tmax = tile_lengths(lens, P.len, b0, P.B, L);

  // B operand: wreg[k] = W_hh[48 g + k][u]; the lane's k range of the 192 is [48 g, 48 g + 48)
  float wreg[48];
#pragma unroll
  for (int k = 0; k < 48; ++k) wreg[k] = P.w_hh[(int64_t)(48 * g + k) * kH + u];
  int mylen[4];
  int64_t row0[4];
  float carry[4];
  // what step t reads from memory, fetched one step ahead: go, r, z, n, gh_n, h_{t-1}
  float nx[6][4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    mylen[reg] = lens[4 * g + reg];
    row0[reg] = (b0 + 4 * g + reg) * L;
    carry[reg] = 0.f;
#pragma unroll
    for (int f = 0; f < 6; ++f) nx[f][reg] = 0.f;
  }
  auto fetch = [&](int t) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      if (t >= 0 && t < mylen[reg]) {
        const int64_t row = row0[reg] + t;
        nx[0][reg] = P.go[row * kH + u];
        const float* gp = P.gates + row * (4 * kH) + u;
        nx[1][reg] = gp[0]; nx[2][reg] = gp[kH]; nx[3][reg] = gp[2 * kH]; nx[4][reg] = gp[3 * kH];
        nx[5][reg] = t > 0 ? P.out[(row - 1) * kH + u] : 0.f;
      }
    }
  };
  fetch(tmax - 1);

  for (int t = tmax - 1; t >= 0; --t) {
    float* dcur = ds[t & 1];
    float dhz[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float dr = 0.f, dz = 0.f, dnr = 0.f;
      dhz[reg] = 0.f;
      if (t < mylen[reg]) {
        const float dh = carry[reg] + nx[0][reg];
        const float r = nx[1][reg], z = nx[2][reg], n = nx[3][reg], ghn = nx[4][reg], hp = nx[5][reg];
        const float dn = dh * (1.f - z) * (1.f - n * n);
        dz = dh * (hp - n) * z * (1.f - z);
        dr = dn * ghn * r * (1.f - r);
        dnr = dn * r;
        dhz[reg] = dh * z;
        const int64_t row = row0[reg] + t;
        float* gp = P.dgi + row * (3 * kH) + u;
        gp[0] = dr; gp[kH] = dz; gp[2 * kH] = dn;
        P.dghn[row * kH + u] = dnr;
      }
      float* dp = &dcur[(4 * g + reg) * kGStride + u];
      dp[0] = dr; dp[kH] = dz; dp[2 * kH] = dnr;
    }
    __syncthreads();
    fetch(t - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float4* arow = reinterpret_cast<const float4*>(&dcur[j16 * kGStride + 48 * g]);
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      const float4 a4 = arow[q];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, wreg[4 * q], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, wreg[4 * q + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, wreg[4 * q + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, wreg[4 * q + 3], acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) carry[reg] = t < mylen[reg] ? dhz[reg] + acc[reg] : 0.f;
  }
  zero_tails(P.dgi, 3 * kH, lens, b0, P.B, L);
  zero_tails(P.dghn, kH, lens, b0, P.B, L);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

srh_status_t gru_shape(const char* who, int64_t B, int32_t L, int32_t H) {
  SRH_SUPPORTED(H == kH, "%s: H=%d unsupported (64; a narrower layer is zero-padded by the caller)", who, H);
  SRH_SUPPORTED(L >= 1 && L <= kMaxLen, "%s: L=%d unsupported (1..%d)", who, L, kMaxLen);
  SRH_REQUIRE(B >= 1 && B < (int64_t(1) << 31), "%s: bad B", who);
  return SRH_OK;
}

}  // namespace

extern "C" {

srh_status_t srh_gru_fwd_f32(const float* d_gi, const float* d_w_hh, const float* d_b_hh, const int32_t* d_len, int64_t B,
                             int32_t L, int32_t H, float* d_out, float* d_gates, void* stream) {
  if (srh_status_t s = gru_shape("gru_fwd_f32", B, L, H)) return s;
  SRH_REQUIRE(d_gi && d_w_hh && d_b_hh && d_len && d_out, "gru_fwd_f32: null argument");
  SRH_REQUIRE(aligned16(d_gi) && aligned16(d_w_hh) && aligned16(d_out) && aligned16(d_gates),
              "gru_fwd_f32: the float tensors must be 16-byte aligned");
  GruArgs a{d_gi, d_w_hh, d_b_hh, d_len, B, L, d_out, d_gates};
  gru_fwd<<<(unsigned)ceil_div(B, kSeqTile), 256, 0, srh::as_stream(stream)>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

srh_status_t srh_gru_bwd_f32(const float* d_go, const float* d_out, const float* d_gates, const float* d_w_hh,
                             const int32_t* d_len, int64_t B, int32_t L, int32_t H, float* d_dgi, float* d_dghn,
                             void* stream) {
  if (srh_status_t s = gru_shape("gru_bwd_f32", B, L, H)) return s;
  SRH_REQUIRE(d_go && d_out && d_gates && d_w_hh && d_len && d_dgi && d_dghn, "gru_bwd_f32: null argument");
  SRH_REQUIRE(aligned16(d_dgi) && aligned16(d_dghn), "gru_bwd_f32: the output tensors must be 16-byte aligned");
  GruBwdArgs a{d_go, d_out, d_gates, d_w_hh, d_len, B, L, d_dgi, d_dghn};
  gru_bwd<<<(unsigned)ceil_div(B, kSeqTile), 256, 0, srh::as_stream(stream)>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // extern "C"

// The MFMA row-tile idiom of the model kernels (contrastive.hip, sept.hip, ncl.hip), one definition of each piece.
// DESIGN.md 4.24.
//
// A 256-thread workgroup owns kRtRows = 64 "R" rows, 16 per wave, and keeps them in registers; "C" rows stream through
// LDS 64 at a time, at a row stride of D + 4 floats (rows 4 floats apart in bank space: both read patterns below are
// conflict-free).  Lane (g = lane >> 4, j16 = lane & 15) of wave w holds R row 64 tile + 16 w + j16.
//   score16   S^T[c][r] = C_c . R_r      v_mfma_f32_16x16x4_f32 with A = the C tile from LDS (row 16 sub + j16, column
//                                        4 k + g at k-step k), B = the R row from registers (rf[k] = R[r][4 k + g]);
//                                        k ascending, so a score depends on its two rows only.
//                                        s[reg] = S^T[c = 16 sub + 4 g + reg][r]
//   (caller)  W[c][r] = weight(S^T[c][r])  on the accumulator, in place
//   accum16   O^T[:, r] += sum_c C_c W[c][r]   the accumulator of the first product is the B operand of the second with no
//                                        lane movement: its c order inside a k-step is 4 g + reg, matched by A (row
//                                        16 sub + 4 g + reg, column 16 b + j16).  o[b][reg] = O[r][16 b + 4 g + reg]
// The four lanes g = 0..3 of one j16 share an R row: sum4 adds their partials (the same bits in all four).
#pragma once
#include "common.h"

namespace srh {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRtRows = 64;   // R rows per workgroup = C rows per LDS tile
template <int D>
constexpr int kRtStride = D + 4;   // floats between two rows of the LDS tile

struct RtLane {
  int wave, lane, g, j16;   // the lane's R row within the tile is 16 wave + j16
};
__device__ __forceinline__ RtLane rt_lane() {
  const int lane = threadIdx.x & 63;
  return RtLane{(int)(threadIdx.x >> 6), lane, lane >> 4, lane & 15};
}

// B operand of score16: rf[s] = Rn[r][4 s + g] (zeros for a row past the end)
template <int D>
__device__ __forceinline__ void load_rf(float (&rf)[D / 4], const float* __restrict__ Rn, int64_t r, bool rok, int g) {
#pragma unroll
  for (int s = 0; s < D / 4; ++s) rf[s] = rok ? Rn[r * D + 4 * s + g] : 0.f;
}

// C rows [c0, c0 + 64) of src (rows >= cend: zeros) into the LDS tile; the caller's barriers surround it
template <int D>
__device__ __forceinline__ void stage_tile(float* cs, const float* __restrict__ src, int64_t c0, int64_t cend) {
  constexpr int LDS_STRIDE = kRtStride<D>;
  for (int e = threadIdx.x; e < kRtRows * (D / 4); e += 256) {
    const int i = e / (D / 4), q = e % (D / 4);
    const int64_t c = c0 + i;
    const float4 x = c < cend ? reinterpret_cast<const float4*>(src + c * D)[q] : f4_zero();
    *reinterpret_cast<float4*>(&cs[i * LDS_STRIDE + 4 * q]) = x;
  }
}

template <int D>
__device__ __forceinline__ f32x4 score16(const float* cs, int sub, int j16, int g, const float (&rf)[D / 4]) {
  constexpr int LDS_STRIDE = kRtStride<D>;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  const float* arow = &cs[(sub * 16 + j16) * LDS_STRIDE + g];
#pragma unroll
  for (int k = 0; k < D / 4; ++k) s = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * k], rf[k], s, 0, 0, 0);
  return s;
}

template <int D>
__device__ __forceinline__ void accum16(f32x4 (&o)[D / 16], const float* cs, int sub, int j16, int g, const f32x4 s) {
  constexpr int LDS_STRIDE = kRtStride<D>;
#pragma unroll
  for (int b = 0; b < D / 16; ++b) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      o[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(cs[(sub * 16 + 4 * g + reg) * LDS_STRIDE + 16 * b + j16], s[reg], o[b],
                                                  0, 0, 0);
  }
}

template <int NB>
__device__ __forceinline__ void zero_acc(f32x4 (&o)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b) o[b] = f32x4{0.f, 0.f, 0.f, 0.f};
}

template <typename T>
__device__ __forceinline__ T sum4(T v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// o[b][reg] = O[r][16 b + 4 g + reg] as 16-byte stores of row r of dst
template <int D>
__device__ __forceinline__ void store_acc(const f32x4 (&o)[D / 16], float* __restrict__ dst, int64_t r, int g) {
#pragma unroll
  for (int b = 0; b < D / 16; ++b)
    reinterpret_cast<float4*>(dst + r * D + 16 * b + 4 * g)[0] = make_float4(o[b][0], o[b][1], o[b][2], o[b][3]);
}

// The normalisation backward of a row held as o[b][reg] = G[r][16 b + 4 g + reg], y = yn[r] the normalised row:
// (G - y (y.G)) inv, or G inv where the forward clamped the norm.  (inv, clamped) are the caller's: F.normalize clamps
// the norm, tf.nn.l2_normalize the squared norm.  Every lane of the wave calls it (the dot crosses lanes).
template <int D>
__device__ __forceinline__ void norm_bwd_store(const f32x4 (&o)[D / 16], const float* __restrict__ yn, float inv,
                                               bool clamped, int64_t r, bool rok, int g, float* __restrict__ dst) {
  float4 y[D / 16];
  float dot = 0.f;
#pragma unroll
  for (int b = 0; b < D / 16; ++b) {
    y[b] = rok ? reinterpret_cast<const float4*>(yn + r * D + 16 * b + 4 * g)[0] : f4_zero();
    dot = fmaf(y[b].x, o[b][0], fmaf(y[b].y, o[b][1], fmaf(y[b].z, o[b][2], fmaf(y[b].w, o[b][3], dot))));
  }
  dot = sum4(dot);
  if (!rok) return;
#pragma unroll
  for (int b = 0; b < D / 16; ++b) {
    float4 out;
    if (clamped) {
      out = make_float4(o[b][0] * inv, o[b][1] * inv, o[b][2] * inv, o[b][3] * inv);
    } else {
      out = make_float4((o[b][0] - y[b].x * dot) * inv, (o[b][1] - y[b].y * dot) * inv, (o[b][2] - y[b].z * dot) * inv,
                        (o[b][3] - y[b].w * dot) * inv);
    }
    reinterpret_cast<float4*>(dst + r * D + 16 * b + 4 * g)[0] = out;
  }
}

// x[0 .. n) summed in a fixed order by a 256-thread workgroup: thread i takes i, i + 256, ... ascending, then the tree
// 128 .. 1.  Every thread gets the sum.
__device__ __forceinline__ double block_sum_d(const double* __restrict__ x, int64_t n) {
  __shared__ double part[256];
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < n; b += 256) s += x[b];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  return part[0];
}

}  // namespace srh

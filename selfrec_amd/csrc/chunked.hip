// The chunk-ordered reductions over rows that the tower backward (ssl4rec.hip) and MHCN's gate, mix and MIM (mhcn.hip)
// share: column sums per chunk of rows and the sum of the chunk partials in chunk order; and the tower backward's strided
// f32 MFMA GEMM, whose K dimension (the rows) can be cut into chunks that each write a slab of their own.  No float
// atomics: every element is one thread's ascending sum, so a call returns the same bits every time, whatever the block
// size.  DESIGN.md 4.24.
#include <algorithm>

#include "rowtile.h"

namespace srh {
namespace {

// (any block size up to 256: thread e of the grid owns column e)
__global__ __launch_bounds__(256) void colsum_part(const float* __restrict__ x, int64_t n, int64_t len, int mats, int chunk,
                                                   float* __restrict__ part) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t z = blockIdx.y / mats;
  const int m = blockIdx.y % mats;
  if (e >= len) return;
  const float* xm = x + (int64_t)m * n * len;
  const int64_t r1 = std::min<int64_t>((z + 1) * chunk, n);
  float s = 0.f;
  for (int64_t r = z * chunk; r < r1; ++r) s += xm[r * len + e];
  part[(int64_t)blockIdx.y * len + e] = s;
}

__global__ __launch_bounds__(256) void reduce_part(const float* __restrict__ part, int64_t chunks, int64_t len, float scale,
                                                   float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  float s = 0.f;
  for (int64_t z = 0; z < chunks; ++z) s += part[z * len + e];
  out[e] = s * scale;
}

// 64 x 64 tile of C per workgroup, 16 rows of it per wave, K staged 16 at a time: as[m][k] is the A operand, bs[k][n] the
// B operand, k ascending in steps of 4
template <int EPI>
__global__ __launch_bounds__(256) void gemm64_kernel(GemmArgs a) {
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

}  // namespace

srh_status_t colsum_chunks(const float* x, int64_t n, int64_t len, int mats, int chunk, float* part, hipStream_t st) {
  const int block = len >= 256 ? 256 : 64;   // a wave per 64 columns; the tower's 1024 hidden units in blocks of 256
  const dim3 grid((unsigned)ceil_div(len, block), (unsigned)(ceil_div(n, chunk) * mats));
  colsum_part<<<grid, block, 0, st>>>(x, n, len, mats, chunk, part);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

srh_status_t reduce_chunks(const float* part, int64_t chunks, int64_t len, float scale, float* out, hipStream_t st) {
  reduce_part<<<(unsigned)ceil_div(len, 256), 256, 0, st>>>(part, chunks, len, scale, out);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

srh_status_t gemm64(const GemmArgs& a, GemmEpi epi, int64_t chunks, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.N, 64), (unsigned)ceil_div(a.M, 64), (unsigned)chunks);
  if (epi == EPI_RELU) gemm64_kernel<EPI_RELU><<<grid, 256, 0, st>>>(a);
  else if (epi == EPI_MASK) gemm64_kernel<EPI_MASK><<<grid, 256, 0, st>>>(a);
  else gemm64_kernel<EPI_STORE><<<grid, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // namespace srh

// The two row losses of util/loss_torch.py that need no product of row sets: triplet_loss (:12-16) and kl_divergence
// (:91-94).  DESIGN.md 4.27.  Each is one row launch that writes every gradient at unit upstream gradient and the row's
// loss term (a double) into the workspace, and one single-workgroup launch that sums the terms in block_sum_d's fixed
// order and takes the mean.  No float atomics: one producer per output element, the same bits on every call.
//
// triplet  x_b = |u_b - p_b|^2 - |u_b - n_b|^2 + margin,  loss = mean_b max(x_b, 0)
//          rows with x_b > 0: gu = 2 (n - p) / B, gp = -2 (u - p) / B, gn = 2 (u - n) / B;  x_b <= 0: exact zeros (relu's
//          subgradient at 0 is 0, as torch's).  LPR lanes per row, one float4 each, as the BPR kernels; the two squared
//          distances are summed in double, so the sign of x_b is that of the float64 evaluation unless |x_b| is of the
//          order of 1e-13 of the distances.
// kl       per row of R x C logits a (p side) and b (q side): p = softmax(a), q = softmax(b),
//          kl_r = sum_c p_c (lp_c - lq_c),  loss = mean_r kl_r
//          d/db_rc = (q_rc - p_rc) / R,   d/da_rc = p_rc ((lp_rc - lq_rc) - kl_r) / R
//          One wave per row, lane l owns columns l, l + 64, ...: any C >= 1, nothing padded (a padded logit is not neutral).
//          Three sweeps of the row -- the two maxima; the two exp-sums and sum_c e^a_c d_c with d_c = (a_c - max a) - (b_c -
//          max b); the gradients -- with kl_r = (sum_c e^a_c d_c) / (sum e^a) - log sum e^a + log sum e^b.  Both softmaxes
//          are max-subtracted; a column with p_c = 0 adds 0 d_c = 0, never NaN (d_c is finite for finite logits).  The
//          sums are double.
#include <cmath>

#include "rowtile.h"

namespace {

using namespace srh;

template <int LPR>
__device__ __forceinline__ double group_sum_d(double v) {
#pragma unroll
  for (int w = 1; w < LPR; w <<= 1) v += __shfl_xor(v, w);
  return v;
}

__device__ __forceinline__ double f4_sqdist_d(const float4 a, const float4 b) {
  const double x = (double)a.x - (double)b.x, y = (double)a.y - (double)b.y, z = (double)a.z - (double)b.z,
               w = (double)a.w - (double)b.w;
  return (x * x + y * y) + (z * z + w * w);
}

__device__ __forceinline__ float4 f4_diff_scaled(const float4 a, const float4 b, const double k) {
  return make_float4((float)(((double)a.x - (double)b.x) * k), (float)(((double)a.y - (double)b.y) * k),
                     (float)(((double)a.z - (double)b.z) * k), (float)(((double)a.w - (double)b.w) * k));
}

template <int LPR>
__global__ __launch_bounds__(256) void triplet_rows(const float4* __restrict__ U, const float4* __restrict__ P,
                                                    const float4* __restrict__ Nn, int B, float margin,
                                                    double* __restrict__ row_loss, float4* __restrict__ GU,
                                                    float4* __restrict__ GP, float4* __restrict__ GN) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63, g = lane / LPR, sub = lane % LPR;
  const int b = (int)((blockIdx.x * 256u + threadIdx.x) >> 6) * G + g;
  const bool valid = b < B;
  const size_t at = (size_t)(valid ? b : 0) * LPR + sub;
  const float4 u = U[at], p = P[at], n = Nn[at];
  // (every lane of the wave takes part in the shuffles; rows past B repeat row 0 and store nothing)
  const double x = group_sum_d<LPR>(f4_sqdist_d(u, p)) - group_sum_d<LPR>(f4_sqdist_d(u, n)) + (double)margin;
  if (!valid) return;
  const bool active = x > 0.0;
  if (sub == 0) row_loss[b] = active ? x : 0.0;
  // (the difference and the product in double, one rounding: an inactive row's 0 * diff is an exact zero)
  const double k = active ? 2.0 / (double)B : 0.0;
  GU[at] = f4_diff_scaled(n, p, k);
  GP[at] = f4_diff_scaled(p, u, k);
  GN[at] = f4_diff_scaled(u, n, k);
}

// the mean of n row terms: one workgroup, block_sum_d's order
__global__ __launch_bounds__(256) void row_mean(const double* __restrict__ rows, int64_t n, double* __restrict__ loss) {
  const double s = block_sum_d(rows, n);
  if (threadIdx.x == 0) loss[0] = s / (double)n;
}

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v = fmaxf(v, __shfl_xor(v, w));
  return v;
}

__global__ __launch_bounds__(256) void kl_rows(const float* __restrict__ A, const float* __restrict__ Bq, int64_t R,
                                               int64_t C, double* __restrict__ row_loss, float* __restrict__ GA,
                                               float* __restrict__ GB) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;  // (a whole wave leaves together)
  const float* __restrict__ a = A + r * C;
  const float* __restrict__ b = Bq + r * C;
  float ma = -INFINITY, mb = -INFINITY;
  for (int64_t c = lane; c < C; c += 64) {
    ma = fmaxf(ma, a[c]);
    mb = fmaxf(mb, b[c]);
  }
  ma = wave_max_f(ma);
  mb = wave_max_f(mb);
  double sa = 0.0, sb = 0.0, sd = 0.0;
  for (int64_t c = lane; c < C; c += 64) {
    const float xa = a[c] - ma, xb = b[c] - mb;
    const float ea = expf(xa);
    sa += (double)ea;
    sb += (double)expf(xb);
    sd += (double)ea * ((double)xa - (double)xb);
  }
  sa = wave_sum_d(sa);
  sb = wave_sum_d(sb);
  sd = wave_sum_d(sd);
  const double la = log(sa), lb = log(sb);
  const double kl = sd / sa - la + lb;
  if (lane == 0) row_loss[r] = kl;
  const double inv_r = 1.0 / (double)R;
  float* __restrict__ ga = GA + r * C;
  float* __restrict__ gb = GB + r * C;
  for (int64_t c = lane; c < C; c += 64) {
    const double xa = (double)(a[c] - ma), xb = (double)(b[c] - mb);
    const double p = (double)expf((float)xa) / sa, q = (double)expf((float)xb) / sb;
    const double dl = (xa - la) - (xb - lb);  // lp_c - lq_c
    ga[c] = (float)(p * (dl - kl) * inv_r);
    gb[c] = (float)((q - p) * inv_r);
  }
}

}  // namespace

extern "C" {

int64_t srh_triplet_ws_bytes(int64_t B) { return B > 0 ? srh::align256(B * (int64_t)sizeof(double)) : 0; }

srh_status_t srh_triplet_fwd_bwd(const float* d_u, const float* d_p, const float* d_n, int64_t B, int32_t d, float margin,
                                 double* d_loss, float* d_gu, float* d_gp, float* d_gn, void* d_ws, void* stream) {
  SRH_REQUIRE(B > 0 && B < (int64_t(1) << 30), "triplet_fwd_bwd: bad batch size");
  SRH_SUPPORTED(srh::dim_supported(d), "triplet_fwd_bwd: d=%d unsupported (32, 64, 128 or 256; narrower rows are zero-padded)",
                d);
  SRH_REQUIRE(d_u && d_p && d_n && d_loss && d_gu && d_gp && d_gn && d_ws, "triplet_fwd_bwd: null argument");
  SRH_REQUIRE(std::isfinite(margin), "triplet_fwd_bwd: the margin must be finite");
  hipStream_t st = srh::as_stream(stream);
  const float4 *U = reinterpret_cast<const float4*>(d_u), *P = reinterpret_cast<const float4*>(d_p),
               *N = reinterpret_cast<const float4*>(d_n);
  float4 *GU = reinterpret_cast<float4*>(d_gu), *GP = reinterpret_cast<float4*>(d_gp), *GN = reinterpret_cast<float4*>(d_gn);
  double* rows = reinterpret_cast<double*>(d_ws);
#define SRH_TRIPLET(LPR)                                                                                        \
  triplet_rows<LPR><<<(int)(((B + 64 / LPR - 1) / (64 / LPR) + 3) / 4), 256, 0, st>>>(U, P, N, (int)B, margin, rows, GU, GP, GN)
  switch (d) {
    case 32: SRH_TRIPLET(8); break;
    case 64: SRH_TRIPLET(16); break;
    case 128: SRH_TRIPLET(32); break;
    default: SRH_TRIPLET(64); break;
  }
#undef SRH_TRIPLET
  SRH_LAUNCH_CHECK();
  row_mean<<<1, 256, 0, st>>>(rows, B, d_loss);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_kl_div_ws_bytes(int64_t R) { return R > 0 ? srh::align256(R * (int64_t)sizeof(double)) : 0; }

srh_status_t srh_kl_div_fwd_bwd(const float* d_p_logit, const float* d_q_logit, int64_t R, int64_t C, double* d_loss,
                                float* d_gp, float* d_gq, void* d_ws, void* stream) {
  SRH_REQUIRE(R > 0 && C > 0 && R < (int64_t(1) << 31) && C < (int64_t(1) << 31), "kl_div_fwd_bwd: bad R / C");
  SRH_REQUIRE(d_p_logit && d_q_logit && d_loss && d_gp && d_gq && d_ws, "kl_div_fwd_bwd: null argument");
  SRH_REQUIRE(d_gp != d_gq, "kl_div_fwd_bwd: d_gp and d_gq must be two buffers");
  hipStream_t st = srh::as_stream(stream);
  double* rows = reinterpret_cast<double*>(d_ws);
  kl_rows<<<(unsigned)((R + 3) / 4), 256, 0, st>>>(d_p_logit, d_q_logit, R, C, rows, d_gp, d_gq);
  SRH_LAUNCH_CHECK();
  row_mean<<<1, 256, 0, st>>>(rows, R, d_loss);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // extern "C"

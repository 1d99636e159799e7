// DuoRec's contrastive section: two info_nce terms (util/loss_torch.py:54-88) that share their anchor
// rows, forward and backward in two launches.  z = [X[idx_a]; X[idx_p]; X[idx_q]] are 3B "virtual" rows, m = blk B + b:
//   u-softmax over U = A u P, s-softmax over V = A u Q; a row never sees itself, P rows see no Q key and vice versa
//   lse^t_m = log sum_{j in keys_t(m)} exp(s_mj),  s = inv_temp z z^T,  loss_t = scale_t / 2B sum_m (lse^t_m - s_{m, partner_t(m)})
//   dz_r = sum_t scale_t inv_temp / 2B sum_{j in keys_t(r)} (exp(s_rj - lse^t_r) + exp(s_rj - lse^t_j) - 2 [j = partner_t(r)]) z_j
// The second exponential is the key side of the loss: s is symmetric, so the score a row forms for its own softmax is
// the score key j's softmax needs too, and one sweep over the key tiles with every lse known finishes the row.  One
// producer per gradient row, one summation order, no float atomics: the same bits on every call.
//   duo_lse   R = 64 virtual rows in registers, C = every virtual row through LDS (rowtile.h); per row two running
//             (max, sum) pairs, the -inf tile rule of ce_pass (contrastive.hip) -> lse^u, lse^s (float) and the row terms
//             lse - s_partner (double; the partner logit is the sweep's own score, so both carry one rounding)
//   duo_grad  the same sweep with the weights above on the score accumulator, accum16 -> the compact G = [ga; gp; gq];
//             one more workgroup sums the row terms in a fixed order into the two losses
// Rows are gathered through the index vectors as they are read; block membership is per row (a tile may hold rows of
// all three blocks).  d = 64 or 128.
#include <cmath>

#include "../../include/selfrec_hip.h"
#include "rowtile.h"

namespace {
using namespace srh;

struct DuoArgs {
  const float* x;          // rows x D
  const int32_t* idx[3];   // B each; all null: virtual row m is row m of x
  int64_t B;
  float inv_temp;
  float coef[2];           // scale_t inv_temp / 2B
  double lscale[2];        // scale_t / 2B
  double* losses;          // 2
  float* g;                // 3B x D
  // workspace
  float* lse[2];           // 3B each (+inf where the row has no such softmax)
  double* term[2];         // 3B each (0 where the row has no such softmax)
};

int64_t duo_layout(DuoArgs& a, void* ws) {
  Carver w(ws);
  for (int t = 0; t < 2; ++t) w.take(a.lse[t], 3 * a.B);
  for (int t = 0; t < 2; ++t) w.take(a.term[t], 3 * a.B);
  return w.used;
}

// the row of x behind virtual row m < 3B
__device__ __forceinline__ int64_t duo_src(const DuoArgs& P, int64_t m) {
  if (!P.idx[0]) return m;
  const int blk = (m >= P.B) + (m >= 2 * P.B);
  return (int64_t)P.idx[blk][m - blk * P.B];
}

// what a lane knows of its R row: block, and its partner's virtual row under each softmax (-1: none)
struct DuoRow {
  int64_t r;
  bool ok;
  int blk;
  int64_t partner[2];
};
__device__ __forceinline__ DuoRow duo_row(const DuoArgs& P, int64_t r) {
  DuoRow q;
  q.r = r;
  q.ok = r < 3 * P.B;
  q.blk = (r >= P.B) + (r >= 2 * P.B);
  const int64_t b = r - q.blk * P.B;
  q.partner[0] = !q.ok || q.blk == 2 ? -1 : (q.blk == 0 ? P.B + b : b);
  q.partner[1] = !q.ok || q.blk == 1 ? -1 : (q.blk == 0 ? 2 * P.B + b : b);
  return q;
}
// is key c one of row q's keys under softmax t (0: u, 1: s)?
__device__ __forceinline__ bool duo_member(const DuoArgs& P, const DuoRow& q, int64_t c, int t) {
  const int other = 2 - t;   // the block this softmax does not hold: Q for u, P for s
  const int cblk = (c >= P.B) + (c >= 2 * P.B);
  return q.ok && c < 3 * P.B && c != q.r && q.blk != other && cblk != other;
}

template <int D>
__device__ __forceinline__ void duo_stage(float* cs, const DuoArgs& P, int64_t c0) {
  constexpr int LDS_STRIDE = kRtStride<D>;
  for (int e = threadIdx.x; e < kRtRows * (D / 4); e += 256) {
    const int i = e / (D / 4), q = e % (D / 4);
    const int64_t c = c0 + i;
    const float4 x = c < 3 * P.B ? reinterpret_cast<const float4*>(P.x + duo_src(P, c) * D)[q] : f4_zero();
    *reinterpret_cast<float4*>(&cs[i * LDS_STRIDE + 4 * q]) = x;
  }
}

__device__ __forceinline__ float duo_max4(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  v = fmaxf(v, __shfl_xor(v, 32));
  return v;
}

template <int D>
__global__ __launch_bounds__(256) void duo_lse(DuoArgs P) {
  __shared__ float cs[kRtRows * kRtStride<D>];
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const DuoRow row = duo_row(P, (int64_t)blockIdx.x * kRtRows + L.wave * 16 + j16);
  const int64_t n = 3 * P.B;
  float rf[D / 4];
  load_rf<D>(rf, P.x, row.ok ? duo_src(P, row.r) : 0, row.ok, g);
  float m[2] = {-INFINITY, -INFINITY};
  double rs[2] = {0.0, 0.0};
  float sp[2] = {0.f, 0.f};

  for (int64_t c0 = 0; c0 < n; c0 += kRtRows) {
    __syncthreads();
    duo_stage<D>(cs, P, c0);
    __syncthreads();
    f32x4 s[kRtRows / 16];
#pragma unroll
    for (int sub = 0; sub < kRtRows / 16; ++sub) s[sub] = score16<D>(cs, sub, j16, g, rf) * P.inv_temp;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      // keys outside the row's softmax are -inf before the max; a tile may hold none of the row's keys (its own key
      // alone, or a whole Q tile for a P row): while the running max is -inf the rescale factor and the weights are 0
      float mx = -INFINITY;
#pragma unroll
      for (int sub = 0; sub < kRtRows / 16; ++sub)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t c = c0 + sub * 16 + 4 * g + reg;
          if (duo_member(P, row, c, t)) mx = fmaxf(mx, s[sub][reg]);
          if (c == row.partner[t]) sp[t] = s[sub][reg];
        }
      const float m_new = fmaxf(m[t], duo_max4(mx));
      rs[t] *= (double)(m[t] == -INFINITY ? 0.f : expf(m[t] - m_new));
      m[t] = m_new;
      const float m_sub = m_new == -INFINITY ? 0.f : m_new;
#pragma unroll
      for (int sub = 0; sub < kRtRows / 16; ++sub)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          if (duo_member(P, row, c0 + sub * 16 + 4 * g + reg, t)) rs[t] += (double)expf(s[sub][reg] - m_sub);
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    rs[t] = sum4(rs[t]);
    // the partner logit is the score the sweep itself formed (one of the row's four lanes met it, the others hold 0):
    // lse and s_pos then carry the same rounding of that score, and where the positive wins, m - s_pos is an exact 0
    const double spos = (double)sum4(sp[t]);
    const bool has = row.partner[t] >= 0;
    if (row.ok && g == 0) {
      const double lrs = log(rs[t]);
      P.lse[t][row.r] = has ? (float)((double)m[t] + lrs) : INFINITY;
      P.term[t][row.r] = has ? ((double)m[t] - spos) + lrs : 0.0;
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void duo_grad(DuoArgs P) {
  __shared__ float cs[kRtRows * kRtStride<D>];
  __shared__ float clse[2][kRtRows];
  const int64_t n = 3 * P.B;
  if ((int64_t)blockIdx.x * kRtRows >= n) {
    // the last workgroup: both losses, the row terms in a fixed order
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
      const double sum = block_sum_d(P.term[t], n);
      if (threadIdx.x == 0) P.losses[t] = P.lscale[t] * sum;
      __syncthreads();
    }
    return;
  }
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const DuoRow row = duo_row(P, (int64_t)blockIdx.x * kRtRows + L.wave * 16 + j16);
  float rf[D / 4];
  load_rf<D>(rf, P.x, row.ok ? duo_src(P, row.r) : 0, row.ok, g);
  const float rl[2] = {row.ok ? P.lse[0][row.r] : INFINITY, row.ok ? P.lse[1][row.r] : INFINITY};
  f32x4 o[D / 16];
  zero_acc(o);

  for (int64_t c0 = 0; c0 < n; c0 += kRtRows) {
    __syncthreads();
    duo_stage<D>(cs, P, c0);
    if (threadIdx.x < 2 * kRtRows) {
      const int t = threadIdx.x / kRtRows, i = threadIdx.x % kRtRows;
      clse[t][i] = c0 + i < n ? P.lse[t][c0 + i] : INFINITY;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kRtRows / 16; ++sub) {
      f32x4 s = score16<D>(cs, sub, j16, g, rf) * P.inv_temp;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ci = sub * 16 + 4 * g + reg;
        const int64_t c = c0 + ci;
        float w = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (duo_member(P, row, c, t))
            w += P.coef[t] * (expf(s[reg] - rl[t]) + expf(s[reg] - clse[t][ci]) - (c == row.partner[t] ? 2.f : 0.f));
        s[reg] = w;
      }
      accum16<D>(o, cs, sub, j16, g, s);
    }
  }
  if (row.ok) store_acc<D>(o, P.g, row.r, g);
}

template <int D>
srh_status_t launch_duo(const DuoArgs& a, hipStream_t st) {
  const unsigned tiles = (unsigned)ceil_div(3 * a.B, kRtRows);
  duo_lse<D><<<tiles, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  duo_grad<D><<<tiles + 1, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // namespace

extern "C" {

int64_t srh_duo_nce_ws_bytes(int64_t B, int32_t d) {
  if (B <= 0 || B >= (int64_t(1) << 29) || (d != 64 && d != 128)) return 0;
  DuoArgs a{};
  a.B = B;
  return duo_layout(a, nullptr);
}

srh_status_t srh_duo_nce_fwd_bwd(const float* d_x, int64_t rows, const int32_t* d_idx_a, const int32_t* d_idx_p,
                                 const int32_t* d_idx_q, int64_t B, int32_t d, float inv_temp, float scale_u, float scale_s,
                                 double* d_losses, float* d_g, void* d_ws, void* stream) {
  SRH_SUPPORTED(d == 64 || d == 128, "duo_nce_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(B >= 1 && B < (int64_t(1) << 29), "duo_nce_fwd_bwd: bad B");
  SRH_REQUIRE(d_x && d_losses && d_g && d_ws, "duo_nce_fwd_bwd: null argument");
  const int n_idx = (d_idx_a != nullptr) + (d_idx_p != nullptr) + (d_idx_q != nullptr);
  SRH_REQUIRE(n_idx == 0 || n_idx == 3, "duo_nce_fwd_bwd: three index vectors, or none");
  SRH_REQUIRE(rows >= 3 * B || n_idx == 3, "duo_nce_fwd_bwd: without index vectors x holds the 3B = %lld rows (got %lld)",
              (long long)(3 * B), (long long)rows);
  SRH_REQUIRE(rows >= 1 && rows < (int64_t(1) << 31), "duo_nce_fwd_bwd: bad row count");
  SRH_REQUIRE(std::isfinite(inv_temp) && inv_temp > 0.f, "duo_nce_fwd_bwd: inv_temp must be positive and finite");
  SRH_REQUIRE(std::isfinite(scale_u) && std::isfinite(scale_s), "duo_nce_fwd_bwd: the scales must be finite");
  hipStream_t st = srh::as_stream(stream);
  if (B == 1) {
    // one key per softmax: lse is the partner logit, every weight is 1 + 1 - 2.  Exact zeros, written as such.
    SRH_HIP(hipMemsetAsync(d_losses, 0, 2 * sizeof(double), st));
    SRH_HIP(hipMemsetAsync(d_g, 0, sizeof(float) * 3 * (size_t)d, st));
    return SRH_OK;
  }
  DuoArgs a{};
  a.x = d_x;
  a.idx[0] = d_idx_a; a.idx[1] = d_idx_p; a.idx[2] = d_idx_q;
  a.B = B;
  a.inv_temp = inv_temp;
  const float scale[2] = {scale_u, scale_s};
  for (int t = 0; t < 2; ++t) {
    a.coef[t] = (float)((double)scale[t] * (double)inv_temp / (2.0 * (double)B));
    a.lscale[t] = (double)scale[t] / (2.0 * (double)B);
  }
  a.losses = d_losses;
  a.g = d_g;
  duo_layout(a, d_ws);
  return d == 64 ? launch_duo<64>(a, st) : launch_duo<128>(a, st);
}

}  // extern "C"

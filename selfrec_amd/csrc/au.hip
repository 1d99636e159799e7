// DirectAU (model/graph/DirectAU.py:37-48 of the reference): the alignment and uniformity losses of a batch's gathered
// rows, forward and backward in one call, with neither an n x n matrix nor torch.pdist's n (n - 1) / 2 distances in
// memory and no float atomics.  DESIGN.md 4.25.
//
// xh_i = x_i / max(|x_i|, 1e-12) (F.normalize), q_i = |xh_i|^2, s_ij = xh_i . xh_j
//   w_ij = exp(-t max(0, q_i + q_j - 2 s_ij)), w_ii = 0;  r_i = sum_j w_ij;  Z = sum_i r_i
//   U(x) = log(Z / (n (n - 1))),  dU/dxh_i = (4 t / Z) (sum_j w_ij xh_j - r_i xh_i)
//   A(x, y) = mean_i |xh_i - yh_i|^2,  dA/dxh_i = 2 (xh_i - yh_i) / n = -dA/dyh_i
//   prep     both sides: xh, 1 / max(|x|, 1e-12), q, and the row's |xh_i - yh_i|^2
//   gram     side x 64-row tile x key chunk: the tile's rows in registers, the SAME matrix through LDS 64 keys at a time;
//            score16 -> the weight on the accumulator (own index and keys >= n: exactly 0) -> accum16; the chunk's partial
//            r_i (double) and partial sum_j w_ij xh_j go to the workspace by plain stores (an empty chunk stores zeros)
//   reduce   one workgroup per side: r_i = the chunk partials in chunk order, Z = the rows in block_sum_d's order, U; a
//            third workgroup: A
//   finish   side x row tile: the partial rows in chunk order, (4 t w_u / Z) (O_i - [clamped] r_i xh_i) +- 2 w_align
//            (xh_i - yh_i) / n, the normalisation backward; workgroup (0, 0) writes the loss
// The radial part r_i xh_i of an ordinary row is what the projection of the normalisation backward removes: it is formed
// on clamped rows only, where nothing removes it.  The exponent is never positive, so there is no running maximum.
#include <cmath>

#include "rowtile.h"

namespace {

using namespace srh;

constexpr int kRows = kRtRows;       // R rows per workgroup = keys per LDS tile
constexpr int kGramTarget = 512;     // gram workgroups aimed for (2 sides x row tiles x key chunks)
constexpr float kNormEps = 1e-12f;   // F.normalize's eps, on the norm
constexpr int64_t kMaxN = int64_t(1) << 24;

struct AuArgs {
  const float* x[2];   // x, y (y may be null: sides == 1)
  float* gx[2];
  int sides;
  int64_t n;
  float t, w_align, w_u[2];
  double* parts;       // [A, U(x), U(y)]
  double* loss;
  // workspace
  float* xn[2];        // n x D   normalised rows
  float* inv[2];       // n       1 / max(|x|, 1e-12)
  float* q[2];         // n       |xh|^2
  float* clamped[2];   // n       1 where the norm was below the eps
  double* arow;        // n       |xh_i - yh_i|^2
  double* part_r[2];   // chunks x n       sum_j w_ij over the chunk's keys
  float* part_o[2];    // chunks x n x D   sum_j w_ij xh_j over the chunk's keys
  double* rs[2];       // n       r_i
  double* red;         // [A, U(x), U(y), Z(x), Z(y)]
  int64_t chunks, chunk_len;
};

// the key chunks: a pure function of n, so the workspace query and the launch agree and every call sums alike
inline int64_t au_chunks(int64_t n) {
  const int64_t tiles = ceil_div(n, kRows);
  int64_t c = ceil_div(kGramTarget, 2 * tiles);
  if (c > tiles) c = tiles;
  return c < 1 ? 1 : c;
}
inline int64_t au_chunk_len(int64_t n) { return ceil_div(ceil_div(n, au_chunks(n)), kRows) * kRows; }

// the workspace of p.n rows: null ws measures, a workspace carves; returns the bytes
int64_t au_layout(AuArgs& p, void* ws, int D) {
  Carver w(ws);
  const int64_t n = p.n;
  p.chunks = au_chunks(n);
  p.chunk_len = au_chunk_len(n);
  for (int s = 0; s < 2; ++s) w.take(p.xn[s], n * D);
  for (int s = 0; s < 2; ++s) w.take(p.inv[s], n);
  for (int s = 0; s < 2; ++s) w.take(p.q[s], n);
  for (int s = 0; s < 2; ++s) w.take(p.clamped[s], n);
  w.take(p.arow, n);
  for (int s = 0; s < 2; ++s) w.take(p.part_r[s], p.chunks * n);
  for (int s = 0; s < 2; ++s) w.take(p.part_o[s], p.chunks * n * D);
  for (int s = 0; s < 2; ++s) w.take(p.rs[s], n);
  w.take(p.red, 8);
  return w.used;
}

// prep: LPR = D/4 lanes per row, one float4 of each side per lane
template <int D>
__global__ __launch_bounds__(256) void au_prep(AuArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  const bool ok = row < a.n;
  float4 h[2] = {f4_zero(), f4_zero()};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s >= a.sides) break;   // (uniform)
    const float4 v = ok ? reinterpret_cast<const float4*>(a.x[s] + row * D)[lane] : f4_zero();
    const float norm = sqrtf(group_sum<LPR>(f4_dot(v, v)));
    const float den = fmaxf(norm, kNormEps);
    h[s] = make_float4(v.x / den, v.y / den, v.z / den, v.w / den);
    const float q = group_sum<LPR>(f4_dot(h[s], h[s]));
    if (ok) {
      reinterpret_cast<float4*>(a.xn[s] + row * D)[lane] = h[s];
      if (lane == 0) {
        a.inv[s][row] = 1.f / den;
        a.q[s][row] = q;
        a.clamped[s][row] = norm < kNormEps ? 1.f : 0.f;
      }
    }
  }
  if (a.sides == 2) {
    const float4 dlt = make_float4(h[0].x - h[1].x, h[0].y - h[1].y, h[0].z - h[1].z, h[0].w - h[1].w);
    const float ss = group_sum<LPR>(f4_dot(dlt, dlt));
    if (ok && lane == 0) a.arow[row] = (double)ss;
  }
}

template <int D>
__global__ __launch_bounds__(256) void au_gram(AuArgs a) {
  __shared__ float cs[kRows * kRtStride<D>];
  __shared__ float qs[kRows];
  const int side = blockIdx.y;
  const int64_t n = a.n;
  const int64_t rtile = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x % a.chunks;
  const int64_t cbeg = chunk * a.chunk_len;
  const int64_t cend = cbeg + a.chunk_len < n ? cbeg + a.chunk_len : n;   // (an empty chunk: cend <= cbeg)
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int64_t r = rtile * kRows + L.wave * 16 + j16;
  const bool rok = r < n;
  const float* __restrict__ xn = a.xn[side];
  const float* __restrict__ qv = a.q[side];
  const float nt = -a.t;
  float rf[D / 4];
  load_rf<D>(rf, xn, r, rok, g);
  const float qr = rok ? qv[r] : 0.f;
  f32x4 o[D / 16];
  zero_acc(o);
  double rsum = 0.0;
  for (int64_t c0 = cbeg; c0 < cend; c0 += kRows) {
    __syncthreads();
    stage_tile<D>(cs, xn, c0, cend);
    if (threadIdx.x < kRows) qs[threadIdx.x] = c0 + threadIdx.x < cend ? qv[c0 + threadIdx.x] : 0.f;
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < kRows / 16; ++sub) {
      f32x4 s = score16<D>(cs, sub, j16, g, rf);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ci = sub * 16 + 4 * g + reg;
        const int64_t c = c0 + ci;
        const float d2 = fmaxf(fmaf(-2.f, s[reg], qr + qs[ci]), 0.f);
        // the own index and the keys past the end weigh exactly nothing (not exp(-t q_i))
        const float w = (c < cend && c != r) ? expf(nt * d2) : 0.f;
        rsum += (double)w;
        s[reg] = w;
      }
      accum16<D>(o, cs, sub, j16, g, s);
    }
  }
  rsum = sum4(rsum);
  if (rok) {
    if (g == 0) a.part_r[side][chunk * n + r] = rsum;
    store_acc<D>(o, a.part_o[side] + chunk * n * D, r, g);
  }
}

// workgroup `side` < sides: r_i, Z and U of that side; workgroup 2 (two sides only): A
__global__ __launch_bounds__(256) void au_reduce(AuArgs a) {
  const int b = blockIdx.x;
  const int64_t n = a.n;
  if (b < 2) {
    const double* pr = a.part_r[b];
    double* rs = a.rs[b];
    for (int64_t e = threadIdx.x; e < n; e += 256) {
      double s = 0.0;
      for (int64_t c = 0; c < a.chunks; ++c) s += pr[c * n + e];
      rs[e] = s;
    }
    __syncthreads();
    const double z = block_sum_d(rs, n);
    if (threadIdx.x == 0) {
      const double u = log(z / ((double)n * (double)(n - 1)));
      a.red[1 + b] = u;
      a.red[3 + b] = z;
      a.parts[1 + b] = u;
    }
  } else {
    const double s = block_sum_d(a.arow, n);
    if (threadIdx.x == 0) {
      a.red[0] = s / (double)n;
      a.parts[0] = s / (double)n;
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void au_finish(AuArgs a) {
  const int side = blockIdx.y;
  const int64_t n = a.n;
  const RtLane L = rt_lane();
  const int g = L.g;
  const int64_t r = (int64_t)blockIdx.x * kRows + L.wave * 16 + L.j16;
  const bool rok = r < n;
  const float* __restrict__ xn = a.xn[side];
  f32x4 o[D / 16];
  zero_acc(o);
  if (rok) {
    for (int64_t c = 0; c < a.chunks; ++c) {
      const float* po = a.part_o[side] + (c * n + r) * D;
#pragma unroll
      for (int b = 0; b < D / 16; ++b) {
        const float4 v = reinterpret_cast<const float4*>(po + 16 * b + 4 * g)[0];
        o[b][0] += v.x; o[b][1] += v.y; o[b][2] += v.z; o[b][3] += v.w;
      }
    }
  }
  const bool clamped = rok && a.clamped[side][r] != 0.f;
  const float cu = (float)(4.0 * (double)a.t * (double)a.w_u[side] / a.red[3 + side]);
  const float ri = clamped ? (float)a.rs[side][r] : 0.f;   // an ordinary row's radial part is projected out below
  const bool two = a.sides == 2;
  const float ca = two ? (side == 0 ? 2.f : -2.f) * a.w_align / (float)n : 0.f;
#pragma unroll
  for (int b = 0; b < D / 16; ++b) {
    const int64_t at = r * D + 16 * b + 4 * g;
    const float4 x0 = rok ? reinterpret_cast<const float4*>(a.xn[0] + at)[0] : f4_zero();
    const float4 x1 = (rok && two) ? reinterpret_cast<const float4*>(a.xn[1] + at)[0] : x0;
    const float4 me = side == 0 ? x0 : x1;
    // xh_i - yh_i, the same difference on both sides (ca carries the sign; one side: ca = 0)
    o[b][0] = fmaf(ca, x0.x - x1.x, cu * (o[b][0] - ri * me.x));
    o[b][1] = fmaf(ca, x0.y - x1.y, cu * (o[b][1] - ri * me.y));
    o[b][2] = fmaf(ca, x0.z - x1.z, cu * (o[b][2] - ri * me.z));
    o[b][3] = fmaf(ca, x0.w - x1.w, cu * (o[b][3] - ri * me.w));
  }
  const float inv = rok ? a.inv[side][r] : 1.f;
  norm_bwd_store<D>(o, xn, inv, clamped, r, rok, g, a.gx[side]);
  if (blockIdx.x == 0 && side == 0 && threadIdx.x == 0) {
    double loss = (double)a.w_u[0] * a.red[1];
    if (two) loss += (double)a.w_align * a.red[0] + (double)a.w_u[1] * a.red[2];
    a.loss[0] = loss;
  }
}

template <int D>
srh_status_t launch_au(const AuArgs& a, hipStream_t st) {
  constexpr int RPB = 256 / (D / 4);
  const unsigned tiles = (unsigned)ceil_div(a.n, kRows);
  au_prep<D><<<(unsigned)ceil_div(a.n, RPB), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  au_gram<D><<<dim3(tiles * (unsigned)a.chunks, a.sides), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  au_reduce<<<a.sides == 2 ? 3 : 1, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  au_finish<D><<<dim3(tiles, a.sides), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // namespace

extern "C" {

int64_t srh_au_ws_bytes(int64_t n, int32_t d) {
  if (n < 2 || n >= kMaxN || (d != 64 && d != 128)) return 0;
  AuArgs a{};
  a.n = n;
  return au_layout(a, nullptr, d);
}

srh_status_t srh_au_chunk_plan(int64_t n, int64_t* chunks, int64_t* chunk_len) {
  SRH_REQUIRE(chunks && chunk_len, "au_chunk_plan: null argument");
  SRH_REQUIRE(n >= 2 && n < kMaxN, "au_chunk_plan: n=%lld outside 2 .. 2^24 - 1", (long long)n);
  *chunks = au_chunks(n);
  *chunk_len = au_chunk_len(n);
  return SRH_OK;
}

srh_status_t srh_au_fwd_bwd(const float* d_x, const float* d_y, int64_t n, int32_t d, float t, float w_align, float w_ux,
                            float w_uy, double* d_parts, double* d_loss, float* d_gx, float* d_gy, void* d_ws,
                            void* stream) {
  SRH_SUPPORTED(d == 64 || d == 128, "au_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(n >= 2, "au_fwd_bwd: n=%lld rows have no pair (the uniformity of fewer than 2 rows is nan)", (long long)n);
  SRH_REQUIRE(n < kMaxN, "au_fwd_bwd: n=%lld too large (below 2^24)", (long long)n);
  SRH_REQUIRE(t > 0.f && std::isfinite(t), "au_fwd_bwd: t must be positive and finite");
  SRH_REQUIRE(std::isfinite(w_ux) && (!d_y || (std::isfinite(w_align) && std::isfinite(w_uy))),
              "au_fwd_bwd: the weights must be finite");
  SRH_REQUIRE(d_x && d_parts && d_loss && d_gx && d_ws, "au_fwd_bwd: null argument");
  SRH_REQUIRE(!d_y || d_gy, "au_fwd_bwd: d_y without d_gy");
  AuArgs a{};
  a.x[0] = d_x; a.x[1] = d_y;
  a.gx[0] = d_gx; a.gx[1] = d_gy;
  a.sides = d_y ? 2 : 1;
  a.n = n; a.t = t;
  a.w_align = d_y ? w_align : 0.f;
  a.w_u[0] = w_ux; a.w_u[1] = d_y ? w_uy : 0.f;
  a.parts = d_parts; a.loss = d_loss;
  au_layout(a, d_ws, d);
  hipStream_t st = srh::as_stream(stream);
  return d == 64 ? launch_au<64>(a, st) : launch_au<128>(a, st);
}

}  // extern "C"

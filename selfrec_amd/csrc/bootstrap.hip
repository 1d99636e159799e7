// The bootstrap family (model/graph/BUIR.py:69-95 and SelfCF.py:64-91 of the reference): the predictor, the two cosine
// terms against momentum-mixed targets, every gradient and the history store in one call, and BUIR's momentum update of
// the batch's target rows.  DESIGN.md 4.26.  All arithmetic fp32, the loss leaves as float64, no float atomics.
//
// p(x) = W x + b (nn.Linear: W is out x in), t_side[r] = alpha T_side[idx_side[r]] + beta x_side[r] (no gradient),
//   vh = v / max(|v|, eps),  cu_r = ph(x_u[r]) . th(t_i[r]),  ci_r = ph(x_i[r]) . th(t_u[r])
//   loss = c0 - c1 (mean_r cu_r + mean_r ci_r)
//   dP_r = -(c1 / B) (th - (ph . th) ph) / |p|; where |p| was clamped: -(c1 / B) th / eps (no projection: F.normalize
//   differentiates its max(|p|, eps)), or, with cos_clamp (F.cosine_similarity clamps the norm outside the graph),
//   -(c1 / B) (th - (ph . th) p / |p|) / eps
//   main     side x 64-row tile: the tile's x rows in registers as the B operand; W streams through LDS 64 output rows at a
//            time (rowtile.h: stage_tile, score16 -> P^T = W X^T on the accumulator, + b); the target row is mixed in the
//            accumulator's layout, so |p|, |t| and p . t are one sum4 each; dP is formed on the accumulator, written for
//            the weight gradients and fed back as the B operand of dX^T = W^T dP^T (accum16) from the same staged rows
//   loss     one workgroup: the row terms of each side in block_sum_d's order, the parts, the loss
//   wgrad    dP_side^T X_side per chunk of kRowChunk rows (chunked.hip: gemm64), the column sums of dP per chunk
//            (colsum_chunks); the user side's chunks, then the item side's, summed in that order (reduce_chunks)
//   store    LAST, a launch of its own: store_side[idx_side[r]] = x_side[r].  Every target read is in `main`, so a slot never
//            sees a history row another slot of the same call has overwritten (gather, then scatter)
#include <cmath>

#include "rowtile.h"

namespace {

using namespace srh;

constexpr int kRows = kRtRows;          // rows per workgroup = output rows of W per LDS tile
constexpr int kRowChunk = 256;          // rows per partial of the weight-gradient reductions
constexpr int64_t kMaxB = int64_t(1) << 24;

struct BootArgs {
  srh_boot_side_t s[2];   // user, item
  const float* w;         // D x D, out x in
  const float* b;         // D
  int64_t B;
  float alpha, beta, eps, c0, c1;
  int cos_clamp;          // a clamped row keeps its projection along p / |p| (SRH_BOOT_CLAMP_COSINE)
  double* loss;
  double* parts;          // [mean cu, mean ci]
  float* gw;
  float* gb;
  // workspace
  float* dp;              // 2 x B x D   dP of the user side, then of the item side
  double* rows;           // 2 x B       cu_r, then ci_r
  float* part_w;          // 2 chunks x D x D
  float* part_b;          // 2 chunks x D
};

// null ws measures, a workspace carves; returns the bytes
int64_t boot_layout(BootArgs& a, void* ws, int D) {
  Carver w(ws);
  const int64_t z = ceil_div(a.B, kRowChunk);
  w.take(a.dp, 2 * a.B * D);
  w.take(a.rows, 2 * a.B);
  w.take(a.part_w, 2 * z * D * D);
  w.take(a.part_b, 2 * z * D);
  return w.used;
}

// the table row of slot r: idx[r] (r itself without an index list), or -1 where it names no row
__device__ __forceinline__ int64_t slot_row(const int32_t* idx, int64_t r, int64_t n_rows) {
  const int64_t id = idx ? (int64_t)idx[r] : r;
  return (id >= 0 && id < n_rows) ? id : -1;
}

template <int D>
__global__ __launch_bounds__(256) void boot_main(BootArgs a) {
  __shared__ float cs[kRows * kRtStride<D>];
  const int side = blockIdx.y;
  const srh_boot_side_t& me = a.s[side];
  const srh_boot_side_t& ot = a.s[1 - side];   // p(x_u) meets the ITEM target, p(x_i) the user target
  const int64_t B = a.B;
  const RtLane L = rt_lane();
  const int g = L.g, j16 = L.j16;
  const int64_t r = (int64_t)blockIdx.x * kRows + L.wave * 16 + j16;
  const bool rok = r < B;

  // P^T = W X^T + b: p[bk][reg] = P[r][16 bk + 4 g + reg]
  f32x4 p[D / 16];
  {
    float rf[D / 4];
    load_rf<D>(rf, me.d_x, r, rok, g);
#pragma unroll
    for (int jc = 0; jc < D / kRows; ++jc) {
      __syncthreads();
      stage_tile<D>(cs, a.w, jc * kRows, D);
      __syncthreads();
#pragma unroll
      for (int sub = 0; sub < kRows / 16; ++sub) {
        const int bk = jc * (kRows / 16) + sub;
        const float4 bv = *reinterpret_cast<const float4*>(a.b + 16 * bk + 4 * g);
        p[bk] = score16<D>(cs, sub, j16, g, rf);
        p[bk][0] += bv.x; p[bk][1] += bv.y; p[bk][2] += bv.z; p[bk][3] += bv.w;
      }
    }
  }

  // the target row in the same layout; an id outside the table reads a zero row
  const int64_t id = rok ? slot_row(ot.d_idx, r, ot.d_idx ? ot.n_tgt : B) : -1;
  float4 t[D / 16];
  float pp = 0.f, tt = 0.f, pt = 0.f;
#pragma unroll
  for (int bk = 0; bk < D / 16; ++bk) {
    const int col = 16 * bk + 4 * g;
    const float4 tv = id >= 0 ? *reinterpret_cast<const float4*>(ot.d_tgt + id * D + col) : f4_zero();
    const float4 xv = rok ? *reinterpret_cast<const float4*>(ot.d_x + r * D + col) : f4_zero();
    t[bk] = make_float4(__fadd_rn(__fmul_rn(tv.x, a.alpha), __fmul_rn(xv.x, a.beta)),
                        __fadd_rn(__fmul_rn(tv.y, a.alpha), __fmul_rn(xv.y, a.beta)),
                        __fadd_rn(__fmul_rn(tv.z, a.alpha), __fmul_rn(xv.z, a.beta)),
                        __fadd_rn(__fmul_rn(tv.w, a.alpha), __fmul_rn(xv.w, a.beta)));
    const float4 pv = make_float4(p[bk][0], p[bk][1], p[bk][2], p[bk][3]);
    pp += f4_dot(pv, pv);
    tt += f4_dot(t[bk], t[bk]);
    pt += f4_dot(pv, t[bk]);
  }
  pp = sum4(pp); tt = sum4(tt); pt = sum4(pt);
  const float np = sqrtf(pp), nt = sqrtf(tt);
  const bool clamped = np < a.eps;
  const float ip = 1.f / fmaxf(np, a.eps), it = 1.f / fmaxf(nt, a.eps);
  const float c = (pt * ip) * it;                       // ph . th
  if (rok && g == 0) a.rows[side * B + r] = (double)c;

  // dP on the accumulator: k (th - cp p) / max(|p|, eps), cp = c / |p| on an ordinary row; on a clamped one 0, or with
  // cos_clamp still c / |p| (0 at p = 0)
  const float k = -a.c1 / (float)B * ip;
  const float cp = clamped ? ((a.cos_clamp && np > 0.f) ? c / np : 0.f) : c * ip;
  float* __restrict__ dpo = a.dp + (int64_t)side * B * D;
#pragma unroll
  for (int bk = 0; bk < D / 16; ++bk) {
    p[bk][0] = k * (t[bk].x * it - cp * p[bk][0]);
    p[bk][1] = k * (t[bk].y * it - cp * p[bk][1]);
    p[bk][2] = k * (t[bk].z * it - cp * p[bk][2]);
    p[bk][3] = k * (t[bk].w * it - cp * p[bk][3]);
  }
  if (rok) store_acc<D>(p, dpo, r, g);

  // dX^T = W^T dP^T: o[bk][reg] = dX[r][16 bk + 4 g + reg]
  f32x4 o[D / 16];
  zero_acc(o);
#pragma unroll
  for (int jc = 0; jc < D / kRows; ++jc) {
    if constexpr (D > kRows) {           // (D = 64: the one tile of W is still staged)
      __syncthreads();
      stage_tile<D>(cs, a.w, jc * kRows, D);
      __syncthreads();
    }
#pragma unroll
    for (int sub = 0; sub < kRows / 16; ++sub) accum16<D>(o, cs, sub, j16, g, p[jc * (kRows / 16) + sub]);
  }
  if (rok) store_acc<D>(o, me.d_gx, r, g);
}

__global__ __launch_bounds__(256) void boot_loss(BootArgs a) {
  const double su = block_sum_d(a.rows, a.B);
  __syncthreads();
  const double si = block_sum_d(a.rows + a.B, a.B);
  if (threadIdx.x == 0) {
    const double mu = su / (double)a.B, mi = si / (double)a.B;
    a.parts[0] = mu;
    a.parts[1] = mi;
    a.loss[0] = (double)a.c0 - (double)a.c1 * (mu + mi);
  }
}

// store_side[idx_side[r]] = x_side[r]; LPR = D / 4 lanes per row.  Slots of one id hold the same bits (the caller's rows
// are gathered by that id), so their order does not matter.
template <int D>
__global__ __launch_bounds__(256) void boot_store(BootArgs a) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const srh_boot_side_t& me = a.s[blockIdx.y];
  if (!me.d_store) return;
  const int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int lane = threadIdx.x % LPR;
  if (r >= a.B) return;
  const int64_t id = slot_row(me.d_idx, r, me.d_idx ? me.n_tgt : a.B);
  if (id < 0) return;
  reinterpret_cast<float4*>(me.d_store + id * D)[lane] = reinterpret_cast<const float4*>(me.d_x + r * D)[lane];
}

template <int D>
srh_status_t launch_boot(const BootArgs& a, hipStream_t st) {
  const unsigned tiles = (unsigned)ceil_div(a.B, kRows);
  const int64_t z = ceil_div(a.B, kRowChunk);
  boot_main<D><<<dim3(tiles, 2), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  boot_loss<<<1, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  srh_status_t s;
  for (int side = 0; side < 2; ++side) {
    const float* dp = a.dp + (int64_t)side * a.B * D;
    GemmArgs g{};
    g.A = dp; g.sam = 1; g.sak = D;                 // A = dP^T (D x B)
    g.B = a.s[side].d_x; g.sbk = D; g.sbn = 1;      // B = X (B x D)
    g.C = a.part_w + side * z * D * D; g.ldc = D; g.c_zstride = (int64_t)D * D;
    g.M = D; g.N = D; g.K = a.B; g.kchunk = kRowChunk;
    if ((s = gemm64(g, EPI_STORE, z, st)) != SRH_OK) return s;
    if ((s = colsum_chunks(dp, a.B, D, 1, kRowChunk, a.part_b + side * z * D, st)) != SRH_OK) return s;
  }
  if ((s = reduce_chunks(a.part_w, 2 * z, (int64_t)D * D, 1.f, a.gw, st)) != SRH_OK) return s;
  if ((s = reduce_chunks(a.part_b, 2 * z, D, 1.f, a.gb, st)) != SRH_OK) return s;
  if (a.s[0].d_store || a.s[1].d_store) {
    constexpr int RPB = 256 / (D / 4);
    boot_store<D><<<dim3((unsigned)ceil_div(a.B, RPB), 2), 256, 0, st>>>(a);
    SRH_LAUNCH_CHECK();
  }
  return SRH_OK;
}

// ---- momentum update of table rows -------------------------------------------------------------------------------------
// phase 1: every slot's new row from the values the table holds, into the workspace; phase 2 (a launch of its own): the
// stores.  Slots of one id compute and store the same bits: a repeated id is updated once.
__global__ __launch_bounds__(256) void momentum_mix(const float* __restrict__ tgt, const float* __restrict__ src,
                                                    const int32_t* __restrict__ idx, int64_t n, int64_t n_table, int d, float m,
                                                    float omm, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * d) return;
  const int64_t slot = e / d, id = slot_row(idx, slot, n_table);
  if (id < 0) return;
  const int64_t at = id * d + e % d;
  out[e] = __fadd_rn(__fmul_rn(tgt[at], m), __fmul_rn(src[at], omm));
}

__global__ __launch_bounds__(256) void momentum_store(float* __restrict__ tgt, const int32_t* __restrict__ idx, int64_t n,
                                                      int64_t n_table, int d, const float* __restrict__ val) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * d) return;
  const int64_t slot = e / d, id = slot_row(idx, slot, n_table);
  if (id < 0) return;
  tgt[id * d + e % d] = val[e];
}

bool boot_shape_ok(int64_t B, int32_t d) { return B >= 1 && B < kMaxB && (d == 64 || d == 128); }

}  // namespace

extern "C" {

int64_t srh_boot_ws_bytes(int64_t B, int32_t d) {
  if (!boot_shape_ok(B, d)) return 0;
  BootArgs a{};
  a.B = B;
  return boot_layout(a, nullptr, d);
}

srh_status_t srh_boot_fwd_bwd(const srh_boot_side_t* user, const srh_boot_side_t* item, const float* d_w, const float* d_b,
                              int64_t B, int32_t d, float alpha, float beta, float eps, float c0, float c1, int32_t clamp,
                              double* d_parts, double* d_loss, float* d_gw, float* d_gb, void* d_ws, void* stream) {
  SRH_SUPPORTED(d == 64 || d == 128, "boot_fwd_bwd: d=%d unsupported (64 or 128; narrower rows are zero-padded)", d);
  SRH_REQUIRE(B >= 1, "boot_fwd_bwd: B=%lld rows have no mean", (long long)B);
  SRH_REQUIRE(B < kMaxB, "boot_fwd_bwd: B=%lld too large (below 2^24)", (long long)B);
  SRH_REQUIRE(std::isfinite(alpha) && std::isfinite(beta) && std::isfinite(c0) && std::isfinite(c1),
              "boot_fwd_bwd: alpha, beta, c0 and c1 must be finite");
  SRH_REQUIRE(eps > 0.f && std::isfinite(eps), "boot_fwd_bwd: eps must be positive and finite");
  SRH_REQUIRE(clamp == SRH_BOOT_CLAMP_NORMALIZE || clamp == SRH_BOOT_CLAMP_COSINE, "boot_fwd_bwd: clamp=%d is neither "
              "SRH_BOOT_CLAMP_NORMALIZE nor SRH_BOOT_CLAMP_COSINE", clamp);
  SRH_REQUIRE(user && item && d_w && d_b && d_parts && d_loss && d_gw && d_gb && d_ws, "boot_fwd_bwd: null argument");
  BootArgs a{};
  a.s[0] = *user; a.s[1] = *item;
  for (int s = 0; s < 2; ++s) {
    const char* who = s == 0 ? "user" : "item";
    SRH_REQUIRE(a.s[s].d_x && a.s[s].d_tgt && a.s[s].d_gx, "boot_fwd_bwd: null argument on the %s side", who);
    SRH_REQUIRE(!a.s[s].d_idx || a.s[s].n_tgt >= 1, "boot_fwd_bwd: n_tgt=%lld on the %s side (an indexed table has rows)",
                (long long)a.s[s].n_tgt, who);
  }
  a.w = d_w; a.b = d_b; a.B = B;
  a.alpha = alpha; a.beta = beta; a.eps = eps; a.c0 = c0; a.c1 = c1;
  a.cos_clamp = clamp == SRH_BOOT_CLAMP_COSINE;
  a.parts = d_parts; a.loss = d_loss; a.gw = d_gw; a.gb = d_gb;
  boot_layout(a, d_ws, d);
  hipStream_t st = srh::as_stream(stream);
  return d == 64 ? launch_boot<64>(a, st) : launch_boot<128>(a, st);
}

int64_t srh_rows_momentum_ws_bytes(int64_t n, int32_t d) {
  if (n < 1 || d < 1) return 0;
  return align256(n * d * (int64_t)sizeof(float));
}

srh_status_t srh_rows_momentum_f32(float* d_tgt, const float* d_src, const int32_t* d_idx, int64_t n, int64_t n_table,
                                   int32_t d, float m, float one_minus_m, void* d_ws, void* stream) {
  SRH_REQUIRE(d >= 1, "rows_momentum: d=%d (at least one column)", d);
  SRH_REQUIRE(n >= 0 && n_table >= 0, "rows_momentum: n=%lld, n_table=%lld", (long long)n, (long long)n_table);
  SRH_REQUIRE(n < kMaxB * 64 && n * (int64_t)d < (int64_t(1) << 39), "rows_momentum: n=%lld rows of %d columns are too many",
              (long long)n, d);
  SRH_REQUIRE(std::isfinite(m) && std::isfinite(one_minus_m), "rows_momentum: m and 1 - m must be finite");
  if (n == 0) return SRH_OK;
  SRH_REQUIRE(d_tgt && d_src && d_idx && d_ws, "rows_momentum: null argument");
  hipStream_t st = srh::as_stream(stream);
  const unsigned grid = (unsigned)ceil_div(n * d, 256);
  momentum_mix<<<grid, 256, 0, st>>>(d_tgt, d_src, d_idx, n, n_table, d, m, one_minus_m, static_cast<float*>(d_ws));
  SRH_LAUNCH_CHECK();
  momentum_store<<<grid, 256, 0, st>>>(d_tgt, d_idx, n, n_table, d, static_cast<const float*>(d_ws));
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // extern "C"

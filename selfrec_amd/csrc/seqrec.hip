// SASRec (reference model/sequential/SASRec.py): causal self-attention over short sequences and the BCE loss.
// DESIGN.md 4.9.
//
// Attention.  Q, K, V are the projected (B, L, H dh) row-major tensors, L <= 64, dh 32 or 64, H dh <= 128.  One workgroup
// owns one (sequence, head); wave w owns the query rows 16w .. 16w + 15 and walks the key tiles t <= w (the tiles above
// the diagonal are masked whole and never computed).
//   srh_seq_attn_fwd_f32  K and V tiles sit in LDS.  S^T = K (Q / sqrt(dh))^T comes out of v_mfma_f32_16x16x4_f32 with
//                         acc[t][reg] = S[query j16][key 16t + 4g + reg]; the causal mask, the row softmax (two
//                         cross-lane steps over the four lanes that share a row) and the dropout multiplier are applied
//                         on the accumulator, which is then the B operand of O^T += V^T P^T with the k order 4g + reg
//                         matched by the A operand's row (the GEMM -> GEMM seam of ssl4rec.hip).  Only O and the row
//                         log-sum-exp are written.
//   srh_seq_attn_bwd_f32  the same ownership.  Pass 1 recomputes S and P = exp(S - lse), forms dP~ = dO V^T on the MFMA,
//                         dS = P (m dP~ - rowsum(m dP~ P)) / sqrt(dh) on the accumulator and dQ = dS K through the seam.
//                         Pass 2 turns the ownership to key tiles: P~ (then dS) of the whole (sequence, head) goes through
//                         one LDS buffer, dO (then Q) replaces V (then K) in theirs, and wave w sums dV = P~^T dO and
//                         dK = dS^T Q of the keys 16w .. 16w + 15 over the query tiles w .. in ascending order.
// Every output element has one producer and one summation order: no atomics, no scratch, the same bits on every call.
//
// BERT4Rec (reference model/sequential/BERT4Rec.py:123, attn_mask=None) takes the same kernels with the
// CAUSAL flag off (srh_seq_attn_full_*): every wave walks all the key tiles below L, the columns >= L of the last tile are
// masked before the row max (for a causal row they lie above the diagonal and need no test of their own), the dropout
// multiplier is drawn for the whole row, and pass 2 sums over all the query tiles from 0, where rows >= L hold zeros.
//
// Longer sequences (64 < L <= 512) take the tiled kernels (srh_seq_attn_tiled_*): the same wave, score and
// seam code over 64 x 64 blocks.  attn_tiled_fwd owns one 64-row query block of a (sequence, head), walks the key blocks in
// ascending order with K and V of one block in LDS, and rescales a per-row running maximum, sum and output at each block.
// attn_tiled_bwd_q has the same ownership and sums dQ over the key blocks; attn_tiled_bwd_kv turns it round: a workgroup
// owns a key block, its waves hold their keys' K and V rows as the register operand, the scaled Q and dO of one query block
// sit in LDS, S^T and dP~^T come out of the same scores() with the roles swapped, and dV and dK are summed over the query
// blocks in ascending order.  Both recompute P from lse and take delta = dO . O from the forward's output.
//
// Dropout on P: keep[b][h][row][col] injected as bytes, or drawn from the counter RNG of common.h at counter
// rng_counter + (b H + h) L + row, float4 number col / 4, word col % 4 (keep = u01(word) >= p); the backward redraws it.
//
// srh_seq_bce_fwd_bwd: one wave per hidden row gathers the target and the negative item rows, forms both logits and
// writes the row's two loss terms (float64), dL/dh and the two per-row table gradients; one workgroup then sums the
// terms in a fixed order.  The table gradient itself is srh_rows_segment_sum_f32 over the per-row gradients.
//
// CL4SRec (reference model/sequential/CL4SRec.py) runs the encoder on three stacked views, most of whose rows
// are padding.  srh_seq_embed_fwd_f32 is the embedding front in one launch: gather of both tables, scale, sum, dropout, and
// exact zeros for the dead rows without reading a table row for them.  srh_rows_live_sum_f32 is the table gradient behind it
// and behind the BCE: a segment sum over a host-built plan that lists live rows only and cuts every segment into chunks of
// SRH_LIVE_SUM_CHUNK rows -- one lane group per chunk, a second launch that adds the partials of the cut segments in chunk
// order; no atomics, one producer and one order per output element.
#include "common.h"

namespace {

using namespace srh;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxL = 64;        // query / key rows a workgroup holds
constexpr int kLdX = kMaxL + 8;  // LDS row stride (floats) of the P~ / dS buffer of the backward's second pass

enum { DROP_NONE = 0, DROP_GIVEN = 1, DROP_DRAWN = 2 };

struct AttnArgs {
  const float *q, *k, *v;
  const float *go, *lse_in;       // backward only
  const float* out_in;            // tiled backward only: the forward's out
  float *out, *lse;               // forward only
  float *gq, *gk, *gv;            // backward only
  const uint8_t* keep;
  int L, H;
  int drop;
  uint32_t seed_lo, seed_hi;
  uint64_t ctr;
  float drop_p, drop_scale, qscale;
};

// rows [0, L) of one head's (L x DH) slice (row stride E floats) -> dst[r][c] with row stride DH + 4; rows >= L zero.
// SCALED: every element times scale, rounded once (the tiled backward's Q block: the bits of the forward's query operand)
template <int DH, bool SCALED = false>
__device__ __forceinline__ void stage_tile(float* dst, const float* src, const int L, const int E, const float scale = 1.f) {
  constexpr int LD = DH + 4;
  for (int e = threadIdx.x; e < kMaxL * (DH / 4); e += 256) {
    const int r = e / (DH / 4), v = e % (DH / 4);
    float4 x = r < L ? *reinterpret_cast<const float4*>(src + (int64_t)r * E + 4 * v) : f4_zero();
    if constexpr (SCALED) x = make_float4(x.x * scale, x.y * scale, x.z * scale, x.w * scale);
    *reinterpret_cast<float4*>(&dst[r * LD + 4 * v]) = x;
  }
}

// the dropout multiplier of P[row][16t + 4g + reg], reg = 0..3 (row < L)
__device__ __forceinline__ void drop_mult4(const AttnArgs& a, const int64_t bh, const int row, const int t, const int g,
                                           float m[4]) {
  if (a.drop == DROP_NONE) {
    m[0] = m[1] = m[2] = m[3] = 1.f;
  } else if (a.drop == DROP_GIVEN) {
    const int c0 = 16 * t + 4 * g;
    const uint8_t* kp = a.keep + (bh * a.L + row) * a.L + c0;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) m[reg] = (c0 + reg < a.L && kp[reg] != 0) ? a.drop_scale : 0.f;
  } else {
    const uint4 w = counter_rng4(a.ctr + (uint64_t)(bh * a.L + row), (uint32_t)(4 * t + g), a.seed_lo, a.seed_hi);
    m[0] = u01(w.x) >= a.drop_p ? a.drop_scale : 0.f;
    m[1] = u01(w.y) >= a.drop_p ? a.drop_scale : 0.f;
    m[2] = u01(w.z) >= a.drop_p ? a.drop_scale : 0.f;
    m[3] = u01(w.w) >= a.drop_p ? a.drop_scale : 0.f;
  }
}

// the dropout multiplier of the single element P[row][col] (row, col < L): drop_mult4's value for it
__device__ __forceinline__ float drop_mult1(const AttnArgs& a, const int64_t bh, const int row, const int col) {
  if (a.drop == DROP_NONE) return 1.f;
  if (a.drop == DROP_GIVEN) return a.keep[(bh * a.L + row) * a.L + col] != 0 ? a.drop_scale : 0.f;
  const uint32_t w = counter_rng_word(a.ctr + (uint64_t)(bh * a.L + row), (uint32_t)(col >> 2), col & 3, a.seed_lo, a.seed_hi);
  return u01(w) >= a.drop_p ? a.drop_scale : 0.f;
}

// sum / max over the four lanes (g = 0..3) that share query row j16: the same bits in all four
__device__ __forceinline__ float row_sum4(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
__device__ __forceinline__ float row_max4(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  v = fmaxf(v, __shfl_xor(v, 32));
  return v;
}

// the key tiles a wave walks: up to its own when causal, every tile that holds a key otherwise
template <bool CAUSAL>
__device__ __forceinline__ bool walks_tile(const int t, const int wave, const int L) {
  return CAUSAL ? t <= wave : 16 * t < L;
}
// the keys a query row attends to
template <bool CAUSAL>
__device__ __forceinline__ bool sees_key(const int col, const int row, const int L) {
  return CAUSAL ? col <= row : col < L;
}

// st[t][reg] = S[query 16 wave + j16][key 16t + 4g + reg] for the tiles walked; qf: the lane's scaled query operand
template <int DH, bool CAUSAL>
__device__ __forceinline__ void scores(const float* Ks, const float (&qf)[DH / 4], const int wave, const int L, const int g,
                                       const int j16, f32x4 (&st)[4]) {
  constexpr int LD = DH + 4;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (walks_tile<CAUSAL>(t, wave, L)) {
      const float* arow = &Ks[(16 * t + j16) * LD + g];
#pragma unroll
      for (int k = 0; k < DH / 4; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * k], qf[k], acc, 0, 0, 0);
    }
    st[t] = acc;
  }
}

// out[u][reg] = sum over the keys of the tiles walked of Xs[key][16u + 4g + reg] bt[key], for query j16: the
// accumulator-shaped bt[t][reg] (key 16t + 4g + reg) is the B operand as it stands, Xs (keys x DH in LDS) gives the A
// operand's row for that k order
template <int DH, bool CAUSAL>
__device__ __forceinline__ void seam_product(const float* Xs, const f32x4 (&bt)[4], const int wave, const int L, const int g,
                                             const int j16, f32x4 (&out)[DH / 16]) {
  constexpr int LD = DH + 4;
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) out[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (walks_tile<CAUSAL>(t, wave, L)) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float* arow = &Xs[(16 * t + 4 * g + reg) * LD + j16];
#pragma unroll
        for (int u = 0; u < DH / 16; ++u)
          out[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[16 * u], bt[t][reg], out[u], 0, 0, 0);
      }
    }
  }
}

// ---- forward -----------------------------------------------------------------------------------------------------------
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_fwd(AttnArgs a) {
  constexpr int LD = DH + 4;
  __shared__ float Ks[kMaxL * LD];
  __shared__ float Vs[kMaxL * LD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int64_t bh = blockIdx.x;
  const int64_t b = bh / a.H;
  const int h = (int)(bh % a.H), L = a.L, E = a.H * DH;
  const int64_t base = b * L * E + h * DH;
  stage_tile<DH>(Ks, a.k + base, L, E);
  stage_tile<DH>(Vs, a.v + base, L, E);
  __syncthreads();
  if (16 * wave >= L) return;
  const int row = 16 * wave + j16;
  const bool rok = row < L;

  float qf[DH / 4];
#pragma unroll
  for (int k = 0; k < DH / 4; ++k) qf[k] = rok ? a.q[base + (int64_t)row * E + 4 * k + g] * a.qscale : 0.f;
  f32x4 st[4];
  scores<DH, CAUSAL>(Ks, qf, wave, L, g, j16, st);

  // the mask and the softmax of the row (key 0 is seen by every row: no empty row)
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      if (sees_key<CAUSAL>(16 * t + 4 * g + reg, row, L)) mx = fmaxf(mx, st[t][reg]);
  mx = row_max4(mx);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float p = sees_key<CAUSAL>(16 * t + 4 * g + reg, row, L) ? expf(st[t][reg] - mx) : 0.f;
      st[t][reg] = p;
      sum += p;
    }
  sum = row_sum4(sum);
  const float inv = 1.f / sum;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float m[4] = {1.f, 1.f, 1.f, 1.f};
    if (rok && walks_tile<CAUSAL>(t, wave, L)) drop_mult4(a, bh, row, t, g, m);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) st[t][reg] = rok ? st[t][reg] * inv * m[reg] : 0.f;
  }

  f32x4 ot[DH / 16];
  seam_product<DH, CAUSAL>(Vs, st, wave, L, g, j16, ot);
  if (!rok) return;
#pragma unroll
  for (int u = 0; u < DH / 16; ++u)
    *reinterpret_cast<float4*>(a.out + base + (int64_t)row * E + 16 * u + 4 * g) =
        make_float4(ot[u][0], ot[u][1], ot[u][2], ot[u][3]);
  if (g == 0) a.lse[bh * L + row] = mx + logf(sum);
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// dX[key 16 wave + j16][dim] = sum over queries of Xs[query][key] Ys[query][dim], query tiles (causal: wave, else 0) ..
// nT - 1 ascending
template <int DH, bool CAUSAL>
__device__ __forceinline__ void key_tile_product(const float* Xs, const float* Ys, const int wave, const int nT, const int g,
                                                 const int j16, f32x4 (&out)[DH / 16]) {
  constexpr int LD = DH + 4;
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) out[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int tq = CAUSAL ? wave : 0; tq < nT; ++tq) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int qr = 16 * tq + 4 * kk + g;
      const float bv = Xs[qr * kLdX + 16 * wave + j16];
      const float* arow = &Ys[qr * LD + j16];
#pragma unroll
      for (int u = 0; u < DH / 16; ++u) out[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[16 * u], bv, out[u], 0, 0, 0);
    }
  }
}

template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_bwd(AttnArgs a) {
  constexpr int LD = DH + 4;
  __shared__ float Ks[kMaxL * LD];     // K, then Q
  __shared__ float Vs[kMaxL * LD];     // V, then dO
  __shared__ float Xs[kMaxL * kLdX];   // P~, then dS
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const int64_t bh = blockIdx.x;
  const int64_t b = bh / a.H;
  const int h = (int)(bh % a.H), L = a.L, E = a.H * DH;
  const int64_t base = b * L * E + h * DH;
  const int nT = (L + 15) / 16;
  const bool active = wave < nT;
  const int row = 16 * wave + j16;
  const bool rok = active && row < L;
  stage_tile<DH>(Ks, a.k + base, L, E);
  stage_tile<DH>(Vs, a.v + base, L, E);
  __syncthreads();

  f32x4 pt[4], ds[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) pt[t] = ds[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    float qf[DH / 4], gof[DH / 4];
#pragma unroll
    for (int k = 0; k < DH / 4; ++k) {
      qf[k] = rok ? a.q[base + (int64_t)row * E + 4 * k + g] * a.qscale : 0.f;
      gof[k] = rok ? a.go[base + (int64_t)row * E + 4 * k + g] : 0.f;
    }
    f32x4 st[4];
    scores<DH, CAUSAL>(Ks, qf, wave, L, g, j16, st);
    scores<DH, CAUSAL>(Vs, gof, wave, L, g, j16, ds);     // ds[t][reg] = dP~[row][key 16t + 4g + reg] for now
    const float lse = rok ? a.lse_in[bh * L + row] : 0.f;
    float delta = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float m[4] = {1.f, 1.f, 1.f, 1.f};
      if (rok && walks_tile<CAUSAL>(t, wave, L)) drop_mult4(a, bh, row, t, g, m);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
#pragma clang fp contract(off)    // dp is rounded before dp - delta: fused into it, a row whose dS is 0 (L = 1) keeps dust
        const float p = (rok && sees_key<CAUSAL>(16 * t + 4 * g + reg, row, L)) ? expf(st[t][reg] - lse) : 0.f;
        const float dp = ds[t][reg] * m[reg];
        st[t][reg] = p;
        ds[t][reg] = dp;
        pt[t][reg] = p * m[reg];
        delta += dp * p;
      }
    }
    delta = row_sum4(delta);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
#pragma clang fp contract(off)
        ds[t][reg] = st[t][reg] * (ds[t][reg] - delta) * a.qscale;
      }
    f32x4 gq[DH / 16];
    seam_product<DH, CAUSAL>(Ks, ds, wave, L, g, j16, gq);
    if (rok) {
#pragma unroll
      for (int u = 0; u < DH / 16; ++u)
        *reinterpret_cast<float4*>(a.gq + base + (int64_t)row * E + 16 * u + 4 * g) =
            make_float4(gq[u][0], gq[u][1], gq[u][2], gq[u][3]);
    }
  }
  __syncthreads();                      // every wave is done with K and V
  stage_tile<DH>(Ks, a.q + base, L, E);
  stage_tile<DH>(Vs, a.go + base, L, E);
  if (active) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (walks_tile<CAUSAL>(t, wave, L))
        *reinterpret_cast<float4*>(&Xs[row * kLdX + 16 * t + 4 * g]) = make_float4(pt[t][0], pt[t][1], pt[t][2], pt[t][3]);
  }
  __syncthreads();
  const int key = 16 * wave + j16;
  f32x4 acc[DH / 16];
  if (active) {
    key_tile_product<DH, CAUSAL>(Xs, Vs, wave, nT, g, j16, acc);     // dV = P~^T dO
    if (key < L) {
#pragma unroll
      for (int u = 0; u < DH / 16; ++u)
        *reinterpret_cast<float4*>(a.gv + base + (int64_t)key * E + 16 * u + 4 * g) =
            make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
    }
  }
  __syncthreads();
  if (active) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (walks_tile<CAUSAL>(t, wave, L))
        *reinterpret_cast<float4*>(&Xs[row * kLdX + 16 * t + 4 * g]) = make_float4(ds[t][0], ds[t][1], ds[t][2], ds[t][3]);
  }
  __syncthreads();
  if (active) {
    key_tile_product<DH, CAUSAL>(Xs, Ks, wave, nT, g, j16, acc);     // dK = dS^T Q  (dS carries 1 / sqrt(dh))
    if (key < L) {
#pragma unroll
      for (int u = 0; u < DH / 16; ++u)
        *reinterpret_cast<float4*>(a.gk + base + (int64_t)key * E + 16 * u + 4 * g) =
            make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
    }
  }
}

// ---- tiled: 64 < L <= 512 -----------------------------------------------------------------------------
constexpr int kTiledMaxL = 512;

// what a tiled workgroup is: block blk of the nB 64-row blocks of (sequence, head) bh
struct TiledOwner {
  int64_t bh, base;       // base: the float offset of row 0 of the head's slice
  int blk, nB, E;
};
template <int DH>
__device__ __forceinline__ TiledOwner tiled_owner(const AttnArgs& a) {
  TiledOwner o;
  o.nB = (a.L + kMaxL - 1) / kMaxL;
  o.bh = blockIdx.x / o.nB;
  o.blk = (int)(blockIdx.x % o.nB);
  o.E = a.H * DH;
  o.base = (o.bh / a.H) * a.L * o.E + (o.bh % a.H) * DH;
  return o;
}

// the lane's share of dO_row . O_row: the columns 4k + g, k ascending.  The row's delta is the sum of the four shares in
// the order (g0 + g1) + (g2 + g3) -- row_sum4 in the dQ kernel, two steps over neighbouring lanes in the dK / dV kernel.
template <int DH>
__device__ __forceinline__ float delta_share(const float* go_row, const float* out_row, const int g) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < DH / 4; ++k) s += go_row[4 * k + g] * out_row[4 * k + g];
  return s;
}

// a query row that sees one key only (row 0 of a causal call, the row of L = 1) has P = 1 and dS = 0 identically; delta
// from dO . O and dP~ from the MFMA round differently, so the identity is written, not their difference
template <bool CAUSAL>
__device__ __forceinline__ bool lone_key(const int row, const int L) {
  return CAUSAL ? row == 0 : L == 1;
}

// one key block of the forward: DIAG = the causal block on the diagonal (local indices against the wave's own tile), else
// every key below Lk is seen
template <int DH, bool DIAG>
__device__ __forceinline__ void tiled_fwd_block(const AttnArgs& a, const float* Ks, const float* Vs,
                                                const float (&qf)[DH / 4], const int64_t bh, const int row, const bool rok,
                                                const int kb, const int Lk, const int wave, const int g, const int j16,
                                                float& mrun, float& lrun, f32x4 (&ot)[DH / 16]) {
  const int rloc = 16 * wave + j16;
  f32x4 st[4];
  scores<DH, DIAG>(Ks, qf, wave, Lk, g, j16, st);
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      if (sees_key<DIAG>(16 * t + 4 * g + reg, rloc, Lk)) mx = fmaxf(mx, st[t][reg]);
  const float mnew = fmaxf(mrun, row_max4(mx));      // finite: every block walked shows every row its key 0
  const float alpha = expf(mrun - mnew);             // 0 at the first block (mrun = -inf)
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float p = sees_key<DIAG>(16 * t + 4 * g + reg, rloc, Lk) ? expf(st[t][reg] - mnew) : 0.f;
      st[t][reg] = p;
      sum += p;
    }
  lrun = lrun * alpha + row_sum4(sum);
  mrun = mnew;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float m[4] = {1.f, 1.f, 1.f, 1.f};
    if (rok && walks_tile<DIAG>(t, wave, Lk)) drop_mult4(a, bh, row, 4 * kb + t, g, m);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) st[t][reg] = rok ? st[t][reg] * m[reg] : 0.f;
  }
  f32x4 pv[DH / 16];
  seam_product<DH, DIAG>(Vs, st, wave, Lk, g, j16, pv);
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) ot[u] = ot[u] * alpha + pv[u];
}

template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_tiled_fwd(AttnArgs a) {
  constexpr int LD = DH + 4;
  __shared__ float Ks[kMaxL * LD];
  __shared__ float Vs[kMaxL * LD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const TiledOwner o = tiled_owner<DH>(a);
  const int L = a.L, E = o.E;
  const int row = kMaxL * o.blk + 16 * wave + j16;
  const bool active = kMaxL * o.blk + 16 * wave < L, rok = row < L;

  float qf[DH / 4];
#pragma unroll
  for (int k = 0; k < DH / 4; ++k) qf[k] = rok ? a.q[o.base + (int64_t)row * E + 4 * k + g] * a.qscale : 0.f;
  float mrun = -INFINITY, lrun = 0.f;
  f32x4 ot[DH / 16];
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) ot[u] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int last = CAUSAL ? o.blk : o.nB - 1;
  for (int kb = 0; kb <= last; ++kb) {
    const int Lk = min(kMaxL, L - kMaxL * kb);
    __syncthreads();                    // every wave is done with the block before
    stage_tile<DH>(Ks, a.k + o.base + (int64_t)kMaxL * kb * E, Lk, E);
    stage_tile<DH>(Vs, a.v + o.base + (int64_t)kMaxL * kb * E, Lk, E);
    __syncthreads();
    if (!active) continue;
    if (CAUSAL && kb == o.blk) tiled_fwd_block<DH, true>(a, Ks, Vs, qf, o.bh, row, rok, kb, Lk, wave, g, j16, mrun, lrun, ot);
    else tiled_fwd_block<DH, false>(a, Ks, Vs, qf, o.bh, row, rok, kb, Lk, wave, g, j16, mrun, lrun, ot);
  }
  if (!rok) return;
  const float inv = 1.f / lrun;
#pragma unroll
  for (int u = 0; u < DH / 16; ++u)
    *reinterpret_cast<float4*>(a.out + o.base + (int64_t)row * E + 16 * u + 4 * g) =
        make_float4(ot[u][0] * inv, ot[u][1] * inv, ot[u][2] * inv, ot[u][3] * inv);
  if (g == 0) a.lse[o.bh * L + row] = mrun + logf(lrun);
}

// one key block of dQ: the first pass of attn_bwd on the block, with delta handed in
template <int DH, bool DIAG>
__device__ __forceinline__ void tiled_bwd_q_block(const AttnArgs& a, const float* Ks, const float* Vs,
                                                  const float (&qf)[DH / 4], const float (&gof)[DH / 4], const int64_t bh,
                                                  const int row, const bool rok, const bool lone, const float lse,
                                                  const float delta, const int kb, const int Lk, const int wave, const int g,
                                                  const int j16, f32x4 (&gq)[DH / 16]) {
  const int rloc = 16 * wave + j16;
  f32x4 st[4], ds[4];
  scores<DH, DIAG>(Ks, qf, wave, Lk, g, j16, st);
  scores<DH, DIAG>(Vs, gof, wave, Lk, g, j16, ds);      // dP~ for now
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float m[4] = {1.f, 1.f, 1.f, 1.f};
    if (rok && walks_tile<DIAG>(t, wave, Lk)) drop_mult4(a, bh, row, 4 * kb + t, g, m);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
#pragma clang fp contract(off)    // dp is rounded before dp - delta, as in attn_bwd
      const float p = (rok && sees_key<DIAG>(16 * t + 4 * g + reg, rloc, Lk)) ? expf(st[t][reg] - lse) : 0.f;
      const float dp = ds[t][reg] * m[reg];
      ds[t][reg] = lone ? 0.f : p * (dp - delta) * a.qscale;
    }
  }
  f32x4 part[DH / 16];
  seam_product<DH, DIAG>(Ks, ds, wave, Lk, g, j16, part);
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) gq[u] += part[u];
}

template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_tiled_bwd_q(AttnArgs a) {
  constexpr int LD = DH + 4;
  __shared__ float Ks[kMaxL * LD];
  __shared__ float Vs[kMaxL * LD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const TiledOwner o = tiled_owner<DH>(a);
  const int L = a.L, E = o.E;
  const int row = kMaxL * o.blk + 16 * wave + j16;
  const bool active = kMaxL * o.blk + 16 * wave < L, rok = row < L;

  float qf[DH / 4], gof[DH / 4];
#pragma unroll
  for (int k = 0; k < DH / 4; ++k) {
    qf[k] = rok ? a.q[o.base + (int64_t)row * E + 4 * k + g] * a.qscale : 0.f;
    gof[k] = rok ? a.go[o.base + (int64_t)row * E + 4 * k + g] : 0.f;
  }
  const float lse = rok ? a.lse_in[o.bh * L + row] : 0.f;
  const float delta =
      row_sum4(rok ? delta_share<DH>(a.go + o.base + (int64_t)row * E, a.out_in + o.base + (int64_t)row * E, g) : 0.f);
  f32x4 gq[DH / 16];
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) gq[u] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int last = CAUSAL ? o.blk : o.nB - 1;
  for (int kb = 0; kb <= last; ++kb) {
    const int Lk = min(kMaxL, L - kMaxL * kb);
    __syncthreads();
    stage_tile<DH>(Ks, a.k + o.base + (int64_t)kMaxL * kb * E, Lk, E);
    stage_tile<DH>(Vs, a.v + o.base + (int64_t)kMaxL * kb * E, Lk, E);
    __syncthreads();
    if (!active) continue;
    const bool lone = lone_key<CAUSAL>(row, L);
    if (CAUSAL && kb == o.blk)
      tiled_bwd_q_block<DH, true>(a, Ks, Vs, qf, gof, o.bh, row, rok, lone, lse, delta, kb, Lk, wave, g, j16, gq);
    else
      tiled_bwd_q_block<DH, false>(a, Ks, Vs, qf, gof, o.bh, row, rok, lone, lse, delta, kb, Lk, wave, g, j16, gq);
  }
  if (!rok) return;
#pragma unroll
  for (int u = 0; u < DH / 16; ++u)
    *reinterpret_cast<float4*>(a.gq + o.base + (int64_t)row * E + 16 * u + 4 * g) =
        make_float4(gq[u][0], gq[u][1], gq[u][2], gq[u][3]);
}

// dK and dV of one key block.  The roles of scores() and seam_product() are swapped: the lane's register operand is its
// KEY's row of K (then V), the LDS tile holds the QUERY block's scaled Q (then dO), so st[t][reg] is
// S[query 16t + 4g + reg][key j16] and the accumulator is again the B operand of the seam, whose sum runs over queries:
// dV^T += dO^T P~, dK^T += Q^T dS.  No P~ / dS buffer, no barrier between the two products.
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_tiled_bwd_kv(AttnArgs a) {
  constexpr int LD = DH + 4;
  __shared__ float Qs[kMaxL * LD];      // Q / sqrt(dh) of the query block
  __shared__ float Gs[kMaxL * LD];      // dO of the query block
  __shared__ float Ls[kMaxL], Ds[kMaxL];   // its rows' lse and delta
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j16 = lane & 15;
  const TiledOwner o = tiled_owner<DH>(a);
  const int L = a.L, E = o.E;
  const int kloc = 16 * wave + j16, key = kMaxL * o.blk + kloc;
  const bool active = kMaxL * o.blk + 16 * wave < L, kok = key < L;

  float kf[DH / 4], vf[DH / 4];
#pragma unroll
  for (int k = 0; k < DH / 4; ++k) {
    kf[k] = kok ? a.k[o.base + (int64_t)key * E + 4 * k + g] : 0.f;
    vf[k] = kok ? a.v[o.base + (int64_t)key * E + 4 * k + g] : 0.f;
  }
  f32x4 gk[DH / 16], gv[DH / 16];
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) gk[u] = gv[u] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int qb = CAUSAL ? o.blk : 0; qb < o.nB; ++qb) {
    const int Lq = min(kMaxL, L - kMaxL * qb);
    const int64_t qbase = o.base + (int64_t)kMaxL * qb * E;
    __syncthreads();
    stage_tile<DH, true>(Qs, a.q + qbase, Lq, E, a.qscale);
    stage_tile<DH>(Gs, a.go + qbase, Lq, E);
    {
      const int r = threadIdx.x >> 2, part = threadIdx.x & 3;      // four neighbouring lanes per query row
      float d = r < Lq ? delta_share<DH>(a.go + qbase + (int64_t)r * E, a.out_in + qbase + (int64_t)r * E, part) : 0.f;
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      if (part == 0) {
        Ds[r] = d;
        Ls[r] = r < Lq ? a.lse_in[o.bh * L + kMaxL * qb + r] : 0.f;
      }
    }
    __syncthreads();
    if (!active) continue;
    const bool diag = CAUSAL && qb == o.blk;
    f32x4 st[4], ds[4];
    scores<DH, false>(Qs, kf, wave, Lq, g, j16, st);
    scores<DH, false>(Gs, vf, wave, Lq, g, j16, ds);      // dP~ for now
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
#pragma clang fp contract(off)
        const int qloc = 16 * t + 4 * g + reg, qrow = kMaxL * qb + qloc;
        const bool seen = kok && qloc < Lq && (!diag || kloc <= qloc);
        const float m = seen ? drop_mult1(a, o.bh, qrow, key) : 0.f;
        const float p = seen ? expf(st[t][reg] - Ls[qloc]) : 0.f;
        const float dp = ds[t][reg] * m;
        st[t][reg] = p * m;                                                      // P~
        ds[t][reg] = lone_key<CAUSAL>(qrow, L) ? 0.f : p * (dp - Ds[qloc]);     // dS sqrt(dh): Qs carries 1 / sqrt(dh)
      }
    f32x4 part[DH / 16];
    seam_product<DH, false>(Gs, st, wave, Lq, g, j16, part);
#pragma unroll
    for (int u = 0; u < DH / 16; ++u) gv[u] += part[u];
    seam_product<DH, false>(Qs, ds, wave, Lq, g, j16, part);
#pragma unroll
    for (int u = 0; u < DH / 16; ++u) gk[u] += part[u];
  }
  if (!kok) return;
#pragma unroll
  for (int u = 0; u < DH / 16; ++u) {
    *reinterpret_cast<float4*>(a.gv + o.base + (int64_t)key * E + 16 * u + 4 * g) =
        make_float4(gv[u][0], gv[u][1], gv[u][2], gv[u][3]);
    *reinterpret_cast<float4*>(a.gk + o.base + (int64_t)key * E + 16 * u + 4 * g) =
        make_float4(gk[u][0], gk[u][1], gk[u][2], gk[u][3]);
  }
}

srh_status_t attn_check(const char* what, int64_t B, int32_t L, int32_t H, int32_t dh, const uint8_t* d_keep,
                        float drop_p, AttnArgs& a, const int max_l = kMaxL) {
  SRH_REQUIRE(B >= 1 && L >= 1 && H >= 1, "%s: bad shape B=%lld L=%d H=%d", what, (long long)B, L, H);
  SRH_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop probability must be in [0, 1)", what);
  SRH_SUPPORTED(L <= max_l, "%s: L=%d -- the kernel holds sequences of up to %d positions", what, L, max_l);
  SRH_SUPPORTED(dh == 32 || dh == 64, "%s: head width %d -- the kernel serves 32 and 64", what, dh);
  SRH_SUPPORTED((int64_t)H * dh <= 128, "%s: H dh = %lld -- the kernel serves up to 128", what, (long long)H * dh);
  SRH_SUPPORTED(B * H < (int64_t(1) << 31) && B * L * H * dh < (int64_t(1) << 40), "%s: too many sequences", what);
  a.L = L; a.H = H; a.keep = d_keep;
  a.drop = d_keep ? DROP_GIVEN : (drop_p > 0.f ? DROP_DRAWN : DROP_NONE);
  a.drop_p = drop_p;
  a.drop_scale = 1.f / (1.f - drop_p);
  a.qscale = 1.f / sqrtf((float)dh);
  return SRH_OK;
}

// ---- BCE ---------------------------------------------------------------------------------------------------------------
// one wave per hidden row
__global__ __launch_bounds__(256) void bce_rows(const float* __restrict__ hid, int64_t R, int32_t d,
                                                const float* __restrict__ table, int64_t n_table,
                                                const int32_t* __restrict__ pos, const int32_t* __restrict__ neg,
                                                const uint8_t* __restrict__ valid, double inv_n, double* __restrict__ terms,
                                                float* __restrict__ gh, float* __restrict__ grows) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const int64_t p = pos[r], n = neg[r];
  const bool ok = valid[r] != 0 && p >= 0 && p < n_table && n >= 0 && n < n_table;
  if (!ok) {
    for (int c = lane; c < d; c += 64) gh[r * d + c] = grows[r * d + c] = grows[(R + r) * d + c] = 0.f;
    if (lane == 0) terms[r] = terms[R + r] = 0.0;
    return;
  }
  float dp = 0.f, dn = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float hv = hid[r * d + c];
    dp = fmaf(hv, table[p * d + c], dp);
    dn = fmaf(hv, table[n * d + c], dn);
  }
  const double xp = (double)wave_sum_f(dp), xn = (double)wave_sum_f(dn);
  // BCE with logits, stable: max(x, 0) - x y + log1p(exp(-|x|));  d/dx = sigmoid(x) - y
  const double ep = exp(-fabs(xp)), en = exp(-fabs(xn));
  const double lp = fmax(xp, 0.0) - xp + log1p(ep), ln = fmax(xn, 0.0) + log1p(en);
  const double sp = xp >= 0.0 ? 1.0 / (1.0 + ep) : ep / (1.0 + ep), sn = xn >= 0.0 ? 1.0 / (1.0 + en) : en / (1.0 + en);
  const float cp = (float)((sp - 1.0) * inv_n), cn = (float)(sn * inv_n);
  for (int c = lane; c < d; c += 64) {
    const float hv = hid[r * d + c];
    gh[r * d + c] = fmaf(cp, table[p * d + c], cn * table[n * d + c]);
    grows[r * d + c] = cp * hv;
    grows[(R + r) * d + c] = cn * hv;
  }
  if (lane == 0) { terms[r] = lp; terms[R + r] = ln; }
}

// loss[0] / loss[1] = the mean of the positive / negative terms: thread i sums rows i, i + 256, ... ascending, then a
// fixed tree over the 256 partials
__global__ __launch_bounds__(256) void bce_reduce(const double* __restrict__ terms, int64_t R, double inv_n,
                                                  double* __restrict__ loss) {
  __shared__ double sp[256], sn[256];
  double a = 0.0, b = 0.0;
  for (int64_t r = threadIdx.x; r < R; r += 256) { a += terms[r]; b += terms[R + r]; }
  sp[threadIdx.x] = a; sn[threadIdx.x] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { sp[threadIdx.x] += sp[threadIdx.x + w]; sn[threadIdx.x] += sn[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { loss[0] = sp[0] * inv_n; loss[1] = sn[0] * inv_n; }
}

// ---- CL4SRec: the embedding front and the live-row table gradient -------------------------------------
// Dropout on the embedding rows: keep[r][c] injected as bytes, or drawn at counter rng_counter + r, float4 number c / 4,
// word c % 4 (keep = u01(word) >= p) -- the tower's contract (ssl4rec.hip).  One lane owns one float4 of a row.
struct RowDrop {
  const uint8_t* keep;
  int mode;
  uint32_t seed_lo, seed_hi;
  uint64_t ctr;
  float p, scale;
};

__device__ __forceinline__ float4 row_drop_mult(const RowDrop& dr, const int64_t r, const int d, const int v) {
  if (dr.mode == DROP_NONE) return make_float4(1.f, 1.f, 1.f, 1.f);
  if (dr.mode == DROP_GIVEN) {
    const uint8_t* kp = dr.keep + r * d + 4 * v;
    return make_float4(kp[0] ? dr.scale : 0.f, kp[1] ? dr.scale : 0.f, kp[2] ? dr.scale : 0.f, kp[3] ? dr.scale : 0.f);
  }
  const uint4 w = counter_rng4(dr.ctr + (uint64_t)r, (uint32_t)v, dr.seed_lo, dr.seed_hi);
  return make_float4(u01(w.x) >= dr.p ? dr.scale : 0.f, u01(w.y) >= dr.p ? dr.scale : 0.f,
                     u01(w.z) >= dr.p ? dr.scale : 0.f, u01(w.w) >= dr.p ? dr.scale : 0.f);
}

inline RowDrop make_row_drop(const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter, float drop_p) {
  RowDrop dr{};
  dr.keep = d_keep;
  dr.mode = d_keep ? DROP_GIVEN : (drop_p > 0.f ? DROP_DRAWN : DROP_NONE);
  dr.seed_lo = (uint32_t)rng_seed; dr.seed_hi = (uint32_t)(rng_seed >> 32); dr.ctr = rng_counter;
  dr.p = drop_p; dr.scale = 1.f / (1.f - drop_p);
  return dr;
}

// out[r] = (item[seq[r]] * scale + pos[posid[r]]) * m(r) for the live rows (seq[r] != 0, both ids inside their tables),
// exact zeros for every other row, whose table rows are not read.  d / 4 lanes per row.
__global__ __launch_bounds__(256) void seq_embed_rows(const float* __restrict__ item, int64_t n_item,
                                                      const float* __restrict__ pos, int64_t n_pos,
                                                      const int32_t* __restrict__ seq, const int32_t* __restrict__ posid,
                                                      int64_t R, int32_t d, float scale, RowDrop dr, float* __restrict__ out) {
  const int lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = t / lpr;
  const int v = (int)(t % lpr);
  if (r >= R) return;
  const int64_t it = seq[r], pl = posid[r];
  float4 o = f4_zero();
  if (it > 0 && it < n_item && pl >= 0 && pl < n_pos) {
    const float4 a = *reinterpret_cast<const float4*>(item + it * d + 4 * v);
    const float4 b = *reinterpret_cast<const float4*>(pos + pl * d + 4 * v);
    const float4 m = row_drop_mult(dr, r, d, v);
    {
#pragma clang fp contract(off)    // product, sum and mask rounded one by one: torch's items * sqrt(d) + places, bit for bit
      const float4 s = make_float4(a.x * scale, a.y * scale, a.z * scale, a.w * scale);
      const float4 e = make_float4(s.x + b.x, s.y + b.y, s.z + b.z, s.w + b.w);
      o = make_float4(e.x * m.x, e.y * m.y, e.z * m.z, e.w * m.w);
    }
  }
  *reinterpret_cast<float4*>(out + r * d + 4 * v) = o;
}

// One problem of srh_rows_live_sum_f32 as the kernels read it.
struct LiveSumTask {
  const float* x;
  const int32_t *rows, *chunk_start, *chunk_dst, *multi_range, *multi_row;
  float* out;
  float* part;          // n_chunk x d partial sums (multi-chunk segments only)
  int64_t n_x, n_live, n_chunk, n_multi, n_table;
  float scale;
  RowDrop dr;
};
struct LiveSumBatch {
  LiveSumTask t[SRH_LIVE_SUM_MAX_PROBLEMS];
  int64_t chunk_end[SRH_LIVE_SUM_MAX_PROBLEMS];   // running totals of n_chunk / n_multi: group g -> (problem, local index)
  int64_t multi_end[SRH_LIVE_SUM_MAX_PROBLEMS];
  int count;
  int d;
};

__device__ __forceinline__ float4 f4_fma_mask(const float4 x, const float4 m, const float4 acc) {
  return make_float4(fmaf(x.x, m.x, acc.x), fmaf(x.y, m.y, acc.y), fmaf(x.z, m.z, acc.z), fmaf(x.w, m.w, acc.w));
}

// launch 1: one group of d / 4 lanes per chunk sums the chunk's rows of x (times their dropout multiplier) in plan order.
// The only chunk of a segment writes scale * sum to its table row; a chunk of a longer segment leaves its sum in part[].
__global__ __launch_bounds__(256) void live_sum_chunks(const LiveSumBatch b) {
  const int d = b.d, lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t g = t / lpr;
  const int v = (int)(t % lpr);
  int k = 0;
  while (k < b.count && g >= b.chunk_end[k]) ++k;
  if (k >= b.count) return;
  if (k > 0) g -= b.chunk_end[k - 1];
  const LiveSumTask& w = b.t[k];
  int64_t p0 = w.chunk_start[g], p1 = w.chunk_start[g + 1];
  p0 = p0 < 0 ? 0 : p0;
  p1 = p1 > w.n_live ? w.n_live : p1;
  float4 acc = f4_zero();
  int64_t p = p0;
  // four rows in flight: their ids, then their loads, then the adds in plan order
  for (; p + 4 <= p1; p += 4) {
    int64_t r[4];
    float4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = w.rows[p + u];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      x[u] = (r[u] >= 0 && r[u] < w.n_x) ? *reinterpret_cast<const float4*>(w.x + r[u] * d + 4 * v) : f4_zero();
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r[u] >= 0 && r[u] < w.n_x) acc = f4_fma_mask(x[u], row_drop_mult(w.dr, r[u], d, v), acc);
  }
  for (; p < p1; ++p) {
    const int64_t r = w.rows[p];
    if (r >= 0 && r < w.n_x)
      acc = f4_fma_mask(*reinterpret_cast<const float4*>(w.x + r * d + 4 * v), row_drop_mult(w.dr, r, d, v), acc);
  }
  const int64_t dst = w.chunk_dst[g];
  if (dst >= 0) {
    if (dst < w.n_table)
      *reinterpret_cast<float4*>(w.out + dst * d + 4 * v) =
          make_float4(w.scale * acc.x, w.scale * acc.y, w.scale * acc.z, w.scale * acc.w);
  } else if (w.part) {
    *reinterpret_cast<float4*>(w.part + g * d + 4 * v) = acc;
  }
}

// launch 2: one group per multi-chunk segment adds its partials in chunk order
__global__ __launch_bounds__(256) void live_sum_finish(const LiveSumBatch b) {
  const int d = b.d, lpr = d >> 2;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t g = t / lpr;
  const int v = (int)(t % lpr);
  int k = 0;
  while (k < b.count && g >= b.multi_end[k]) ++k;
  if (k >= b.count) return;
  if (k > 0) g -= b.multi_end[k - 1];
  const LiveSumTask& w = b.t[k];
  int64_t c0 = w.multi_range[2 * g], c1 = w.multi_range[2 * g + 1];
  c0 = c0 < 0 ? 0 : c0;
  c1 = c1 > w.n_chunk ? w.n_chunk : c1;
  float4 acc = f4_zero();
  for (int64_t c = c0; c < c1; ++c) {
    const float4 x = *reinterpret_cast<const float4*>(w.part + c * d + 4 * v);
    acc = make_float4(acc.x + x.x, acc.y + x.y, acc.z + x.z, acc.w + x.w);
  }
  const int64_t dst = w.multi_row[g];
  if (dst >= 0 && dst < w.n_table)
    *reinterpret_cast<float4*>(w.out + dst * d + 4 * v) =
        make_float4(w.scale * acc.x, w.scale * acc.y, w.scale * acc.z, w.scale * acc.w);
}

template <bool CAUSAL>
srh_status_t attn_fwd_launch(const char* what, const float* d_q, const float* d_k, const float* d_v, int64_t B, int32_t L,
                             int32_t H, int32_t dh, const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter,
                             float drop_p, float* d_out, float* d_lse, void* stream) {
  SRH_REQUIRE(d_q && d_k && d_v && d_out && d_lse, "%s: null argument", what);
  AttnArgs a{};
  const srh_status_t s = attn_check(what, B, L, H, dh, d_keep, drop_p, a);
  if (s != SRH_OK) return s;
  a.q = d_q; a.k = d_k; a.v = d_v; a.out = d_out; a.lse = d_lse;
  a.seed_lo = (uint32_t)rng_seed; a.seed_hi = (uint32_t)(rng_seed >> 32); a.ctr = rng_counter;
  const unsigned grid = (unsigned)(B * H);
  if (dh == 64) attn_fwd<64, CAUSAL><<<grid, 256, 0, as_stream(stream)>>>(a);
  else attn_fwd<32, CAUSAL><<<grid, 256, 0, as_stream(stream)>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

template <bool CAUSAL>
srh_status_t attn_bwd_launch(const char* what, const float* d_q, const float* d_k, const float* d_v, const float* d_go,
                             const float* d_lse, int64_t B, int32_t L, int32_t H, int32_t dh, const uint8_t* d_keep,
                             uint64_t rng_seed, uint64_t rng_counter, float drop_p, float* d_gq, float* d_gk, float* d_gv,
                             void* stream) {
  SRH_REQUIRE(d_q && d_k && d_v && d_go && d_lse && d_gq && d_gk && d_gv, "%s: null argument", what);
  AttnArgs a{};
  const srh_status_t s = attn_check(what, B, L, H, dh, d_keep, drop_p, a);
  if (s != SRH_OK) return s;
  a.q = d_q; a.k = d_k; a.v = d_v; a.go = d_go; a.lse_in = d_lse; a.gq = d_gq; a.gk = d_gk; a.gv = d_gv;
  a.seed_lo = (uint32_t)rng_seed; a.seed_hi = (uint32_t)(rng_seed >> 32); a.ctr = rng_counter;
  const unsigned grid = (unsigned)(B * H);
  if (dh == 64) attn_bwd<64, CAUSAL><<<grid, 256, 0, as_stream(stream)>>>(a);
  else attn_bwd<32, CAUSAL><<<grid, 256, 0, as_stream(stream)>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

// the checks and the grid of a tiled call: one workgroup per (sequence, head, 64-row block)
srh_status_t attn_tiled_check(const char* what, int64_t B, int32_t L, int32_t H, int32_t dh, const uint8_t* d_keep,
                              uint64_t rng_seed, uint64_t rng_counter, float drop_p, AttnArgs& a, unsigned& grid) {
  const srh_status_t s = attn_check(what, B, L, H, dh, d_keep, drop_p, a, kTiledMaxL);
  if (s != SRH_OK) return s;
  const int64_t blocks = B * H * ((L + kMaxL - 1) / kMaxL);
  SRH_SUPPORTED(blocks < (int64_t(1) << 31), "%s: too many sequences", what);
  a.seed_lo = (uint32_t)rng_seed; a.seed_hi = (uint32_t)(rng_seed >> 32); a.ctr = rng_counter;
  grid = (unsigned)blocks;
  return SRH_OK;
}

template <bool CAUSAL>
void attn_tiled_fwd_launch(const AttnArgs& a, int32_t dh, unsigned grid, hipStream_t st) {
  if (dh == 64) attn_tiled_fwd<64, CAUSAL><<<grid, 256, 0, st>>>(a);
  else attn_tiled_fwd<32, CAUSAL><<<grid, 256, 0, st>>>(a);
}

template <bool CAUSAL>
srh_status_t attn_tiled_bwd_launch(const AttnArgs& a, int32_t dh, unsigned grid, hipStream_t st) {
  if (dh == 64) attn_tiled_bwd_q<64, CAUSAL><<<grid, 256, 0, st>>>(a);
  else attn_tiled_bwd_q<32, CAUSAL><<<grid, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  if (dh == 64) attn_tiled_bwd_kv<64, CAUSAL><<<grid, 256, 0, st>>>(a);
  else attn_tiled_bwd_kv<32, CAUSAL><<<grid, 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // namespace

extern "C" {

srh_status_t srh_seq_attn_tiled_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t B, int32_t L,
                                        int32_t H, int32_t dh, int32_t causal, const uint8_t* d_keep, uint64_t rng_seed,
                                        uint64_t rng_counter, float drop_p, float* d_out, float* d_lse, void* stream) {
  SRH_REQUIRE(d_q && d_k && d_v && d_out && d_lse, "seq_attn_tiled_fwd: null argument");
  AttnArgs a{};
  unsigned grid = 0;
  const srh_status_t s = attn_tiled_check("seq_attn_tiled_fwd", B, L, H, dh, d_keep, rng_seed, rng_counter, drop_p, a, grid);
  if (s != SRH_OK) return s;
  a.q = d_q; a.k = d_k; a.v = d_v; a.out = d_out; a.lse = d_lse;
  if (causal) attn_tiled_fwd_launch<true>(a, dh, grid, as_stream(stream));
  else attn_tiled_fwd_launch<false>(a, dh, grid, as_stream(stream));
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

srh_status_t srh_seq_attn_tiled_bwd_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_out,
                                        const float* d_go, const float* d_lse, int64_t B, int32_t L, int32_t H, int32_t dh,
                                        int32_t causal, const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter,
                                        float drop_p, float* d_gq, float* d_gk, float* d_gv, void* stream) {
  SRH_REQUIRE(d_q && d_k && d_v && d_out && d_go && d_lse && d_gq && d_gk && d_gv, "seq_attn_tiled_bwd: null argument");
  AttnArgs a{};
  unsigned grid = 0;
  const srh_status_t s = attn_tiled_check("seq_attn_tiled_bwd", B, L, H, dh, d_keep, rng_seed, rng_counter, drop_p, a, grid);
  if (s != SRH_OK) return s;
  a.q = d_q; a.k = d_k; a.v = d_v; a.out_in = d_out; a.go = d_go; a.lse_in = d_lse; a.gq = d_gq; a.gk = d_gk; a.gv = d_gv;
  return causal ? attn_tiled_bwd_launch<true>(a, dh, grid, as_stream(stream))
                : attn_tiled_bwd_launch<false>(a, dh, grid, as_stream(stream));
}

srh_status_t srh_seq_attn_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t B, int32_t L, int32_t H,
                                  int32_t dh, const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter, float drop_p,
                                  float* d_out, float* d_lse, void* stream) {
  return attn_fwd_launch<true>("seq_attn_fwd", d_q, d_k, d_v, B, L, H, dh, d_keep, rng_seed, rng_counter, drop_p, d_out,
                               d_lse, stream);
}

srh_status_t srh_seq_attn_bwd_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_go,
                                  const float* d_lse, int64_t B, int32_t L, int32_t H, int32_t dh, const uint8_t* d_keep,
                                  uint64_t rng_seed, uint64_t rng_counter, float drop_p, float* d_gq, float* d_gk,
                                  float* d_gv, void* stream) {
  return attn_bwd_launch<true>("seq_attn_bwd", d_q, d_k, d_v, d_go, d_lse, B, L, H, dh, d_keep, rng_seed, rng_counter,
                               drop_p, d_gq, d_gk, d_gv, stream);
}

srh_status_t srh_seq_attn_full_fwd_f32(const float* d_q, const float* d_k, const float* d_v, int64_t B, int32_t L,
                                       int32_t H, int32_t dh, const uint8_t* d_keep, uint64_t rng_seed,
                                       uint64_t rng_counter, float drop_p, float* d_out, float* d_lse, void* stream) {
  return attn_fwd_launch<false>("seq_attn_full_fwd", d_q, d_k, d_v, B, L, H, dh, d_keep, rng_seed, rng_counter, drop_p,
                                d_out, d_lse, stream);
}

srh_status_t srh_seq_attn_full_bwd_f32(const float* d_q, const float* d_k, const float* d_v, const float* d_go,
                                       const float* d_lse, int64_t B, int32_t L, int32_t H, int32_t dh,
                                       const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter, float drop_p,
                                       float* d_gq, float* d_gk, float* d_gv, void* stream) {
  return attn_bwd_launch<false>("seq_attn_full_bwd", d_q, d_k, d_v, d_go, d_lse, B, L, H, dh, d_keep, rng_seed,
                                rng_counter, drop_p, d_gq, d_gk, d_gv, stream);
}

int64_t srh_seq_bce_ws_bytes(int64_t R) { return R > 0 ? align256(16 * R) : 0; }

srh_status_t srh_seq_bce_fwd_bwd(const float* d_hidden, int64_t R, int32_t d, const float* d_table, int64_t n_table,
                                 const int32_t* d_pos, const int32_t* d_neg, const uint8_t* d_valid, int64_t n_valid,
                                 double* d_loss2, float* d_gh, float* d_grows, void* d_ws, void* stream) {
  SRH_REQUIRE(d_hidden && d_table && d_pos && d_neg && d_valid && d_loss2 && d_gh && d_grows && d_ws,
              "seq_bce: null argument");
  SRH_REQUIRE(R > 0 && R < (int64_t(1) << 30) && d > 0 && d <= 1024 && n_table > 0, "seq_bce: bad sizes");
  SRH_REQUIRE(n_valid > 0 && n_valid <= R, "seq_bce: n_valid=%lld must be in [1, R]", (long long)n_valid);
  hipStream_t st = as_stream(stream);
  double* terms = static_cast<double*>(d_ws);
  const double inv_n = 1.0 / (double)n_valid;
  bce_rows<<<(unsigned)((R + 3) / 4), 256, 0, st>>>(d_hidden, R, d, d_table, n_table, d_pos, d_neg, d_valid, inv_n, terms,
                                                     d_gh, d_grows);
  SRH_LAUNCH_CHECK();
  bce_reduce<<<1, 256, 0, st>>>(terms, R, inv_n, d_loss2);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

srh_status_t srh_seq_embed_fwd_f32(const float* d_item, int64_t n_item, const float* d_pos, int64_t n_pos,
                                   const int32_t* d_seq, const int32_t* d_posid, int64_t R, int32_t d, float scale,
                                   const uint8_t* d_keep, uint64_t rng_seed, uint64_t rng_counter, float drop_p,
                                   float* d_out, void* stream) {
  SRH_REQUIRE(d_item && d_pos && d_seq && d_posid && d_out, "seq_embed_fwd: null argument");
  SRH_REQUIRE(R >= 1 && R < (int64_t(1) << 31) && n_item >= 1 && n_pos >= 1, "seq_embed_fwd: bad sizes");
  SRH_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "seq_embed_fwd: drop probability must be in [0, 1)");
  SRH_SUPPORTED(d == 32 || d == 64 || d == 128, "seq_embed_fwd: width %d -- the kernel serves 32, 64 and 128", d);
  const RowDrop dr = make_row_drop(d_keep, rng_seed, rng_counter, drop_p);
  const int64_t threads = R * (d / 4);
  seq_embed_rows<<<(unsigned)((threads + 255) / 256), 256, 0, as_stream(stream)>>>(d_item, n_item, d_pos, n_pos, d_seq,
                                                                                    d_posid, R, d, scale, dr, d_out);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_rows_live_sum_ws_bytes(const srh_live_sum_problem_t* problems, int32_t n_problems, int32_t d) {
  int64_t need = 0;
  for (int k = 0; problems && k < n_problems; ++k)
    if (problems[k].n_multi > 0) need += align256(problems[k].n_chunk * d * (int64_t)sizeof(float));
  return need;
}

srh_status_t srh_rows_live_sum_f32(const srh_live_sum_problem_t* problems, int32_t n_problems, int32_t d, void* d_ws,
                                   void* stream) {
  SRH_REQUIRE(problems && n_problems >= 1 && n_problems <= SRH_LIVE_SUM_MAX_PROBLEMS,
              "rows_live_sum: 1..%d problems per call", SRH_LIVE_SUM_MAX_PROBLEMS);
  SRH_SUPPORTED(d == 32 || d == 64 || d == 128, "rows_live_sum: width %d -- the kernel serves 32, 64 and 128", d);
  LiveSumBatch b{};
  b.d = d;
  char* cursor = static_cast<char*>(d_ws);
  int64_t chunks = 0, multis = 0;
  for (int k = 0; k < n_problems; ++k) {
    const srh_live_sum_problem_t& p = problems[k];
    SRH_REQUIRE(p.n_rows >= 1 && p.n_rows < (int64_t(1) << 31) && p.n_table >= 1 && p.n_live >= 0 && p.n_live <= p.n_rows &&
                    p.n_chunk >= 0 && p.n_chunk <= p.n_live && p.n_multi >= 0 && 2 * p.n_multi <= p.n_chunk,
                "rows_live_sum: problem %d: bad sizes", k);
    SRH_REQUIRE(p.drop_p >= 0.f && p.drop_p < 1.f, "rows_live_sum: drop probability must be in [0, 1)");
    SRH_REQUIRE(p.n_chunk == 0 || (p.d_x && p.d_rows && p.d_chunk_start && p.d_chunk_dst && p.d_out),
                "rows_live_sum: problem %d: null argument", k);
    SRH_REQUIRE(p.n_multi == 0 || (p.d_multi_range && p.d_multi_row && d_ws),
                "rows_live_sum: problem %d: multi-chunk segments without their lists or a workspace", k);
    LiveSumTask& w = b.t[k];
    w.x = p.d_x; w.rows = p.d_rows; w.chunk_start = p.d_chunk_start; w.chunk_dst = p.d_chunk_dst;
    w.multi_range = p.d_multi_range; w.multi_row = p.d_multi_row; w.out = p.d_out;
    w.n_x = p.n_rows; w.n_live = p.n_live; w.n_chunk = p.n_chunk; w.n_multi = p.n_multi; w.n_table = p.n_table;
    w.scale = p.scale;
    w.dr = make_row_drop(p.d_keep, p.rng_seed, p.rng_counter, p.drop_p);
    w.part = nullptr;
    if (p.n_multi > 0) {
      w.part = reinterpret_cast<float*>(cursor);
      cursor += align256(p.n_chunk * d * (int64_t)sizeof(float));
    }
    chunks += p.n_chunk; multis += p.n_multi;
    b.chunk_end[k] = chunks; b.multi_end[k] = multis;
  }
  b.count = n_problems;
  hipStream_t st = as_stream(stream);
  const int lpr = d / 4;
  if (chunks > 0) {
    live_sum_chunks<<<(unsigned)((chunks * lpr + 255) / 256), 256, 0, st>>>(b);
    SRH_LAUNCH_CHECK();
  }
  if (multis > 0) {
    live_sum_finish<<<(unsigned)((multis * lpr + 255) / 256), 256, 0, st>>>(b);
    SRH_LAUNCH_CHECK();
  }
  return SRH_OK;
}

}  // extern "C"

// SSL4Rec (reference model/graph/SSL4Rec.py): the two MLP towers.  DESIGN.md 4.8.
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
//                       dW2 = dZ2^T H, dW1 = dZ1^T X, db2 / db1 the column sums.  The products run on the strided MFMA
//                       GEMM of chunked.hip; the reductions over rows are cut into fixed chunks of kRowChunk rows whose
//                       partials are summed in chunk order (chunked.hip): no float atomics, the same bits on every call.
//   srh_rows_segment_sum_f32  the deterministic scatter of dX into the embedding-table gradient: rows grouped by the
//                       host's stable sort of the ids, each table row sums its rows in that order.
//
// batch_softmax_loss (srh_batch_softmax_fwd_bwd) is the shared two-pass kernel of contrastive.hip.
#include <algorithm>

#include "rowtile.h"

namespace {

using namespace srh;

constexpr int kIn = 64, kHid = 1024, kOut = 128;
constexpr int kHc = 64;                 // hidden units per chunk of the forward walk
constexpr int kLds = kHc + 4;           // LDS row stride (floats) of the staged chunk
constexpr int kRowChunk = 256;          // rows per partial of the weight-gradient reductions

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
// dZ2 = dY (1 - Y^2) (torch's tanh_backward)
__global__ __launch_bounds__(256) void tw_tanh_bwd(const float* __restrict__ gy, const float* __restrict__ y, int64_t len,
                                                   float* __restrict__ dz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < len) dz[i] = gy[i] * (1.f - y[i] * y[i]);
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

struct BwdWs {
  float* dz2;     // n x 128
  float* dz1;     // n x 1024
  float* part_w;  // chunks x (1024 x 64 + 128 x 1024)  (dW1 partials, then dW2 partials)
  float* part_b;  // chunks x (1024 + 128)
};

// null ws measures, a workspace carves; returns the bytes
int64_t bwd_layout(BwdWs& w, void* ws, int64_t n) {
  Carver cv(ws);
  const int64_t c = ceil_div(n, kRowChunk);
  cv.take(w.dz2, n * kOut);
  cv.take(w.dz1, n * kHid);
  cv.take(w.part_w, c * (kHid * kIn + kOut * kHid));
  cv.take(w.part_b, c * (kHid + kOut));
  return cv.used;
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
  BwdWs w;
  return bwd_layout(w, nullptr, n);
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
  BwdWs ws;
  bwd_layout(ws, d_ws, n);
  const int64_t chunks = ceil_div(n, kRowChunk);
  srh_status_t s;
  // dZ2
  tw_tanh_bwd<<<(unsigned)((n * kOut + 255) / 256), 256, 0, st>>>(d_gy, d_y, n * kOut, ws.dz2);
  SRH_LAUNCH_CHECK();
  // dZ1 = (dZ2 W2) [H > 0]         (n x 128) (128 x 1024)
  GemmArgs g{};
  g.A = ws.dz2; g.sam = kOut; g.sak = 1; g.B = w->d_w2; g.sbk = kHid; g.sbn = 1; g.C = ws.dz1; g.ldc = kHid; g.M = n; g.N = kHid; g.K = kOut; g.kchunk = kOut;
  g.aux = d_hidden;
  if ((s = gemm64(g, EPI_RELU, 1, st)) != SRH_OK) return s;
  // dX = (dZ1 W1) m                (n x 1024) (1024 x 64)
  g = GemmArgs{};
  g.A = ws.dz1; g.sam = kHid; g.sak = 1; g.B = w->d_w1; g.sbk = kIn; g.sbn = 1; g.C = d_gx; g.ldc = kIn;
  g.M = n; g.N = kIn; g.K = kHid; g.kchunk = kHid;
  g.mask = d_mask; g.mask_row0 = d_mask ? mask_row0 : n; g.mask_scale = 1.f / (1.f - drop_p);
  if ((s = gemm64(g, d_mask ? EPI_MASK : EPI_STORE, 1, st)) != SRH_OK) return s;
  // dW1 partials = dZ1^T X per chunk of rows     (1024 x n) (n x 64)
  float* part_w1 = ws.part_w;
  float* part_w2 = ws.part_w + chunks * kHid * kIn;
  g = GemmArgs{};
  g.A = ws.dz1; g.sam = 1; g.sak = kHid; g.B = d_x; g.sbk = kIn; g.sbn = 1; g.C = part_w1; g.ldc = kIn;
  g.c_zstride = kHid * kIn; g.M = kHid; g.N = kIn; g.K = n; g.kchunk = kRowChunk;
  if ((s = gemm64(g, EPI_STORE, chunks, st)) != SRH_OK) return s;
  // dW2 partials = dZ2^T H per chunk of rows     (128 x n) (n x 1024)
  g = GemmArgs{};
  g.A = ws.dz2; g.sam = 1; g.sak = kOut; g.B = d_hidden; g.sbk = kHid; g.sbn = 1; g.C = part_w2; g.ldc = kHid;
  g.c_zstride = kOut * kHid; g.M = kOut; g.N = kHid; g.K = n; g.kchunk = kRowChunk;
  if ((s = gemm64(g, EPI_STORE, chunks, st)) != SRH_OK) return s;
  // bias partials
  float* part_b1 = ws.part_b;
  float* part_b2 = ws.part_b + chunks * kHid;
  if ((s = colsum_chunks(ws.dz1, n, kHid, 1, kRowChunk, part_b1, st)) != SRH_OK) return s;
  if ((s = colsum_chunks(ws.dz2, n, kOut, 1, kRowChunk, part_b2, st)) != SRH_OK) return s;
  // the partials in chunk order
  if ((s = reduce_chunks(part_w1, chunks, kHid * kIn, 1.f, d_gw1, st)) != SRH_OK) return s;
  if ((s = reduce_chunks(part_w2, chunks, kOut * kHid, 1.f, d_gw2, st)) != SRH_OK) return s;
  if ((s = reduce_chunks(part_b1, chunks, kHid, 1.f, d_gb1, st)) != SRH_OK) return s;
  return reduce_chunks(part_b2, chunks, kOut, 1.f, d_gb2, st);
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

}  // extern "C"

// MixGCF's hop mixing (negative_mixup, model/graph/MixGCF.py:96-114 of the reference).  DESIGN.md 4.22.
// Per (pair b, hop k): the C candidates T_k[neg[b C + c]] are mixed with the positive T_k[pos[b]] by a per-element alpha,
// scored against the user row, and only the hardest one survives; the survivors and the positives are averaged over hops.
// All arithmetic fp32, no float atomics, nothing waits on the host.
//
// Forward   one workgroup per pair, one wave per hop (64 H threads).  A lane holds one float4 of a row, G = the power of
//           two >= d / 4 lanes hold a row (lanes at or past d / 4 of a group hold zeros), so a wave scores 64 / G
//           candidates per iteration with a log2(G)-step reduction; kInFlight iterations are loaded before the first is
//           used and the next batch's indices are fetched under the current batch's arithmetic.  The best candidate's mixed
//           float4 stays in registers; the lane groups are merged at the end (higher score, then lower c).  The waves leave
//           their winner and their positive in LDS and wave 0 sums them in hop order.
// Backward  mixup_keys writes key[k][2 b + s] = the item row entry (pair b, s = 0 its positive, s = 1 its picked
//           candidate) adds to, or -1.  mixup_scatter runs one wave per entry: a wave whose key occurs EARLIER in its hop
//           leaves; the first one (the row's leader) walks the later entries of the same key in ascending order and
//           stores the row once -- ascending b, positive before negative, one writer per row.  The scan is over the hop's
//           2 B keys (16 KB at B = 2048: L2 resident), so the pass is quadratic in B; see DESIGN.md 4.22 for where a sort
//           would take over.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

using namespace srh;

constexpr int kInFlight = 4;            // iterations (of 64 / G candidates) whose loads are issued before the first use
constexpr int kScanUnroll = 4;          // 64-key strides of the leader test between two early-exit votes

struct MixupArgs {
  const float* table[SRH_MIXUP_MAX_HOPS];
  const float* alpha[SRH_MIXUP_MAX_HOPS];     // all NULL: drawn
  float* grad[SRH_MIXUP_MAX_HOPS];
  const float* u;
  const int32_t* pos;
  const int32_t* neg;
  int64_t I, B;
  int H, C, d;
  uint64_t ctr;
  uint32_t seed_lo, seed_hi;
  float *pos_out, *neg_out;
  int32_t* pick;            // H x B (forward: written, backward: read)
  const float *g_pos, *g_neg;
  int32_t* key;             // backward workspace: H x 2 B
};

__device__ __forceinline__ bool in_table(int32_t i, int64_t I) { return (uint32_t)i < (uint32_t)I; }

// alpha of float4 q of row (k, b, c): injected, or the counter RNG at rng_counter + (k B + b) C + c, sub = q
__device__ __forceinline__ float4 alpha_of(const MixupArgs& a, int k, int64_t b, int c, int q) {
  const float* inj = a.alpha[k];
  if (inj) return reinterpret_cast<const float4*>(inj + ((size_t)b * a.C + c) * a.d)[q];
  const uint64_t row = ((uint64_t)k * (uint64_t)a.B + (uint64_t)b) * (uint64_t)a.C + (uint64_t)c;
  const uint4 w = counter_rng4(a.ctr + row, (uint32_t)q, a.seed_lo, a.seed_hi);
  return make_float4(u01(w.x), u01(w.y), u01(w.z), u01(w.w));
}

// m = alpha p + (1 - alpha) n, the one rounding order of the file
__device__ __forceinline__ float mix1(float al, float p, float n) { return fmaf(al, p, (1.f - al) * n); }
__device__ __forceinline__ float4 mix4(float4 al, float4 p, float4 n) {
  return make_float4(mix1(al.x, p.x, n.x), mix1(al.y, p.y, n.y), mix1(al.z, p.z, n.z), mix1(al.w, p.w, n.w));
}

// does candidate (s, c) beat (bs, bc)?  Higher score, an exact tie to the lower c; bc == INT_MAX: nothing held yet
__device__ __forceinline__ bool beats(float s, int c, float bs, int bc) {
  return bc == INT_MAX || s > bs || (s == bs && c < bc);
}

template <int G>
__global__ __launch_bounds__(64 * SRH_MIXUP_MAX_HOPS) void mixup_fwd_kernel(const MixupArgs a) {
  constexpr int CPI = 64 / G;                       // candidates per iteration
  __shared__ float4 s_neg[SRH_MIXUP_MAX_HOPS][64];
  __shared__ float4 s_pos[SRH_MIXUP_MAX_HOPS][64];
  const int64_t b = blockIdx.x;
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane / G, q = lane % G;
  const int nq = a.d >> 2;
  const bool live = q < nq;                          // this lane holds a float4 of the row
  const float4* tab = reinterpret_cast<const float4*>(a.table[k]);

  const int32_t pi = a.pos[b];
  float4 p = f4_zero(), uu = f4_zero();
  if (live) {
    uu = reinterpret_cast<const float4*>(a.u)[(size_t)b * nq + q];
    if (in_table(pi, a.I)) p = tab[(size_t)pi * nq + q];
  }

  float best_s = -INFINITY;
  int best_c = INT_MAX;
  float4 best_m = f4_zero();

  const int32_t* negs = a.neg + (size_t)b * a.C;
  constexpr int STEP = CPI * kInFlight;
  int32_t idx[kInFlight], idx_next[kInFlight];
#pragma unroll
  for (int t = 0; t < kInFlight; ++t) {
    const int c = t * CPI + g;
    idx[t] = c < a.C ? negs[c] : -1;
  }
  for (int c0 = 0; c0 < a.C; c0 += STEP) {
    float4 n[kInFlight], al[kInFlight];
#pragma unroll
    for (int t = 0; t < kInFlight; ++t) {            // every load of the batch before its first use
      const int c = c0 + t * CPI + g;
      n[t] = f4_zero();
      al[t] = f4_zero();
      if (live && c < a.C) {
        if (in_table(idx[t], a.I)) n[t] = tab[(size_t)idx[t] * nq + q];
        al[t] = alpha_of(a, k, b, c, q);
      }
    }
#pragma unroll
    for (int t = 0; t < kInFlight; ++t) {            // the next batch's indices, under this batch's arithmetic
      const int c = c0 + STEP + t * CPI + g;
      idx_next[t] = c < a.C ? negs[c] : -1;
    }
#pragma unroll
    for (int t = 0; t < kInFlight; ++t) {
      const int c = c0 + t * CPI + g;
      const float4 m = mix4(al[t], p, n[t]);
      float s = group_sum<G>(f4_dot(uu, m));
      if (!in_table(idx[t], a.I)) s = -INFINITY;     // an index outside the table is never read and never wins a score
      if (c < a.C && beats(s, c, best_s, best_c)) { best_s = s; best_c = c; best_m = m; }
    }
#pragma unroll
    for (int t = 0; t < kInFlight; ++t) idx[t] = idx_next[t];
  }
  // merge the lane groups: after the last step every group holds the wave's winner
#pragma unroll
  for (int mask = G; mask < 64; mask <<= 1) {
    const float os = __shfl_xor(best_s, mask);
    const int oc = __shfl_xor(best_c, mask);
    const float4 om = f4_shfl_xor(best_m, mask);
    if (oc != INT_MAX && beats(os, oc, best_s, best_c)) { best_s = os; best_c = oc; best_m = om; }
  }
  if (lane == 0) a.pick[(size_t)k * a.B + b] = best_c;        // C >= 1: some group took candidate 0
  if (lane < G) {
    s_neg[k][lane] = best_m;
    s_pos[k][lane] = p;
  }
  __syncthreads();
  if (k == 0 && live && g == 0) {                   // hop order, then one division
    float4 sn = s_neg[0][q], sp = s_pos[0][q];
    for (int h = 1; h < a.H; ++h) {
      sn = f4_add(sn, s_neg[h][q]);
      sp = f4_add(sp, s_pos[h][q]);
    }
    const float hf = (float)a.H;
    reinterpret_cast<float4*>(a.neg_out)[(size_t)b * nq + q] = make_float4(sn.x / hf, sn.y / hf, sn.z / hf, sn.w / hf);
    reinterpret_cast<float4*>(a.pos_out)[(size_t)b * nq + q] = make_float4(sp.x / hf, sp.y / hf, sp.z / hf, sp.w / hf);
  }
}

// key[k][2 b] = pos[b], key[k][2 b + 1] = neg[b C + pick[k][b]]; -1 where the index (or the pick) is out of range
__global__ __launch_bounds__(256) void mixup_keys(const MixupArgs a) {
  const int64_t n = 2 * a.B, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * a.H) return;
  const int k = (int)(i / n);
  const int64_t e = i % n, b = e >> 1;
  int32_t item = -1;
  if ((e & 1) == 0) {
    item = a.pos[b];
  } else {
    const int32_t c = a.pick[(size_t)k * a.B + b];
    if ((uint32_t)c < (uint32_t)a.C) item = a.neg[(size_t)b * a.C + c];
  }
  a.key[i] = in_table(item, a.I) ? item : -1;
}

// what entry e of hop k adds to its row, float4 q:  positive (g_pos + alpha* g_neg) / H, negative ((1 - alpha*) g_neg) / H
__device__ __forceinline__ float4 mixup_share(const MixupArgs& a, int k, int64_t e, int q, int nq) {
  const int64_t b = e >> 1;
  const bool is_pos = (e & 1) == 0;
  float4 gn = f4_zero(), gp = f4_zero(), al = f4_zero();
  if (a.g_neg) {
    gn = reinterpret_cast<const float4*>(a.g_neg)[(size_t)b * nq + q];
    const int32_t c = a.pick[(size_t)k * a.B + b];
    if ((uint32_t)c < (uint32_t)a.C) al = alpha_of(a, k, b, c, q);       // (a pick outside [0, C) reads no alpha)
  }
  if (is_pos && a.g_pos) gp = reinterpret_cast<const float4*>(a.g_pos)[(size_t)b * nq + q];
  const float hf = (float)a.H;
  if (is_pos)
    return make_float4(fmaf(al.x, gn.x, gp.x) / hf, fmaf(al.y, gn.y, gp.y) / hf, fmaf(al.z, gn.z, gp.z) / hf,
                       fmaf(al.w, gn.w, gp.w) / hf);
  return make_float4(((1.f - al.x) * gn.x) / hf, ((1.f - al.y) * gn.y) / hf, ((1.f - al.z) * gn.z) / hf,
                     ((1.f - al.w) * gn.w) / hf);
}

__global__ __launch_bounds__(256) void mixup_scatter(const MixupArgs a) {
  const int64_t n = 2 * a.B, w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n * a.H) return;                          // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int k = (int)(w / n);
  const int64_t e = w % n;
  const int32_t* key = a.key + (size_t)k * n;
  const int32_t mine = key[e];
  if (mine < 0) return;
  // leader test: does the key occur before e?
  for (int64_t j0 = 0; j0 < e; j0 += 64 * kScanUnroll) {
    bool seen = false;
#pragma unroll
    for (int t = 0; t < kScanUnroll; ++t) {
      const int64_t j = j0 + t * 64 + lane;
      seen |= (j < e) && key[j] == mine;
    }
    if (__any(seen)) return;
  }
  const int nq = a.d >> 2;
  const bool live = lane < nq;
  float4 acc = live ? mixup_share(a, k, e, lane, nq) : f4_zero();
  for (int64_t j0 = e + 1; j0 < n; j0 += 64) {       // the later entries of the row, ascending
    const int64_t j = j0 + lane;
    unsigned long long hits = __ballot(j < n && key[j] == mine);
    while (hits) {
      const int t = __ffsll((long long)hits) - 1;
      hits &= hits - 1;
      if (live) acc = f4_add(acc, mixup_share(a, k, j0 + t, lane, nq));
    }
  }
  if (live) reinterpret_cast<float4*>(a.grad[k])[(size_t)mine * nq + lane] = acc;
}

inline int group_width(int d) {
  int g = 1;
  while (g * 4 < d) g <<= 1;
  return g;
}

inline bool shape_served(int64_t d, int64_t H, int64_t C) {
  return d >= 4 && d <= 256 && d % 4 == 0 && H >= 1 && H <= SRH_MIXUP_MAX_HOPS && C >= 1;
}

// the checks both entry points share; fills the kernels' arguments
srh_status_t mixup_args(const srh_mixup_args_t* in, const char* what, MixupArgs& a) {
  SRH_REQUIRE(in, "%s: null argument", what);
  const srh_mixup_args_t& s = *in;
  SRH_SUPPORTED(s.d >= 4 && s.d <= 256 && s.d % 4 == 0, "%s: d=%d unsupported (a multiple of 4 in 4..256)", what, s.d);
  SRH_SUPPORTED(s.n_hops >= 1 && s.n_hops <= SRH_MIXUP_MAX_HOPS, "%s: %d hops unsupported (1..%d)", what, s.n_hops,
                SRH_MIXUP_MAX_HOPS);
  SRH_SUPPORTED(s.n_negs >= 1, "%s: n_negs=%d unsupported (>= 1)", what, s.n_negs);
  SRH_REQUIRE(s.n_items >= 0 && s.n_items < (int64_t(1) << 31), "%s: bad n_items", what);
  SRH_REQUIRE(s.B >= 0 && s.B * s.n_hops < (int64_t(1) << 28) && s.B * (int64_t)s.n_negs < (int64_t(1) << 40),
              "%s: bad B", what);
  a = MixupArgs{};
  int injected = 0;
  for (int k = 0; k < s.n_hops; ++k) {
    a.table[k] = s.d_table[k];
    a.alpha[k] = s.d_alpha[k];
    a.grad[k] = s.d_grad[k];
    injected += s.d_alpha[k] != nullptr;
  }
  SRH_REQUIRE(injected == 0 || injected == s.n_hops, "%s: alpha is injected for every hop or for none", what);
  a.pos = s.d_pos; a.neg = s.d_neg; a.I = s.n_items; a.B = s.B; a.H = s.n_hops; a.C = s.n_negs; a.d = s.d;
  a.ctr = s.rng_counter; a.seed_lo = (uint32_t)s.rng_seed; a.seed_hi = (uint32_t)(s.rng_seed >> 32);
  return SRH_OK;
}

template <int G>
void launch_fwd(const MixupArgs& a, hipStream_t st) {
  mixup_fwd_kernel<G><<<(unsigned)a.B, 64 * a.H, 0, st>>>(a);
}

}  // namespace

extern "C" {

srh_status_t srh_mixup_fwd_f32(const srh_mixup_args_t* args, const float* d_u, float* d_pos_out, float* d_neg_out,
                               int32_t* d_pick, void* stream) {
  MixupArgs a;
  const srh_status_t rc = mixup_args(args, "mixup_fwd", a);
  if (rc != SRH_OK) return rc;
  if (a.B == 0) return SRH_OK;
  SRH_REQUIRE(d_u && d_pos_out && d_neg_out && d_pick && a.pos && a.neg, "mixup_fwd: null argument");
  for (int k = 0; k < a.H; ++k) SRH_REQUIRE(a.table[k], "mixup_fwd: null hop table %d", k);
  a.u = d_u; a.pos_out = d_pos_out; a.neg_out = d_neg_out; a.pick = d_pick;
  hipStream_t st = as_stream(stream);
  switch (group_width(a.d)) {
    case 1: launch_fwd<1>(a, st); break;
    case 2: launch_fwd<2>(a, st); break;
    case 4: launch_fwd<4>(a, st); break;
    case 8: launch_fwd<8>(a, st); break;
    case 16: launch_fwd<16>(a, st); break;
    case 32: launch_fwd<32>(a, st); break;
    default: launch_fwd<64>(a, st); break;
  }
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

int64_t srh_mixup_bwd_ws_bytes(int64_t B, int32_t n_hops) {
  if (B <= 0 || n_hops < 1 || n_hops > SRH_MIXUP_MAX_HOPS || B * n_hops >= (int64_t(1) << 28)) return 0;
  return align256((int64_t)sizeof(int32_t) * 2 * B * n_hops);
}

srh_status_t srh_mixup_bwd_f32(const srh_mixup_args_t* args, const int32_t* d_pick, const float* d_g_pos,
                               const float* d_g_neg, void* d_ws, void* stream) {
  MixupArgs a;
  const srh_status_t rc = mixup_args(args, "mixup_bwd", a);
  if (rc != SRH_OK) return rc;
  hipStream_t st = as_stream(stream);
  for (int k = 0; k < a.H; ++k) {                    // the tables are written whole: zero, then one store per touched row
    SRH_REQUIRE(a.grad[k] || a.I == 0, "mixup_bwd: null gradient table %d", k);
    if (a.I > 0) SRH_HIP(hipMemsetAsync(a.grad[k], 0, sizeof(float) * (size_t)a.I * a.d, st));
  }
  if (a.B == 0 || a.I == 0 || (!d_g_pos && !d_g_neg)) return SRH_OK;
  SRH_REQUIRE(d_pick && d_ws && a.pos && a.neg, "mixup_bwd: null argument");
  a.pick = const_cast<int32_t*>(d_pick); a.g_pos = d_g_pos; a.g_neg = d_g_neg; a.key = static_cast<int32_t*>(d_ws);
  const int64_t entries = 2 * a.B * a.H;
  mixup_keys<<<(unsigned)((entries + 255) / 256), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  mixup_scatter<<<(unsigned)((entries + 3) / 4), 256, 0, st>>>(a);
  SRH_LAUNCH_CHECK();
  return SRH_OK;
}

}  // extern "C"

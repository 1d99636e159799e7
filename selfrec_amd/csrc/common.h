// Shared helpers for libselfrec_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include "../../include/selfrec_hip.h"

namespace srh {


void set_error(const char* fmt, ...);

#define SRH_REQUIRE(cond, ...)                    \
  do {                                            \
    if (!(cond)) {                                \
      ::srh::set_error(__VA_ARGS__);              \
      return SRH_ERR_INVALID_ARG;                 \
    }                                             \
  } while (0)

// a well-formed call for a shape the kernels do not cover
#define SRH_SUPPORTED(cond, ...)                  \
  do {                                            \
    if (!(cond)) {                                \
      ::srh::set_error(__VA_ARGS__);              \
      return SRH_ERR_UNSUPPORTED;                 \
    }                                             \
  } while (0)

#define SRH_HIP(call)                                                              \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess) {                                                        \
      ::srh::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),      \
                       __FILE__, __LINE__);                                        \
      return SRH_ERR_HIP;                                                          \
    }                                                                              \
  } while (0)

// Every launch is followed by this: catches bad configurations without synchronising.
#define SRH_LAUNCH_CHECK() SRH_HIP(hipGetLastError())

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kWave = 64;  // gfx950 wavefront

constexpr int64_t ceil_div(int64_t n, int64_t per) { return (n + per - 1) / per; }

// workspace carving: every array starts on a 256-byte boundary
inline int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

// One layout function per kernel family names its workspace arrays ONCE, in order, through a Carver: run on a null
// base it only counts (`used` is what the family's *_ws_bytes entry point returns), run on the workspace it hands out
// the pointers.  The size Python allocates and the addresses the kernels write cannot drift apart.
struct Carver {
  char* base;
  int64_t used = 0;
  explicit Carver(void* ws) : base(static_cast<char*>(ws)) {}
  template <typename T>
  void take(T*& p, int64_t count) {
    p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += align256((int64_t)sizeof(T) * count);
  }
};

// ---- chunk-ordered reductions over rows (chunked.hip): no float atomics, the same bits on every call ------------------
// part[z * mats + m][e] = sum over rows r of chunk z (`chunk` rows each), ascending, of x[m][r][e]   (x: mats x n x len)
srh_status_t colsum_chunks(const float* x, int64_t n, int64_t len, int mats, int chunk, float* part, hipStream_t st);
// out[e] = scale * sum over z, ascending, of part[z][e]
srh_status_t reduce_chunks(const float* part, int64_t chunks, int64_t len, float scale, float* out, hipStream_t st);

// C (M x N) = A (M x K) B (K x N) with element strides, K cut into chunks of kchunk rows: chunk z takes rows
// [z kchunk, (z + 1) kchunk) of K and writes its own slab C + z c_zstride (a weight gradient's partials per row chunk,
// summed afterwards by reduce_chunks).
enum GemmEpi { EPI_STORE = 0, EPI_RELU = 1, EPI_MASK = 2 };
struct GemmArgs {
  const float* A;
  int64_t sam, sak;
  const float* B;
  int64_t sbk, sbn;
  float* C;
  int64_t ldc, c_zstride;
  int64_t M, N, K, kchunk;
  const float* aux;      // EPI_RELU: C *= (aux[m ldc + n] > 0)
  const uint8_t* mask;   // EPI_MASK: rows m >= mask_row0: C *= mask[(m - mask_row0) N + n] ? mask_scale : 0
  int64_t mask_row0;
  float mask_scale;
};
srh_status_t gemm64(const GemmArgs& a, GemmEpi epi, int64_t chunks, hipStream_t st);

// lanes per embedding row when each lane owns one float4 of it
inline bool dim_supported(int d) { return d == 32 || d == 64 || d == 128 || d == 256; }

// compute units of the current device (cached per device; 256 on MI355X)
int cu_count();

// the checks srh_batch_fetch promises; `out` = the args as the kernels take them (optional groups normalised)
srh_status_t check_fetch_args(const srh_batch_fetch_args_t* in, srh_batch_fetch_args_t& out);

}  // namespace srh

#ifdef __HIPCC__
namespace srh {

// Stages batch *cursor[0] of the epoch arrays into fixed buffers, publishes its sizes and stamps the
// activity marks with the current optimiser step *cursor[1].  Read-only on the cursor, so any number of
// workgroups can share the copy; the cursor is advanced at the END of the step (Adam's reset pass / zero_rows_kernel /
// cursor_advance_kernel), after the last kernel that reads it.  `block` of `n_blocks` 256-thread workgroups: the body
// of batch_fetch_kernel (optim.hip) and of the fetch workgroups riding on an SpMM launch (spmm.hip).
constexpr int kFetchBlocks = 8;
__device__ __forceinline__ void batch_fetch_body(const srh_batch_fetch_args_t& f, const int block, const int n_blocks) {
  const int64_t b = f.d_cursor[0];
  const int32_t stamp = (int32_t)f.d_cursor[1];
  const int64_t bs = f.batch_size, ptr = b * bs;
  // (two epochs back to back: batch b >= half_batches is batch b - half_batches of the second one)
  const int64_t in_epoch = ((f.half_batches > 0 && b >= f.half_batches) ? b - f.half_batches : b) * bs;
  const int64_t rows = (in_epoch >= f.n_edges) ? 0 : ((in_epoch + bs < f.n_edges) ? bs : f.n_edges - in_epoch);
  const int64_t tid = (int64_t)block * 256 + threadIdx.x, nth = (int64_t)n_blocks * 256;
  for (int64_t i = tid; i < rows; i += nth) {
    const int32_t u = f.d_epoch_u[ptr + i], p = f.d_epoch_i[ptr + i], n = f.d_epoch_j[ptr + i];
    f.d_stage_u[i] = u; f.d_stage_i[i] = p; f.d_stage_j[i] = n;
    if (f.d_row_mark) {
      f.d_row_mark[u] = stamp; f.d_row_mark[f.mark_item_offset + p] = stamp; f.d_row_mark[f.mark_item_offset + n] = stamp;
    }
  }
  int32_t a = 0, c = 0;
  if (f.d_epoch_uniq_u && rows > 0) {
    a = f.d_n_uniq_u[b];
    c = f.d_n_uniq_i[b];
    for (int64_t i = tid; i < a; i += nth) f.d_stage_uniq_u[i] = f.d_epoch_uniq_u[b * bs + i];
    for (int64_t i = tid; i < c; i += nth) f.d_stage_uniq_i[i] = f.d_epoch_uniq_i[b * bs + i];
    if (f.d_stage_cat) {   // [unique users ; unique items] as one index list (SGL.py:120-125 concatenates the two sides)
      for (int64_t i = tid; i < a; i += nth) f.d_stage_cat[i] = f.d_epoch_uniq_u[b * bs + i];
      for (int64_t i = tid; i < c; i += nth) f.d_stage_cat[a + i] = f.d_epoch_uniq_i[b * bs + i] + f.cat_item_offset;
    }
  }
  if (f.d_n_cat && tid == 0) *f.d_n_cat = a + c;
  if (f.d_zero4 && tid < 4) f.d_zero4[tid] = 0.0;        // the step's loss accumulators
  if (f.d_now && tid < 2) f.d_now[tid] = f.d_cursor[tid];
  if (f.d_adam_coef && tid == 0) {
    // torch: bias_correction = 1 - beta ** step (python double), step_size = lr / bc1, denom = sqrt(v) / sqrt(bc2) + eps
    // (the same expressions as adam_kernel, optim.hip -- same bits)
    const double t = (double)f.d_cursor[1];
    f.d_adam_coef[0] = (float)((double)f.adam_lr / (1.0 - pow((double)f.adam_beta1, t)));
    f.d_adam_coef[1] = (float)sqrt(1.0 - pow((double)f.adam_beta2, t));
  }
  if (tid == 0) {
    f.d_meta[0] = (int32_t)rows;
    f.d_meta[1] = a;
    f.d_meta[2] = c;
    f.d_meta[3] = (int32_t)b;
  }
}

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
// 16-byte store of a streamed output.  WT = write-through (`sc1`): the bytes go to the fabric as they are produced and the
// line is not left dirty in this XCD's L2 -- a kernel that ends with tens of MB of dirty lines pays their write-back at
// its boundary (MI355X_MICROARCH.md price list, row "boundary": + B / 6 TB/s), and nothing on this XCD reads them again.
template <bool WT>
__device__ __forceinline__ void st_f4(float4* p, float4 v) {
  if constexpr (WT) {
    typedef float fx4_t __attribute__((ext_vector_type(4)));
    const fx4_t x = {v.x, v.y, v.z, v.w};
    // (s_nop 1 INSIDE the statement: a 16-byte store reads its data registers after issue, and the compiler pads no hazards
    // of an asm statement -- without it the next instruction may overwrite them first: cdna_hip_programming.md 5.7)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
  } else {
    *p = v;
  }
}
// One element of torch.optim.Adam's step (no weight decay, no amsgrad): the ONE definition both the stand-alone pass
// (adam_kernel, optim.hip) and the SpMM epilogue (SRH_EPI_ADAM, spmm.hip) inline, so that they round alike.
//   step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
__device__ __forceinline__ void adam_element(float& m, float& v, float& p, const float g, const float b1, const float omb1,
                                             const float b2, const float omb2, const float step_size, const float bc2_sqrt,
                                             const float eps) {
#pragma clang fp contract(off)    // the fused multiply-adds are the three written here, in every caller
  m = fmaf(m, b1, omb1 * g);
  v = fmaf(v, b2, omb2 * (g * g));
  p = fmaf(-step_size, m / (sqrtf(v) / bc2_sqrt + eps), p);
}
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 f4_fma(float s, float4 x, float4 acc) {
  return make_float4(fmaf(s, x.x, acc.x), fmaf(s, x.y, acc.y), fmaf(s, x.z, acc.z), fmaf(s, x.w, acc.w));
}
__device__ __forceinline__ float4 f4_scale(float4 a, float s) {
  return make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
}
__device__ __forceinline__ float f4_dot(float4 a, float4 b) {
  return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w)));
}
__device__ __forceinline__ float4 f4_shfl_xor(float4 v, int mask) {
  return make_float4(__shfl_xor(v.x, mask), __shfl_xor(v.y, mask), __shfl_xor(v.z, mask), __shfl_xor(v.w, mask));
}
// Sum over the LPR lanes that share one embedding row (LPR a power of two <= 64).
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float sgnf(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }

// ---- the all-f32 InfoNCE passes' work list (losses.hip; here because the SpMM rider below cuts it too) ------------------
constexpr int kNceSplits = 16;      // workspace is sized for this many key splits
constexpr int kNceMaxProblems = 4;
constexpr unsigned long long kLossUnreported = ~0ull;      // (see rows_finish: a loss-partial slot nobody has written yet)
__host__ __device__ inline int64_t nce_pad(int64_t n) { return (n + 63) / 64 * 64; }

// The row counts n_k of a step (unique users / items of the batch: ~1880 and ~1620 of 2048 on the Yelp shape) exist only on
// the device, and the passes' work goes with n_k^2: a grid cut on the host for n_max runs 36 % more key blocks than the
// batch holds and leaves a sixth of the CUs without a workgroup.  So the f32 passes launch one workgroup per CU and every
// workgroup derives the SAME task list from the device counts: problem k is cut into qb_k = ceil(np_k / 128) query blocks
// (8 waves x 16 queries) times splits_k key ranges of per_k 32-key blocks, with the block budget T per task the one that
// minimises rounds(T) x T (rounds = tasks over workgroups; T >= kb_k / 16: the split partials' workspace holds 16).
struct NcePlan {
  int n[kNceMaxProblems], per[kNceMaxProblems], splits[kNceMaxProblems], first[kNceMaxProblems + 1];
};
constexpr int kNceQueryBlock = 128, kNceKeyBlock = 32, kNceMaxPer = 128;

// The cut from the live counts n[0 .. kNceMaxProblems) (0: no such problem) on `slots` workgroups.  Host and device: the
// passes' prep kernel (or the stage rider of the product before them) runs it once per step, srh_infonce_plan answers the
// same question without a launch.
// A task's 1 / l values sit in kNceMaxPer x 32 floats of LDS (NceF32::kLds), so the block budget never exceeds kNceMaxPer:
// with n <= 65 536 (launch_infonce refuses more) t_min <= kNceMaxPer and a cut exists; what the budget leaves over
// becomes more tasks than workgroups, which the passes' task loop strides over.
__host__ __device__ inline void nce_plan(const int* n_live, int slots, NcePlan& p) {
  int qb[kNceMaxProblems], kb[kNceMaxProblems];
  int t_min = 1;
  long long work = 0;
#pragma unroll
  for (int k = 0; k < kNceMaxProblems; ++k) {
    const int n = n_live[k];
    p.n[k] = n;
    const int np = (int)nce_pad(n);
    qb[k] = (np + kNceQueryBlock - 1) / kNceQueryBlock;
    kb[k] = np / kNceKeyBlock;
    const int need = (kb[k] + kNceSplits - 1) / kNceSplits;
    t_min = t_min > need ? t_min : need;
    work += (long long)qb[k] * kb[k];
  }
  const long long even = (work + slots - 1) / slots;
  int t = even > t_min ? (even < kNceMaxPer ? (int)even : kNceMaxPer) : t_min;
  int best_t = t;
  long long best_cost = -1;
  for (int it = 0; it < 32 && (t <= kNceMaxPer || it == 0); ++it, ++t) {
    int tasks = 0;
#pragma unroll
    for (int k = 0; k < kNceMaxProblems; ++k) tasks += qb[k] * ((kb[k] + t - 1) / t);
    const int rounds = (tasks + slots - 1) / slots;
    const long long cost = (long long)rounds * t;
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_t = t; }
    if (rounds <= 1) break;
  }
  p.first[0] = 0;
#pragma unroll
  for (int k = 0; k < kNceMaxProblems; ++k) {
    const int sp = kb[k] > 0 ? (kb[k] + best_t - 1) / best_t : 0;
    p.splits[k] = sp;
    p.per[k] = sp > 0 ? (kb[k] + sp - 1) / sp : 0;       // the even cut of kb_k over its splits (<= best_t)
    p.first[k + 1] = p.first[k] + qb[k] * sp;
  }
}

// One row of an InfoNCE view as nce_prep_body (losses.hip) leaves it: x / max(|x|, 1e-12) (F.normalize's eps), |x| in
// `norm`.  v: this lane's float4 of the row, held by an LPR-lane row-group.  The ONE definition of that arithmetic for the
// prep kernel and the stage rider (pass 1 restates it on its own register layout: nce_tile_f32).
template <int LPR>
__device__ __forceinline__ float4 nce_unit_row(const float4 v, float& norm) {
  const float ss = group_sum<LPR>(f4_dot(v, v));
  norm = sqrtf(ss);
  const float den = fmaxf(norm, 1e-12f);           // F.normalize eps
  return make_float4(v.x / den, v.y / den, v.z / den, v.w / den);
}

// "nce stage": what the all-f32 InfoNCE passes need from before their first launch and that depends on nothing later than
// the contrast table -- the key-side view v2n / norm2, the armed tickets and loss partials, the step's task plan -- done by
// rider workgroups at the head of the product that READS that table (srh_spmm_f32_with_nce_stage), where nce_prep would
// be a launch of its own.  Pass 1 then normalises its own queries (srh_bpr_infonce_fwd_bwd_staged).
struct NceStageProblem {
  const float* src2;          // the key-side table (rows idx[i])
  const int32_t* idx;
  const int32_t* d_n;
  int n_max, np;
  float *v2n, *norm2, *v1n, *norm1;
  int32_t* ticket;
  unsigned long long* losspart;
};
struct NceStageArgs {
  NceStageProblem p[kNceMaxProblems];
  NcePlan* plan;
  int count, slots;
  int gpx;                    // workgroups per problem: 256 threads = 4 waves of 64 / LPR rows each
};
// host: the rider's arguments for `count` problems whose workspaces lie back to back in ws (losses.hip: the carve is there)
srh_status_t nce_stage_args(const srh_infonce_problem_t* problems, int count, int d, void* ws, NceStageArgs& out);
// block: 0 .. count * gpx (more: nothing to do).  Same arithmetic and the same stores as nce_prep_body's key-side half.
template <int LPR>
__device__ __forceinline__ void nce_stage_body(const NceStageArgs& s, const unsigned block) {
  constexpr int G = 64 / LPR;
  const unsigned bz = block / (unsigned)s.gpx, bx = block % (unsigned)s.gpx;
  if ((int)bz >= s.count) return;
  const NceStageProblem& w = s.p[bz];
  const int n = w.d_n ? min(*w.d_n, w.n_max) : w.n_max;
  const int lane = threadIdx.x & 63, g = lane / LPR, sub = lane % LPR;
  const int i = (int)((bx * 256u + threadIdx.x) >> 6) * G + g;
  if (bx == 0) {
    for (int k = threadIdx.x; k <= w.np / 16; k += 256) w.ticket[k] = 0;
    for (int k = threadIdx.x; k < w.np; k += 256) w.losspart[k] = kLossUnreported;
  }
  if (bx == 0 && bz == 0 && threadIdx.x == 0) {
    NcePlan plan;
    int n_live[kNceMaxProblems];
#pragma unroll
    for (int k = 0; k < kNceMaxProblems; ++k) {
      n_live[k] = 0;
      if (k < s.count) n_live[k] = max(0, s.p[k].d_n ? min(*s.p[k].d_n, s.p[k].n_max) : s.p[k].n_max);
    }
    nce_plan(n_live, s.slots, plan);
    *s.plan = plan;
  }
  const bool valid = i < n;
  const int src = valid ? (w.idx ? w.idx[i] : i) : 0;
  const float4 v = reinterpret_cast<const float4*>(w.src2)[(size_t)src * LPR + sub];
  float norm;
  float4 o = nce_unit_row<LPR>(v, norm);
  if (!valid) o = f4_zero();
  if (i < w.np) {
    reinterpret_cast<float4*>(w.v2n)[(size_t)i * LPR + sub] = o;
    if (sub == 0) w.norm2[i] = valid ? norm : 0.f;
    // the query-side rows no query block of pass 1 covers (the plan cuts nce_pad(n) rows, the workspace holds np)
    if (i >= (int)nce_pad(max(n, 0))) {
      reinterpret_cast<float4*>(w.v1n)[(size_t)i * LPR + sub] = f4_zero();
      if (sub == 0) w.norm1[i] = 0.f;
    }
  }
}

// first position in the ascending a[lo, hi) whose value is >= x (hi if there is none); a: global memory or LDS
__device__ __forceinline__ int lower_bound_i32(const int32_t* a, int lo, int hi, int x) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// is x one of the ascending a[lo, hi)?  (a CSR row with sorted columns; an empty range reads nothing)
__device__ __forceinline__ bool sorted_contains(const int32_t* a, int lo, int hi, int x) {
  const int p = lower_bound_i32(a, lo, hi, x);
  return p < hi && a[p] == x;
}

// Counter-based noise: every element's uniform is a pure function of (seed, counter, element),
// so there is no generator state in memory and a captured graph replays with fresh noise by
// bumping one device-side counter.  The mixer is the 2-multiply "lowbias32" integer hash (full
// avalanche, bias < 0.2 bits): the perturbation only needs decorrelated U[0,1) draws, and
// profiling showed the SpMM row epilogue -- not memory -- bounding the kernel, where Philox4x32-10
// costs ~100 VALU ops per float4 against ~35 here.
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t counter_rng_base(uint64_t ctr, uint32_t sub, uint32_t seed_lo, uint32_t seed_hi) {
  const uint32_t key = lowbias32((uint32_t)ctr ^ seed_lo) + lowbias32((uint32_t)(ctr >> 32) ^ seed_hi);
  return key + sub * 0x9E3779B1U;
}
constexpr uint32_t kRngWord1 = 0x85EBCA6BU, kRngWord2 = 0xC2B2AE35U, kRngWord3 = 0x27D4EB2FU;
__device__ __forceinline__ uint4 counter_rng4(uint64_t ctr, uint32_t sub, uint32_t seed_lo, uint32_t seed_hi) {
  const uint32_t base = counter_rng_base(ctr, sub, seed_lo, seed_hi);
  return make_uint4(lowbias32(base), lowbias32(base + kRngWord1), lowbias32(base + kRngWord2), lowbias32(base + kRngWord3));
}
// word w (0..3: x, y, z, w) of counter_rng4 alone, for a consumer that owns one element of the float4
__device__ __forceinline__ uint32_t counter_rng_word(uint64_t ctr, uint32_t sub, int w, uint32_t seed_lo, uint32_t seed_hi) {
  const uint32_t base = counter_rng_base(ctr, sub, seed_lo, seed_hi);
  return lowbias32(base + (w == 0 ? 0U : w == 1 ? kRngWord1 : w == 2 ? kRngWord2 : kRngWord3));
}
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

}  // namespace srh
#endif

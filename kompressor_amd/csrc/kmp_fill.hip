// kmp_fill.hip -- masked float32 fields: the hold-fill of a quantiser's marked integer
// array (KMP_CODER_FILL) and the patch of a float32 array from a run table (KMP_CODER_RUNS).
//
// FILL is three launches on one stream, in the shape of kmp_compare.hip: every workgroup summarises its
// span (last and first unmarked value), one wave folds the summaries into each workgroup's incoming
// carry, then every workgroup fills its span.  The spans are a function of the count alone
// (fill_plan).  No atomics, no tickets, no spinning: a later launch sees an earlier one's stores
// because it is a later launch on the same stream, and the result is a function of the buffers alone.
// HBM-bound: the array is read twice and written once.
//
// The fill never reads an element another lane writes (a lane loads its own item, then stores it; the
// carries come from the workspace, which the earlier launches finished), so ``out`` may be ``x`` itself.
#include "kmp_primitives.h"

namespace kmp {

constexpr int kFillItem = 8;                     // consecutive elements of one lane
constexpr int kFillTile = kThreads * kFillItem;  // consecutive elements of one workgroup step
constexpr int kFillWaves = kThreads / 64;
static_assert(kFillTile == KMP_FILL_TILE, "the header states the tile");

// workgroup g owns [g * span, min(n, (g + 1) * span))
struct FillPlan {
  int64_t span;
  int groups;
};
static inline FillPlan fill_plan(int64_t n) {
  const int64_t tiles = ceil_div(n, kFillTile);
  const int64_t per = ceil_div(tiles, KMP_FILL_GROUPS);
  return FillPlan{per * kFillTile, (int)ceil_div(tiles, per)};
}

// the workspace: one record of four 32-bit words per workgroup
struct FillRec {
  int32_t last, first;  // the span's last / first unmarked value (when ``has``)
  int32_t has;          // 1: the span holds an unmarked element
  int32_t carry;        // what a marked element with no unmarked one before it in the span takes
};
static_assert(sizeof(FillRec) * KMP_FILL_GROUPS == KMP_FILL_BYTES, "the header states the workspace");

template <typename T>
struct FillItem {
  T e[kFillItem];
};

// a lane's item: one aligned 16-byte access per 16 bytes (VEC, a whole item inside the array), else
// element by element, an element at or past ``n`` read as marked
template <typename T, bool VEC>
__device__ __forceinline__ FillItem<T> fill_load(const T* x, int64_t base, int64_t n) {
  constexpr T MARK = std::numeric_limits<T>::min();
  FillItem<T> it;
  if (VEC && base + kFillItem <= n) {
    constexpr int NV = kFillItem * (int)sizeof(T) / 16;
    const u32x4v* p = (const u32x4v*)(x + base);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const u32x4v w = __builtin_nontemporal_load(p + v);
      __builtin_memcpy((char*)it.e + 16 * v, &w, 16);
    }
  } else {
#pragma unroll
    for (int i = 0; i < kFillItem; ++i) it.e[i] = base + i < n ? x[base + i] : MARK;
  }
  return it;
}

template <typename T, bool VEC>
__device__ __forceinline__ void fill_store(T* out, int64_t base, int64_t n, const FillItem<T>& it) {
  if (VEC && base + kFillItem <= n) {
    constexpr int NV = kFillItem * (int)sizeof(T) / 16;
    u32x4v* p = (u32x4v*)(out + base);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      u32x4v w;
      __builtin_memcpy(&w, (const char*)it.e + 16 * v, 16);
      __builtin_nontemporal_store(w, p + v);
    }
  } else {
#pragma unroll
    for (int i = 0; i < kFillItem; ++i)
      if (base + i < n) out[base + i] = it.e[i];
  }
}

// launch 1: the span's summary.  A lane keeps the positions (in items) of its first and last item with an
// unmarked element; the wave's are the lowest / highest such lane's, the workgroup's by wave order in LDS.
template <typename T, bool VEC>
__global__ void __launch_bounds__(kThreads) fill_summary_kernel(const T* x, int64_t n, int64_t span, FillRec* ws) {
  constexpr T MARK = std::numeric_limits<T>::min();
  __shared__ int64_t s_fpos[kFillWaves], s_lpos[kFillWaves];
  __shared__ int32_t s_fval[kFillWaves], s_lval[kFillWaves];
  const int64_t lo = (int64_t)blockIdx.x * span, hi = lo + span < n ? lo + span : n;
  int64_t fpos = INT64_MAX, lpos = -1;
  int32_t fval = 0, lval = 0;
  for (int64_t base = lo + (int64_t)threadIdx.x * kFillItem; base < hi; base += kFillTile) {
    const FillItem<T> it = fill_load<T, VEC>(x, base, n);
    bool any = false;
    int32_t f = 0, l = 0;
#pragma unroll
    for (int i = 0; i < kFillItem; ++i) {
      const bool ok = it.e[i] != MARK;
      f = (ok && !any) ? (int32_t)it.e[i] : f;
      l = ok ? (int32_t)it.e[i] : l;
      any = any || ok;
    }
    if (any) {
      if (fpos == INT64_MAX) { fpos = base; fval = f; }
      lpos = base;
      lval = l;
    }
  }
  // the 64 lanes: minimum fpos / maximum lpos, the value travelling with its position
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t of = (int64_t)(((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)((uint64_t)fpos >> 32), d, 64) << 32) |
                                 (uint32_t)__shfl_down((int)(uint32_t)(uint64_t)fpos, d, 64));
    const int64_t ol = (int64_t)(((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)((uint64_t)lpos >> 32), d, 64) << 32) |
                                 (uint32_t)__shfl_down((int)(uint32_t)(uint64_t)lpos, d, 64));
    const int32_t ofv = __shfl_down(fval, d, 64), olv = __shfl_down(lval, d, 64);
    if (of < fpos) { fpos = of; fval = ofv; }
    if (ol > lpos) { lpos = ol; lval = olv; }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_fpos[w] = fpos; s_fval[w] = fval;
    s_lpos[w] = lpos; s_lval[w] = lval;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kFillWaves; ++k) {
      if (s_fpos[k] < fpos) { fpos = s_fpos[k]; fval = s_fval[k]; }
      if (s_lpos[k] > lpos) { lpos = s_lpos[k]; lval = s_lval[k]; }
    }
    FillRec r;
    r.last = lval;
    r.first = fval;
    r.has = lpos >= 0 ? 1 : 0;
    r.carry = 0;
    ws[blockIdx.x] = r;
  }
}

// the highest lane below ``lane`` whose bit is set in ``mask``, or -1
__device__ __forceinline__ int fill_source_below(uint64_t mask, int lane) {
  const uint64_t below = mask & ((1ull << lane) - 1ull);
  return below ? 63 - __builtin_clzll(below) : -1;
}

// launch 2, one wave: lane l owns the ``per`` consecutive workgroups from l * per.  A workgroup's carry is the
// last unmarked value of the workgroups before it; with none before it, the array's first unmarked value
// (the leading marked stretch); with none at all, 0.
__global__ void __launch_bounds__(64) fill_carry_kernel(FillRec* ws, int groups) {
  const int lane = threadIdx.x;
  const int per = (groups + 63) / 64;
  const int g0 = lane * per, g1 = g0 + per < groups ? g0 + per : groups;
  bool has = false;
  int32_t last = 0, first = 0;
  for (int g = g0; g < g1; ++g) {
    const FillRec r = ws[g];
    if (r.has) {
      if (!has) first = r.first;
      last = r.last;
      has = true;
    }
  }
  const uint64_t mask = __ballot(has);
  const int src = fill_source_below(mask, lane);
  const int32_t before = __shfl(last, src < 0 ? 0 : src, 64);
  const int32_t lead = __shfl(first, mask ? __builtin_ctzll(mask) : 0, 64);  // the array's first unmarked value
  bool seen = src >= 0;
  int32_t carry = seen ? before : (mask ? lead : 0);
  for (int g = g0; g < g1; ++g) {
    const FillRec r = ws[g];
    ws[g].carry = carry;
    if (r.has) carry = r.last;
  }
}

// launch 3: the fill.  Within a lane the item is walked in order; a lane's incoming value is the last
// unmarked one of the highest lane below it that has any (a ballot and one __shfl), else the wave's
// incoming value: the waves before it in this step (LDS, wave order), else the workgroup's running carry.
template <typename T, bool VEC>
__global__ void __launch_bounds__(kThreads) fill_kernel(const T* x, int64_t n, int64_t span, const FillRec* ws, T* out) {
  constexpr T MARK = std::numeric_limits<T>::min();
  __shared__ int32_t s_has[2][kFillWaves], s_val[2][kFillWaves];
  const int64_t lo = (int64_t)blockIdx.x * span, hi = lo + span < n ? lo + span : n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t run = ws[blockIdx.x].carry;  // the workgroup's running carry, the same in every thread
  int buf = 0;
  // every thread takes every step of the workgroup: the barrier is uniform
  for (int64_t tile = lo; tile < hi; tile += kFillTile, buf ^= 1) {
    const int64_t base = tile + (int64_t)threadIdx.x * kFillItem;
    FillItem<T> it = fill_load<T, VEC>(x, base, n);
    bool any = false;
    int32_t l = 0;
#pragma unroll
    for (int i = 0; i < kFillItem; ++i) {
      const bool ok = it.e[i] != MARK;
      l = ok ? (int32_t)it.e[i] : l;
      any = any || ok;
    }
    const uint64_t mask = __ballot(any);
    const int src = fill_source_below(mask, lane);
    const int32_t below = __shfl(l, src < 0 ? 0 : src, 64);
    const int32_t wave_last = __shfl(l, mask ? 63 - __builtin_clzll(mask) : 0, 64);
    if (lane == 0) {
      s_has[buf][w] = mask ? 1 : 0;
      s_val[buf][w] = wave_last;
    }
    __syncthreads();
    int32_t in = run;
#pragma unroll
    for (int k = 0; k < kFillWaves; ++k) {
      const bool h = s_has[buf][k] != 0;
      const int32_t v = s_val[buf][k];
      in = (k < w && h) ? v : in;
      run = h ? v : run;
    }
    int32_t cur = src >= 0 ? below : in;
#pragma unroll
    for (int i = 0; i < kFillItem; ++i) {
      const bool ok = it.e[i] != MARK;
      cur = ok ? (int32_t)it.e[i] : cur;
      it.e[i] = (T)cur;
    }
    fill_store<T, VEC>(out, base, n, it);
    // the other LDS buffer serves the next step: a thread that writes this one again has passed the next
    // step's barrier, which every thread reaches only after reading this one
  }
}

template <typename T>
static int fill_go(const void* x, int64_t n, void* out, void* ws, hipStream_t s) {
  const FillPlan p = fill_plan(n);
  FillRec* rec = (FillRec*)ws;
  if ((((uintptr_t)x | (uintptr_t)out) & 15) == 0) {
    fill_summary_kernel<T, true><<<p.groups, kThreads, 0, s>>>((const T*)x, n, p.span, rec);
    fill_carry_kernel<<<1, 64, 0, s>>>(rec, p.groups);
    fill_kernel<T, true><<<p.groups, kThreads, 0, s>>>((const T*)x, n, p.span, rec, (T*)out);
  } else {
    fill_summary_kernel<T, false><<<p.groups, kThreads, 0, s>>>((const T*)x, n, p.span, rec);
    fill_carry_kernel<<<1, 64, 0, s>>>(rec, p.groups);
    fill_kernel<T, false><<<p.groups, kThreads, 0, s>>>((const T*)x, n, p.span, rec, (T*)out);
  }
  return check_launch("fill");
}

int launch_fill(int dtype, const void* x, int64_t n, void* out, void* ws, hipStream_t stream) {
  switch (dtype) {
    case KMP_I16: return fill_go<int16_t>(x, n, out, ws, stream);
    case KMP_I32: return fill_go<int32_t>(x, n, out, ws, stream);
    default: return fail(KMP_ERR_ARG, "kmp_code: fill takes int16 or int32 arrays");
  }
}

// ------------------------------------------------------------------------------------------
// RUNS: out[start, start + length) = bits for every record (start low, start high, length, bits)
// ------------------------------------------------------------------------------------------
constexpr uint32_t kRunsShort = 8;  // up to this length a lane writes its own run

// A wave owns 64 consecutive records, one per lane (a 16-byte load).  Short runs are written by their
// lane; the long ones are taken one after the other by the whole wave: single elements up to the first
// 16-byte boundary, 16-byte stores, single elements after the last.  Any length is served.  The long
// records among a wave's 64 are walked by that wave alone, one after the other: a table cuts long runs
// into pieces of KMP_RUNS_PIECE, so a long run spreads over one wave per 64 pieces and no wave walks more
// than 64 * KMP_RUNS_PIECE elements of it.
__global__ void __launch_bounds__(kThreads) runs_kernel(const u32x4v* __restrict__ table, int64_t R,
                                                      uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * kFillWaves;
  for (int64_t r0 = ((int64_t)blockIdx.x * kFillWaves + (threadIdx.x >> 6)) * 64; r0 < R; r0 += waves * 64) {
    const int64_t r = r0 + lane;
    u32x4v rec = {0u, 0u, 0u, 0u};
    if (r < R) rec = table[r];
    const uint32_t len = rec[2], bits = rec[3];
    uint32_t* p = out + (int64_t)(((uint64_t)rec[1] << 32) | rec[0]);
    if (len <= kRunsShort)
      for (uint32_t i = 0; i < len; ++i) p[i] = bits;
    uint64_t todo = __ballot(len > kRunsShort);
    while (todo) {  // wave-uniform
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t slo = (uint32_t)__shfl((int)rec[0], src, 64), shi = (uint32_t)__shfl((int)rec[1], src, 64);
      const uint32_t n = (uint32_t)__shfl((int)len, src, 64), b = (uint32_t)__shfl((int)bits, src, 64);
      uint32_t* q = out + (int64_t)(((uint64_t)shi << 32) | slo);
      uint32_t head = (uint32_t)((0u - (uint32_t)((uintptr_t)q >> 2)) & 3u);  // elements to the 16-byte boundary
      head = head < n ? head : n;
      if ((uint32_t)lane < head) q[lane] = b;
      const uint32_t nvec = (n - head) / 4, tail = (n - head) % 4;
      u32x4v* qv = (u32x4v*)(q + head);
      const u32x4v bv = {b, b, b, b};
      for (uint32_t v = lane; v < nvec; v += 64) __builtin_nontemporal_store(bv, qv + v);
      if ((uint32_t)lane < tail) q[head + 4 * nvec + lane] = b;
    }
  }
}

int launch_runs(const void* table, int64_t R, void* out, hipStream_t stream) {
  const int64_t groups = ceil_div(R, 64 * kFillWaves);
  runs_kernel<<<(unsigned)(groups > 65536 ? 65536 : groups), kThreads, 0, stream>>>((const u32x4v*)table, R,
                                                                                  (uint32_t*)out);
  return check_launch("runs");
}

}  // namespace kmp

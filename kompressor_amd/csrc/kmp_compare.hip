// kmp_compare.hip -- error statistics of a restored array against its original (KMP_CODER_COMPARE,
// DESIGN.md §20): one pass over both arrays, a record of eight 64-bit words per workgroup, then one wave
// that folds the workgroups' records in index order.  HBM-bound reads, 64 KiB written.
//
// Determinism: every reduction is a fixed tree -- a lane's items in grid-stride order, the 64 lanes by
// shuffles at distances 32, 16, .. 1, a workgroup's waves in wave order, the workgroups in index order
// (lane l of the finishing wave folds partials l, l + 64, ..., then the same shuffle tree).  The grid is
// a function of the count and the alignment alone.  No atomics, no tickets, no spinning: the second
// launch sees the first one's stores because it is a later launch on the same stream.
#include "kmp_primitives.h"

namespace kmp {

constexpr int kCmpWaves = kThreads / 64;

// the common form every kernel reduces in: the record's first six words
template <bool FSSE>
struct CmpAcc {
  using Sse = typename std::conditional<FSSE, double, uint64_t>::type;
  uint64_t count, mismatch;
  double max_abs;
  Sse sse;
  double xmin, xmax;
};

template <bool FSSE>
__device__ __forceinline__ CmpAcc<FSSE> cmp_identity() {
  return CmpAcc<FSSE>{0, 0, 0.0, 0, __builtin_inf(), -__builtin_inf()};
}

// a (earlier in the order) with b folded in
template <bool FSSE>
__device__ __forceinline__ void cmp_fold(CmpAcc<FSSE>& a, const CmpAcc<FSSE>& b) {
  a.count += b.count;
  a.mismatch += b.mismatch;
  a.max_abs = __builtin_fmax(a.max_abs, b.max_abs);
  a.sse += b.sse;
  a.xmin = __builtin_fmin(a.xmin, b.xmin);
  a.xmax = __builtin_fmax(a.xmax, b.xmax);
}

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d, 64);
  const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double shfl_down_f64(double v, int d) {
  return __longlong_as_double((long long)shfl_down_u64((uint64_t)__double_as_longlong(v), d));
}

// the fixed tree over the 64 lanes: lane 0 ends with the wave's value
template <bool FSSE>
__device__ __forceinline__ void cmp_wave_reduce(CmpAcc<FSSE>& a) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    CmpAcc<FSSE> b;
    b.count = shfl_down_u64(a.count, d);
    b.mismatch = shfl_down_u64(a.mismatch, d);
    b.max_abs = shfl_down_f64(a.max_abs, d);
    if constexpr (FSSE) b.sse = shfl_down_f64(a.sse, d);
    else b.sse = shfl_down_u64(a.sse, d);
    b.xmin = shfl_down_f64(a.xmin, d);
    b.xmax = shfl_down_f64(a.xmax, d);
    cmp_fold(a, b);
  }
}

// a zero as +0.0 (min / max of -0.0 and +0.0 is either)
__device__ __forceinline__ double plus_zero(double v) { return v == 0.0 ? 0.0 : v; }

template <bool FSSE>
__device__ __forceinline__ void cmp_store(uint64_t* rec, const CmpAcc<FSSE>& a) {
  rec[0] = a.count;
  rec[1] = a.mismatch;
  rec[2] = (uint64_t)__double_as_longlong(a.max_abs);
  if constexpr (FSSE) rec[3] = (uint64_t)__double_as_longlong(a.sse);
  else rec[3] = a.sse;
  rec[4] = (uint64_t)__double_as_longlong(plus_zero(a.xmin));
  rec[5] = (uint64_t)__double_as_longlong(plus_zero(a.xmax));
  rec[6] = 0;
  rec[7] = 0;
}

template <bool FSSE>
__device__ __forceinline__ CmpAcc<FSSE> cmp_load(const uint64_t* rec) {
  CmpAcc<FSSE> a;
  a.count = rec[0];
  a.mismatch = rec[1];
  a.max_abs = __longlong_as_double((long long)rec[2]);
  if constexpr (FSSE) a.sse = __longlong_as_double((long long)rec[3]);
  else a.sse = rec[3];
  a.xmin = __longlong_as_double((long long)rec[4]);
  a.xmax = __longlong_as_double((long long)rec[5]);
  return a;
}

// the workgroup's waves through LDS in wave order; thread 0 stores partial ``blockIdx.x``
template <bool FSSE>
__device__ __forceinline__ void cmp_block_finish(CmpAcc<FSSE> a, uint64_t* __restrict__ out) {
  __shared__ CmpAcc<FSSE> waves[kCmpWaves];
  cmp_wave_reduce(a);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kCmpWaves; ++w) cmp_fold(a, waves[w]);
    cmp_store(out + 8 * (1 + (int64_t)blockIdx.x), a);
  }
}

// ---- per-lane accumulators ----
// float32: u64 counts, an f64 max and an f64 sum; the range of x in float32 (exact), widened at the end
struct LaneF32 {
  static constexpr bool FSSE = true;
  uint64_t count = 0, mismatch = 0;
  double max_abs = 0.0, sse = 0.0;
  float xmin = __builtin_inff(), xmax = -__builtin_inff();
  __device__ __forceinline__ void add(uint32_t xb, uint32_t rb) {
    const bool fin = (xb & 0x7f800000u) != 0x7f800000u && (rb & 0x7f800000u) != 0x7f800000u;
    const float xf = __uint_as_float(xb), rf = __uint_as_float(rb);
    const double e = fin ? (double)rf - (double)xf : 0.0;
    count += fin ? 1u : 0u;
    mismatch += (!fin && xb != rb) ? 1u : 0u;
    max_abs = __builtin_fmax(max_abs, __builtin_fabs(e));
    sse += e * e;
    xmin = __builtin_fminf(xmin, fin ? xf : __builtin_inff());
    xmax = __builtin_fmaxf(xmax, fin ? xf : -__builtin_inff());
  }
  __device__ __forceinline__ CmpAcc<true> acc() const {
    return CmpAcc<true>{count, mismatch, max_abs, sse, (double)xmin, (double)xmax};
  }
};

// integer samples: |e| <= 65535, so a square fits 32 bits and sixteen 8-bit squares do too
template <typename T>
struct LaneInt {
  static constexpr bool FSSE = false;
  uint64_t count = 0, sse = 0;
  uint32_t max_abs = 0, item_sse = 0;
  int32_t xmin = std::numeric_limits<int32_t>::max(), xmax = std::numeric_limits<int32_t>::min();
  __device__ __forceinline__ void add(T xv, T rv) {
    const int32_t x = (int32_t)xv, d = (int32_t)rv - x;
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
    max_abs = ad > max_abs ? ad : max_abs;
    if constexpr (sizeof(T) == 1) item_sse += ad * ad;
    else sse += (uint64_t)(ad * ad);
    xmin = x < xmin ? x : xmin;
    xmax = x > xmax ? x : xmax;
  }
  // after at most 16 elements
  __device__ __forceinline__ void end_item(uint32_t elements) {
    count += elements;
    if constexpr (sizeof(T) == 1) {
      sse += item_sse;
      item_sse = 0;
    }
  }
  __device__ __forceinline__ CmpAcc<false> acc() const {
    return CmpAcc<false>{count, 0, (double)max_abs, sse, count ? (double)xmin : __builtin_inf(),
                         count ? (double)xmax : -__builtin_inf()};
  }
};

// vector form: one item = 16 bytes of each array, both 16-byte aligned; ``items`` of them
template <typename T>
__global__ void __launch_bounds__(kThreads) compare_vec_kernel(const u32x4v* __restrict__ x,
                                                             const u32x4v* __restrict__ r, int64_t items,
                                                             uint64_t* __restrict__ out) {
  constexpr bool F = std::is_same<T, float>::value;
  typename std::conditional<F, LaneF32, LaneInt<T>>::type lane;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < items; t += (int64_t)gridDim.x * kThreads) {
    const u32x4v xv = __builtin_nontemporal_load(x + t), rv = __builtin_nontemporal_load(r + t);
    if constexpr (F) {
#pragma unroll
      for (int i = 0; i < 4; ++i) lane.add(xv[i], rv[i]);
    } else {
      constexpr int V = 16 / (int)sizeof(T);
      const T* xx = (const T*)&xv;
      const T* rr = (const T*)&rv;
#pragma unroll
      for (int i = 0; i < V; ++i) lane.add(xx[i], rr[i]);
      lane.end_item(V);
    }
  }
  cmp_block_finish(lane.acc(), out);
}

// element form: any alignment, any count
template <typename T>
__global__ void __launch_bounds__(kThreads) compare_kernel(const void* __restrict__ x, const void* __restrict__ r,
                                                         int64_t n, uint64_t* __restrict__ out) {
  constexpr bool F = std::is_same<T, float>::value;
  typename std::conditional<F, LaneF32, LaneInt<T>>::type lane;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < n; t += (int64_t)gridDim.x * kThreads) {
    if constexpr (F) {
      lane.add(((const uint32_t*)x)[t], ((const uint32_t*)r)[t]);
    } else {
      lane.add(((const T*)x)[t], ((const T*)r)[t]);
      lane.end_item(1);
    }
  }
  cmp_block_finish(lane.acc(), out);
}

// one wave: lane l folds partials l, l + 64, ... in order, the tree, lane 0 writes the record -- seeded
// from the record already there when ``cont``
template <bool FSSE>
__global__ void __launch_bounds__(64) compare_finish_kernel(uint64_t* __restrict__ out, int groups, int cont) {
  CmpAcc<FSSE> a = cmp_identity<FSSE>();
  for (int g = threadIdx.x; g < groups; g += 64) cmp_fold(a, cmp_load<FSSE>(out + 8 * (1 + (int64_t)g)));
  cmp_wave_reduce(a);
  if (threadIdx.x == 0) {
    if (cont) {
      CmpAcc<FSSE> old = cmp_load<FSSE>(out);
      cmp_fold(old, a);
      a = old;
    }
    cmp_store(out, a);
  }
}

static unsigned compare_grid(int64_t items) {
  const int64_t g = ceil_div(items, kThreads);
  return (unsigned)(g > KMP_COMPARE_GROUPS ? KMP_COMPARE_GROUPS : g);
}

template <typename T>
static int compare_go(const void* x, const void* r, int64_t n, void* out, int cont, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr bool F = std::is_same<T, float>::value;
  unsigned grid;
  if ((((uintptr_t)x | (uintptr_t)r) & 15) == 0 && n % V == 0) {
    grid = compare_grid(n / V);
    compare_vec_kernel<T><<<grid, kThreads, 0, s>>>((const u32x4v*)x, (const u32x4v*)r, n / V, (uint64_t*)out);
  } else {
    grid = compare_grid(n);
    compare_kernel<T><<<grid, kThreads, 0, s>>>(x, r, n, (uint64_t*)out);
  }
  compare_finish_kernel<F><<<1, 64, 0, s>>>((uint64_t*)out, (int)grid, cont);
  return check_launch("compare");
}

int launch_compare(int dtype, const void* x, const void* r, int64_t n, void* out, int cont, hipStream_t stream) {
  switch (dtype) {
    case KMP_F32: return compare_go<float>(x, r, n, out, cont, stream);
    case KMP_U8: return compare_go<uint8_t>(x, r, n, out, cont, stream);
    case KMP_U16: return compare_go<uint16_t>(x, r, n, out, cont, stream);
    case KMP_I8: return compare_go<int8_t>(x, r, n, out, cont, stream);
    case KMP_I16: return compare_go<int16_t>(x, r, n, out, cont, stream);
    default: return fail(KMP_ERR_ARG, "kmp_code: compare takes float32, uint8, uint16, int8 or int16 samples");
  }
}

}  // namespace kmp

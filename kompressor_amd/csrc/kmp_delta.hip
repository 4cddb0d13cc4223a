// kmp_delta.hip -- time series: the delta of two integer arrays modulo 2^W
// (KMP_CODER_DELTA).  ENCODE writes out[i] = x[i] - pred[i], DECODE out[i] = x[i] + pred[i], in the
// unsigned type of the samples' width, so signed and unsigned samples give the same bits.
//
// One launch, in the shape of quant_vec_kernel / quant_kernel: a 16-byte non-temporal form when the three
// pointers are 16-byte aligned and the count is a multiple of 16 / sizeof(sample), an element form for
// everything else.  No atomics, no LDS, no workspace: the result is a function of the buffers alone.
// HBM-bound: two arrays read, one written.
//
// A lane loads what it stores before it stores it and reads nothing another lane writes, so ``out`` may be
// ``x`` itself (no __restrict__ on those two); ``pred`` never overlaps ``out`` (kmp_code refuses it).
#include "kmp_primitives.h"

namespace kmp {

template <int DIR, typename T>
__device__ __forceinline__ T delta_one(T x, T p) {
  return DIR == KMP_ENCODE ? (T)(x - p) : (T)(x + p);
}

// element form: any alignment (the dtype's at least), any count
template <int DIR, typename T>
__global__ void __launch_bounds__(kThreads) delta_kernel(const T* pred, const T* x, int64_t n, T* out) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    out[t] = delta_one<DIR, T>(x[t], pred[t]);
}

// vector form: one item = 16 bytes of each array; ``n16`` items
template <int DIR, typename T>
__global__ void __launch_bounds__(kThreads) delta_vec_kernel(const u32x4v* pred, const u32x4v* x, int64_t n16,
                                                           u32x4v* out) {
  constexpr int V = 16 / (int)sizeof(T);
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n16; t += (int64_t)gridDim.x * blockDim.x) {
    const u32x4v pv = __builtin_nontemporal_load(pred + t), xv = __builtin_nontemporal_load(x + t);
    const T* pp = (const T*)&pv;
    const T* xx = (const T*)&xv;
    u32x4v ov;
    T* oo = (T*)&ov;
#pragma unroll
    for (int i = 0; i < V; ++i) oo[i] = delta_one<DIR, T>(xx[i], pp[i]);
    __builtin_nontemporal_store(ov, out + t);
  }
}

template <int DIR, typename T>
static int delta_go(const void* pred, const void* x, int64_t n, void* out, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  if ((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)out) & 15) == 0 && n % V == 0)
    delta_vec_kernel<DIR, T><<<grid_for(n / V), kThreads, 0, s>>>((const u32x4v*)pred, (const u32x4v*)x, n / V,
                                                                 (u32x4v*)out);
  else
    delta_kernel<DIR, T><<<grid_for(n), kThreads, 0, s>>>((const T*)pred, (const T*)x, n, (T*)out);
  return check_launch("delta");
}

template <int DIR>
static int delta_width(int width, const void* pred, const void* x, int64_t n, void* out, hipStream_t s) {
  switch (width) {
    case 1: return delta_go<DIR, uint8_t>(pred, x, n, out, s);
    case 2: return delta_go<DIR, uint16_t>(pred, x, n, out, s);
    case 4: return delta_go<DIR, uint32_t>(pred, x, n, out, s);
    default: return fail(KMP_ERR_ARG, "kmp_code: delta takes 8-, 16- or 32-bit integer samples");
  }
}

int launch_delta(int direction, int width, const void* pred, const void* x, int64_t n, void* out,
                 hipStream_t stream) {
  return direction == KMP_ENCODE ? delta_width<KMP_ENCODE>(width, pred, x, n, out, stream)
                                 : delta_width<KMP_DECODE>(width, pred, x, n, out, stream);
}

}  // namespace kmp

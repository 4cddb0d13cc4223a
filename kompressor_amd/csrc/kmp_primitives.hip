// kmp_primitives.hip -- the geometry primitives of the reference API as gfx950 kernels.
//
// These back the generic ``predictions_fn`` callback path (a caller's predictor composes
// features_from_lowres / maps_from_predictions / coders exactly as in the reference) and the
// standalone re-exports of volume/__init__.py:31-35 and image/__init__.py:31-35.  They are
// HBM-bound gathers/scatters: one thread per output element group, 64-bit index math,
// grid-stride loops, 256-thread workgroups.  The fused one-pass codec lives in kmp_codec*.hip, the
// predictor primitives in kmp_maps_from_predictions.hip and kmp_mean_predict.hip.
#include "kmp_primitives.h"

namespace kmp {

// ------------------------------------------------------------------------------------------
// Parity (de)interleave: lowres_from_highres, maps_from_highres, highres_from_lowres_and_maps
// ------------------------------------------------------------------------------------------
// out_k[b, o, c] = in[b, 2*o + par_k, c] for every class k whose pointer is set and whose
// extent contains o.  Class 0 = all-even (lowres), classes 1..7 (1..3) = maps.
template <typename T, typename I>
__global__ void __launch_bounds__(kThreads) deinterleave_kernel(const T* __restrict__ in, I B, E3<I> n,
                                                              I C, int nsp, MapPtrs outs, void* lowres,
                                                              I total) {
  const int nmaps = nsp == 3 ? 7 : 3;
  // frame = ceil(n/2) per axis (dummy axes: 1)
  const I f0 = (n.e[0] + 1) / 2, f1 = (n.e[1] + 1) / 2, f2 = (n.e[2] + 1) / 2;
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < total; t += (I)gridDim.x * blockDim.x) {
    IdxT<I> q = unflat_t<I>(t, f0, f1, f2, C);
    auto src = [&](int pz, int py, int px) -> T {
      const I z = 2 * q.i0 + pz, y = 2 * q.i1 + py, x = 2 * q.i2 + px;
      return in[(((q.b * n.e[0] + z) * n.e[1] + y) * n.e[2] + x) * C + q.c];
    };
    if (lowres) {
      T* o = (T*)lowres;
      o[(((q.b * f0 + q.i0) * f1 + q.i1) * f2 + q.i2) * C + q.c] = src(0, 0, 0);
    }
    for (int k = 0; k < nmaps; ++k) {
      if (!outs.p[k]) continue;
      int par[3];
      map_parity(nsp, k, par);
      // extent of class: parity 1 -> floor(n/2), parity 0 -> ceil(n/2); dummy axis -> 1
      I e[3];
      const I idx[3] = {q.i0, q.i1, q.i2};
      bool ok = true;
      for (int a = 0; a < 3; ++a) {
        e[a] = (a < 3 - nsp) ? 1 : (par[a] ? n.e[a] / 2 : (n.e[a] + 1) / 2);
        ok = ok && idx[a] < e[a];
      }
      if (!ok) continue;
      T* o = (T*)outs.p[k];
      o[(((q.b * e[0] + q.i0) * e[1] + q.i1) * e[2] + q.i2) * C + q.c] = src(par[0], par[1], par[2]);
    }
  }
}

// out[b, 2*o + par_k, c] = class_k[b, o, c]; out extent 2L-1 per axis.  Class extents follow
// highres_from_lowres_and_maps: lowres L, maps (par ? L-1 : L).
template <typename T, typename I>
__global__ void __launch_bounds__(kThreads) interleave_kernel(const T* __restrict__ lowres, CMapPtrs maps,
                                                            I B, E3<I> L, I C, int nsp, T* __restrict__ out,
                                                            I total) {
  const int nmaps = nsp == 3 ? 7 : 3;
  const I h0 = 2 * L.e[0] - 1, h1 = 2 * L.e[1] - 1, h2 = 2 * L.e[2] - 1;
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < total; t += (I)gridDim.x * blockDim.x) {
    IdxT<I> q = unflat_t<I>(t, L.e[0], L.e[1], L.e[2], C);
    auto dst = [&](int pz, int py, int px) -> T& {
      const I z = 2 * q.i0 + pz, y = 2 * q.i1 + py, x = 2 * q.i2 + px;
      return out[(((q.b * h0 + z) * h1 + y) * h2 + x) * C + q.c];
    };
    dst(0, 0, 0) = lowres[t];
    for (int k = 0; k < nmaps; ++k) {
      int par[3];
      map_parity(nsp, k, par);
      I e[3];
      const I idx[3] = {q.i0, q.i1, q.i2};
      bool ok = true;
      for (int a = 0; a < 3; ++a) {
        e[a] = (a < 3 - nsp) ? 1 : (par[a] ? L.e[a] - 1 : L.e[a]);
        ok = ok && idx[a] < e[a];
      }
      if (!ok) continue;
      const T* m = (const T*)maps.p[k];
      dst(par[0], par[1], par[2]) = m[(((q.b * e[0] + q.i0) * e[1] + q.i1) * e[2] + q.i2) * C + q.c];
    }
  }
}

// ------------------------------------------------------------------------------------------
// targets_from_highres: [B, cells..., K, C], K = 19 (5); cells = (n-1)/2 per axis.
// Offsets (relative to 2*cell) per target in reference order, volume/utils.py:40-72.
// ------------------------------------------------------------------------------------------
__constant__ int8_t c_targets3[19][3] = {
    {1, 1, 0}, {1, 1, 2}, {1, 0, 1}, {1, 2, 1}, {0, 1, 1}, {2, 1, 1}, {1, 1, 1},  // L R U D F B C
    {1, 0, 0}, {1, 0, 2}, {1, 2, 2}, {1, 2, 0},                                 // z0..z3
    {0, 1, 0}, {0, 1, 2}, {2, 1, 2}, {2, 1, 0},                                 // y0..y3
    {0, 0, 1}, {0, 2, 1}, {2, 2, 1}, {2, 0, 1}};                                // x0..x3
__constant__ int8_t c_targets2[5][2] = {{1, 0}, {1, 2}, {0, 1}, {2, 1}, {1, 1}};  // image/utils.py:40-44

template <typename T, typename I>
__global__ void __launch_bounds__(kThreads) targets_kernel(const T* __restrict__ in, I B, E3<I> n, I C,
                                                         int nsp, T* __restrict__ out, I total) {
  const int K = nsp == 3 ? 19 : 5;
  const I c0 = nsp == 3 ? (n.e[0] - 1) / 2 : 1, c1 = (n.e[1] - 1) / 2, c2 = (n.e[2] - 1) / 2;
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < total; t += (I)gridDim.x * blockDim.x) {
    IdxT<I> q = unflat_t<I>(t, c0, c1, c2, C);
    const I cell = ((q.b * c0 + q.i0) * c1 + q.i1) * c2 + q.i2;
    for (int k = 0; k < K; ++k) {
      int dz, dy, dx;
      if (nsp == 3) { dz = c_targets3[k][0]; dy = c_targets3[k][1]; dx = c_targets3[k][2]; }
      else { dz = 0; dy = c_targets2[k][0]; dx = c_targets2[k][1]; }
      const I z = nsp == 3 ? 2 * q.i0 + dz : 0, y = 2 * q.i1 + dy, x = 2 * q.i2 + dx;
      out[(cell * K + k) * C + q.c] = in[(((q.b * n.e[0] + z) * n.e[1] + y) * n.e[2] + x) * C + q.c];
    }
  }
}

// features_from_lowres: [B, S-2p-1..., N, C], N = (2p+2)^d, offsets z-major then y, x.
template <typename T, typename I>
__global__ void __launch_bounds__(kThreads) features_kernel(const T* __restrict__ in, I B, E3<I> S, I C,
                                                          int nsp, int p, T* __restrict__ out, I total) {
  const int k = 2 * p + 2;
  const int kz = nsp == 3 ? k : 1;
  const int N = kz * k * k;
  const I c0 = nsp == 3 ? S.e[0] - 2 * p - 1 : 1, c1 = S.e[1] - 2 * p - 1, c2 = S.e[2] - 2 * p - 1;
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < total; t += (I)gridDim.x * blockDim.x) {
    IdxT<I> q = unflat_t<I>(t, c0, c1, c2, C);
    const I cell = ((q.b * c0 + q.i0) * c1 + q.i1) * c2 + q.i2;
    int f = 0;
    for (int dz = 0; dz < kz; ++dz)
      for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx, ++f) {
          const I z = q.i0 + dz, y = q.i1 + dy, x = q.i2 + dx;
          out[(cell * N + f) * C + q.c] = in[(((q.b * S.e[0] + z) * S.e[1] + y) * S.e[2] + x) * C + q.c];
        }
  }
}

// C == 1, 32-bit indices, compile-time neighbourhood: one cell per thread, its N features
// gathered into registers and written as 16-byte vectors (or one 4 / 8-byte store when the whole
// cell is smaller); the output is 16-byte aligned.
template <typename T, int NSP, int P>
__global__ void __launch_bounds__(kThreads) features_vec_kernel(const T* __restrict__ in, int32_t S0, int32_t S1,
                                                              int32_t S2, T* __restrict__ out, int32_t cells) {
  constexpr int K = 2 * P + 2, KZ = NSP == 3 ? K : 1, N = KZ * K * K;
  constexpr int NB = N * (int)sizeof(T);
  constexpr int SB = NB >= 16 ? 16 : NB;  // store width: 16 bytes, or the whole cell when smaller
  static_assert(NB % SB == 0 && (SB == 16 || SB == 8 || SB == 4), "whole stores per cell");
  using SV = typename std::conditional<SB == 16, uint4, typename std::conditional<SB == 8, uint2, uint32_t>::type>::type;
  const int32_t c0 = NSP == 3 ? S0 - 2 * P - 1 : 1, c1 = S1 - 2 * P - 1, c2 = S2 - 2 * P - 1;
  for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < cells; t += gridDim.x * blockDim.x) {
    uint32_t q = (uint32_t)t;
    const int32_t x = q % (uint32_t)c2; q /= (uint32_t)c2;
    const int32_t y = q % (uint32_t)c1; q /= (uint32_t)c1;
    const int32_t z = q % (uint32_t)c0;
    const int32_t b = q / (uint32_t)c0;
    const T* base = in + ((b * S0 + z) * S1 + y) * S2 + x;
    T f[N];
#pragma unroll
    for (int dz = 0; dz < KZ; ++dz)
#pragma unroll
      for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) f[(dz * K + dy) * K + dx] = base[(dz * S1 + dy) * S2 + dx];
    SV* o = (SV*)(out + (int64_t)t * N);
#pragma unroll
    for (int v = 0; v < NB / SB; ++v) {
      SV w;
      __builtin_memcpy(&w, (const char*)f + v * SB, SB);
      o[v] = w;
    }
  }
}

// ------------------------------------------------------------------------------------------
// jnp.pad on the spatial axes ('symmetric' / 'reflect'); negative pads crop.
// ------------------------------------------------------------------------------------------
template <typename I>
__device__ __forceinline__ I reflect_index(I i, I n) {
  if (n == 1) return 0;
  const I per = 2 * (n - 1);
  I m = i % per;
  if (m < 0) m += per;
  return m < n ? m : per - m;
}

template <typename T, typename I>
__global__ void __launch_bounds__(kThreads) pad_kernel(const T* __restrict__ in, I B, E3<I> n, I C,
                                                     E3<I> lo, E3<I> out_e, int mode, T* __restrict__ out,
                                                     I total) {
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < total; t += (I)gridDim.x * blockDim.x) {
    IdxT<I> q = unflat_t<I>(t, out_e.e[0], out_e.e[1], out_e.e[2], C);
    const I o[3] = {q.i0, q.i1, q.i2};
    I s[3];
    for (int a = 0; a < 3; ++a) {
      const I i = o[a] - lo.e[a];
      s[a] = (i >= 0 && i < n.e[a]) ? i : (mode == 0 ? sym_idx<I>(i, n.e[a]) : reflect_index<I>(i, n.e[a]));
    }
    out[t] = in[(((q.b * n.e[0] + s[0]) * n.e[1] + s[1]) * n.e[2] + s[2]) * C + q.c];
  }
}

// ------------------------------------------------------------------------------------------
// Coders (utils.py:28-55), one element per thread.
// ------------------------------------------------------------------------------------------
// 16-byte vector form for operands and result of one element size (the common case: the coder
// of the sample dtype on same-dtype predictions), 16-byte aligned; ``n16`` vectors.
template <int DIR, int CODER, typename TV>
__global__ void __launch_bounds__(kThreads) code_vec_kernel(const u32x4v* __restrict__ pred,
                                                          const u32x4v* __restrict__ x, int64_t n16,
                                                          u32x4v* __restrict__ out) {
  using TO = typename coder_out<CODER>::type;
  constexpr int V = 16 / sizeof(TV);
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n16; t += (int64_t)gridDim.x * blockDim.x) {
    const u32x4v pv = __builtin_nontemporal_load(pred + t), xv = __builtin_nontemporal_load(x + t);
    const TV* pp = (const TV*)&pv;
    const TV* xx = (const TV*)&xv;
    u32x4v ov;
    TO* oo = (TO*)&ov;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int32_t p = to_i32(pp[i]), v = to_i32(xx[i]);
      oo[i] = DIR == KMP_ENCODE ? code_encode<CODER>(p, v) : code_decode<CODER>(p, v);
    }
    __builtin_nontemporal_store(ov, out + t);
  }
}

template <int DIR, int CODER, typename TP, typename TX, typename I>
__global__ void __launch_bounds__(kThreads) code_kernel(const TP* __restrict__ pred, const TX* __restrict__ x, I n,
                                                      typename coder_out<CODER>::type* __restrict__ out) {
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < n; t += (I)gridDim.x * blockDim.x) {
    const int32_t p = to_i32(pred[t]);
    const int32_t v = to_i32(x[t]);
    out[t] = DIR == KMP_ENCODE ? code_encode<CODER>(p, v) : code_decode<CODER>(p, v);
  }
}

// Near-lossless coders (kmp_common.h), one element per thread.  ``pred`` holds the sample dtype's bit
// patterns or float32, ``x`` the samples (encode) or the stored W-bit residuals (decode); SGN: the
// samples are signed, so samples and predictions are taken through M and a decode stores M^-1 of
// its result.  A float32 prediction is truncated and clamped to the sample type's own range.
template <int DIR, int CODER, bool SGN, typename TP>
__global__ void __launch_bounds__(kThreads) code_near_kernel(const TP* __restrict__ pred,
                                                           const typename coder_out<CODER>::type* __restrict__ x,
                                                           int64_t n, typename coder_out<CODER>::type* __restrict__ out,
                                                           NearQ q) {
  using TO = typename coder_out<CODER>::type;
  constexpr int32_t MAX = (int32_t)std::numeric_limits<TO>::max();
  constexpr int32_t HALF = SGN ? (MAX + 1) / 2 : 0;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    int32_t p;
    if constexpr (std::is_same<TP, float>::value) {
      p = to_i32(pred[t]);
      p = p < -HALF ? 0 : (p > MAX - HALF ? MAX : p + HALF);
    } else {
      p = (int32_t)(TO)(pred[t] ^ (TO)HALF);
    }
    if constexpr (DIR == KMP_ENCODE) out[t] = coder_enc<CODER>(q, p, (int32_t)(TO)(x[t] ^ (TO)HALF));
    else out[t] = (TO)(coder_dec<CODER>(q, p, (int32_t)x[t]) ^ (TO)HALF);
  }
}

// Error-bounded float32 quantisers (KMP_CODER_QUANT_I16 / _I32).  The step is a power
// of two, so the float64 products are exact and the one rounding is the final conversion to float32:
// the same bits as tests/quant_spec.py on any device.  An exception (not finite, out of the integer
// type's range, or further than eps from its restored value) is written as the type's minimum.
struct QuantP {
  double inv, step, eps;  // 2^-e, 2^e, 2^(e-1)
};

template <typename TN>
__device__ __forceinline__ TN quant_one(float x, const QuantP& q) {
  constexpr double QMAX = (double)std::numeric_limits<TN>::max();
  const double xd = (double)x;
  const double n = __builtin_rint(xd * q.inv);  // NaN and infinities stay what they are
  const float r = (float)(n * q.step);
  // every comparison is false for a NaN; an infinite x gives an infinite n
  const bool ok = __builtin_fabs(n) <= QMAX && __builtin_fabsf(r) <= std::numeric_limits<float>::max() &&
                  __builtin_fabs((double)r - xd) <= q.eps;
  return ok ? (TN)(int32_t)n : std::numeric_limits<TN>::min();
}

template <typename TN>
__device__ __forceinline__ float dequant_one(TN n, const QuantP& q) {
  return (float)((double)n * q.step);
}

// element form: any alignment, any count
template <int DIR, typename TN>
__global__ void __launch_bounds__(kThreads) quant_kernel(const void* __restrict__ x, int64_t n, void* __restrict__ out,
                                                       QuantP q) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (DIR == KMP_ENCODE) ((TN*)out)[t] = quant_one<TN>(((const float*)x)[t], q);
    else ((float*)out)[t] = dequant_one<TN>(((const TN*)x)[t], q);
  }
}

// vector form: one item = four elements, a 16-byte access on the float32 side and an 8- (int16) or
// 16-byte (int32) one on the integer side, both aligned to their size; ``n4`` items
template <int DIR, typename TN>
__global__ void __launch_bounds__(kThreads) quant_vec_kernel(const void* __restrict__ x, int64_t n4,
                                                           void* __restrict__ out, QuantP q) {
  using NV = typename std::conditional<sizeof(TN) == 2, u32x2v, u32x4v>::type;  // four TN
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n4; t += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (DIR == KMP_ENCODE) {
      const u32x4v xv = __builtin_nontemporal_load((const u32x4v*)x + t);
      const float* xx = (const float*)&xv;
      NV ov;
      TN* oo = (TN*)&ov;
#pragma unroll
      for (int i = 0; i < 4; ++i) oo[i] = quant_one<TN>(xx[i], q);
      __builtin_nontemporal_store(ov, (NV*)out + t);
    } else {
      const NV xv = __builtin_nontemporal_load((const NV*)x + t);
      const TN* xx = (const TN*)&xv;
      u32x4v ov;
      float* oo = (float*)&ov;
#pragma unroll
      for (int i = 0; i < 4; ++i) oo[i] = dequant_one<TN>(xx[i], q);
      __builtin_nontemporal_store(ov, (u32x4v*)out + t);
    }
  }
}

// Relative-error float32 quantisers (KMP_CODER_PREC_I16 / _I32): keep the top m mantissa
// bits, rounded to nearest even, by shifts, adds and compares on the bit pattern -- ``t`` = 23 - m and
// ``rnd`` = 2^(t-1) - 1 are kernel arguments.  The float32 side is loaded and stored as uint32 and no
// floating-point instruction runs, so NaN payloads and subnormals pass whatever the mode registers
// say: the same bits as tests/prec_spec.py on any device.  An exception (not finite, rounds up to
// infinity, or out of the integer type's range) is written as the type's minimum.
template <typename TN>
__device__ __forceinline__ TN prec_one(uint32_t u, uint32_t t, uint32_t rnd) {
  constexpr uint32_t QMAX = (uint32_t)std::numeric_limits<TN>::max();
  const uint32_t a = u & 0x7fffffffu;
  const uint32_t k = (a + rnd + ((a >> t) & 1u)) >> t;  // a + 2^22 < 2^32: no carry out
  const bool exc = a >= 0x7f800000u || (k << t) >= 0x7f800000u || k > QMAX;
  const int32_t n = (u >> 31) ? -(int32_t)k : (int32_t)k;
  return exc ? std::numeric_limits<TN>::min() : (TN)n;
}

// total over every integer: |n| as uint32 (2^15 / 2^31 for the type's minimum), the exponent's carry masked
template <typename TN>
__device__ __forceinline__ uint32_t unprec_one(TN n, uint32_t t) {
  const int32_t v = (int32_t)n;
  const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  return ((mag << t) & 0x7fffffffu) | (v < 0 ? 0x80000000u : 0u);
}

// element form: any alignment, any count.  The loop is left as written: interleaved or unrolled, a
// grid-stride loop divides for its trip count, and the compiler does that with a floating-point
// reciprocal -- on the index, not the data, but these kernels hold no such instruction at all; one
// pass covers 2^24 elements, so there is little to interleave
template <int DIR, typename TN>
__global__ void __launch_bounds__(kThreads) prec_kernel(const void* __restrict__ x, int64_t n, void* __restrict__ out,
                                                      uint32_t t, uint32_t rnd) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (DIR == KMP_ENCODE) ((TN*)out)[i] = prec_one<TN>(((const uint32_t*)x)[i], t, rnd);
    else ((uint32_t*)out)[i] = unprec_one<TN>(((const TN*)x)[i], t);
  }
}

// vector form: one item = four elements, a 16-byte access on the float32 side and an 8- (int16) or
// 16-byte (int32) one on the integer side, both aligned to their size; ``n4`` items
template <int DIR, typename TN>
__global__ void __launch_bounds__(kThreads) prec_vec_kernel(const void* __restrict__ x, int64_t n4,
                                                          void* __restrict__ out, uint32_t t, uint32_t rnd) {
  using NV = typename std::conditional<sizeof(TN) == 2, u32x2v, u32x4v>::type;  // four TN
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (DIR == KMP_ENCODE) {
      const u32x4v xv = __builtin_nontemporal_load((const u32x4v*)x + i);
      NV ov;
      TN* oo = (TN*)&ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) oo[j] = prec_one<TN>(xv[j], t, rnd);
      __builtin_nontemporal_store(ov, (NV*)out + i);
    } else {
      const NV xv = __builtin_nontemporal_load((const NV*)x + i);
      const TN* xx = (const TN*)&xv;
      u32x4v ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = unprec_one<TN>(xx[j], t);
      __builtin_nontemporal_store(ov, (u32x4v*)out + i);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Box copy with conversion (slicing / .at[box].set of the chunk driver)
// ------------------------------------------------------------------------------------------
template <typename TO, typename TI>
__device__ __forceinline__ TO convert(TI v) {
  if constexpr (std::is_same<TI, float>::value && !std::is_same<TO, float>::value) return cast_f32<TO>(v);
  else return (TO)v;
}

template <typename TI, typename TO, typename I>
__global__ void __launch_bounds__(kThreads) copy_box_kernel(const TI* __restrict__ in, E3<I> in_e, E3<I> in_off,
                                                          TO* __restrict__ out, E3<I> out_e, E3<I> out_off, E3<I> ext,
                                                          I C, I total) {
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < total; t += (I)gridDim.x * blockDim.x) {
    IdxT<I> q = unflat_t<I>(t, ext.e[0], ext.e[1], ext.e[2], C);
    const I si = (((q.b * in_e.e[0] + in_off.e[0] + q.i0) * in_e.e[1] + in_off.e[1] + q.i1) * in_e.e[2] +
                        in_off.e[2] + q.i2) * C + q.c;
    const I so = (((q.b * out_e.e[0] + out_off.e[0] + q.i0) * out_e.e[1] + out_off.e[1] + q.i1) * out_e.e[2] +
                        out_off.e[2] + q.i2) * C + q.c;
    out[so] = convert<TO>(in[si]);
  }
}

// ------------------------------------------------------------------------------------------
// Row kernels (C == 1, < 2^31 elements): one work item = V = 16 / sizeof(T) consecutive outputs
// of one row.  The row decomposition (3 divisions) is paid once per 16 bytes instead of once per
// element, and interior chunks move as one 16-byte load / store per lane.  Rows of these arrays
// have odd lengths (65, 33, ...), so row starts are only element-aligned: the vectors are
// declared byte-aligned and gfx950 serves them as unaligned dwordx4 accesses.  Partial chunks
// and mirrored edges fall back to per-element accesses inside the same item.
// ------------------------------------------------------------------------------------------
// jnp.pad rows: out[b, z, y, x] = in[b, m(z - lz), m(y - ly), m(x - lx)]
template <typename T>
__global__ void __launch_bounds__(kThreads) rows_pad_kernel(const T* __restrict__ in, E3<int32_t> n, E3<int32_t> lo,
                                                          E3<int32_t> oe, int mode, T* __restrict__ out, int32_t nch,
                                                          int32_t items) {
  constexpr int V = Vec16<T>::V;
  auto m = [&](int32_t i, int32_t ext) { return (i >= 0 && i < ext) ? i : (mode == 0 ? sym_idx<int32_t>(i, ext)
                                                                                      : reflect_index<int32_t>(i, ext)); };
  for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < items; t += gridDim.x * kThreads) {
    const RowItem q = row_item((uint32_t)t, oe.e[0], oe.e[1], nch);
    const int32_t sz = m(q.z - lo.e[0], n.e[0]), sy = m(q.y - lo.e[1], n.e[1]);
    const T* src = in + ((q.b * n.e[0] + sz) * n.e[1] + sy) * n.e[2];
    T* dst = out + ((q.b * oe.e[0] + q.z) * oe.e[1] + q.y) * oe.e[2];
    const int32_t x0 = q.j * V, s0 = x0 - lo.e[2];
    if (x0 + V <= oe.e[2] && s0 >= 0 && s0 + V <= n.e[2]) {
      Vec16<T> v;
      v.load(src + s0);
      v.store(dst + x0);
    } else {
      for (int32_t x = x0; x < x0 + V && x < oe.e[2]; ++x) dst[x] = src[m(x - lo.e[2], n.e[2])];
    }
  }
}

// Parity split of highres rows (lowres_from_highres / maps_from_highres): item = (b, hz, hy)
// highres row (every ``step``-th when only the lowres is wanted), chunk j = highres x in
// [2jV, 2jV + 2V): even x -> class (pz, py, 0), odd x -> class (pz, py, 1).
template <typename T>
__global__ void __launch_bounds__(kThreads) rows_deinterleave_kernel(const T* __restrict__ in, E3<int32_t> n, int nsp,
                                                                   int step, T* lowres, MapPtrs outs, int32_t nch,
                                                                   int32_t items) {
  constexpr int V = Vec16<T>::V;
  const int32_t rz = (n.e[0] + step - 1) / step, ry = (n.e[1] + step - 1) / step;
  for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < items; t += gridDim.x * kThreads) {
    const RowItem q = row_item((uint32_t)t, rz, ry, nch);
    const int32_t hz = q.z * step, hy = q.y * step;
    const int pz = (nsp == 3) ? (hz & 1) : 0, py = hy & 1;
    T* dst[2] = {nullptr, nullptr};
    int32_t ex[2];
    int32_t ez = nsp == 3 ? (pz ? n.e[0] / 2 : (n.e[0] + 1) / 2) : 1, ey = py ? n.e[1] / 2 : (n.e[1] + 1) / 2;
    ex[0] = (n.e[2] + 1) / 2;
    ex[1] = n.e[2] / 2;
    const int32_t orow = (q.b * ez + (hz >> 1)) * ey + (hy >> 1);
    if (pz == 0 && py == 0 && lowres) dst[0] = (T*)lowres + orow * ex[0];
    if (outs.p[0]) {
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        if (k >= (nsp == 3 ? 7 : 3)) break;
        int par[3];
        map_parity(nsp, k, par);
        if (par[0] == pz && par[1] == py) dst[par[2]] = (T*)outs.p[k] + orow * ex[par[2]];
      }
    }
    const T* src = in + ((q.b * n.e[0] + hz) * n.e[1] + hy) * n.e[2];
    const int32_t x0 = q.j * V;
    if (2 * x0 + 2 * V <= n.e[2]) {
      Vec16<T> a, b, ev, od;
      a.load(src + 2 * x0);
      b.load(src + 2 * x0 + V);
#pragma unroll
      for (int i = 0; i < V / 2; ++i) {
        ev.e[i] = a.e[2 * i]; od.e[i] = a.e[2 * i + 1];
        ev.e[V / 2 + i] = b.e[2 * i]; od.e[V / 2 + i] = b.e[2 * i + 1];
      }
      if (dst[0]) ev.store(dst[0] + x0);
      if (dst[1]) od.store(dst[1] + x0);
    } else {
      for (int32_t x = 2 * x0; x < 2 * x0 + 2 * V && x < n.e[2]; ++x)
        if (dst[x & 1]) dst[x & 1][x >> 1] = src[x];
    }
  }
}

// Parity merge (highres_from_lowres_and_maps): item = highres row (b, hz, hy), chunk j = highres x
// in [2jV, 2jV + 2V) from class (pz, py, 0) (lowres when pz = py = 0) and class (pz, py, 1).
template <typename T>
__global__ void __launch_bounds__(kThreads) rows_interleave_kernel(const T* __restrict__ lowres, CMapPtrs maps,
                                                                 E3<int32_t> L, int nsp, T* __restrict__ out,
                                                                 int32_t nch, int32_t items) {
  constexpr int V = Vec16<T>::V;
  const int32_t h0 = 2 * L.e[0] - 1, h1 = 2 * L.e[1] - 1, h2 = 2 * L.e[2] - 1;
  for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < items; t += gridDim.x * kThreads) {
    const RowItem q = row_item((uint32_t)t, h0, h1, nch);
    const int pz = (nsp == 3) ? (q.z & 1) : 0, py = q.y & 1;
    const T* srcp[2] = {nullptr, nullptr};
    const int32_t ez = nsp == 3 ? (pz ? L.e[0] - 1 : L.e[0]) : 1, ey = py ? L.e[1] - 1 : L.e[1];
    const int32_t ex[2] = {L.e[2], L.e[2] - 1};
    const int32_t irow = (q.b * ez + (q.z >> 1)) * ey + (q.y >> 1);
    if (pz == 0 && py == 0) srcp[0] = lowres + irow * ex[0];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      if (k >= (nsp == 3 ? 7 : 3)) break;
      int par[3];
      map_parity(nsp, k, par);
      if (par[0] == pz && par[1] == py) srcp[par[2]] = (const T*)maps.p[k] + irow * ex[par[2]];
    }
    T* dst = out + ((q.b * h0 + q.z) * h1 + q.y) * h2;
    const int32_t x0 = q.j * V;
    if (x0 + V <= ex[1]) {
      Vec16<T> ev, od, a, b;
      ev.load(srcp[0] + x0);
      od.load(srcp[1] + x0);
#pragma unroll
      for (int i = 0; i < V / 2; ++i) {
        a.e[2 * i] = ev.e[i]; a.e[2 * i + 1] = od.e[i];
        b.e[2 * i] = ev.e[V / 2 + i]; b.e[2 * i + 1] = od.e[V / 2 + i];
      }
      a.store(dst + 2 * x0);
      b.store(dst + 2 * x0 + V);
    } else {
      for (int32_t x = 2 * x0; x < 2 * x0 + 2 * V && x < h2; ++x) dst[x] = srcp[x & 1][x >> 1];
    }
  }
}

// Same-dtype box copy (slicing / .at[box].set of the chunk driver, trims)
template <typename T>
__global__ void __launch_bounds__(kThreads) rows_copy_kernel(const T* __restrict__ in, E3<int32_t> ie, E3<int32_t> io,
                                                           T* __restrict__ out, E3<int32_t> oe, E3<int32_t> oo,
                                                           E3<int32_t> ext, int32_t nch, int32_t items) {
  constexpr int V = Vec16<T>::V;
  for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < items; t += gridDim.x * kThreads) {
    const RowItem q = row_item((uint32_t)t, ext.e[0], ext.e[1], nch);
    const T* src = in + ((q.b * ie.e[0] + io.e[0] + q.z) * ie.e[1] + io.e[1] + q.y) * ie.e[2] + io.e[2];
    T* dst = out + ((q.b * oe.e[0] + oo.e[0] + q.z) * oe.e[1] + oo.e[1] + q.y) * oe.e[2] + oo.e[2];
    const int32_t x0 = q.j * V;
    if (x0 + V <= ext.e[2]) {
      Vec16<T> v;
      v.load(src + x0);
      v.store(dst + x0);
    } else {
      for (int32_t x = x0; x < ext.e[2]; ++x) dst[x] = src[x];
    }
  }
}

// The parity split behind lowres_from_highres (``lowres`` set: every second highres row) and
// maps_from_highres (``outs`` set: every row).
static int deinterleave_launch(const char* name, int nsp, int dtype, const void* in, int64_t B, const Ext3& n,
                               int64_t C, void* lowres, const MapPtrs& outs, hipStream_t stream) {
  const int64_t total = B * ((n.e[0] + 1) / 2) * ((n.e[1] + 1) / 2) * ((n.e[2] + 1) / 2) * C;
  if (total == 0) return KMP_OK;
  const int step = lowres ? 2 : 1;
  return dispatch_any_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (rows_ok(C, {vol(B, n, C)})) {
      const int32_t nch = row_chunks<T>((n.e[2] + 1) / 2);
      const int64_t items = B * ceil_div(n.e[0], step) * ceil_div(n.e[1], step) * nch;
      rows_deinterleave_kernel<T><<<grid_for(items), kThreads, 0, stream>>>((const T*)in, e32(n), nsp, step, (T*)lowres,
                                                                            outs, nch, (int32_t)items);
    } else {
      with_index(fits32({vol(B, n, C)}), [&](auto itag) {
        using I = decltype(itag);
        deinterleave_kernel<T, I><<<grid_for(total), kThreads, 0, stream>>>((const T*)in, (I)B, e3<I>(n), (I)C, nsp,
                                                                            outs, lowres, (I)total);
      });
    }
    return check_launch(name);
  });
}

}  // namespace kmp

using namespace kmp;

extern "C" {

int kmp_device_ok(void) {
  // The real requirement: this library's code object loads on the current device (gfx950).
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_error(std::string("no HIP device visible: ") + hipGetErrorString(e));
    return 0;
  }
  hipFuncAttributes attr;
  e = hipFuncGetAttributes(&attr, (const void*)&pad_kernel<uint8_t, int32_t>);
  if (e != hipSuccess) {
    set_error(std::string("libkompressor_hip has no code object for this device (built for gfx950): ") +
              hipGetErrorString(e));
    return 0;
  }
  return 1;
}

int kmp_lowres_from_highres(int32_t nsp, int32_t dtype, const void* in, int64_t B, const int64_t shape[3],
                            int64_t C, void* out, kmp_stream_t stream) {
  if (int s = check_common(nsp, B, shape, C)) return s;
  KMP_REQUIRE(in && out, "null pointer");
  return deinterleave_launch("lowres_from_highres", nsp, dtype, in, B, ext_from(nsp, shape), C, out, MapPtrs{},
                             (hipStream_t)stream);
}

int kmp_maps_from_highres(int32_t nsp, int32_t dtype, const void* in, int64_t B, const int64_t shape[3], int64_t C,
                          void* const out[7], kmp_stream_t stream) {
  if (int s = check_common(nsp, B, shape, C)) return s;
  KMP_REQUIRE(in && out, "null pointer");
  MapPtrs outs{};
  KMP_REQUIRE(bind_maps(nsp, out, outs), "null map pointer");
  return deinterleave_launch("maps_from_highres", nsp, dtype, in, B, ext_from(nsp, shape), C, nullptr, outs,
                             (hipStream_t)stream);
}

int kmp_targets_from_highres(int32_t nsp, int32_t dtype, const void* in, int64_t B, const int64_t shape[3], int64_t C,
                             void* out, kmp_stream_t stream) {
  if (int s = check_common(nsp, B, shape, C)) return s;
  KMP_REQUIRE(in && out, "null pointer");
  Ext3 n = ext_from(nsp, shape);
  const int64_t c0 = nsp == 3 ? (n.e[0] - 1) / 2 : 1;
  const int64_t total = B * c0 * ((n.e[1] - 1) / 2) * ((n.e[2] - 1) / 2) * C;
  if (total <= 0) return KMP_OK;
  return dispatch_any_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return with_index(fits32({vol(B, n, C), total * (nsp == 3 ? 19 : 5)}), [&](auto itag) {
      using I = decltype(itag);
      targets_kernel<T, I><<<grid_for(total), kThreads, 0, (hipStream_t)stream>>>((const T*)in, (I)B, e3<I>(n), (I)C,
                                                                                  nsp, (T*)out, (I)total);
      return check_launch("targets_from_highres");
    });
  });
}

int kmp_highres_from_lowres_and_maps(int32_t nsp, int32_t dtype, const void* lowres, const void* const maps[7],
                                     int64_t B, const int64_t lshape[3], int64_t C, void* out, kmp_stream_t stream) {
  if (int s = check_common(nsp, B, lshape, C)) return s;
  KMP_REQUIRE(lowres && maps && out, "null pointer");
  Ext3 L = ext_from(nsp, lshape);
  CMapPtrs mp{};
  KMP_REQUIRE(bind_maps(nsp, maps, mp), "null map pointer");
  const int64_t total = B * L.e[0] * L.e[1] * L.e[2] * C;
  if (total == 0) return KMP_OK;
  return dispatch_any_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const Ext3 H{{2 * L.e[0] - 1, 2 * L.e[1] - 1, 2 * L.e[2] - 1}};
    if (rows_ok(C, {vol(B, H, C)})) {
      const int32_t nch = row_chunks<T>(L.e[2]);
      const int64_t items = B * H.e[0] * H.e[1] * nch;
      rows_interleave_kernel<T><<<grid_for(items), kThreads, 0, (hipStream_t)stream>>>(
          (const T*)lowres, mp, e32(L), nsp, (T*)out, nch, (int32_t)items);
    } else {
      with_index(fits32({vol(B, H, C)}), [&](auto itag) {
        using I = decltype(itag);
        interleave_kernel<T, I><<<grid_for(total), kThreads, 0, (hipStream_t)stream>>>(
            (const T*)lowres, mp, (I)B, e3<I>(L), (I)C, nsp, (T*)out, (I)total);
      });
    }
    return check_launch("highres_from_lowres_and_maps");
  });
}

int kmp_features_from_lowres(int32_t nsp, int32_t dtype, const void* lowres, int64_t B, const int64_t shape[3],
                             int64_t C, int32_t padding, void* out, kmp_stream_t stream) {
  if (int s = check_common(nsp, B, shape, C)) return s;
  KMP_REQUIRE(lowres && out && padding >= 0, "null pointer or negative padding");
  Ext3 S = ext_from(nsp, shape);
  int64_t cells = B * C;
  for (int a = 3 - nsp; a < 3; ++a) {
    KMP_REQUIRE(S.e[a] - 2 * padding - 1 >= 0, "window smaller than the neighbourhood");
    cells *= S.e[a] - 2 * padding - 1;
  }
  if (cells == 0) return KMP_OK;
  return dispatch_any_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const int k = 2 * padding + 2;
    const bool small = fits32({vol(B, S, C), cells * (nsp == 3 ? k * k * k : k * k)});
    if constexpr (sizeof(T) <= 2) {
      if (small && C == 1 && ((uintptr_t)out & 15) == 0 && padding <= 1) {
        auto kern = nsp == 3 ? (padding == 0 ? features_vec_kernel<T, 3, 0> : features_vec_kernel<T, 3, 1>)
                             : (padding == 0 ? features_vec_kernel<T, 2, 0> : features_vec_kernel<T, 2, 1>);
        kern<<<grid_for(cells), kThreads, 0, (hipStream_t)stream>>>((const T*)lowres, (int32_t)S.e[0], (int32_t)S.e[1],
                                                                    (int32_t)S.e[2], (T*)out, (int32_t)cells);
        return check_launch("features_from_lowres");
      }
    }
    return with_index(small, [&](auto itag) {
      using I = decltype(itag);
      features_kernel<T, I><<<grid_for(cells), kThreads, 0, (hipStream_t)stream>>>((const T*)lowres, (I)B, e3<I>(S),
                                                                                   (I)C, nsp, padding, (T*)out,
                                                                                   (I)cells);
      return check_launch("features_from_lowres");
    });
  });
}

int kmp_pad(int32_t nsp, int32_t dtype, const void* in, int64_t B, const int64_t shape[3], int64_t C,
            const int64_t pad_lo[3], const int64_t pad_hi[3], int32_t mode, void* out, kmp_stream_t stream) {
  if (int s = check_common(nsp, B, shape, C)) return s;
  KMP_REQUIRE(in && out && pad_lo && pad_hi && (mode == 0 || mode == 1), "bad pointer or mode");
  Ext3 n = ext_from(nsp, shape);
  Ext3 lo{}, oe{};
  int64_t total = B * C;
  for (int a = 0; a < 3; ++a) {
    if (a < 3 - nsp) { lo.e[a] = 0; oe.e[a] = 1; continue; }
    const int i = a - (3 - nsp);
    lo.e[a] = pad_lo[i];
    oe.e[a] = n.e[a] + pad_lo[i] + pad_hi[i];
    KMP_REQUIRE(oe.e[a] >= 0, "pads remove more than the extent");
    KMP_REQUIRE(n.e[a] > 0 || oe.e[a] == 0, "cannot pad an empty axis");
    total *= oe.e[a];
  }
  if (total == 0) return KMP_OK;
  return dispatch_any_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (rows_ok(C, {vol(B, n, C), total})) {
      const int32_t nch = row_chunks<T>(oe.e[2]);
      const int64_t items = B * oe.e[0] * oe.e[1] * nch;
      rows_pad_kernel<T><<<grid_for(items), kThreads, 0, (hipStream_t)stream>>>(
          (const T*)in, e32(n), e32(lo), e32(oe), mode, (T*)out, nch, (int32_t)items);
    } else {
      with_index(fits32({vol(B, n, C), total}), [&](auto itag) {
        using I = decltype(itag);
        pad_kernel<T, I><<<grid_for(total), kThreads, 0, (hipStream_t)stream>>>(
            (const T*)in, (I)B, e3<I>(n), (I)C, e3<I>(lo), e3<I>(oe), mode, (T*)out, (I)total);
      });
    }
    return check_launch("pad");
  });
}

int kmp_copy_box(int32_t nsp, int32_t in_dtype, const void* in, const int64_t in_shape[3], const int64_t in_off[3],
                 int32_t out_dtype, void* out, const int64_t out_shape[3], const int64_t out_off[3], int64_t B,
                 int64_t C, const int64_t ext[3], kmp_stream_t stream) {
  if (int s = check_common(nsp, B, in_shape, C)) return s;
  if (int s = check_common(nsp, B, out_shape, C)) return s;
  KMP_REQUIRE(in && out && in_off && out_off && ext, "null pointer");
  Ext3 ie = ext_from(nsp, in_shape), oe = ext_from(nsp, out_shape);
  Ext3 io{}, oo{}, ee{};
  int64_t total = B * C;
  for (int a = 0; a < 3; ++a) {
    if (a < 3 - nsp) { io.e[a] = 0; oo.e[a] = 0; ee.e[a] = 1; continue; }
    const int i = a - (3 - nsp);
    io.e[a] = in_off[i]; oo.e[a] = out_off[i]; ee.e[a] = ext[i];
    KMP_REQUIRE(ext[i] >= 0 && in_off[i] >= 0 && out_off[i] >= 0 && in_off[i] + ext[i] <= ie.e[a] &&
                    out_off[i] + ext[i] <= oe.e[a], "box out of bounds");
    total *= ext[i];
  }
  if (total == 0) return KMP_OK;
  return dispatch_any_dtype(in_dtype, [&](auto itag) {
    using TI = decltype(itag);
    return dispatch_any_dtype(out_dtype, [&](auto otag) {
      using TO = decltype(otag);
      if constexpr (std::is_same<TI, TO>::value) {
        if (rows_ok(C, {vol(B, ie, C), vol(B, oe, C)})) {
          const int32_t nch = row_chunks<TI>(ee.e[2]);
          const int64_t items = B * ee.e[0] * ee.e[1] * nch;
          rows_copy_kernel<TI><<<grid_for(items), kThreads, 0, (hipStream_t)stream>>>(
              (const TI*)in, e32(ie), e32(io), (TO*)out, e32(oe), e32(oo), e32(ee), nch, (int32_t)items);
          return check_launch("copy_box");
        }
      }
      with_index(fits32({vol(B, ie, C), vol(B, oe, C)}), [&](auto itag) {
        using I = decltype(itag);
        copy_box_kernel<TI, TO, I><<<grid_for(total), kThreads, 0, (hipStream_t)stream>>>(
            (const TI*)in, e3<I>(ie), e3<I>(io), (TO*)out, e3<I>(oe), e3<I>(oo), e3<I>(ee), (I)C, (I)total);
      });
      return check_launch("copy_box");
    });
  });
}

int kmp_code(int32_t direction, int32_t coder, int32_t pred_dtype, const void* pred, int32_t x_dtype, const void* x,
             int64_t n, void* out, kmp_stream_t stream) {
  KMP_REQUIRE(direction == KMP_ENCODE || direction == KMP_DECODE, "bad direction");
  KMP_REQUIRE(n >= 0, "negative count");
  if (coder >= 0 && coder_code(coder) == KMP_CODER_COMPARE) {
    // error statistics (kmp_compare.hip): x the original, pred the restored array, nothing coded
    const int32_t field = coder >> 8;  // 0: start a record, 1: continue the one at out
    KMP_REQUIRE(pred, "compare: pred is the restored array (must not be NULL)");
    KMP_REQUIRE(direction == KMP_ENCODE, "compare: KMP_ENCODE alone");
    KMP_REQUIRE(field == 0 || field == 1, "compare: the mode field is 0 (start) or 1 (continue)");
    KMP_REQUIRE(pred_dtype == x_dtype, "compare: both arrays in one dtype");
    KMP_REQUIRE(x_dtype == KMP_F32 || x_dtype == KMP_U8 || x_dtype == KMP_U16 || x_dtype == KMP_I8 || x_dtype == KMP_I16,
                "compare takes float32, uint8, uint16, int8 or int16 samples");
    KMP_REQUIRE(((uintptr_t)out & 7) == 0, "compare: out must be 8-byte aligned");
    KMP_REQUIRE(dtype_size(x_dtype) != 2 || n < ((int64_t)1 << 32), "compare: 16-bit samples take n < 2^32");
    if (n == 0) return KMP_OK;
    KMP_REQUIRE(x && out, "null pointer");
    return launch_compare(x_dtype, x, pred, n, out, field, (hipStream_t)stream);
  }
  if (coder >= 0 && coder_code(coder) == KMP_CODER_SSIM) {
    // structural similarity (kmp_ssim.hip): x the original, pred the restored array, the request in out
    KMP_REQUIRE(pred, "ssim: pred is the restored array (must not be NULL)");
    KMP_REQUIRE(direction == KMP_ENCODE, "ssim: KMP_ENCODE alone");
    KMP_REQUIRE((coder >> 8) == 0, "ssim: the code carries no field");
    KMP_REQUIRE(pred_dtype == x_dtype, "ssim: both arrays in one dtype");
    KMP_REQUIRE(x_dtype == KMP_F32 || x_dtype == KMP_U8 || x_dtype == KMP_U16 || x_dtype == KMP_I8 || x_dtype == KMP_I16,
                "ssim takes float32, uint8, uint16, int8 or int16 samples");
    KMP_REQUIRE(((uintptr_t)out & 7) == 0, "ssim: out must be 8-byte aligned");
    if (n == 0) return KMP_OK;
    KMP_REQUIRE(x && out, "null pointer");
    KMP_REQUIRE((((uintptr_t)x | (uintptr_t)pred) & (uintptr_t)(dtype_size(x_dtype) - 1)) == 0,
                "ssim: arrays aligned to their dtype");
    return launch_ssim(x_dtype, x, pred, n, out, (hipStream_t)stream);
  }
  if (coder >= 0 && coder_code(coder) == KMP_CODER_FILL) {
    // hold-fill of a marked integer array (kmp_fill.hip): pred is the scratch
    const int64_t w = x_dtype == KMP_I16 ? 2 : 4;
    KMP_REQUIRE(direction == KMP_ENCODE, "fill: KMP_ENCODE alone");
    KMP_REQUIRE((coder >> 8) == 0, "fill: the code carries no field");
    KMP_REQUIRE(x_dtype == KMP_I16 || x_dtype == KMP_I32, "fill takes int16 or int32 arrays");
    KMP_REQUIRE(pred && ((uintptr_t)pred & 7) == 0, "fill: pred is the 8-byte aligned KMP_FILL_BYTES of scratch");
    if (n == 0) return KMP_OK;
    KMP_REQUIRE(x && out, "null pointer");
    KMP_REQUIRE((((uintptr_t)x | (uintptr_t)out) & (uintptr_t)(w - 1)) == 0, "fill: arrays aligned to their dtype");
    KMP_REQUIRE(n <= INT64_MAX / 8, "fill: count too large");
    KMP_REQUIRE(x == out || (uintptr_t)x + (uintptr_t)(n * w) <= (uintptr_t)out ||
                    (uintptr_t)out + (uintptr_t)(n * w) <= (uintptr_t)x, "fill: x and out overlap in part");
    return launch_fill(x_dtype, x, n, out, const_cast<void*>(pred), (hipStream_t)stream);
  }
  if (coder >= 0 && coder_code(coder) == KMP_CODER_RUNS) {
    // patch of a float32 array from a run table (kmp_fill.hip): bounds are the caller's duty
    KMP_REQUIRE(direction == KMP_DECODE, "runs: KMP_DECODE alone");
    KMP_REQUIRE((coder >> 8) == 0, "runs: the code carries no field");
    KMP_REQUIRE(x_dtype == KMP_U32, "runs: the table is uint32 (x_dtype KMP_U32)");
    KMP_REQUIRE(!pred, "runs takes no prediction (pred must be NULL)");
    if (n == 0) return KMP_OK;
    KMP_REQUIRE(x && out, "null pointer");
    KMP_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0,
                "runs: a 16-byte aligned table and a 4-byte aligned array");
    return launch_runs(x, n, out, (hipStream_t)stream);
  }
  if (coder >= 0 && coder_code(coder) == KMP_CODER_DELTA) {
    // x - pred / x + pred modulo 2^W of two integer arrays of one dtype (kmp_delta.hip)
    KMP_REQUIRE(pred, "delta: pred is the other array (must not be NULL)");
    KMP_REQUIRE((coder >> 8) == 0, "delta: the code carries no field");
    KMP_REQUIRE(pred_dtype == x_dtype, "delta: both arrays in one dtype");
    KMP_REQUIRE(x_dtype == KMP_U8 || x_dtype == KMP_I8 || x_dtype == KMP_U16 || x_dtype == KMP_I16 || x_dtype == KMP_I32,
                "delta takes uint8, int8, uint16, int16 or int32 samples");
    if (n == 0) return KMP_OK;
    KMP_REQUIRE(x && out, "null pointer");
    const int64_t w = (int64_t)dtype_size(x_dtype);
    KMP_REQUIRE((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)out) & (uintptr_t)(w - 1)) == 0,
                "delta: arrays aligned to their dtype");
    KMP_REQUIRE(n <= INT64_MAX / 8, "delta: count too large");
    const uintptr_t nb = (uintptr_t)(n * w), xa = (uintptr_t)x, pa = (uintptr_t)pred, oa = (uintptr_t)out;
    KMP_REQUIRE(x == out || xa + nb <= oa || oa + nb <= xa, "delta: x and out overlap in part");
    KMP_REQUIRE(pa + nb <= oa || oa + nb <= pa, "delta: pred and out overlap");
    return launch_delta(direction, (int)w, pred, x, n, out, (hipStream_t)stream);
  }
  if (coder >= 0 && is_quant_code(coder_code(coder))) {
    // float32 <-> int16 / int32 on a power-of-two step: no prediction, so none may be passed
    const int code = coder_code(coder);
    const int32_t field = coder >> 8;  // exponent + 127
    const int ndt = code == KMP_CODER_QUANT_I16 ? KMP_I16 : KMP_I32;
    KMP_REQUIRE(!pred, "the quantising coders take no prediction (pred must be NULL)");
    KMP_REQUIRE(field >= 1 && field <= 254, "quantiser exponent outside [-126, 127]");
    KMP_REQUIRE(x_dtype == (direction == KMP_ENCODE ? (int)KMP_F32 : ndt),
                "quantising coders: float32 in (encode), the code's int16 / int32 in (decode)");
    if (n == 0) return KMP_OK;
    KMP_REQUIRE(x && out, "null pointer");
    const int e = field - 127;
    const QuantP q{std::ldexp(1.0, -e), std::ldexp(1.0, e), std::ldexp(1.0, e - 1)};
    hipStream_t s = (hipStream_t)stream;
    auto go = [&](auto dir_c, auto ntag) {
      constexpr int DIR = decltype(dir_c)::value;
      using TN = decltype(ntag);
      // the integer side of a vector item is 4 * sizeof(TN) bytes, the float32 side 16
      const uintptr_t fa = (uintptr_t)(DIR == KMP_ENCODE ? x : out), na = (uintptr_t)(DIR == KMP_ENCODE ? out : x);
      if ((fa & 15) == 0 && (na & (4 * sizeof(TN) - 1)) == 0 && n % 4 == 0)
        quant_vec_kernel<DIR, TN><<<grid_for(n / 4), kThreads, 0, s>>>(x, n / 4, out, q);
      else
        quant_kernel<DIR, TN><<<grid_for(n), kThreads, 0, s>>>(x, n, out, q);
      return check_launch("code");
    };
    auto with_t = [&](auto dir_c) { return ndt == KMP_I16 ? go(dir_c, int16_t{}) : go(dir_c, int32_t{}); };
    return direction == KMP_ENCODE ? with_t(std::integral_constant<int, KMP_ENCODE>{})
                                   : with_t(std::integral_constant<int, KMP_DECODE>{});
  }
  if (coder >= 0 && is_prec_code(coder_code(coder))) {
    // float32 <-> int16 / int32 by the top m mantissa bits: no prediction either
    const int code = coder_code(coder);
    const int32_t field = coder >> 8;  // m + 1
    const int ndt = code == KMP_CODER_PREC_I16 ? KMP_I16 : KMP_I32;
    KMP_REQUIRE(!pred, "the quantising coders take no prediction (pred must be NULL)");
    KMP_REQUIRE(field >= 1 && field <= 23, "kept mantissa bits outside [0, 22]");
    KMP_REQUIRE(x_dtype == (direction == KMP_ENCODE ? (int)KMP_F32 : ndt),
                "quantising coders: float32 in (encode), the code's int16 / int32 in (decode)");
    if (n == 0) return KMP_OK;
    KMP_REQUIRE(x && out, "null pointer");
    const uint32_t t = (uint32_t)(24 - field), rnd = (1u << (t - 1)) - 1u;
    hipStream_t s = (hipStream_t)stream;
    auto go = [&](auto dir_c, auto ntag) {
      constexpr int DIR = decltype(dir_c)::value;
      using TN = decltype(ntag);
      // the integer side of a vector item is 4 * sizeof(TN) bytes, the float32 side 16
      const uintptr_t fa = (uintptr_t)(DIR == KMP_ENCODE ? x : out), na = (uintptr_t)(DIR == KMP_ENCODE ? out : x);
      if ((fa & 15) == 0 && (na & (4 * sizeof(TN) - 1)) == 0 && n % 4 == 0)
        prec_vec_kernel<DIR, TN><<<grid_for(n / 4), kThreads, 0, s>>>(x, n / 4, out, t, rnd);
      else
        prec_kernel<DIR, TN><<<grid_for(n), kThreads, 0, s>>>(x, n, out, t, rnd);
      return check_launch("code");
    };
    auto with_t = [&](auto dir_c) { return ndt == KMP_I16 ? go(dir_c, int16_t{}) : go(dir_c, int32_t{}); };
    return direction == KMP_ENCODE ? with_t(std::integral_constant<int, KMP_ENCODE>{})
                                   : with_t(std::integral_constant<int, KMP_DECODE>{});
  }
  if (n == 0) return KMP_OK;
  KMP_REQUIRE(pred && x && out, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (int st = check_coder_arg(coder, dtype_size(x_dtype), "kmp_code")) return st;
  if (is_near_code(coder_code(coder))) {
    // the samples' dtype is x's (a decode's residuals are labelled with it: the signed codes say
    // "signed samples"); predictions are in that dtype or float32
    KMP_REQUIRE(x_dtype == KMP_U8 || x_dtype == KMP_U16 || x_dtype == KMP_I8 || x_dtype == KMP_I16,
                "near coders take 8- / 16-bit integer samples");
    KMP_REQUIRE(pred_dtype == x_dtype || pred_dtype == KMP_F32, "near coders: predictions in the sample dtype or float32");
    const NearQ q = make_nearq(coder_max_error(coder));
    const bool sgn = x_dtype == KMP_I8 || x_dtype == KMP_I16, pf = pred_dtype == KMP_F32;
    auto go = [&](auto dir_c, auto coder_c, auto sgn_c, auto ptag) {
      constexpr int CODER = decltype(coder_c)::value;
      using TO = typename coder_out<CODER>::type;
      using TP = std::conditional_t<std::is_same<decltype(ptag), float>::value, float, TO>;
      code_near_kernel<decltype(dir_c)::value, CODER, decltype(sgn_c)::value, TP>
          <<<grid_for(n), kThreads, 0, s>>>((const TP*)pred, (const TO*)x, n, (TO*)out, q);
      return check_launch("code");
    };
    auto with_p = [&](auto dir_c, auto coder_c, auto sgn_c) {
      return pf ? go(dir_c, coder_c, sgn_c, float{}) : go(dir_c, coder_c, sgn_c, int{});
    };
    auto with_s = [&](auto dir_c, auto coder_c) {
      return sgn ? with_p(dir_c, coder_c, std::true_type{}) : with_p(dir_c, coder_c, std::false_type{});
    };
    auto with_c = [&](auto dir_c) {
      return coder_code(coder) == KMP_CODER_NEAR_U8 ? with_s(dir_c, std::integral_constant<int, KMP_CODER_NEAR_U8>{})
                                                    : with_s(dir_c, std::integral_constant<int, KMP_CODER_NEAR_U16>{});
    };
    return direction == KMP_ENCODE ? with_c(std::integral_constant<int, KMP_ENCODE>{})
                                   : with_c(std::integral_constant<int, KMP_DECODE>{});
  }
  pred_dtype = unsigned_twin(pred_dtype);  // signed samples: the same bits mod 2^W (kmp_common.h)
  x_dtype = unsigned_twin(x_dtype);
  auto launch = [&](auto dir_c, auto coder_c) {
    constexpr int DIR = decltype(dir_c)::value;
    constexpr int CODER = decltype(coder_c)::value;
    return dispatch_any_dtype(pred_dtype, [&](auto ptag) {
      using TP = decltype(ptag);
      return dispatch_any_dtype(x_dtype, [&](auto xtag) {
        using TX = decltype(xtag);
        using TO = typename coder_out<CODER>::type;
        if constexpr (sizeof(TP) == sizeof(TX) && sizeof(TX) == sizeof(TO) && !std::is_same<TP, float>::value &&
                      !std::is_same<TX, float>::value) {
          constexpr int V = 16 / sizeof(TX);
          if ((((uintptr_t)pred | (uintptr_t)x | (uintptr_t)out) & 15) == 0 && n % V == 0) {
            code_vec_kernel<DIR, CODER, TX><<<grid_for(n / V), kThreads, 0, s>>>(
                (const u32x4v*)pred, (const u32x4v*)x, n / V, (u32x4v*)out);
            return check_launch("code");
          }
        }
        return with_index(fits32({n}), [&](auto itag) {
          using I = decltype(itag);
          code_kernel<DIR, CODER, TP, TX, I><<<grid_for(n), kThreads, 0, s>>>(
              (const TP*)pred, (const TX*)x, (I)n, (typename coder_out<CODER>::type*)out);
          return check_launch("code");
        });
      });
    });
  };
  auto with_coder = [&](auto dir_c) {
    switch (coder) {
      case KMP_CODER_RAW: return launch(dir_c, std::integral_constant<int, KMP_CODER_RAW>{});
      case KMP_CODER_U8: return launch(dir_c, std::integral_constant<int, KMP_CODER_U8>{});
      case KMP_CODER_U16: return launch(dir_c, std::integral_constant<int, KMP_CODER_U16>{});
      case KMP_CODER_U32: return launch(dir_c, std::integral_constant<int, KMP_CODER_U32>{});
      default: return fail(KMP_ERR_ARG, "kmp_code: bad coder");
    }
  };
  return direction == KMP_ENCODE ? with_coder(std::integral_constant<int, KMP_ENCODE>{})
                                 : with_coder(std::integral_constant<int, KMP_DECODE>{});
}

}  // extern "C"

// kmp_fit.hip -- exact second moments of (features, targets, 1) over every cell of a highres batch:
// the normal equations of a least-squares LinearPredictor fit.
//
// For a highres batch h and padding p the quantity is M = X^T X with one row of X per cell,
//   X = [ features_from_lowres(pad_neighborhood(lowres_from_highres(pad_highres(h)), p), p),
//         targets_from_highres(pad_highres(h)), 1 ]
// (volume/utils.py:37-74,199-218,226-237; image/utils.py:38-49,121-137,146-156) as exact int64.
//
// The kernel reads the unpadded highres directly (the reflect pad of even dims and the symmetric
// neighbourhood pad are index mirroring, fold() below) and never materialises X.  Samples are split
// into bytes (uint16: lo and hi, uint8: one), each biased by -128 into a signed i8 column; with the
// constant column these are NB byte columns, NBLK = ceil(NB / 16) column blocks.  A workgroup stages
// the byte columns of 64 consecutive cells in LDS ([column][cell], tails as zero) and its 4 waves
// share the NBLK (NBLK + 1) / 2 block pairs (I <= J): one v_mfma_i32_16x16x64_i8 per pair and step,
// K = the cell axis, the fragment of block I as the A operand and of block J as the B operand.  Both
// operands index k the same way, so the result does not depend on the k order inside a fragment.
//
// |product| <= 2^14, so an i32 accumulator holds 2^17 of them; every accumulator is added to the
// zeroed int64 workspace table (64-bit integer vector atomics: order-free, so deterministic) after at
// most kFlushSteps * 64 = 2^16 cells.  fit_finish_kernel then recombines the biased byte moments
// into sample moments:  sum(ab) = sum(a'b') + 128 (sum(a) + sum(b)) - 16384 n,  sum(a) = sum(a') + 128 n,
// f = 256 hi + lo, and writes the full symmetric M.
#include <utility>

#include "kmp_common.h"

namespace kmp {
namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

constexpr int kFitThreads = 256;
constexpr int kFitWaves = 4;
constexpr int kStepCells = 64;     // cells per K step == K of the MFMA
constexpr int kFlushSteps = 1024;  // steps between flushes: 2^16 products per accumulator element
constexpr int kFitGrid = 512;      // workgroups at most (2 per CU); each takes a contiguous run of steps
static_assert((int64_t)kFlushSteps * kStepCells <= (1 << 17), "an i32 accumulator holds 2^17 products of 2^14");

template <typename T, int NSP, int P>
struct FitCfg {
  static constexpr int KW = 2 * P + 2;                            // neighbourhood width
  static constexpr int N = NSP == 3 ? KW * KW * KW : KW * KW;     // features
  static constexpr int K = NSP == 3 ? 19 : 5;                     // targets
  static constexpr int NV = N + K;                                // sample columns
  static constexpr int S = (int)sizeof(T);                        // bytes per sample
  static constexpr int NB = S * NV + 1;                           // byte columns (+ the constant)
  static constexpr int NBLK = (NB + 15) / 16;
  static constexpr int NBP = NBLK * 16;
  static constexpr int NPAIR = NBLK * (NBLK + 1) / 2;
  static constexpr int NACC = (NPAIR + kFitWaves - 1) / kFitWaves;  // accumulator tiles per wave
  static constexpr int NVW = (NV + kFitWaves - 1) / kFitWaves;      // samples a lane stages per step
};

// target k's source per axis (z, y, x): 0 = the cell's low node (2c), 1 = its odd sample (2c + 1),
// 2 = its high node (2c + 2, mirrored at an even dim's end).  volume/utils.py:37-74: L R U D F B C
// z0..z3 y0..y3 x0..x3; image/utils.py:38-49: L R U D C.
constexpr int8_t kTgt3[19][3] = {{1, 1, 0}, {1, 1, 2}, {1, 0, 1}, {1, 2, 1}, {0, 1, 1}, {2, 1, 1}, {1, 1, 1},
                                 {1, 0, 0}, {1, 0, 2}, {1, 2, 2}, {1, 2, 0},
                                 {0, 1, 0}, {0, 1, 2}, {2, 1, 2}, {2, 1, 0},
                                 {0, 0, 1}, {0, 2, 1}, {2, 2, 1}, {2, 0, 1}};
constexpr int8_t kTgt2[5][3] = {{0, 1, 0}, {0, 1, 2}, {0, 0, 1}, {0, 2, 1}, {0, 1, 1}};

// pair p of the row-major upper triangle of NBLK x NBLK blocks
constexpr int pair_i(int nblk, int p) {
  int i = 0;
  while (p >= nblk - i) { p -= nblk - i; ++i; }
  return i;
}
constexpr int pair_j(int nblk, int p) {
  int i = 0;
  while (p >= nblk - i) { p -= nblk - i; ++i; }
  return i + p;
}

template <int... I, typename F>
__device__ __forceinline__ void sfor_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void sfor(F&& f) {  // f(integral_constant<int, i>) for i in [0, N)
  sfor_impl(std::make_integer_sequence<int, N>{}, f);
}

struct FitArgs {
  const void* hin;
  unsigned long long* ws;
  int64_t plane, vol;  // H * W and D * H * W elements
  int32_t W;
  int32_t L[3], E[3], Lc[3];  // z, y, x (2D: z unused)
  UDiv dx, dy, dz;            // division by Lc
  uint32_t cells;
  int32_t steps;
};

// lowres source node of padded node r in [-P, L + P - 1], P <= 2 <= L: the symmetric neighbourhood pad
// over L nodes, then the reflect pad of an even dim (node L - 1 == node E - 1 when E == L - 1).  One
// reflection each suffices in that range (-1 - r <= 1 < L;  2L - 1 - r >= L - 2 >= 0;  E >= 1).
__device__ __forceinline__ int fold(int r, int L, int E) {
  if (r < 0) r = -1 - r;
  if (r >= L) r = 2 * L - 1 - r;
  if (r >= E) r = 2 * E - 1 - r;
  return r;
}

// the samples wave part WV stages for this lane's cell of ``step`` (sample v of the N + K goes to part
// v % 4); ``valid`` is false past the last cell, whose lanes read cell 0 and contribute zero
template <typename T, int NSP, int P, int WV>
__device__ __forceinline__ bool fit_load(const FitArgs& a, int step, uint32_t (&vals)[FitCfg<T, NSP, P>::NVW]) {
  using Cf = FitCfg<T, NSP, P>;
  const int lane = threadIdx.x & 63;
  uint32_t t = (uint32_t)step * kStepCells + lane;
  const bool valid = t < a.cells;
  if (!valid) t = 0;
  uint32_t q = udiv(t, a.dx);
  const int cx = (int)(t - q * (uint32_t)a.Lc[2]);
  t = q;
  q = udiv(t, a.dy);
  const int cy = (int)(t - q * (uint32_t)a.Lc[1]);
  int cz = 0;
  uint32_t b = q;
  if constexpr (NSP == 3) {
    t = q;
    b = udiv(t, a.dz);
    cz = (int)(t - b * (uint32_t)a.Lc[0]);
  }
  const T* base = (const T*)a.hin + (int64_t)b * a.vol;
  // element offsets per axis: the KW feature sources, then the 3 target sources
  int xs[Cf::KW + 3];
  int64_t ys[Cf::KW + 3], zs[Cf::KW + 3];
#pragma unroll
  for (int d = 0; d < Cf::KW; ++d) {
    xs[d] = 2 * fold(cx + d - P, a.L[2], a.E[2]);
    ys[d] = (int64_t)(2 * fold(cy + d - P, a.L[1], a.E[1])) * a.W;
    zs[d] = NSP == 3 ? (int64_t)(2 * fold(cz + d - P, a.L[0], a.E[0])) * a.plane : 0;
  }
  xs[Cf::KW] = 2 * cx; xs[Cf::KW + 1] = 2 * cx + 1; xs[Cf::KW + 2] = 2 * fold(cx + 1, a.L[2], a.E[2]);
  ys[Cf::KW] = (int64_t)(2 * cy) * a.W; ys[Cf::KW + 1] = (int64_t)(2 * cy + 1) * a.W;
  ys[Cf::KW + 2] = (int64_t)(2 * fold(cy + 1, a.L[1], a.E[1])) * a.W;
  if constexpr (NSP == 3) {
    zs[Cf::KW] = (int64_t)(2 * cz) * a.plane; zs[Cf::KW + 1] = (int64_t)(2 * cz + 1) * a.plane;
    zs[Cf::KW + 2] = (int64_t)(2 * fold(cz + 1, a.L[0], a.E[0])) * a.plane;
  } else {
    zs[Cf::KW] = zs[Cf::KW + 1] = zs[Cf::KW + 2] = 0;
  }
  sfor<Cf::NV>([&](auto vi) {
    constexpr int v = decltype(vi)::value;
    if constexpr (v % kFitWaves == WV) {
      constexpr bool feat = v < Cf::N;
      constexpr int k = feat ? 0 : v - Cf::N;
      // features in z-major, y, x order (volume/utils.py:199-210)
      constexpr int iz = feat ? (NSP == 3 ? v / (Cf::KW * Cf::KW) : 0) : Cf::KW + (NSP == 3 ? kTgt3[k][0] : 0);
      constexpr int iy = feat ? (v / Cf::KW) % Cf::KW : Cf::KW + (NSP == 3 ? kTgt3[k][1] : kTgt2[k % 5][1]);
      constexpr int ix = feat ? v % Cf::KW : Cf::KW + (NSP == 3 ? kTgt3[k][2] : kTgt2[k % 5][2]);
      vals[v / kFitWaves] = (uint32_t)base[zs[iz] + ys[iy] + xs[ix]];
    }
  });
  return valid;
}

// write the staged samples as biased byte columns: lds[column][cell], column S v + s (s = 0: low byte)
template <typename T, int NSP, int P, int WV>
__device__ __forceinline__ void fit_store(int8_t* lds, const uint32_t (&vals)[FitCfg<T, NSP, P>::NVW], bool valid) {
  using Cf = FitCfg<T, NSP, P>;
  const int lane = threadIdx.x & 63;
  sfor<Cf::NV>([&](auto vi) {
    constexpr int v = decltype(vi)::value;
    if constexpr (v % kFitWaves == WV) {
      const uint32_t x = vals[v / kFitWaves];
#pragma unroll
      for (int s = 0; s < Cf::S; ++s)
        lds[(Cf::S * v + s) * kStepCells + lane] = valid ? (int8_t)(((x >> (8 * s)) & 0xffu) ^ 0x80u) : (int8_t)0;
    }
  });
  if constexpr (WV == 0) lds[(Cf::NB - 1) * kStepCells + lane] = valid ? (int8_t)1 : (int8_t)0;  // the constant column
}

// one K step: this wave's block pairs (pair p goes to wave p % 4)
template <typename T, int NSP, int P, int WV>
__device__ __forceinline__ void fit_mma(const int8_t* lds, i32x4 (&acc)[FitCfg<T, NSP, P>::NACC]) {
  using Cf = FitCfg<T, NSP, P>;
  const int lane = threadIdx.x & 63;
  // lane l holds column 16 I + (l & 15), cells 16 (l >> 4) .. + 15 of block I: the A (row = column of I)
  // and the B (col = column of J) fragment alike
  const int8_t* p = lds + (lane & 15) * kStepCells + (lane >> 4) * 16;
  i32x4 fr[Cf::NBLK];
  sfor<Cf::NBLK>([&](auto bi) {
    constexpr int I = decltype(bi)::value;
    fr[I] = *(const i32x4*)(p + I * 16 * kStepCells);
  });
  sfor<Cf::NPAIR>([&](auto pi) {
    constexpr int pr = decltype(pi)::value;
    if constexpr (pr % kFitWaves == WV) {
      constexpr int I = pair_i(Cf::NBLK, pr), J = pair_j(Cf::NBLK, pr);
      acc[pr / kFitWaves] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fr[I], fr[J], acc[pr / kFitWaves], 0, 0, 0);
    }
  });
}

// add this wave's accumulators to the table and clear them.  C/D map: column = lane & 15 (block J),
// row = 4 (lane >> 4) + register (block I)
template <typename T, int NSP, int P, int WV>
__device__ __forceinline__ void fit_flush(unsigned long long* ws, i32x4 (&acc)[FitCfg<T, NSP, P>::NACC]) {
  using Cf = FitCfg<T, NSP, P>;
  const int lane = threadIdx.x & 63;
  sfor<Cf::NPAIR>([&](auto pi) {
    constexpr int pr = decltype(pi)::value;
    if constexpr (pr % kFitWaves == WV) {
      constexpr int I = pair_i(Cf::NBLK, pr), J = pair_j(Cf::NBLK, pr);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int32_t v = acc[pr / kFitWaves][r];
        const int row = 16 * I + 4 * (lane >> 4) + r, col = 16 * J + (lane & 15);
        if (v != 0) atomicAdd(ws + row * Cf::NBP + col, (unsigned long long)(long long)v);
      }
      acc[pr / kFitWaves] = i32x4{0, 0, 0, 0};
    }
  });
}

// one wave's share of the workgroup's run of steps [s0, s1): part WV of the staging and of the block
// pairs.  The four parts execute the same sequence of barriers.
template <typename T, int NSP, int P, int WV>
__device__ __forceinline__ void fit_wave(const FitArgs& a, int8_t (&lds)[2][FitCfg<T, NSP, P>::NBP * kStepCells],
                                         int s0, int s1) {
  using Cf = FitCfg<T, NSP, P>;
  i32x4 acc[Cf::NACC];
#pragma unroll
  for (int i = 0; i < Cf::NACC; ++i) acc[i] = i32x4{0, 0, 0, 0};
  uint32_t vals[Cf::NVW];
  bool valid = fit_load<T, NSP, P, WV>(a, s0, vals);
  fit_store<T, NSP, P, WV>(lds[0], vals, valid);
  __syncthreads();
  // step s - 1 is in LDS; the loads of step s are in flight while the matrix cores take step s - 1
  for (int s = s0 + 1; s <= s1; ++s) {
    if (s < s1) valid = fit_load<T, NSP, P, WV>(a, s, vals);
    fit_mma<T, NSP, P, WV>(lds[(s - 1 - s0) & 1], acc);
    if ((s - s0) % kFlushSteps == 0 || s == s1) fit_flush<T, NSP, P, WV>(a.ws, acc);
    if (s < s1) fit_store<T, NSP, P, WV>(lds[(s - s0) & 1], vals, valid);
    __syncthreads();
  }
}

template <typename T, int NSP, int P>
__global__ __launch_bounds__(kFitThreads) void fit_kernel(FitArgs a) {
  using Cf = FitCfg<T, NSP, P>;
  __shared__ __attribute__((aligned(16))) int8_t lds[2][Cf::NBP * kStepCells];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int per = (a.steps + (int)gridDim.x - 1) / (int)gridDim.x;
  const int s0 = (int)blockIdx.x * per;
  const int s1 = s0 + per < a.steps ? s0 + per : a.steps;
  if (s0 >= s1) return;

  // the padding columns NB .. NBP - 1 stay zero for the whole kernel
  for (int i = threadIdx.x; i < 2 * Cf::NBP * kStepCells / 4; i += kFitThreads) ((uint32_t*)&lds[0][0])[i] = 0u;
  __syncthreads();

  switch (wave) {  // wave-uniform
    case 0: fit_wave<T, NSP, P, 0>(a, lds, s0, s1); break;
    case 1: fit_wave<T, NSP, P, 1>(a, lds, s0, s1); break;
    case 2: fit_wave<T, NSP, P, 2>(a, lds, s0, s1); break;
    default: fit_wave<T, NSP, P, 3>(a, lds, s0, s1); break;
  }
}

// biased byte moments (upper block triangle of ws) -> sample moments M [Q, Q], Q = NV + 1
template <int S>
__global__ void fit_finish_kernel(const long long* __restrict__ ws, int NBP, int NV, long long* __restrict__ M) {
  const int Q = NV + 1;
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (idx >= Q * Q) return;
  const int i = idx / Q, j = idx % Q;
  auto g = [&](int c, int d) { return c <= d ? ws[c * NBP + d] : ws[d * NBP + c]; };
  const int one = S * NV;
  const long long n = g(one, one);
  auto sum1 = [&](int c) { return g(c, one) + 128 * n; };  // sum of the unbiased byte column c
  unsigned long long m = 0;
  if (i == NV && j == NV) {
    m = (unsigned long long)n;
  } else if (i == NV || j == NV) {
    const int q = i == NV ? j : i;
    for (int s = 0; s < S; ++s) m += (unsigned long long)sum1(S * q + s) << (8 * s);
  } else {
    for (int s = 0; s < S; ++s)
      for (int u = 0; u < S; ++u) {
        const int c = S * i + s, d = S * j + u;
        const long long ab = g(c, d) + 128 * (sum1(c) + sum1(d)) - 16384 * n;
        m += (unsigned long long)ab << (8 * (s + u));
      }
  }
  M[idx] = (long long)m;
}

template <typename F>
int fit_dispatch(int nsp, int dtype, int padding, F&& f) {
  auto with_t = [&](auto tag) {
    if (nsp == 3) {
      if (padding == 0) return f(tag, std::integral_constant<int, 3>{}, std::integral_constant<int, 0>{});
      if (padding == 1) return f(tag, std::integral_constant<int, 3>{}, std::integral_constant<int, 1>{});
    } else if (nsp == 2) {
      if (padding == 0) return f(tag, std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{});
      if (padding == 1) return f(tag, std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{});
      if (padding == 2) return f(tag, std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
    }
    return fail(KMP_ERR_UNSUPPORTED, "linear_moments: volumes take padding 0 or 1, images 0, 1 or 2");
  };
  if (dtype == KMP_U8) return with_t(uint8_t{});
  if (dtype == KMP_U16) return with_t(uint16_t{});
  return fail(KMP_ERR_UNSUPPORTED, "linear_moments: uint8 / uint16 samples only");
}

}  // namespace
}  // namespace kmp

using namespace kmp;

extern "C" {

size_t kmp_linear_moments_workspace_bytes(int32_t nsp, int32_t dtype, int32_t padding) {
  size_t bytes = 0;
  fit_dispatch(nsp, dtype, padding, [&](auto tag, auto nsp_c, auto p_c) {
    using Cf = FitCfg<decltype(tag), decltype(nsp_c)::value, decltype(p_c)::value>;
    bytes = (size_t)Cf::NBP * Cf::NBP * sizeof(int64_t);
    return (int)KMP_OK;
  });
  return bytes;
}

int kmp_linear_moments(int32_t nsp, int32_t dtype, const void* highres, int64_t B, const int64_t shape[3], int64_t C,
                       int32_t padding, int64_t* moments, void* workspace, kmp_stream_t stream) {
  KMP_REQUIRE(nsp == 2 || nsp == 3, "nsp must be 2 or 3");
  KMP_REQUIRE(shape && B >= 1 && C >= 1, "empty batch or null shape");
  if (C != 1) return fail(KMP_ERR_UNSUPPORTED, "linear_moments: C == 1 only");
  return fit_dispatch(nsp, dtype, padding, [&](auto tag, auto nsp_c, auto p_c) {
    using T = decltype(tag);
    constexpr int NSP = decltype(nsp_c)::value, P = decltype(p_c)::value;
    using Cf = FitCfg<T, NSP, P>;
    KMP_REQUIRE(highres && moments && workspace, "null pointer");
    KMP_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)moments & 7) == 0, "workspace / moments misaligned");
    for (int i = 0; i < nsp; ++i) KMP_REQUIRE(shape[i] >= 2 && shape[i] < (1ll << 30), "spatial dims must be >= 2");
    const Geo g = make_geo_from_highres(nsp, shape);
    int64_t cells = B;
    for (int ax = 3 - nsp; ax < 3; ++ax) {
      cells *= g.Lc[ax];
      KMP_REQUIRE(cells <= 0x7fffffffll, "more than 2^31 - 1 cells in one call (the sums must stay below 2^63)");
    }
    FitArgs a{};
    a.hin = highres;
    a.ws = (unsigned long long*)workspace;
    a.W = (int32_t)g.n[2];
    a.plane = g.n[1] * g.n[2];
    a.vol = g.n[0] * g.n[1] * g.n[2];
    for (int ax = 0; ax < 3; ++ax) {
      a.L[ax] = (int32_t)g.L[ax];
      a.E[ax] = (int32_t)g.E[ax];
      a.Lc[ax] = (int32_t)g.Lc[ax];
    }
    a.dx = make_udiv((uint32_t)g.Lc[2]);
    a.dy = make_udiv((uint32_t)g.Lc[1]);
    a.dz = make_udiv((uint32_t)g.Lc[0]);
    a.cells = (uint32_t)cells;
    a.steps = (int32_t)ceil_div(cells, kStepCells);
    const size_t wbytes = (size_t)Cf::NBP * Cf::NBP * sizeof(int64_t);
    if (hipMemsetAsync(workspace, 0, wbytes, (hipStream_t)stream) != hipSuccess) return check_launch("linear_moments");
    const int grid = a.steps < kFitGrid ? a.steps : kFitGrid;
    fit_kernel<T, NSP, P><<<grid, kFitThreads, 0, (hipStream_t)stream>>>(a);
    if (int s = check_launch("linear_moments")) return s;
    constexpr int Q = Cf::NV + 1;
    fit_finish_kernel<Cf::S><<<(Q * Q + 255) / 256, 256, 0, (hipStream_t)stream>>>((const long long*)workspace, Cf::NBP,
                                                                               Cf::NV, (long long*)moments);
    return check_launch("linear_moments_finish");
  });
}

}  // extern "C"

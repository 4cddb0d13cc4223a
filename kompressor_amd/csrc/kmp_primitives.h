// kmp_primitives.h -- what the primitive units (kmp_primitives.hip, kmp_maps_from_predictions.hip,
// kmp_mean_predict.hip) share: the kernels' index types and the host rules that pick an index width
// and a kernel form.
#pragma once

#include <algorithm>
#include <initializer_list>

#include "kmp_aggregate.h"

namespace kmp {

// Every element kernel of these units is instantiated with a 32-bit index type when all the arrays
// it touches have fewer than 2^30 elements (64-bit multiplies and divisions are multi-instruction
// sequences on gfx950), and with I otherwise.
template <typename I>
struct IdxT {
  I b, i0, i1, i2, c;
};
// Decompose a flat index over [B, e0, e1, e2, C].
template <typename I>
__device__ __forceinline__ IdxT<I> unflat_t(I t, I e0, I e1, I e2, I C) {
  IdxT<I> r;
  if constexpr (sizeof(I) == 4) {
    uint32_t u = (uint32_t)t;
    if (C == 1) {
      r.c = 0;
    } else {
      r.c = (I)(u % (uint32_t)C);
      u /= (uint32_t)C;
    }
    r.i2 = (I)(u % (uint32_t)e2); u /= (uint32_t)e2;
    r.i1 = (I)(u % (uint32_t)e1); u /= (uint32_t)e1;
    r.i0 = (I)(u % (uint32_t)e0);
    r.b = (I)(u / (uint32_t)e0);
  } else {
    unflat5(t, e0, e1, e2, C, r.b, r.i0, r.i1, r.i2, r.c);
  }
  return r;
}

// spatial extents (z, y, x; a 2D array's z is 1): on the host, and in a kernel's index type
struct Ext3 {
  int64_t e[3];
};
template <typename I>
struct E3 {
  I e[3];
};
template <typename I>
static inline E3<I> e3(const Ext3& x) {
  return E3<I>{{(I)x.e[0], (I)x.e[1], (I)x.e[2]}};
}
static inline E3<int32_t> e32(const Ext3& x) { return e3<int32_t>(x); }

__device__ __forceinline__ void divmod_small(int32_t i, int32_t n, float rcp, int32_t& q, int32_t& r) {
  q = (int32_t)((float)i * rcp);  // i < 2^21: off by at most one
  r = i - q * n;
  if (r < 0) { --q; r += n; } else if (r >= n) { ++q; r -= n; }
}

// ---- host rules ----
static inline Ext3 ext_from(int nsp, const int64_t* shape) {
  Ext3 e;
  for (int a = 0; a < 3; ++a) e.e[a] = (a < 3 - nsp) ? 1 : shape[a - (3 - nsp)];
  return e;
}

// 32-bit kernel indices when every array the launch touches is below 2^30 elements
static inline bool fits32(std::initializer_list<int64_t> counts) {
  for (int64_t c : counts)
    if (c >= ((int64_t)1 << 30)) return false;
  return true;
}
template <typename F>
static auto with_index(bool small, F&& f) {  // f(I{}): returns a status, or nothing
  return small ? f(int32_t{}) : f(int64_t{});
}
static inline int64_t vol(int64_t B, const Ext3& e, int64_t C) { return B * e.e[0] * e.e[1] * e.e[2] * C; }

// the row kernels serve C == 1 arrays below 2^30 elements (KMP_DISABLE_ROWS=1: element kernels)
static inline bool rows_ok(int64_t C, std::initializer_list<int64_t> counts) {
  return !opt(OPT_DISABLE_ROWS, 0) && C == 1 && fits32(counts);
}
template <typename T>
static inline int32_t row_chunks(int64_t n) { return (int32_t)ceil_div(n, 16 / (int64_t)sizeof(T)); }

static inline int check_common(int nsp, int64_t B, const int64_t* shape, int64_t C) {
  KMP_REQUIRE(nsp == 2 || nsp == 3, "nsp must be 2 or 3");
  KMP_REQUIRE(B >= 0 && C >= 1 && shape, "bad batch/channel/shape");
  for (int a = 0; a < nsp; ++a) KMP_REQUIRE(shape[a] >= 0, "negative extent");
  return KMP_OK;
}

// The 7 (3) map pointers of an entry point into the kernels' by-value argument (void* -> MapPtrs,
// const void* -> CMapPtrs); false when one is null.
template <typename P, typename M>
static inline bool bind_maps(int nsp, P* const* ptrs, M& m) {
  for (int k = 0; k < (nsp == 3 ? 7 : 3); ++k)
    if (!(m.p[k] = ptrs[k])) return false;
  return true;
}

// Tile plan of the z-rolling LDS kernels (maps_from_predictions_lds_kernel, mean_predict_lds_kernel): a workgroup
// owns YB frame rows x XO frame columns of ZC consecutive output planes; the frame is cells + 1 per spatial axis.
struct ZRollPlan {
  int32_t XO, YB, nyb, nxb, ZC, nzc;
  int64_t nblk;
};
static inline ZRollPlan plan_zroll(int64_t B, const Ext3& frame, int nsp) {
  const int32_t XO = (int32_t)std::min<int64_t>(frame.e[2], 64);
  const int32_t YB = std::max(1, std::min(8, kThreads / XO));
  const int32_t nyb = (int32_t)ceil_div(frame.e[1], YB), nxb = (int32_t)ceil_div(frame.e[2], XO);
  // enough workgroups to fill the chip: split the z roll into nzc runs of ZC output planes
  const int64_t fz = nsp == 3 ? frame.e[0] : 1;
  const int64_t want = ceil_div(4096, B * nyb * nxb);
  const int32_t ZC = (int32_t)ceil_div(fz, std::max<int64_t>(1, std::min<int64_t>(want, fz)));
  const int32_t nzc = (int32_t)ceil_div(fz, ZC);
  return ZRollPlan{XO, YB, nyb, nxb, ZC, nzc, B * nzc * nyb * nxb};
}

// kmp_maps_from_predictions.hip: every map but the centre one from the [B, cells..., C] cell means
// ``cm`` of the sample dtype (the mean predictor's second pass; ``total`` = B x frame x C elements,
// ``small`` = 32-bit indices serve).  The launch is named "mean_predict_maps".
int launch_maps_from_cell_means(int nsp, int dtype, const void* cm, int64_t B, const Ext3& cells, int64_t C,
                                const MapPtrs& outs, int64_t total, bool small, hipStream_t stream);

// kmp_compare.hip: the error statistics of ``r`` against ``x`` (KMP_CODER_COMPARE; n >= 1 elements of
// ``dtype``, ``out`` the 8-byte aligned KMP_COMPARE_BYTES, ``cont`` = continue the record at its start).
// Two launches, named "compare"; KMP_ERR_ARG for a dtype it does not take.
int launch_compare(int dtype, const void* x, const void* r, int64_t n, void* out, int cont, hipStream_t stream);

// kmp_ssim.hip: the structural similarity of ``r`` against ``x`` (KMP_CODER_SSIM; n >= 1 elements of ``dtype``,
// ``out`` the 8-byte aligned KMP_SSIM_BYTES whose second 64 bytes hold the request).  Two launches, named
// "ssim"; KMP_ERR_ARG for a dtype it does not take.
int launch_ssim(int dtype, const void* x, const void* r, int64_t n, void* out, hipStream_t stream);

// kmp_fill.hip: the hold-fill of the marked int16 / int32 array ``x`` into ``out`` (KMP_CODER_FILL; n >= 1,
// ``ws`` the 8-byte aligned KMP_FILL_BYTES; ``out`` may be ``x``).  Three launches, named "fill"; KMP_ERR_ARG
// for another dtype.
int launch_fill(int dtype, const void* x, int64_t n, void* out, void* ws, hipStream_t stream);
// ... and the patch of the float32 array ``out`` from the R >= 1 records of a run table (KMP_CODER_RUNS).
// One launch, named "runs".
int launch_runs(const void* table, int64_t R, void* out, hipStream_t stream);

// kmp_delta.hip: out = x - pred (KMP_ENCODE) or x + pred (KMP_DECODE) modulo 2^(8 width) over n >= 1 samples of
// ``width`` bytes (KMP_CODER_DELTA; ``out`` may be ``x``).  One launch, named "delta"; KMP_ERR_ARG for
// another width.
int launch_delta(int direction, int width, const void* pred, const void* x, int64_t n, void* out,
                 hipStream_t stream);

}  // namespace kmp

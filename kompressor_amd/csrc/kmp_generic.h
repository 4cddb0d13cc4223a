// kmp_generic.h -- internal to the generic two-pass codec (kmp_codec_generic*.hip): the index
// helpers and casts its kernels share, the host's frames, and the launchers of its translation units.
#pragma once

#include "kmp_codec.h"
#include "kmp_wave.h"

namespace kmp {

struct Src {
  int64_t S[3];  // source extents (highres n for encode, trimmed lowres E for decode)
  int32_t mult;  // 2 (encode: lowres node j <- highres 2j) or 1 (decode)
};

// a box of outputs or of cells: first index and extent per axis
struct Frame {
  int64_t begin[3], ext[3];
};

// Unsigned 32-bit division by a runtime constant as multiply-high + add + shift (the host computes
// the magic number): n / d for n < 2^31.  The generic kernels' per-element index split was four
// integer divisions (~40 VALU each, emulated); this is 3 VALU per division.
struct FDiv {
  uint32_t d, m, s;
};
static inline FDiv fdiv(int64_t d64) {
  const uint32_t d = (uint32_t)(d64 < 1 ? 1 : d64);
  uint32_t s = 0;
  while (s < 32 && (1ull << s) < d) ++s;
  const uint64_t m = ((1ull << 32) * ((1ull << s) - d)) / d + 1;
  return FDiv{d, (uint32_t)m, s};
}
__device__ __forceinline__ uint32_t fdiv_q(uint32_t n, const FDiv& f) {
  return (__umulhi(n, f.m) + n) >> f.s;
}

// The index space of a frame: t -> (b, i0, i1, i2, c), c fastest (as unflat5)
struct Flat {
  FDiv dC, d2, d1, d0;
};
static inline Flat make_flat(const int64_t (&ext)[3], int64_t C) {
  return Flat{fdiv(C), fdiv(ext[2]), fdiv(ext[1]), fdiv(ext[0])};
}
template <typename I>
__device__ __forceinline__ void unflat_i(int64_t t, const Flat& F, const int64_t (&ext)[3], int64_t C, I& b, I& i0,
                                         I& i1, I& i2, I& c) {
  if constexpr (sizeof(I) == 4) {  // t < 2^31 (the host's choice of I)
    uint32_t u = (uint32_t)t, q;
    q = fdiv_q(u, F.dC); c = (I)(u - q * F.dC.d); u = q;
    q = fdiv_q(u, F.d2); i2 = (I)(u - q * F.d2.d); u = q;
    q = fdiv_q(u, F.d1); i1 = (I)(u - q * F.d1.d); u = q;
    q = fdiv_q(u, F.d0); i0 = (I)(u - q * F.d0.d); b = (I)q;
  } else {
    int64_t bb, z, y, x, cc;
    unflat5(t, ext[0], ext[1], ext[2], C, bb, z, y, x, cc);
    b = bb; i0 = z; i1 = y; i2 = x; c = cc;
  }
}

// astype(T) of the aggregation / mean: the saturating hardware conversion for 8- / 16-bit samples
// (cvt_sat, kmp_wave.h), the exact restatement otherwise
template <typename T>
__device__ __forceinline__ T gcast(float v) {
  if constexpr (is_small_sample<T>) return (T)wv::cvt_sat<T>(v);
  else return cast_f32<T>(v);
}

// astype(T) of an f32 LinearPredictor value (kmp_linear.hip lin_cast: the clamp-then-convert form
// of the saturating conversion for 8- / 16-bit samples, cast_f32 otherwise)
template <typename T>
__device__ __forceinline__ T lin_cast_t(float v) {
  if constexpr (sizeof(T) <= 2) return (T)wv::cvt_sat_mfma<T>(v);
  else return cast_f32<T>(v);
}

// the 7 (3) maps' lattice parities (z, y, x) and contributions at compile time (kmp_aggregate.h)
template <int NSP>
__device__ __forceinline__ constexpr int gpar(int k, int a) {
  constexpr int8_t t3[7][3] = {{1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  constexpr int8_t t2[3][3] = {{0, 1, 0}, {0, 0, 1}, {0, 1, 1}};
  return NSP == 3 ? t3[k][a] : t2[k][a];
}

// Lowres node source index along an axis: mult * sym(sym(j, L), E) (even reflect pad, then the
// neighbourhood's symmetric pad)
__device__ __forceinline__ int64_t node_src(int64_t j, int64_t L, int64_t E, int mult) {
  return mult * sym_index(sym_index(j, L), E);
}

// the outputs of a request: every stored node, or the region's clamped span of them
inline Frame make_frame(int nsp, const Geo& g, const kmp_region* region) {
  Frame f{};
  for (int a = 0; a < 3; ++a) {
    int64_t lo = 0, hi = g.E[a];
    if (region && a >= 3 - nsp) region_clamp(region, g, a, lo, hi);
    f.begin[a] = lo;
    f.ext[a] = hi > lo ? hi - lo : 0;
  }
  return f;
}

// Cells a frame of outputs depends on: [begin-1, end) clipped to [0, Lc).
inline Frame cell_frame(const Geo& g, const Frame& f) {
  Frame cf{};
  for (int a = 0; a < 3; ++a) {
    int64_t lo = f.begin[a] - 1, hi = f.begin[a] + f.ext[a];
    lo = lo < 0 ? 0 : lo;
    hi = hi > g.Lc[a] ? g.Lc[a] : hi;
    cf.begin[a] = lo;
    cf.ext[a] = (f.ext[a] > 0 && hi > lo) ? hi - lo : 0;
  }
  return cf;
}

// 32-bit element indexing when every array the generic kernels address (highres, cells, lowres,
// maps: all at most the padded highres size x K) and the index space stay below 2^31
inline bool fits32(const Geo& g, int64_t B, int64_t C, int K) {
  const int64_t lim = (int64_t)1 << 31;
  const int64_t hi = B * (g.n[0] + 1) * (g.n[1] + 1) * (g.n[2] + 1) * C;
  const int64_t cells = B * g.L[0] * g.L[1] * g.L[2] * K * C;
  return B > 0 && hi < lim && cells < lim;
}

// f(NSP, PERCH): the rank and "a prediction per map channel" (LinearPredictor) as integral constants
template <typename F>
inline void with_nsp_perch(int nsp, bool perch, F&& f) {
  using N3 = std::integral_constant<int, 3>;
  using N2 = std::integral_constant<int, 2>;
  if (nsp == 3) {
    if (perch) f(N3{}, std::true_type{});
    else f(N3{}, std::false_type{});
  } else {
    if (perch) f(N2{}, std::true_type{});
    else f(N2{}, std::false_type{});
  }
}

// the maps as a kernel that only reads them takes them
inline CMapPtrs cmaps(const MapPtrs& m) {
  CMapPtrs c{};
  for (int k = 0; k < kMaxMaps; ++k) c.p[k] = m.p[k];
  return c;
}

// Pass 1 (kmp_codec_generic_cells.hip): the predictor's values of the cells the outputs ``f``
// depend on, at their global position in ``cells`` [K, B, Lc..., C]
template <typename T>
int run_predictor(const T* src, const Src& s, const Geo& g, int nsp, int64_t B, int64_t C, const kmp_predictor* pred,
                  const Frame& f, T* cells, hipStream_t stream);

// Pass 2 with 4 output columns a thread (kmp_codec_generic_row4.hip; the caller checked C <= 4,
// 2 for volumes, and fits32).  ``cells`` null: the kernel computes them from the nodes of ``s``
// (fuse_lin2d).  The caller names the launch (check_launch).
template <typename T, bool DEC>
void launch_row4(const CodecCall<T, DEC>& c, const Src& s, const Frame& f, const T* cells);

}  // namespace kmp

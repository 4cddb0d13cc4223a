// kmp_codec.h -- internal interfaces between the fused-codec translation units: the request every
// kernel family takes, one entry point per family, and the host checks they share.
#pragma once

#include "kmp_aggregate.h"

namespace kmp {

template <typename T> constexpr int dtype_code();
template <> constexpr int dtype_code<uint8_t>() { return KMP_U8; }
template <> constexpr int dtype_code<uint16_t>() { return KMP_U16; }
template <> constexpr int dtype_code<int32_t>() { return KMP_I32; }
template <> constexpr int dtype_code<uint32_t>() { return KMP_U32; }
template <> constexpr int dtype_code<float>() { return KMP_F32; }
template <> constexpr int dtype_code<i8s>() { return KMP_I8; }
template <> constexpr int dtype_code<i16s>() { return KMP_I16; }

int64_t generic_workspace_bytes(int dtype, int nsp, const Geo& g, int64_t B, int64_t C, const kmp_predictor* pred);

// Linear predictor over a box of cells: writes cells[b, c..., k, C] (K = 19 / 5) in T
// (kmp_linear.hip).  ``src`` is highres (mult 2) or trimmed lowres (mult 1), extents S.
template <typename T>
int linear_cells(const T* src, const int64_t* S, int mult, const Geo& g, int nsp, int64_t B, int64_t C,
                 const kmp_predictor* pred, const int64_t* cbegin, const int64_t* cext, T* cells, hipStream_t stream);

// One encode (DEC = false) or decode (DEC = true) request of the fused codec.
template <typename T, bool DEC>
struct CodecCall {
  int nsp;
  const Geo& g;
  int64_t B, C;
  const kmp_predictor* pred;
  const kmp_region* region;
  const T* in;   // highres (encode) / lowres (decode)
  T* out;        // lowres (encode) / highres (decode)
  MapPtrs maps;  // written by encode, read by decode
  void* ws;
  size_t ws_bytes;
  hipStream_t stream;
  int32_t max_error = 0;  // > 0: the near-lossless coder of T's width with this bound (generic family only)
};

// The coder of a request is the natural coder of its sample type (the front door admits no other
// pair): (u8, U8), (u16, U16), (i32, RAW), (u32, U32), and the signed (i8, U8), (i16, U16), whose
// residuals are the unsigned type's (Signed, kmp_common.h).
template <typename T> struct natural_coder;
template <> struct natural_coder<uint8_t> { static constexpr int value = KMP_CODER_U8; };
template <> struct natural_coder<uint16_t> { static constexpr int value = KMP_CODER_U16; };
template <> struct natural_coder<int32_t> { static constexpr int value = KMP_CODER_RAW; };
template <> struct natural_coder<uint32_t> { static constexpr int value = KMP_CODER_U32; };
template <> struct natural_coder<i8s> { static constexpr int value = KMP_CODER_U8; };
template <> struct natural_coder<i16s> { static constexpr int value = KMP_CODER_U16; };

// the near-lossless coder of an 8- / 16-bit sample type (KMP_CODER_NEAR(code, max_error) requests)
template <typename T> struct near_coder {
  static_assert(sizeof(T) <= 2, "near coders: 8- / 16-bit samples");
  static constexpr int value = sizeof(T) == 1 ? KMP_CODER_NEAR_U8 : KMP_CODER_NEAR_U16;
};

// Kernel families, one per kmp_codec_<family>.hip.  Each returns KMP_ERR_UNSUPPORTED (without
// touching anything) when the request is not eligible, and knows nothing of the others: the order
// they are tried in is the table next to codec_encode / codec_decode (kmp_codec.hip).  The one-pass
// families are instantiated for uint8_t / uint16_t, wave3d32 for int32_t / uint32_t; the generic
// two-pass path for all four, and it takes every request.  Signed samples (i8s / i16s) are served by
// wave3d, wave2d and the generic path only: their lists in the table name no other family.
template <typename T, bool DEC> int try_wave3d(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_wave3d32(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_wave3dp(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_fast3d(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_linear3d(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_linear3dp(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_linear3m(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_linear3pm(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_wave2d(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_wave2dp(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_fast2d(const CodecCall<T, DEC>& c);
template <typename T, bool DEC> int try_generic(const CodecCall<T, DEC>& c);

#define KMP_INST_FAMILY(F, T)                           \
  template int F<T, false>(const CodecCall<T, false>&); \
  template int F<T, true>(const CodecCall<T, true>&);
#define KMP_INST_FAMILY_U8_U16(F) KMP_INST_FAMILY(F, uint8_t) KMP_INST_FAMILY(F, uint16_t)
#define KMP_INST_FAMILY_SIGNED(F) KMP_INST_FAMILY(F, i8s) KMP_INST_FAMILY(F, i16s)
#define KMP_FOR_SAMPLE_TYPES(M) M(uint8_t) M(uint16_t) M(int32_t) M(uint32_t) M(i8s) M(i16s)

// ------------------------------------------------------------------------------------------
// Host checks and argument filling the families share
// ------------------------------------------------------------------------------------------

// the region's span along axis ``a`` clamped to [0, E) (may come out empty: end <= begin)
inline void region_clamp(const kmp_region* region, const Geo& g, int a, int64_t& begin, int64_t& end) {
  begin = region->begin[a] < 0 ? 0 : region->begin[a];
  end = region->end[a] > g.E[a] ? g.E[a] : region->end[a];
}

// A region may only restrict ``axis`` (0: the z slabs of a volume, 1: the row ranges of an image,
// whose axis 0 is a dummy): [begin, end) is its clamped span; false when it restricts another axis
// or is empty.  No region: the whole axis.
inline bool region_span(const kmp_region* region, const Geo& g, int axis, int64_t& begin, int64_t& end) {
  begin = 0;
  end = g.E[axis];
  if (!region) return true;
  for (int a = 1; a < 3; ++a)
    if (a != axis && (region->begin[a] > 0 || region->end[a] < g.E[a])) return false;
  region_clamp(region, g, axis, begin, end);
  return end > begin;
}

// highres aligned to ``hi_align`` bytes, lowres and the first ``nmaps`` maps to ``lo_align``
template <typename T, bool DEC>
inline bool ptrs_aligned(const CodecCall<T, DEC>& c, size_t hi_align, size_t lo_align, int nmaps) {
  const void* hi = DEC ? (const void*)c.out : (const void*)c.in;
  const void* lo = DEC ? (const void*)c.in : (const void*)c.out;
  if (((uintptr_t)hi & (hi_align - 1)) || ((uintptr_t)lo & (lo_align - 1))) return false;
  for (int k = 0; k < nmaps; ++k)
    if ((uintptr_t)c.maps.p[k] & (lo_align - 1)) return false;
  return true;
}

// the kernel argument structs' pointers: encode reads hi_in and writes lo_out, decode reads lo_in
// and writes hi_out; the other pair stays null
template <typename A, typename T, bool DEC>
inline void bind(A& a, const CodecCall<T, DEC>& c) {
  if constexpr (DEC) {
    a.lo_in = c.in;
    a.hi_out = c.out;
  } else {
    a.hi_in = c.in;
    a.lo_out = c.out;
  }
  a.maps = c.maps;
}

// the 32-bit extents of the kernel argument structs (NSP = 2: no z members)
template <int NSP, typename A>
inline void set_extents(A& a, const Geo& g) {
  if constexpr (NSP == 3) {
    a.D = (int)g.n[0];
    a.Lz = (int)g.L[0];
    a.Ez = (int)g.E[0];
    a.Lcz = (int)g.Lc[0];
  }
  a.H = (int)g.n[1]; a.W = (int)g.n[2];
  a.Ly = (int)g.L[1]; a.Lx = (int)g.L[2];
  a.Ey = (int)g.E[1]; a.Ex = (int)g.E[2];
  a.Lcy = (int)g.Lc[1]; a.Lcx = (int)g.Lc[2];
}

// XCD-contiguous block order (xcd_block in kmp_wave.h) for batches that fill the 8 XCDs evenly:
// ``per`` blocks per tile, 0 = identity order (KMP_W3_XCD / KMP_W2_XCD = 0, or B % 8 != 0)
inline int xcd_per_tile(Opt xcd_opt, int64_t B, int64_t per) {
  return (opt(xcd_opt, 1) && B % 8 == 0) ? (int)per : 0;
}

}  // namespace kmp

// kmp_common.h -- shared device/host helpers for libkompressor_hip (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <limits>
#include <string>
#include <type_traits>

#include "../../include/kompressor_hip.h"

namespace kmp {

// ------------------------------------------------------------------------------------------
// Error plumbing: every C entry point returns a kmp_status and leaves a thread-local message.
// ------------------------------------------------------------------------------------------
void set_error(const std::string& msg);
int fail(int status, const std::string& msg);
int check_launch(const char* what);

// Device-side bounds checks of the debug build (``KMP_DEBUG=1 python kompressor_amd/_build.py``
// -> libkompressor_hip_debug.so, loaded when KMP_DEBUG=1): a failed check prints the kernel's
// file:line and the offending access, then traps so the fault is localised to one access instead
// of surfacing as a memory fault somewhere later.  Compiled out of the release library.
#ifdef KMP_DEBUG
#define KMP_DCHECK(cond, ...)                                                               \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      printf("KMP_DCHECK failed %s:%d: %s -- ", __FILE__, __LINE__, #cond);               \
      printf(__VA_ARGS__);                                                                 \
      printf("\n");                                                                        \
      __builtin_trap();                                                                    \
    }                                                                                      \
  } while (0)
#else
#define KMP_DCHECK(cond, ...) do { } while (0)
#endif

// [p, p + cnt) inside the array [base, base + n) (elements); a no-op in the release build
template <typename T>
__device__ __forceinline__ void dcheck_span(const T* base, const T* p, int64_t cnt, int64_t n, int line) {
  KMP_DCHECK(p >= base && p + cnt <= base + n, "line %d: access [%lld, %lld) of an array of %lld elements", line,
             (long long)(p - base), (long long)(p - base + cnt), (long long)n);
}
#define KMP_SPAN(base, p, cnt, n) ::kmp::dcheck_span((base), (p), (int64_t)(cnt), (int64_t)(n), __LINE__)

// ------------------------------------------------------------------------------------------
// Dispatch options (kmp_set_option): one table per process, seeded from the
// environment once at load (kmp_options.hip); a launch reads it with one relaxed atomic load.
// ------------------------------------------------------------------------------------------
enum Opt {
  OPT_DISABLE_WAVE, OPT_DISABLE_FAST, OPT_DISABLE_LINEAR_FUSED, OPT_DISABLE_ROWS, OPT_DISABLE_SWAR,
  OPT_W3_PL, OPT_W3P_PL, OPT_W3_XCD, OPT_W2_XCD, OPT_W3_ST_ENC, OPT_W3P_ST_ENC, OPT_W2_ST_ENC,
  OPT_W2P_ST_ENC, OPT_L3Y, OPT_LINEAR_F32_MFMA, OPT_W3_DEC_REV, OPT_W3_ST_TAIL, OPT_COUNT
};
// the option's value, or ``dflt`` while it is unset
int opt(Opt id, int dflt);

#define KMP_REQUIRE(cond, msg)                                         \
  do {                                                                 \
    if (!(cond)) return ::kmp::fail(KMP_ERR_ARG, std::string(__func__) + ": " + (msg)); \
  } while (0)

// ------------------------------------------------------------------------------------------
// dtype traits
// ------------------------------------------------------------------------------------------
// Signed 8- / 16-bit samples (KMP_I8 / KMP_I16).  Storage is the caller's two's-complement bit
// pattern; every arithmetic view of a sample is M(x) = x ^ signbit, the order-preserving map onto the
// unsigned type of the same width (DESIGN.md "Signed samples").  A kernel templated on its sample
// type gets the map from the conversions alone: reading a Signed<U> as a number gives M(x), and
// constructing one from a number stores M^-1 of it, so predictions, means and casts run on exactly
// the unsigned arithmetic.  Kernels that move packed registers apply sample_sign<T> themselves.
template <typename U>
struct Signed {
  static constexpr U kSign = (U)(U(1) << (8 * sizeof(U) - 1));
  U raw;
  Signed() = default;
  __host__ __device__ constexpr Signed(U mapped) : raw((U)(mapped ^ kSign)) {}
  __host__ __device__ constexpr operator U() const { return (U)(raw ^ kSign); }
};
using i8s = Signed<uint8_t>;
using i16s = Signed<uint16_t>;

// the sign bit M flips (0: the type is not mapped), and the unsigned type arithmetic runs in
template <typename T> struct sample_traits { static constexpr uint32_t sign = 0u; using mapped = T; };
template <typename U> struct sample_traits<Signed<U>> { static constexpr uint32_t sign = Signed<U>::kSign; using mapped = U; };
template <typename T> constexpr uint32_t sample_sign = sample_traits<T>::sign;
// 8- / 16-bit integer samples, mapped or not: the types with exact f32 sums and the saturating cast
template <typename T> constexpr bool is_small_sample =
    std::is_same<typename sample_traits<T>::mapped, uint8_t>::value || std::is_same<typename sample_traits<T>::mapped, uint16_t>::value;

template <int DT> struct dtype_of;
template <> struct dtype_of<KMP_U8> { using type = uint8_t; };
template <> struct dtype_of<KMP_U16> { using type = uint16_t; };
template <> struct dtype_of<KMP_I32> { using type = int32_t; };
template <> struct dtype_of<KMP_F32> { using type = float; };
template <> struct dtype_of<KMP_U32> { using type = uint32_t; };
template <> struct dtype_of<KMP_I8> { using type = i8s; };
template <> struct dtype_of<KMP_I16> { using type = i16s; };

inline int dtype_size(int dt) {
  switch (dt) {
    case KMP_U8: case KMP_I8: return 1;
    case KMP_U16: case KMP_I16: return 2;
    case KMP_I32: case KMP_F32: case KMP_U32: return 4;
    default: return 0;
  }
}

// Dispatch a runtime dtype to a templated callable: f(T{}) with T the element type.
template <typename F>
int dispatch_int_dtype(int dt, F&& f) {  // integer sample dtypes (highres / lowres / maps)
  switch (dt) {
    case KMP_U8: return f(uint8_t{});
    case KMP_U16: return f(uint16_t{});
    case KMP_I32: return f(int32_t{});
    case KMP_U32: return f(uint32_t{});
    default: return fail(KMP_ERR_ARG, "unsupported sample dtype " + std::to_string(dt));
  }
}
// integer sample dtypes of the launches that do arithmetic on samples: the signed ones too (the
// data-movement primitives take the same-width unsigned code instead)
template <typename F>
int dispatch_sample_dtype(int dt, F&& f) {
  if (dt == KMP_I8) return f(i8s{});
  if (dt == KMP_I16) return f(i16s{});
  return dispatch_int_dtype(dt, f);
}
template <typename F>
int dispatch_any_sample_dtype(int dt, F&& f) {
  if (dt == KMP_F32) return f(float{});
  return dispatch_sample_dtype(dt, f);
}
template <typename F>
int dispatch_any_dtype(int dt, F&& f) {
  if (dt == KMP_F32) return f(float{});
  return dispatch_int_dtype(dt, f);
}

// The same-width unsigned code of a signed sample dtype (any other code: itself).  The coders work
// mod 2^W, where M cancels: (M(gt) - M(pred)) mod 2^W == (gt - pred) mod 2^W, so the stand-alone
// coder launches run the unsigned kernels on the same bits.
inline int unsigned_twin(int dt) { return dt == KMP_I8 ? KMP_U8 : (dt == KMP_I16 ? KMP_U16 : dt); }

// ------------------------------------------------------------------------------------------
// Reference arithmetic restated on device
// ------------------------------------------------------------------------------------------

// ``astype(T)`` of a float32 as XLA does it: identity for float;
// truncation toward zero for integers, saturating at the range, NaN -> 0.
template <typename T>
__host__ __device__ __forceinline__ T cast_f32(float v) {
  if constexpr (std::is_same<T, float>::value) {
    return v;
  } else if constexpr (sample_sign<T> != 0) {
    return T(cast_f32<typename sample_traits<T>::mapped>(v));  // signed samples: the cast in the mapped domain
  } else {
    constexpr double lo = (double)std::numeric_limits<T>::min();
    constexpr double hi = (double)std::numeric_limits<T>::max();
    double t = (double)v;
    if (!(t == t)) return T(0);
    t = t < 0 ? ceil(t) : floor(t);
    if (t <= lo) return std::numeric_limits<T>::min();
    if (t >= hi) return std::numeric_limits<T>::max();
    return T(t);
  }
}

// ``jnp.int32(x)`` on an operand: integers wrap into int32, floats truncate (saturating).
template <typename T>
__host__ __device__ __forceinline__ int32_t to_i32(T v) {
  if constexpr (std::is_same<T, float>::value) return cast_f32<int32_t>(v);
  else return (int32_t)v;
}

// Coders: utils.py:28-55.  Every coder is "wrapping int32 add/sub, narrowed to the coder's
// width": ((a + 2^k) % 2^k) of an int32 equals its low k bits for a floor-mod.
template <int CODER> struct coder_out;
template <> struct coder_out<KMP_CODER_RAW> { using type = int32_t; };
template <> struct coder_out<KMP_CODER_U8> { using type = uint8_t; };
template <> struct coder_out<KMP_CODER_U16> { using type = uint16_t; };
template <> struct coder_out<KMP_CODER_U32> { using type = uint32_t; };

template <int CODER>
__host__ __device__ __forceinline__ typename coder_out<CODER>::type code_encode(int32_t pred, int32_t gt) {
  return (typename coder_out<CODER>::type)(uint32_t)((uint32_t)gt - (uint32_t)pred);
}
template <int CODER>
__host__ __device__ __forceinline__ typename coder_out<CODER>::type code_decode(int32_t pred, int32_t enc) {
  return (typename coder_out<CODER>::type)(uint32_t)((uint32_t)pred + (uint32_t)enc);
}

// numpy/jnp mode='symmetric' source index for any integer i (periodic mirror, period 2n).
__host__ __device__ __forceinline__ int64_t sym_index(int64_t i, int64_t n) {
  if (i >= 0 && i < n) return i;  // interior: no (emulated 64-bit) modulo
  if (i >= -n && i < 2 * n) return i < 0 ? -1 - i : 2 * n - 1 - i;  // one reflection
  int64_t m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}
template <typename I>
__device__ __forceinline__ I sym_idx(I i, I n) {  // sym_index in the kernel's index type
  if (i >= 0 && i < n) return i;
  if (i >= -n && i < 2 * n) return i < 0 ? -1 - i : 2 * n - 1 - i;
  I m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// ------------------------------------------------------------------------------------------
// Geometry of the reference's single pyramid level (volume/utils.py:226-237, 263-276)
// ------------------------------------------------------------------------------------------
struct Geo {
  int64_t n[3];    // highres extent per spatial axis (unpadded); unused axes = 1
  int64_t L[3];    // lowres nodes of the padded highres
  int64_t E[3];    // stored (trimmed) node extent = L - dims
  int64_t Lc[3];   // cells = L - 1
  int32_t dims[3]; // even padding
};

inline Geo make_geo_from_highres(int nsp, const int64_t* sp) {
  Geo g{};
  for (int a = 0; a < 3; ++a) {
    if (a < 3 - nsp) { g.n[a] = 1; g.L[a] = 1; g.E[a] = 1; g.Lc[a] = 1; g.dims[a] = 0; continue; }
    int64_t n = sp[a - (3 - nsp)];
    g.n[a] = n;
    g.dims[a] = (int32_t)((n + 1) % 2);
    g.L[a] = (n + g.dims[a] + 1) / 2;
    g.E[a] = g.L[a] - g.dims[a];
    g.Lc[a] = g.L[a] - 1;
  }
  return g;
}

inline Geo make_geo_from_lowres(int nsp, const int64_t* E, const int32_t* dims) {
  Geo g{};
  for (int a = 0; a < 3; ++a) {
    if (a < 3 - nsp) { g.n[a] = 1; g.L[a] = 1; g.E[a] = 1; g.Lc[a] = 1; g.dims[a] = 0; continue; }
    int i = a - (3 - nsp);
    g.E[a] = E[i];
    g.dims[a] = dims[i];
    g.L[a] = E[i] + dims[i];
    g.Lc[a] = g.L[a] - 1;
    g.n[a] = 2 * g.L[a] - 1 - dims[i];
  }
  return g;
}

// Map tables.  Class 0 is the lowres (all-even) class; classes 1..7 (1..3 in 2D) are the maps
// in the reference's order.  Parities are (z, y, x); in 2D z is a dummy axis.
// volume/utils.py:161-169 : LR(1,1,0) UD(1,0,1) FB(0,1,1) C(1,1,1) Z(1,0,0) Y(0,1,0) X(0,0,1)
// image/utils.py:92-94    : LR(y1,x0) UD(y0,x1) C(y1,x1)
__host__ __device__ __forceinline__ void map_parity(int nsp, int k, int par[3]) {
  if (nsp == 3) {
    const int t[7][3] = {{1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    par[0] = t[k][0]; par[1] = t[k][1]; par[2] = t[k][2];
  } else {
    const int t[3][2] = {{1, 0}, {0, 1}, {1, 1}};
    par[0] = 0; par[1] = t[k][0]; par[2] = t[k][1];
  }
}

// Extent of map k (0-based, excluding lowres) along axis a in its trimmed (stored) form.
inline int64_t map_extent(const Geo& g, int nsp, int k, int a) {
  int par[3];
  map_parity(nsp, k, par);
  if (a < 3 - nsp) return 1;
  return par[a] ? g.Lc[a] : g.E[a];
}

constexpr int kMaxMaps = 7;

struct MapPtrs {  // passed by value to kernels
  void* p[kMaxMaps];
};
struct CMapPtrs {
  const void* p[kMaxMaps];
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the grid-stride kernels' block size, and their grid for n work items
constexpr int kThreads = 256;
inline unsigned grid_for(int64_t n) {
  const int64_t g = ceil_div(n, kThreads);
  return (unsigned)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

// n / d for a wave-uniform 0 <= n < 2^31 and a launch-constant d >= 1 as q = mulhi(n, m) >> s (s < 0:
// d == 1, q = n), m = floor(2^(31+l) / d) + 1 with l = ceil(log2 d): exact on 31-bit n (error m d - 2^(31+l)
// is in (0, d] and n d < 2^(31+l)).  Computed on the host, so the kernel divides with two scalar
// instructions instead of a VALU reciprocal sequence with quarter-rate multiplies.
struct UDiv {
  uint32_t m;
  int32_t s;
};
inline UDiv make_udiv(uint32_t d) {
  if (d <= 1) return UDiv{0u, -1};
  int l = 0;
  while ((1ull << l) < d) ++l;
  return UDiv{(uint32_t)(((uint64_t)1 << (31 + l)) / d + 1), l - 1};
}
__device__ __forceinline__ uint32_t udiv(uint32_t n, UDiv f) {
  return f.s < 0 ? n : __umulhi(n, f.m) >> f.s;
}

// ------------------------------------------------------------------------------------------
// Near-lossless coders (KMP_CODER_NEAR_U8 / U16)
// ------------------------------------------------------------------------------------------
// The residual e = x - P of a sample against its prediction, clamped to [0, MAX], is quantised to
// q = sign(e) ((|e| + delta) / step), step = 2 delta + 1, and stored as W-bit two's complement
// (|q| <= (MAX + delta) / step < 2^(W-1)); the reconstruction is clamp(P + q step, 0, MAX), within
// delta of x with no modular wrap.  Signed samples are coded on M(x), as everywhere.  The bound
// reaches a kernel at run time in a NearQ; the modular coders carry no state (Lossless), so a
// kernel body templated on the state compiles to what it was without one.
template <> struct coder_out<KMP_CODER_NEAR_U8> { using type = uint8_t; };
template <> struct coder_out<KMP_CODER_NEAR_U16> { using type = uint16_t; };
template <int CODER> constexpr bool coder_is_near = CODER == KMP_CODER_NEAR_U8 || CODER == KMP_CODER_NEAR_U16;

struct Lossless {};
struct NearQ {
  int32_t delta, step;
  UDiv div;  // / step: exact below 2^31, and |e| + delta <= MAX + 2^(W-1) - 1 < 2^17
};
inline NearQ make_nearq(int32_t delta) { return NearQ{delta, 2 * delta + 1, make_udiv((uint32_t)(2 * delta + 1))}; }

// the low byte of a C-ABI ``coder`` argument is the kmp_coder, the rest the near coders' max_error
inline int coder_code(int32_t coder) { return coder & 0xff; }
inline int32_t coder_max_error(int32_t coder) { return (int32_t)((uint32_t)coder >> 8); }
inline bool is_near_code(int code) { return code == KMP_CODER_NEAR_U8 || code == KMP_CODER_NEAR_U16; }
// the float32 quantisers are kmp_code's alone: check_coder_arg refuses them everywhere else
inline bool is_quant_code(int code) { return code == KMP_CODER_QUANT_I16 || code == KMP_CODER_QUANT_I32; }
// so are the relative-error ones
inline bool is_prec_code(int code) { return code == KMP_CODER_PREC_I16 || code == KMP_CODER_PREC_I32; }
// KMP_OK for a well-formed ``coder`` argument whose sample width (bytes) is ``width``: a lossless
// code carries no max_error; a near code's width is the samples' (1 / 2; none for 32-bit samples:
// KMP_ERR_UNSUPPORTED) and 1 <= max_error <= 2^(W-1) - 1
inline int check_coder_arg(int32_t coder, int width, const char* who) {
  const int code = coder_code(coder);
  const int32_t delta = coder_max_error(coder);
  if (coder < 0 || code > KMP_CODER_NEAR_U16) return fail(KMP_ERR_ARG, std::string(who) + ": bad coder");
  if (!is_near_code(code))
    return delta ? fail(KMP_ERR_ARG, std::string(who) + ": a lossless coder takes no max_error") : KMP_OK;
  if (width == 4) return fail(KMP_ERR_UNSUPPORTED, std::string(who) + ": no near-lossless coder for 32-bit samples");
  if (width != (code == KMP_CODER_NEAR_U8 ? 1 : 2))
    return fail(KMP_ERR_ARG, std::string(who) + ": the near coder's width does not match the sample dtype");
  if (delta < 1 || delta > (1 << (8 * width - 1)) - 1)
    return fail(KMP_ERR_ARG, std::string(who) + ": max_error " + std::to_string(delta) + " outside [1, 2^(W-1) - 1]");
  return KMP_OK;
}

template <int CODER>
__device__ __forceinline__ typename coder_out<CODER>::type coder_enc(Lossless, int32_t pred, int32_t gt) {
  return code_encode<CODER>(pred, gt);
}
template <int CODER>
__device__ __forceinline__ typename coder_out<CODER>::type coder_dec(Lossless, int32_t pred, int32_t enc) {
  return code_decode<CODER>(pred, enc);
}
// ``gt`` in [0, MAX]; ``pred`` any int32 (an out-of-range float32 prediction, truncated)
template <int CODER>
__device__ __forceinline__ typename coder_out<CODER>::type coder_enc(const NearQ& q, int32_t pred, int32_t gt) {
  constexpr int32_t MAX = (int32_t)((1u << (8 * sizeof(typename coder_out<CODER>::type))) - 1u);
  const int32_t P = pred < 0 ? 0 : (pred > MAX ? MAX : pred);
  const int32_t e = gt - P;
  const int32_t k = (int32_t)udiv((uint32_t)((e < 0 ? -e : e) + q.delta), q.div);
  return (typename coder_out<CODER>::type)(uint32_t)(e < 0 ? -k : k);
}
// ``enc``: the stored W bits (any extension above them)
template <int CODER>
__device__ __forceinline__ typename coder_out<CODER>::type coder_dec(const NearQ& q, int32_t pred, int32_t enc) {
  constexpr int SH = 32 - 8 * (int)sizeof(typename coder_out<CODER>::type);
  constexpr int32_t MAX = (int32_t)(0xffffffffu >> SH);
  const int32_t P = pred < 0 ? 0 : (pred > MAX ? MAX : pred);
  const int32_t k = (int32_t)((uint32_t)enc << SH) >> SH;
  const int32_t r = P + k * q.step;  // |k| <= 2^(W-1), step < 2^W: no overflow
  return (typename coder_out<CODER>::type)(r < 0 ? 0 : (r > MAX ? MAX : r));
}

// 16-byte vectors: aligned, and any-alignment (gfx950 serves unaligned dwordx4 global accesses;
// rows of odd length are only element-aligned)
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));

// V = 16 / sizeof(T) consecutive elements moved as one 16-byte access
template <typename T>
struct Vec16 {
  static constexpr int V = 16 / (int)sizeof(T);
  T e[V];
  __device__ __forceinline__ void load(const T* p) {
    const u32x4u v = *(const u32x4u*)p;
    __builtin_memcpy(e, &v, 16);
  }
  __device__ __forceinline__ void store(T* p) const {
    u32x4u v;
    __builtin_memcpy(&v, e, 16);
    *(u32x4u*)p = v;
  }
};

// row-kernel work item: chunk j of row (b, z, y)
struct RowItem {
  int32_t b, z, y, j;
};
// item t over [B, nz, ny, nch] (all extents >= 1)
__device__ __forceinline__ RowItem row_item(uint32_t t, uint32_t nz, uint32_t ny, uint32_t nch) {
  RowItem r;
  r.j = (int32_t)(t % nch); t /= nch;
  r.y = (int32_t)(t % ny); t /= ny;
  r.z = (int32_t)(t % nz);
  r.b = (int32_t)(t / nz);
  return r;
}


// Flat index t over [B, e0, e1, e2, C] (C fastest).  The grid-stride kernels decompose one index
// per element: 64-bit division is a long emulated sequence on gfx950, so indices below 2^32 (every
// array axis and, in practice, every flat index fits) take 32-bit divisions; C == 1 skips one.
__device__ __forceinline__ void unflat5(int64_t t, int64_t e0, int64_t e1, int64_t e2, int64_t C, int64_t& b,
                                        int64_t& i0, int64_t& i1, int64_t& i2, int64_t& c) {
  if ((uint64_t)t < 0x100000000ull) {
    uint32_t u = (uint32_t)t;
    const uint32_t uC = (uint32_t)C, u2 = (uint32_t)e2, u1 = (uint32_t)e1, u0 = (uint32_t)e0;
    if (uC == 1) {
      c = 0;
    } else {
      c = u % uC;
      u /= uC;
    }
    i2 = u % u2; u /= u2;
    i1 = u % u1; u /= u1;
    i0 = u % u0;
    b = u / u0;
  } else {
    c = t % C; t /= C;
    i2 = t % e2; t /= e2;
    i1 = t % e1; t /= e1;
    i0 = t % e0;
    b = t / e0;
  }
}

}  // namespace kmp

// kmp_ssim.hip -- structural similarity of a restored array against its original (KMP_CODER_SSIM, DESIGN.md
// §23): the mean and the minimum of the SSIM index over every 7 x 7 (images) or 7 x 7 x 7 (volumes) window that
// lies wholly inside one item, uniform weights, sample variances -- the set and the formula scikit-image keeps.
//
// A workgroup owns UNITS: kSsimTileH x kSsimTileW window origins of one item, marched along z over kSsimTileD
// origins (one plane for images).  Per input plane it stages both arrays with their 6-sample halo in LDS,
// forms the box sums of x, r, x^2, r^2, x r (and, float32, of the non-finite flags) along W into LDS, a lane
// sums seven of those rows for its own origin, and a ring of the last six plane sums in registers closes the
// window along z.  Every window's moments are sums of that window's own terms in one fixed grouping: no
// running sum enters and leaves, so the float32 cancellation bound of §23 holds.
//
// Determinism: a lane's windows in unit order, the 64 lanes by shuffles at distances 32 .. 1, the waves in wave
// order, the workgroups in index order by a second one-wave launch.  The grid is a function of the count
// alone; the geometry is read from the request in ``out``.  No atomics, no tickets, no spinning.
#include "kmp_primitives.h"

namespace kmp {

constexpr int kSsimTH = KMP_SSIM_TILE_H, kSsimTW = KMP_SSIM_TILE_W, kSsimTD = KMP_SSIM_TILE_D;
constexpr int kSsimWin = 7;
constexpr int kSsimSH = kSsimTH + kSsimWin - 1, kSsimSW = kSsimTW + kSsimWin - 1;  // the staged plane: 22 x 22
// the staged row's stride in samples: 32 columns serve the widest 16-byte form (two chunks of 16 bytes of
// 8-bit samples), and 48 puts the four rows a wave reads 32 banks apart for 4- and 8-byte reads alike
constexpr int kSsimStride = 48;
constexpr int kSsimRows = kSsimSH * kSsimTW;  // row sums per plane
constexpr int kSsimWaves = kThreads / 64;
static_assert(kSsimTH * kSsimTW == kThreads, "one window origin per lane");
static_assert(2 * kThreads >= kSsimSH * kSsimSW && kThreads >= kSsimSH * 6, "the staging loops' trip counts");

// staged sample S, first moments A1, second moments A2
template <typename T>
struct SsimKind {  // 16-bit samples: 343 * 65535 < 2^25, 343 * 65535^2 < 2^41
  using S = uint32_t;
  using A1 = uint32_t;
  using A2 = uint64_t;
};
template <>
struct SsimKind<uint8_t> {  // 343 * 255^2 < 2^25
  using S = uint32_t;
  using A1 = uint32_t;
  using A2 = uint32_t;
};
template <>
struct SsimKind<float> {
  using S = double;
  using A1 = double;
  using A2 = double;
};

struct SsimReq {
  int64_t D, H, W, N;
  double c1, c2, base;
  bool ok;
};

__device__ __forceinline__ bool ssim_finite(uint64_t bits) {
  return (bits & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// the request at out + 64 bytes: D, H, W (int64), C1, C2, base (f64 bits); ``ok`` = well formed for n samples
__device__ __forceinline__ SsimReq ssim_request(const uint64_t* out, int64_t n) {
  SsimReq q;
  q.D = (int64_t)out[8];
  q.H = (int64_t)out[9];
  q.W = (int64_t)out[10];
  const uint64_t b1 = out[11], b2 = out[12], b3 = out[13];
  q.c1 = __longlong_as_double((long long)b1);
  q.c2 = __longlong_as_double((long long)b2);
  q.base = __longlong_as_double((long long)b3);
  q.N = 0;
  q.ok = (q.D == 1 || q.D >= kSsimWin) && q.H >= kSsimWin && q.W >= kSsimWin && q.D <= n && q.H <= n / q.D &&
         q.W <= n / (q.D * q.H) && n % (q.D * q.H * q.W) == 0 && ssim_finite(b1) && q.c1 > 0.0 && ssim_finite(b2) &&
         q.c2 > 0.0 && ssim_finite(b3);
  if (q.ok) q.N = n / (q.D * q.H * q.W);
  return q;
}

// the record's first five words as a lane holds them
struct SsimAcc {
  uint64_t windows, skipped;
  double sum, lo;
};

// a (earlier in the order) with b folded in
__device__ __forceinline__ void ssim_fold(SsimAcc& a, const SsimAcc& b) {
  a.windows += b.windows;
  a.skipped += b.skipped;
  a.sum += b.sum;
  a.lo = __builtin_fmin(a.lo, b.lo);
}

__device__ __forceinline__ uint64_t ssim_shfl_u64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d, 64);
  const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double ssim_shfl_f64(double v, int d) {
  return __longlong_as_double((long long)ssim_shfl_u64((uint64_t)__double_as_longlong(v), d));
}

// the fixed tree over the 64 lanes: lane 0 ends with the wave's value
__device__ __forceinline__ void ssim_wave_reduce(SsimAcc& a) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    SsimAcc b;
    b.windows = ssim_shfl_u64(a.windows, d);
    b.skipped = ssim_shfl_u64(a.skipped, d);
    b.sum = ssim_shfl_f64(a.sum, d);
    b.lo = ssim_shfl_f64(a.lo, d);
    ssim_fold(a, b);
  }
}

__device__ __forceinline__ void ssim_store(uint64_t* rec, const SsimAcc& a, bool ok) {
  rec[0] = a.windows;
  rec[1] = a.skipped;
  rec[2] = (uint64_t)__double_as_longlong(a.sum);
  rec[3] = (uint64_t)__double_as_longlong(a.lo);
  rec[4] = ok ? 0u : 1u;
  rec[5] = 0;
  rec[6] = 0;
  rec[7] = 0;
}

// the index of one window from its five sums, all in float64 (integer sums arrive exact)
__device__ __forceinline__ double ssim_index(double sx, double sr, double sxx, double srr, double sxr, double np,
                                             double inv_np, double inv_v, double c1, double c2) {
  const double mx = sx * inv_np, mr = sr * inv_np;
  const double vx = (np * sxx - sx * sx) * inv_v;
  const double vr = (np * srr - sr * sr) * inv_v;
  const double vxr = (np * sxr - sx * sr) * inv_v;
  return ((2.0 * mx * mr + c1) * (2.0 * vxr + c2)) / ((mx * mx + mr * mr + c1) * (vx + vr + c2));
}

// one plane's samples on their way from memory to LDS: a 16-byte chunk of each array, or two elements
template <typename T>
struct SsimFetch {
  u32x4v vx, vr;
  T ex[2], er[2];
};

// VEC: both pointers are 16-byte aligned, so rows are read in 16-byte chunks when W is a multiple of the chunk
template <typename T, bool VEC>
__global__ void __launch_bounds__(kThreads) ssim_kernel(const T* x, const T* r, int64_t n, uint32_t flip,
                                                      uint64_t* out) {
  using K = SsimKind<T>;
  using S = typename K::S;
  using A1 = typename K::A1;
  using A2 = typename K::A2;
  constexpr bool F = std::is_same<T, float>::value;
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int CH = (kSsimSW + V - 1) / V;  // chunks per staged row
  static_assert(CH * V <= kSsimStride, "a staged row holds its chunks");

  __shared__ S st_x[kSsimSH * kSsimStride], st_r[kSsimSH * kSsimStride];
  __shared__ uint8_t st_nf[F ? kSsimSH * kSsimStride : 4];
  __shared__ A1 w_x[kSsimRows], w_r[kSsimRows];
  __shared__ A2 w_xx[kSsimRows], w_rr[kSsimRows], w_xr[kSsimRows];
  __shared__ uint32_t w_nf[F ? kSsimRows : 1];
  __shared__ SsimAcc waves[kSsimWaves];

  const SsimReq q = ssim_request(out, n);
  SsimAcc acc{0, 0, 0.0, __builtin_inf()};
  const int tid = (int)threadIdx.x, ly = tid / kSsimTW, lx = tid % kSsimTW;

  if (q.ok) {
    const int kd = q.D == 1 ? 1 : kSsimWin;
    const int64_t OD = q.D - (kd - 1), OH = q.H - (kSsimWin - 1), OW = q.W - (kSsimWin - 1);
    const int64_t ntx = (OW + kSsimTW - 1) / kSsimTW, nty = (OH + kSsimTH - 1) / kSsimTH, nzc = (OD + kSsimTD - 1) / kSsimTD;
    const int64_t units = q.N * nzc * nty * ntx;
    const double np = kd == 1 ? 49.0 : 343.0, inv_np = 1.0 / np, inv_v = 1.0 / (np * (np - 1.0));
    const bool vec = VEC && q.W % V == 0;
    const int64_t plane = q.H * q.W;

    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
      int64_t t = u;
      const int64_t x0 = (t % ntx) * kSsimTW; t /= ntx;
      const int64_t y0 = (t % nty) * kSsimTH; t /= nty;
      const int64_t z0 = (t % nzc) * kSsimTD;
      const int64_t item = t / nzc;
      const int64_t zo = OD - z0 < kSsimTD ? OD - z0 : kSsimTD;  // origins along z
      const int planes = (int)zo + kd - 1;                        // input planes z0 .. z0 + planes - 1
      const int64_t item_off = item * q.D * plane;
      const bool counted = y0 + ly < OH && x0 + lx < OW;

      // where this lane reads: a chunk (row, c) or the elements idx = tid, tid + 256 of the 22 x 22 plane
      auto fetch = [&](int64_t z) {
        SsimFetch<T> f;
        const int64_t zoff = item_off + z * plane;
        if (vec) {
          f.vx = u32x4v{0, 0, 0, 0};
          f.vr = f.vx;
          const int row = tid / CH, c = tid % CH;
          const int64_t gy = y0 + row, gx = x0 + c * V;
          if (tid < kSsimSH * CH && gy < q.H && gx < q.W) {  // W % V == 0: a chunk is inside or outside whole
            const int64_t o = zoff + gy * q.W + gx;
            KMP_SPAN(x, x + o, V, n);
            f.vx = *(const u32x4v*)(x + o);
            f.vr = *(const u32x4v*)(r + o);
          }
        } else {
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int idx = tid + k * kThreads;
            const int row = idx / kSsimSW, col = idx % kSsimSW;
            const int64_t gy = y0 + row, gx = x0 + col;
            f.ex[k] = T(0);
            f.er[k] = T(0);
            if (idx < kSsimSH * kSsimSW && gy < q.H && gx < q.W) {
              const int64_t o = zoff + gy * q.W + gx;
              KMP_SPAN(x, x + o, 1, n);
              f.ex[k] = x[o];
              f.er[k] = r[o];
            }
          }
        }
        return f;
      };
      // one sample of each array into the staged plane at ``at``
      auto put = [&](int at, T xv, T rv) {
        if constexpr (F) {
          const uint32_t xb = __float_as_uint(xv), rb = __float_as_uint(rv);
          const bool fin = (xb & 0x7f800000u) != 0x7f800000u && (rb & 0x7f800000u) != 0x7f800000u;
          st_x[at] = fin ? (double)xv - q.base : 0.0;
          st_r[at] = fin ? (double)rv - q.base : 0.0;
          st_nf[at] = fin ? 0 : 1;
        } else {
          st_x[at] = (uint32_t)xv ^ flip;
          st_r[at] = (uint32_t)rv ^ flip;
        }
      };
      auto stage = [&](const SsimFetch<T>& f) {
        if (vec) {
          if (tid < kSsimSH * CH) {
            const int at = (tid / CH) * kSsimStride + (tid % CH) * V;
            const T* xx = (const T*)&f.vx;
            const T* rr = (const T*)&f.vr;
#pragma unroll
            for (int i = 0; i < V; ++i) put(at + i, xx[i], rr[i]);
          }
        } else {
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int idx = tid + k * kThreads;
            if (idx < kSsimSH * kSsimSW) put((idx / kSsimSW) * kSsimStride + idx % kSsimSW, f.ex[k], f.er[k]);
          }
        }
      };

      // the last six plane sums of this lane's origin, oldest first
      A1 g_x[kSsimWin - 1], g_r[kSsimWin - 1];
      A2 g_xx[kSsimWin - 1], g_rr[kSsimWin - 1], g_xr[kSsimWin - 1];
      uint32_t g_nf[kSsimWin - 1];
#pragma unroll
      for (int k = 0; k < kSsimWin - 1; ++k) {
        g_x[k] = g_r[k] = A1(0);
        g_xx[k] = g_rr[k] = g_xr[k] = A2(0);
        g_nf[k] = 0;
      }

      SsimFetch<T> f = fetch(z0);
      for (int p = 0; p < planes; ++p) {
        stage(f);
        __syncthreads();  // the plane is staged; the row sums of the plane before have been read
        if (p + 1 < planes) f = fetch(z0 + p + 1);
        // along W: 22 rows x 16 origins
        for (int i = tid; i < kSsimRows; i += kThreads) {
          const int at = (i / kSsimTW) * kSsimStride + i % kSsimTW;
          A1 ax = 0, ar = 0;
          A2 axx = 0, arr = 0, axr = 0;
          uint32_t anf = 0;
#pragma unroll
          for (int k = 0; k < kSsimWin; ++k) {
            const S xv = st_x[at + k], rv = st_r[at + k];
            ax += xv;
            ar += rv;
            axx += (A2)(xv * xv);  // 16-bit samples: a product fits 32 bits
            arr += (A2)(rv * rv);
            axr += (A2)(xv * rv);
            if constexpr (F) anf += st_nf[at + k];
          }
          w_x[i] = ax;
          w_r[i] = ar;
          w_xx[i] = axx;
          w_rr[i] = arr;
          w_xr[i] = axr;
          if constexpr (F) w_nf[i] = anf;
        }
        __syncthreads();  // the row sums are there; the staged plane has been read
        // along H: seven rows at this lane's origin
        A1 cx = 0, cr = 0;
        A2 cxx = 0, crr = 0, cxr = 0;
        uint32_t cnf = 0;
#pragma unroll
        for (int k = 0; k < kSsimWin; ++k) {
          const int i = (ly + k) * kSsimTW + lx;
          cx += w_x[i];
          cr += w_r[i];
          cxx += w_xx[i];
          crr += w_rr[i];
          cxr += w_xr[i];
          if constexpr (F) cnf += w_nf[i];
        }
        // along D: the six planes before, oldest first, then this one
        A1 tx = cx, tr = cr;
        A2 txx = cxx, trr = crr, txr = cxr;
        uint32_t tnf = cnf;
        if (kd != 1) {
          tx = g_x[0]; tr = g_r[0]; txx = g_xx[0]; trr = g_rr[0]; txr = g_xr[0]; tnf = g_nf[0];
#pragma unroll
          for (int k = 1; k < kSsimWin - 1; ++k) {
            tx += g_x[k]; tr += g_r[k]; txx += g_xx[k]; trr += g_rr[k]; txr += g_xr[k]; tnf += g_nf[k];
          }
          tx += cx; tr += cr; txx += cxx; trr += crr; txr += cxr; tnf += cnf;
#pragma unroll
          for (int k = 0; k < kSsimWin - 2; ++k) {
            g_x[k] = g_x[k + 1]; g_r[k] = g_r[k + 1]; g_xx[k] = g_xx[k + 1]; g_rr[k] = g_rr[k + 1];
            g_xr[k] = g_xr[k + 1]; g_nf[k] = g_nf[k + 1];
          }
          g_x[kSsimWin - 2] = cx; g_r[kSsimWin - 2] = cr; g_xx[kSsimWin - 2] = cxx; g_rr[kSsimWin - 2] = crr;
          g_xr[kSsimWin - 2] = cxr; g_nf[kSsimWin - 2] = cnf;
        }
        if (counted && p >= kd - 1) {
          if (F && tnf != 0) {
            acc.skipped += 1;
          } else {
            const double s = ssim_index((double)tx, (double)tr, (double)txx, (double)trr, (double)txr, np, inv_np,
                                        inv_v, q.c1, q.c2);
            acc.windows += 1;
            acc.sum += s;
            acc.lo = __builtin_fmin(acc.lo, s);
          }
        }
      }
      // the next unit's first plane is staged after this one's last row sums were formed (the barrier
      // above), and its row sums after the barrier that follows its staging: no barrier between units
    }
  }

  ssim_wave_reduce(acc);
  if ((tid & 63) == 0) waves[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSsimWaves; ++w) ssim_fold(acc, waves[w]);
    ssim_store(out + 8 * (2 + (int64_t)blockIdx.x), acc, q.ok);
  }
}

// one wave: lane l folds partials l, l + 64, ... in order, the tree, lane 0 writes the record
__global__ void __launch_bounds__(64) ssim_finish_kernel(uint64_t* out, int64_t n, int groups) {
  const SsimReq q = ssim_request(out, n);
  SsimAcc a{0, 0, 0.0, __builtin_inf()};
  if (q.ok) {
    for (int g = (int)threadIdx.x; g < groups; g += 64) {
      const uint64_t* rec = out + 8 * (2 + (int64_t)g);
      ssim_fold(a, SsimAcc{rec[0], rec[1], __longlong_as_double((long long)rec[2]),
                           __longlong_as_double((long long)rec[3])});
    }
  }
  ssim_wave_reduce(a);
  if (threadIdx.x == 0) ssim_store(out, a, q.ok);
}

template <typename T>
static int ssim_go(const void* x, const void* r, int64_t n, uint32_t flip, void* out, hipStream_t s) {
  const int64_t g = ceil_div(n, kSsimTH * kSsimTW);
  const unsigned grid = (unsigned)(g > KMP_SSIM_GROUPS ? KMP_SSIM_GROUPS : g);
  if ((((uintptr_t)x | (uintptr_t)r) & 15) == 0)
    ssim_kernel<T, true><<<grid, kThreads, 0, s>>>((const T*)x, (const T*)r, n, flip, (uint64_t*)out);
  else
    ssim_kernel<T, false><<<grid, kThreads, 0, s>>>((const T*)x, (const T*)r, n, flip, (uint64_t*)out);
  ssim_finish_kernel<<<1, 64, 0, s>>>((uint64_t*)out, n, (int)grid);
  return check_launch("ssim");
}

int launch_ssim(int dtype, const void* x, const void* r, int64_t n, void* out, hipStream_t stream) {
  switch (dtype) {
    case KMP_F32: return ssim_go<float>(x, r, n, 0u, out, stream);
    case KMP_U8: return ssim_go<uint8_t>(x, r, n, 0u, out, stream);
    case KMP_U16: return ssim_go<uint16_t>(x, r, n, 0u, out, stream);
    case KMP_I8: return ssim_go<uint8_t>(x, r, n, 0x80u, out, stream);
    case KMP_I16: return ssim_go<uint16_t>(x, r, n, 0x8000u, out, stream);
    default: return fail(KMP_ERR_ARG, "kmp_code: ssim takes float32, uint8, uint16, int8 or int16 samples");
  }
}

}  // namespace kmp

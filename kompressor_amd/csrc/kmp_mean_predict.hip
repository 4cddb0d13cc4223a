// kmp_mean_predict.hip -- the mean predictor as an opaque callable: kmp_mean_predict_maps[_typed] turn a padded
// lowres window into the 7 (3) prediction maps the reference's mean predictions_fn returns.  Kernel families, in
// the order they are tried: eight positions per lane (p = 0), one workgroup per output plane, the z-rolling rows
// kernel, and the two-pass element fallback (the cell means here, their aggregation in kmp_maps_from_predictions.hip).
#include "kmp_primitives.h"
#include "kmp_wave.h"

namespace kmp {

// Fused mean predictor on a padded window (u8 / u16, C == 1): the z-rolling LDS aggregation of
// maps_from_predictions_lds_kernel with the staged cell plane computed on the fly -- cell
// (z, y, x) = astype(T)(f32 sum of its (2p+2)^d window nodes / N), exactly cell_mean_padded --
// so the cell means are written once (as the C map, straight from LDS) and never re-read from
// HBM; the two element kernels below (cell means, then maps) stay for the other layouts.
constexpr int kMpCpt = 4;  // cells per thread per staged plane (host-checked)

template <typename T, int NSP>
__global__ void __launch_bounds__(kThreads) mean_predict_lds_kernel(
    const T* __restrict__ win, E3<int32_t> S, int p, int32_t Lcz, int32_t Lcy, int32_t Lcx, MapPtrs outs, int32_t YB,
    int32_t XO, int32_t ZC, int32_t nzc, int32_t nyb, int32_t nxb, int32_t RP) {
  constexpr int NM = NSP == 3 ? 7 : 3;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* lds = (uint32_t*)smem;  // [2 slots][YB + 1 rows][RP] cell means
  int32_t w = (int32_t)blockIdx.x;
  const int32_t xb = w % nxb; w /= nxb;
  const int32_t yb = w % nyb; w /= nyb;
  const int32_t zc = w % nzc;
  const int32_t b = w / nzc;
  const int32_t y0 = yb * YB, ox0 = xb * XO;
  const int32_t xc0 = ox0 > 0 ? ox0 - 1 : 0;
  const int32_t xc1 = (ox0 + XO - 1 < Lcx - 1) ? ox0 + XO - 1 : Lcx - 1;
  const int32_t ncx = xc1 - xc0 + 1;
  const int32_t cz = NSP == 3 ? Lcz : 1;
  const int32_t fz = NSP == 3 ? Lcz + 1 : 1;
  const int32_t oz0 = zc * ZC, oz1 = (oz0 + ZC < fz) ? oz0 + ZC : fz;
  const int kk = 2 * p + 2, kz = NSP == 3 ? kk : 1;
  const float nn = (float)(kz * kk * kk);
  const int32_t slice = (YB + 1) * ncx;
  const float rcp = 1.0f / (float)ncx;

  uint32_t buf[kMpCpt];
  auto fetch = [&](int32_t z) {  // cell means of cell plane z -> registers
#pragma unroll
    for (int c = 0; c < kMpCpt; ++c) {
      buf[c] = 0;
      const int32_t i = threadIdx.x + c * kThreads;
      if (i >= slice) continue;
      int32_t r, x;
      divmod_small(i, ncx, rcp, r, x);
      const int32_t y = y0 - 1 + r;
      if (y < 0 || y >= Lcy) continue;
      float sum = 0.0f;  // f32 sum in feature order (exact here: < 2^24)
      for (int dz = 0; dz < kz; ++dz)
        for (int dy = 0; dy < kk; ++dy) {
          const T* row = win + ((b * S.e[0] + z + dz) * S.e[1] + y + dy) * S.e[2] + xc0 + x;
          for (int dx = 0; dx < kk; ++dx) sum += (float)row[dx];
        }
      buf[c] = (uint32_t)cast_f32<T>(sum / nn);
    }
  };
  auto put = [&](int32_t z) {
    uint32_t* base = lds + (z & 1) * (YB + 1) * RP;
#pragma unroll
    for (int c = 0; c < kMpCpt; ++c) {
      const int32_t i = threadIdx.x + c * kThreads;
      if (i >= slice) continue;
      int32_t r, x;
      divmod_small(i, ncx, rcp, r, x);
      base[r * RP + x] = buf[c];
    }
  };
  auto at = [&](int32_t z, int32_t r, int32_t x) -> uint32_t { return lds[((z & 1) * (YB + 1) + r) * RP + (x - xc0)]; };

  if (NSP == 3 && oz0 >= 1) {
    fetch(oz0 - 1);
    put(oz0 - 1);
  }
  if (oz0 < cz) {
    fetch(oz0);
    put(oz0);
  }
  __syncthreads();

  for (int32_t oz = oz0; oz < oz1; ++oz) {
    const bool more = oz + 1 < oz1 && oz + 1 < cz;
    if (more) fetch(oz + 1);
    for (int32_t i = threadIdx.x; i < YB * XO; i += kThreads) {
      const int32_t xo = i % XO, r = i / XO;
      const int32_t oy = y0 + r, ox = ox0 + xo;
      if (oy > Lcy || ox > Lcx) continue;
#pragma unroll
      for (int k = 0; k < NM; ++k) {
        int par[3];
        map_parity(NSP, k, par);
        const int32_t e0 = NSP == 3 ? (par[0] ? Lcz : Lcz + 1) : 1, e1 = par[1] ? Lcy : Lcy + 1,
                      e2 = par[2] ? Lcx : Lcx + 1;
        if (oz >= e0 || oy >= e1 || ox >= e2) continue;
        Contrib cb[4];
        const int nc = map_contribs(NSP, k, cb);
        uint32_t sum = 0, cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= nc) break;
          const int32_t z = oz - cb[j].dz, y = oy - cb[j].dy, x = ox - cb[j].dx;
          if (z >= 0 && z < cz && y >= 0 && y < Lcy && x >= 0 && x < Lcx) {
            sum += at(z, r + 1 - cb[j].dy, x);
            ++cnt;
          }
        }
        ((T*)outs.p[k])[((b * e0 + oz) * e1 + oy) * e2 + ox] = (T)(k == center_map(NSP) ? sum : sum >> (cnt >> 1));
      }
    }
    if (!more) break;  // uniform
    __syncthreads();
    put(oz + 1);
    __syncthreads();
  }
}

// Words of padding before and after the two LDS cell planes of the mean predictor kernels.
__host__ __device__ __forceinline__ int32_t mp_pad_words(int64_t Lcx) { return (int32_t)(4 * ((Lcx + 4) / 4)); }

// Row mapping of a plane's positions onto the workgroup: a wave covers R = 64 / W rows of W
// consecutive x positions (lane = r * W + x), the 4 waves interleave row groups.  Every lane's
// (row, x) is fixed per call, so the per-position work has no index division, and the
// conditions that depend on the row (first / last row) change only between row groups.
struct RowMap {
  int32_t lr, lx, R;  // this lane's row within the group, its x, rows per wave
  bool lane_ok;
};
__device__ __forceinline__ RowMap row_map(int32_t W) {
  RowMap m;
  const int32_t lane = threadIdx.x & 63;
  m.R = 64 / W;
  m.lr = (int32_t)((float)lane * (1.0f / (float)W));  // lane < 64: exact after the fix-up
  if (m.lr * W > lane) --m.lr;
  else if ((m.lr + 1) * W <= lane) ++m.lr;
  m.lx = lane - m.lr * W;
  m.lane_ok = m.lr < m.R;
  return m;
}

// The 7 maps at the output positions of plane oz from two LDS cell planes (cell plane oz in slot
// s_cur, oz - 1 in s_prev; ``cells`` must have Lcx + 1 readable words before slot 0 and after
// slot 1).  Positions
// ox < Lcx go through the row mapping in x chunks of <= 64; the last column (ox == Lcx, where
// only the three maps with an even x parity exist and only the cells at ox - 1 contribute) is a
// separate pass with one lane per row.
template <typename T, typename O>
__device__ __forceinline__ void mean_maps_plane(const uint32_t* cells, int32_t oz, int64_t b, int32_t Lcz,
                                                int32_t Lcy, int32_t Lcx, const MapPtrs& outs, int s_cur, int s_prev) {
  const int32_t nplanes = Lcz + 1, oyn = Lcy + 1, oxn = Lcx + 1, cplane = Lcy * Lcx;
  const bool z0 = oz < Lcz, z1 = oz >= 1;  // cell planes oz and oz - 1 exist
  O* const o0 = (O*)outs.p[0] + ((b * Lcz + oz) * Lcy) * oxn;       // LR (1,1,0)
  O* const o1 = (O*)outs.p[1] + ((b * Lcz + oz) * oyn) * Lcx;       // UD (1,0,1)
  O* const o2 = (O*)outs.p[2] + ((b * nplanes + oz) * Lcy) * Lcx;   // FB (0,1,1)
  O* const o3 = (O*)outs.p[3] + ((b * Lcz + oz) * Lcy) * Lcx;       // C  (1,1,1)
  O* const o4 = (O*)outs.p[4] + ((b * Lcz + oz) * oyn) * oxn;       // Z  (1,0,0)
  O* const o5 = (O*)outs.p[5] + ((b * nplanes + oz) * Lcy) * oxn;   // Y  (0,1,0)
  O* const o6 = (O*)outs.p[6] + ((b * nplanes + oz) * oyn) * Lcx;   // X  (0,0,1)
  const uint32_t* cur = cells + s_cur * cplane;
  const uint32_t* prev = cells + s_prev * cplane;
  const uint32_t nz = (uint32_t)z0 + z1;
  const int32_t wv = threadIdx.x >> 6;
  for (int32_t xc = 0; xc < Lcx; xc += 64) {
    const RowMap m = row_map(Lcx - xc < 64 ? Lcx - xc : 64);
    const int32_t ox = xc + m.lx;
    const bool x1 = ox >= 1;
    for (int32_t oy0 = wv * m.R; oy0 <= Lcy; oy0 += 4 * m.R) {
      const int32_t oy = oy0 + m.lr;
      if (!m.lane_ok || oy > Lcy) continue;
      const bool y0 = oy < Lcy, y1 = oy >= 1;
      const int32_t q = oy * Lcx + ox;  // cell (oy, ox)
      // c<z><y><x>: cell (oz - z, oy - y, ox - x); 0 where it does not exist.  The reads are
      // unconditional (the cell slots carry Lcx + 1 words of padding on both sides, so every
      // index here stays inside the workgroup's LDS) and masked afterwards: no exec-mask
      // branch per read.
      const uint32_t mz0 = z0 ? ~0u : 0u, mz1 = z1 ? ~0u : 0u;
      const uint32_t my0 = y0 ? ~0u : 0u, my1 = y1 ? ~0u : 0u, mx1 = x1 ? ~0u : 0u;
      const uint32_t c000 = cur[q] & (mz0 & my0), c001 = cur[q - 1] & (mz0 & my0 & mx1);
      const uint32_t c010 = cur[q - Lcx] & (mz0 & my1), c011 = cur[q - Lcx - 1] & (mz0 & my1 & mx1);
      const uint32_t c100 = prev[q] & (mz1 & my0), c101 = prev[q - 1] & (mz1 & my0 & mx1);
      const uint32_t c110 = prev[q - Lcx] & (mz1 & my1);
      const uint32_t nx = 1u + x1, ny = (uint32_t)y0 + y1;
      const int32_t px = oy * oxn + ox, pc = oy * Lcx + ox;
      o6[pc] = (O)((c000 + c010 + c110 + c100) >> ((nz * ny) >> 1));
      if (z0) {
        o1[pc] = (O)((c000 + c010) >> (ny >> 1));
        o4[px] = (O)((c000 + c001 + c011 + c010) >> ((ny * nx) >> 1));
      }
      if (y0) {
        o2[pc] = (O)((c000 + c100) >> (nz >> 1));
        o5[px] = (O)((c000 + c001 + c101 + c100) >> ((nz * nx) >> 1));
        if (z0) {
          o0[px] = (O)((c000 + c001) >> (nx >> 1));
          o3[pc] = (O)c000;
        }
      }
    }
  }
  // the last column, ox = Lcx: LR, Z, Y from the cells at x = Lcx - 1
  for (int32_t oy = threadIdx.x; oy <= Lcy; oy += kThreads) {
    const bool y0 = oy < Lcy, y1 = oy >= 1;
    const int32_t q = oy * Lcx + Lcx - 1;
    const uint32_t c001 = cur[q] & (z0 && y0 ? ~0u : 0u), c011 = cur[q - Lcx] & (z0 && y1 ? ~0u : 0u);
    const uint32_t c101 = prev[q] & (z1 && y0 ? ~0u : 0u);
    const uint32_t ny = (uint32_t)y0 + y1;
    const int32_t px = oy * oxn + Lcx;
    if (z0) o4[px] = (O)((c001 + c011) >> (ny >> 1));
    if (y0) {
      o5[px] = (O)((c001 + c101) >> (nz >> 1));
      if (z0) o0[px] = (O)c001;
    }
  }
}

// Fused mean predictor, one workgroup per output plane (3D, u8 / u16, C == 1, p <= 2).  The
// 2p+3 window planes that output plane oz reads are copied into LDS as one contiguous byte range
// with 16-byte loads; the two cell planes it aggregates (oz - 1 and oz) are summed there --
// directly for p = 0 (8 nodes), separably for p >= 1 (x sums of 2p+2 nodes first, then the
// (2p+2)^2 box of x sums) -- and each thread then owns output positions (oy, ox) and writes all 7
// maps at that position from the 8 cells around it.  The rolling kernel above fetches every
// node of every cell with its own 2-byte global load; that was its cost (131 -> 93 us for the
// 512 C3 windows).  A z-rolling variant of this kernel (3-slot node ring, next plane prefetched
// in registers, each cell plane summed once) measured slower, 100-108 us: the plane-parallel grid
// hides the load latency as well and has 8x the workgroups.
// PPB output planes per workgroup (1 or 2): with 2, the cell plane between them is summed once
// for both (3 cell planes for 2 outputs instead of 4) -- the kernel is VALU-bound
// (profiles/round2/sq_callback_kernels.txt)
template <typename T, int P, int PPB, typename O = T>
__global__ void __launch_bounds__(kThreads) mean_predict_plane_kernel(
    const T* __restrict__ win, E3<int32_t> S, int32_t Lcz, int32_t Lcy, int32_t Lcx, MapPtrs outs, int32_t xcd_per,
    int32_t nodes_bytes, int32_t xs_bytes) {
  static_assert(PPB == 1 || PPB == 2, "one or two output planes per workgroup");
  constexpr int KK = 2 * P + 2;
  constexpr float NN = (float)(KK * KK * KK);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int32_t nplanes = Lcz + 1, ngrp = (nplanes + PPB - 1) / PPB;
  // consecutive planes of one window on one XCD: shared node planes hit its L2
  int32_t blk = wv::xcd_block((int32_t)blockIdx.x, xcd_per);
  const int32_t oz = (blk % ngrp) * PPB;  // the first output plane; cell slot s is plane oz - 1 + s
  const int64_t b = blk / ngrp;
  const int32_t S1 = S.e[1], S2 = S.e[2], plane = S1 * S2;
  const int32_t zlo = oz >= 1 ? oz - 1 : 0;
  const int32_t zhi = oz + PPB - 1 + KK < S.e[0] ? oz + PPB - 1 + KK : S.e[0];  // node planes [zlo, zhi)

  // ---- node planes -> LDS: the aligned 16-byte blocks covering the byte range; the partial
  // blocks at either end copy only the window's own bytes ----
  const unsigned char* g0 = (const unsigned char*)(win + (b * S.e[0] + zlo) * (int64_t)plane);
  const int32_t shift = (int32_t)((uintptr_t)g0 & 15);
  const int32_t nbytes = (zhi - zlo) * plane * (int32_t)sizeof(T);
  const uint4* src = (const uint4*)(g0 - shift);
  const int32_t nchunk = (nbytes + shift + 15) >> 4;
  for (int32_t i = threadIdx.x; i < nchunk; i += kThreads) {
    const int32_t lo = 16 * i - shift;  // byte range [lo, lo + 16) of the window planes
    if (lo >= 0 && lo + 16 <= nbytes) {
      *(uint4*)(smem + 16 * i) = src[i];
    } else {  // the partial first / last block: only its bytes inside the window, element by element
      for (int32_t k = lo < 0 ? 0 : lo; k < lo + 16 && k < nbytes; k += (int32_t)sizeof(T))
        *(T*)(smem + shift + k) = *(const T*)(g0 + k);
    }
  }
  const T* nodes = (const T*)(smem + shift);  // [z - zlo][y][x]
  uint32_t* xs = (uint32_t*)(smem + nodes_bytes);  // p >= 1: [z - zlo][y][cx] sums over x
  // [slot: z = oz - 1 + slot][cy][cx], PPB + 1 slots, after a pad of >= Lcx + 1 words
  uint32_t* cells = (uint32_t*)(smem + nodes_bytes + xs_bytes) + mp_pad_words(Lcx);
  __syncthreads();

  const int32_t cplane = Lcy * Lcx;
  const float rcx = 1.0f / (float)Lcx;
  if constexpr (P > 0) {
    const int32_t nxs = (zhi - zlo) * S1 * Lcx;
    for (int32_t i = threadIdx.x; i < nxs; i += kThreads) {
      int32_t zy, cx;
      divmod_small(i, Lcx, rcx, zy, cx);
      const T* row = nodes + zy * S2 + cx;  // (z - zlo) * plane + y * S2 == zy * S2
      uint32_t s = 0;
#pragma unroll
      for (int dx = 0; dx < KK; ++dx) s += row[dx];
      xs[i] = s;
    }
    __syncthreads();
  }
  // cell planes oz - 1 .. oz + PPB - 1 (slots 0 .. PPB), rows of all through the row mapping
  const int32_t wv = threadIdx.x >> 6;
  for (int32_t xc = 0; xc < Lcx; xc += 64) {
    const RowMap m = row_map(Lcx - xc < 64 ? Lcx - xc : 64);
    const int32_t cx = xc + m.lx;
    for (int32_t r0 = wv * m.R; r0 < (PPB + 1) * Lcy; r0 += 4 * m.R) {
      const int32_t r = r0 + m.lr;
      const int32_t slot = PPB == 1 ? (int32_t)(r >= Lcy) : (int32_t)(r >= Lcy) + (int32_t)(r >= 2 * Lcy);
      const int32_t cy = r - slot * Lcy;
      const int32_t z = oz - 1 + slot;
      if (!m.lane_ok || r >= (PPB + 1) * Lcy || z < 0 || z >= Lcz) continue;  // (a missing plane is never read)
      uint32_t s = 0;
      if constexpr (P == 0) {
        const T* q = nodes + (z - zlo) * plane + cy * S2 + cx;
        s = (uint32_t)q[0] + q[1] + q[S2] + q[S2 + 1] + q[plane] + q[plane + 1] + q[plane + S2] + q[plane + S2 + 1];
      } else {
#pragma unroll
        for (int dz = 0; dz < KK; ++dz)
#pragma unroll
          for (int dy = 0; dy < KK; ++dy) s += xs[((z - zlo + dz) * S1 + cy + dy) * Lcx + cx];
      }
      cells[slot * cplane + cy * Lcx + cx] = (uint32_t)cast_f32<T>((float)s / NN);  // exact sum (< 2^24)
    }
  }
  __syncthreads();

  mean_maps_plane<T, O>(cells, oz, b, Lcz, Lcy, Lcx, outs, 1, 0);
  if (PPB == 2 && oz + 1 < nplanes) mean_maps_plane<T, O>(cells, oz + 1, b, Lcz, Lcy, Lcx, outs, 2, 1);
}

// ---- p = 0, eight x positions per lane (3D, C == 1, Lcx % 8 == 0) ----
// The same maps as mean_predict_plane_kernel<T, 0, *> with the per-position work cut to adds and
// shifts: the LDS cell planes carry a zero border (row -1 / Lcy, column -1, whole planes -1 /
// Lcz), so a cell that does not exist reads 0 and no read is masked, and each map is a sum of the
// existing cells shifted by log2 of their count (the per-axis flags sz, sy, sx below).  A lane
// owns 8 consecutive x of one row: 2 x 16-byte node-row loads per cell row, 2 ds_read_b128 + 1
// ds_read_b32 per cell row read, one 8-element store per map.  A workgroup computes ZP output
// planes from ZP + 1 cell planes (cell plane oz - 1 is summed by two workgroups).

typedef uint32_t u32x2u __attribute__((ext_vector_type(2), aligned(1)));

// nodes p[0 .. 8] of a window row (unaligned: rows of odd length)
template <typename T>
__device__ __forceinline__ void load_row9(const T* p, uint32_t (&n)[9]) {
  if constexpr (sizeof(T) == 2) {
    const u32x4u v = *(const u32x4u*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      n[2 * k] = v[k] & 0xFFFFu;
      n[2 * k + 1] = v[k] >> 16;
    }
  } else {
    const u32x2u v = *(const u32x2u*)p;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) n[4 * k + i] = (v[k] >> (8 * i)) & 0xFFu;
  }
  n[8] = p[8];
}

// 8 map values (each < 2^(8 sizeof(T))) as O at p (element-aligned)
template <typename O>
__device__ __forceinline__ void store_row8(O* p, const uint32_t (&v)[8]) {
  if constexpr (std::is_same<O, float>::value) {
    u32x4u a, b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] = __float_as_uint((float)v[k]);
      b[k] = __float_as_uint((float)v[4 + k]);
    }
    *(u32x4u*)p = a;
    *(u32x4u*)(p + 4) = b;
  } else if constexpr (sizeof(O) == 2) {
    u32x4u a;
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = v[2 * k] | (v[2 * k + 1] << 16);
    *(u32x4u*)p = a;
  } else {
    u32x2u a;
#pragma unroll
    for (int k = 0; k < 2; ++k) a[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
    *(u32x2u*)p = a;
  }
}

// words of one LDS cell plane: rows -1 .. Lcy, pitch Lcx + 8 (cell x at word x + 4: 16-byte aligned)
__host__ __device__ __forceinline__ int32_t mp8_plane_words(int32_t Lcy, int32_t Lcx) { return (Lcy + 2) * (Lcx + 8); }

template <typename T, typename O>
__global__ void __launch_bounds__(kThreads) mean_predict_p0x8_kernel(const T* __restrict__ win, E3<int32_t> S,
                                                                    int32_t Lcz, int32_t Lcy, int32_t Lcx, MapPtrs outs,
                                                                    int32_t xcd_per, int32_t ZP, int32_t ngrp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cl[];  // [ZP + 1][Lcy + 2][Lcx + 8]
  // the groups of one window on one XCD (their shared node planes hit its L2)
  int32_t blk = wv::xcd_block((int32_t)blockIdx.x, xcd_per);
  const int32_t b = blk / ngrp, z0 = (blk - b * ngrp) * ZP;  // output planes z0 .. z0 + ZP - 1
  const int32_t RP = Lcx + 8, PW = mp8_plane_words(Lcy, Lcx), NJ = Lcx >> 3;
  const int32_t S1 = S.e[1], S2 = S.e[2];

  // zero border (and the planes outside the window's cells)
  for (int32_t i = threadIdx.x; i < (ZP + 1) * PW / 4; i += kThreads) ((uint4*)cl)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();

  // cell planes zc = z0 - 1 + s: 8 cells per lane = (8 nodes) >> 3, summed over 4 node rows
  const float rnj = 1.0f / (float)NJ, rlcy = 1.0f / (float)Lcy;
  for (int32_t t = threadIdx.x; t < (ZP + 1) * Lcy * NJ; t += kThreads) {
    int32_t sy, j, s, cy;
    divmod_small(t, NJ, rnj, sy, j);
    divmod_small(sy, Lcy, rlcy, s, cy);
    const int32_t zc = z0 - 1 + s;
    if (zc < 0 || zc >= Lcz) continue;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        uint32_t n[9];
        load_row9<T>(win + (((int64_t)b * S.e[0] + zc + dz) * S1 + cy + dy) * S2 + 8 * j, n);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += n[i] + n[i + 1];
      }
    uint32_t* dst = cl + s * PW + (cy + 1) * RP + 4 + 8 * j;
    *(uint4*)dst = make_uint4(acc[0] >> 3, acc[1] >> 3, acc[2] >> 3, acc[3] >> 3);
    *(uint4*)(dst + 4) = make_uint4(acc[4] >> 3, acc[5] >> 3, acc[6] >> 3, acc[7] >> 3);
  }
  __syncthreads();

  const int32_t nz = Lcz + 1 - z0 < ZP ? Lcz + 1 - z0 : ZP;  // output planes of this group
  const int32_t oyn = Lcy + 1, oxn = Lcx + 1;
  const float roy = 1.0f / (float)oyn;
  // cells x = 8j - 1 .. 8j + 7 of one LDS row
  auto row9 = [&](const uint32_t* r, int32_t j, uint32_t (&v)[9]) {
    v[0] = r[3 + 8 * j];
    const uint4 a = *(const uint4*)(r + 4 + 8 * j), c = *(const uint4*)(r + 8 + 8 * j);
    v[1] = a.x; v[2] = a.y; v[3] = a.z; v[4] = a.w;
    v[5] = c.x; v[6] = c.y; v[7] = c.z; v[8] = c.w;
  };
  for (int32_t t = threadIdx.x; t < nz * oyn * NJ; t += kThreads) {
    int32_t py, j, pz, oy;
    divmod_small(t, NJ, rnj, py, j);
    divmod_small(py, oyn, roy, pz, oy);
    const int32_t oz = z0 + pz, ox = 8 * j;
    const bool z0f = oz < Lcz, y0f = oy < Lcy;
    const uint32_t sz = (uint32_t)(z0f && oz >= 1), sy = (uint32_t)(y0f && oy >= 1);
    const uint32_t* cur = cl + (pz + 1) * PW;  // cell plane oz
    const uint32_t* prv = cl + pz * PW;        // cell plane oz - 1
    uint32_t a[9], bb[9], c[9], d[9];          // cur row oy, cur row oy - 1, prev row oy, prev row oy - 1
    row9(cur + (oy + 1) * RP, j, a);
    row9(cur + oy * RP, j, bb);
    row9(prv + (oy + 1) * RP, j, c);
    row9(prv + oy * RP, j, d);
    uint32_t m0[8], m1[8], m2[8], m3[8], m4[8], m5[8], m6[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t sx = i > 0 ? 1u : (uint32_t)(ox >= 1);
      const uint32_t lr = a[i + 1] + a[i];
      m0[i] = lr >> sx;                                          // LR (1,1,0)
      m1[i] = (a[i + 1] + bb[i + 1]) >> sy;                      // UD (1,0,1)
      m2[i] = (a[i + 1] + c[i + 1]) >> sz;                       // FB (0,1,1)
      m3[i] = a[i + 1];                                          // C  (1,1,1)
      m4[i] = (lr + bb[i] + bb[i + 1]) >> (sy + sx);             // Z  (1,0,0)
      m5[i] = (lr + c[i] + c[i + 1]) >> (sz + sx);               // Y  (0,1,0)
      m6[i] = (a[i + 1] + bb[i + 1] + c[i + 1] + d[i + 1]) >> (sz + sy);  // X (0,0,1)
    }
    const int32_t zL = b * Lcz + oz, zN = b * (Lcz + 1) + oz;  // plane index in a map of Lcz / Lcz + 1 planes
    store_row8<O>((O*)outs.p[6] + (zN * oyn + oy) * Lcx + ox, m6);
    if (z0f) {
      store_row8<O>((O*)outs.p[1] + (zL * oyn + oy) * Lcx + ox, m1);
      store_row8<O>((O*)outs.p[4] + (zL * oyn + oy) * oxn + ox, m4);
    }
    if (y0f) {
      store_row8<O>((O*)outs.p[2] + (zN * Lcy + oy) * Lcx + ox, m2);
      store_row8<O>((O*)outs.p[5] + (zN * Lcy + oy) * oxn + ox, m5);
      if (z0f) {
        store_row8<O>((O*)outs.p[0] + (zL * Lcy + oy) * oxn + ox, m0);
        store_row8<O>((O*)outs.p[3] + (zL * Lcy + oy) * Lcx + ox, m3);
      }
    }
  }
  // the last column, ox = Lcx: LR, Z, Y from the cells at x = Lcx - 1
  for (int32_t t = threadIdx.x; t < nz * oyn; t += kThreads) {
    int32_t pz, oy;
    divmod_small(t, oyn, roy, pz, oy);
    const int32_t oz = z0 + pz;
    const bool z0f = oz < Lcz, y0f = oy < Lcy;
    const uint32_t sz = (uint32_t)(z0f && oz >= 1), sy = (uint32_t)(y0f && oy >= 1);
    const uint32_t* cur = cl + (pz + 1) * PW + 3 + Lcx;  // x = Lcx - 1
    const uint32_t* prv = cl + pz * PW + 3 + Lcx;
    const uint32_t c001 = cur[(oy + 1) * RP], c011 = cur[oy * RP], c101 = prv[(oy + 1) * RP];
    const int32_t zL = b * Lcz + oz, zN = b * (Lcz + 1) + oz;
    if (z0f) ((O*)outs.p[4])[(zL * oyn + oy) * oxn + Lcx] = (O)((c001 + c011) >> sy);
    if (y0f) {
      ((O*)outs.p[5])[(zN * Lcy + oy) * oxn + Lcx] = (O)((c001 + c101) >> sz);
      if (z0f) ((O*)outs.p[0])[(zL * Lcy + oy) * oxn + Lcx] = (O)c001;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Mean predictor on a padded lowres window (tests/volume/test_encode_decode.py:46-53):
// cell mean = astype(T)(f32 sum of the (2p+2)^d neighbourhood / N), then the map aggregation.
// ------------------------------------------------------------------------------------------
template <typename T, typename I>
__device__ __forceinline__ T cell_mean_padded(const T* __restrict__ in, I b, I cz, I cy, I cx,
                                              I c, E3<I> S, I C, int nsp, int p) {
  const int k = 2 * p + 2;
  const int kz = nsp == 3 ? k : 1;
  float s = 0.0f;
  for (int dz = 0; dz < kz; ++dz)
    for (int dy = 0; dy < k; ++dy)
      for (int dx = 0; dx < k; ++dx)
        s += (float)in[(((b * S.e[0] + cz + dz) * S.e[1] + cy + dy) * S.e[2] + cx + dx) * C + c];
  return cast_f32<T>(s / (float)(kz * k * k));
}

// Two passes: (1) the per-cell means ARE the C map (volume/utils.py:117: channel 6 unscaled; 2D
// channel 4), so they are written there once; (2) every other map aggregates up to 4 of them
// (the f32 scatter-add / scale / truncate of volume/utils.py:83-155, kmp_aggregate.h).
template <typename T, typename I>
__global__ void __launch_bounds__(kThreads) cell_mean_map_kernel(const T* __restrict__ in, I B, E3<I> S,
                                                               I C, int nsp, int p, E3<I> cells,
                                                               T* __restrict__ out, I total) {
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < total; t += (I)gridDim.x * blockDim.x) {
    IdxT<I> q = unflat_t<I>(t, cells.e[0], cells.e[1], cells.e[2], C);
    out[t] = cell_mean_padded<T, I>(in, q.b, q.i0, q.i1, q.i2, q.c, S, C, nsp, p);
  }
}

// Host: a checked request, and the kernel families in the order they are tried.  A try_<family>
// either launches or answers KMP_ERR_UNSUPPORTED, having touched nothing.
struct MeanRequest {
  int nsp, dtype, padding;
  bool f32;  // float32 maps of integer samples (a network-shaped predictor's output; the same integers)
  const void* win;  // [B, S..., C] padded lowres
  int64_t B, C;
  hipStream_t stream;
  Ext3 S, cells;
  MapPtrs outs;
  int64_t total;  // output positions (frame = cells + 1 per spatial axis) x B x C
};

static inline Ext3 frame_of(const Ext3& cells) { return Ext3{{cells.e[0] + 1, cells.e[1] + 1, cells.e[2] + 1}}; }

// p = 0, Lcx % 8 == 0: eight x positions per lane (mean_predict_p0x8_kernel), ZP = 3 output
// planes per workgroup (4 cell planes); 32-bit map offsets
template <typename T>
static int try_p0x8(const MeanRequest& r) {
  const Ext3& c = r.cells;
  const int64_t zp8 = std::min<int64_t>(3, c.e[0] + 1), ngrp8 = ceil_div(c.e[0] + 1, zp8);
  const int64_t lds8 = 4 * (zp8 + 1) * mp8_plane_words((int32_t)std::min<int64_t>(c.e[1], 1 << 20),
                                                       (int32_t)std::min<int64_t>(c.e[2], 1 << 20));
  if (!(r.nsp == 3 && r.C == 1 && r.padding == 0 && c.e[2] % 8 == 0 && lds8 <= 64 * 1024 &&
        vol(r.B, frame_of(c), 1) < ((int64_t)1 << 31) && r.B * ngrp8 < ((int64_t)1 << 31) &&
        (zp8 + 1) * c.e[1] * (c.e[2] / 8) < ((int64_t)1 << 21)))
    return KMP_ERR_UNSUPPORTED;
  auto kern = r.f32 ? mean_predict_p0x8_kernel<T, float> : mean_predict_p0x8_kernel<T, T>;
  kern<<<(unsigned)(r.B * ngrp8), kThreads, (size_t)lds8, r.stream>>>(
      (const T*)r.win, e32(r.S), (int32_t)c.e[0], (int32_t)c.e[1], (int32_t)c.e[2], r.outs,
      r.B % 8 == 0 ? (int32_t)ngrp8 : 0, (int32_t)zp8, (int32_t)ngrp8);
  return check_launch("mean_predict_p0x8");
}

// mean_predict_plane_kernel<T, padding, ppb, O>; O = float writes float32 maps
template <typename T>
using PlaneKernel = void (*)(const T*, E3<int32_t>, int32_t, int32_t, int32_t, MapPtrs, int32_t, int32_t, int32_t);
template <typename T, typename O>
static PlaneKernel<T> plane_kernel(int padding, int ppb) {
  static const PlaneKernel<T> k[2][3] = {
      {mean_predict_plane_kernel<T, 0, 1, O>, mean_predict_plane_kernel<T, 1, 1, O>, mean_predict_plane_kernel<T, 2, 1, O>},
      {mean_predict_plane_kernel<T, 0, 2, O>, mean_predict_plane_kernel<T, 1, 2, O>, mean_predict_plane_kernel<T, 2, 2, O>}};
  return k[ppb - 1][padding];
}

// one workgroup per output plane when the plane's window planes fit LDS
template <typename T>
static int try_plane(const MeanRequest& r) {
  const Ext3 &S = r.S, &c = r.cells;
  const int padding = r.padding;
  const int64_t plane = S.e[1] * S.e[2];
  // PPB output planes per workgroup: 2 where its LDS fits (the cell plane between the two output
  // planes summed once: p = 0 101 -> 94 us, p = 1 300 -> 270 us at 512 C3 windows,
  // profiles/round2/ab_mean_predict_ppb.log), else 1 (e.g. the C3 window at p = 2)
  auto lds_for = [&](int q, int64_t& nb_, int64_t& xs_) {
    nb_ = 16 * (ceil_div((2 * padding + 2 + q) * plane * (int64_t)sizeof(T), 16) + 1);
    xs_ = padding > 0 ? 4 * (2 * padding + 2 + q) * S.e[1] * c.e[2] : 0;
    return nb_ + xs_ + 4 * (q + 1) * c.e[1] * c.e[2] + 8 * mp_pad_words(c.e[2]);
  };
  int64_t nodes_bytes = 0, xs_bytes = 0;
  int ppb = 2;
  int64_t lds_plane = lds_for(ppb, nodes_bytes, xs_bytes);
  if (lds_plane > 64 * 1024) {
    ppb = 1;
    lds_plane = lds_for(ppb, nodes_bytes, xs_bytes);
  }
  const int64_t ngrp = ceil_div(c.e[0] + 1, (int64_t)ppb);
  const int64_t nblk_plane = r.B * ngrp;
  if (!(r.nsp == 3 && r.C == 1 && padding <= 2 && lds_plane <= 64 * 1024 && nblk_plane < ((int64_t)1 << 31) &&
        vol(1, frame_of(c), 1) < ((int64_t)1 << 31)))
    return KMP_ERR_UNSUPPORTED;
  auto kern = r.f32 ? plane_kernel<T, float>(padding, ppb) : plane_kernel<T, T>(padding, ppb);
  kern<<<(unsigned)nblk_plane, kThreads, (size_t)lds_plane, r.stream>>>(
      (const T*)r.win, e32(S), (int32_t)c.e[0], (int32_t)c.e[1], (int32_t)c.e[2], r.outs,
      r.B % 8 == 0 ? (int32_t)ngrp : 0, (int32_t)nodes_bytes, (int32_t)xs_bytes);
  return check_launch(ppb == 2 ? "mean_predict_plane2" : "mean_predict_plane");
}

// the z-rolling rows kernel (mean_predict_lds_kernel): C == 1 windows of either dimension, p <= 1
template <typename T>
static int try_rows(const MeanRequest& r) {
  if (!(rows_ok(r.C, {vol(r.B, r.S, r.C), r.total}) && r.padding <= 1)) return KMP_ERR_UNSUPPORTED;
  const ZRollPlan z = plan_zroll(r.B, frame_of(r.cells), r.nsp);
  const int32_t RP = z.XO + 1;
  const size_t lds = (size_t)2 * (z.YB + 1) * RP * sizeof(uint32_t);
  if ((int64_t)(z.YB + 1) * RP > kThreads * kMpCpt) return fail(KMP_ERR_ARG, "mean_predict_maps: tile");
  auto kern = r.nsp == 3 ? mean_predict_lds_kernel<T, 3> : mean_predict_lds_kernel<T, 2>;
  kern<<<(unsigned)z.nblk, kThreads, lds, r.stream>>>((const T*)r.win, e32(r.S), r.padding, (int32_t)r.cells.e[0],
                                                      (int32_t)r.cells.e[1], (int32_t)r.cells.e[2], r.outs, z.YB, z.XO,
                                                      z.ZC, z.nzc, z.nyb, z.nxb, RP);
  return check_launch("mean_predict_maps");
}

// the element pair: the cell means into the centre map, then every other map from them
template <typename T>
static int element_pair(const MeanRequest& r) {
  T* cm = (T*)r.outs.p[center_map(r.nsp)];
  const bool small = fits32({vol(r.B, r.S, r.C), r.total});
  const int64_t ncell = vol(r.B, r.cells, r.C);
  int st = with_index(small, [&](auto itag) {
    using I = decltype(itag);
    cell_mean_map_kernel<T, I><<<grid_for(ncell), kThreads, 0, r.stream>>>(
        (const T*)r.win, (I)r.B, e3<I>(r.S), (I)r.C, r.nsp, r.padding, e3<I>(r.cells), cm, (I)ncell);
    return check_launch("mean_predict_maps");
  });
  if (st) return st;
  return launch_maps_from_cell_means(r.nsp, r.dtype, cm, r.B, r.cells, r.C, r.outs, r.total, small, r.stream);
}

// out_dtype: the maps' dtype -- the sample dtype, or KMP_F32 (a network-shaped predictor's
// float32 output; the values are the same integers) on the 3D C == 1 LDS kernels.
static int mean_predict_maps_impl(int32_t nsp, int32_t dtype, int32_t out_dtype, const void* padded_lowres, int64_t B,
                                  const int64_t shape[3], int64_t C, int32_t padding, void* const out[7],
                                  kmp_stream_t stream) {
  if (int s = check_common(nsp, B, shape, C)) return s;
  KMP_REQUIRE(out_dtype == dtype || out_dtype == KMP_F32, "map dtype must be the sample dtype or float32");
  KMP_REQUIRE(padded_lowres && out && padding >= 0, "null pointer or negative padding");
  MeanRequest r{nsp, dtype, padding, out_dtype != dtype, padded_lowres, B, C, (hipStream_t)stream, ext_from(nsp, shape)};
  KMP_REQUIRE(bind_maps(nsp, out, r.outs), "null map pointer");
  r.total = B * C;
  for (int a = 0; a < 3; ++a) {
    if (a < 3 - nsp) { r.cells.e[a] = 1; continue; }
    KMP_REQUIRE(r.S.e[a] - 2 * padding - 1 >= 1, "window has no cells");
    r.cells.e[a] = r.S.e[a] - 2 * padding - 1;
    r.total *= r.S.e[a] - 2 * padding;
  }
  if (r.total == 0) return KMP_OK;
  // (signed samples, Signed in kmp_common.h, take the element pair: the LDS kernels read packed words)
  return dispatch_sample_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if constexpr (std::is_same<T, uint8_t>::value || std::is_same<T, uint16_t>::value) {
      for (auto family : {try_p0x8<T>, try_plane<T>})
        if (int s = family(r); s != KMP_ERR_UNSUPPORTED) return s;
      if (r.f32) return fail(KMP_ERR_UNSUPPORTED, "mean_predict_maps: float32 maps need the 3D C == 1 LDS kernels");
      if (int s = try_rows<T>(r); s != KMP_ERR_UNSUPPORTED) return s;
    }
    if (r.f32) return fail(KMP_ERR_UNSUPPORTED, "mean_predict_maps: float32 maps of this window");
    return element_pair<T>(r);
  });
}

}  // namespace kmp

using namespace kmp;

extern "C" {

int kmp_mean_predict_maps(int32_t nsp, int32_t dtype, const void* padded_lowres, int64_t B, const int64_t shape[3],
                          int64_t C, int32_t padding, void* const out[7], kmp_stream_t stream) {
  return mean_predict_maps_impl(nsp, dtype, dtype, padded_lowres, B, shape, C, padding, out, stream);
}

int kmp_mean_predict_maps_typed(int32_t nsp, int32_t dtype, int32_t out_dtype, const void* padded_lowres, int64_t B,
                                const int64_t shape[3], int64_t C, int32_t padding, void* const out[7],
                                kmp_stream_t stream) {
  return mean_predict_maps_impl(nsp, dtype, out_dtype, padded_lowres, B, shape, C, padding, out, stream);
}

}  // extern "C"

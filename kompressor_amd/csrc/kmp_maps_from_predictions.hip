// kmp_maps_from_predictions.hip -- the reference's aggregation of per-cell predictions into the 7 (3)
// maps (volume/utils.py:83-155, kmp_aggregate.h): kmp_maps_from_predictions, and the same aggregation
// of bare cell means for the mean predictor's two-pass fallback (kmp_mean_predict.hip).
#include "kmp_primitives.h"

namespace kmp {

// Per-element aggregation, one thread per frame position.  The source is fixed at compile time:
//   MEANS = false  [B, cells..., K, C] predictions, every map written;
//   MEANS = true   [B, cells..., C] cell means: every channel of a cell reads its mean, and the centre
//                  map is skipped (the means ARE that map, written by the pass before).
// u8 / u16, C == 1, 32-bit indices: the f32 sum of at most 4 integer predictions is exact, so the
// reference's scale-and-truncate is an integer shift (the values of aggregate_map).
template <typename T, int NSP, bool MEANS>
__global__ void __launch_bounds__(kThreads) aggregate_maps_int_kernel(const T* __restrict__ src, int32_t Lcz,
                                                                    int32_t Lcy, int32_t Lcx, MapPtrs outs,
                                                                    int32_t total) {
  constexpr int NM = NSP == 3 ? 7 : 3, K = NSP == 3 ? 19 : 5;
  const int32_t f0 = NSP == 3 ? Lcz + 1 : 1, f1 = Lcy + 1, f2 = Lcx + 1, cz = NSP == 3 ? Lcz : 1;
  for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    uint32_t q = (uint32_t)t;
    const int32_t ox = q % (uint32_t)f2; q /= (uint32_t)f2;
    const int32_t oy = q % (uint32_t)f1; q /= (uint32_t)f1;
    const int32_t oz = q % (uint32_t)f0;
    const int32_t b = q / (uint32_t)f0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      if (MEANS && k == center_map(NSP)) continue;
      int par[3];
      map_parity(NSP, k, par);
      const int32_t e0 = NSP == 3 ? (par[0] ? Lcz : Lcz + 1) : 1, e1 = par[1] ? Lcy : Lcy + 1, e2 = par[2] ? Lcx : Lcx + 1;
      if (oz >= e0 || oy >= e1 || ox >= e2) continue;
      Contrib c[4];
      const int nc = map_contribs(NSP, k, c);
      uint32_t s = 0, cnt = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i >= nc) break;
        const int32_t z = oz - c[i].dz, y = oy - c[i].dy, x = ox - c[i].dx;
        if (z >= 0 && z < cz && y >= 0 && y < Lcy && x >= 0 && x < Lcx) {
          if constexpr (MEANS) s += src[((b * cz + z) * Lcy + y) * Lcx + x];
          else s += src[(((b * cz + z) * Lcy + y) * Lcx + x) * K + c[i].ch];
          ++cnt;
        }
      }
      ((T*)outs.p[k])[((b * e0 + oz) * e1 + oy) * e2 + ox] = (T)(!MEANS && k == center_map(NSP) ? s : s >> (cnt >> 1));
    }
  }
}

// The general form: the reference's float32 aggregation (aggregate_map), any dtype, C and index width.
template <typename T, typename I, bool MEANS>
__global__ void __launch_bounds__(kThreads) aggregate_maps_kernel(const T* __restrict__ src, I B, E3<I> cells, I C,
                                                                int nsp, MapPtrs outs, I total) {
  const int nmaps = nsp == 3 ? 7 : 3;
  const int K = nsp == 3 ? 19 : 5;
  // frame = cells + 1 per spatial axis
  const I f0 = nsp == 3 ? cells.e[0] + 1 : 1, f1 = cells.e[1] + 1, f2 = cells.e[2] + 1;
  const I Lcz = cells.e[0], Lcy = cells.e[1], Lcx = cells.e[2];
  for (I t = blockIdx.x * (I)blockDim.x + threadIdx.x; t < total; t += (I)gridDim.x * blockDim.x) {
    IdxT<I> q = unflat_t<I>(t, f0, f1, f2, C);
    auto get = [&](int64_t z64, int64_t y64, int64_t x64, int ch) -> T {
      const I cell = ((q.b * Lcz + (I)z64) * Lcy + (I)y64) * Lcx + (I)x64;
      return src[(MEANS ? cell : cell * K + ch) * C + q.c];
    };
    for (int k = 0; k < nmaps; ++k) {
      if (MEANS && k == center_map(nsp)) continue;
      int par[3];
      map_parity(nsp, k, par);
      I e[3];
      const I idx[3] = {q.i0, q.i1, q.i2};
      bool ok = true;
      for (int a = 0; a < 3; ++a) {
        e[a] = (a < 3 - nsp) ? 1 : (par[a] ? cells.e[a] : cells.e[a] + 1);
        ok = ok && idx[a] < e[a];
      }
      if (!ok) continue;
      T* o = (T*)outs.p[k];
      o[(((q.b * e[0] + q.i0) * e[1] + q.i1) * e[2] + q.i2) * C + q.c] =
          aggregate_map<T>(nsp, k, (int64_t)q.i0, (int64_t)q.i1, (int64_t)q.i2, (int64_t)Lcz, (int64_t)Lcy, (int64_t)Lcx, get);
    }
  }
}

// LDS-staged form (C == 1, < 2^30 elements).  A workgroup owns YB frame rows x XO frame columns
// of ZC consecutive output planes, for all maps, and rolls along z: cell plane z (rows y0-1 ..
// y0+YB-1, cells ox0-1 .. ox0+XO-1: YB+1 contiguous runs of cells x K channels in HBM) is staged
// into an LDS ring of two planes with 16-byte loads (row pitch rounded to 16 B, so every LDS
// store is aligned), and plane z+1 is fetched into registers while plane z's outputs aggregate
// from LDS.  HBM reads are (YB+1)/YB x (ZC+1)/ZC of the predictions; the per-element kernel
// above reads the channel-interleaved cells with a 19-element lane stride instead (~19 cache
// lines per load instruction).  Arithmetic is the same: integer shifts for u8 / u16, the
// reference's f32 channel-order sum + scale + truncation otherwise.
constexpr int kMfpCpt = 8;  // 16-byte chunks per thread per staged plane (host-checked)

template <typename T, int NSP>
__global__ void __launch_bounds__(kThreads) maps_from_predictions_lds_kernel(
    const T* __restrict__ preds, int32_t Lcz, int32_t Lcy, int32_t Lcx, MapPtrs outs, int32_t YB, int32_t XO,
    int32_t ZC, int32_t nzc, int32_t nyb, int32_t nxb, int32_t RP, int32_t nchunk, float rcp_nchunk,
    int64_t total_elems) {
  constexpr int NM = NSP == 3 ? 7 : 3, K = NSP == 3 ? 19 : 5;
  constexpr int V = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* lds = (T*)smem;
  int32_t w = (int32_t)blockIdx.x;
  const int32_t xb = w % nxb; w /= nxb;
  const int32_t yb = w % nyb; w /= nyb;
  const int32_t zc = w % nzc;
  const int32_t b = w / nzc;
  const int32_t y0 = yb * YB, ox0 = xb * XO;
  const int32_t xc0 = ox0 > 0 ? ox0 - 1 : 0;
  const int32_t xc1 = (ox0 + XO - 1 < Lcx - 1) ? ox0 + XO - 1 : Lcx - 1;  // last staged cell
  const int32_t nxc_k = (xc1 - xc0 + 1) * K;                                // staged elements per row
  const int32_t cz = NSP == 3 ? Lcz : 1;
  const int32_t fz = NSP == 3 ? Lcz + 1 : 1;
  const int32_t oz0 = zc * ZC, oz1 = (oz0 + ZC < fz) ? oz0 + ZC : fz;  // output planes [oz0, oz1)
  const int32_t slice_work = (YB + 1) * nchunk;

  u32x4v buf[kMfpCpt];
  auto fetch = [&](int32_t z) {  // cell plane z -> registers
#pragma unroll
    for (int c = 0; c < kMfpCpt; ++c) {
      buf[c] = u32x4v{0u, 0u, 0u, 0u};
      const int32_t i = threadIdx.x + c * kThreads;
      if (i >= slice_work) continue;
      int32_t r, ch;
      divmod_small(i, nchunk, rcp_nchunk, r, ch);
      const int32_t y = y0 - 1 + r;
      if (y < 0 || y >= Lcy || ch * V >= nxc_k) continue;
      const int64_t g = ((((int64_t)b * cz + z) * Lcy + y) * Lcx + xc0) * K + (int64_t)ch * V;
      if (g + V <= total_elems) {
        buf[c] = *(const u32x4u*)(preds + g);
      } else {
        T* bt = (T*)&buf[c];
        for (int e = 0; e < V && g + e < total_elems; ++e) bt[e] = preds[g + e];
      }
    }
  };
  auto put = [&](int32_t z) {  // registers -> ring slot z & 1
    T* base = lds + (z & 1) * (YB + 1) * RP;
#pragma unroll
    for (int c = 0; c < kMfpCpt; ++c) {
      const int32_t i = threadIdx.x + c * kThreads;
      if (i >= slice_work) continue;
      int32_t r, ch;
      divmod_small(i, nchunk, rcp_nchunk, r, ch);
      *(u32x4v*)(base + r * RP + ch * V) = buf[c];
    }
  };
  auto at = [&](int32_t z, int32_t r, int32_t x, int ch) -> T {  // cell (z, y0-1+r, x), channel ch
    return lds[((z & 1) * (YB + 1) + r) * RP + (x - xc0) * K + ch];
  };

  // prologue: cell plane oz0 - 1 (3D, when it exists) and oz0
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
    if (more) fetch(oz + 1);  // in flight while plane oz aggregates
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
        Contrib c[4];
        const int nc = map_contribs(NSP, k, c);
        T v;
        if constexpr (sizeof(T) <= 2 && !std::is_same<T, float>::value) {
          uint32_t sum = 0, cnt = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j >= nc) break;
            const int32_t z = oz - c[j].dz, y = oy - c[j].dy, x = ox - c[j].dx;
            if (z >= 0 && z < cz && y >= 0 && y < Lcy && x >= 0 && x < Lcx) {
              sum += at(z, r + 1 - c[j].dy, x, c[j].ch);
              ++cnt;
            }
          }
          v = (T)(k == center_map(NSP) ? sum : sum >> (cnt >> 1));
        } else if (k == center_map(NSP)) {
          v = at(oz, r + 1, ox, c[0].ch);
        } else {
          float sum = 0.0f;
          int cnt = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j >= nc) break;
            const int32_t z = oz - c[j].dz, y = oy - c[j].dy, x = ox - c[j].dx;
            if (z >= 0 && z < cz && y >= 0 && y < Lcy && x >= 0 && x < Lcx) {
              sum += (float)at(z, r + 1 - c[j].dy, x, c[j].ch);
              ++cnt;
            }
          }
          if (cnt == 4) sum *= 0.25f;
          else if (cnt == 2) sum *= 0.5f;
          v = cast_f32<T>(sum);
        }
        ((T*)outs.p[k])[((b * e0 + oz) * e1 + oy) * e2 + ox] = v;
      }
    }
    if (!more) break;  // uniform
    __syncthreads();  // plane oz - 1's slot is free
    put(oz + 1);
    __syncthreads();
  }
}

// The element form of either source; ``name`` is the launch's name.
template <typename T, bool MEANS>
static int aggregate_elements(const char* name, int nsp, const T* src, int64_t B, const Ext3& cells, int64_t C,
                              const MapPtrs& outs, int64_t total, bool small, bool shifts, hipStream_t stream) {
  if constexpr (is_small_sample<T>) {
    if (shifts) {
      auto kern = nsp == 3 ? aggregate_maps_int_kernel<T, 3, MEANS> : aggregate_maps_int_kernel<T, 2, MEANS>;
      kern<<<grid_for(total), kThreads, 0, stream>>>(src, (int32_t)cells.e[0], (int32_t)cells.e[1], (int32_t)cells.e[2],
                                                     outs, (int32_t)total);
      return check_launch(name);
    }
  }
  return with_index(small, [&](auto itag) {
    using I = decltype(itag);
    aggregate_maps_kernel<T, I, MEANS><<<grid_for(total), kThreads, 0, stream>>>(src, (I)B, e3<I>(cells), (I)C, nsp,
                                                                                 outs, (I)total);
    return check_launch(name);
  });
}

int launch_maps_from_cell_means(int nsp, int dtype, const void* cm, int64_t B, const Ext3& cells, int64_t C,
                                const MapPtrs& outs, int64_t total, bool small, hipStream_t stream) {
  return dispatch_sample_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return aggregate_elements<T, true>("mean_predict_maps", nsp, (const T*)cm, B, cells, C, outs, total, small,
                                       C == 1 && total < ((int64_t)1 << 31), stream);
  });
}

}  // namespace kmp

using namespace kmp;

extern "C" {

int kmp_maps_from_predictions(int32_t nsp, int32_t dtype, const void* preds, int64_t B, const int64_t cells[3],
                              int64_t C, void* const out[7], kmp_stream_t stream) {
  if (int s = check_common(nsp, B, cells, C)) return s;
  KMP_REQUIRE(preds && out, "null pointer");
  Ext3 ce = ext_from(nsp, cells);
  MapPtrs outs{};
  KMP_REQUIRE(bind_maps(nsp, out, outs), "null map pointer");
  int64_t total = B * C;
  for (int a = 3 - nsp; a < 3; ++a) total *= ce.e[a] + 1;
  if (total == 0) return KMP_OK;
  return dispatch_any_sample_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const int K = nsp == 3 ? 19 : 5;
    const bool small = fits32({vol(B, ce, C) * K, total});
    if (rows_ok(C, {vol(B, ce, C) * K, total})) {
      constexpr int V = 16 / (int)sizeof(T);
      const ZRollPlan z = plan_zroll(B, Ext3{{ce.e[0] + 1, ce.e[1] + 1, ce.e[2] + 1}}, nsp);
      const int32_t nchunk = (int32_t)ceil_div((int64_t)(z.XO + 1) * K, V);
      const int32_t RP = nchunk * V;
      const size_t lds = (size_t)(nsp == 3 ? 2 : 1) * (z.YB + 1) * RP * sizeof(T);
      if ((int64_t)(z.YB + 1) * nchunk > kThreads * kMfpCpt) return fail(KMP_ERR_ARG, "maps_from_predictions: tile");
      auto kern = nsp == 3 ? maps_from_predictions_lds_kernel<T, 3> : maps_from_predictions_lds_kernel<T, 2>;
      kern<<<(unsigned)z.nblk, kThreads, lds, (hipStream_t)stream>>>(
          (const T*)preds, (int32_t)ce.e[0], (int32_t)ce.e[1], (int32_t)ce.e[2], outs, z.YB, z.XO, z.ZC, z.nzc, z.nyb,
          z.nxb, RP, nchunk, 1.0f / (float)nchunk, vol(B, ce, C) * K);
      return check_launch("maps_from_predictions");
    }
    return aggregate_elements<T, false>("maps_from_predictions", nsp, (const T*)preds, B, ce, C, outs, total, small,
                                        small && C == 1, (hipStream_t)stream);
  });
}

}  // extern "C"

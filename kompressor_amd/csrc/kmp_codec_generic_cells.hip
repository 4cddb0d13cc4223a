// kmp_codec_generic_cells.hip -- pass 1 of the generic two-pass codec (kmp_codec_generic.hip): the
// MeanPredictor's value of every cell into the workspace, and the workspace's size.  (The
// LinearPredictor's cells are kmp_linear.hip's.)
#include "kmp_generic.h"

namespace kmp {

// Cell mean, float32 sum in feature order (z-major, y, x) / N, XLA cast (the reference test
// predictor).  Exact (order-independent) for uint8 with p <= 4 and uint16 with p <= 2.
// ``cf`` is the box of cells to compute (a region launch needs cells [begin-1, end) only);
// results land at their global position in ``cells`` [B, Lc..., C].  KK = 2p + 2 at compile time
// (p <= 2: the node offsets per axis in registers, the (2p+2)^d loads unrolled) or 0 (any p).
template <typename T, int NSP, int KK, typename I>
__global__ void __launch_bounds__(kThreads) cell_mean_kernel(const T* __restrict__ src, Src s, Geo g, int64_t B,
                                                            int64_t C, int p, Frame cf, Flat F, T* __restrict__ cells,
                                                            int64_t total) {
  const int k = KK ? KK : 2 * p + 2;
  const int kz = NSP == 3 ? k : 1;
  const int pz = NSP == 3 ? p : 0;
  const float inv_n = (float)(kz * k * k);
  const I Cc = (I)C, sy = (I)s.S[2] * Cc, sz = (I)s.S[1] * sy, sb = (I)s.S[0] * sz;
  const I cy = (I)g.Lc[2] * Cc, cz = (I)g.Lc[1] * cy, cb = (I)g.Lc[0] * cz;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    I b, z, y, x, c;
    unflat_i<I>(t, F, cf.ext, C, b, z, y, x, c);
    z += (I)cf.begin[0];
    y += (I)cf.begin[1];
    x += (I)cf.begin[2];
    const I base = b * sb + c;
    float sum = 0.0f;
    if constexpr (KK > 0) {
      I ox[KK], oy[KK];
#pragma unroll
      for (int d = 0; d < KK; ++d) {
        ox[d] = (I)node_src(x - p + d, g.L[2], g.E[2], s.mult) * Cc;
        oy[d] = (I)node_src(y - p + d, g.L[1], g.E[1], s.mult) * sy;
      }
#pragma unroll
      for (int dz = 0; dz < (NSP == 3 ? KK : 1); ++dz) {
        const I zo = base + (NSP == 3 ? (I)node_src(z - pz + dz, g.L[0], g.E[0], s.mult) * sz : 0);
#pragma unroll
        for (int dy = 0; dy < KK; ++dy)
#pragma unroll
          for (int dx = 0; dx < KK; ++dx) sum += (float)src[zo + oy[dy] + ox[dx]];
      }
    } else {
      for (int dz = 0; dz < kz; ++dz) {
        const I zo = base + (NSP == 3 ? (I)node_src(z - pz + dz, g.L[0], g.E[0], s.mult) * sz : 0);
        for (int dy = 0; dy < k; ++dy) {
          const I yo = zo + (I)node_src(y - p + dy, g.L[1], g.E[1], s.mult) * sy;
          for (int dx = 0; dx < k; ++dx) sum += (float)src[yo + (I)node_src(x - p + dx, g.L[2], g.E[2], s.mult) * Cc];
        }
      }
    }
    cells[b * cb + z * cz + y * cy + x * Cc + c] = gcast<T>(sum / inv_n);
  }
}

// The cell mean, R = 4 consecutive cells of a row per thread: each (dz, dy) row of R + KK - 1 nodes
// is read once for the 4 cells (28 loads for 4 cells at p = 1 instead of 4 x 64).  EXACT (8- /
// 16-bit samples with N x max sample < 2^24: u8 at p <= 4, u16 at p <= 2): the reference's
// in-order float sum is the integer sum, formed by sliding windows; otherwise each cell's float
// sum is accumulated in the reference's feature order (z-major, y, x), exactly cell_mean_kernel's.
constexpr int kMeanR = 4;

template <typename T, int NSP, int KK, bool EXACT>
__global__ void __launch_bounds__(kThreads) cell_mean_row_kernel(const T* __restrict__ src, Src s, Geo g, int64_t C,
                                                                int p, Frame cf, Flat F, T* __restrict__ cells,
                                                                int64_t total) {
  constexpr int R = kMeanR, NX = R + KK - 1;
  using I = int32_t;
  const float n_f = (float)((NSP == 3 ? KK : 1) * KK * KK);
  const I Cc = (I)C, sy = (I)s.S[2] * Cc, sz = (I)s.S[1] * sy, sb = (I)s.S[0] * sz;
  const I cy = (I)g.Lc[2] * Cc, cz = (I)g.Lc[1] * cy, cb = (I)g.Lc[0] * cz;
  const int pz = NSP == 3 ? p : 0;
  const I xend = (I)(cf.begin[2] + cf.ext[2]);
  const int64_t jmax = xend - 1 - p + (KK - 1);  // the last node a valid cell reads
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ext_q[3] = {cf.ext[0], cf.ext[1], (cf.ext[2] + R - 1) / R};
    I b, z, y, xq, c;
    unflat_i<I>(t, F, ext_q, C, b, z, y, xq, c);
    z += (I)cf.begin[0];
    y += (I)cf.begin[1];
    const I x0 = (I)cf.begin[2] + R * xq;
    const I base = b * sb + c;
    I ox[NX], oy[KK], oz[NSP == 3 ? KK : 1];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      int64_t j = (int64_t)x0 - p + i;
      j = j > jmax ? jmax : j;
      ox[i] = (I)node_src(j, g.L[2], g.E[2], s.mult) * Cc;
    }
#pragma unroll
    for (int d = 0; d < KK; ++d) {
      oy[d] = (I)node_src(y - p + d, g.L[1], g.E[1], s.mult) * sy;
      if constexpr (NSP == 3) oz[d] = (I)node_src(z - pz + d, g.L[0], g.E[0], s.mult) * sz;
    }
    uint32_t sum[R];
    float fsum[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      sum[r] = 0u;
      fsum[r] = 0.0f;
    }
    constexpr int ZU = NSP == 3 && KK <= 4 ? KK : 1;  // 3D p = 2: a runtime z loop (all 324 loads
                                                    // hoisted took 267 VGPRs)
#pragma unroll ZU
    for (int dz = 0; dz < (NSP == 3 ? KK : 1); ++dz) {
      I zo = NSP == 3 ? oz[0] : 0;
#pragma unroll
      for (int d = 1; d < (NSP == 3 ? KK : 1); ++d) zo = dz == d ? oz[d] : zo;
#pragma unroll
      for (int dy = 0; dy < KK; ++dy) {
        const I rb = base + zo + oy[dy];
        if constexpr (EXACT) {
          uint32_t v[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) v[i] = (uint32_t)src[rb + ox[i]];
          uint32_t w = 0u;
#pragma unroll
          for (int i = 0; i < KK; ++i) w += v[i];
          sum[0] += w;
#pragma unroll
          for (int r = 1; r < R; ++r) {
            w += v[r + KK - 1] - v[r - 1];
            sum[r] += w;
          }
        } else {
          float v[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) v[i] = (float)src[rb + ox[i]];
#pragma unroll
          for (int dx = 0; dx < KK; ++dx)
#pragma unroll
            for (int r = 0; r < R; ++r) fsum[r] += v[r + dx];
        }
      }
    }
    const I ob = b * cb + z * cz + y * cy + x0 * Cc + c;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (x0 + r < xend) cells[ob + r * Cc] = gcast<T>((EXACT ? (float)sum[r] : fsum[r]) / n_f);
  }
}

int64_t generic_workspace_bytes(int dtype, int nsp, const Geo& g, int64_t B, int64_t C, const kmp_predictor* pred) {
  const bool lin = pred && (pred->kind == KMP_PRED_LINEAR || pred->kind == KMP_PRED_LINEAR_MFMA);
  const int K = lin ? (nsp == 3 ? 19 : 5) : 1;
  int64_t need = B * g.Lc[0] * g.Lc[1] * g.Lc[2] * K * C * dtype_size(dtype);
  if (lin && B > 0) {  // the fused LinearPredictor kernels keep a reordered copy of W [N, K] there
    const int64_t nb = 2 * pred->padding + 2, N = nsp == 3 ? nb * nb * nb : nb * nb;
    int64_t wbytes = N * K * (int64_t)sizeof(float);
    // the matrix-core kernels' B fragments (3 column tiles x 8 chunks x 64 lanes x 16 B) + biases
    // + linear3pm's dummy store slots (64 lanes x 16 B)
    constexpr int64_t kMfmaWs = 3 * 8 * 64 * 16 + 3 * 64 * 4 + 64 * 16;
    if (pred->kind == KMP_PRED_LINEAR_MFMA) wbytes = wbytes > kMfmaWs ? wbytes : kMfmaWs;
    need = need > wbytes ? need : wbytes;
  }
  return need;
}

template <typename T>
int run_predictor(const T* src, const Src& s, const Geo& g, int nsp, int64_t B, int64_t C, const kmp_predictor* pred,
                  const Frame& f, T* cells, hipStream_t stream) {
  const Frame cf = cell_frame(g, f);
  const int64_t ncell = B * cf.ext[0] * cf.ext[1] * cf.ext[2] * C;
  if (ncell == 0) return KMP_OK;
  if (pred->kind == KMP_PRED_MEAN) {
    const bool i32 = fits32(g, B, C, 1);
    const int p = pred->padding, kk = 2 * p + 2;
    const int64_t nn = (nsp == 3 ? kk : 1) * (int64_t)kk * kk;
    // (signed samples are summed as M(x), Signed in kmp_common.h: the unsigned type's range)
    using TM = typename sample_traits<T>::mapped;
    const int64_t top = std::is_same<TM, uint8_t>::value ? 255 : (std::is_same<TM, uint16_t>::value ? 65535 : -1);
    if (i32 && p <= 3) {  // cell_mean_row_kernel: exact integer sums when they are, else in-order floats
      const bool exact = top > 0 && nn * top < ((int64_t)1 << 24);
      const int64_t ext_q[3] = {cf.ext[0], cf.ext[1], ceil_div(cf.ext[2], (int64_t)kMeanR)};
      const Flat Fq = make_flat(ext_q, C);
      const int64_t nq = B * ext_q[0] * ext_q[1] * ext_q[2] * C;
      auto go = [&](auto nsp_c, auto kk_c) {
        constexpr int NSP = decltype(nsp_c)::value, KK = decltype(kk_c)::value;
        if (exact) cell_mean_row_kernel<T, NSP, KK, true><<<grid_for(nq), kThreads, 0, stream>>>(src, s, g, C, p, cf, Fq, cells, nq);
        else cell_mean_row_kernel<T, NSP, KK, false><<<grid_for(nq), kThreads, 0, stream>>>(src, s, g, C, p, cf, Fq, cells, nq);
      };
      auto with_kk = [&](auto nsp_c) {
        if (p == 0) go(nsp_c, std::integral_constant<int, 2>{});
        else if (p == 1) go(nsp_c, std::integral_constant<int, 4>{});
        else if (p == 2) go(nsp_c, std::integral_constant<int, 6>{});
        else go(nsp_c, std::integral_constant<int, 8>{});
      };
      if (nsp == 3) with_kk(std::integral_constant<int, 3>{});
      else with_kk(std::integral_constant<int, 2>{});
      return check_launch("cell_mean");
    }
    const Flat F = make_flat(cf.ext, C);
    auto go = [&](auto nsp_c, auto i_tag) {
      constexpr int NSP = decltype(nsp_c)::value;
      using I = decltype(i_tag);
#define KMP_CM(KK) cell_mean_kernel<T, NSP, KK, I><<<grid_for(ncell), kThreads, 0, stream>>>(src, s, g, B, C, p, cf, F, cells, ncell)
      if (p == 0) KMP_CM(2);
      else if (p == 1) KMP_CM(4);
      else if (p == 2) KMP_CM(6);
      else KMP_CM(0);
#undef KMP_CM
    };
    if (nsp == 3) {
      if (i32) go(std::integral_constant<int, 3>{}, int32_t{});
      else go(std::integral_constant<int, 3>{}, int64_t{});
    } else {
      if (i32) go(std::integral_constant<int, 2>{}, int32_t{});
      else go(std::integral_constant<int, 2>{}, int64_t{});
    }
    return check_launch("cell_mean");
  }
  const int64_t cbeg[3] = {cf.begin[0], cf.begin[1], cf.begin[2]}, cext[3] = {cf.ext[0], cf.ext[1], cf.ext[2]};
  return linear_cells<T>(src, s.S, s.mult, g, nsp, B, C, pred, cbeg, cext, cells, stream);
}

#define KMP_INST_PREDICTOR(T)                                                                                  \
  template int run_predictor<T>(const T*, const Src&, const Geo&, int, int64_t, int64_t, const kmp_predictor*, \
                                const Frame&, T*, hipStream_t);
KMP_FOR_SAMPLE_TYPES(KMP_INST_PREDICTOR)

}  // namespace kmp

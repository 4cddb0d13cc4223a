// kmp_codec_generic_row4.hip -- pass 2 of the generic two-pass codec (kmp_codec_generic.hip) for up
// to 4 interleaved channels: a thread owns 4 consecutive output columns of a row.
#ifndef KMP_PASS_KERNEL  // (this file includes its own kernel section, below)
#include "kmp_generic.h"

namespace kmp {

// The per-element kernel (kmp_codec_generic.hip) moves 2-byte values (u16) one per thread; with
// C == 1 (the common case outside the one-pass kernels: odd or wide rows, p >= 3) a thread here
// reads the 8 highres samples of each of its 2^d rows as one unaligned vector access (element-wise
// only in a row's last partial group), the cells around its outputs once, and writes each map's 4
// values together.
typedef uint32_t g32x2a1 __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t g32x4a1 __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t g32a1 __attribute__((aligned(1)));
typedef uint8_t g8x4 __attribute__((ext_vector_type(4)));
typedef uint8_t g8x4a1 __attribute__((ext_vector_type(4), aligned(1)));

// N consecutive samples (N x sizeof(T) a multiple of 4 bytes) as unaligned dword vector accesses.
// The values are the samples as numbers: M(x) for signed T (Signed, kmp_common.h), which these
// word-level accesses apply themselves (wv::smap: one xor per dword, nothing for any other type).
template <typename T, int N>
__device__ __forceinline__ void g_loadn(const T* p, uint32_t (&v)[N]) {
  constexpr int NW = N * (int)sizeof(T) / 4;
  static_assert(N * sizeof(T) % 4 == 0, "g_loadn: whole dwords");
  uint32_t w[NW];
  const char* c = (const char*)p;
  constexpr int N4 = NW / 4 * 4;  // dwordx4 pieces, then one x2 and / or one x1
#pragma unroll
  for (int i = 0; i < N4; i += 4) {
    const g32x4a1 t = *(const g32x4a1*)(c + 4 * i);
    w[i] = t[0]; w[i + 1] = t[1]; w[i + 2] = t[2]; w[i + 3] = t[3];
  }
  if constexpr (NW - N4 >= 2) {
    const g32x2a1 t = *(const g32x2a1*)(c + 4 * N4);
    w[N4] = t[0]; w[N4 + 1] = t[1];
  }
  if constexpr ((NW - N4) % 2) w[NW - 1] = *(const g32a1*)(c + 4 * (NW - 1));
  constexpr int PER = 4 / (int)(sizeof(T) < 4 ? sizeof(T) : 4);
  constexpr uint32_t MASK = sizeof(T) == 1 ? 0xffu : (sizeof(T) == 2 ? 0xffffu : 0xffffffffu);
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = wv::smap<T>(w[i]);  // signed samples: one xor per dword
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = (w[e / PER] >> (8 * sizeof(T) * (e % PER))) & MASK;
}
template <typename T, int N>
__device__ __forceinline__ void g_storen(T* p, const uint32_t (&v)[N]) {
  constexpr int NW = N * (int)sizeof(T) / 4;
  static_assert(N * sizeof(T) % 4 == 0, "g_storen: whole dwords");
  constexpr int PER = 4 / (int)(sizeof(T) < 4 ? sizeof(T) : 4);
  constexpr uint32_t MASK = sizeof(T) == 1 ? 0xffu : (sizeof(T) == 2 ? 0xffffu : 0xffffffffu);
  uint32_t w[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = 0u;
#pragma unroll
  for (int e = 0; e < N; ++e) w[e / PER] |= (v[e] & MASK) << (8 * sizeof(T) * (e % PER));
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = wv::smap<T>(w[i]);  // signed samples: one xor per dword
  char* c = (char*)p;
  constexpr int N4 = NW / 4 * 4;
#pragma unroll
  for (int i = 0; i < N4; i += 4) *(g32x4a1*)(c + 4 * i) = g32x4a1{w[i], w[i + 1], w[i + 2], w[i + 3]};
  if constexpr (NW - N4 >= 2) *(g32x2a1*)(c + 4 * N4) = g32x2a1{w[N4], w[N4 + 1]};
  if constexpr ((NW - N4) % 2) *(g32a1*)(c + 4 * (NW - 1)) = w[NW - 1];
}

// (b, oz, oy, xq) of a flat thread index over B x ext0 x ext1 x nxq (xq: a group of 4 columns)
struct Row4 {
  FDiv dq, d1, d0;
};
#endif

#ifdef KMP_PASS_KERNEL  // ---- the kernel section: KMP_PASS_KERNEL its name, KMP_PASS_PARAM what follows its
// last parameter, KMP_PASS_ENC / KMP_PASS_DEC the coder's calls (defined where the section is included) ----
// CC channels (1..4, interleaved): a thread owns 4 output positions x CC channels of a row, so
// its highres rows are 8 x CC consecutive samples, its lowres / map values 4 x CC, its cells 5 x CC
// FK > 0 (images, one channel, f32 LinearPredictor with KK = FK = 2p + 2 <= 4): no cells array --
// the thread computes the 2 x 5 cells around its outputs itself, from a (FK + 1) x (FK + 4) patch
// of lowres nodes, with the reference's fma chain (linear_valu_kernel's arithmetic: same bits).
// Each cell is computed by ~2.5 threads; the cells pass (a write and a re-read of 5 predictions a
// cell) is gone.
template <typename T, int CODER, bool PERCH, int NSP, int CC, bool DEC, int FK = 0>
__global__ void __launch_bounds__(kThreads) KMP_PASS_KERNEL(const T* __restrict__ src, CMapPtrs imaps, Geo g,
                                                             const T* __restrict__ cells, int64_t B, T* __restrict__ dst,
                                                             MapPtrs omaps, Frame f, Row4 R, int64_t nxq,
                                                             int64_t total, Src ns = Src{}, const float* W = nullptr,
                                                             const float* bias = nullptr, int p = 0 KMP_PASS_PARAM) {
  static_assert(FK == 0 || (NSP == 2 && CC == 1 && PERCH), "fused cells: images, one channel, LinearPredictor");
  constexpr int FKO = 5, FN = FK * FK;  // outputs / features of a 2D cell
  __shared__ float wl[FK > 0 ? FN * FKO + FKO : 1];
  if constexpr (FK > 0) {
    for (int i = threadIdx.x; i < FN * FKO + FKO; i += blockDim.x) wl[i] = i < FN * FKO ? W[i] : bias[i - FN * FKO];
    __syncthreads();
  }
  using I = int32_t;
  using TO = typename coder_out<CODER>::type;
  // the numbers of the samples (signed samples: M(x), Signed in kmp_common.h; any other type: T
  // itself): cells and samples are converted once where they are loaded and kept as numbers
  using TM = typename sample_traits<T>::mapped;
  constexpr int NM = NSP == 3 ? 7 : 3;
  constexpr int NZ = NSP == 3 ? 2 : 1;
  constexpr int NH = 8 * CC, NO = 4 * CC;  // samples of a highres row segment / of an output group
  const I hy = (I)g.n[2] * CC, hz = (I)g.n[1] * hy, hb = (I)g.n[0] * hz;
  const I ly = (I)g.E[2] * CC, lz = (I)g.E[1] * ly, lb = (I)g.E[0] * lz;
  const I cy = (I)g.Lc[2] * CC, cz = (I)g.Lc[1] * cy, cb = (I)g.Lc[0] * cz;
  const I kp = (I)B * cb;  // LinearPredictor: channel plane stride (planar cells)
  const I end2 = (I)(f.begin[2] + f.ext[2]);
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    I b, oz, oy, xq;
    {
      uint32_t u = (uint32_t)t, q;
      q = fdiv_q(u, R.dq); xq = (I)(u - q * R.dq.d); u = q;
      q = fdiv_q(u, R.d1); oy = (I)(u - q * R.d1.d); u = q;
      q = fdiv_q(u, R.d0); oz = (I)(u - q * R.d0.d); b = (I)q;
    }
    oz += (I)f.begin[0];
    oy += (I)f.begin[1];
    const I ox0 = (I)f.begin[2] + 4 * xq;
    const int nout = (int)(end2 - ox0 < 4 ? end2 - ox0 : 4);
    // ---- the cells around the 4 outputs: (oz - dz, oy - dy, ox0 - 1 + j), j = 0..4 ----
    const I cbase = b * cb + oz * cz + oy * cy + ox0 * CC;  // cell (oz, oy, ox0), channel 0
    bool cv[2][2][5];
    TM cm[2][2][5][CC];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const bool rowok = (NSP == 3 || dz == 0) && oz - dz >= 0 && oz - dz < (I)g.Lc[0] && oy - dy >= 0 &&
                           oy - dy < (I)g.Lc[1];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const I x = ox0 - 1 + j;
          cv[dz][dy][j] = rowok && x >= 0 && x < (I)g.Lc[2];
#pragma unroll
          for (int ch = 0; ch < CC; ++ch)
            if (!PERCH) cm[dz][dy][j][ch] = cv[dz][dy][j] ? (TM)cells[cbase - dz * cz - dy * cy + (j - 1) * CC + ch] : TM(0);
        }
      }
    // map k's contribution channel kch of the cell (oz - dz, oy - dy, ox0 + i - dx), sample channel ch
    // FK > 0: the cells (oy - dy, ox0 - 1 + j), channels kch, computed here
    TM pc[FK > 0 ? 2 : 1][FK > 0 ? 5 : 1][FKO];
    if constexpr (FK > 0) {
      constexpr int NRW = FK + 1, NCL = FK + 4;  // node patch: rows oy - 1 - p .., cols ox0 - 1 - p ..
      const I sr = DEC ? (I)g.E[2] : (I)g.n[2];
      const I sb = DEC ? (I)(g.E[0] * g.E[1] * g.E[2]) : (I)(g.n[0] * g.n[1] * g.n[2]);
      I col[NCL];
#pragma unroll
      for (int c2 = 0; c2 < NCL; ++c2) col[c2] = (I)node_src((int64_t)ox0 - 1 - p + c2, g.L[2], g.E[2], ns.mult);
      float nd[NRW][NCL];
#pragma unroll
      for (int r2 = 0; r2 < NRW; ++r2) {
        const I rb = b * sb + (I)node_src((int64_t)oy - 1 - p + r2, g.L[1], g.E[1], ns.mult) * sr;
#pragma unroll
        for (int c2 = 0; c2 < NCL; ++c2) nd[r2][c2] = (float)src[rb + col[c2]];
      }
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          float acc[FKO];
#pragma unroll
          for (int k = 0; k < FKO; ++k) acc[k] = wl[FN * FKO + k];
#pragma unroll
          for (int fy = 0; fy < FK; ++fy)
#pragma unroll
            for (int fx = 0; fx < FK; ++fx) {
              const float fv = nd[1 - dy + fy][j + fx];
#pragma unroll
              for (int k = 0; k < FKO; ++k) acc[k] = __builtin_fmaf(fv, wl[(fy * FK + fx) * FKO + k], acc[k]);
            }
#pragma unroll
          for (int k = 0; k < FKO; ++k) pc[dy][j][k] = lin_cast_t<TM>(acc[k]);
        }
    }
    auto cell = [&](int i, int dz, int dy, int dx, int kch, int ch) -> TM {
      if constexpr (FK > 0) return pc[dy][i + 1 - dx][kch];
      else if constexpr (PERCH) return (TM)cells[cbase - dz * cz - dy * cy + (i - dx) * CC + ch + (I)kch * kp];
      else return cm[dz][dy][i + 1 - dx][ch];
    };
    auto pred = [&](int k, int i, int ch) -> uint32_t {
      Contrib c[4];
      const int nc = map_contribs(NSP, k, c);
      if (k == center_map(NSP)) return (uint32_t)to_i32(cell(i, 0, 0, 0, c[0].ch, ch));
      float sacc = 0.0f;
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q >= nc) break;
        if (cv[c[q].dz][c[q].dy][i + 1 - c[q].dx]) {
          sacc += (float)cell(i, c[q].dz, c[q].dy, c[q].dx, c[q].ch, ch);
          ++cnt;
        }
      }
      if (cnt == 4) sacc *= 0.25f;
      else if (cnt == 2) sacc *= 0.5f;
      return (uint32_t)to_i32(gcast<TM>(sacc));
    };
    if constexpr (!DEC) {
      // ---- encode: the 8 x CC samples of each of the 2^d highres rows, then lowres + maps ----
      uint32_t hv[NZ][2][NH];
#pragma unroll
      for (int pz = 0; pz < NZ; ++pz)
#pragma unroll
        for (int py = 0; py < 2; ++py) {
          const I hz_ = 2 * oz + pz, hy_ = 2 * oy + py;
          const bool rowok = hz_ < (I)g.n[0] && hy_ < (I)g.n[1];
          const T* rp = src + b * hb + hz_ * hz + hy_ * hy + 2 * ox0 * CC;
          if (rowok && 2 * ox0 + 8 <= (I)g.n[2]) {
            g_loadn<T, NH>(rp, hv[pz][py]);
          } else {
#pragma unroll
            for (int e = 0; e < NH; ++e) hv[pz][py][e] = (rowok && 2 * ox0 + e / CC < (I)g.n[2]) ? (uint32_t)rp[e] : 0u;
          }
        }
      if (oz < (I)g.E[0] && oy < (I)g.E[1]) {
        uint32_t lv[NO];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int ch = 0; ch < CC; ++ch) lv[i * CC + ch] = hv[0][0][2 * i * CC + ch];
        T* lp = dst + b * lb + oz * lz + oy * ly + ox0 * CC;
        const int n = (int)((I)g.E[2] - ox0 < nout ? (I)g.E[2] - ox0 : nout);
        if (n == 4) g_storen<T, NO>(lp, lv);
        else
#pragma unroll
          for (int e = 0; e < NO; ++e)
            if (e / CC < n) lp[e] = (T)lv[e];
      }
#pragma unroll
      for (int k = 0; k < NM; ++k) {
        const int p0 = gpar<NSP>(k, 0), p1 = gpar<NSP>(k, 1), p2 = gpar<NSP>(k, 2);
        const I e0 = (I)(p0 ? g.Lc[0] : g.E[0]), e1 = (I)(p1 ? g.Lc[1] : g.E[1]), e2 = (I)(p2 ? g.Lc[2] : g.E[2]);
        if (oz >= e0 || oy >= e1) continue;
        const int n = (int)(e2 - ox0 < nout ? e2 - ox0 : nout);
        if (n <= 0) continue;
        uint32_t ov[NO];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int ch = 0; ch < CC; ++ch)
            ov[i * CC + ch] = (uint32_t)KMP_PASS_ENC((int32_t)pred(k, i, ch),
                                                           to_i32((TM)hv[NSP == 3 ? p0 : 0][p1][(2 * i + p2) * CC + ch]));
        TO* mp = (TO*)omaps.p[k] + (((b * e0 + oz) * e1 + oy) * e2 + ox0) * CC;
        if (n == 4) g_storen<TO, NO>(mp, ov);
        else
#pragma unroll
          for (int e = 0; e < NO; ++e)
            if (e / CC < n) mp[e] = (TO)ov[e];
      }
    } else {
      // ---- decode: lowres + maps into the 8 x CC samples of each highres row ----
      uint32_t hv[NZ][2][8][CC];
      bool hok[NZ][2][8];
#pragma unroll
      for (int pz = 0; pz < NZ; ++pz)
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
#pragma unroll
            for (int ch = 0; ch < CC; ++ch) hv[pz][py][e][ch] = 0u;
            hok[pz][py][e] = false;
          }
      if (oz < (I)g.E[0] && oy < (I)g.E[1]) {
        const T* lp = src + b * lb + oz * lz + oy * ly + ox0 * CC;
        const int n = (int)((I)g.E[2] - ox0 < nout ? (I)g.E[2] - ox0 : nout);
        uint32_t lv[NO];
        if (n == 4) g_loadn<T, NO>(lp, lv);
        else
#pragma unroll
          for (int e = 0; e < NO; ++e) lv[e] = e / CC < n ? (uint32_t)lp[e] : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int ch = 0; ch < CC; ++ch) hv[0][0][2 * i][ch] = lv[i * CC + ch];
          hok[0][0][2 * i] = i < n;
        }
      }
#pragma unroll
      for (int k = 0; k < NM; ++k) {
        const int p0 = gpar<NSP>(k, 0), p1 = gpar<NSP>(k, 1), p2 = gpar<NSP>(k, 2);
        const I e0 = (I)(p0 ? g.Lc[0] : g.E[0]), e1 = (I)(p1 ? g.Lc[1] : g.E[1]), e2 = (I)(p2 ? g.Lc[2] : g.E[2]);
        if (oz >= e0 || oy >= e1) continue;
        const int n = (int)(e2 - ox0 < nout ? e2 - ox0 : nout);
        if (n <= 0) continue;
        const TO* mp = (const TO*)imaps.p[k] + (((b * e0 + oz) * e1 + oy) * e2 + ox0) * CC;
        uint32_t mv[NO];
        if (n == 4) g_loadn<TO, NO>(mp, mv);
        else
#pragma unroll
          for (int e = 0; e < NO; ++e) mv[e] = e / CC < n ? (uint32_t)mp[e] : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int ch = 0; ch < CC; ++ch)
            hv[NSP == 3 ? p0 : 0][p1][2 * i + p2][ch] =
                (uint32_t)(TM)KMP_PASS_DEC((int32_t)pred(k, i, ch), (int32_t)(TO)mv[i * CC + ch]);
          hok[NSP == 3 ? p0 : 0][p1][2 * i + p2] = i < n;
        }
      }
#pragma unroll
      for (int pz = 0; pz < NZ; ++pz)
#pragma unroll
        for (int py = 0; py < 2; ++py) {
          const I hz_ = 2 * oz + pz, hy_ = 2 * oy + py;
          if (hz_ >= (I)g.n[0] || hy_ >= (I)g.n[1]) continue;
          T* rp = dst + b * hb + hz_ * hz + hy_ * hy + 2 * ox0 * CC;
          bool all = true;
#pragma unroll
          for (int e = 0; e < 8; ++e) all = all && hok[pz][py][e];
          uint32_t row[NH];
#pragma unroll
          for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int ch = 0; ch < CC; ++ch) row[e * CC + ch] = hv[pz][py][e][ch];
          if (all) g_storen<T, NH>(rp, row);
          else
#pragma unroll
            for (int e = 0; e < NH; ++e)
              if (hok[pz][py][e / CC]) rp[e] = (T)row[e];
        }
    }
  }
}

#else  // ---- the whole file ----
// The kernel above, compiled once per coder family by including this file's kernel section: the
// modular coders (the token stream it always was), and the near-lossless coders (kmp_common.h) with
// their bound as one more argument.
#define KMP_PASS_KERNEL codec_row4_kernel
#define KMP_PASS_PARAM
#define KMP_PASS_ENC(p, x) code_encode<CODER>(p, x)
#define KMP_PASS_DEC(p, e) code_decode<CODER>(p, e)
#include "kmp_codec_generic_row4.hip"
#undef KMP_PASS_KERNEL
#undef KMP_PASS_PARAM
#undef KMP_PASS_ENC
#undef KMP_PASS_DEC
#define KMP_PASS_KERNEL codec_row4_near_kernel
#define KMP_PASS_PARAM , NearQ nq = NearQ{}
#define KMP_PASS_ENC(p, x) coder_enc<CODER>(nq, p, x)
#define KMP_PASS_DEC(p, e) coder_dec<CODER>(nq, p, e)
#include "kmp_codec_generic_row4.hip"
#undef KMP_PASS_KERNEL
#undef KMP_PASS_PARAM
#undef KMP_PASS_ENC
#undef KMP_PASS_DEC

// the row kernel's compile-time channel count (1..4; 3D takes 1..2 -- with 3-4 channels its
// 7 maps' values outgrow the registers and spill)
template <typename F>
static void with_cc(int64_t C, F&& f) {
  if (C == 1) f(std::integral_constant<int, 1>{});
  else if (C == 2) f(std::integral_constant<int, 2>{});
  else if (C == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

template <typename T, bool DEC>
void launch_row4(const CodecCall<T, DEC>& c, const Src& s, const Frame& f, const T* cells) {
  constexpr int CODER = natural_coder<T>::value;
  const int64_t nxq = ceil_div(f.ext[2], 4), n4 = c.B * f.ext[0] * f.ext[1] * nxq;
  const Row4 R{fdiv(nxq), fdiv(f.ext[1]), fdiv(f.ext[0])};
  const CMapPtrs imaps = DEC ? cmaps(c.maps) : CMapPtrs{};
  const MapPtrs omaps = DEC ? MapPtrs{} : c.maps;
  if (!cells) {  // the cells computed in the kernel, FK = 2p + 2 nodes per axis (p <= 1)
    auto fused = [&](auto fk_c) {
      if constexpr (sizeof(T) <= 2) {
        if (c.max_error) {
          codec_row4_near_kernel<T, near_coder<T>::value, true, 2, 1, DEC, decltype(fk_c)::value>
              <<<grid_for(n4), kThreads, 0, c.stream>>>(c.in, imaps, c.g, nullptr, c.B, c.out, omaps, f, R, nxq, n4, s,
                                                        c.pred->weights, c.pred->bias, c.pred->padding,
                                                        make_nearq(c.max_error));
          return;
        }
      }
      codec_row4_kernel<T, CODER, true, 2, 1, DEC, decltype(fk_c)::value><<<grid_for(n4), kThreads, 0, c.stream>>>(
          c.in, imaps, c.g, nullptr, c.B, c.out, omaps, f, R, nxq, n4, s, c.pred->weights, c.pred->bias,
          c.pred->padding);
    };
    if (c.pred->padding == 0) fused(std::integral_constant<int, 2>{});
    else fused(std::integral_constant<int, 4>{});
    return;
  }
  with_nsp_perch(c.nsp, c.pred->kind != KMP_PRED_MEAN, [&](auto nsp_c, auto perch_c) {
    with_cc(c.C, [&](auto cc_c) {
      constexpr int NSP = decltype(nsp_c)::value, CC = decltype(cc_c)::value;
      if constexpr (NSP == 2 || CC <= 2) {
        if constexpr (sizeof(T) <= 2) {
          if (c.max_error) {
            codec_row4_near_kernel<T, near_coder<T>::value, decltype(perch_c)::value, NSP, CC, DEC>
                <<<grid_for(n4), kThreads, 0, c.stream>>>(c.in, imaps, c.g, cells, c.B, c.out, omaps, f, R, nxq, n4,
                                                          Src{}, nullptr, nullptr, 0, make_nearq(c.max_error));
            return;
          }
        }
        codec_row4_kernel<T, CODER, decltype(perch_c)::value, NSP, CC, DEC>
            <<<grid_for(n4), kThreads, 0, c.stream>>>(c.in, imaps, c.g, cells, c.B, c.out, omaps, f, R, nxq, n4);
      }
    });
  });
}

#define KMP_INST_ROW4(T)                                                                               \
  template void launch_row4<T, false>(const CodecCall<T, false>&, const Src&, const Frame&, const T*); \
  template void launch_row4<T, true>(const CodecCall<T, true>&, const Src&, const Frame&, const T*);
KMP_FOR_SAMPLE_TYPES(KMP_INST_ROW4)

}  // namespace kmp
#endif

// kmp_codec_generic.hip -- the fused encode/decode for ANY shape, channel count, padding and
// integer dtype: two launches per direction.
//
//   1. predictor apply: one value per cell (MEAN) or K per cell (LINEAR) into a workspace
//      [K, B, Lc..., C] (channel planes) -- the reference's features_from_lowres + mean/astype
//      (tests/volume/test_encode_decode.py:46-51) without materialising the features;
//   2. residual pass: per output block position o, read the 2^d highres block at 2o, aggregate
//      the cell predictions exactly as maps_from_predictions does (kmp_aggregate.h), apply the
//      coder and write lowres + every map in its trimmed shape (encode), or the inverse
//      (decode: interleave into highres, highres_from_lowres_and_maps + trim).
//
// Lowres node j of the padded volume along an axis is source sample 2*sym(j, E) (encode: even
// reflect pad volume/utils.py:226-237) or sym(j, E) of the trimmed lowres (decode: symmetric
// pad_lowres volume/utils.py:240-244); the neighbourhood padding adds sym(., L)
// (pad_neighborhood volume/utils.py:213-218).  Costs ~1.25x the HBM bytes of the one-pass
// fast kernels (kmp_codec_fast3d.hip); used whenever those are not eligible: the last entry of
// every list of the dispatch table (kmp_codec.hip), and the only entry of a near-lossless request's
// (CodecCall::max_error > 0).  Here: the host side and the per-element residual
// kernel (compiled once per coder family, below); kmp_codec_generic_cells.hip is pass 1,
// kmp_codec_generic_row4.hip the residual pass for up to 4 channels.
#ifndef KMP_PASS_KERNEL  // (this file includes its own kernel section, below)
#include "kmp_generic.h"

namespace kmp {

// Per output position o (and channel): the lowres node and the 7 (3) maps.  The cell values the
// maps aggregate are read once: the 2^d cells o - {0,1}^d (MeanPredictor: one value per cell), or
// each contribution's channel (LinearPredictor: K per cell, planar: channel ch of every cell in
// plane ch, kmp_linear.hip launch_linear); missing cells (past the cell box) are skipped exactly as
// maps_from_predictions does, in the reference's channel order.
template <typename T, int NSP, bool PERCH, typename I>
struct GenCells {
  const T* cells;
  I base, sx, sy, sz;  // cells[base - dz sz - dy sy - dx sx + ch kp]
  I kp;                // LinearPredictor: the channel plane stride
  bool v[2][2][2];     // cell o - (dz, dy, dx) exists
  T m[2][2][2];        // MeanPredictor: the cell means

  __device__ __forceinline__ void init(const T* c_, I b, I oz, I oy, I ox, I c, const Geo& g, I Cc, I kp_) {
    cells = c_;
    kp = kp_;
    sx = Cc;
    sy = (I)g.Lc[2] * Cc;
    sz = (I)g.Lc[1] * sy;
    base = b * ((I)g.Lc[0] * sz) + oz * sz + oy * sy + ox * sx + c;
    const bool vz[2] = {oz < (I)g.Lc[0], oz >= 1}, vy[2] = {oy < (I)g.Lc[1], oy >= 1},
               vx[2] = {ox < (I)g.Lc[2], ox >= 1};
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          v[dz][dy][dx] = (NSP == 3 || dz == 0) && vz[dz] && vy[dy] && vx[dx];
          if (!PERCH) m[dz][dy][dx] = v[dz][dy][dx] ? cells[base - dz * sz - dy * sy - dx * sx] : T(0);
        }
  }
  __device__ __forceinline__ T get(int dz, int dy, int dx, int ch) const {
    if constexpr (PERCH) return cells[base - dz * sz - dy * sy - dx * sx + (I)ch * kp];
    else return m[dz][dy][dx];
  }
  // map k's prediction (maps_from_predictions for one element)
  __device__ __forceinline__ T pred(int k) const {
    Contrib c[4];
    const int nc = map_contribs(NSP, k, c);
    if (k == center_map(NSP)) return get(0, 0, 0, c[0].ch);
    float s = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= nc) break;
      if (v[c[i].dz][c[i].dy][c[i].dx]) {
        s += (float)get(c[i].dz, c[i].dy, c[i].dx, c[i].ch);
        ++cnt;
      }
    }
    if (cnt == 4) s *= 0.25f;
    else if (cnt == 2) s *= 0.5f;
    return gcast<T>(s);
  }
};
#endif

#ifdef KMP_PASS_KERNEL  // ---- the kernel section: KMP_PASS_KERNEL its name, KMP_PASS_PARAM what follows its
// last parameter, KMP_PASS_ENC / KMP_PASS_DEC the coder's calls (defined where the section is included) ----
// The residual pass, one thread per output position and channel: any channel count, 64-bit indices
// when the arrays need them.  Encode reads highres ``src`` and writes lowres ``dst`` + ``omaps``;
// decode reads lowres ``src`` + ``imaps`` and writes highres ``dst`` (the other maps stay unused).
template <typename T, int CODER, bool PERCH, int NSP, typename I, bool DEC>
__global__ void __launch_bounds__(kThreads) KMP_PASS_KERNEL(const T* __restrict__ src, CMapPtrs imaps, Geo g,
                                                                int64_t B, int64_t C, const T* __restrict__ cells,
                                                                int K, T* __restrict__ dst, MapPtrs omaps, Frame f,
                                                                Flat F, int64_t total KMP_PASS_PARAM) {
  using TO = typename coder_out<CODER>::type;
  constexpr int NM = NSP == 3 ? 7 : 3;
  const I Cc = (I)C;
  const I hy = (I)g.n[2] * Cc, hz = (I)g.n[1] * hy, hb = (I)g.n[0] * hz;
  const I ly = (I)g.E[2] * Cc, lz = (I)g.E[1] * ly, lb = (I)g.E[0] * lz;
  const I kp = (I)(B * g.Lc[0] * g.Lc[1] * g.Lc[2] * C);  // LinearPredictor: channel plane stride
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    I b, oz, oy, ox, c;
    unflat_i<I>(t, F, f.ext, C, b, oz, oy, ox, c);
    oz += (I)f.begin[0];
    oy += (I)f.begin[1];
    ox += (I)f.begin[2];
    const I h0 = b * hb + (2 * oz) * hz + (2 * oy) * hy + (2 * ox) * Cc + c;
    if (oz < (I)g.E[0] && oy < (I)g.E[1] && ox < (I)g.E[2]) {
      if constexpr (DEC) dst[h0] = src[b * lb + oz * lz + oy * ly + ox * Cc + c];
      else dst[b * lb + oz * lz + oy * ly + ox * Cc + c] = src[h0];
    }
    GenCells<T, NSP, PERCH, I> gc;
    gc.init(cells, b, oz, oy, ox, c, g, Cc, kp);
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const int p0 = gpar<NSP>(k, 0), p1 = gpar<NSP>(k, 1), p2 = gpar<NSP>(k, 2);
      const I e0 = (I)(p0 ? g.Lc[0] : g.E[0]), e1 = (I)(p1 ? g.Lc[1] : g.E[1]), e2 = (I)(p2 ? g.Lc[2] : g.E[2]);
      if (oz >= e0 || oy >= e1 || ox >= e2) continue;
      const T pred = gc.pred(k);
      if constexpr (DEC) {
        const TO enc = ((const TO*)imaps.p[k])[((b * e0 + oz) * e1 + oy) * e2 * Cc + ox * Cc + c];
        dst[h0 + p0 * hz + p1 * hy + p2 * Cc] = (T)KMP_PASS_DEC(to_i32(pred), to_i32(enc));
      } else {
        const T gt = src[h0 + p0 * hz + p1 * hy + p2 * Cc];
        ((TO*)omaps.p[k])[((b * e0 + oz) * e1 + oy) * e2 * Cc + ox * Cc + c] =
            KMP_PASS_ENC(to_i32(pred), to_i32(gt));
      }
    }
  }
}

#else  // ---- the whole file ----
// The kernel above, compiled once per coder family by including this file's kernel section: the
// modular coders (the token stream it always was), and the near-lossless coders (kmp_common.h) with
// their bound as one more argument.
#define KMP_PASS_KERNEL codec_generic_kernel
#define KMP_PASS_PARAM
#define KMP_PASS_ENC(p, x) code_encode<CODER>(p, x)
#define KMP_PASS_DEC(p, e) code_decode<CODER>(p, e)
#include "kmp_codec_generic.hip"
#undef KMP_PASS_KERNEL
#undef KMP_PASS_PARAM
#undef KMP_PASS_ENC
#undef KMP_PASS_DEC
#define KMP_PASS_KERNEL codec_generic_near_kernel
#define KMP_PASS_PARAM , NearQ nq
#define KMP_PASS_ENC(p, x) coder_enc<CODER>(nq, p, x)
#define KMP_PASS_DEC(p, e) coder_dec<CODER>(nq, p, e)
#include "kmp_codec_generic.hip"
#undef KMP_PASS_KERNEL
#undef KMP_PASS_PARAM
#undef KMP_PASS_ENC
#undef KMP_PASS_DEC

// Images with one channel and the f32 LinearPredictor at p <= 1: the row kernel computes its cells
// itself (codec_row4_kernel FK > 0; at p = 2 the 7 x 10 node patch and 36 x 5 weights outgrow the
// registers); KMP_DISABLE_LINEAR_FUSED=1 keeps the two-pass path
static bool fuse_lin2d(int nsp, int64_t C, const Geo& g, int64_t B, const kmp_predictor* pred) {
  return nsp == 2 && C == 1 && pred->kind == KMP_PRED_LINEAR && pred->padding <= 1 && pred->weights && pred->bias &&
         fits32(g, B, C, 5) && !opt(OPT_DISABLE_LINEAR_FUSED, 0);
}

// The family of last resort: takes every request, so it never answers KMP_ERR_UNSUPPORTED.
template <typename T, bool DEC>
int try_generic(const CodecCall<T, DEC>& c) {
  const Geo& g = c.g;
  const char* name = DEC ? "decode_generic" : "encode_generic";
  const int64_t need = generic_workspace_bytes(dtype_code<T>(), c.nsp, g, c.B, c.C, c.pred);
  if ((int64_t)c.ws_bytes < need || (!c.ws && need > 0))
    return fail(KMP_ERR_ARG, std::string(DEC ? "decode" : "encode") + ": workspace too small (" +
                                 std::to_string(c.ws_bytes) + " < " + std::to_string(need) + ")");
  // the lowres nodes the predictor reads: every other highres sample (encode), the lowres (decode)
  const Src s = DEC ? Src{{g.E[0], g.E[1], g.E[2]}, 1} : Src{{g.n[0], g.n[1], g.n[2]}, 2};
  T* cells = (T*)c.ws;  // not null: B > 0 and every axis has a cell, so need > 0
  const Frame f = make_frame(c.nsp, g, c.region);
  const int64_t total = c.B * f.ext[0] * f.ext[1] * f.ext[2] * c.C;
  if (fuse_lin2d(c.nsp, c.C, g, c.B, c.pred)) {  // the cells computed in the row kernel
    if (total == 0) return KMP_OK;
    launch_row4<T, DEC>(c, s, f, nullptr);
    return check_launch(name);
  }
  if (int st = run_predictor<T>(c.in, s, g, c.nsp, c.B, c.C, c.pred, f, cells, c.stream)) return st;
  if (total == 0) return KMP_OK;
  const bool perch = c.pred->kind != KMP_PRED_MEAN;
  const int K = perch ? (c.nsp == 3 ? 19 : 5) : 1;
  const bool i32 = fits32(g, c.B, c.C, K);
  if (c.C <= (c.nsp == 3 ? 2 : 4) && i32) {  // 4 output positions (x C) a thread (with_cc)
    launch_row4<T, DEC>(c, s, f, cells);
    return check_launch(name);
  }
  const Flat F = make_flat(f.ext, c.C);
  const CMapPtrs imaps = DEC ? cmaps(c.maps) : CMapPtrs{};
  const MapPtrs omaps = DEC ? MapPtrs{} : c.maps;
  with_nsp_perch(c.nsp, perch, [&](auto nsp_c, auto perch_c) {
    auto go = [&](auto i_tag) {
      if constexpr (sizeof(T) <= 2) {
        if (c.max_error) {
          codec_generic_near_kernel<T, near_coder<T>::value, decltype(perch_c)::value, decltype(nsp_c)::value,
                                    decltype(i_tag), DEC><<<grid_for(total), kThreads, 0, c.stream>>>(
              c.in, imaps, g, c.B, c.C, cells, K, c.out, omaps, f, F, total, make_nearq(c.max_error));
          return;
        }
      }
      codec_generic_kernel<T, natural_coder<T>::value, decltype(perch_c)::value, decltype(nsp_c)::value,
                           decltype(i_tag), DEC>
          <<<grid_for(total), kThreads, 0, c.stream>>>(c.in, imaps, g, c.B, c.C, cells, K, c.out, omaps, f, F, total);
    };
    if (i32) go(int32_t{});
    else go(int64_t{});
  });
  return check_launch(name);
}

KMP_INST_FAMILY(try_generic, uint8_t)
KMP_INST_FAMILY(try_generic, uint16_t)
KMP_INST_FAMILY(try_generic, int32_t)
KMP_INST_FAMILY(try_generic, uint32_t)
KMP_INST_FAMILY_SIGNED(try_generic)

}  // namespace kmp
#endif

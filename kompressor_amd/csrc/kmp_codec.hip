// kmp_codec.hip -- the fused codec's front door: the C entry points (kmp_volume_* / kmp_image_*),
// the checks of a request, and the table that picks the kernel family serving it.
#include "kmp_codec.h"

namespace kmp {

// f(T{}) for a dtype with its natural coder (natural_coder, kmp_codec.h) or, for 8- / 16-bit samples,
// the near-lossless coder of its width (near_coder; the bound travels in CodecCall); nothing else is served
template <typename F>
static int dispatch_natural(int dtype, int coder, F&& f) {
  if (int st = check_coder_arg(coder, dtype_size(dtype), "fused codec")) return st;
  if (is_near_code(coder_code(coder))) {  // the width matches the dtype's: checked
    if (dtype == KMP_U8) return f(uint8_t{});
    if (dtype == KMP_U16) return f(uint16_t{});
    if (dtype == KMP_I8) return f(i8s{});
    if (dtype == KMP_I16) return f(i16s{});
    return fail(KMP_ERR_ARG, "fused codec: unsupported sample dtype " + std::to_string(dtype));
  }
  if (dtype == KMP_U8 && coder == natural_coder<uint8_t>::value) return f(uint8_t{});
  if (dtype == KMP_U16 && coder == natural_coder<uint16_t>::value) return f(uint16_t{});
  if (dtype == KMP_I32 && coder == natural_coder<int32_t>::value) return f(int32_t{});
  if (dtype == KMP_U32 && coder == natural_coder<uint32_t>::value) return f(uint32_t{});
  if (dtype == KMP_I8 && coder == natural_coder<i8s>::value) return f(i8s{});
  if (dtype == KMP_I16 && coder == natural_coder<i16s>::value) return f(i16s{});
  return fail(KMP_ERR_UNSUPPORTED, "fused codec supports (uint8, U8), (uint16, U16), (int32, RAW), (uint32, U32), (int8, U8), (int16, U16); got dtype " +
                                       std::to_string(dtype) + " coder " + std::to_string(coder));
}

// ------------------------------------------------------------------------------------------
// Kernel selection: THE dispatch table.  The kernel families (kmp_codec.h) of a request's
// (spatial rank, sample width), in the order they are tried; encode and decode walk the same list,
// so one family serves both directions of a configuration.  The first family that does not answer
// KMP_ERR_UNSUPPORTED served (or failed) the call.  Every list ends with the generic two-pass path
// (kmp_codec_generic.hip), which takes any request and never answers KMP_ERR_UNSUPPORTED, so the
// walk always ends at a family.  A family earlier in a list shadows the later ones wherever both
// are eligible: the barrier-free wave kernels before the fused linear kernels (disjoint predictor
// kinds), the LDS kernels (fast3d / fast2d) as the fallback for the geometries the wave kernels
// refuse.
// ------------------------------------------------------------------------------------------
template <typename T, bool DEC>
static int serve(const CodecCall<T, DEC>& c) {
  using Try = int (*)(const CodecCall<T, DEC>&);
  const Try* family;  // nullptr-terminated
  // a near-lossless request: the generic family alone has the quantising coder
  static constexpr Try near[] = {try_generic<T, DEC>, nullptr};
  if (c.max_error) {
    family = near;
  } else if constexpr (sizeof(T) == 4) {
    static constexpr Try volume[] = {try_wave3d32<T, DEC>, try_generic<T, DEC>, nullptr};
    static constexpr Try image[] = {try_generic<T, DEC>, nullptr};
    family = c.nsp == 3 ? volume : image;
  } else if constexpr (sample_sign<T> != 0) {
    // signed samples: the kernels that apply the sign map (DESIGN.md "Signed samples"); the others
    // are not instantiated for them, so everything else is the generic path's
    static constexpr Try volume[] = {try_wave3d<T, DEC>, try_generic<T, DEC>, nullptr};  // mean p = 0 | anything
    static constexpr Try image[] = {try_wave2d<T, DEC>, try_generic<T, DEC>, nullptr};   // mean p = 0 | anything
    family = c.nsp == 3 ? volume : image;
  } else {
    static constexpr Try volume[] = {
        try_wave3d<T, DEC>,     // mean p = 0
        try_linear3m<T, DEC>,   // matrix-core linear p = 0
        try_linear3d<T, DEC>,   // f32 linear p = 0
        try_wave3dp<T, DEC>,    // mean p = 1, 2
        try_linear3dp<T, DEC>,  // f32 linear p = 1
        try_linear3pm<T, DEC>,  // matrix-core linear p = 1
        try_fast3d<T, DEC>,     // mean p <= 2, the LDS kernel
        try_generic<T, DEC>,  // anything
        nullptr};
    static constexpr Try image[] = {
        try_wave2d<T, DEC>,   // mean / f32 linear p = 0
        try_wave2dp<T, DEC>,  // mean p = 1, 2
        try_fast2d<T, DEC>,   // mean p <= 2, the LDS kernel
        try_generic<T, DEC>,  // anything
        nullptr};
    family = c.nsp == 3 ? volume : image;
  }
  for (; *family; ++family) {
    const int st = (*family)(c);
    if (st != KMP_ERR_UNSUPPORTED) return st;
  }
  return KMP_ERR_UNSUPPORTED;  // not reached: try_generic took the request
}

static int check_predictor(const kmp_predictor* pred, int dtype) {
  KMP_REQUIRE(pred, "null predictor");
  KMP_REQUIRE(pred->padding >= 0, "negative padding");
  KMP_REQUIRE(pred->kind == KMP_PRED_MEAN || pred->kind == KMP_PRED_LINEAR || pred->kind == KMP_PRED_LINEAR_MFMA,
              "unknown predictor kind");
  if (pred->kind != KMP_PRED_MEAN) KMP_REQUIRE(pred->weights && pred->bias, "linear predictor needs weights and bias");
  if (pred->kind == KMP_PRED_LINEAR_MFMA)
    KMP_REQUIRE(dtype == KMP_U8 || dtype == KMP_U16,
                "the matrix-core LinearPredictor takes uint8 / uint16 samples (signed int8 / int16: use KMP_PRED_LINEAR)");
  return KMP_OK;
}

int codec_encode(int nsp, int dtype, const void* highres, int64_t B, const int64_t* shape, int64_t C,
                 const kmp_predictor* pred, int coder, void* lowres_out, void* const* maps_out, int32_t* dims_out,
                 const kmp_region* region, void* ws, size_t ws_bytes, hipStream_t stream) {
  KMP_REQUIRE(B >= 0 && C >= 1, "bad batch or channel count");
  for (int a = 0; a < nsp; ++a) KMP_REQUIRE(shape[a] >= 2, "spatial dims must be >= 2 (>= 3 after even padding)");
  if (int st = check_predictor(pred, dtype)) return st;
  Geo g = make_geo_from_highres(nsp, shape);
  if (dims_out)
    for (int a = 0; a < nsp; ++a) dims_out[a] = g.dims[a + 3 - nsp];
  KMP_REQUIRE(highres && lowres_out && maps_out, "null pointer");
  MapPtrs maps{};
  for (int k = 0; k < (nsp == 3 ? 7 : 3); ++k) {
    KMP_REQUIRE(maps_out[k], "null map pointer");
    maps.p[k] = maps_out[k];
  }
  if (B == 0) return KMP_OK;
  return dispatch_natural(dtype, coder, [&](auto tag) {
    using T = decltype(tag);
    return serve(CodecCall<T, false>{nsp, g, B, C, pred, region, (const T*)highres, (T*)lowres_out,
                                     maps, ws, ws_bytes, stream, coder_max_error(coder)});
  });
}

int codec_decode(int nsp, int dtype, const void* lowres, const void* const* maps_in, int64_t B, const int64_t* E,
                 int64_t C, const int32_t* dims, const kmp_predictor* pred, int coder, void* highres_out,
                 const kmp_region* region, void* ws, size_t ws_bytes, hipStream_t stream) {
  KMP_REQUIRE(B >= 0 && C >= 1 && dims, "bad batch/channel count or dims");
  for (int a = 0; a < nsp; ++a) {
    KMP_REQUIRE(dims[a] == 0 || dims[a] == 1, "dims must be 0 or 1");
    KMP_REQUIRE(E[a] >= 1 && E[a] + dims[a] >= 2, "lowres too small");
  }
  if (int st = check_predictor(pred, dtype)) return st;
  Geo g = make_geo_from_lowres(nsp, E, dims);
  KMP_REQUIRE(lowres && maps_in && highres_out, "null pointer");
  MapPtrs maps{};  // the request holds one pointer type; a decode only reads through it
  for (int k = 0; k < (nsp == 3 ? 7 : 3); ++k) {
    KMP_REQUIRE(maps_in[k], "null map pointer");
    maps.p[k] = const_cast<void*>(maps_in[k]);
  }
  if (B == 0) return KMP_OK;
  return dispatch_natural(dtype, coder, [&](auto tag) {
    using T = decltype(tag);
    return serve(CodecCall<T, true>{nsp, g, B, C, pred, region, (const T*)lowres, (T*)highres_out,
                                    maps, ws, ws_bytes, stream, coder_max_error(coder)});
  });
}

}  // namespace kmp

using namespace kmp;

extern "C" {

int kmp_volume_encode(int32_t dtype, const void* highres, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                      const kmp_predictor* predictor, int32_t coder, void* lowres_out, void* const maps_out[7],
                      int32_t dims_out[3], const kmp_region* region, void* workspace, size_t workspace_bytes,
                      kmp_stream_t stream) {
  const int64_t shape[3] = {D, H, W};
  return codec_encode(3, dtype, highres, B, shape, C, predictor, coder, lowres_out, maps_out, dims_out, region,
                      workspace, workspace_bytes, (hipStream_t)stream);
}

int kmp_volume_decode(int32_t dtype, const void* lowres, const void* const maps[7], int64_t B, int64_t Ed, int64_t Eh,
                      int64_t Ew, int64_t C, const int32_t dims[3], const kmp_predictor* predictor, int32_t coder,
                      void* highres_out, const kmp_region* region, void* workspace, size_t workspace_bytes,
                      kmp_stream_t stream) {
  const int64_t E[3] = {Ed, Eh, Ew};
  return codec_decode(3, dtype, lowres, maps, B, E, C, dims, predictor, coder, highres_out, region, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

int64_t kmp_volume_workspace_bytes(int32_t dtype, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                                   const kmp_predictor* predictor) {
  const int64_t shape[3] = {D, H, W};
  Geo g = make_geo_from_highres(3, shape);
  return generic_workspace_bytes(dtype, 3, g, B, C, predictor);
}

int kmp_image_encode(int32_t dtype, const void* highres, int64_t B, int64_t H, int64_t W, int64_t C,
                     const kmp_predictor* predictor, int32_t coder, void* lowres_out, void* const maps_out[3],
                     int32_t dims_out[2], const kmp_region* region, void* workspace, size_t workspace_bytes,
                     kmp_stream_t stream) {
  const int64_t shape[2] = {H, W};
  return codec_encode(2, dtype, highres, B, shape, C, predictor, coder, lowres_out, maps_out, dims_out, region,
                      workspace, workspace_bytes, (hipStream_t)stream);
}

int kmp_image_decode(int32_t dtype, const void* lowres, const void* const maps[3], int64_t B, int64_t Eh, int64_t Ew,
                     int64_t C, const int32_t dims[2], const kmp_predictor* predictor, int32_t coder,
                     void* highres_out, const kmp_region* region, void* workspace, size_t workspace_bytes,
                     kmp_stream_t stream) {
  const int64_t E[2] = {Eh, Ew};
  return codec_decode(2, dtype, lowres, maps, B, E, C, dims, predictor, coder, highres_out, region, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

int64_t kmp_image_workspace_bytes(int32_t dtype, int64_t B, int64_t H, int64_t W, int64_t C,
                                  const kmp_predictor* predictor) {
  const int64_t shape[2] = {H, W};
  Geo g = make_geo_from_highres(2, shape);
  return generic_workspace_bytes(dtype, 2, g, B, C, predictor);
}

}  // extern "C"

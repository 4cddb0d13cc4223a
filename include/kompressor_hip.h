/*
 * kompressor_hip.h -- C-ABI of libkompressor_hip.so, the MI355X (gfx950) engine behind the
 * drop-in ``kompressor_amd.{image,volume}`` API.
 *
 * Conventions
 *   - Arrays are dense, C-contiguous, channels-last device buffers: volumes [B, D, H, W, C],
 *     images [B, H, W, C].  ``C`` is the product of all trailing (channel) dims.
 *   - Every entry point is stream-ordered on ``stream`` (a hipStream_t; NULL = legacy default
 *     stream), returns 0 on success or a negative kmp_status, and never synchronises the
 *     device, allocates, or frees memory (graph-capturable).  ``kmp_last_error()`` returns a
 *     thread-local message for the last failure.
 *   - Geometry follows the reference: an even spatial dim ``n`` is reflect-padded by one
 *     (``dims`` = 1), the lowres grid has L = (n + dims + 1) / 2 nodes, L - 1 cells, and the
 *     stored (trimmed) extent of node-lattice arrays is E = L - dims = ceil(n / 2).
 *
 * Each function names the reference interface it replaces (reference @ v1, file:line).  The
 * reference is pure Python on JAX: "replaces" means the Python function whose semantics the
 * kernel reproduces; the Python layer in kompressor_amd binds these through ctypes.
 */
#ifndef KOMPRESSOR_HIP_H
#define KOMPRESSOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* kmp_stream_t; /* ABI-identical to hipStream_t */

typedef enum {
  KMP_OK = 0,
  KMP_ERR_ARG = -1,      /* bad pointer, shape, dtype or enum */
  KMP_ERR_UNSUPPORTED = -2, /* valid request the engine does not implement */
  KMP_ERR_LAUNCH = -3,   /* HIP launch / runtime error */
} kmp_status;

/* KMP_I8 / KMP_I16: signed samples.  Predictors see M(x) = x ^ signbit (the order-preserving map onto
 * the unsigned type of the same width) and run the unsigned arithmetic on it; residual maps are the
 * unsigned type's, (M(gt) - P) mod 2^W; every sample-domain array a caller passes or receives
 * (highres, lowres, predictions) is in the signed type, bit for bit.  Their natural coders are
 * KMP_CODER_U8 / KMP_CODER_U16.  The data-movement primitives (lowres, maps, targets, pad, tiles,
 * copy_box, features) take the same-width unsigned code for them. */
typedef enum { KMP_U8 = 0, KMP_U16 = 1, KMP_I32 = 2, KMP_F32 = 3, KMP_U32 = 4, KMP_I8 = 5, KMP_I16 = 6 } kmp_dtype;

/* Residual coders, utils.py:28-55 (+ the build's mod-2^32 coder for bit-cast float32). */
typedef enum {
  KMP_CODER_RAW = 0, KMP_CODER_U8 = 1, KMP_CODER_U16 = 2, KMP_CODER_U32 = 3,
  /* Near-lossless coders for 8- / 16-bit samples (signed ones on M(x)).  With the caller's bound
     max_error = d, 1 <= d <= 2^(W-1) - 1, step = 2 d + 1 and P the prediction clamped to [0, 2^W - 1]
     (a float32 prediction truncated first, NaN -> 0): the map holds q = sign(e) ((|e| + d) / step),
     e = x - P, as W-bit two's complement in the unsigned map dtype, and the decode returns
     clamp(P + q step, 0, 2^W - 1), within d of x.  Every ``int32_t coder`` argument that takes them
     carries KMP_CODER_NEAR(code, d).  A lossless code with a max_error, a bound out of range or a width
     that is not the samples' is KMP_ERR_ARG; 32-bit samples are KMP_ERR_UNSUPPORTED.  The fused
     entry points serve them with the generic two-pass family alone. */
  KMP_CODER_NEAR_U8 = 4, KMP_CODER_NEAR_U16 = 5,
  /* Error-bounded float32 quantisers (kmp_code alone).  The step is 2^e, -126 <= e <= 127,
     and the ``coder`` argument carries KMP_CODER_QUANT(code, e).  With QMAX = 32767 (I16) or
     2^31 - 1 (I32), all arithmetic in float64 (every operation is exact but the last conversion):
       n = rint(x 2^-e) (ties to even),  r = (float)(n 2^e);
       x is an exception iff x is not finite, |n| > QMAX, r is not finite or |r - x| > 2^(e-1).
     ENCODE (x_dtype = KMP_F32) writes n as int16 / int32, an exception as the type's minimum
     (-QMAX - 1, which no legal n takes); DECODE (x_dtype = KMP_I16 / KMP_I32, matching the code)
     writes the float32 r of every element.  They take no prediction: ``pred`` must be NULL and
     ``pred_dtype`` is not read.  A non-NULL pred, an exponent field of 0 or >= 255, an x_dtype that
     does not fit, or these codes on any other entry point: KMP_ERR_ARG. */
  KMP_CODER_QUANT_I16 = 6, KMP_CODER_QUANT_I32 = 7,
  /* Relative-error float32 quantisers (kmp_code alone).  They keep the top m mantissa
     bits, 0 <= m <= 22, and the ``coder`` argument carries KMP_CODER_PREC(code, m).  With t = 23 - m,
     QMAX as above, u the float32's bits, s = u >> 31 and a = u & 0x7fffffff, in 32-bit unsigned arithmetic:
       k = (a + 2^(t-1) - 1 + ((a >> t) & 1)) >> t                (round to nearest, ties to even)
       x is an exception iff a >= 0x7f800000, (k << t) >= 0x7f800000 or k > QMAX;  n = s ? -k : k.
     ENCODE (x_dtype = KMP_F32) writes n as int16 / int32, an exception as the type's minimum (no legal
     n takes it: |n| <= 255 2^m - 1); DECODE (x_dtype = KMP_I16 / KMP_I32, matching the code) writes for
     every element the float32 of bits ((|n| << t) & 0x7fffffff) | (n < 0 ? 0x80000000 : 0), |n| as
     uint32.  Every non-exception restores within 2^-(m+1) max(|x|, 2^-126) of x.  ``pred`` must be
     NULL and ``pred_dtype`` is not read.  A non-NULL pred, a field (m + 1) outside [1, 23] -- a bare
     8 or 9 included --, an x_dtype that does not fit, or these codes on any other entry point:
     KMP_ERR_ARG. */
  KMP_CODER_PREC_I16 = 8, KMP_CODER_PREC_I32 = 9,
  /* Error statistics of a restored array against its original (kmp_code alone, KMP_ENCODE alone;
     DESIGN.md §20).  It codes nothing: ``x`` is the original, ``pred`` the restored array (non-NULL),
     both of ``x_dtype`` == ``pred_dtype``, one of KMP_F32, KMP_U8, KMP_U16, KMP_I8, KMP_I16, and ``out`` an
     8-byte aligned device buffer of KMP_COMPARE_BYTES.  The ``coder`` argument carries
     KMP_CODER_COMPARE_MODE(continue).
       float32: element i is COMPARED iff x_i and r_i are both finite; otherwise it is a MISMATCH iff
       their 32-bit patterns differ (a NaN or an infinity restored bit for bit is neither).  Integer
       samples: every element is compared, there are no mismatches.
     Over the compared elements, e_i = (double)r_i - (double)x_i, a RECORD is eight 64-bit words:
       0  count (u64)                       1  mismatch (u64)
       2  max |e_i| (f64 bits; 0.0 when count == 0)
       3  sum e_i^2 (float32 samples: f64 bits; integer samples: u64, exact)
       4, 5  min / max of the compared x_i (f64 bits, a zero as +0.0; +inf / -inf when count == 0)
       6, 7  0
     After the call ``out + 0`` holds the record and ``out + 64 (1 + g)`` the partial record of workgroup g
     for the min(KMP_COMPARE_GROUPS, ceil(items / 256)) workgroups that ran (an item: 16 bytes of each
     array when both are 16-byte aligned and n is a multiple of 16 / sizeof(sample), else one
     element); the rest of ``out`` is untouched.  Mode 0 starts a record; mode 1 CONTINUES the record
     already at ``out + 0``: it is folded in first, then the partials in index order, so a caller walks a
     large array slab by slab with one read-back and no host combine.  Every word but the float32
     sum is the same on every device and in any order; the float32 sum is a fixed tree (lanes, waves,
     workgroups in index order): the same buffers, count and alignment give the same 64 bits on every
     call.  Two launches on ``stream``, no atomics.  KMP_ERR_ARG, with nothing launched: a NULL pred
     (whatever the count), KMP_DECODE, a mode field other than 0 / 1, differing or unsupported dtypes, a
     misaligned ``out``, 16-bit samples with n >= 2^32 (the u64 sum could overflow), or this code on
     any other entry point.  kmp_last_launch() names it "compare". */
  KMP_CODER_COMPARE = 10,
  /* Hold-fill of a quantiser's marked output (kmp_code alone, KMP_ENCODE alone).  ``x`` is
     an int16 / int32 array (``x_dtype`` KMP_I16 / KMP_I32) in which the type's minimum MARKS an element,
     as the quantisers' ENCODE writes it; ``out`` is the array of the same dtype and count in which every
     marked element holds the last unmarked value before it in index order, the marked elements before
     the first unmarked one hold that first value, an array with no unmarked element is all 0, and
     every unmarked element is unchanged.  ``out`` may be ``x`` itself (a lane reads the 8 elements it
     writes before it writes them, and nothing else reads them); any other overlap of the two arrays is
     refused.  ``pred`` is the scratch: a device buffer of KMP_FILL_BYTES, 8-byte aligned, non-NULL whatever
     the count; its contents on entry do not matter and ``pred_dtype`` is not read.  Workgroup g of
     ceil(T / P), T = ceil(n / KMP_FILL_TILE), P = ceil(T / KMP_FILL_GROUPS), owns the elements
     [g P KMP_FILL_TILE, (g + 1) P KMP_FILL_TILE): a function of n alone.  Both arrays 16-byte
     aligned: 16-byte non-temporal accesses; any other alignment (the dtype's at least): element accesses.
     Three launches on ``stream``, no atomics; the same buffers give the same bytes on every call.
     KMP_ERR_ARG, with nothing launched: KMP_DECODE, another x_dtype, a non-zero field above the low byte, a
     NULL or misaligned ``pred``, arrays not aligned to their dtype, partly overlapping arrays, or this
     code on any other entry point.  n == 0 is KMP_OK and touches nothing.  kmp_last_launch() names
     it "fill". */
  KMP_CODER_FILL = 11,
  /* Patch of a float32 array from a run table (kmp_code alone, KMP_DECODE alone).  ``x`` is
     the table on the device: n = R records of four uint32 -- the low and the high word of ``start``,
     ``length``, ``bits`` --, 16-byte aligned, ``x_dtype`` KMP_U32; ``out`` is the float32 array, 4-byte
     aligned, patched in place: ``bits`` is written over the elements [start, start + length) of every
     record and nothing else is touched.  ``pred`` must be NULL.  The bounds are the CALLER's duty: the
     kernel does not know the array's size, so every [start, start + length) must lie inside it (the
     Python layer checks the extents on the device, with one read-back, before the launch); records
     must not overlap.  A record of any length is served, but a wave owns 64 consecutive records and
     walks the long ones among them (more than 8 elements) one after the other: cut long runs into records
     of at most KMP_RUNS_PIECE elements when the table is built, so that a long run spreads over one wave per
     64 records.  KMP_ERR_ARG, with nothing launched:
     KMP_ENCODE, another x_dtype, a non-zero field above the low byte, a non-NULL ``pred``, a misaligned
     table or array, or this code on any other entry point.  R == 0 is KMP_OK.  One launch;
     kmp_last_launch() names it "runs". */
  KMP_CODER_RUNS = 12,
  /* Delta of two integer arrays modulo 2^W (kmp_code alone): the step of time-series coding
     along the batch axis.  ``x`` and ``pred`` (non-NULL whatever the count) are arrays of ``x_dtype`` ==
     ``pred_dtype``, one of KMP_U8, KMP_I8, KMP_U16, KMP_I16, KMP_I32, W its width; ``out`` has the same dtype
     and count.  ENCODE writes out[i] = (x[i] - pred[i]) mod 2^W, DECODE out[i] = (x[i] + pred[i]) mod 2^W:
     signed and unsigned samples of one width give the same bits.  ``out`` may be ``x`` itself (a lane loads
     what it stores before it stores it); any other overlap of ``out`` with ``x``, and any overlap of ``out``
     with ``pred``, is refused.  All three pointers 16-byte aligned and n a multiple of 16 / sizeof(sample):
     16-byte non-temporal accesses; anything else (the dtype's alignment at least): element accesses.  One
     launch on ``stream``, no atomics, no LDS, no workspace; the same buffers give the same bytes on every call.
     A sequence of T frames of F samples: the encode of every frame against the one before it is ONE call
     (x = n + F, pred = n, count (T - 1) F, out of place); the decode is one call per frame, in order,
     ``pred`` the frame just restored.  KMP_ERR_ARG, with nothing launched: a NULL ``pred`` (whatever the
     count), a non-zero field above the low byte, differing or other dtypes, a direction other than
     KMP_ENCODE / KMP_DECODE, arrays not aligned to their dtype, a refused overlap, or this code on any
     other entry point.  n == 0 is KMP_OK and touches nothing.  kmp_last_launch() names it "delta". */
  KMP_CODER_DELTA = 13,
  /* Structural similarity of a restored array against its original (kmp_code alone, KMP_ENCODE alone;
     DESIGN.md §23).  It codes nothing: ``x`` is the original, ``pred`` the restored array (non-NULL), both of
     ``x_dtype`` == ``pred_dtype``, one of KMP_F32, KMP_U8, KMP_U16, KMP_I8, KMP_I16; n = N D H W samples, N items of
     D x H x W (D == 1: images); ``out`` an 8-byte aligned device buffer of KMP_SSIM_BYTES.  kmp_code carries one
     count, so the geometry travels in ``out``: before the call ``out + 64`` holds the REQUEST, eight 64-bit words
     that the kernels only read:
       0, 1, 2  D, H, W (int64)       3, 4  C1, C2 (f64 bits)       5  base (f64 bits)       6, 7  0
     Windows: side 7, uniform weights, NP = 49 samples (D == 1) or 343; only the windows that lie wholly inside
     one item are counted, (D - 6)(H - 6)(W - 6) per item ((H - 6)(W - 6) for images), no padding.  Samples:
     integers enter as unsigned (int8 / int16 through v ^ signbit), float32 as (double)v - base; a float32
     window is SKIPPED iff one of its NP positions holds a non-finite x or r.  Per counted window, with Sx, Sr,
     Sxx, Srr, Sxr the sums of x, r, x^2, r^2, x r over its samples (exact for integers), in float64:
       mx = Sx / NP, mr = Sr / NP, vx = (NP Sxx - Sx^2) / (NP (NP - 1)), vr, vxr alike,
       s = ((2 mx mr + C1)(2 vxr + C2)) / ((mx^2 + mr^2 + C1)(vx + vr + C2)).
     A RECORD is eight 64-bit words:
       0  windows counted (u64)             1  windows skipped (u64)
       2  sum of s over the counted windows (f64 bits)
       3  their minimum (f64 bits; +inf when there are none)
       4  status: 0, or 1 for a malformed request, with nothing counted
       5, 6, 7  0
     After the call ``out + 0`` holds the record and ``out + 64 (2 + g)`` the partial record of workgroup g for the
     min(KMP_SSIM_GROUPS, ceil(n / (KMP_SSIM_TILE_H KMP_SSIM_TILE_W))) workgroups that ran; the request and the rest
     of ``out`` are untouched.  A workgroup owns KMP_SSIM_TILE_H x KMP_SSIM_TILE_W window origins of one item over
     KMP_SSIM_TILE_D origins along D.  The kernel checks the request: D == 1 or D >= 7; H, W >= 7; D H W divides n
     (without overflow); C1, C2 finite and > 0; base finite -- a request that fails gives status 1 and zero
     counts, and no sample is read.  Both arrays 16-byte aligned and W a multiple of 16 / sizeof(sample):
     16-byte reads; anything else: element reads.  Every window's moments are sums of its own terms in one
     fixed grouping, the windows are summed in a fixed tree (lanes, waves, workgroups in index order): the
     same buffers and count give the same 64 bits on every call.  Two launches on ``stream``, no atomics.
     KMP_ERR_ARG, with nothing launched: a NULL pred (whatever the count), KMP_DECODE, a non-zero field above
     the low byte, differing or unsupported dtypes, a misaligned ``out``, NULL x or out with n > 0, arrays not
     aligned to their dtype, or this code on any other entry point.  n == 0 is KMP_OK and touches nothing.  kmp_last_launch() names it
     "ssim". */
  KMP_CODER_SSIM = 14
} kmp_coder;
#define KMP_CODER_NEAR(code, max_error) ((code) | ((max_error) << 8))
#define KMP_CODER_QUANT(code, exp) ((code) | (((exp) + 127) << 8))
#define KMP_CODER_PREC(code, m) ((code) | (((m) + 1) << 8))
#define KMP_CODER_COMPARE_MODE(cont) (KMP_CODER_COMPARE | ((cont) << 8))
#define KMP_COMPARE_GROUPS 1024
#define KMP_COMPARE_BYTES (64 * (1 + KMP_COMPARE_GROUPS))
#define KMP_FILL_TILE 2048
#define KMP_FILL_GROUPS 1024
#define KMP_FILL_BYTES (16 * KMP_FILL_GROUPS)
#define KMP_RUNS_PIECE 256
#define KMP_SSIM_GROUPS 1024
#define KMP_SSIM_BYTES (64 * (2 + KMP_SSIM_GROUPS))
#define KMP_SSIM_TILE_D 32
#define KMP_SSIM_TILE_H 16
#define KMP_SSIM_TILE_W 16
typedef enum { KMP_ENCODE = 0, KMP_DECODE = 1 } kmp_direction;

typedef enum {
  /* mean of the (2p+2)^d lowres neighbourhood, cast to the dtype, broadcast to all channels:
     the reference test predictor, tests/volume/test_encode_decode.py:43-55 */
  KMP_PRED_MEAN = 0,
  /* pred[k] = sum_n feat[n] * W[n, k] + b[k] in float32 (MFMA), cast to the dtype
     (build-defined; fills the reference's predictions_fn slot, volume/encode_decode.py:48) */
  KMP_PRED_LINEAR = 1,
  /* the same predictor on the matrix cores: bf16x2 split of features and weights, one
     v_mfma_f32_16x16x32_bf16 per chunk of 8 features (kmp_bf16x2.h); within the north star's 1e-5
     of the f64 value rather than bit-equal to the f32 fma chain; uint8 / uint16 samples (a signed
     dtype with this kind is KMP_ERR_ARG: signed samples take KMP_PRED_LINEAR) */
  KMP_PRED_LINEAR_MFMA = 2,
} kmp_predictor_kind;

typedef struct {
  int32_t kind;         /* kmp_predictor_kind */
  int32_t padding;      /* neighbourhood padding p >= 0 */
  const float* weights; /* LINEAR: device [N, K] row-major, N = (2p+2)^d, K = 19 (3D) / 5 (2D) */
  const float* bias;    /* LINEAR: device [K] */
} kmp_predictor;

/* Sub-box of the output frame [0, E) per spatial axis (z, y, x; 2D uses y, x).  NULL = all.
   Used by the chunked drivers (encode_decode_chunk.py:77-117): a launch writes exactly the
   outputs whose block coordinate lies in the box. */
typedef struct {
  int64_t begin[3];
  int64_t end[3];
} kmp_region;

/* ---------------------------------------------------------------------------------------- */
/* Library                                                                                   */
/* ---------------------------------------------------------------------------------------- */
const char* kmp_version(void);
const char* kmp_last_error(void);
/* Name of the last kernel family this thread launched (e.g. "wave3d_encode", "fast3d_decode",
   "generic_encode"): lets tests and callers see which code path served a call. */
const char* kmp_last_launch(void);
/* 1 if the kernels were built for the device's ISA (gfx950) and a device is visible. */
int kmp_device_ok(void);

/* Process-wide dispatch options: switches to a fallback kernel family, the
   encode store policy, the block order.  Each starts from the environment variable of the same
   name, read once when the library loads; launches read the table, never the environment.
   ``kmp_set_option(name, value)`` sets one (KMP_ERR_ARG for an unknown name);
   ``kmp_clear_option`` returns it to the kernel's own default; ``kmp_get_option`` returns 1 and
   the value when set, 0 when unset, KMP_ERR_ARG for an unknown name.  Not part of the
   reference (which has no such switches); no production use needs them. */
int kmp_set_option(const char* name, int value);
int kmp_clear_option(const char* name);
int kmp_get_option(const char* name, int* value);

/* Device address of pinned (page-locked, device-mapped) host memory, for zero-copy streaming:
   the fused kernels then read the input from / write the outputs to host memory over the host
   link directly (kompressor_amd.stream, the reference's host-resident arrays,
   volume/encode_decode.py:30-85).  KMP_ERR_UNSUPPORTED if ``host`` is not such memory. */
int kmp_host_device_pointer(void* host, void** device);

/* ---------------------------------------------------------------------------------------- */
/* Fused encode / decode (one pass over HBM each).                                           */
/* ---------------------------------------------------------------------------------------- */

/* Replaces volume/encode_decode.py:30-56 ``encode`` for a built-in predictor and coder:
   pad_highres -> lowres_from_highres -> maps_from_highres -> predictor ->
   maps_from_predictions -> encode_fn per map -> trim.  ``highres`` [B, D, H, W, C] of
   ``dtype``; writes ``lowres_out`` [B, Ed, Eh, Ew, C] (dtype) and ``maps_out[7]`` in
   LR, UD, FB, C, Z, Y, X order with trimmed shapes (volume/utils.py:270-276) in the coder's
   dtype (RAW -> int32).  ``dims_out[3]`` receives the even-dim padding.  ``workspace`` must
   hold ``kmp_volume_workspace_bytes`` bytes (may be NULL when that is 0). */
int kmp_volume_encode(int32_t dtype, const void* highres, int64_t B, int64_t D, int64_t H, int64_t W,
                      int64_t C, const kmp_predictor* predictor, int32_t coder, void* lowres_out,
                      void* const maps_out[7], int32_t dims_out[3], const kmp_region* region,
                      void* workspace, size_t workspace_bytes, kmp_stream_t stream);

/* Replaces volume/encode_decode.py:59-85 ``decode``: pad_lowres/pad_maps -> predictor ->
   decode_fn per map -> highres_from_lowres_and_maps -> trim.  ``lowres`` [B, Ed, Eh, Ew, C],
   ``maps[7]`` as produced by kmp_volume_encode, ``dims[3]`` the even padding; writes
   ``highres_out`` [B, 2Ed-1+dd, 2Eh-1+dh, 2Ew-1+dw, C]. */
int kmp_volume_decode(int32_t dtype, const void* lowres, const void* const maps[7], int64_t B,
                      int64_t Ed, int64_t Eh, int64_t Ew, int64_t C, const int32_t dims[3],
                      const kmp_predictor* predictor, int32_t coder, void* highres_out,
                      const kmp_region* region, void* workspace, size_t workspace_bytes,
                      kmp_stream_t stream);

/* Bytes of device workspace the fused calls need for this shape/predictor (0 on the fast path). */
int64_t kmp_volume_workspace_bytes(int32_t dtype, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                                   const kmp_predictor* predictor);

/* 2D analogues: image/encode_decode.py:30-85; maps_out[3] in LR, UD, C order. */
int kmp_image_encode(int32_t dtype, const void* highres, int64_t B, int64_t H, int64_t W, int64_t C,
                     const kmp_predictor* predictor, int32_t coder, void* lowres_out,
                     void* const maps_out[3], int32_t dims_out[2], const kmp_region* region,
                     void* workspace, size_t workspace_bytes, kmp_stream_t stream);
int kmp_image_decode(int32_t dtype, const void* lowres, const void* const maps[3], int64_t B, int64_t Eh,
                     int64_t Ew, int64_t C, const int32_t dims[2], const kmp_predictor* predictor,
                     int32_t coder, void* highres_out, const kmp_region* region, void* workspace,
                     size_t workspace_bytes, kmp_stream_t stream);
int64_t kmp_image_workspace_bytes(int32_t dtype, int64_t B, int64_t H, int64_t W, int64_t C,
                                  const kmp_predictor* predictor);

/* ---------------------------------------------------------------------------------------- */
/* Primitives (the geometry API re-exported by volume/__init__.py:31-35, image/__init__.py)  */
/* ``nsp`` = number of spatial axes (2 = image, 3 = volume); ``shape`` holds them z,y,x      */
/* (image: y,x).                                                                            */
/* ---------------------------------------------------------------------------------------- */

/* volume/utils.py:77-80, image/utils.py:52-55: out = in[:, ::2, ::2(, ::2)] */
int kmp_lowres_from_highres(int32_t nsp, int32_t dtype, const void* in, int64_t B, const int64_t shape[3],
                            int64_t C, void* out, kmp_stream_t stream);

/* volume/utils.py:158-171, image/utils.py:89-96: the 7 (3) parity-class maps, untrimmed. */
int kmp_maps_from_highres(int32_t nsp, int32_t dtype, const void* in, int64_t B, const int64_t shape[3],
                          int64_t C, void* const out[7], kmp_stream_t stream);

/* volume/utils.py:37-74, image/utils.py:37-49: [B, cells..., 19 (5), C] training targets. */
int kmp_targets_from_highres(int32_t nsp, int32_t dtype, const void* in, int64_t B, const int64_t shape[3],
                             int64_t C, void* out, kmp_stream_t stream);

/* volume/utils.py:174-195, image/utils.py:99-116: interleave lowres [B, L..., C] and the
   7 (3) maps (shapes as maps_from_highres of a (2L-1)^d grid) into [B, 2L-1..., C]. */
int kmp_highres_from_lowres_and_maps(int32_t nsp, int32_t dtype, const void* lowres, const void* const maps[7],
                                     int64_t B, const int64_t lshape[3], int64_t C, void* out,
                                     kmp_stream_t stream);

/* volume/utils.py:199-210, image/utils.py:120-129: stack of the (2p+2)^d shifted windows of
   an already padded lowres [B, S..., C] -> [B, S-2p-1..., N, C]. */
int kmp_features_from_lowres(int32_t nsp, int32_t dtype, const void* lowres, int64_t B, const int64_t shape[3],
                             int64_t C, int32_t padding, void* out, kmp_stream_t stream);

/* volume/utils.py:83-155, image/utils.py:58-86: float32 aggregation of [B, cells..., K, C]
   predictions (K = 19 / 5) onto the 7 (3) maps, normalised, cast back to dtype. */
int kmp_maps_from_predictions(int32_t nsp, int32_t dtype, const void* preds, int64_t B, const int64_t cells[3],
                              int64_t C, void* const out[7], kmp_stream_t stream);

/* Mean predictor applied to a padded lowres window (the reference test predictor, as used by
   predictions_fn): == maps_from_predictions(repeat(mean(features_from_lowres(x, p)))) */
int kmp_mean_predict_maps(int32_t nsp, int32_t dtype, const void* padded_lowres, int64_t B,
                          const int64_t shape[3], int64_t C, int32_t padding, void* const out[7],
                          kmp_stream_t stream);

/* The same maps written as ``out_dtype``: the sample dtype, or KMP_F32 -- the values a
   float32-emitting predictions_fn (a network, volume/encode_decode.py:48) hands the coder; 3D,
   C == 1 windows only (else KMP_ERR_UNSUPPORTED). */
int kmp_mean_predict_maps_typed(int32_t nsp, int32_t dtype, int32_t out_dtype, const void* padded_lowres,
                                int64_t B, const int64_t shape[3], int64_t C, int32_t padding,
                                void* const out[7], kmp_stream_t stream);

/* Linear predictor on a padded lowres window: per-cell [B, cells..., K, C] predictions in the
   dtype (MFMA f32), optionally also the f32 pre-cast values (``preds_f32`` may be NULL).
   KMP_I8 / KMP_I16: the features are M(window), the chain's value is cast in the mapped domain
   (truncate, saturate to [0, 2^W - 1], NaN -> 0) and stored as M^-1 of it; ``preds_f32`` holds the
   chain's own (mapped-domain) values. */
int kmp_linear_predict(int32_t nsp, int32_t dtype, const void* padded_lowres, int64_t B, const int64_t shape[3],
                       int64_t C, int32_t padding, const float* weights, const float* bias, void* preds_out,
                       float* preds_f32, kmp_stream_t stream);
/* the same for KMP_PRED_LINEAR_MFMA (kmp_bf16x2.h): the matrix-core arithmetic every fused kernel of
   that kind reproduces bit for bit; uint8 / uint16 samples */
int kmp_linear_predict_mfma(int32_t nsp, int32_t dtype, const void* padded_lowres, int64_t B, const int64_t shape[3],
                            int64_t C, int32_t padding, const float* weights, const float* bias, void* preds_out,
                            float* preds_f32, kmp_stream_t stream);

/* Exact second moments for a least-squares fit of the linear predictor: M = X^T X [Q, Q] int64
   (row-major, overwritten), one row of X per cell of the UNPADDED highres [B, shape..., 1]:
     X = [ features_from_lowres(pad_neighborhood(lowres_from_highres(pad_highres(h)), p), p)  (N columns),
           targets_from_highres(pad_highres(h))                                             (K = 19 / 5),
           1 ],   Q = N + K + 1
   (volume/utils.py:37-74,199-218,226-237; image/utils.py:38-49,121-137,146-156) -- the cells and
   feature windows ``encode`` evaluates the predictor on.  uint8 / uint16 samples, C == 1, volumes
   with padding 0 or 1, images with padding 0, 1 or 2 (else KMP_ERR_UNSUPPORTED); at most 2^31 - 1
   cells per call (else KMP_ERR_ARG; moments add, so split the batch).  ``workspace`` holds
   kmp_linear_moments_workspace_bytes() bytes (0 for an unsupported configuration), 8-byte aligned. */
size_t kmp_linear_moments_workspace_bytes(int32_t nsp, int32_t dtype, int32_t padding);
int kmp_linear_moments(int32_t nsp, int32_t dtype, const void* highres, int64_t B, const int64_t shape[3],
                       int64_t C, int32_t padding, int64_t* moments, void* workspace, kmp_stream_t stream);

/* jnp.pad on the spatial axes (volume/utils.py:213-260, image/utils.py:132-178):
   mode 0 = 'symmetric', 1 = 'reflect'.  Negative pads crop (== trim, volume/utils.py:263-276). */
int kmp_pad(int32_t nsp, int32_t dtype, const void* in, int64_t B, const int64_t shape[3], int64_t C,
            const int64_t pad_lo[3], const int64_t pad_hi[3], int32_t mode, void* out, kmp_stream_t stream);

/* Box copy with dtype conversion -- the slicing and ``.at[box].set`` steps of the chunked
   driver (volume/encode_decode_chunk.py:101-115): for o in [0, ext) per spatial axis,
   out[b, out_off + o, c] = cast(in[b, in_off + o, c]).  Integer narrowing wraps; float -> int is
   the XLA truncating cast. */
int kmp_copy_box(int32_t nsp, int32_t in_dtype, const void* in, const int64_t in_shape[3], const int64_t in_off[3],
                 int32_t out_dtype, void* out, const int64_t out_shape[3], const int64_t out_off[3], int64_t B,
                 int64_t C, const int64_t ext[3], kmp_stream_t stream);

/* Tile split / reassembly for the batched metric workload (BASELINE configs C3/C4): the
   reference codes a batch of independent arrays along its leading axis (every primitive is
   [:, ...]-parallel, volume/utils.py:80,161-169); this turns ONE volume [D, H, W, C] (image
   [H, W, C]) into the batch [n, Tz, Ty, Tx, C] of its tiles in z-major tile order
   (direction 0) and back (direction 1).  Every extent must be a multiple of the tile's. */
int kmp_tiles(int32_t nsp, int32_t dtype, int32_t direction, const void* src, const int64_t shape[3], int64_t C,
              const int64_t tile[3], void* dst, kmp_stream_t stream);

/* Residual coders utils.py:28-55 on n elements.  ``pred_dtype``/``x_dtype`` are the operand
   dtypes (x = gt for ENCODE, encoded for DECODE); the output is uint8 / uint16 / int32 /
   uint32 for KMP_CODER_U8 / U16 / RAW / U32.  KMP_I8 / KMP_I16 operands with KMP_CODER_U8 / U16:
   (gt - pred) mod 2^W of the signed values -- the same bits as the unsigned codes give, the sign
   map cancels in the difference; a decode's output holds the signed sample's bit pattern.
   Near coders (KMP_CODER_NEAR): ``x_dtype`` is the SAMPLE dtype in both directions -- KMP_U8 / KMP_U16 /
   KMP_I8 / KMP_I16; a decode's residuals are the unsigned W-bit map, labelled with the samples' code,
   which says whether they are signed -- and ``pred_dtype`` is that dtype or KMP_F32 (truncated, then
   clamped to the sample type's range).  The output is the unsigned map (encode) or the samples'
   bit patterns (decode).
   Quantisers (KMP_CODER_QUANT and KMP_CODER_PREC, see kmp_coder): ``pred`` is NULL; float32 ->
   int16 / int32 (ENCODE), int16 / int32 -> float32 (DECODE).
   KMP_CODER_COMPARE (see kmp_coder): ``x`` the original, ``pred`` the restored array of the same dtype,
   ``out`` the KMP_COMPARE_BYTES of the error statistics; ENCODE alone.
   KMP_CODER_FILL (see kmp_coder): ``x`` the marked int16 / int32 array, ``out`` the filled one, ``pred`` the
   KMP_FILL_BYTES of scratch; ENCODE alone.  KMP_CODER_RUNS (see kmp_coder): ``x`` the run table (n records),
   ``out`` the float32 array patched in place, ``pred`` NULL; DECODE alone.
   KMP_CODER_DELTA (see kmp_coder): ``x`` and ``pred`` two integer arrays of one dtype, ``out`` their
   difference (ENCODE) or sum (DECODE) modulo 2^W in that dtype.
   KMP_CODER_SSIM (see kmp_coder): ``x`` the original, ``pred`` the restored array of the same dtype, ``out`` the
   KMP_SSIM_BYTES that hold the request on entry and the record after; ENCODE alone. */
int kmp_code(int32_t direction, int32_t coder, int32_t pred_dtype, const void* pred, int32_t x_dtype,
             const void* x, int64_t n, void* out, kmp_stream_t stream);

/* ---------------------------------------------------------------------------------------- */
/* Callback path: an opaque predictions_fn with a built-in coder (kmp_callback.hip).  The    */
/* reference's steps on either side of the callback, fused; results identical to them.      */
/* ---------------------------------------------------------------------------------------- */

/* pad_neighborhood(lowres_from_highres(pad_highres(h)), p) (volume/encode_decode.py:36-48):
   the window encode hands predictions_fn, [B, L+2p..., C], straight from the highres. */
int kmp_window_from_highres(int32_t nsp, int32_t dtype, const void* highres, int64_t B, const int64_t shape[3],
                            int64_t C, int32_t padding, void* window_out, kmp_stream_t stream);

/* pad_neighborhood(pad_lowres(lowres, dims), p) (volume/encode_decode.py:70-76): the window
   decode hands predictions_fn, from the trimmed lowres [B, E..., C]. */
int kmp_window_from_lowres(int32_t nsp, int32_t dtype, const void* lowres, int64_t B, const int64_t shape[3],
                           int64_t C, const int32_t dims[3], int32_t padding, void* window_out, kmp_stream_t stream);

/* trim(lowres) and trim_maps([encode_fn(p, g) for p, g in zip(preds, maps_from_highres(
   pad_highres(h)))]) (volume/encode_decode.py:49-56) with encode_fn the built-in coder of the
   dtype: ``preds`` are predictions_fn's 7 (3) untrimmed maps in the sample dtype. */
int kmp_encode_with_predictions(int32_t nsp, int32_t dtype, int32_t coder, const void* highres, int64_t B,
                                const int64_t shape[3], int64_t C, const void* const preds[7], void* lowres_out,
                                void* const maps_out[7], kmp_stream_t stream);

/* trim(highres_from_lowres_and_maps(pad_lowres(lowres), [decode_fn(p, e) for p, e in
   zip(preds, pad_maps(maps))])) (volume/encode_decode.py:77-85), built-in decode_fn. */
int kmp_decode_with_predictions(int32_t nsp, int32_t dtype, int32_t coder, const void* lowres,
                                const void* const maps[7], int64_t B, const int64_t shape[3], int64_t C,
                                const int32_t dims[3], const void* const preds[7], void* highres_out,
                                kmp_stream_t stream);

/* The two above with the prediction maps' dtype given separately: ``pred_dtype`` is the sample
   dtype or KMP_F32 -- a network's float32 output, which the reference's coders read as
   jnp.int32(pred) (truncating; out-of-range saturates here), utils.py:28-55.  All four take the near
   coders too (``coder`` = KMP_CODER_NEAR of the dtype's width): the lowres passes through, the maps
   hold the quantised residuals, and a decode returns samples within max_error of the coded ones. */
int kmp_encode_with_predictions_typed(int32_t nsp, int32_t dtype, int32_t coder, int32_t pred_dtype,
                                      const void* highres, int64_t B, const int64_t shape[3], int64_t C,
                                      const void* const preds[7], void* lowres_out, void* const maps_out[7],
                                      kmp_stream_t stream);
int kmp_decode_with_predictions_typed(int32_t nsp, int32_t dtype, int32_t coder, int32_t pred_dtype,
                                      const void* lowres, const void* const maps[7], int64_t B, const int64_t shape[3],
                                      int64_t C, const int32_t dims[3], const void* const preds[7], void* highres_out,
                                      kmp_stream_t stream);

/* ---------------------------------------------------------------------------------------- */
/* Bit-plane container payload (kmp_pack.hip; SURVEY.md §8f f-3 -- no reference counterpart, */
/* the reference returns the residual arrays unreduced, volume/encode_decode.py:56; format    */
/* spec: oracle/packing.py).  n samples of ``dtype`` (8/16/32-bit), zigzag-mapped, blocks of 64 */
/* stored as width 64-bit bit-planes.  ``workspace`` holds kmp_pack_workspace_bytes(n) bytes.  */
/* ---------------------------------------------------------------------------------------- */
int64_t kmp_pack_blocks(int64_t n);
int64_t kmp_pack_workspace_bytes(int64_t n);
/* byte offset in the workspace of the uint64 payload length (in 64-bit words) the plan writes */
int64_t kmp_pack_total_offset(int64_t n);
/* widths[nblocks] of x, and the block offsets + total payload words into the workspace */
int kmp_pack_plan(int32_t dtype, const void* x, int64_t n, uint8_t* widths, void* workspace, kmp_stream_t stream);
/* the payload (8-byte aligned) of x, after kmp_pack_plan on the same workspace */
int kmp_pack(int32_t dtype, const void* x, int64_t n, const uint8_t* widths, const void* workspace,
             uint64_t* payload, kmp_stream_t stream);
/* block offsets from stored widths, then the samples */
/* container header bytes written by a kernel (no host copy): dst[0:len) = bytes (len <= 128),  */
/* dst[zero_from:zero_to) = 0, and, when words_at >= 0, the u64 payload word count of the last    */
/* kmp_pack_plan on ``workspace`` (n samples) at dst + words_at -- stream-ordered after the plan */
int kmp_pack_header(uint8_t* dst, const uint8_t* bytes, int32_t len, int64_t zero_from, int64_t zero_to,
                    const void* workspace, int64_t n, int64_t words_at, kmp_stream_t stream);
int kmp_unpack_plan(const uint8_t* widths, int64_t n, void* workspace, kmp_stream_t stream);
int kmp_unpack(int32_t dtype, const uint64_t* payload, int64_t n, const uint8_t* widths, const void* workspace,
               void* out, kmp_stream_t stream);

/* ---------------------------------------------------------------------------------------- */
/* Block-adaptive Rice entropy coding of coded maps, bundle format v2 (kmp_rice.hip; SURVEY.md  */
/* §8f f-3 -- no reference counterpart, volume/encode_decode.py:56 returns the residuals         */
/* unreduced; byte layout spec: oracle/rice.py pack_bundle).  n samples of ``dtype`` (8/16/32-bit), */
/* zigzag-mapped, blocks of 64: params[b] = Rice k + 1 (0 = all-zero block), bw[b] = the block's  */
/* 32-bit payload words; tiles of 256 blocks.  All arrays of a bundle share ONE payload region in  */
/* tile order; each array keeps a u64 table of its tiles' word offsets into it.                  */
/* ---------------------------------------------------------------------------------------- */
typedef struct kmp_rice_array {
  const void* samples; /* encode: the input samples; decode: the output samples (written)      */
  int64_t n;           /* samples                                                                */
  int64_t side_off;    /* byte offset in the bundle of params[nb]; bw[nb] at side_off + pad8(nb)  */
  int64_t toff_off;    /* byte offset of the u64 tile offsets [kmp_rice_tiles(n)] (8-aligned)    */
  int64_t rec_off;     /* byte offset of the array's {u64 first word, u64 end word} (8-aligned)  */
} kmp_rice_array;
/* tiles of 256 blocks of 64 samples: ceil(ceil(n / 64) / 256) */
int64_t kmp_rice_tiles(int64_t n);
/* workspace of the single-pass encode: the look-back states of tiles_total tiles + a ticket */
int64_t kmp_rice_bundle_workspace_bytes(int64_t tiles_total);
/* one launch for ``count`` (<= 32) arrays of one dtype, whose tiles are global tiles           */
/* tile_begin .. + their count of the bundle's ``tiles_total``: samples read once, side          */
/* information / tile offsets / records / payload written into ``bundle`` (payload region at    */
/* byte payload_off); the tile of global index tiles_total - 1 writes the bundle's payload words */
/* (u64 at byte 56) and byte size (u64 at byte 64).  Calls for one bundle go in tile order on    */
/* one stream (replaces round 2's kmp_rice_plan / kmp_rice_pack and their two scan launches).   */
/* Capacity: ``bundle`` (8-byte aligned) holds at least payload_off + worst bytes, worst = the sum */
/* over all arrays of the bundle of ceil(n / 64) * (2 W + 2) * 4 (a block codes into at most       */
/* 2 W + 2 words, W the sample bits).  The caller writes the header [0, 80 + 128 * arrays); the    */
/* launches write the rest up to the byte size ``total`` they store at byte 64, total <=           */
/* payload_off + worst, and no byte at or past ``total`` (tests/test_gpu_guard_packing.py).        */
/* MEASURING MODE, ``bundle == NULL``: the size of the bundle without producing it.  Same arrays,  */
/* count, tile_begin, tiles_total, workspace and stream; payload_off and the records' side_off /   */
/* toff_off / rec_off are ignored.  The call with tile_begin == 0 clears the u64 at workspace + 0; */
/* every call adds the payload words of its tiles to it, so after the bundle's last call it holds  */
/* exactly the payload words the encode stores at byte 56 (the bundle is then payload_off +        */
/* pad8(4 * words) bytes).  The samples are read once; nothing else is written, nothing allocated, */
/* no synchronisation (graph-capturable); a call without tiles returns KMP_OK after the clear.     */
/* kmp_last_launch() names it "rice_bundle_measure" (tests/test_gpu_guard_measure.py).             */
int kmp_rice_bundle_encode(int32_t dtype, const kmp_rice_array* arrays, int32_t count, int64_t tile_begin,
                           int64_t tiles_total, uint8_t* bundle, int64_t payload_off, void* workspace,
                           kmp_stream_t stream);
/* the inverse into each array's ``samples``: no scan launch (tile offsets from the table); side */
/* information checked in the same pass -- every read stays inside the tile's / payload's        */
/* extent, inconsistent tiles decode as zeros and add 1 to *bad (caller-zeroed device uint64)   */
/* (replaces round 2's kmp_unpack_plan + kmp_unpack_check + kmp_rice_unpack)                    */
int kmp_rice_bundle_decode(int32_t dtype, const kmp_rice_array* arrays, int32_t count, int64_t tile_begin,
                           const uint8_t* bundle, int64_t payload_off, uint64_t payload_words,
                           unsigned long long* bad, kmp_stream_t stream);

/* Decode of SAMPLE RANGES of bundle arrays (extends kmp_rice_bundle_decode, which always decodes  */
/* whole arrays from a whole resident bundle; no reference counterpart, as above).  One record   */
/* decodes samples [first, end) of one array; its tiles T0 = first / 16384 .. T1 = (end - 1) /    */
/* 16384 are the only ones read.  The side information, the tile table and the payload are       */
/* separate device pointers, so each may point into a resident bundle or at a small WINDOW of a   */
/* bundle that is mostly not on the device (a partial file read):                                */
typedef struct kmp_rice_range {
  void* samples;           /* out: samples[i - first] = sample i of the array, first <= i < end;  */
                           /* no other byte is written                                             */
  int64_t n;               /* samples of the whole array (fixes the block count, the short last   */
                           /* block)                                                               */
  int64_t first, end;      /* 0 <= first < end <= n                                                */
  const uint8_t* params;   /* params / bw from block 256 * T0 on, up to block                     */
  const uint8_t* bw;       /* min(ceil(n / 64), 256 * (T1 + 1)) - 1                               */
  const uint64_t* toff;    /* 8-aligned: the word offsets of tiles T0 .. T1, then ONE closing     */
                           /* entry (the next tile's offset, or the array's end word after its   */
                           /* last tile): T1 - T0 + 2 entries                                      */
  const uint32_t* payload; /* 4-aligned: the payload from word ``payload_first`` on               */
  uint64_t payload_first;  /* the payload word payload[0] holds: 0 for a bundle's whole payload   */
                           /* region, toff[0] for a window cut at the first touched tile          */
  uint64_t payload_words;  /* words readable at ``payload``                                        */
} kmp_rice_range;
/* One launch for ``count`` (<= 32) records of one dtype; the grid is one workgroup per touched   */
/* tile.  Per touched tile the checks of kmp_rice_bundle_decode (k < W, bw within [2k + 2, 2W + 2], */
/* a zero block without payload, the tile's words meeting the closing offset, every read inside  */
/* [payload_first, payload_first + payload_words)); a tile that fails decodes as zeros and adds 1 */
/* to *bad (caller-zeroed device uint64).  That an array's first tile starts at its record's     */
/* first word is the caller's check (the record is not passed).  No allocation, no             */
/* synchronisation; graph-capturable.                                                            */
int kmp_rice_bundle_decode_ranges(int32_t dtype, const kmp_rice_range* ranges, int32_t count,
                                  unsigned long long* bad, kmp_stream_t stream);

/* CRC-32 (zlib / IEEE: reflected 0xEDB88320, init and final xor 0xFFFFFFFF; == zlib.crc32) of   */
/* ``data`` into the device uint32 *crc_out (kmp_crc.hip): the container file's integrity check    */
/* (container.py; the reference has no file format, volume/encode_decode.py:56   */
/* returns arrays in memory).  ``n_max`` bytes are covered, or -- when ``n_dev`` is a device       */
/* int64 -- min(*n_dev, n_max), the length read by the kernel (a bundle's size field, no host sync). */
/* ``data`` 16-byte aligned.  One memset of *crc_out + one launch.                               */
int kmp_crc32(const uint8_t* data, int64_t n_max, const int64_t* n_dev, uint32_t* crc_out, kmp_stream_t stream);

/* Per-tile CRC-32 of a v2 Rice bundle (kmp_crc.hip; no reference counterpart, as above): the      */
/* checksum at the granularity a partial read touches.  For tile t of an array of n samples, with  */
/* nbk = min(256, ceil(n / 64) - 256 t) blocks and payload words [toff[t], closing):               */
/*   tile_crc = zlib.crc32(params[256 t : 256 t + nbk] || bw[256 t : 256 t + nbk] || the payload   */
/*              words as little-endian bytes)                                                      */
/* (a tile without payload words: the CRC of its 2 nbk side bytes).  One record covers tiles       */
/* t0 .. t1 of one array; as in kmp_rice_range every piece is a device pointer of its own, into a  */
/* resident bundle or at a WINDOW read from a file:                                                */
typedef struct kmp_rice_crc_range {
  int64_t n;               /* samples of the whole array (fixes the last tile's block count)      */
  int64_t t0, t1;          /* 0 <= t0 <= t1 < kmp_rice_tiles(n)                                    */
  const uint8_t* params;   /* params / bw from block 256 * t0 on, up to block                     */
  const uint8_t* bw;       /* min(ceil(n / 64), 256 * (t1 + 1)) - 1                               */
  const uint64_t* toff;    /* 8-aligned: the word offsets of tiles t0 .. t1 (t1 - t0 + 1 entries) */
  const uint64_t* closing; /* 8-aligned: the word tile t1 ends at -- the next table entry, or the */
                           /* end-word field of the array's record inside the bundle (so a fresh  */
                           /* encode is checksummed without a copy or a host round trip)          */
  const uint32_t* payload; /* 4-aligned: the payload from word ``payload_first`` on               */
  uint64_t payload_first;  /* the payload word payload[0] holds                                    */
  uint64_t payload_words;  /* words readable at ``payload``                                        */
  uint32_t* crc_out;       /* write mode: crc_out[t - t0] = tile_crc(t); no other byte is written */
  const uint32_t* expect;  /* check mode (crc_out null): every tile whose CRC differs from        */
                           /* expect[t - t0] adds 1 to *bad                                        */
} kmp_rice_crc_range;
/* One launch for ``count`` (<= 32) records of any dtypes; a wave checksums one tile at a time and */
/* a workgroup walks several.  A tile whose span lies outside [payload_first, payload_first +     */
/* payload_words), runs backwards or exceeds 256 * (2 * 32 + 2) words is unusable: nothing is     */
/* read from it, it adds 1 to *bad (caller-zeroed device uint64; may be null in write mode) and   */
/* write mode stores 0.  No allocation, no synchronisation; graph-capturable.                     */
int kmp_rice_tile_crc(const kmp_rice_crc_range* ranges, int32_t count, unsigned long long* bad, kmp_stream_t stream);

/* Bit-plane side-information check (the planes format): count the blocks whose stored widths   */
/* no encoder produces (> W) -- format 0 -- or, format 1, Rice params / bw -- into the uint64 at  */
/* workspace + kmp_pack_total_offset(n) + 8, beside the payload length of the last scan          */
int kmp_unpack_check(int32_t format, int32_t dtype, const uint8_t* side_a, const uint8_t* side_b, int64_t n,
                     void* workspace, kmp_stream_t stream);

/* Categorical rank coder utils.py:58-111: ``logits`` float32 [n, L]; x/out of ``dtype`` [n]. */
int kmp_categorical(int32_t direction, const float* logits, int64_t n, int64_t L, int32_t dtype, const void* x,
                    void* out, kmp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KOMPRESSOR_HIP_H */

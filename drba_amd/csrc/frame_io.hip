// The frame source and sink of the pipeline: bilinear resize and the uint8 / uint16 <-> fp32 frame conversions used by
// to_inp / to_out.  Each conversion is written once, over a sample trait with two instances (bytes, 16-bit samples); the
// __global__ kernels keep one symbol per depth and form, because the launch trace and the profiles are keyed on them.
#include "common.hpp"

using namespace drba;

namespace {

// ---- frame source / sink (tools.py:33-38,59-72): bit-exact with ATen's CPU upsample_bilinear2d --------------------
// ATen evaluates the source coordinate as fma(scale, dst + 0.5, -0.5) and each 1-D interpolation as
// fma(w0, a, w1 * b) (its vectorised kernels are compiled with contraction; established by comparing every
// contraction variant against F.interpolate on the 480p/1080p/4K frame sizes: only this one matches in every bit).
// hipcc would pick its own contraction, so the operations are spelled out.
__device__ __forceinline__ Lerp lerp_src_aten(int dst, float scale, int size) {
  float s = __fmaf_rn(scale, (float)dst + 0.5f, -0.5f);
  if (s < 0.f) s = 0.f;
  Lerp l;
  l.i0 = min((int)s, size - 1);
  l.i1 = l.i0 + (l.i0 < size - 1 ? 1 : 0);
  l.w1 = __fsub_rn(s, (float)l.i0);
  l.w0 = __fsub_rn(1.f, l.w1);
  return l;
}
__device__ __forceinline__ float lerp2_aten(const Lerp &ly, const Lerp &lx, float a, float b, float c, float d) {
  const float top = __fmaf_rn(lx.w0, a, __fmul_rn(lx.w1, b));
  const float bot = __fmaf_rn(lx.w0, c, __fmul_rn(lx.w1, d));
  return __fmaf_rn(ly.w0, top, __fmul_rn(ly.w1, bot));
}

// ATen takes BOTH taps of an axis whose size does not change from the pixel itself, weights (1, 0) ("scale_factor = 1, simply
// copy"); lerp_src_aten's (x, x + 1) with the same weights gives the same value for finite data only: 1 * inf + 0 * inf is NaN,
// and the right neighbour's inf must not reach this pixel.  The 16-bit frames on the way out may hold anything, so they keep the
// rule (Samples16::kCopyTaps).
__device__ __forceinline__ Lerp lerp_src_aten_sized(int dst, float scale, int in_size, int out_size) {
  if (in_size == out_size) {
    Lerp l;
    l.i0 = l.i1 = dst;
    l.w0 = 1.f;
    l.w1 = 0.f;
    return l;
  }
  return lerp_src_aten(dst, scale, in_size);
}

// F.interpolate(bilinear, align_corners=False): out = wy0*(wx0*a + wx1*b) + wy1*(wx0*c + wx1*d)
// (ATen's separable evaluation order: innermost axis first).
__global__ void __launch_bounds__(256) resize_bilinear_kernel(const float *__restrict__ in, float *__restrict__ out, int NC, int Hin,
                                       int Win, int Hout, int Wout, float sy, float sx) {
  const size_t total = (size_t)NC * Hout * Wout;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % Wout);
    const int oy = (int)((i / Wout) % Hout);
    const int c = (int)(i / ((size_t)Wout * Hout));
    const Lerp ly = lerp_src_aten(oy, sy, Hin), lx = lerp_src_aten(ox, sx, Win);
    const float *p = in + (size_t)c * Hin * Win;
    const float *r0 = p + (size_t)ly.i0 * Win, *r1 = p + (size_t)ly.i1 * Win;
    out[i] = lerp2_aten(ly, lx, r0[lx.i0], r0[lx.i1], r1[lx.i0], r1[lx.i1]);
  }
}

// ---- the two sample kinds: everything in which a 16-bit kernel differs from its 8-bit sibling -------------------------------
// Bytes must equal the reference's: / 255. on the way in, trunc(x * 255.) with no clamp and its wrap-around on the way out
// (tools.py:37-38: (x*255.).astype(uint8), the x86 float -> int32 -> uint8 conversion numpy performs), plain lerp_src_aten taps.
struct Samples8 {
  typedef uint8_t sample_t;
  static constexpr bool kCopyTaps = false;
  __device__ __forceinline__ float to_unit(float v) const { return v / 255.f; }
  __device__ __forceinline__ float scale() const { return 255.f; }
  __device__ __forceinline__ uint32_t quantise(float scaled) const { return (uint32_t)(uint8_t)(int)scaled; }
  // four pixels of a row are 12 bytes, 4-byte aligned (W % 4 == 0): three 4-byte words
  static __device__ __forceinline__ void load12(const uint8_t *p, uint32_t (&w)[3]) {
    const uint32_t *r = reinterpret_cast<const uint32_t *>(p);
    w[0] = r[0], w[1] = r[1], w[2] = r[2];
  }
  static __device__ __forceinline__ void store12(uint8_t *p, const uint32_t (&s)[12]) {
    uint32_t *o = reinterpret_cast<uint32_t *>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = s[4 * k] | (s[4 * k + 1] << 8) | (s[4 * k + 2] << 16) | (s[4 * k + 3] << 24);
  }
};

// uint16 HWC with samples in [0, maxval] (1023: 10-bit data, 65535: full range).  The way in is the 8-bit one with the divisor
// exchanged (a true fp32 division, then the same ATen-order lerp).  The way out is NOT the 8-bit one: a 16-bit frame has no
// reference to equal, so it is rounded to nearest even and saturated, NaN -> 0.  v / maxval * maxval lies within
// 65535 * 2^-23 of v, so an unresized frame comes back bit for bit.
__device__ __forceinline__ uint32_t round_sat_u16(float scaled, float maxval) {
  float r = rintf(scaled);  // half to even (torch.round)
  if (!(r >= 0.f)) r = 0.f;  // negative values and NaN
  if (r > maxval) r = maxval;
  return (uint32_t)(int)r;
}
struct Samples16 {
  typedef uint16_t sample_t;
  static constexpr bool kCopyTaps = true;
  float maxval;
  __device__ __forceinline__ float to_unit(float v) const { return __fdiv_rn(v, maxval); }
  __device__ __forceinline__ float scale() const { return maxval; }
  __device__ __forceinline__ uint32_t quantise(float scaled) const { return round_sat_u16(scaled, maxval); }
  // four pixels of a row are 24 bytes, 8-byte aligned (W % 4 == 0): three 8-byte words
  static __device__ __forceinline__ void load12(const uint16_t *p, uint32_t (&w)[6]) {
    const uint2 *r = reinterpret_cast<const uint2 *>(p);
    const uint2 a0 = r[0], a1 = r[1], a2 = r[2];
    w[0] = a0.x, w[1] = a0.y, w[2] = a1.x, w[3] = a1.y, w[4] = a2.x, w[5] = a2.y;
  }
  static __device__ __forceinline__ void store12(uint16_t *p, const uint32_t (&s)[12]) {
    uint2 *o = reinterpret_cast<uint2 *>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = make_uint2(s[4 * k] | (s[4 * k + 1] << 16), s[4 * k + 2] | (s[4 * k + 3] << 16));
  }
};
template <class S>
struct Packed {  // 12 samples in 32-bit words
  static constexpr int kBits = 8 * (int)sizeof(typename S::sample_t), kPerWord = 32 / kBits, kWords = 12 / kPerWord;
  uint32_t w[kWords];
  __device__ __forceinline__ float sample(int k) const { return (float)((w[k / kPerWord] >> (kBits * (k % kPerWord))) & ((1u << kBits) - 1u)); }
};
// the taps of an axis on the way out
template <class S>
__device__ __forceinline__ Lerp lerp_out(int dst, float scale, int in_size, int out_size) {
  if constexpr (S::kCopyTaps)
    return lerp_src_aten_sized(dst, scale, in_size, out_size);
  else
    return lerp_src_aten(dst, scale, in_size);
}

// blockDim.x for the grid-stride bodies.  Read in a __global__ function, blockDim.x is one scalar load of the (uniform)
// work-group size; read in a function inlined into it, the compiler also provides for a partial last work-group.  The builtin
// is the single load in both places, so the kernels keep the code they had when the loops stood in them.
__device__ __forceinline__ unsigned block_dim_x() { return __builtin_amdgcn_workgroup_size_x(); }

// ---- the six conversions ---------------------------------------------------------------------------------------------------------
// to_inp = resize(to_tensor(img), dst_size) in ONE pass: HWC samples -> to unit range -> bilinear -> fp32 [1,3,Hout,Wout]
// (the reference materialises the full-size fp32 frame in between, tools.py:33-34,59-60), and the same values pixel-major,
// [Hout,Wout,4] = (c0, c1, c2, 0), when out_x4 is given.
template <class S>
__device__ __forceinline__ void to_inp_body(const S s, const typename S::sample_t *__restrict__ in, float *__restrict__ out,
                                            float *__restrict__ out_x4, int Hin, int Win, int Hout, int Wout, float sy, float sx) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  const Lerp ly = lerp_src_aten(p.y, sy, Hin), lx = lerp_src_aten(p.x, sx, Win);
  const typename S::sample_t *r0 = in + (size_t)ly.i0 * Win * 3, *r1 = in + (size_t)ly.i1 * Win * 3;
  const size_t P = (size_t)Hout * Wout, o = (size_t)p.y * Wout + p.x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = s.to_unit((float)r0[lx.i0 * 3 + c]), b = s.to_unit((float)r0[lx.i1 * 3 + c]);
    const float cc = s.to_unit((float)r1[lx.i0 * 3 + c]), d = s.to_unit((float)r1[lx.i1 * 3 + c]);
    const float v = lerp2_aten(ly, lx, a, b, cc, d);
    out[c * P + o] = v;
    if (out_x4) out_x4[4 * o + c] = v;
  }
  if (out_x4) out_x4[4 * o + 3] = 0.f;
}

// to_out = to_cv2(resize(x, src_size)) in ONE pass: fp32 [1,3,Hin,Win] -> bilinear -> * scale, quantised -> HWC samples,
// channels reversed when `rev` (the BGR -> RGB flip of the encoder pipe, tools.py:202, otherwise a host-side copy).
template <class S>
__device__ __forceinline__ void to_out_body(const S s, const float *__restrict__ in, typename S::sample_t *__restrict__ out, int Hin,
                                            int Win, int Hout, int Wout, float sy, float sx, int rev) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  const Lerp ly = lerp_out<S>(p.y, sy, Hin, Hout), lx = lerp_out<S>(p.x, sx, Win, Wout);
  const size_t P = (size_t)Hin * Win;
  typename S::sample_t *o = out + ((size_t)p.y * Wout + p.x) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float *r0 = in + c * P + (size_t)ly.i0 * Win, *r1 = in + c * P + (size_t)ly.i1 * Win;
    const float v = __fmul_rn(lerp2_aten(ly, lx, r0[lx.i0], r0[lx.i1], r1[lx.i0], r1[lx.i1]), s.scale());
    o[rev ? 2 - c : c] = (typename S::sample_t)s.quantise(v);
  }
}

// The frame sizes of the 1080p / 4K configurations change the HEIGHT only (1080 -> 1088, 2160 -> 2176: the width is already a
// multiple of the padding): the horizontal interpolation is the identity -- scale_x == 1 gives s = x, weights (1, 0), and
// fma(1, a, 0 * b) == a for finite b -- so a lane takes FOUR consecutive pixels of a row with 16-byte loads / stores instead of
// one pixel with 12 scalar loads and 3 sample (or 3 dword) stores: same values bit for bit, a third of the time (round 4: the
// one-pixel kernels were 46 + 2 x 34 us of a 2.43 ms 1080p step at 0.9 TB/s).
typedef float f32x4g __attribute__((ext_vector_type(4)));
template <class S>
__device__ __forceinline__ void to_inp_rows_body(const S s, const typename S::sample_t *__restrict__ in, float *__restrict__ out,
                                                 float *__restrict__ out_x4, int Hin, int W, int Hout, float sy) {
  const int W4 = W >> 2;
  const size_t total = (size_t)W4 * Hout, P = (size_t)Hout * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W4), x = (int)(i - (size_t)y * W4) * 4;
    const Lerp ly = lerp_src_aten(y, sy, Hin);
    Packed<S> a, b;
    S::load12(in + ((size_t)ly.i0 * W + x) * 3, a.w);
    S::load12(in + ((size_t)ly.i1 * W + x) * 3, b.w);
    f32x4g o[3];
#pragma unroll
    for (int px = 0; px < 4; ++px)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = s.to_unit(a.sample(px * 3 + c)), bot = s.to_unit(b.sample(px * 3 + c));
        o[c][px] = __fmaf_rn(ly.w0, top, __fmul_rn(ly.w1, bot));
      }
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4g *>(out + (size_t)c * P + (size_t)y * W + x) = o[c];
    if (out_x4) {  // the same values pixel-major, (c0, c1, c2, 0): 64 contiguous bytes per lane
#pragma unroll
      for (int px = 0; px < 4; ++px)
        *reinterpret_cast<f32x4g *>(out_x4 + ((size_t)y * W + x + px) * 4) = (f32x4g){o[0][px], o[1][px], o[2][px], 0.f};
    }
  }
}
// ... and 12 contiguous samples stored per lane.  With kCopyTaps the horizontal pass is ATen's copy, fma(1, a, 0 * a): a for
// finite a, NaN otherwise.
template <class S>
__device__ __forceinline__ void to_out_rows_body(const S s, const float *__restrict__ in, typename S::sample_t *__restrict__ out,
                                                 int Hin, int W, int Hout, float sy, int rev) {
  const int W4 = W >> 2;
  const size_t total = (size_t)W4 * Hout, P = (size_t)Hin * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W4), x = (int)(i - (size_t)y * W4) * 4;
    const Lerp ly = lerp_out<S>(y, sy, Hin, Hout);
    uint32_t q[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4g t = *reinterpret_cast<const f32x4g *>(in + (size_t)c * P + (size_t)ly.i0 * W + x);
      const f32x4g u = *reinterpret_cast<const f32x4g *>(in + (size_t)c * P + (size_t)ly.i1 * W + x);
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        float top = t[px], bot = u[px];
        if constexpr (S::kCopyTaps) {
          top = __fmaf_rn(1.f, top, __fmul_rn(0.f, top));
          bot = __fmaf_rn(1.f, bot, __fmul_rn(0.f, bot));
        }
        const float v = __fmul_rn(__fmaf_rn(ly.w0, top, __fmul_rn(ly.w1, bot)), s.scale());
        q[px * 3 + (rev ? 2 - c : c)] = s.quantise(v);
      }
    }
    S::store12(out + ((size_t)y * W + x) * 3, q);
  }
}

// the no-resize pair (tools.py:33-34, 37-38): HWC samples -> [1,3,H,W] fp32 in unit range, and back through the quantiser
template <class S>
__device__ __forceinline__ void samples_to_f32_body(const S s, const typename S::sample_t *__restrict__ in, float *__restrict__ out, int H,
                                                    int W) {
  const size_t P = (size_t)H * W;
  for (size_t p = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; p < P; p += (size_t)gridDim.x * block_dim_x()) {
    const typename S::sample_t *px = in + p * 3;
    out[p] = s.to_unit((float)px[0]);
    out[P + p] = s.to_unit((float)px[1]);
    out[2 * P + p] = s.to_unit((float)px[2]);
  }
}
template <class S>
__device__ __forceinline__ void f32_to_samples_body(const S s, const float *__restrict__ in, typename S::sample_t *__restrict__ out, int H,
                                                    int W) {
  const size_t P = (size_t)H * W;
  for (size_t p = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; p < P; p += (size_t)gridDim.x * block_dim_x()) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = (typename S::sample_t)s.quantise(__fmul_rn(in[(size_t)c * P + p], s.scale()));
  }
}

// ---- one kernel symbol per depth and form ---------------------------------------------------------------------------------------
#define DRBA_FRAME_KERNEL __global__ void __launch_bounds__(256)
DRBA_FRAME_KERNEL to_inp_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                int Hout, int Wout, float sy, float sx) {
  to_inp_body(Samples8{}, in, out, out_x4, Hin, Win, Hout, Wout, sy, sx);
}
DRBA_FRAME_KERNEL to_inp16_kernel(const uint16_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                  int Hout, int Wout, float sy, float sx, float maxval) {
  to_inp_body(Samples16{maxval}, in, out, out_x4, Hin, Win, Hout, Wout, sy, sx);
}
DRBA_FRAME_KERNEL to_out_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, int Hin, int Win, int Hout, int Wout, float sy,
                                float sx, int rev) {
  to_out_body(Samples8{}, in, out, Hin, Win, Hout, Wout, sy, sx, rev);
}
DRBA_FRAME_KERNEL to_out16_kernel(const float *__restrict__ in, uint16_t *__restrict__ out, int Hin, int Win, int Hout, int Wout, float sy,
                                  float sx, int rev, float maxval) {
  to_out_body(Samples16{maxval}, in, out, Hin, Win, Hout, Wout, sy, sx, rev);
}
DRBA_FRAME_KERNEL to_inp_rows_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int W,
                                     int Hout, float sy) {
  to_inp_rows_body(Samples8{}, in, out, out_x4, Hin, W, Hout, sy);
}
DRBA_FRAME_KERNEL to_inp16_rows_kernel(const uint16_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int W,
                                       int Hout, float sy, float maxval) {
  to_inp_rows_body(Samples16{maxval}, in, out, out_x4, Hin, W, Hout, sy);
}
DRBA_FRAME_KERNEL to_out_rows_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, int Hin, int W, int Hout, float sy, int rev) {
  to_out_rows_body(Samples8{}, in, out, Hin, W, Hout, sy, rev);
}
DRBA_FRAME_KERNEL to_out16_rows_kernel(const float *__restrict__ in, uint16_t *__restrict__ out, int Hin, int W, int Hout, float sy, int rev,
                                       float maxval) {
  to_out_rows_body(Samples16{maxval}, in, out, Hin, W, Hout, sy, rev);
}
DRBA_FRAME_KERNEL u8_to_f32_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, int H, int W) {
  samples_to_f32_body(Samples8{}, in, out, H, W);
}
DRBA_FRAME_KERNEL u16_to_f32_kernel(const uint16_t *__restrict__ in, float *__restrict__ out, int H, int W, float maxval) {
  samples_to_f32_body(Samples16{maxval}, in, out, H, W);
}
DRBA_FRAME_KERNEL f32_to_u8_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, int H, int W) {
  f32_to_samples_body(Samples8{}, in, out, H, W);
}
DRBA_FRAME_KERNEL f32_to_u16_kernel(const float *__restrict__ in, uint16_t *__restrict__ out, int H, int W, float maxval) {
  f32_to_samples_body(Samples16{maxval}, in, out, H, W);
}
#undef DRBA_FRAME_KERNEL

// ---- launch helpers: one per operation; M... is empty for bytes and (float maxval) for 16-bit samples ---------------------------
// The rows form needs an unchanged width that is a multiple of 4, 16-byte aligned fp32 rows and the samples of four pixels aligned
// to their load / store word: 4 bytes for bytes, 8 for 16-bit samples.
// (The launch trace names a kernel by its address, so it reads the same as when the entries launched their kernels by name; only
// DRBA_LAUNCH's textual fallback for an address without a name would now read `one` / `rows` / `kernel`.)
template <class T>
bool rows_form_ok(int Win, int Wout, float scale_x, const T *samples, const float *planes) {
  return Win == Wout && scale_x == 1.f && (Wout & 3) == 0 && (((uintptr_t)samples & (4 * sizeof(T) - 1)) | ((uintptr_t)planes & 15)) == 0;
}

template <class T, class... M>
int to_inp_launch(void (*one)(const T *, float *, float *, int, int, int, int, float, float, M...),
                  void (*rows)(const T *, float *, float *, int, int, int, float, M...), const T *img_hwc, float *out, float *out_x4, int Hin,
                  int Win, int Hout, int Wout, float scale_y, float scale_x, void *stream, M... maxval) {
  if (!img_hwc || !out || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || ((uintptr_t)out_x4 & 15) != 0) return DRBA_EINVAL;
  if (rows_form_ok(Win, Wout, scale_x, img_hwc, out))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 2) * Hout)), dim3(kBlock), 0, (hipStream_t)stream, img_hwc, out, out_x4, Hin, Wout,
                Hout, scale_y, maxval...);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wout, Hout)), dim3(kBlock), 0, (hipStream_t)stream, img_hwc, out, out_x4, Hin, Win, Hout, Wout, scale_y,
                scale_x, maxval...);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

template <class T, class... M>
int to_out_launch(void (*one)(const float *, T *, int, int, int, int, float, float, int, M...),
                  void (*rows)(const float *, T *, int, int, int, float, int, M...), const float *in, T *out_hwc, int Hin, int Win, int Hout,
                  int Wout, float scale_y, float scale_x, int reverse_channels, void *stream, M... maxval) {
  if (!in || !out_hwc || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return DRBA_EINVAL;
  if (rows_form_ok(Win, Wout, scale_x, out_hwc, in))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 2) * Hout)), dim3(kBlock), 0, (hipStream_t)stream, in, out_hwc, Hin, Wout, Hout,
                scale_y, reverse_channels, maxval...);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wout, Hout)), dim3(kBlock), 0, (hipStream_t)stream, in, out_hwc, Hin, Win, Hout, Wout, scale_y,
                scale_x, reverse_channels, maxval...);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

// the no-resize pair, either direction
template <class Tin, class Tout, class... M>
int plane_launch(void (*kernel)(const Tin *, Tout *, int, int, M...), const Tin *in, Tout *out, int H, int W, void *stream, M... maxval) {
  if (!in || !out || H <= 0 || W <= 0) return DRBA_EINVAL;
  DRBA_LAUNCH(kernel, dim3(grid_for((size_t)H * W)), dim3(kBlock), 0, (hipStream_t)stream, in, out, H, W, maxval...);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

// the 16-bit entries check this and the 2-byte alignment of their samples in front
bool maxval_ok(float maxval) { return maxval > 255.f && maxval <= 65535.f; }  // (NaN fails both)

}  // namespace

extern "C" {

int drba_resize_bilinear(const float *in, float *out, int NC, int Hin, int Win, int Hout, int Wout, float scale_y,
                         float scale_x, void *stream) {
  if (!in || !out || NC <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return DRBA_EINVAL;
  DRBA_LAUNCH(resize_bilinear_kernel, dim3(grid_for((size_t)NC * Hout * Wout)), dim3(kBlock), 0,
                     (hipStream_t)stream, in, out, NC, Hin, Win, Hout, Wout, scale_y, scale_x);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

int drba_u8hwc_to_f32nchw(const uint8_t *in, float *out, int H, int W, void *stream) {
  return plane_launch(u8_to_f32_kernel, in, out, H, W, stream);
}

int drba_f32nchw_to_u8hwc(const float *in, uint8_t *out, int H, int W, void *stream) {
  return plane_launch(f32_to_u8_kernel, in, out, H, W, stream);
}

int drba_to_inp_x4(const uint8_t *img_hwc, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                   void *stream) {
  return to_inp_launch(to_inp_kernel, to_inp_rows_kernel, img_hwc, out, out_x4, Hin, Win, Hout, Wout, scale_y, scale_x, stream);
}

int drba_to_inp(const uint8_t *img_hwc, float *out, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                void *stream) {
  return drba_to_inp_x4(img_hwc, out, nullptr, Hin, Win, Hout, Wout, scale_y, scale_x, stream);
}

int drba_to_out(const float *in, uint8_t *out_hwc, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                int reverse_channels, void *stream) {
  return to_out_launch(to_out_kernel, to_out_rows_kernel, in, out_hwc, Hin, Win, Hout, Wout, scale_y, scale_x, reverse_channels, stream);
}

int drba_u16hwc_to_f32nchw(const uint16_t *in, float *out, int H, int W, float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)in & 1) != 0) return DRBA_EINVAL;
  return plane_launch(u16_to_f32_kernel, in, out, H, W, stream, maxval);
}

int drba_f32nchw_to_u16hwc(const float *in, uint16_t *out, int H, int W, float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)out & 1) != 0) return DRBA_EINVAL;
  return plane_launch(f32_to_u16_kernel, in, out, H, W, stream, maxval);
}

int drba_to_inp16_x4(const uint16_t *img_hwc, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, float scale_y,
                     float scale_x, float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)img_hwc & 1) != 0) return DRBA_EINVAL;
  return to_inp_launch(to_inp16_kernel, to_inp16_rows_kernel, img_hwc, out, out_x4, Hin, Win, Hout, Wout, scale_y, scale_x, stream, maxval);
}

int drba_to_out16(const float *in, uint16_t *out_hwc, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                  int reverse_channels, float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)out_hwc & 1) != 0) return DRBA_EINVAL;
  return to_out_launch(to_out16_kernel, to_out16_rows_kernel, in, out_hwc, Hin, Win, Hout, Wout, scale_y, scale_x, reverse_channels, stream,
                       maxval);
}

}  // extern "C"

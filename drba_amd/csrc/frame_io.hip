// The frame source and sink of the pipeline: bilinear resize and the uint8 / uint16 <-> fp32 frame conversions used by
// to_inp / to_out, and their copy forms without a resize (fit = pad: replicate padding in, a crop out).  Each conversion is written once, over a sample trait with two instances (bytes, 16-bit samples); the
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
                                            float *__restrict__ out_x4, int Hin, int Win, int Hout, int Wout, float sy, float sx,
                                            size_t pitch) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  const Lerp ly = lerp_src_aten(p.y, sy, Hin), lx = lerp_src_aten(p.x, sx, Win);
  const typename S::sample_t *r0 = in + (size_t)ly.i0 * pitch, *r1 = in + (size_t)ly.i1 * pitch;
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
                                            int Win, int Hout, int Wout, float sy, float sx, int rev, size_t pitch) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  const Lerp ly = lerp_out<S>(p.y, sy, Hin, Hout), lx = lerp_out<S>(p.x, sx, Win, Wout);
  const size_t P = (size_t)Hin * Win;
  typename S::sample_t *o = out + (size_t)p.y * pitch + (size_t)p.x * 3;
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
                                                 float *__restrict__ out_x4, int Hin, int W, int Hout, float sy, size_t pitch) {
  const int W4 = W >> 2;
  const size_t total = (size_t)W4 * Hout, P = (size_t)Hout * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W4), x = (int)(i - (size_t)y * W4) * 4;
    const Lerp ly = lerp_src_aten(y, sy, Hin);
    Packed<S> a, b;
    S::load12(in + (size_t)ly.i0 * pitch + (size_t)x * 3, a.w);
    S::load12(in + (size_t)ly.i1 * pitch + (size_t)x * 3, b.w);
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
                                                 int Hin, int W, int Hout, float sy, int rev, size_t pitch) {
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
    S::store12(out + (size_t)y * pitch + (size_t)x * 3, q);
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

// ---- fit = pad: the frame at the top left of the network tensor, no interpolation (include/drba_hip.h, ABI 16) -------------------
// Way in, the bottom and right margins repeat the last row and column: out(y, x) = to_unit(in(min(y, Hin - 1), min(x, Win - 1))).
// Way out, the top-left Hout x Wout window is quantised as it stands; nothing outside it is read.
//
// ATen's copy of an axis whose size does not change, fma(1, a, 0 * a): a for finite a, NaN otherwise.  The 16-bit and planar
// ways out keep it (kCopyTaps) so that a cropped frame is, sample for sample, what the unresized conversion of the same window
// gives: NaN and +-inf -> 0 at the quantiser.  Only the pixel itself is read.
__device__ __forceinline__ float aten_copy(float a) { return __fmaf_rn(1.f, a, __fmul_rn(0.f, a)); }
template <class S>
__device__ __forceinline__ float crop_value(float a) {
  if constexpr (S::kCopyTaps)
    return aten_copy(a);
  else
    return a;
}

// the general form of the way in: one output pixel per lane, any size
template <class S>
__device__ __forceinline__ void to_inp_pad_body(const S s, const typename S::sample_t *__restrict__ in, float *__restrict__ out,
                                                float *__restrict__ out_x4, int Hin, int Win, int Hout, int Wout, size_t pitch) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  const typename S::sample_t *px = in + (size_t)min(p.y, Hin - 1) * pitch + (size_t)min(p.x, Win - 1) * 3;
  const size_t P = (size_t)Hout * Wout, o = (size_t)p.y * Wout + p.x;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c] = s.to_unit((float)px[c]);
    out[c * P + o] = v[c];
  }
  if (out_x4) *reinterpret_cast<f32x4g *>(out_x4 + 4 * o) = (f32x4g){v[0], v[1], v[2], 0.f};
}
// the rows form (an unchanged width that is a multiple of 4: only rows are added): four pixels per lane, as to_inp_rows_body
template <class S>
__device__ __forceinline__ void to_inp_pad_rows_body(const S s, const typename S::sample_t *__restrict__ in, float *__restrict__ out,
                                                     float *__restrict__ out_x4, int Hin, int W, int Hout, size_t pitch) {
  const int W4 = W >> 2;
  const size_t total = (size_t)W4 * Hout, P = (size_t)Hout * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W4), x = (int)(i - (size_t)y * W4) * 4;
    Packed<S> a;
    S::load12(in + (size_t)min(y, Hin - 1) * pitch + (size_t)x * 3, a.w);
    f32x4g o[3];
#pragma unroll
    for (int px = 0; px < 4; ++px)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c][px] = s.to_unit(a.sample(px * 3 + c));
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4g *>(out + (size_t)c * P + (size_t)y * W + x) = o[c];
    if (out_x4) {
#pragma unroll
      for (int px = 0; px < 4; ++px)
        *reinterpret_cast<f32x4g *>(out_x4 + ((size_t)y * W + x + px) * 4) = (f32x4g){o[0][px], o[1][px], o[2][px], 0.f};
    }
  }
}
// the way out: pixel (y, x) of the Hout x Wout window of fp32 [1,3,Hin,Win] -> * scale, quantised
template <class S>
__device__ __forceinline__ void to_out_crop_body(const S s, const float *__restrict__ in, typename S::sample_t *__restrict__ out, int Hin,
                                                 int Win, int Hout, int Wout, int rev, size_t pitch) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  const size_t P = (size_t)Hin * Win, i = (size_t)p.y * Win + p.x;
  typename S::sample_t *o = out + (size_t)p.y * pitch + (size_t)p.x * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    o[rev ? 2 - c : c] = (typename S::sample_t)s.quantise(__fmul_rn(crop_value<S>(in[c * P + i]), s.scale()));
}
template <class S>
__device__ __forceinline__ void to_out_crop_rows_body(const S s, const float *__restrict__ in, typename S::sample_t *__restrict__ out,
                                                      int Hin, int W, int Hout, int rev, size_t pitch) {
  const int W4 = W >> 2;
  const size_t total = (size_t)W4 * Hout, P = (size_t)Hin * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W4), x = (int)(i - (size_t)y * W4) * 4;
    uint32_t q[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4g t = *reinterpret_cast<const f32x4g *>(in + (size_t)c * P + (size_t)y * W + x);
#pragma unroll
      for (int px = 0; px < 4; ++px) q[px * 3 + (rev ? 2 - c : c)] = s.quantise(__fmul_rn(crop_value<S>(t[px]), s.scale()));
    }
    S::store12(out + (size_t)y * pitch + (size_t)x * 3, q);
  }
}

// ---- one kernel symbol per depth and form ---------------------------------------------------------------------------------------
#define DRBA_FRAME_KERNEL __global__ void __launch_bounds__(256)
DRBA_FRAME_KERNEL to_inp_pad_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                    int Hout, int Wout, size_t pitch) {
  to_inp_pad_body(Samples8{}, in, out, out_x4, Hin, Win, Hout, Wout, pitch);
}
DRBA_FRAME_KERNEL to_inp16_pad_kernel(const uint16_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                      int Hout, int Wout, size_t pitch, float maxval) {
  to_inp_pad_body(Samples16{maxval}, in, out, out_x4, Hin, Win, Hout, Wout, pitch);
}
DRBA_FRAME_KERNEL to_inp_pad_rows_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int W,
                                         int Hout, size_t pitch) {
  to_inp_pad_rows_body(Samples8{}, in, out, out_x4, Hin, W, Hout, pitch);
}
DRBA_FRAME_KERNEL to_inp16_pad_rows_kernel(const uint16_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin,
                                           int W, int Hout, size_t pitch, float maxval) {
  to_inp_pad_rows_body(Samples16{maxval}, in, out, out_x4, Hin, W, Hout, pitch);
}
DRBA_FRAME_KERNEL to_out_crop_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, int Hin, int Win, int Hout, int Wout, int rev,
                                     size_t pitch) {
  to_out_crop_body(Samples8{}, in, out, Hin, Win, Hout, Wout, rev, pitch);
}
DRBA_FRAME_KERNEL to_out16_crop_kernel(const float *__restrict__ in, uint16_t *__restrict__ out, int Hin, int Win, int Hout, int Wout, int rev,
                                       size_t pitch, float maxval) {
  to_out_crop_body(Samples16{maxval}, in, out, Hin, Win, Hout, Wout, rev, pitch);
}
DRBA_FRAME_KERNEL to_out_crop_rows_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, int Hin, int W, int Hout, int rev, size_t pitch) {
  to_out_crop_rows_body(Samples8{}, in, out, Hin, W, Hout, rev, pitch);
}
DRBA_FRAME_KERNEL to_out16_crop_rows_kernel(const float *__restrict__ in, uint16_t *__restrict__ out, int Hin, int W, int Hout, int rev,
                                            size_t pitch, float maxval) {
  to_out_crop_rows_body(Samples16{maxval}, in, out, Hin, W, Hout, rev, pitch);
}
DRBA_FRAME_KERNEL to_inp_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                int Hout, int Wout, float sy, float sx, size_t pitch) {
  to_inp_body(Samples8{}, in, out, out_x4, Hin, Win, Hout, Wout, sy, sx, pitch);
}
DRBA_FRAME_KERNEL to_inp16_kernel(const uint16_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                  int Hout, int Wout, float sy, float sx, size_t pitch, float maxval) {
  to_inp_body(Samples16{maxval}, in, out, out_x4, Hin, Win, Hout, Wout, sy, sx, pitch);
}
DRBA_FRAME_KERNEL to_out_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, int Hin, int Win, int Hout, int Wout, float sy,
                                float sx, int rev, size_t pitch) {
  to_out_body(Samples8{}, in, out, Hin, Win, Hout, Wout, sy, sx, rev, pitch);
}
DRBA_FRAME_KERNEL to_out16_kernel(const float *__restrict__ in, uint16_t *__restrict__ out, int Hin, int Win, int Hout, int Wout, float sy,
                                  float sx, int rev, size_t pitch, float maxval) {
  to_out_body(Samples16{maxval}, in, out, Hin, Win, Hout, Wout, sy, sx, rev, pitch);
}
DRBA_FRAME_KERNEL to_inp_rows_kernel(const uint8_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int W,
                                     int Hout, float sy, size_t pitch) {
  to_inp_rows_body(Samples8{}, in, out, out_x4, Hin, W, Hout, sy, pitch);
}
DRBA_FRAME_KERNEL to_inp16_rows_kernel(const uint16_t *__restrict__ in, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int W,
                                       int Hout, float sy, size_t pitch, float maxval) {
  to_inp_rows_body(Samples16{maxval}, in, out, out_x4, Hin, W, Hout, sy, pitch);
}
DRBA_FRAME_KERNEL to_out_rows_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, int Hin, int W, int Hout, float sy, int rev,
                                     size_t pitch) {
  to_out_rows_body(Samples8{}, in, out, Hin, W, Hout, sy, rev, pitch);
}
DRBA_FRAME_KERNEL to_out16_rows_kernel(const float *__restrict__ in, uint16_t *__restrict__ out, int Hin, int W, int Hout, float sy, int rev,
                                       size_t pitch, float maxval) {
  to_out_rows_body(Samples16{maxval}, in, out, Hin, W, Hout, sy, rev, pitch);
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

// ---- planar YCbCr 4:2:0 frames (include/drba_hip.h, ABI 14) -------------------------------------------------------------------
// Three planes instead of HWC samples: Y [H][W], U and V [ceil(H/2)][ceil(W/2)].  The colour conversion and the chroma
// resampling happen inside the conversion kernels, on the taps the resize reads (way in) or on the pixels it produced (way
// out): the full-size RGB frame is never formed.  The network tensor keeps the BGR channel order.  The constants are worked
// out on the host in double (yuv_in_consts / yuv_out_consts below); everything here is fp32.
struct YuvIn {
  float y_off, y_mul, c_off, c_mul;  // Y' = (y - y_off) * y_mul, Cb = (u - c_off) * c_mul
  float r_cr, b_cb, kr, kb, inv_kg;  // R = Y' + r_cr Cr, B = Y' + b_cb Cb, G = (Y' - kr R - kb B) * inv_kg
};
struct YuvOut {
  float kr, kg, kb, cb_mul, cr_mul;  // Y' = kr R + kg G + kb B, Cb = (B - Y') * cb_mul, Cr = (R - Y') * cr_mul
  float y_off, y_mul, c_off, c_mul;  // y = y_off + y_mul Y', u = c_off + c_mul Cb
  float maxval;
};

// The two chroma taps of luma coordinate p along one axis of nc chroma samples: the bilinear taps at s = p / 2 - 0.25 clamped
// to [0, nc - 1].  Even p: (p/2 - 1, p/2) with weights (1/4, 3/4); odd p: ((p-1)/2, (p+1)/2) with (3/4, 1/4).  At the two ends
// the clamp of s makes the weights (1, 0) on the edge sample; clamping the INDEX instead gives both taps the edge sample, and
// a / 4 + 3 a / 4 == a exactly for a sample of at most 20 bits, so no case is told apart.  Sums of samples weighted by
// sixteenths are exact in fp32 too: the interpolated chroma carries no rounding at all.
struct CTap {
  int i0, i1;
  float w0, w1;
};
__device__ __forceinline__ CTap chroma_tap(int p, int nc) {
  CTap t;
  const int h = p >> 1;
  if (p & 1) {
    t.i0 = h, t.i1 = min(h + 1, nc - 1);
    t.w0 = 0.75f, t.w1 = 0.25f;
  } else {
    t.i0 = max(h - 1, 0), t.i1 = h;
    t.w0 = 0.25f, t.w1 = 0.75f;
  }
  return t;
}
__device__ __forceinline__ float clamp01(float v) {  // NaN -> 0
  v = v >= 0.f ? v : 0.f;
  return v > 1.f ? 1.f : v;
}
// one pixel: raw luma sample, raw chroma interpolated to its position -> (B, G, R) clamped to [0, 1]
__device__ __forceinline__ void yuv_to_bgr(const YuvIn &k, float y, float u, float v, float (&bgr)[3]) {
  const float Y = (y - k.y_off) * k.y_mul, Cb = (u - k.c_off) * k.c_mul, Cr = (v - k.c_off) * k.c_mul;
  const float R = Y + k.r_cr * Cr, B = Y + k.b_cb * Cb;
  const float G = (Y - k.kr * R - k.kb * B) * k.inv_kg;
  bgr[0] = clamp01(B), bgr[1] = clamp01(G), bgr[2] = clamp01(R);
}
// yuv_to_bgr with every operation spelled out, for the pad forms (below), which must give the values of their resize siblings at an
// unchanged size bit for bit.  yuv_to_bgr leaves the contraction to hipcc, and hipcc settles it per body: R and B are
// fma(coef, C, Y') everywhere, but Y' - Kr R is fma(y_mul, y - y_off, -(Kr R)) -- the product behind Y' taken unrounded -- in the
// general resize bodies and Y' - (Kr R) on the rounded Y' in the rows bodies (read from the ISA of the 8- and 16-bit kernels of
// both forms; the two differ by a few ulp in G).  A pad body names the form it stands beside: kFusedLuma = the general one.
// (Everything else in the planar kernels has one contraction only: the chroma taps are exact, and bgr_to_ycc with the code
// computation behind it compiles to the same operations in every body.)
template <bool kFusedLuma>
__device__ __forceinline__ void yuv_to_bgr_as(const YuvIn &k, float y, float u, float v, float (&bgr)[3]) {
#pragma clang fp contract(off)  // (the __f*_rn functions are plain operators to hipcc and would be contracted again)
  const float ys = y - k.y_off, Y = ys * k.y_mul;
  const float Cb = (u - k.c_off) * k.c_mul, Cr = (v - k.c_off) * k.c_mul;
  const float R = __builtin_fmaf(k.r_cr, Cr, Y), B = __builtin_fmaf(k.b_cb, Cb, Y);
  const float krR = k.kr * R, kbB = k.kb * B;
  const float t = kFusedLuma ? __builtin_fmaf(k.y_mul, ys, -krR) : Y - krR;
  const float G = (t - kbB) * k.inv_kg;
  bgr[0] = clamp01(B), bgr[1] = clamp01(G), bgr[2] = clamp01(R);
}
// (B, G, R) as the resize left them -> clamped, Y' and the two colour differences
__device__ __forceinline__ void bgr_to_ycc(const YuvOut &k, float b, float g, float r, float &Y, float &Cb, float &Cr) {
  b = clamp01(b), g = clamp01(g), r = clamp01(r);
  Y = k.kr * r + k.kg * g + k.kb * b;
  Cb = (b - Y) * k.cb_mul;
  Cr = (r - Y) * k.cr_mul;
}

// the general form of the way in: one output pixel per lane, any size.  Each of the four taps of the resize is a source PIXEL,
// converted from its luma sample and the 2 x 2 chroma taps of either plane.  (kSpelled: the pad form, yuv_to_bgr_as.)
template <class T, bool kSpelled = false>
__device__ __forceinline__ void yuv_pixel(const YuvIn &k, const T *__restrict__ yp, const T *__restrict__ up, const T *__restrict__ vp,
                                          int ys, int cs, int Hc, int Wc, int sy, int sx, float (&bgr)[3]) {
  const CTap ty = chroma_tap(sy, Hc), tx = chroma_tap(sx, Wc);
  const size_t r0 = (size_t)ty.i0 * cs, r1 = (size_t)ty.i1 * cs;
  const float u = ty.w0 * (tx.w0 * (float)up[r0 + tx.i0] + tx.w1 * (float)up[r0 + tx.i1]) +
                  ty.w1 * (tx.w0 * (float)up[r1 + tx.i0] + tx.w1 * (float)up[r1 + tx.i1]);
  const float v = ty.w0 * (tx.w0 * (float)vp[r0 + tx.i0] + tx.w1 * (float)vp[r0 + tx.i1]) +
                  ty.w1 * (tx.w0 * (float)vp[r1 + tx.i0] + tx.w1 * (float)vp[r1 + tx.i1]);
  if constexpr (kSpelled)
    yuv_to_bgr_as<true>(k, (float)yp[(size_t)sy * ys + sx], u, v, bgr);
  else
    yuv_to_bgr(k, (float)yp[(size_t)sy * ys + sx], u, v, bgr);
}
template <class T>
__device__ __forceinline__ void to_inp_yuv_body(const YuvIn k, const T *__restrict__ yp, const T *__restrict__ up, const T *__restrict__ vp,
                                                int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                                int Hout, int Wout, float sy, float sx) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  const Lerp ly = lerp_src_aten(p.y, sy, Hin), lx = lerp_src_aten(p.x, sx, Win);
  const int Hc = (Hin + 1) >> 1, Wc = (Win + 1) >> 1;
  float a[3], b[3], c[3], d[3];
  yuv_pixel(k, yp, up, vp, ys, cs, Hc, Wc, ly.i0, lx.i0, a);
  yuv_pixel(k, yp, up, vp, ys, cs, Hc, Wc, ly.i0, lx.i1, b);
  yuv_pixel(k, yp, up, vp, ys, cs, Hc, Wc, ly.i1, lx.i0, c);
  yuv_pixel(k, yp, up, vp, ys, cs, Hc, Wc, ly.i1, lx.i1, d);
  const size_t P = (size_t)Hout * Wout, o = (size_t)p.y * Wout + p.x;
  float v[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    v[ch] = lerp2_aten(ly, lx, a[ch], b[ch], c[ch], d[ch]);
    out[ch * P + o] = v[ch];
  }
  if (out_x4) *reinterpret_cast<f32x4g *>(out_x4 + 4 * o) = (f32x4g){v[0], v[1], v[2], 0.f};
}

// N consecutive samples of a plane row with one aligned load: 4 bytes (N = 4) or 8 (N = 8) for bytes, 8 or 16 for 16-bit samples
template <class T, int N>
struct SampleRow {
  static constexpr int kBits = 8 * (int)sizeof(T), kPerWord = 32 / kBits, kWords = N / kPerWord;
  uint32_t w[kWords];
  __device__ __forceinline__ void load(const T *p) {
    if constexpr (kWords == 1) {
      w[0] = *reinterpret_cast<const uint32_t *>(p);
    } else if constexpr (kWords == 2) {
      const uint2 r = *reinterpret_cast<const uint2 *>(p);
      w[0] = r.x, w[1] = r.y;
    } else {
      const uint4 r = *reinterpret_cast<const uint4 *>(p);
      w[0] = r.x, w[1] = r.y, w[2] = r.z, w[3] = r.w;
    }
  }
  __device__ __forceinline__ float sample(int j) const { return (float)((w[j / kPerWord] >> (kBits * (j % kPerWord))) & ((1u << kBits) - 1u)); }
  // ... and N quantised samples (one per element of q) stored the same way
  static __device__ __forceinline__ void store(T *p, const uint32_t (&q)[N]) {
    uint32_t o[kWords];
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
      o[j] = 0;
#pragma unroll
      for (int e = 0; e < kPerWord; ++e) o[j] |= q[j * kPerWord + e] << (kBits * e);
    }
    if constexpr (kWords == 1)
      *reinterpret_cast<uint32_t *>(p) = o[0];
    else if constexpr (kWords == 2)
      *reinterpret_cast<uint2 *>(p) = make_uint2(o[0], o[1]);
    else
      *reinterpret_cast<uint4 *>(p) = make_uint4(o[0], o[1], o[2], o[3]);
  }
};

// The rows form of the way in (an unchanged width that is a multiple of 8: only the height is resized).  A lane takes EIGHT
// consecutive pixels of an output row: per source row one aligned load of 8 luma samples and, per chroma plane and chroma row,
// one aligned load of the 4 samples under them plus their two neighbours (index clamped: see chroma_tap), then 2 x 3 16-byte
// stores of the planes and 8 of the pixel-major copy.  The horizontal pass of the resize is the identity as in to_inp_rows_body.
template <class T>
__device__ __forceinline__ void chroma_raw6(const T *__restrict__ row, int Wc, int xc, float (&c)[6]) {
  SampleRow<T, 4> a;
  a.load(row + xc);
  c[0] = (float)row[max(xc - 1, 0)];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[1 + j] = a.sample(j);
  c[5] = (float)row[min(xc + 4, Wc - 1)];
}
// The two source rows of an output row are neighbours (i1 == i0 + 1, or i0 itself at the bottom), and so are their chroma taps:
// rows (h-1, h) and (h, h+1) for i0 = 2h, the one pair (h, h+1) with the weights exchanged for i0 = 2h + 1.  So at most THREE
// chroma rows per plane are loaded, base .. base + 2 with base = floor((i0 - 1) / 2), each index clamped (a clamped duplicate
// holds the samples its tap asks for), and the third only where the second source row reaches it.
template <class T>
__device__ __forceinline__ void to_inp_yuv_rows_body(const YuvIn k, const T *__restrict__ yp, const T *__restrict__ up,
                                                     const T *__restrict__ vp, int ys, int cs, float *__restrict__ out,
                                                     float *__restrict__ out_x4, int Hin, int W, int Hout, float sy) {
  const int W8 = W >> 3, Hc = (Hin + 1) >> 1, Wc = W >> 1;
  const size_t total = (size_t)W8 * Hout, P = (size_t)Hout * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W8), x = (int)(i - (size_t)y * W8) * 8, xc = x >> 1;
    const Lerp ly = lerp_src_aten(y, sy, Hin);
    const CTap t0 = chroma_tap(ly.i0, Hc), t1 = chroma_tap(ly.i1, Hc);
    const int base = (ly.i0 - 1) >> 1;
    const int rk0 = min(max(base, 0), Hc - 1), rk1 = min(max(base + 1, 0), Hc - 1), rk2 = min(base + 2, Hc - 1);
    float ru[3][6], rv[3][6];
    chroma_raw6(up + (size_t)rk0 * cs, Wc, xc, ru[0]), chroma_raw6(vp + (size_t)rk0 * cs, Wc, xc, rv[0]);
    chroma_raw6(up + (size_t)rk1 * cs, Wc, xc, ru[1]), chroma_raw6(vp + (size_t)rk1 * cs, Wc, xc, rv[1]);
    if (t1.i1 != rk0 && t1.i1 != rk1) {
      chroma_raw6(up + (size_t)rk2 * cs, Wc, xc, ru[2]), chroma_raw6(vp + (size_t)rk2 * cs, Wc, xc, rv[2]);
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) ru[2][j] = ru[1][j], rv[2][j] = rv[1][j];
    }
    float px[2][8][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      SampleRow<T, 8> luma;
      luma.load(yp + (size_t)(r ? ly.i1 : ly.i0) * ys + x);
      const CTap ty = r ? t1 : t0;
      const int sa = ty.i0 == rk0 ? 0 : (ty.i0 == rk1 ? 1 : 2), sb = ty.i1 == rk0 ? 0 : (ty.i1 == rk1 ? 1 : 2);
      float cu[6], cv[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const float ua = sa == 0 ? ru[0][j] : (sa == 1 ? ru[1][j] : ru[2][j]), ub = sb == 0 ? ru[0][j] : (sb == 1 ? ru[1][j] : ru[2][j]);
        const float va = sa == 0 ? rv[0][j] : (sa == 1 ? rv[1][j] : rv[2][j]), vb = sb == 0 ? rv[0][j] : (sb == 1 ? rv[1][j] : rv[2][j]);
        cu[j] = ty.w0 * ua + ty.w1 * ub;
        cv[j] = ty.w0 * va + ty.w1 * vb;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {  // pixel x + j: taps (j/2, j/2 + 1) of the six for even j, ((j+1)/2, (j+1)/2 + 1) for odd j
        const int c0 = (j + 1) >> 1;
        const float w0 = (j & 1) ? 0.75f : 0.25f, w1 = (j & 1) ? 0.25f : 0.75f;
        yuv_to_bgr(k, luma.sample(j), w0 * cu[c0] + w1 * cu[c0 + 1], w0 * cv[c0] + w1 * cv[c0 + 1], px[r][j]);
      }
    }
    f32x4g o[3][2];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c][j >> 2][j & 3] = __fmaf_rn(ly.w0, px[0][j][c], __fmul_rn(ly.w1, px[1][j][c]));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4g *dst = reinterpret_cast<f32x4g *>(out + (size_t)c * P + (size_t)y * W + x);
      dst[0] = o[c][0], dst[1] = o[c][1];
    }
    if (out_x4) {
      f32x4g *dst = reinterpret_cast<f32x4g *>(out_x4 + ((size_t)y * W + x) * 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = (f32x4g){o[0][j >> 2][j & 3], o[1][j >> 2][j & 3], o[2][j >> 2][j & 3], 0.f};
    }
  }
}

// The general form of the way out: one 2 x 2 luma block per lane, so the chroma mean stays in the lane.  A pixel past an odd
// edge repeats the edge pixel in the mean and is not stored.  The resize follows to_out16's rules (lerp_out<Samples16>).
template <class T>
__device__ __forceinline__ void to_out_yuv_body(const YuvOut k, const float *__restrict__ in, T *__restrict__ yp, T *__restrict__ up,
                                                T *__restrict__ vp, int ys, int cs, int Hin, int Win, int Hout, int Wout, float sy,
                                                float sx) {
  const int Hc = (Hout + 1) >> 1, Wc = (Wout + 1) >> 1;
  const Tile2D p = tile_pixel(Wc, Hc);
  if (!p.valid) return;
  const size_t P = (size_t)Hin * Win;
  float cb = 0.f, cr = 0.f;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int oy = min(2 * p.y + dy, Hout - 1);
    const Lerp ly = lerp_out<Samples16>(oy, sy, Hin, Hout);
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int ox = min(2 * p.x + dx, Wout - 1);
      const Lerp lx = lerp_out<Samples16>(ox, sx, Win, Wout);
      float ch[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float *r0 = in + c * P + (size_t)ly.i0 * Win, *r1 = in + c * P + (size_t)ly.i1 * Win;
        ch[c] = lerp2_aten(ly, lx, r0[lx.i0], r0[lx.i1], r1[lx.i0], r1[lx.i1]);
      }
      float Y, Cb, Cr;
      bgr_to_ycc(k, ch[0], ch[1], ch[2], Y, Cb, Cr);
      cb += Cb, cr += Cr;
      if (2 * p.y + dy < Hout && 2 * p.x + dx < Wout) yp[(size_t)oy * ys + ox] = (T)round_sat_u16(k.y_off + k.y_mul * Y, k.maxval);
    }
  }
  const size_t o = (size_t)p.y * cs + p.x;
  up[o] = (T)round_sat_u16(k.c_off + k.c_mul * (cb * 0.25f), k.maxval);
  vp[o] = (T)round_sat_u16(k.c_off + k.c_mul * (cr * 0.25f), k.maxval);
}

// The rows form of the way out (an unchanged width that is a multiple of 8): a lane takes two output rows of four blocks,
// 2 x 8 pixels, with 16-byte loads of the fp32 planes, and stores 8 luma samples per row and 4 of either chroma plane with one
// store each.  With an odd height the last lane row repeats the last output row in the mean and stores it once.
template <class T>
__device__ __forceinline__ void to_out_yuv_rows_body(const YuvOut k, const float *__restrict__ in, T *__restrict__ yp, T *__restrict__ up,
                                                     T *__restrict__ vp, int ys, int cs, int Hin, int W, int Hout, float sy) {
  const int W8 = W >> 3, Hc = (Hout + 1) >> 1;
  const size_t total = (size_t)W8 * Hc, P = (size_t)Hin * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int j = (int)(i / W8), x = (int)(i - (size_t)j * W8) * 8;
    float cb[4] = {0.f, 0.f, 0.f, 0.f}, cr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int oy = min(2 * j + r, Hout - 1);
      const Lerp ly = lerp_out<Samples16>(oy, sy, Hin, Hout);
      uint32_t q[8];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4g ch[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const f32x4g t = *reinterpret_cast<const f32x4g *>(in + (size_t)c * P + (size_t)ly.i0 * W + x + 4 * h);
          const f32x4g u = *reinterpret_cast<const f32x4g *>(in + (size_t)c * P + (size_t)ly.i1 * W + x + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) {  // the horizontal pass is ATen's copy, fma(1, a, 0 * a): a for finite a, NaN otherwise
            const float top = __fmaf_rn(1.f, t[e], __fmul_rn(0.f, t[e])), bot = __fmaf_rn(1.f, u[e], __fmul_rn(0.f, u[e]));
            ch[c][e] = __fmaf_rn(ly.w0, top, __fmul_rn(ly.w1, bot));
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float Y, Cb, Cr;
          bgr_to_ycc(k, ch[0][e], ch[1][e], ch[2][e], Y, Cb, Cr);
          q[4 * h + e] = round_sat_u16(k.y_off + k.y_mul * Y, k.maxval);
          cb[2 * h + (e >> 1)] += Cb, cr[2 * h + (e >> 1)] += Cr;
        }
      }
      if (2 * j + r < Hout) SampleRow<T, 8>::store(yp + (size_t)oy * ys + x, q);
    }
    uint32_t qu[4], qv[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      qu[b] = round_sat_u16(k.c_off + k.c_mul * (cb[b] * 0.25f), k.maxval);
      qv[b] = round_sat_u16(k.c_off + k.c_mul * (cr[b] * 0.25f), k.maxval);
    }
    SampleRow<T, 4>::store(up + (size_t)j * cs + (x >> 1), qu);
    SampleRow<T, 4>::store(vp + (size_t)j * cs + (x >> 1), qv);
  }
}

// ---- fit = pad for planar frames: as the packed forms above -------------------------------------------------------------------------
// Way in, an output pixel is the source PIXEL at the clamped coordinate (its luma sample and the 2 x 2 chroma taps of that source
// coordinate), so the margin continues the converted picture and no chroma tap is taken past the frame.
template <class T>
__device__ __forceinline__ void to_inp_yuv_pad_body(const YuvIn k, const T *__restrict__ yp, const T *__restrict__ up, const T *__restrict__ vp,
                                                    int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                                    int Hout, int Wout) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  float v[3];
  yuv_pixel<T, true>(k, yp, up, vp, ys, cs, (Hin + 1) >> 1, (Win + 1) >> 1, min(p.y, Hin - 1), min(p.x, Win - 1), v);
  const size_t P = (size_t)Hout * Wout, o = (size_t)p.y * Wout + p.x;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch * P + o] = v[ch];
  if (out_x4) *reinterpret_cast<f32x4g *>(out_x4 + 4 * o) = (f32x4g){v[0], v[1], v[2], 0.f};
}
// The rows form (an unchanged width that is a multiple of 8): eight pixels of an output row per lane from ONE source row, its
// 8 luma samples and the two chroma rows of its taps, loaded as in to_inp_yuv_rows_body.
template <class T>
__device__ __forceinline__ void to_inp_yuv_pad_rows_body(const YuvIn k, const T *__restrict__ yp, const T *__restrict__ up,
                                                         const T *__restrict__ vp, int ys, int cs, float *__restrict__ out,
                                                         float *__restrict__ out_x4, int Hin, int W, int Hout) {
  const int W8 = W >> 3, Hc = (Hin + 1) >> 1, Wc = W >> 1;
  const size_t total = (size_t)W8 * Hout, P = (size_t)Hout * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W8), x = (int)(i - (size_t)y * W8) * 8, xc = x >> 1, sy = min(y, Hin - 1);
    const CTap ty = chroma_tap(sy, Hc);
    float ua[6], ub[6], va[6], vb[6], cu[6], cv[6];
    chroma_raw6(up + (size_t)ty.i0 * cs, Wc, xc, ua), chroma_raw6(vp + (size_t)ty.i0 * cs, Wc, xc, va);
    chroma_raw6(up + (size_t)ty.i1 * cs, Wc, xc, ub), chroma_raw6(vp + (size_t)ty.i1 * cs, Wc, xc, vb);
#pragma unroll
    for (int j = 0; j < 6; ++j) cu[j] = ty.w0 * ua[j] + ty.w1 * ub[j], cv[j] = ty.w0 * va[j] + ty.w1 * vb[j];
    SampleRow<T, 8> luma;
    luma.load(yp + (size_t)sy * ys + x);
    f32x4g o[3][2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // the taps of pixel x + j among the six: to_inp_yuv_rows_body
      const int c0 = (j + 1) >> 1;
      const float w0 = (j & 1) ? 0.75f : 0.25f, w1 = (j & 1) ? 0.25f : 0.75f;
      float px[3];
      yuv_to_bgr_as<false>(k, luma.sample(j), w0 * cu[c0] + w1 * cu[c0 + 1], w0 * cv[c0] + w1 * cv[c0 + 1], px);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c][j >> 2][j & 3] = px[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4g *dst = reinterpret_cast<f32x4g *>(out + (size_t)c * P + (size_t)y * W + x);
      dst[0] = o[c][0], dst[1] = o[c][1];
    }
    if (out_x4) {
      f32x4g *dst = reinterpret_cast<f32x4g *>(out_x4 + ((size_t)y * W + x) * 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = (f32x4g){o[0][j >> 2][j & 3], o[1][j >> 2][j & 3], o[2][j >> 2][j & 3], 0.f};
    }
  }
}

// Way out: one 2 x 2 luma block of the Hout x Wout window per lane.  A pixel past an odd edge repeats the edge pixel of the WINDOW
// in the chroma mean, as in to_out_yuv_body: the margin of the network tensor is never read.
template <class T>
__device__ __forceinline__ void to_out_yuv_crop_body(const YuvOut k, const float *__restrict__ in, T *__restrict__ yp, T *__restrict__ up,
                                                     T *__restrict__ vp, int ys, int cs, int Hin, int Win, int Hout, int Wout) {
  const int Hc = (Hout + 1) >> 1, Wc = (Wout + 1) >> 1;
  const Tile2D p = tile_pixel(Wc, Hc);
  if (!p.valid) return;
  const size_t P = (size_t)Hin * Win;
  float cb = 0.f, cr = 0.f;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int oy = min(2 * p.y + dy, Hout - 1);
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int ox = min(2 * p.x + dx, Wout - 1);
      const float *px = in + (size_t)oy * Win + ox;
      float Y, Cb, Cr;
      bgr_to_ycc(k, aten_copy(px[0]), aten_copy(px[P]), aten_copy(px[2 * P]), Y, Cb, Cr);
      cb += Cb, cr += Cr;
      if (2 * p.y + dy < Hout && 2 * p.x + dx < Wout) yp[(size_t)oy * ys + ox] = (T)round_sat_u16(k.y_off + k.y_mul * Y, k.maxval);
    }
  }
  const size_t o = (size_t)p.y * cs + p.x;
  up[o] = (T)round_sat_u16(k.c_off + k.c_mul * (cb * 0.25f), k.maxval);
  vp[o] = (T)round_sat_u16(k.c_off + k.c_mul * (cr * 0.25f), k.maxval);
}
// the rows form: two window rows of four blocks per lane, as to_out_yuv_rows_body
template <class T>
__device__ __forceinline__ void to_out_yuv_crop_rows_body(const YuvOut k, const float *__restrict__ in, T *__restrict__ yp,
                                                          T *__restrict__ up, T *__restrict__ vp, int ys, int cs, int Hin, int W, int Hout) {
  const int W8 = W >> 3, Hc = (Hout + 1) >> 1;
  const size_t total = (size_t)W8 * Hc, P = (size_t)Hin * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int j = (int)(i / W8), x = (int)(i - (size_t)j * W8) * 8;
    float cb[4] = {0.f, 0.f, 0.f, 0.f}, cr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int oy = min(2 * j + r, Hout - 1);
      uint32_t q[8];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4g ch[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c] = *reinterpret_cast<const f32x4g *>(in + (size_t)c * P + (size_t)oy * W + x + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float Y, Cb, Cr;
          bgr_to_ycc(k, aten_copy(ch[0][e]), aten_copy(ch[1][e]), aten_copy(ch[2][e]), Y, Cb, Cr);
          q[4 * h + e] = round_sat_u16(k.y_off + k.y_mul * Y, k.maxval);
          cb[2 * h + (e >> 1)] += Cb, cr[2 * h + (e >> 1)] += Cr;
        }
      }
      if (2 * j + r < Hout) SampleRow<T, 8>::store(yp + (size_t)oy * ys + x, q);
    }
    uint32_t qu[4], qv[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      qu[b] = round_sat_u16(k.c_off + k.c_mul * (cb[b] * 0.25f), k.maxval);
      qv[b] = round_sat_u16(k.c_off + k.c_mul * (cr[b] * 0.25f), k.maxval);
    }
    SampleRow<T, 4>::store(up + (size_t)j * cs + (x >> 1), qu);
    SampleRow<T, 4>::store(vp + (size_t)j * cs + (x >> 1), qv);
  }
}

// ---- planar 4:2:2 and 4:4:4 (include/drba_hip.h: the drba_to_*_yuv* entries that take a layout) ------------------------------------
// Chroma at full vertical resolution: U and V are [H][ceil(W / SX)] with SX = 2 (4:2:2) or 1 (4:4:4).  A chroma row belongs to the
// luma row of the same index, so no vertical tap is taken; horizontally 4:2:2 keeps the centre-sited pair of chroma_tap and 4:4:4 reads
// the sample itself.  The way out means over the SX pixels of a pair.  All eight bodies spell their arithmetic out (contraction off,
// explicit fma): a pad / crop body and its resize sibling run the same operations on a pixel, so the two agree bit for bit at an
// unchanged size by construction, not by what hipcc settles per body (yuv_to_bgr_as).  The 4:2:0 bodies above are not touched.
__device__ __forceinline__ void bgr_to_ycc_as(const YuvOut &k, float b, float g, float r, float &Y, float &Cb, float &Cr) {
#pragma clang fp contract(off)
  b = clamp01(b), g = clamp01(g), r = clamp01(r);
  Y = __builtin_fmaf(k.kb, b, __builtin_fmaf(k.kg, g, k.kr * r));
  Cb = (b - Y) * k.cb_mul;
  Cr = (r - Y) * k.cr_mul;
}
__device__ __forceinline__ uint32_t yuv_code(float off, float mul, float v, float maxval) {
#pragma clang fp contract(off)
  return round_sat_u16(__builtin_fmaf(mul, v, off), maxval);
}
// the mean of the SX colour differences of a chroma sample (sum of SX terms, in pixel order)
template <int SX>
__device__ __forceinline__ float chroma_mean(float sum) {
  return SX == 2 ? sum * 0.5f : sum;
}

// one source pixel (sy, sx) of a 4:2:2 / 4:4:4 frame -> (B, G, R)
template <class T, int SX>
__device__ __forceinline__ void yuvl_pixel(const YuvIn &k, const T *__restrict__ yp, const T *__restrict__ up, const T *__restrict__ vp,
                                           int ys, int cs, int Wc, int sy, int sx, float (&bgr)[3]) {
  const size_t r = (size_t)sy * cs;
  float u, v;
  if constexpr (SX == 2) {
    const CTap tx = chroma_tap(sx, Wc);
    u = tx.w0 * (float)up[r + tx.i0] + tx.w1 * (float)up[r + tx.i1];  // exact: quarters of samples of at most 16 bits
    v = tx.w0 * (float)vp[r + tx.i0] + tx.w1 * (float)vp[r + tx.i1];
  } else {
    u = (float)up[r + sx], v = (float)vp[r + sx];
  }
  yuv_to_bgr_as<false>(k, (float)yp[(size_t)sy * ys + sx], u, v, bgr);
}
// eight consecutive pixels x .. x + 7 of source row sy with aligned loads: 8 luma samples, and per chroma plane the 4 samples under
// them plus their two neighbours (4:2:2: chroma_raw6 without the vertical taps) or the 8 samples themselves (4:4:4)
template <class T, int SX>
__device__ __forceinline__ void yuvl_row8(const YuvIn &k, const T *__restrict__ yp, const T *__restrict__ up, const T *__restrict__ vp,
                                          int ys, int cs, int Wc, int sy, int x, float (&px)[8][3]) {
  SampleRow<T, 8> luma;
  luma.load(yp + (size_t)sy * ys + x);
  const T *urow = up + (size_t)sy * cs, *vrow = vp + (size_t)sy * cs;
  if constexpr (SX == 2) {
    float cu[6], cv[6];
    chroma_raw6(urow, Wc, x >> 1, cu), chroma_raw6(vrow, Wc, x >> 1, cv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // the taps of pixel x + j among the six: to_inp_yuv_rows_body
      const int c0 = (j + 1) >> 1;
      const float w0 = (j & 1) ? 0.75f : 0.25f, w1 = (j & 1) ? 0.25f : 0.75f;
      yuv_to_bgr_as<false>(k, luma.sample(j), w0 * cu[c0] + w1 * cu[c0 + 1], w0 * cv[c0] + w1 * cv[c0 + 1], px[j]);
    }
  } else {
    SampleRow<T, 8> u, v;
    u.load(urow + x), v.load(vrow + x);
#pragma unroll
    for (int j = 0; j < 8; ++j) yuv_to_bgr_as<false>(k, luma.sample(j), u.sample(j), v.sample(j), px[j]);
  }
}
// 8 pixels of an output row -> the three planes (two 16-byte stores each) and the pixel-major copy
__device__ __forceinline__ void store_row8(const f32x4g (&o)[3][2], float *__restrict__ out, float *__restrict__ out_x4, size_t P, size_t at) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f32x4g *dst = reinterpret_cast<f32x4g *>(out + (size_t)c * P + at);
    dst[0] = o[c][0], dst[1] = o[c][1];
  }
  if (out_x4) {
    f32x4g *dst = reinterpret_cast<f32x4g *>(out_x4 + at * 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j] = (f32x4g){o[0][j >> 2][j & 3], o[1][j >> 2][j & 3], o[2][j >> 2][j & 3], 0.f};
  }
}

// way in, general form: to_inp_yuv_body with yuvl_pixel
template <class T, int SX>
__device__ __forceinline__ void to_inp_yuvl_body(const YuvIn k, const T *__restrict__ yp, const T *__restrict__ up, const T *__restrict__ vp,
                                                 int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,
                                                 int Hout, int Wout, float sy, float sx) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  const Lerp ly = lerp_src_aten(p.y, sy, Hin), lx = lerp_src_aten(p.x, sx, Win);
  const int Wc = (Win + SX - 1) / SX;
  float a[3], b[3], c[3], d[3];
  yuvl_pixel<T, SX>(k, yp, up, vp, ys, cs, Wc, ly.i0, lx.i0, a);
  yuvl_pixel<T, SX>(k, yp, up, vp, ys, cs, Wc, ly.i0, lx.i1, b);
  yuvl_pixel<T, SX>(k, yp, up, vp, ys, cs, Wc, ly.i1, lx.i0, c);
  yuvl_pixel<T, SX>(k, yp, up, vp, ys, cs, Wc, ly.i1, lx.i1, d);
  const size_t P = (size_t)Hout * Wout, o = (size_t)p.y * Wout + p.x;
  float v[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    v[ch] = lerp2_aten(ly, lx, a[ch], b[ch], c[ch], d[ch]);
    out[ch * P + o] = v[ch];
  }
  if (out_x4) *reinterpret_cast<f32x4g *>(out_x4 + 4 * o) = (f32x4g){v[0], v[1], v[2], 0.f};
}
// way in, rows form: eight pixels of an output row per lane from its two source rows, ONE chroma row per luma row
template <class T, int SX>
__device__ __forceinline__ void to_inp_yuvl_rows_body(const YuvIn k, const T *__restrict__ yp, const T *__restrict__ up,
                                                      const T *__restrict__ vp, int ys, int cs, float *__restrict__ out,
                                                      float *__restrict__ out_x4, int Hin, int W, int Hout, float sy) {
  const int W8 = W >> 3, Wc = W / SX;
  const size_t total = (size_t)W8 * Hout, P = (size_t)Hout * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W8), x = (int)(i - (size_t)y * W8) * 8;
    const Lerp ly = lerp_src_aten(y, sy, Hin);
    float p0[8][3], p1[8][3];
    yuvl_row8<T, SX>(k, yp, up, vp, ys, cs, Wc, ly.i0, x, p0);
    yuvl_row8<T, SX>(k, yp, up, vp, ys, cs, Wc, ly.i1, x, p1);
    f32x4g o[3][2];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c][j >> 2][j & 3] = __fmaf_rn(ly.w0, p0[j][c], __fmul_rn(ly.w1, p1[j][c]));
    store_row8(o, out, out_x4, P, (size_t)y * W + x);
  }
}
// fit = pad, way in: the converted pixel of the clamped source coordinate
template <class T, int SX>
__device__ __forceinline__ void to_inp_yuvl_pad_body(const YuvIn k, const T *__restrict__ yp, const T *__restrict__ up,
                                                     const T *__restrict__ vp, int ys, int cs, float *__restrict__ out,
                                                     float *__restrict__ out_x4, int Hin, int Win, int Hout, int Wout) {
  const Tile2D p = tile_pixel(Wout, Hout);
  if (!p.valid) return;
  float v[3];
  yuvl_pixel<T, SX>(k, yp, up, vp, ys, cs, (Win + SX - 1) / SX, min(p.y, Hin - 1), min(p.x, Win - 1), v);
  const size_t P = (size_t)Hout * Wout, o = (size_t)p.y * Wout + p.x;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch * P + o] = v[ch];
  if (out_x4) *reinterpret_cast<f32x4g *>(out_x4 + 4 * o) = (f32x4g){v[0], v[1], v[2], 0.f};
}
template <class T, int SX>
__device__ __forceinline__ void to_inp_yuvl_pad_rows_body(const YuvIn k, const T *__restrict__ yp, const T *__restrict__ up,
                                                          const T *__restrict__ vp, int ys, int cs, float *__restrict__ out,
                                                          float *__restrict__ out_x4, int Hin, int W, int Hout) {
  const int W8 = W >> 3, Wc = W / SX;
  const size_t total = (size_t)W8 * Hout, P = (size_t)Hout * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int y = (int)(i / W8), x = (int)(i - (size_t)y * W8) * 8;
    float px[8][3];
    yuvl_row8<T, SX>(k, yp, up, vp, ys, cs, Wc, min(y, Hin - 1), x, px);
    f32x4g o[3][2];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c][j >> 2][j & 3] = px[j][c];
    store_row8(o, out, out_x4, P, (size_t)y * W + x);
  }
}

// way out, general form: the SX pixels of one chroma sample per lane (a horizontal pair, or the pixel itself), so the mean stays in
// the lane; a pixel past an odd last column repeats it in the mean and is not stored.  kCrop: the window as it stands (fit = pad).
template <class T, int SX, bool kCrop>
__device__ __forceinline__ void to_out_yuvl_body(const YuvOut k, const float *__restrict__ in, T *__restrict__ yp, T *__restrict__ up,
                                                 T *__restrict__ vp, int ys, int cs, int Hin, int Win, int Hout, int Wout, float sy,
                                                 float sx) {
#pragma clang fp contract(off)
  const int Wc = (Wout + SX - 1) / SX;
  const Tile2D p = tile_pixel(Wc, Hout);
  if (!p.valid) return;
  const size_t P = (size_t)Hin * Win;
  Lerp ly;
  if constexpr (!kCrop) ly = lerp_out<Samples16>(p.y, sy, Hin, Hout);
  float cb = 0.f, cr = 0.f;
#pragma unroll
  for (int dx = 0; dx < SX; ++dx) {
    const int ox = min(SX * p.x + dx, Wout - 1);
    float ch[3];
    if constexpr (kCrop) {
      const float *px = in + (size_t)p.y * Win + ox;
      ch[0] = aten_copy(px[0]), ch[1] = aten_copy(px[P]), ch[2] = aten_copy(px[2 * P]);
    } else {
      const Lerp lx = lerp_out<Samples16>(ox, sx, Win, Wout);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float *r0 = in + c * P + (size_t)ly.i0 * Win, *r1 = in + c * P + (size_t)ly.i1 * Win;
        ch[c] = lerp2_aten(ly, lx, r0[lx.i0], r0[lx.i1], r1[lx.i0], r1[lx.i1]);
      }
    }
    float Y, Cb, Cr;
    bgr_to_ycc_as(k, ch[0], ch[1], ch[2], Y, Cb, Cr);
    cb = __fadd_rn(cb, Cb), cr = __fadd_rn(cr, Cr);
    if (SX * p.x + dx < Wout) yp[(size_t)p.y * ys + ox] = (T)yuv_code(k.y_off, k.y_mul, Y, k.maxval);
  }
  const size_t o = (size_t)p.y * cs + p.x;
  up[o] = (T)yuv_code(k.c_off, k.c_mul, chroma_mean<SX>(cb), k.maxval);
  vp[o] = (T)yuv_code(k.c_off, k.c_mul, chroma_mean<SX>(cr), k.maxval);
}
// way out, rows form: eight pixels of ONE output row per lane, 16-byte loads of the fp32 planes, one store of 8 luma samples and one
// of 4 (4:2:2) or 8 (4:4:4) samples per chroma plane
template <class T, int SX, bool kCrop>
__device__ __forceinline__ void to_out_yuvl_rows_body(const YuvOut k, const float *__restrict__ in, T *__restrict__ yp, T *__restrict__ up,
                                                      T *__restrict__ vp, int ys, int cs, int Hin, int W, int Hout, float sy) {
#pragma clang fp contract(off)
  constexpr int NC = 8 / SX;
  const int W8 = W >> 3;
  const size_t total = (size_t)W8 * Hout, P = (size_t)Hin * W;
  for (size_t i = (size_t)blockIdx.x * block_dim_x() + threadIdx.x; i < total; i += (size_t)gridDim.x * block_dim_x()) {
    const int oy = (int)(i / W8), x = (int)(i - (size_t)oy * W8) * 8;
    Lerp ly;
    if constexpr (kCrop)
      ly.i0 = ly.i1 = oy, ly.w0 = 1.f, ly.w1 = 0.f;
    else
      ly = lerp_out<Samples16>(oy, sy, Hin, Hout);
    float cb[8], cr[8];
    uint32_t q[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4g ch[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4g t = *reinterpret_cast<const f32x4g *>(in + (size_t)c * P + (size_t)ly.i0 * W + x + 4 * h);
        if constexpr (kCrop) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ch[c][e] = aten_copy(t[e]);
        } else {
          const f32x4g u = *reinterpret_cast<const f32x4g *>(in + (size_t)c * P + (size_t)ly.i1 * W + x + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e)  // the horizontal pass is ATen's copy, then the vertical lerp: to_out_yuv_rows_body
            ch[c][e] = __fmaf_rn(ly.w0, aten_copy(t[e]), __fmul_rn(ly.w1, aten_copy(u[e])));
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float Y;
        bgr_to_ycc_as(k, ch[0][e], ch[1][e], ch[2][e], Y, cb[4 * h + e], cr[4 * h + e]);
        q[4 * h + e] = yuv_code(k.y_off, k.y_mul, Y, k.maxval);
      }
    }
    SampleRow<T, 8>::store(yp + (size_t)oy * ys + x, q);
    uint32_t qu[NC], qv[NC];
#pragma unroll
    for (int b = 0; b < NC; ++b) {
      const float sb = SX == 2 ? __fadd_rn(cb[2 * b], cb[2 * b + 1]) : cb[b], sr = SX == 2 ? __fadd_rn(cr[2 * b], cr[2 * b + 1]) : cr[b];
      qu[b] = yuv_code(k.c_off, k.c_mul, chroma_mean<SX>(sb), k.maxval);
      qv[b] = yuv_code(k.c_off, k.c_mul, chroma_mean<SX>(sr), k.maxval);
    }
    SampleRow<T, NC>::store(up + (size_t)oy * cs + x / SX, qu);
    SampleRow<T, NC>::store(vp + (size_t)oy * cs + x / SX, qv);
  }
}

DRBA_FRAME_KERNEL to_inp_yuv_pad_kernel(YuvIn k, const uint8_t *__restrict__ y, const uint8_t *__restrict__ u, const uint8_t *__restrict__ v,
                                        int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win, int Hout,
                                        int Wout) {
  to_inp_yuv_pad_body(k, y, u, v, ys, cs, out, out_x4, Hin, Win, Hout, Wout);
}
DRBA_FRAME_KERNEL to_inp16_yuv_pad_kernel(YuvIn k, const uint16_t *__restrict__ y, const uint16_t *__restrict__ u,
                                          const uint16_t *__restrict__ v, int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4,
                                          int Hin, int Win, int Hout, int Wout) {
  to_inp_yuv_pad_body(k, y, u, v, ys, cs, out, out_x4, Hin, Win, Hout, Wout);
}
DRBA_FRAME_KERNEL to_inp_yuv_pad_rows_kernel(YuvIn k, const uint8_t *__restrict__ y, const uint8_t *__restrict__ u,
                                             const uint8_t *__restrict__ v, int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4,
                                             int Hin, int W, int Hout) {
  to_inp_yuv_pad_rows_body(k, y, u, v, ys, cs, out, out_x4, Hin, W, Hout);
}
DRBA_FRAME_KERNEL to_inp16_yuv_pad_rows_kernel(YuvIn k, const uint16_t *__restrict__ y, const uint16_t *__restrict__ u,
                                               const uint16_t *__restrict__ v, int ys, int cs, float *__restrict__ out,
                                               float *__restrict__ out_x4, int Hin, int W, int Hout) {
  to_inp_yuv_pad_rows_body(k, y, u, v, ys, cs, out, out_x4, Hin, W, Hout);
}
DRBA_FRAME_KERNEL to_out_yuv_crop_kernel(YuvOut k, const float *__restrict__ in, uint8_t *__restrict__ y, uint8_t *__restrict__ u,
                                         uint8_t *__restrict__ v, int ys, int cs, int Hin, int Win, int Hout, int Wout) {
  to_out_yuv_crop_body(k, in, y, u, v, ys, cs, Hin, Win, Hout, Wout);
}
DRBA_FRAME_KERNEL to_out16_yuv_crop_kernel(YuvOut k, const float *__restrict__ in, uint16_t *__restrict__ y, uint16_t *__restrict__ u,
                                           uint16_t *__restrict__ v, int ys, int cs, int Hin, int Win, int Hout, int Wout) {
  to_out_yuv_crop_body(k, in, y, u, v, ys, cs, Hin, Win, Hout, Wout);
}
DRBA_FRAME_KERNEL to_out_yuv_crop_rows_kernel(YuvOut k, const float *__restrict__ in, uint8_t *__restrict__ y, uint8_t *__restrict__ u,
                                              uint8_t *__restrict__ v, int ys, int cs, int Hin, int W, int Hout) {
  to_out_yuv_crop_rows_body(k, in, y, u, v, ys, cs, Hin, W, Hout);
}
DRBA_FRAME_KERNEL to_out16_yuv_crop_rows_kernel(YuvOut k, const float *__restrict__ in, uint16_t *__restrict__ y, uint16_t *__restrict__ u,
                                                uint16_t *__restrict__ v, int ys, int cs, int Hin, int W, int Hout) {
  to_out_yuv_crop_rows_body(k, in, y, u, v, ys, cs, Hin, W, Hout);
}
DRBA_FRAME_KERNEL to_inp_yuv_kernel(YuvIn k, const uint8_t *__restrict__ y, const uint8_t *__restrict__ u, const uint8_t *__restrict__ v, int ys,
                                    int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win, int Hout, int Wout, float sy,
                                    float sx) {
  to_inp_yuv_body(k, y, u, v, ys, cs, out, out_x4, Hin, Win, Hout, Wout, sy, sx);
}
DRBA_FRAME_KERNEL to_inp16_yuv_kernel(YuvIn k, const uint16_t *__restrict__ y, const uint16_t *__restrict__ u, const uint16_t *__restrict__ v,
                                      int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win, int Hout, int Wout,
                                      float sy, float sx) {
  to_inp_yuv_body(k, y, u, v, ys, cs, out, out_x4, Hin, Win, Hout, Wout, sy, sx);
}
DRBA_FRAME_KERNEL to_inp_yuv_rows_kernel(YuvIn k, const uint8_t *__restrict__ y, const uint8_t *__restrict__ u, const uint8_t *__restrict__ v,
                                         int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int W, int Hout, float sy) {
  to_inp_yuv_rows_body(k, y, u, v, ys, cs, out, out_x4, Hin, W, Hout, sy);
}
DRBA_FRAME_KERNEL to_inp16_yuv_rows_kernel(YuvIn k, const uint16_t *__restrict__ y, const uint16_t *__restrict__ u,
                                           const uint16_t *__restrict__ v, int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4,
                                           int Hin, int W, int Hout, float sy) {
  to_inp_yuv_rows_body(k, y, u, v, ys, cs, out, out_x4, Hin, W, Hout, sy);
}
DRBA_FRAME_KERNEL to_out_yuv_kernel(YuvOut k, const float *__restrict__ in, uint8_t *__restrict__ y, uint8_t *__restrict__ u,
                                    uint8_t *__restrict__ v, int ys, int cs, int Hin, int Win, int Hout, int Wout, float sy, float sx) {
  to_out_yuv_body(k, in, y, u, v, ys, cs, Hin, Win, Hout, Wout, sy, sx);
}
DRBA_FRAME_KERNEL to_out16_yuv_kernel(YuvOut k, const float *__restrict__ in, uint16_t *__restrict__ y, uint16_t *__restrict__ u,
                                      uint16_t *__restrict__ v, int ys, int cs, int Hin, int Win, int Hout, int Wout, float sy, float sx) {
  to_out_yuv_body(k, in, y, u, v, ys, cs, Hin, Win, Hout, Wout, sy, sx);
}
DRBA_FRAME_KERNEL to_out_yuv_rows_kernel(YuvOut k, const float *__restrict__ in, uint8_t *__restrict__ y, uint8_t *__restrict__ u,
                                         uint8_t *__restrict__ v, int ys, int cs, int Hin, int W, int Hout, float sy) {
  to_out_yuv_rows_body(k, in, y, u, v, ys, cs, Hin, W, Hout, sy);
}
DRBA_FRAME_KERNEL to_out16_yuv_rows_kernel(YuvOut k, const float *__restrict__ in, uint16_t *__restrict__ y, uint16_t *__restrict__ u,
                                           uint16_t *__restrict__ v, int ys, int cs, int Hin, int W, int Hout, float sy) {
  to_out_yuv_rows_body(k, in, y, u, v, ys, cs, Hin, W, Hout, sy);
}
// 4:2:2 and 4:4:4: the eight kernels of a (depth, layout) pair; D is empty or 16, L the layout's name, SX its horizontal factor
#define DRBA_YUVL_KERNELS(D, T, L, SX)                                                                                                    \
  DRBA_FRAME_KERNEL to_inp##D##_yuv##L##_kernel(YuvIn k, const T *__restrict__ y, const T *__restrict__ u, const T *__restrict__ v,      \
                                                int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin, int Win,  \
                                                int Hout, int Wout, float sy, float sx) {                                               \
    to_inp_yuvl_body<T, SX>(k, y, u, v, ys, cs, out, out_x4, Hin, Win, Hout, Wout, sy, sx);                                               \
  }                                                                                                                                       \
  DRBA_FRAME_KERNEL to_inp##D##_yuv##L##_rows_kernel(YuvIn k, const T *__restrict__ y, const T *__restrict__ u, const T *__restrict__ v, \
                                                     int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin,      \
                                                     int W, int Hout, float sy) {                                                       \
    to_inp_yuvl_rows_body<T, SX>(k, y, u, v, ys, cs, out, out_x4, Hin, W, Hout, sy);                                                      \
  }                                                                                                                                       \
  DRBA_FRAME_KERNEL to_inp##D##_yuv##L##_pad_kernel(YuvIn k, const T *__restrict__ y, const T *__restrict__ u, const T *__restrict__ v,  \
                                                    int ys, int cs, float *__restrict__ out, float *__restrict__ out_x4, int Hin,       \
                                                    int Win, int Hout, int Wout) {                                                      \
    to_inp_yuvl_pad_body<T, SX>(k, y, u, v, ys, cs, out, out_x4, Hin, Win, Hout, Wout);                                                   \
  }                                                                                                                                       \
  DRBA_FRAME_KERNEL to_inp##D##_yuv##L##_pad_rows_kernel(YuvIn k, const T *__restrict__ y, const T *__restrict__ u,                      \
                                                         const T *__restrict__ v, int ys, int cs, float *__restrict__ out,              \
                                                         float *__restrict__ out_x4, int Hin, int W, int Hout) {                        \
    to_inp_yuvl_pad_rows_body<T, SX>(k, y, u, v, ys, cs, out, out_x4, Hin, W, Hout);                                                      \
  }                                                                                                                                       \
  DRBA_FRAME_KERNEL to_out##D##_yuv##L##_kernel(YuvOut k, const float *__restrict__ in, T *__restrict__ y, T *__restrict__ u,            \
                                                T *__restrict__ v, int ys, int cs, int Hin, int Win, int Hout, int Wout, float sy,      \
                                                float sx) {                                                                             \
    to_out_yuvl_body<T, SX, false>(k, in, y, u, v, ys, cs, Hin, Win, Hout, Wout, sy, sx);                                                 \
  }                                                                                                                                       \
  DRBA_FRAME_KERNEL to_out##D##_yuv##L##_rows_kernel(YuvOut k, const float *__restrict__ in, T *__restrict__ y, T *__restrict__ u,       \
                                                     T *__restrict__ v, int ys, int cs, int Hin, int W, int Hout, float sy) {           \
    to_out_yuvl_rows_body<T, SX, false>(k, in, y, u, v, ys, cs, Hin, W, Hout, sy);                                                        \
  }                                                                                                                                       \
  DRBA_FRAME_KERNEL to_out##D##_yuv##L##_crop_kernel(YuvOut k, const float *__restrict__ in, T *__restrict__ y, T *__restrict__ u,       \
                                                     T *__restrict__ v, int ys, int cs, int Hin, int Win, int Hout, int Wout) {         \
    to_out_yuvl_body<T, SX, true>(k, in, y, u, v, ys, cs, Hin, Win, Hout, Wout, 1.f, 1.f);                                                \
  }                                                                                                                                       \
  DRBA_FRAME_KERNEL to_out##D##_yuv##L##_crop_rows_kernel(YuvOut k, const float *__restrict__ in, T *__restrict__ y,                     \
                                                          T *__restrict__ u, T *__restrict__ v, int ys, int cs, int Hin, int W,         \
                                                          int Hout) {                                                                   \
    to_out_yuvl_rows_body<T, SX, true>(k, in, y, u, v, ys, cs, Hin, W, Hout, 1.f);                                                        \
  }
DRBA_YUVL_KERNELS(, uint8_t, 422, 2)
DRBA_YUVL_KERNELS(16, uint16_t, 422, 2)
DRBA_YUVL_KERNELS(, uint8_t, 444, 1)
DRBA_YUVL_KERNELS(16, uint16_t, 444, 1)
#undef DRBA_YUVL_KERNELS
#undef DRBA_FRAME_KERNEL

// ---- launch helpers: one per operation; M... is empty for bytes and (float maxval) for 16-bit samples ---------------------------
// The rows form needs an unchanged width that is a multiple of 4, 16-byte aligned fp32 rows and the samples of four pixels aligned
// to their load / store word: 4 bytes for bytes, 8 for 16-bit samples.
// (The launch trace names a kernel by its address, so it reads the same as when the entries launched their kernels by name; only
// DRBA_LAUNCH's textual fallback for an address without a name would now read `one` / `rows` / `kernel`.)
template <class T>
bool rows_form_ok(int Win, int Wout, float scale_x, const T *samples, const float *planes, size_t pitch) {
  return Win == Wout && scale_x == 1.f && (Wout & 3) == 0 && (pitch & 3) == 0 &&
         (((uintptr_t)samples & (4 * sizeof(T) - 1)) | ((uintptr_t)planes & 15)) == 0;
}
// `pitch`: samples from one row of the packed frame to the next.  The entries without one pass 3 * W (rows without padding); the
// windowed entries (drba_*_win*) the pitch of the frame their rectangle lies in, which must hold a row of the rectangle.
bool pitch_ok(int pitch, int W) { return pitch > 0 && (size_t)pitch >= 3 * (size_t)W; }

template <class T, class... M>
int to_inp_launch(void (*one)(const T *, float *, float *, int, int, int, int, float, float, size_t, M...),
                  void (*rows)(const T *, float *, float *, int, int, int, float, size_t, M...), const T *img_hwc, int pitch, float *out,
                  float *out_x4, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x, void *stream, M... maxval) {
  if (!img_hwc || !out || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || ((uintptr_t)out_x4 & 15) != 0 || !pitch_ok(pitch, Win))
    return DRBA_EINVAL;
  if (rows_form_ok(Win, Wout, scale_x, img_hwc, out, pitch))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 2) * Hout)), dim3(kBlock), 0, (hipStream_t)stream, img_hwc, out, out_x4, Hin, Wout,
                Hout, scale_y, (size_t)pitch, maxval...);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wout, Hout)), dim3(kBlock), 0, (hipStream_t)stream, img_hwc, out, out_x4, Hin, Win, Hout, Wout, scale_y,
                scale_x, (size_t)pitch, maxval...);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

template <class T, class... M>
int to_out_launch(void (*one)(const float *, T *, int, int, int, int, float, float, int, size_t, M...),
                  void (*rows)(const float *, T *, int, int, int, float, int, size_t, M...), const float *in, T *out_hwc, int pitch, int Hin,
                  int Win, int Hout, int Wout, float scale_y, float scale_x, int reverse_channels, void *stream, M... maxval) {
  if (!in || !out_hwc || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || !pitch_ok(pitch, Wout)) return DRBA_EINVAL;
  if (rows_form_ok(Win, Wout, scale_x, out_hwc, in, pitch))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 2) * Hout)), dim3(kBlock), 0, (hipStream_t)stream, in, out_hwc, Hin, Wout, Hout,
                scale_y, reverse_channels, (size_t)pitch, maxval...);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wout, Hout)), dim3(kBlock), 0, (hipStream_t)stream, in, out_hwc, Hin, Win, Hout, Wout, scale_y,
                scale_x, reverse_channels, (size_t)pitch, maxval...);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

// fit = pad: the network tensor is at least the frame (way in) and the frame at most the network tensor (way out); the rows form
// under the same rule as above, the width being unchanged where only rows are added or dropped
template <class T, class... M>
int to_inp_pad_launch(void (*one)(const T *, float *, float *, int, int, int, int, size_t, M...),
                      void (*rows)(const T *, float *, float *, int, int, int, size_t, M...), const T *img_hwc, int pitch, float *out,
                      float *out_x4, int Hin, int Win, int Hout, int Wout, void *stream, M... maxval) {
  if (!img_hwc || !out || Hin <= 0 || Win <= 0 || Hout < Hin || Wout < Win || ((uintptr_t)out_x4 & 15) != 0 || !pitch_ok(pitch, Win))
    return DRBA_EINVAL;
  if (rows_form_ok(Win, Wout, 1.f, img_hwc, out, pitch))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 2) * Hout)), dim3(kBlock), 0, (hipStream_t)stream, img_hwc, out, out_x4, Hin, Wout,
                Hout, (size_t)pitch, maxval...);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wout, Hout)), dim3(kBlock), 0, (hipStream_t)stream, img_hwc, out, out_x4, Hin, Win, Hout, Wout,
                (size_t)pitch, maxval...);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

template <class T, class... M>
int to_out_crop_launch(void (*one)(const float *, T *, int, int, int, int, int, size_t, M...),
                       void (*rows)(const float *, T *, int, int, int, int, size_t, M...), const float *in, T *out_hwc, int pitch, int Hin,
                       int Win, int Hout, int Wout, int reverse_channels, void *stream, M... maxval) {
  if (!in || !out_hwc || Hout <= 0 || Wout <= 0 || Hout > Hin || Wout > Win || !pitch_ok(pitch, Wout)) return DRBA_EINVAL;
  if (rows_form_ok(Win, Wout, 1.f, out_hwc, in, pitch))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 2) * Hout)), dim3(kBlock), 0, (hipStream_t)stream, in, out_hwc, Hin, Wout, Hout,
                reverse_channels, (size_t)pitch, maxval...);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wout, Hout)), dim3(kBlock), 0, (hipStream_t)stream, in, out_hwc, Hin, Win, Hout, Wout, reverse_channels,
                (size_t)pitch, maxval...);
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

// ---- planar 4:2:0: constants and launch helpers -----------------------------------------------------------------------------------
// m = maxval (255 | 1023 | ...), k = (m + 1) / 256: limited range is Y in [16k, 235k], chroma 128k +- 112k; full range divides
// by m.  matrix 0 = bt709, 1 = bt601.
bool yuv_coeffs(int matrix, double &kr, double &kb) {
  if (matrix == 0) kr = 0.2126, kb = 0.0722;
  else if (matrix == 1) kr = 0.299, kb = 0.114;
  else return false;
  return true;
}
YuvIn yuv_in_consts(double kr, double kb, int full_range, double m) {
  const double k = (m + 1.0) / 256.0, kg = 1.0 - kr - kb;
  YuvIn c;
  c.y_off = (float)(full_range ? 0.0 : 16.0 * k), c.y_mul = (float)(1.0 / (full_range ? m : 219.0 * k));
  c.c_off = (float)(128.0 * k), c.c_mul = (float)(1.0 / (full_range ? m : 224.0 * k));
  c.r_cr = (float)(2.0 * (1.0 - kr)), c.b_cb = (float)(2.0 * (1.0 - kb));
  c.kr = (float)kr, c.kb = (float)kb, c.inv_kg = (float)(1.0 / kg);
  return c;
}
YuvOut yuv_out_consts(double kr, double kb, int full_range, double m) {
  const double k = (m + 1.0) / 256.0;
  YuvOut c;
  c.kr = (float)kr, c.kg = (float)(1.0 - kr - kb), c.kb = (float)kb;
  c.cb_mul = (float)(1.0 / (2.0 * (1.0 - kb))), c.cr_mul = (float)(1.0 / (2.0 * (1.0 - kr)));
  c.y_off = (float)(full_range ? 0.0 : 16.0 * k), c.y_mul = (float)(full_range ? m : 219.0 * k);
  c.c_off = (float)(128.0 * k), c.c_mul = (float)(full_range ? m : 224.0 * k);
  c.maxval = (float)m;
  return c;
}
// The rows form: an unchanged width that is a multiple of 8, luma rows aligned to 8 samples and chroma rows to the 8 / subx samples
// under them -- 4 for 4:2:0 and 4:2:2, 8 for 4:4:4 -- (pointers and strides), 16-byte aligned fp32 rows.
template <class T>
bool yuv_rows_form_ok(int Win, int Wout, float scale_x, const T *y, const T *u, const T *v, int ys, int cs, const float *planes,
                      int subx = 2) {
  const int nc = 8 / subx;
  return Win == Wout && scale_x == 1.f && (Wout & 7) == 0 && (ys & 7) == 0 && (cs & (nc - 1)) == 0 &&
         (((uintptr_t)y & (8 * sizeof(T) - 1)) | (((uintptr_t)u | (uintptr_t)v) & (nc * sizeof(T) - 1)) | ((uintptr_t)planes & 15)) == 0;
}
template <class T>
bool yuv_args_ok(const T *y, const T *u, const T *v, int ys, int cs, const float *planes, int Hin, int Win, int Hout, int Wout, int H, int W,
                 float maxval, int subx = 2) {
  // (H, W): the size of the planar frame, which the strides must hold (a chroma row is ceil(W / subx) samples); every plane aligned
  // to its sample
  return y && u && v && planes && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && ys >= W && cs >= (W + subx - 1) / subx && H > 0 &&
         (((uintptr_t)y | (uintptr_t)u | (uintptr_t)v) & (sizeof(T) - 1)) == 0 && (sizeof(T) == 1 || maxval_ok(maxval));
}

template <class T>
int to_inp_yuv_launch(void (*one)(YuvIn, const T *, const T *, const T *, int, int, float *, float *, int, int, int, int, float, float),
                      void (*rows)(YuvIn, const T *, const T *, const T *, int, int, float *, float *, int, int, int, float), const T *y,
                      const T *u, const T *v, int ys, int cs, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, float scale_y,
                      float scale_x, int matrix, int full_range, float maxval, void *stream, int subx = 2) {
  double kr, kb;
  if (!yuv_args_ok(y, u, v, ys, cs, out, Hin, Win, Hout, Wout, Hin, Win, maxval, subx) || ((uintptr_t)out_x4 & 15) != 0 ||
      !yuv_coeffs(matrix, kr, kb))
    return DRBA_EINVAL;
  const YuvIn k = yuv_in_consts(kr, kb, full_range, maxval);
  if (yuv_rows_form_ok(Win, Wout, scale_x, y, u, v, ys, cs, out, subx))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 3) * Hout)), dim3(kBlock), 0, (hipStream_t)stream, k, y, u, v, ys, cs, out, out_x4, Hin,
                Wout, Hout, scale_y);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wout, Hout)), dim3(kBlock), 0, (hipStream_t)stream, k, y, u, v, ys, cs, out, out_x4, Hin, Win, Hout, Wout,
                scale_y, scale_x);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

template <class T>
int to_out_yuv_launch(void (*one)(YuvOut, const float *, T *, T *, T *, int, int, int, int, int, int, float, float),
                      void (*rows)(YuvOut, const float *, T *, T *, T *, int, int, int, int, int, float), const float *in, T *y, T *u, T *v,
                      int ys, int cs, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x, int matrix, int full_range,
                      float maxval, void *stream, int subx = 2, int suby = 2) {
  double kr, kb;
  if (!yuv_args_ok(y, u, v, ys, cs, in, Hin, Win, Hout, Wout, Hout, Wout, maxval, subx) || !yuv_coeffs(matrix, kr, kb)) return DRBA_EINVAL;
  const YuvOut k = yuv_out_consts(kr, kb, full_range, maxval);
  const int Hc = (Hout + suby - 1) / suby, Wc = (Wout + subx - 1) / subx;  // a lane takes the pixels of one chroma sample (general form)
  if (yuv_rows_form_ok(Win, Wout, scale_x, y, u, v, ys, cs, in, subx))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 3) * Hc)), dim3(kBlock), 0, (hipStream_t)stream, k, in, y, u, v, ys, cs, Hin, Wout, Hout,
                scale_y);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wc, Hc)), dim3(kBlock), 0, (hipStream_t)stream, k, in, y, u, v, ys, cs, Hin, Win, Hout, Wout, scale_y,
                scale_x);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

// fit = pad, planar
template <class T>
int to_inp_yuv_pad_launch(void (*one)(YuvIn, const T *, const T *, const T *, int, int, float *, float *, int, int, int, int),
                          void (*rows)(YuvIn, const T *, const T *, const T *, int, int, float *, float *, int, int, int), const T *y,
                          const T *u, const T *v, int ys, int cs, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, int matrix,
                          int full_range, float maxval, void *stream, int subx = 2) {
  double kr, kb;
  if (!yuv_args_ok(y, u, v, ys, cs, out, Hin, Win, Hout, Wout, Hin, Win, maxval, subx) || Hout < Hin || Wout < Win ||
      ((uintptr_t)out_x4 & 15) != 0 || !yuv_coeffs(matrix, kr, kb))
    return DRBA_EINVAL;
  const YuvIn k = yuv_in_consts(kr, kb, full_range, maxval);
  if (yuv_rows_form_ok(Win, Wout, 1.f, y, u, v, ys, cs, out, subx))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 3) * Hout)), dim3(kBlock), 0, (hipStream_t)stream, k, y, u, v, ys, cs, out, out_x4, Hin,
                Wout, Hout);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wout, Hout)), dim3(kBlock), 0, (hipStream_t)stream, k, y, u, v, ys, cs, out, out_x4, Hin, Win, Hout, Wout);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

template <class T>
int to_out_yuv_crop_launch(void (*one)(YuvOut, const float *, T *, T *, T *, int, int, int, int, int, int),
                           void (*rows)(YuvOut, const float *, T *, T *, T *, int, int, int, int, int), const float *in, T *y, T *u, T *v,
                           int ys, int cs, int Hin, int Win, int Hout, int Wout, int matrix, int full_range, float maxval, void *stream,
                           int subx = 2, int suby = 2) {
  double kr, kb;
  if (!yuv_args_ok(y, u, v, ys, cs, in, Hin, Win, Hout, Wout, Hout, Wout, maxval, subx) || Hout > Hin || Wout > Win ||
      !yuv_coeffs(matrix, kr, kb))
    return DRBA_EINVAL;
  const YuvOut k = yuv_out_consts(kr, kb, full_range, maxval);
  const int Hc = (Hout + suby - 1) / suby, Wc = (Wout + subx - 1) / subx;
  if (yuv_rows_form_ok(Win, Wout, 1.f, y, u, v, ys, cs, in, subx))
    DRBA_LAUNCH(rows, dim3(grid_for((size_t)(Wout >> 3) * Hc)), dim3(kBlock), 0, (hipStream_t)stream, k, in, y, u, v, ys, cs, Hin, Wout, Hout);
  else
    DRBA_LAUNCH(one, dim3(tiles_for(Wc, Hc)), dim3(kBlock), 0, (hipStream_t)stream, k, in, y, u, v, ys, cs, Hin, Win, Hout, Wout);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

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
  return to_inp_launch(to_inp_kernel, to_inp_rows_kernel, img_hwc, 3 * Win, out, out_x4, Hin, Win, Hout, Wout, scale_y, scale_x, stream);
}

int drba_to_inp(const uint8_t *img_hwc, float *out, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                void *stream) {
  return drba_to_inp_x4(img_hwc, out, nullptr, Hin, Win, Hout, Wout, scale_y, scale_x, stream);
}

int drba_to_out(const float *in, uint8_t *out_hwc, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                int reverse_channels, void *stream) {
  return to_out_launch(to_out_kernel, to_out_rows_kernel, in, out_hwc, 3 * Wout, Hin, Win, Hout, Wout, scale_y, scale_x, reverse_channels, stream);
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
  return to_inp_launch(to_inp16_kernel, to_inp16_rows_kernel, img_hwc, 3 * Win, out, out_x4, Hin, Win, Hout, Wout, scale_y, scale_x, stream, maxval);
}

int drba_to_out16(const float *in, uint16_t *out_hwc, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                  int reverse_channels, float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)out_hwc & 1) != 0) return DRBA_EINVAL;
  return to_out_launch(to_out16_kernel, to_out16_rows_kernel, in, out_hwc, 3 * Wout, Hin, Win, Hout, Wout, scale_y, scale_x, reverse_channels,
                       stream, maxval);
}

int drba_to_inp_yuv420_x4(const uint8_t *y, const uint8_t *u, const uint8_t *v, int y_stride, int c_stride, float *out, float *out_x4, int Hin,
                          int Win, int Hout, int Wout, float scale_y, float scale_x, int matrix, int full_range, void *stream) {
  return to_inp_yuv_launch(to_inp_yuv_kernel, to_inp_yuv_rows_kernel, y, u, v, y_stride, c_stride, out, out_x4, Hin, Win, Hout, Wout, scale_y,
                           scale_x, matrix, full_range, 255.f, stream);
}

int drba_to_inp16_yuv420_x4(const uint16_t *y, const uint16_t *u, const uint16_t *v, int y_stride, int c_stride, float *out, float *out_x4,
                            int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x, int matrix, int full_range, float maxval,
                            void *stream) {
  return to_inp_yuv_launch(to_inp16_yuv_kernel, to_inp16_yuv_rows_kernel, y, u, v, y_stride, c_stride, out, out_x4, Hin, Win, Hout, Wout,
                           scale_y, scale_x, matrix, full_range, maxval, stream);
}

int drba_to_out_yuv420(const float *in, uint8_t *y, uint8_t *u, uint8_t *v, int y_stride, int c_stride, int Hin, int Win, int Hout, int Wout,
                       float scale_y, float scale_x, int matrix, int full_range, void *stream) {
  return to_out_yuv_launch(to_out_yuv_kernel, to_out_yuv_rows_kernel, in, y, u, v, y_stride, c_stride, Hin, Win, Hout, Wout, scale_y, scale_x,
                           matrix, full_range, 255.f, stream);
}

int drba_to_out16_yuv420(const float *in, uint16_t *y, uint16_t *u, uint16_t *v, int y_stride, int c_stride, int Hin, int Win, int Hout,
                         int Wout, float scale_y, float scale_x, int matrix, int full_range, float maxval, void *stream) {
  return to_out_yuv_launch(to_out16_yuv_kernel, to_out16_yuv_rows_kernel, in, y, u, v, y_stride, c_stride, Hin, Win, Hout, Wout, scale_y,
                           scale_x, matrix, full_range, maxval, stream);
}

// ---- fit = pad: each entry takes its resize sibling's arguments without the two scale factors -----------------------------------
int drba_to_inp_pad_x4(const uint8_t *img_hwc, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, void *stream) {
  return to_inp_pad_launch(to_inp_pad_kernel, to_inp_pad_rows_kernel, img_hwc, 3 * Win, out, out_x4, Hin, Win, Hout, Wout, stream);
}

int drba_to_inp16_pad_x4(const uint16_t *img_hwc, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)img_hwc & 1) != 0) return DRBA_EINVAL;
  return to_inp_pad_launch(to_inp16_pad_kernel, to_inp16_pad_rows_kernel, img_hwc, 3 * Win, out, out_x4, Hin, Win, Hout, Wout, stream, maxval);
}

int drba_to_out_crop(const float *in, uint8_t *out_hwc, int Hin, int Win, int Hout, int Wout, int reverse_channels, void *stream) {
  return to_out_crop_launch(to_out_crop_kernel, to_out_crop_rows_kernel, in, out_hwc, 3 * Wout, Hin, Win, Hout, Wout, reverse_channels, stream);
}

int drba_to_out16_crop(const float *in, uint16_t *out_hwc, int Hin, int Win, int Hout, int Wout, int reverse_channels, float maxval,
                       void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)out_hwc & 1) != 0) return DRBA_EINVAL;
  return to_out_crop_launch(to_out16_crop_kernel, to_out16_crop_rows_kernel, in, out_hwc, 3 * Wout, Hin, Win, Hout, Wout, reverse_channels, stream,
                            maxval);
}

int drba_to_inp_yuv420_pad_x4(const uint8_t *y, const uint8_t *u, const uint8_t *v, int y_stride, int c_stride, float *out, float *out_x4,
                              int Hin, int Win, int Hout, int Wout, int matrix, int full_range, void *stream) {
  return to_inp_yuv_pad_launch(to_inp_yuv_pad_kernel, to_inp_yuv_pad_rows_kernel, y, u, v, y_stride, c_stride, out, out_x4, Hin, Win, Hout, Wout,
                               matrix, full_range, 255.f, stream);
}

int drba_to_inp16_yuv420_pad_x4(const uint16_t *y, const uint16_t *u, const uint16_t *v, int y_stride, int c_stride, float *out, float *out_x4,
                                int Hin, int Win, int Hout, int Wout, int matrix, int full_range, float maxval, void *stream) {
  return to_inp_yuv_pad_launch(to_inp16_yuv_pad_kernel, to_inp16_yuv_pad_rows_kernel, y, u, v, y_stride, c_stride, out, out_x4, Hin, Win, Hout,
                               Wout, matrix, full_range, maxval, stream);
}

int drba_to_out_yuv420_crop(const float *in, uint8_t *y, uint8_t *u, uint8_t *v, int y_stride, int c_stride, int Hin, int Win, int Hout,
                            int Wout, int matrix, int full_range, void *stream) {
  return to_out_yuv_crop_launch(to_out_yuv_crop_kernel, to_out_yuv_crop_rows_kernel, in, y, u, v, y_stride, c_stride, Hin, Win, Hout, Wout,
                                matrix, full_range, 255.f, stream);
}

int drba_to_out16_yuv420_crop(const float *in, uint16_t *y, uint16_t *u, uint16_t *v, int y_stride, int c_stride, int Hin, int Win, int Hout,
                              int Wout, int matrix, int full_range, float maxval, void *stream) {
  return to_out_yuv_crop_launch(to_out16_yuv_crop_kernel, to_out16_yuv_crop_rows_kernel, in, y, u, v, y_stride, c_stride, Hin, Win, Hout, Wout,
                                matrix, full_range, maxval, stream);
}

// ---- a window of a packed frame (--crop): the eight packed entries above with the frame's row pitch -----------------------------------
// `img_hwc` / `out_hwc` point at the window's first sample, `pitch` counts the samples from one row of the FRAME to the next
// (>= 3 * the window's width, otherwise DRBA_EINVAL); the window is converted exactly as a frame of its own size: same kernels, the
// clamps at its edges.  The rows form also asks for pitch % 4 == 0, so that every row of the window is aligned as its first.
int drba_to_inp_win_x4(const uint8_t *img_hwc, int pitch, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, float scale_y,
                       float scale_x, void *stream) {
  return to_inp_launch(to_inp_kernel, to_inp_rows_kernel, img_hwc, pitch, out, out_x4, Hin, Win, Hout, Wout, scale_y, scale_x, stream);
}

int drba_to_inp16_win_x4(const uint16_t *img_hwc, int pitch, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, float scale_y,
                         float scale_x, float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)img_hwc & 1) != 0) return DRBA_EINVAL;
  return to_inp_launch(to_inp16_kernel, to_inp16_rows_kernel, img_hwc, pitch, out, out_x4, Hin, Win, Hout, Wout, scale_y, scale_x, stream,
                       maxval);
}

int drba_to_out_win(const float *in, uint8_t *out_hwc, int pitch, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                    int reverse_channels, void *stream) {
  return to_out_launch(to_out_kernel, to_out_rows_kernel, in, out_hwc, pitch, Hin, Win, Hout, Wout, scale_y, scale_x, reverse_channels,
                       stream);
}

int drba_to_out16_win(const float *in, uint16_t *out_hwc, int pitch, int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x,
                      int reverse_channels, float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)out_hwc & 1) != 0) return DRBA_EINVAL;
  return to_out_launch(to_out16_kernel, to_out16_rows_kernel, in, out_hwc, pitch, Hin, Win, Hout, Wout, scale_y, scale_x, reverse_channels,
                       stream, maxval);
}

int drba_to_inp_pad_win_x4(const uint8_t *img_hwc, int pitch, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout, void *stream) {
  return to_inp_pad_launch(to_inp_pad_kernel, to_inp_pad_rows_kernel, img_hwc, pitch, out, out_x4, Hin, Win, Hout, Wout, stream);
}

int drba_to_inp16_pad_win_x4(const uint16_t *img_hwc, int pitch, float *out, float *out_x4, int Hin, int Win, int Hout, int Wout,
                             float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)img_hwc & 1) != 0) return DRBA_EINVAL;
  return to_inp_pad_launch(to_inp16_pad_kernel, to_inp16_pad_rows_kernel, img_hwc, pitch, out, out_x4, Hin, Win, Hout, Wout, stream, maxval);
}

int drba_to_out_crop_win(const float *in, uint8_t *out_hwc, int pitch, int Hin, int Win, int Hout, int Wout, int reverse_channels,
                         void *stream) {
  return to_out_crop_launch(to_out_crop_kernel, to_out_crop_rows_kernel, in, out_hwc, pitch, Hin, Win, Hout, Wout, reverse_channels, stream);
}

int drba_to_out16_crop_win(const float *in, uint16_t *out_hwc, int pitch, int Hin, int Win, int Hout, int Wout, int reverse_channels,
                           float maxval, void *stream) {
  if (!maxval_ok(maxval) || ((uintptr_t)out_hwc & 1) != 0) return DRBA_EINVAL;
  return to_out_crop_launch(to_out16_crop_kernel, to_out16_crop_rows_kernel, in, out_hwc, pitch, Hin, Win, Hout, Wout, reverse_channels,
                            stream, maxval);
}

// ---- planar frames by layout: 420 (the entries above), 422, 444; anything else is DRBA_EINVAL ---------------------------------------
#define DRBA_BY_LAYOUT(launch, D, one, rows, ...)                                                                  \
  switch (layout) {                                                                                               \
    case 420: return launch(one(D, 420), rows(D, 420), __VA_ARGS__, 2, 2);                                         \
    case 422: return launch(one(D, 422), rows(D, 422), __VA_ARGS__, 2, 1);                                         \
    case 444: return launch(one(D, 444), rows(D, 444), __VA_ARGS__, 1, 1);                                         \
    default: return DRBA_EINVAL;                                                                                  \
  }
#define DRBA_BY_LAYOUT_IN(launch, D, one, rows, ...)                                                               \
  switch (layout) {                                                                                               \
    case 420: return launch(one(D, 420), rows(D, 420), __VA_ARGS__, 2);                                            \
    case 422: return launch(one(D, 422), rows(D, 422), __VA_ARGS__, 2);                                            \
    case 444: return launch(one(D, 444), rows(D, 444), __VA_ARGS__, 1);                                            \
    default: return DRBA_EINVAL;                                                                                  \
  }
// (the 4:2:0 kernels keep their names without the layout)
#define to_inp_yuv420_kernel to_inp_yuv_kernel
#define to_inp16_yuv420_kernel to_inp16_yuv_kernel
#define to_inp_yuv420_rows_kernel to_inp_yuv_rows_kernel
#define to_inp16_yuv420_rows_kernel to_inp16_yuv_rows_kernel
#define to_inp_yuv420_pad_kernel to_inp_yuv_pad_kernel
#define to_inp16_yuv420_pad_kernel to_inp16_yuv_pad_kernel
#define to_inp_yuv420_pad_rows_kernel to_inp_yuv_pad_rows_kernel
#define to_inp16_yuv420_pad_rows_kernel to_inp16_yuv_pad_rows_kernel
#define to_out_yuv420_kernel to_out_yuv_kernel
#define to_out16_yuv420_kernel to_out16_yuv_kernel
#define to_out_yuv420_rows_kernel to_out_yuv_rows_kernel
#define to_out16_yuv420_rows_kernel to_out16_yuv_rows_kernel
#define to_out_yuv420_crop_kernel to_out_yuv_crop_kernel
#define to_out16_yuv420_crop_kernel to_out16_yuv_crop_kernel
#define to_out_yuv420_crop_rows_kernel to_out_yuv_crop_rows_kernel
#define to_out16_yuv420_crop_rows_kernel to_out16_yuv_crop_rows_kernel
#define K_INP(D, L) to_inp##D##_yuv##L##_kernel
#define K_INP_ROWS(D, L) to_inp##D##_yuv##L##_rows_kernel
#define K_INP_PAD(D, L) to_inp##D##_yuv##L##_pad_kernel
#define K_INP_PAD_ROWS(D, L) to_inp##D##_yuv##L##_pad_rows_kernel
#define K_OUT(D, L) to_out##D##_yuv##L##_kernel
#define K_OUT_ROWS(D, L) to_out##D##_yuv##L##_rows_kernel
#define K_OUT_CROP(D, L) to_out##D##_yuv##L##_crop_kernel
#define K_OUT_CROP_ROWS(D, L) to_out##D##_yuv##L##_crop_rows_kernel

int drba_to_inp_yuv_x4(const uint8_t *y, const uint8_t *u, const uint8_t *v, int y_stride, int c_stride, float *out, float *out_x4, int Hin,
                       int Win, int Hout, int Wout, float scale_y, float scale_x, int matrix, int full_range, int layout, void *stream) {
  DRBA_BY_LAYOUT_IN(to_inp_yuv_launch, , K_INP, K_INP_ROWS, y, u, v, y_stride, c_stride, out, out_x4, Hin, Win, Hout, Wout, scale_y, scale_x,
                    matrix, full_range, 255.f, stream)
}

int drba_to_inp16_yuv_x4(const uint16_t *y, const uint16_t *u, const uint16_t *v, int y_stride, int c_stride, float *out, float *out_x4,
                         int Hin, int Win, int Hout, int Wout, float scale_y, float scale_x, int matrix, int full_range, int layout,
                         float maxval, void *stream) {
  DRBA_BY_LAYOUT_IN(to_inp_yuv_launch, 16, K_INP, K_INP_ROWS, y, u, v, y_stride, c_stride, out, out_x4, Hin, Win, Hout, Wout, scale_y,
                    scale_x, matrix, full_range, maxval, stream)
}

int drba_to_out_yuv(const float *in, uint8_t *y, uint8_t *u, uint8_t *v, int y_stride, int c_stride, int Hin, int Win, int Hout, int Wout,
                    float scale_y, float scale_x, int matrix, int full_range, int layout, void *stream) {
  DRBA_BY_LAYOUT(to_out_yuv_launch, , K_OUT, K_OUT_ROWS, in, y, u, v, y_stride, c_stride, Hin, Win, Hout, Wout, scale_y, scale_x, matrix,
                 full_range, 255.f, stream)
}

int drba_to_out16_yuv(const float *in, uint16_t *y, uint16_t *u, uint16_t *v, int y_stride, int c_stride, int Hin, int Win, int Hout,
                      int Wout, float scale_y, float scale_x, int matrix, int full_range, int layout, float maxval, void *stream) {
  DRBA_BY_LAYOUT(to_out_yuv_launch, 16, K_OUT, K_OUT_ROWS, in, y, u, v, y_stride, c_stride, Hin, Win, Hout, Wout, scale_y, scale_x, matrix,
                 full_range, maxval, stream)
}

int drba_to_inp_yuv_pad_x4(const uint8_t *y, const uint8_t *u, const uint8_t *v, int y_stride, int c_stride, float *out, float *out_x4,
                           int Hin, int Win, int Hout, int Wout, int matrix, int full_range, int layout, void *stream) {
  DRBA_BY_LAYOUT_IN(to_inp_yuv_pad_launch, , K_INP_PAD, K_INP_PAD_ROWS, y, u, v, y_stride, c_stride, out, out_x4, Hin, Win, Hout, Wout,
                    matrix, full_range, 255.f, stream)
}

int drba_to_inp16_yuv_pad_x4(const uint16_t *y, const uint16_t *u, const uint16_t *v, int y_stride, int c_stride, float *out, float *out_x4,
                             int Hin, int Win, int Hout, int Wout, int matrix, int full_range, int layout, float maxval, void *stream) {
  DRBA_BY_LAYOUT_IN(to_inp_yuv_pad_launch, 16, K_INP_PAD, K_INP_PAD_ROWS, y, u, v, y_stride, c_stride, out, out_x4, Hin, Win, Hout, Wout,
                    matrix, full_range, maxval, stream)
}

int drba_to_out_yuv_crop(const float *in, uint8_t *y, uint8_t *u, uint8_t *v, int y_stride, int c_stride, int Hin, int Win, int Hout,
                         int Wout, int matrix, int full_range, int layout, void *stream) {
  DRBA_BY_LAYOUT(to_out_yuv_crop_launch, , K_OUT_CROP, K_OUT_CROP_ROWS, in, y, u, v, y_stride, c_stride, Hin, Win, Hout, Wout, matrix,
                 full_range, 255.f, stream)
}

int drba_to_out16_yuv_crop(const float *in, uint16_t *y, uint16_t *u, uint16_t *v, int y_stride, int c_stride, int Hin, int Win, int Hout,
                           int Wout, int matrix, int full_range, int layout, float maxval, void *stream) {
  DRBA_BY_LAYOUT(to_out_yuv_crop_launch, 16, K_OUT_CROP, K_OUT_CROP_ROWS, in, y, u, v, y_stride, c_stride, Hin, Win, Hout, Wout, matrix,
                 full_range, maxval, stream)
}

}  // extern "C"

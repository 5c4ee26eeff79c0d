// Picture metrics on finished frames: ssim_matlab at full size and exact frame differences.
//
// drba_ssim3d: the mean of the ssim_matlab map (pytorch_msssim/__init__.py:83-136) of N image pairs at any H, W >= 11: the five
// fields a, b, a^2, b^2, ab blurred by the separable 11-tap gaussian along x, y and the channel axis with replicate padding 5
// on all three (on three channels the channel pass is a fixed 3 x 3 mix).  Unlike scdet.hip -- which reproduces the reference's
// fp32 rounding because the scene DECISION must match it -- this kernel computes the value of the definition: the blurs are
// accumulated in fp64 (products of fp32 inputs are exact there), so blur(a a) - blur(a)^2 does not cancel on flat content.
// One workgroup owns a 32 x 16 tile of all three channels; the fields are taken one at a time through one LDS buffer
// (x pass into LDS, y pass + channel mix into registers).  Tile sums go to the workspace, a second kernel adds them in a fixed
// order: no floating-point atomics, the same bits on every run and for an item alone or in a batch.
//
// drba_ssim2d: the single-channel 2-D ssim of the same file (pytorch_msssim/__init__.py:29-80) on N planes addressed by a row and an
// item stride (the luma planes of packed 4:2:0 frames): the tile kernel above without the channel axis, one plane per workgroup.
//
// drba_frame_error_u8 / _u16 / _f32: sum d^2, sum |d|, max |d| and a count per item, integers for bytes and 16-bit samples and
// fp64 for floats, through the same two-stage reduction.
#include "common.hpp"

#include <math.h>

using namespace drba;

// identical inputs must give identical bits in s1, s2 and s12 (SSIM exactly 1), and the sums must not depend on what the
// compiler fuses: every fma in this file is written out
#pragma clang fp contract(off)

namespace {

constexpr int kTX = 32, kTY = 16;                  // output tile
constexpr int kHX = kTX + 10, kHY = kTY + 10;      // with the window's halo
constexpr int kRangeParts = 256;                   // range pre-pass: workgroups per item
constexpr int kErrParts = 512;                     // frame error: workgroups per item, at most

struct SsimArgs {
  double g[11];     // gaussian(11, 1.5) as scdet.hip builds it (double exp -> fp32, normalised in fp32), widened
  double mix[3][3]; // the channel pass on three channels with replicate padding 5
  double val_range; // > 0: L; 0: inferred per item from the first image
};

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the sum over a 256-thread workgroup in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum256(double v, double *red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool U8>
__device__ __forceinline__ float load_px(const void *img, size_t item, int c, int y, int x, int H, int W) {
  if (U8) return (float)static_cast<const uint8_t *>(img)[((item * H + y) * W + x) * 3 + c] / 255.f;
  return static_cast<const float *>(img)[((item * 3 + c) * H + y) * W + x];
}

// min / max of the first image per item (pytorch_msssim/__init__.py:85-97), kRangeParts partial pairs per item
__global__ void __launch_bounds__(256) ssim_range_kernel(const float *__restrict__ x1, size_t n_per_item, float *__restrict__ parts) {
  __shared__ float smx[4], smn[4];
  const float *p = x1 + (size_t)blockIdx.y * n_per_item;
  float mx = -INFINITY, mn = INFINITY;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n_per_item; e += (size_t)kRangeParts * 256) {
    const float v = p[e];
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_down(mx, o, 64));
    mn = fminf(mn, __shfl_down(mn, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    smx[threadIdx.x >> 6] = mx;
    smn[threadIdx.x >> 6] = mn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float *o = parts + ((size_t)blockIdx.y * kRangeParts + blockIdx.x) * 2;
    o[0] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    o[1] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
  }
}

// one field of the five from the staged pair
template <int F>
__device__ __forceinline__ double field(float a, float b) {
  const double da = (double)a, db = (double)b;
  return F == 0 ? da : F == 1 ? db : F == 2 ? da * da : F == 3 ? db * db : da * db;
}

template <int F>
__device__ __forceinline__ void blur_field(const float (*sa)[kHY][kHX], const float (*sb)[kHY][kHX], double (*tmp)[kHY][kTX],
                                           const SsimArgs &A, double (&out)[2][3]) {
  const int tid = threadIdx.x;
  __syncthreads();  // tmp is free again
  for (int e = tid; e < 3 * kHY * kTX; e += 256) {  // along x
    const int x = e & (kTX - 1), r = (e / kTX) % kHY, c = e / (kTX * kHY);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) s = fma(A.g[k], field<F>(sa[c][r][x + k], sb[c][r][x + k]), s);
    tmp[c][r][x] = s;
  }
  __syncthreads();
  const int x = tid & (kTX - 1), y0 = tid >> 5;
#pragma unroll
  for (int j = 0; j < 2; ++j) {  // along y, then the channel mix
    const int y = y0 + 8 * j;
    double v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 11; ++k) s = fma(A.g[k], tmp[c][y + k][x], s);
      v[c] = s;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[j][c] = fma(A.mix[c][2], v[2], fma(A.mix[c][1], v[1], A.mix[c][0] * v[0]));
  }
}

template <bool U8>
__global__ void __launch_bounds__(256) ssim3d_tile_kernel(const void *__restrict__ img1, const void *__restrict__ img2,
                                                          double *__restrict__ partial, const float *__restrict__ range_parts,
                                                          int H, int W, int tiles_x, SsimArgs A) {
  __shared__ float sa[3][kHY][kHX], sb[3][kHY][kHX];
  __shared__ double tmp[3][kHY][kTX];
  __shared__ double red[4];
  __shared__ float lim[2];
  const int tid = threadIdx.x;
  const size_t item = blockIdx.y;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int x0 = tx * kTX - 5, y0 = ty * kTY - 5;
  for (int e = tid; e < 3 * kHY * kHX; e += 256) {  // replicate padding = clamped reads
    const int i = e % kHX, r = (e / kHX) % kHY, c = e / (kHX * kHY);
    const int gx = min(max(x0 + i, 0), W - 1), gy = min(max(y0 + r, 0), H - 1);
    sa[c][r][i] = load_px<U8>(img1, item, c, gy, gx, H, W);
    sb[c][r][i] = load_px<U8>(img2, item, c, gy, gx, H, W);
  }
  double L = A.val_range;
  if (!(L > 0.0)) {
    if (U8) {
      L = 1.0;  // bytes are scaled into [0, 1]
    } else {
      if (tid < 64) {
        float mx = -INFINITY, mn = INFINITY;
        for (int i = tid; i < kRangeParts; i += 64) {
          mx = fmaxf(mx, range_parts[(item * kRangeParts + i) * 2]);
          mn = fminf(mn, range_parts[(item * kRangeParts + i) * 2 + 1]);
        }
        for (int o = 32; o > 0; o >>= 1) {
          mx = fmaxf(mx, __shfl_down(mx, o, 64));
          mn = fminf(mn, __shfl_down(mn, o, 64));
        }
        if (tid == 0) {
          lim[0] = mx;
          lim[1] = mn;
        }
      }
      __syncthreads();
      L = ((lim[0] > 128.f) ? 255.0 : 1.0) - ((lim[1] < -0.5f) ? -1.0 : 0.0);
    }
  }
  const double C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);

  double mu1[2][3], mu2[2][3], e11[2][3], e22[2][3], e12[2][3];
  blur_field<0>(sa, sb, tmp, A, mu1);  // (its first barrier also publishes sa / sb)
  blur_field<1>(sa, sb, tmp, A, mu2);
  blur_field<2>(sa, sb, tmp, A, e11);
  blur_field<3>(sa, sb, tmp, A, e22);
  blur_field<4>(sa, sb, tmp, A, e12);

  const int px = tx * kTX + (tid & (kTX - 1));
  double part = 0.0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int py = ty * kTY + (tid >> 5) + 8 * j;
    if (px < W && py < H) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double m1 = mu1[j][c], m2 = mu2[j][c];
        const double m1sq = m1 * m1, m2sq = m2 * m2, m12 = m1 * m2;
        const double s1 = e11[j][c] - m1sq, s2 = e22[j][c] - m2sq, s12 = e12[j][c] - m12;
        const double v1 = 2.0 * s12 + C2, v2 = (s1 + s2) + C2;
        part += ((2.0 * m12 + C1) * v1) / (((m1sq + m2sq) + C1) * v2);
      }
    }
  }
  const double tot = block_sum256(part, red);
  if (tid == 0) partial[item * gridDim.x + blockIdx.x] = tot;
}

// out[item] = (sum of the item's partials, in a fixed order) / count
__global__ void __launch_bounds__(256) sum_partials_kernel(const double *__restrict__ partial, int n_parts, double count,
                                                           double *__restrict__ out) {
  __shared__ double red[4];
  const double *p = partial + (size_t)blockIdx.x * n_parts;
  double s = 0.0;
  for (int i = threadIdx.x; i < n_parts; i += 256) s += p[i];
  const double tot = block_sum256(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = tot / count;
}

// ---- one plane: the 2-D ssim ------------------------------------------------------------------------------------------------
struct Ssim2dArgs {
  double g[11];   // the same window as SsimArgs::g
  double L;       // the value range: the caller's for fp32 samples, 1 for integer ones
  float maxval;   // what integer samples are divided by
};

// DT: 0 = fp32, 1 = uint8, 2 = uint16 samples; integer ones as (float)s / (float)maxval, a true fp32 division
template <int DT>
__device__ __forceinline__ float load_sample(const void *plane, size_t at, float maxval) {
  if (DT == 1) return (float)static_cast<const uint8_t *>(plane)[at] / maxval;
  if (DT == 2) return (float)static_cast<const uint16_t *>(plane)[at] / maxval;
  return static_cast<const float *>(plane)[at];
}

// blur_field on one plane: no channel mix
template <int F>
__device__ __forceinline__ void blur_plane(const float (*sa)[kHX], const float (*sb)[kHX], double (*tmp)[kTX], const Ssim2dArgs &A,
                                           double (&out)[2]) {
  const int tid = threadIdx.x;
  __syncthreads();  // tmp is free again
  for (int e = tid; e < kHY * kTX; e += 256) {  // along x
    const int x = e & (kTX - 1), r = e / kTX;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) s = fma(A.g[k], field<F>(sa[r][x + k], sb[r][x + k]), s);
    tmp[r][x] = s;
  }
  __syncthreads();
  const int x = tid & (kTX - 1), y0 = tid >> 5;
#pragma unroll
  for (int j = 0; j < 2; ++j) {  // along y
    const int y = y0 + 8 * j;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) s = fma(A.g[k], tmp[y + k][x], s);
    out[j] = s;
  }
}

// ssim3d_tile_kernel for single planes: the same 32 x 16 tile, halo, passes and sums, a third of its LDS (two fp32 halo tiles of
// 26 x 42 and one fp64 row buffer of 26 x 32: 15.4 KB against 46 KB).
// Occupancy: 8 workgroups (32 waves) per CU, the most the CU's wave slots hold -- the launch bound asks for 8 waves per SIMD, i.e.
// at most 64 VGPRs, and the kernel needs fewer (ten fp64 results and a window held in SGPRs).  LDS would admit 10 workgroups of
// 15.4 KB in 160 KB, so the wave slots bind, not LDS.  The kernel alternates LDS-bound passes with barriers between them (ten per
// tile): with few resident workgroups (the three-channel kernel's 46 KB and 144 VGPRs allow three) a CU idles at every barrier;
// eight give the scheduler other tiles' passes to run meanwhile.  Measured: 62 VGPRs, no scratch, 41 us per 1080 x 1920 plane
// against 147 us for the three-channel kernel on the BGR frame (profiles/metrics_yuv.md).
template <int DT>
__global__ void __launch_bounds__(256, 8) ssim2d_tile_kernel(const void *__restrict__ p1, const void *__restrict__ p2,
                                                             double *__restrict__ partial, int H, int W, size_t row_stride,
                                                             size_t item_stride, int tiles_x, Ssim2dArgs A) {
  __shared__ float sa[kHY][kHX], sb[kHY][kHX];
  __shared__ double tmp[kHY][kTX];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.y * item_stride;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int x0 = tx * kTX - 5, y0 = ty * kTY - 5;
  for (int e = tid; e < kHY * kHX; e += 256) {  // replicate padding = clamped reads: no read leaves [0, H) x [0, W)
    const int i = e % kHX, r = e / kHX;
    const int gx = min(max(x0 + i, 0), W - 1), gy = min(max(y0 + r, 0), H - 1);
    const size_t at = base + (size_t)gy * row_stride + (size_t)gx;
    sa[r][i] = load_sample<DT>(p1, at, A.maxval);
    sb[r][i] = load_sample<DT>(p2, at, A.maxval);
  }
  const double C1 = (0.01 * A.L) * (0.01 * A.L), C2 = (0.03 * A.L) * (0.03 * A.L);

  double mu1[2], mu2[2], e11[2], e22[2], e12[2];
  blur_plane<0>(sa, sb, tmp, A, mu1);  // (its first barrier also publishes sa / sb)
  blur_plane<1>(sa, sb, tmp, A, mu2);
  blur_plane<2>(sa, sb, tmp, A, e11);
  blur_plane<3>(sa, sb, tmp, A, e22);
  blur_plane<4>(sa, sb, tmp, A, e12);

  const int px = tx * kTX + (tid & (kTX - 1));
  double part = 0.0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int py = ty * kTY + (tid >> 5) + 8 * j;
    if (px < W && py < H) {
      const double m1 = mu1[j], m2 = mu2[j];
      const double m1sq = m1 * m1, m2sq = m2 * m2, m12 = m1 * m2;
      const double s1 = e11[j] - m1sq, s2 = e22[j] - m2sq, s12 = e12[j] - m12;
      const double v1 = 2.0 * s12 + C2, v2 = (s1 + s2) + C2;
      part += ((2.0 * m12 + C1) * v1) / (((m1sq + m2sq) + C1) * v2);
    }
  }
  const double tot = block_sum256(part, red);
  if (tid == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// ---- frame differences ---------------------------------------------------------------------------------------------------
typedef unsigned long long u64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4u __attribute__((ext_vector_type(4), aligned(1)));

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_down(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// One difference into the sums.  SQ is what the squares are added in, and why each width is exact:
// bytes: unsigned, one per 16-byte chunk -- 16 * 255^2 is far inside 32 bits -- that is then added to the 64-bit sum;
// uint16: the 64-bit sum itself -- one d^2 fits 32 bits (65535^2 < 2^32), two do not.
template <class SQ>
__device__ __forceinline__ void acc_sample(unsigned a, unsigned b, SQ &sq, unsigned &ab, unsigned &mx, unsigned &nz) {
  const unsigned d = a > b ? a - b : b - a;
  sq += (SQ)(d * d);
  ab += d;
  mx = max(mx, d);
  nz += d != 0u;
}

// T = uint8_t / uint16_t.  Per item: head samples up to a's next 16-byte boundary (a is aligned to its samples), 16-byte chunks
// (b's loads unaligned when its phase differs), tail samples; the wave and workgroup reduction; one partial
// (sum d^2, sum |d|, max |d|, differing) per workgroup for frame_error_u8_final.
template <class T>
__device__ __forceinline__ void frame_error_body(const T *__restrict__ a, const T *__restrict__ b, size_t n, int parts,
                                                 u64 *__restrict__ partial) {
  constexpr int kBits = 8 * (int)sizeof(T), kPerWord = 32 / kBits;
  constexpr size_t kPerChunk = 16 / sizeof(T);
  __shared__ u64 red[4][4];
  const T *pa = a + (size_t)blockIdx.y * n, *pb = b + (size_t)blockIdx.y * n;
  size_t head = (size_t)(((16u - (unsigned)((uintptr_t)pa & 15u)) & 15u) / (unsigned)sizeof(T));
  if (head > n) head = n;
  const size_t chunks = (n - head) / kPerChunk, tail0 = head + chunks * kPerChunk;
  const bool same_phase = (((uintptr_t)pa ^ (uintptr_t)pb) & 15u) == 0;
  u64 sq = 0, ab = 0;
  unsigned mx = 0, nz = 0;
  auto with_sq = [&](auto &&step) {  // step(what the squares of one chunk, or of one edge sample, are added in)
    if constexpr (sizeof(T) == 1) {
      unsigned csq = 0;
      step(csq);
      sq += csq;
    } else {
      step(sq);
    }
  };
  const size_t gtid = (size_t)blockIdx.x * 256 + threadIdx.x, gstride = (size_t)parts * 256;
  for (size_t i = gtid; i < chunks; i += gstride) {
    const u32x4 va = *reinterpret_cast<const u32x4 *>(pa + head + i * kPerChunk);
    u32x4 vb;
    if (same_phase)
      vb = *reinterpret_cast<const u32x4 *>(pb + head + i * kPerChunk);
    else
      vb = *reinterpret_cast<const u32x4u *>(pb + head + i * kPerChunk);
    unsigned cab = 0;  // at most 16 * 255 or 8 * 65535
    with_sq([&](auto &csq) {
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < kPerWord; ++k)
          acc_sample((va[w] >> (kBits * k)) & ((1u << kBits) - 1u), (vb[w] >> (kBits * k)) & ((1u << kBits) - 1u), csq, cab, mx, nz);
    });
    ab += cab;
  }
  // head and tail: fewer than two chunks of samples per item, taken by the first workgroup
  if (blockIdx.x == 0) {
    const size_t edge = head + (n - tail0);
    if (threadIdx.x < edge) {
      const size_t e = threadIdx.x < head ? threadIdx.x : tail0 + (threadIdx.x - head);
      unsigned cab = 0;
      with_sq([&](auto &csq) { acc_sample(pa[e], pb[e], csq, cab, mx, nz); });
      ab += cab;
    }
  }
  sq = wave_sum_u64(sq);
  ab = wave_sum_u64(ab);
  const u64 m = wave_max_u64(mx), z = wave_sum_u64(nz);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[w][0] = sq;
    red[w][1] = ab;
    red[w][2] = m;
    red[w][3] = z;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 *o = partial + ((size_t)blockIdx.y * parts + blockIdx.x) * 4;
    o[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    o[1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    o[2] = max(max(red[0][2], red[1][2]), max(red[2][2], red[3][2]));
    o[3] = red[0][3] + red[1][3] + red[2][3] + red[3][3];
  }
}

__global__ void __launch_bounds__(256) frame_error_u8_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                             size_t n, int parts, u64 *__restrict__ partial) {
  frame_error_body(a, b, n, parts, partial);
}
__global__ void __launch_bounds__(256) frame_error_u16_kernel(const uint16_t *__restrict__ a, const uint16_t *__restrict__ b,
                                                              size_t n, int parts, u64 *__restrict__ partial) {
  frame_error_body(a, b, n, parts, partial);
}

__global__ void __launch_bounds__(256) frame_error_u8_final(const u64 *__restrict__ partial, int parts, u64 *__restrict__ out) {
  __shared__ u64 red[4][4];
  const u64 *p = partial + (size_t)blockIdx.x * parts * 4;
  u64 sq = 0, ab = 0, mx = 0, nz = 0;
  for (int i = threadIdx.x; i < parts; i += 256) {
    sq += p[i * 4];
    ab += p[i * 4 + 1];
    mx = max(mx, p[i * 4 + 2]);
    nz += p[i * 4 + 3];
  }
  sq = wave_sum_u64(sq);
  ab = wave_sum_u64(ab);
  mx = wave_max_u64(mx);
  nz = wave_sum_u64(nz);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[w][0] = sq;
    red[w][1] = ab;
    red[w][2] = mx;
    red[w][3] = nz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 *o = out + (size_t)blockIdx.x * 4;
    o[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    o[1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    o[2] = max(max(red[0][2], red[1][2]), max(red[2][2], red[3][2]));
    o[3] = red[0][3] + red[1][3] + red[2][3] + red[3][3];
  }
}

// fp32 data: the sums and the maximum run over the FINITE differences, the others are counted
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}

__device__ __forceinline__ void block_err_f32(double sq, double ab, double mx, u64 nf, double *o) {
  __shared__ double red[4][3];
  __shared__ u64 redn[4];
  sq = wave_sum(sq);
  ab = wave_sum(ab);
  mx = wave_max(mx);
  nf = wave_sum_u64(nf);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[w][0] = sq;
    red[w][1] = ab;
    red[w][2] = mx;
    redn[w] = nf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    o[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    o[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    o[2] = fmax(fmax(red[0][2], red[1][2]), fmax(red[2][2], red[3][2]));
    reinterpret_cast<u64 *>(o)[3] = redn[0] + redn[1] + redn[2] + redn[3];
  }
}

__global__ void __launch_bounds__(256) frame_error_f32_kernel(const float *__restrict__ a, const float *__restrict__ b, size_t n,
                                                              int parts, double *__restrict__ partial) {
  const float *pa = a + (size_t)blockIdx.y * n, *pb = b + (size_t)blockIdx.y * n;
  double sq = 0.0, ab = 0.0, mx = 0.0;
  u64 nf = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)parts * 256) {
    const double d = fabs((double)pa[i] - (double)pb[i]);  // exact: both operands are fp32
    if (d <= 1.0e300) {  // finite (NaN fails the comparison)
      sq += d * d;
      ab += d;
      mx = fmax(mx, d);
    } else {
      ++nf;
    }
  }
  block_err_f32(sq, ab, mx, nf, partial + ((size_t)blockIdx.y * parts + blockIdx.x) * 4);
}

__global__ void __launch_bounds__(256) frame_error_f32_final(const double *__restrict__ partial, int parts, double *__restrict__ out) {
  const double *p = partial + (size_t)blockIdx.x * parts * 4;
  double sq = 0.0, ab = 0.0, mx = 0.0;
  u64 nf = 0;
  for (int i = threadIdx.x; i < parts; i += 256) {
    sq += p[i * 4];
    ab += p[i * 4 + 1];
    mx = fmax(mx, p[i * 4 + 2]);
    nf += reinterpret_cast<const u64 *>(p)[i * 4 + 3];
  }
  block_err_f32(sq, ab, mx, nf, out + (size_t)blockIdx.x * 4);
}

int err_parts(size_t n_per_item, size_t per_thread_bytes_or_elems) {
  size_t p = (n_per_item + 256 * per_thread_bytes_or_elems - 1) / (256 * per_thread_bytes_or_elems);
  if (p < 1) p = 1;
  if (p > (size_t)kErrParts) p = kErrParts;
  return (int)p;
}

// gaussian(11, 1.5): double exp -> fp32, normalised in fp32 (as scdet.hip), widened
void gaussian11(double (&out)[11]) {
  float g[11], sum = 0.f;
  for (int k = 0; k < 11; ++k) {
    g[k] = (float)exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  for (int k = 0; k < 11; ++k) out[k] = (double)(g[k] / sum);
}

}  // namespace

// ---- entry points -------------------------------------------------------------------------------------------------------------
extern "C" size_t drba_ssim3d_ws_floats(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  const size_t tiles = (size_t)((W + kTX - 1) / kTX) * (size_t)((H + kTY - 1) / kTY);
  return (size_t)N * tiles * 2 + (size_t)N * kRangeParts * 2;  // [tile sums, doubles][range partials, floats]
}

extern "C" int drba_ssim3d(const void *img1, const void *img2, double *out, float *ws, int N, int H, int W, int dtype,
                           double val_range, void *stream) {
  if (!img1 || !img2 || !out || !ws || N < 1 || H < 1 || W < 1) return DRBA_EINVAL;
  if (dtype != 0 && dtype != 1) return DRBA_EINVAL;
  if (!(val_range >= 0.0) || isinf(val_range)) return DRBA_EINVAL;
  if (((uintptr_t)ws & 7u) || ((uintptr_t)out & 7u)) return DRBA_EINVAL;
  if (H < 11 || W < 11) return DRBA_EUNSUPPORTED;  // the reference shrinks the window there
  if (N > 65535) return DRBA_EUNSUPPORTED;
  const int tiles_x = (W + kTX - 1) / kTX, tiles_y = (H + kTY - 1) / kTY;
  if ((size_t)tiles_x * tiles_y > 0x7fffffffu) return DRBA_EUNSUPPORTED;
  const int tiles = tiles_x * tiles_y;

  SsimArgs A;
  gaussian11(A.g);
  for (int c = 0; c < 3; ++c) {
    for (int s = 0; s < 3; ++s) A.mix[c][s] = 0.0;
    for (int k = 0; k < 11; ++k) {
      const int s = c + k - 5 < 0 ? 0 : c + k - 5 > 2 ? 2 : c + k - 5;
      A.mix[c][s] += A.g[k];
    }
  }
  A.val_range = val_range;

  double *partial = reinterpret_cast<double *>(ws);
  float *range_parts = ws + (size_t)N * tiles * 2;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 0 && val_range == 0.0) {
    DRBA_LAUNCH(ssim_range_kernel, dim3(kRangeParts, N), dim3(256), 0, s, static_cast<const float *>(img1), (size_t)3 * H * W,
                range_parts);
    DRBA_CHECK_LAUNCH();
  }
  if (dtype == 0)
    DRBA_LAUNCH(ssim3d_tile_kernel<false>, dim3(tiles, N), dim3(256), 0, s, img1, img2, partial, range_parts, H, W, tiles_x, A);
  else
    DRBA_LAUNCH(ssim3d_tile_kernel<true>, dim3(tiles, N), dim3(256), 0, s, img1, img2, partial, range_parts, H, W, tiles_x, A);
  DRBA_CHECK_LAUNCH();
  DRBA_LAUNCH(sum_partials_kernel, dim3(N), dim3(256), 0, s, partial, tiles, 3.0 * (double)H * (double)W, out);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

extern "C" size_t drba_ssim2d_ws_floats(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  const size_t tiles = (size_t)((W + kTX - 1) / kTX) * (size_t)((H + kTY - 1) / kTY);
  return (size_t)N * tiles * 2;  // tile sums, doubles
}

extern "C" int drba_ssim2d(const void *p1, const void *p2, double *out, float *ws, int N, int H, int W, size_t row_stride,
                           size_t item_stride, int dtype, double maxval, void *stream) {
  if (!p1 || !p2 || !out || !ws || N < 1 || H < 1 || W < 1) return DRBA_EINVAL;
  if (dtype < 0 || dtype > 2) return DRBA_EINVAL;
  if (row_stride < (size_t)W) return DRBA_EINVAL;
  if (((uintptr_t)ws & 7u) || ((uintptr_t)out & 7u)) return DRBA_EINVAL;
  Ssim2dArgs A;
  if (dtype == 0) {
    if (!(maxval > 0.0) || isinf(maxval)) return DRBA_EINVAL;
    A.L = maxval;
    A.maxval = 1.f;
  } else if (dtype == 1) {
    if (maxval != 0.0 && maxval != 255.0) return DRBA_EINVAL;
    A.L = 1.0;
    A.maxval = 255.f;
  } else {
    if ((((uintptr_t)p1 | (uintptr_t)p2) & 1u)) return DRBA_EINVAL;
    if (!(maxval > 255.0 && maxval <= 65535.0) || maxval != floor(maxval)) return DRBA_EINVAL;
    A.L = 1.0;
    A.maxval = (float)maxval;
  }
  if (H < 11 || W < 11) return DRBA_EUNSUPPORTED;  // the reference shrinks the window there
  if (N > 65535) return DRBA_EUNSUPPORTED;
  const int tiles_x = (W + kTX - 1) / kTX, tiles_y = (H + kTY - 1) / kTY;
  if ((size_t)tiles_x * tiles_y > 0x7fffffffu) return DRBA_EUNSUPPORTED;
  const int tiles = tiles_x * tiles_y;
  gaussian11(A.g);

  double *partial = reinterpret_cast<double *>(ws);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 0)
    DRBA_LAUNCH(ssim2d_tile_kernel<0>, dim3(tiles, N), dim3(256), 0, s, p1, p2, partial, H, W, row_stride, item_stride, tiles_x, A);
  else if (dtype == 1)
    DRBA_LAUNCH(ssim2d_tile_kernel<1>, dim3(tiles, N), dim3(256), 0, s, p1, p2, partial, H, W, row_stride, item_stride, tiles_x, A);
  else
    DRBA_LAUNCH(ssim2d_tile_kernel<2>, dim3(tiles, N), dim3(256), 0, s, p1, p2, partial, H, W, row_stride, item_stride, tiles_x, A);
  DRBA_CHECK_LAUNCH();
  DRBA_LAUNCH(sum_partials_kernel, dim3(N), dim3(256), 0, s, partial, tiles, (double)H * (double)W, out);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

extern "C" size_t drba_frame_error_ws_floats(int N, size_t n_per_item) {
  if (N < 1 || n_per_item < 1) return 0;
  return (size_t)N * kErrParts * 4 * 2;  // 4 x 8 bytes per workgroup
}

// the integer kinds: a partial per workgroup, then frame_error_u8_final; a thread takes 8 chunks of 16 bytes
template <class T>
static int frame_error_int(void (*kernel)(const T *, const T *, size_t, int, u64 *), const T *a, const T *b, unsigned long long *out,
                           float *ws, int N, size_t n_per_item, size_t n_max, void *stream) {
  if (!a || !b || !out || !ws || N < 1 || n_per_item < 1) return DRBA_EINVAL;
  if (((uintptr_t)ws & 7u) || ((uintptr_t)out & 7u)) return DRBA_EINVAL;
  if (N > 65535 || n_per_item > n_max) return DRBA_EUNSUPPORTED;
  const int parts = err_parts(n_per_item, (16 / sizeof(T)) * 8);
  hipStream_t s = (hipStream_t)stream;
  DRBA_LAUNCH(kernel, dim3(parts, N), dim3(256), 0, s, a, b, n_per_item, parts, reinterpret_cast<u64 *>(ws));
  DRBA_CHECK_LAUNCH();
  DRBA_LAUNCH(frame_error_u8_final, dim3(N), dim3(256), 0, s, reinterpret_cast<const u64 *>(ws), parts, reinterpret_cast<u64 *>(out));
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

extern "C" int drba_frame_error_u8(const uint8_t *a, const uint8_t *b, unsigned long long *out, float *ws, int N,
                                   size_t n_per_item, void *stream) {
  return frame_error_int(frame_error_u8_kernel, a, b, out, ws, N, n_per_item, SIZE_MAX, stream);
}

extern "C" size_t drba_frame_error_u16_ws_floats(int N, size_t n_per_item) { return drba_frame_error_ws_floats(N, n_per_item); }

extern "C" int drba_frame_error_u16(const uint16_t *a, const uint16_t *b, unsigned long long *out, float *ws, int N,
                                    size_t n_per_item, void *stream) {
  if ((((uintptr_t)a | (uintptr_t)b) & 1u)) return DRBA_EINVAL;
  return frame_error_int(frame_error_u16_kernel, a, b, out, ws, N, n_per_item, (size_t)0xffffffffull, stream);  // sum d^2 < 2^32 * 2^32
}

extern "C" int drba_frame_error_f32(const float *a, const float *b, double *out, float *ws, int N, size_t n_per_item,
                                    void *stream) {
  if (!a || !b || !out || !ws || N < 1 || n_per_item < 1) return DRBA_EINVAL;
  if (((uintptr_t)ws & 7u) || ((uintptr_t)out & 7u)) return DRBA_EINVAL;
  if (N > 65535) return DRBA_EUNSUPPORTED;
  const int parts = err_parts(n_per_item, 8);
  hipStream_t s = (hipStream_t)stream;
  DRBA_LAUNCH(frame_error_f32_kernel, dim3(parts, N), dim3(256), 0, s, a, b, n_per_item, parts, reinterpret_cast<double *>(ws));
  DRBA_CHECK_LAUNCH();
  DRBA_LAUNCH(frame_error_f32_final, dim3(N), dim3(256), 0, s, reinterpret_cast<const double *>(ws), parts, out);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

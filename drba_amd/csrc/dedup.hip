// Duplicate-frame statistic (--dedup): ffmpeg mpdecimate's block test on the [0, 1] scale.  Over 8 x 8 pixel blocks aligned at the
// origin (right / bottom edge blocks partial, divided by their own pixel count) the mean of |a - b| over the block's pixels and all
// channels; the frame-level results are the largest block mean and the number of blocks whose mean is > lo.
//
// A pure streaming kernel: 2 * c * h * w * 4 bytes, each read once.  A wave takes a 32 x 8 pixel strip (four blocks): lane
// (row r = lane >> 3, quad q = lane & 7) reads the four pixels x = 4 q .. 4 q + 3 of row r of every channel -- one 16-byte load per
// tensor and channel where the address allows (a row of a wave is 128 contiguous bytes), four scalar loads otherwise (a row start
// that is not 16-byte aligned when w % 4 != 0, the partial quad at the right edge) -- and adds |a - b| in the order (channel, x).
// The 16 lanes of a block are then combined by an xor butterfly over the lane bits 0, 3, 4, 5: every sum is taken in an order fixed
// by the data layout.  The maximum and the count are kept per lane across the grid-stride loop, reduced once per workgroup (wave
// shuffles, then four words of LDS) and stored as one partial pair per workgroup; a second one-workgroup launch folds the pairs.
// No atomics: a maximum and an integer count do not depend on the order of the partials, so two calls return the same bytes.
#include "common.hpp"

using namespace drba;

namespace {

typedef float f32x4a __attribute__((ext_vector_type(4)));  // 16-byte aligned

constexpr int kStripW32 = 32, kStripH8 = 8;

__device__ __forceinline__ float quad_absdiff(const float *__restrict__ a, const float *__restrict__ b, size_t off, int nx, bool vec) {
  if (vec) {
    const f32x4a va = *reinterpret_cast<const f32x4a *>(a + off), vb = *reinterpret_cast<const f32x4a *>(b + off);
    return ((fabsf(va.x - vb.x) + fabsf(va.y - vb.y)) + fabsf(va.z - vb.z)) + fabsf(va.w - vb.w);
  }
  // the same four terms in the same order; a pixel past the row's end adds +0
  float d[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = i < nx ? fabsf(a[off + i] - b[off + i]) : 0.f;
  return ((d[0] + d[1]) + d[2]) + d[3];
}

__global__ void __launch_bounds__(kBlock) dup_stats_kernel(const float *__restrict__ a, const float *__restrict__ b, int c, int h, int w,
                                                           float lo, int strips_x, int n_strips, bool aligned, unsigned *__restrict__ part) {
  __shared__ unsigned red[2 * (kBlock / 64)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane >> 3, q = lane & 7;
  const size_t plane = (size_t)h * w;
  float vmax = 0.f;
  int above = 0;
  for (int s = blockIdx.x * (kBlock / 64) + wave; s < n_strips; s += gridDim.x * (kBlock / 64)) {  // (wave-uniform)
    const int sy = s / strips_x, sx = s - sy * strips_x;
    const int x = sx * kStripW32 + q * 4, y = sy * kStripH8 + r;
    float sum = 0.f;
    if (x < w && y < h) {
      const int nx = min(4, w - x);
      size_t off = (size_t)y * w + x;
      for (int ch = 0; ch < c; ++ch, off += plane) sum += quad_absdiff(a, b, off, nx, aligned && nx == 4 && (off & 3) == 0);
    }
    // the block's 16 lanes: the other quad of the row, then the rows
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 8, 64);
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const int bx = sx * kStripW32 + (q >> 1) * 8;  // the block's left column; its leader is the lane of row 0, even quad
    if (r == 0 && !(q & 1) && bx < w) {
      const int bw = min(8, w - bx), bh = min(8, h - sy * kStripH8);
      const float mean = sum / (float)(bw * bh * c);
      vmax = fmaxf(vmax, mean);
      above += mean > lo ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    vmax = fmaxf(vmax, __shfl_down(vmax, o, 64));
    above += __shfl_down(above, o, 64);
  }
  if (lane == 0) {
    red[2 * wave] = __float_as_uint(vmax);  // non-negative floats order like their bit patterns
    red[2 * wave + 1] = (unsigned)above;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned m = red[0], n = red[1];
    for (int i = 1; i < kBlock / 64; ++i) {
      m = max(m, red[2 * i]);
      n += red[2 * i + 1];
    }
    part[2 * blockIdx.x] = m;
    part[2 * blockIdx.x + 1] = n;
  }
}

__global__ void __launch_bounds__(kBlock) dup_stats_finish_kernel(const unsigned *__restrict__ part, int n_part, int n_blocks,
                                                                  unsigned *__restrict__ out) {
  __shared__ unsigned red[2 * (kBlock / 64)];
  unsigned m = 0, n = 0;
  for (int i = threadIdx.x; i < n_part; i += kBlock) {
    m = max(m, part[2 * i]);
    n += part[2 * i + 1];
  }
  for (int o = 32; o > 0; o >>= 1) {
    m = max(m, (unsigned)__shfl_down((int)m, o, 64));
    n += (unsigned)__shfl_down((int)n, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[2 * wave] = m;
    red[2 * wave + 1] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kBlock / 64; ++i) {
      m = max(m, red[2 * i]);
      n += red[2 * i + 1];
    }
    out[0] = m;
    out[1] = n;
    out[2] = (unsigned)n_blocks;
  }
}

// workgroups of the first launch: one wave per 32 x 8 strip, four per workgroup, capped (grid-stride above the cap)
int dup_grid(int h, int w) {
  const size_t strips = (size_t)((w + kStripW32 - 1) / kStripW32) * (size_t)((h + kStripH8 - 1) / kStripH8);
  return grid_for(strips, kBlock / 64);
}

bool dup_shape_ok(int c, int h, int w) {
  if (c < 1 || h < 1 || w < 1) return false;
  // strips, blocks and a block's divisor are ints; the element offsets are size_t
  return (size_t)((w + 7) / 8) * (size_t)((h + 7) / 8) < ((size_t)1 << 31) && c <= (1 << 24);
}

}  // namespace

extern "C" size_t drba_dup_stats_ws_floats(int c, int h, int w) {
  if (!dup_shape_ok(c, h, w)) return 0;
  return 2 * (size_t)dup_grid(h, w);
}

extern "C" int drba_dup_stats_f32(const float *a, const float *b, int c, int h, int w, float lo, void *out, float *ws, void *stream) {
  if (!a || !b || !out || !ws) return DRBA_EINVAL;
  if (c < 1 || h < 1 || w < 1) return DRBA_EINVAL;
  if (!dup_shape_ok(c, h, w)) return DRBA_EUNSUPPORTED;
  if (((uintptr_t)out & 3) || ((uintptr_t)ws & 3)) return DRBA_EINVAL;
  const int strips_x = (w + kStripW32 - 1) / kStripW32, strips_y = (h + kStripH8 - 1) / kStripH8;
  const int n_blocks = ((w + 7) / 8) * ((h + 7) / 8);
  const int grid = dup_grid(h, w);
  const bool aligned = !(((uintptr_t)a | (uintptr_t)b) & 15);
  DRBA_LAUNCH(dup_stats_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, b, c, h, w, lo, strips_x, strips_x * strips_y, aligned,
              (unsigned *)ws);
  DRBA_CHECK_LAUNCH();
  DRBA_LAUNCH(dup_stats_finish_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const unsigned *)ws, grid, n_blocks,
              (unsigned *)out);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

// Active-picture statistic (--crop): the largest sample of every row and of every pixel column of a 2-D sample array, from which
// the host finds letterbox / pillarbox bars (drba_amd/crop.py: ffmpeg cropdetect's rule, a row or column is picture when its
// maximum exceeds the limit).  rows x cols samples with a row pitch; `group` g samples make one pixel of a column (3: a packed BGR
// frame seen as H x 3W samples, 1: a luma plane): row_max[rows], col_max[cols / g], both uint32.
//
// One streaming pass, every sample read once.  A workgroup takes a strip of 64 lanes x VB bytes of kBandRows = 16 rows; its four waves
// take the rows of the band in turn, four rows each, all loaded before the first is reduced.  A lane loads VB bytes of a row in one
// instruction -- VB is the largest of 16, 4 and the sample size that divides both the base address and the pitch in bytes, so that
// every row of the frame is aligned as the first: a packed 1080p frame (pitch 5760 bytes) and a luma plane take 16-byte loads, a
// 50-pixel frame (pitch 150 bytes) byte loads -- and the strip's last, partial chunk of a row is read sample by sample: nothing past
// `cols` is touched.  A lane keeps the column maxima of its samples in registers over the band; the row maximum is a wave reduction
// and one integer atomic per (row, strip).  At the end of the band the four waves meet in LDS (integer LDS atomics), the samples of a
// pixel are folded, and one integer atomic per pixel column and band goes to memory (none for a zero: black bars cost no atomics).
// The band is short on purpose: a 1080p frame is only 6 MB, and the form in which a wave walked a 64-row band in four passes (a
// quarter of the atomics, a quarter of the workgroups) took about twice as long for the pass (profiles/crop.md has both).  A first
// small launch zeroes the two arrays, so the entry places no condition on their contents.  The results are integer maxima: exact,
// and the same for every launch geometry and every load width.
#include "common.hpp"

using namespace drba;

namespace {

constexpr int kWaveRows = 4;                          // rows a wave has in flight: all loaded before the first is reduced
constexpr int kBandRows = kWaveRows * (kBlock / 64);  // rows of a workgroup's band: 16

template <int VB>
struct Word;
template <>
struct Word<16> {
  typedef uint4 type;
};
template <>
struct Word<4> {
  typedef uint32_t type;
};
template <>
struct Word<2> {
  typedef uint16_t type;
};
template <>
struct Word<1> {
  typedef uint8_t type;
};

// the S = VB / sizeof(T) samples at p (aligned to VB bytes), widened
template <class T, int VB>
__device__ __forceinline__ void load_samples(const T *__restrict__ p, unsigned (&v)[VB / (int)sizeof(T)]) {
  constexpr int S = VB / (int)sizeof(T), kBits = 8 * (int)sizeof(T), kPerWord = 32 / kBits;
  if constexpr (VB >= 4) {
    const typename Word<VB>::type raw = *reinterpret_cast<const typename Word<VB>::type *>(p);
    uint32_t w[VB / 4];
    __builtin_memcpy(w, &raw, VB);
#pragma unroll
    for (int i = 0; i < S; ++i) v[i] = (w[i / kPerWord] >> (kBits * (i % kPerWord))) & ((1u << kBits) - 1u);
  } else {
    v[0] = (unsigned)*p;  // (VB == sizeof(T))
  }
}

__global__ void __launch_bounds__(kBlock) edge_max_zero_kernel(unsigned *__restrict__ row_max, int rows, unsigned *__restrict__ col_max,
                                                               int ncol) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < rows + ncol; i += gridDim.x * kBlock) {
    if (i < rows)
      row_max[i] = 0u;
    else
      col_max[i - rows] = 0u;
  }
}

template <class T, int VB>
__global__ void __launch_bounds__(kBlock) edge_max_kernel(const T *__restrict__ in, int rows, int cols, size_t pitch, int g,
                                                          unsigned *__restrict__ row_max, unsigned *__restrict__ col_max) {
  constexpr int S = VB / (int)sizeof(T), kStrip = 64 * S;  // samples of a lane, of a strip
  __shared__ unsigned cmax[kStrip];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s0 = blockIdx.x * kStrip, c0 = s0 + lane * S;  // the strip's and the lane's first sample column
  const int r_end = min(rows, ((int)blockIdx.y + 1) * kBandRows);
  for (int i = threadIdx.x; i < kStrip; i += kBlock) cmax[i] = 0u;
  unsigned cm[S];
#pragma unroll
  for (int i = 0; i < S; ++i) cm[i] = 0u;
  unsigned v[kWaveRows][S];
#pragma unroll
  for (int k = 0; k < kWaveRows; ++k) {
    const int r = (int)blockIdx.y * kBandRows + k * (kBlock / 64) + wave;  // (wave-uniform)
    const T *p = in + (size_t)r * pitch + c0;
    if (r < r_end && c0 + S <= cols) {
      load_samples<T, VB>(p, v[k]);
    } else {  // the row's partial last chunk, a lane past the row, a row past the frame: only samples inside are read
#pragma unroll
      for (int i = 0; i < S; ++i) v[k][i] = (r < r_end && c0 + i < cols) ? (unsigned)p[i] : 0u;
    }
  }
#pragma unroll
  for (int k = 0; k < kWaveRows; ++k) {
    const int r = (int)blockIdx.y * kBandRows + k * (kBlock / 64) + wave;
    unsigned rm = 0u;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      rm = max(rm, v[k][i]);
      cm[i] = max(cm[i], v[k][i]);
    }
    for (int o = 32; o > 0; o >>= 1) rm = max(rm, (unsigned)__shfl_xor((int)rm, o, 64));
    if (lane == 0 && r < r_end && rm) atomicMax(&row_max[r], rm);  // (the arrays start at zero: a zero changes nothing)
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < S; ++i)
    if (cm[i]) atomicMax(&cmax[lane * S + i], cm[i]);
  __syncthreads();
  // the pixel columns this strip holds samples of; a pixel cut by the strip's edge gets its other samples from the next strip
  const int s_end = min(cols, s0 + kStrip);
  if (s0 >= s_end) return;
  const int p_lo = s0 / g, p_hi = (s_end - 1) / g;
  for (int px = p_lo + threadIdx.x; px <= p_hi; px += kBlock) {
    const int a = max(px * g, s0), b = min(px * g + g, s_end);
    unsigned m = 0u;
    for (int s = a; s < b; ++s) m = max(m, cmax[s - s0]);
    if (m) atomicMax(&col_max[px], m);
  }
}

template <class T, int VB>
void edge_max_go(const T *in, int rows, int cols, int pitch, int g, unsigned *row_max, unsigned *col_max, hipStream_t stream) {
  constexpr int kStrip = 64 * (VB / (int)sizeof(T));
  const dim3 grid((cols + kStrip - 1) / kStrip, (rows + kBandRows - 1) / kBandRows);
  DRBA_LAUNCH((edge_max_kernel<T, VB>), grid, dim3(kBlock), 0, stream, in, rows, cols, (size_t)pitch, g, row_max, col_max);
}

template <class T>
int edge_max_launch(const T *in, int rows, int cols, int pitch, int group, uint32_t *row_max, uint32_t *col_max, void *stream) {
  if (!in || !row_max || !col_max || rows <= 0 || cols <= 0 || pitch < cols || group <= 0 || cols % group != 0) return DRBA_EINVAL;
  if (((uintptr_t)in & (sizeof(T) - 1)) || (((uintptr_t)row_max | (uintptr_t)col_max) & 3)) return DRBA_EINVAL;
  // the band index is a grid dimension; rows + cols / group is an int in the zeroing launch
  if ((rows + kBandRows - 1) / kBandRows > 65535 || (size_t)rows + (size_t)(cols / group) > (size_t)0x7fffffff) return DRBA_EUNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  const int ncol = cols / group;
  DRBA_LAUNCH(edge_max_zero_kernel, dim3(grid_for((size_t)rows + ncol)), dim3(kBlock), 0, st, row_max, rows, col_max, ncol);
  DRBA_CHECK_LAUNCH();
  const uintptr_t span = (uintptr_t)in | ((uintptr_t)pitch * sizeof(T));  // every row start is aligned to what divides both
  if ((span & 15) == 0)
    edge_max_go<T, 16>(in, rows, cols, pitch, group, row_max, col_max, st);
  else if ((span & 3) == 0)
    edge_max_go<T, 4>(in, rows, cols, pitch, group, row_max, col_max, st);
  else
    edge_max_go<T, (int)sizeof(T)>(in, rows, cols, pitch, group, row_max, col_max, st);
  DRBA_CHECK_LAUNCH();
  return DRBA_OK;
}

}  // namespace

extern "C" int drba_edge_max_u8(const uint8_t *in, int rows, int cols, int pitch, int group, uint32_t *row_max, uint32_t *col_max,
                                void *stream) {
  return edge_max_launch(in, rows, cols, pitch, group, row_max, col_max, stream);
}

extern "C" int drba_edge_max_u16(const uint16_t *in, int rows, int cols, int pitch, int group, uint32_t *row_max, uint32_t *col_max,
                                 void *stream) {
  return edge_max_launch(in, rows, cols, pitch, group, row_max, col_max, stream);
}

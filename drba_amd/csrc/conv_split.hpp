// Split-operand 3x3 convolution backends (conv_split.hip, conv_dma.hip, conv_ks.hip) behind drba_conv3x3 /
// drba_deconv4x4s2.  Every backend numbers its own configurations from 0; conv.hip's run table (kConvRuns / kDeconvRuns) is
// the one place that says where they sit among the public cfg ids.
#pragma once
#include "common.hpp"

#include <stddef.h>
#include <string.h>

namespace drba {

// Two-term fp16 form of the split (conv_split.hip "Two-term form"): activations are pre-scaled by 2^-kSplitActShift
// before the split (undone exactly in the epilogue), so that they stay finite up to 65504 * 2^kSplitActShift.
constexpr int kSplitActShift = 4;

// the PL 16-bit terms of a weight as the kernels expect them: bf16 h, m, l with x = h + m + l (PL = 3), or fp16 h and
// (x - h) * 2^11 (PL = 2); round-to-nearest-even at every step (host side of every split family's pack function)
static inline void split_weight_terms(float x, int PL, unsigned short *bits) {
  if (PL == 3) {
    float r = x;
    for (int t = 0; t < 3; ++t) {
      unsigned u;
      memcpy(&u, &r, 4);
      u += 0x7fffu + ((u >> 16) & 1u);
      u &= 0xffff0000u;
      float h;
      memcpy(&h, &u, 4);
      bits[t] = (unsigned short)(u >> 16);
      r -= h;
    }
  } else {
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)((x - (float)h) * 2048.f);
    memcpy(&bits[0], &h, 2);
    memcpy(&bits[1], &l, 2);
  }
}

// what conv.hip's table needs to know about a backend's configuration: 16-bit terms per operand (3 bf16 / 2 fp16) and the
// convolution stride it was built for; {0, 0} for an id outside the backend's table
struct SplitDesc {
  int planes, stride;
};
// a backend table of n_three_term three-term ids followed by their two-term forms
constexpr int planes(int id, int n_three_term) { return id < n_three_term ? 3 : 2; }

// Packed weights of every split backend: [unit][plane][lane][8 x 16 bit], the PL terms of weight(unit, lane, i) in element i
// (split_weight_terms).  `weight` returns the address of the fp32 weight, or nullptr for padding (stays zero).  The two-term
// form refuses weights beyond fp16 (DRBA_EUNSUPPORTED, common.hpp two_term_weights_ok).
template <class F>
int pack_fragments(const float *w, size_t n_weights, float *packed, size_t units, int PL, F &&weight) {
  if (PL == 2 && !two_term_weights_ok(w, n_weights)) return DRBA_EUNSUPPORTED;
  unsigned short *dst = reinterpret_cast<unsigned short *>(packed);
  memset(dst, 0, units * PL * 64 * 8 * sizeof(unsigned short));
  for (size_t unit = 0; unit < units; ++unit)
    for (int lane = 0; lane < 64; ++lane)
      for (int i = 0; i < 8; ++i) {
        const float *x = weight(unit, lane, i);
        if (!x) continue;
        unsigned short term[3];
        split_weight_terms(*x, PL, term);
        for (int pl = 0; pl < PL; ++pl) dst[((unit * PL + pl) * 64 + lane) * 8 + i] = term[pl];
      }
  return DRBA_OK;
}

// conv_split.hip: three-term and two-term tiles, stride 1 (Cin a multiple of 32) and stride 2 (two-term, any Cin; H, W = the
// INPUT map)
constexpr int kConvSplitCfgs = 20;
SplitDesc conv_split_desc(int id);
bool conv_split_supports(int Cin, int Cout, int id);
size_t conv_split_packed_floats(int Cin, int Cout, int id);
int conv_split_pack(const float *w, float *packed, int Cin, int Cout, int id);
int conv_split_launch(int id, const float *in, const float *packed_w, const float *bias, const float *beta,
                      const float *residual, const float *residual2, float *out, int N, int Cin, int H, int W, int Cout,
                      int act, float post_slope, int pre_act, float pre_slope, void *stream, int pixel_shuffle = 0);
// (pixel_shuffle: MODE 0 tiles that carry the PixelShuffle(2) store form -- the two-term 4 x 32 x 64 ones -- else DRBA_EUNSUPPORTED)

// the same arithmetic with every operand streamed by LDS-DMA and the activations split on the way into the MFMAs
// (conv_dma.hip): Cin = 32, Cout <= 32, W % 4 == 0
constexpr int kConvDmaCfgs = 2;
SplitDesc conv_dma_desc(int id);
bool conv_dma_supports(int Cin, int Cout, int id);
size_t conv_dma_packed_floats(int Cin, int Cout, int id);
int conv_dma_pack(const float *w, float *packed, int Cin, int Cout, int id);
int conv_dma_launch(int id, const float *in, const float *packed_w, const float *bias, const float *beta,
                    const float *residual, const float *residual2, float *out, int N, int Cin, int H, int W, int Cout,
                    int act, float post_slope, int pre_act, float pre_slope, void *stream);

// the same per-wave program with the K dimension split across the waves of a workgroup, for multi-chunk layers on small
// maps (conv_ks.hip): Cin = 64 / 96 / 128 / 192
constexpr int kConvKsCfgs = 2;
SplitDesc conv_ks_desc(int id);
bool conv_ks_supports(int Cin, int Cout, int id);
size_t conv_ks_packed_floats(int Cin, int Cout, int id);
int conv_ks_pack(const float *w, float *packed, int Cin, int Cout, int id);
int conv_ks_launch(int id, const float *in, const float *packed_w, const float *bias, const float *beta, const float *residual,
                   const float *residual2, float *out, int N, int Cin, int H, int W, int Cout, int act, float post_slope,
                   int pre_act, float pre_slope, void *stream);

// transposed convolution 4x4 s2 p1 (conv_split.hip MODE 1)
constexpr int kDeconvSplitCfgs = 9;
SplitDesc deconv_split_desc(int id);
bool deconv_split_supports(int Cin, int Cout, int id);
size_t deconv_split_packed_floats(int Cin, int Cout, int id);
int deconv_split_pack(const float *w, float *packed, int Cin, int Cout, int id);
int deconv_split_launch(int id, const float *in, const float *packed_w, const float *bias, float *out, int N, int Cin, int H,
                        int W, int Cout, int pixel_shuffle, int pre_act, float pre_slope, void *stream);

}  // namespace drba

// Kernel-side view of the C-ABI argument structs.
#pragma once
#include "../../include/jabd.h"

namespace jabd {
typedef jabd_conv_args ConvArgs;
typedef jabd_dw_args DwArgs;
enum {
  ACT_NONE = JABD_ACT_NONE,
  ACT_RELU = JABD_ACT_RELU,
  ACT_LEAKY = JABD_ACT_LEAKY,
  ACT_HSWISH = JABD_ACT_HSWISH,
  ACT_HSIGMOID = JABD_ACT_HSIGMOID,
  ACT_SIGMOID = JABD_ACT_SIGMOID,
};
// The 32x32 GEMM's BatchNorm-backward epilogue (jabd_conv_bn_bwd_sums_f32):
// the GEMM output is the dy of a BatchNorm (+ act) whose pre-BN input x and
// parameters these are; rows: per-32-pixel-tile sums of dz and dz * xhat.
// mask set (jabd_conv_bn_bwd_sums_res_f32): the BatchNorm's act is a ReLU
// after a residual add, taken from its saved output: dz = (y + res) *
// [mask > 0] is what the GEMM writes (gamma / beta / act unused).
struct BnEpi {
  const float* x;
  const float *mean, *invstd, *gamma, *beta;
  float* rows;
  int x_ps, act;
  float slope;
  const float* mask;
  int mask_ps;
};
// One conv call, classified once (conv_setup, conv.hip): every entry point,
// query and route predicate reads these fields.
struct ConvLayer {
  ConvArgs a;        // the arguments, with M and flags set
  bool is1x1;        // 1 x 1, stride 1, no padding (forward or data gradient)
  bool vec4;         // float4 loads of the input rows
  bool v4out;        // float4 epilogue (a.flags & 1)
  bool fast1x1;      // the forward 1x1 kernels' layout: all rows contiguous, v4 both ways
  bool rows_contig;  // output rows, and the residual's, contiguous over an image
  int64_t OHW;
  int Ktot;          // KH * KW * Cin (+ Cin2)
  // the 32x32 weight view covers Cout in whole launches of tn32 in [lo, hi] N tiles
  bool w32(int lo, int hi) const {
    return a.w32 && a.tn32 >= lo && a.tn32 <= hi && a.ntiles32 % a.tn32 == 0 &&
           a.ntiles32 * 32 >= a.Cout;
  }
  // layout the 32x32 kernel's k x k implicit GEMM needs: 32-channel float4
  // stages inside one tap, contiguous output rows
  bool kxk32() const { return vec4 && a.Cin % 32 == 0 && a.x_bs % 4 == 0 && rows_contig; }
  // the arguments with the 32x32 packing in place of the 16x16 one
  ConvArgs view32() const {
    ConvArgs v = a;
    v.w = a.w32;
    v.Ntiles = a.ntiles32;
    return v;
  }
};
// Where jabd_conv2d_nhwc_f32 sends a layer (conv_route, conv.hip), in the
// order the families are asked (the streaming 1x1 and the m32 k x k never
// compete: one takes 1x1 layers only, the other none).  tm / tn: wave tiles
// of the m32 tile, 3x3 tile and generic kernels; m32 stream: tn N tiles, ks
// K stages; ks of the m32 tile: its K split given a workspace (1: none).
enum ConvFamily {
  kFamStem7, kFamM32Stream, kFamM32Tile, kFamStream, kFamM32Kxk, kFamTile3x3, kFamConv1x1,
  kFamGemm
};
struct ConvRoute {
  ConvFamily family;
  int tm, tn, ks;
};
// conv1x1_stream_dispatch's statistics form (jabd_conv1x1_bn_stats_*)
struct StreamStats {
  float* part;
  float* shift;
  int64_t nblk;
  bool query;
};
}  // namespace jabd

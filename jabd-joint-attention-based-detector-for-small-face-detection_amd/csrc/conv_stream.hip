// A1/A4 short-K, narrow-N 1x1 convolutions as a streaming GEMM: the
// MobileNetV3 project convs at 512^2..128^2 (K 16-120, Cout 16-40), the FPN
// laterals (K 40-80, Cout 40) and the training-forward twins of those layers
// (nets/mobilenetV3.py:146-150 conv3 + bn3 + skip, nets/retinaface_r.py FPN
// output1..3).
//
// These layers are HBM-bound (2 K N / 4 (K + N) = 6-20 FLOP/B, left of the
// 19.7 FLOP/B ridge), and the tile kernel (conv1x1_kernel) holds one or two
// 16-channel K stages in flight per wave: ~1-2 KiB per wave, too little to
// cover HBM latency at the occupancy it gets, and every wave re-reads the
// whole packed weight matrix through L1 for its 16 pixels.  Here:
//  * a persistent workgroup copies the packed weights (Kc x Ntiles KiB) and
//    the per-image ECA gates once into LDS; the four waves then walk 16-pixel
//    blocks (block = wave id + k * waves in the grid, so neighbouring waves
//    stream neighbouring pixels);
//  * every K stage of the NEXT block is issued while the current block runs
//    its MFMAs: stage kc's register is refilled as soon as it has been
//    consumed, so a wave keeps the whole K extent (Kc KiB) of loads in
//    flight and the in-order vmcnt needs no per-stage drain;
//  * B fragments come from LDS (ds_read_b128, one per 4 MFMAs), the ECA gate
//    is applied to A on consumption, bias + residual + activation in
//    registers, NHWC float4 stores straight from the accumulators (four lane
//    groups cover 64 contiguous bytes of a pixel row).
// Operand mapping and packing are those of conv.hip (Wp[kc][nt][lane] =
// float4{W[16kc+4g+e][16nt+j]}); Ntiles == TN (one workgroup covers every
// output channel, so A is read from HBM exactly once).
#include <stdlib.h>

#include <algorithm>

#include "common.h"
#include "conv_args.h"

namespace jabd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float cs_act(float v, int act, float slope) {
  switch (act) {
    case ACT_RELU: return relu_f(v);
    case ACT_LEAKY: return v > 0.f ? v : v * slope;
    case ACT_HSWISH: return hswish_f(v);
    case ACT_HSIGMOID: return hsigmoid_f(v);
    case ACT_SIGMOID: return 1.f / (1.f + expf(-v));
    default: return v;
  }
}

// FULL: p.Kc == KC, every compiled stage is real and the K loop is one basic
// block.  !FULL (the rounded instances, KC - 2 <= p.Kc < KC by stream_kc's
// list): only the last two stages test p.Kc; a stage past p.Kc issues a load
// of the last real stage (an L1 hit, keeps the load sequence unpredicated)
// and skips its MFMAs (wave-uniform branch).
// Within a stage the TN accumulators are interleaved (acc[0..TN) with w.x,
// then with w.y, ...) so consecutive MFMAs are independent, and the LDS
// operands roll one stage ahead in a single register set: fragment u of stage
// kc + 1 is read right behind the last MFMA that uses fragment u of stage kc
// (TN - 1 MFMAs before its first use), the gate float4 of stage kc + 1 behind
// the stage's first MFMA group, across the block boundary too.  Per
// accumulator the order is still bias, then stages in ascending k with
// x, y, z, w inside a stage.
// Workgroup: 4 waves; 8 when the weights exceed 24 KiB (Kc x Ntiles > 24: the
// Cout = 80 layers), so the one workgroup that fits a CU's LDS still gives
// each SIMD two waves.
template <int TN, int KC>
struct CsCfg {
  static constexpr int NW = KC * TN > 24 ? 8 : 4;
};

// ST: also the BatchNorm statistics of the output for the training forward
// (MNv3 Block_eca conv1 -> bn1; no gate, residual or second source): per
// workgroup the shifted sums sum(y - sh), sum((y - sh)^2) over its blocks,
// reduced in a fixed order to stp[blockIdx.x][0|1][Cout] (bn_stats_part's
// format) around sh = the output at pixel 0, which every workgroup computes
// with the same MFMA sequence as the real pixel 0 (workgroup 0 stores it to
// shift[] for bn_stats_final).  Saves bn1's statistics pass over the
// expanded tensor.
template <int TN, int KC, int X2, bool AS, bool ST = false, bool FULL = true>
__global__ __launch_bounds__((CsCfg<TN, KC>::NW * 64)) void conv1x1_stream_kernel(
    const ConvArgs p, int nblk, int ohw, float* __restrict__ stp, float* __restrict__ shift) {
  constexpr int NW = CsCfg<TN, KC>::NW, NT = NW * 64;
  // stages from here on can be partial (K % 16 != 0) or, !FULL, past p.Kc
  constexpr int KTAIL = FULL ? KC - 1 : (KC > 3 ? KC - 3 : 0);
  constexpr int RSTAGE = KC >= 16 ? KC * 3 / 4 : 0;  // where a block requests its residual
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Kc = FULL ? KC : p.Kc;
  f32x4* wl = reinterpret_cast<f32x4*>(smem);
  float4* gl = reinterpret_cast<float4*>(smem + Kc * TN * 64 * 4);
  const int t = threadIdx.x, lane = t & 63, g = lane >> 4, j = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nwv = gridDim.x * NW;
  int blk = blockIdx.x * NW + wave;
  const int M = (int)p.M, Cin = p.Cin, Ktot = p.Cin + (X2 ? p.Cin2 : 0);
  const int c4n = Cin >> 2;
  const float* xg = p.x + p.x_c0;

  // one float4 of A: pixel of lane j in block bk, channels 16kc + 4g .. +3
  auto issue = [&](int bk, int kc) -> float4 {
    int m = bk * 16 + j;
    m = m < M ? m : M - 1;
    const int kq = (FULL || kc < KC - 2 || kc < Kc ? kc : Kc - 1) * 16 + 4 * g;
    const float* src;
    if (X2 && kq >= Cin) {
      const int k2 = kq - Cin < p.Cin2 ? kq - Cin : 0;
      src = p.x2 + m * p.x2_ps + k2;
    } else {
      // only a stage from KTAIL on can reach past Cin; the others keep kq a
      // constant so it folds into the load's immediate offset
      src = xg + m * p.x_ps + (!X2 && kc >= KTAIL && kq >= Cin ? 0 : kq);
    }
    return *reinterpret_cast<const float4*>(src);
  };

  // the first block's operands are requested before the weights, so their
  // HBM latency runs under the staging below
  float4 bias[TN];
#pragma unroll
  for (int u = 0; u < TN; ++u) {
    const int n0 = 16 * u + 4 * g;
    bias[u] = p.bias && n0 < p.Cout ? *reinterpret_cast<const float4*>(p.bias + n0)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float4 A[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) A[kc] = issue(blk < nblk ? blk : 0, kc);
  {
    // every load of a thread is in flight before its first LDS write (loads
    // past the end re-read the last float4, their writes are dropped)
    const f32x4* ws = reinterpret_cast<const f32x4*>(p.w);
    const int nw = Kc * TN * 64;
    constexpr int NI = (KC * TN * 64 + NT - 1) / NT;
    f32x4 wv[NI];
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      const int i = t + q * NT;
      wv[q] = ws[i < nw ? i : nw - 1];
    }
    if (AS) {
      // gate rows: a wave takes rows wave, wave + NW, ... (four in flight),
      // its lanes the row's float4 -- no division.  Rows past the end fold
      // onto the last row (the same bytes written again), so neither the
      // loads nor the writes carry a test.
      const int64_t bs = p.ascale_bs;
      const int bl = p.B - 1;
      for (int c = lane; c < c4n; c += 64) {
        for (int b0 = wave; b0 < p.B; b0 += 4 * NW) {
          const int b1 = min(b0 + NW, bl), b2 = min(b0 + 2 * NW, bl), b3 = min(b0 + 3 * NW, bl);
          const float* s0 = p.ascale + 4 * c;
          const float4 v0 = *reinterpret_cast<const float4*>(s0 + b0 * bs);
          const float4 v1 = *reinterpret_cast<const float4*>(s0 + b1 * bs);
          const float4 v2 = *reinterpret_cast<const float4*>(s0 + b2 * bs);
          const float4 v3 = *reinterpret_cast<const float4*>(s0 + b3 * bs);
          gl[b0 * c4n + c] = v0;
          gl[b1 * c4n + c] = v1;
          gl[b2 * c4n + c] = v2;
          gl[b3 * c4n + c] = v3;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      const int i = t + q * NT;
      if (i < nw) wl[i] = wv[q];
    }
  }
  __syncthreads();
  // ST: the shift (pixel 0's output, channels 16u + 4g .. +3 in every lane)
  float4 sh[ST ? TN : 1], ss[ST ? TN : 1], sq[ST ? TN : 1];
  if (ST) {
    f32x4 a0[TN];
#pragma unroll
    for (int u = 0; u < TN; ++u) {
      const int n0 = 16 * u + 4 * g;
      const float4 bb = p.bias && n0 < p.Cout ? *reinterpret_cast<const float4*>(p.bias + n0)
                                              : make_float4(0.f, 0.f, 0.f, 0.f);
      a0[u] = (f32x4){bb.x, bb.y, bb.z, bb.w};
    }
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      if (!FULL && kc >= p.Kc) break;
      const int kq = kc * 16 + 4 * g;
      const float4 a = kq < p.Cin ? *reinterpret_cast<const float4*>(p.x + p.x_c0 + kq)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < TN; ++u) {
        const f32x4 w = wl[(kc * TN + u) * 64 + lane];
        a0[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, a.x, a0[u], 0, 0, 0);
        a0[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, a.y, a0[u], 0, 0, 0);
        a0[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, a.z, a0[u], 0, 0, 0);
        a0[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, a.w, a0[u], 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < TN; ++u) {
      sh[u] = make_float4(cs_act(a0[u][0], p.act, p.slope), cs_act(a0[u][1], p.act, p.slope),
                          cs_act(a0[u][2], p.act, p.slope), cs_act(a0[u][3], p.act, p.slope));
      ss[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      sq[u] = ss[u];
      const int n0 = 16 * u + 4 * g;
      if (blockIdx.x == 0 && wave == 0 && j == 0 && n0 < p.Cout)
        *reinterpret_cast<float4*>(shift + n0) = sh[u];
    }
  }
  if (!ST && blk >= nblk) return;  // no barrier below (ST: the reduction has one)

  // LDS operands of one stage: the TN weight fragments, and the gate float4
  // of image gi (skip-source and padded channels read the row's first float4,
  // which the consumer replaces by 1)
  auto wfrag = [&](int kc, int u) -> f32x4 {
    return wl[((FULL || kc < KC - 2 || kc < Kc ? kc : 0) * TN + u) * 64 + lane];
  };
  auto gate = [&](int gi, int kc) -> float4 {
    const int kq = kc * 16 + 4 * g;
    const bool sel = X2 || kc >= KTAIL;
    return gl[gi * c4n + (!sel || kq < Cin ? kq >> 2 : 0)];
  };
  // stage 0 of the first block; every later stage is read from the stage before
  int gb = AS && blk < nblk ? (blk * 16) / ohw : 0;  // block-uniform (host: ohw % 16 == 0)
  // residual row base, pixel stride and channel bound as uniform values (a
  // null residual: stride 0 on the weights), so the loads carry no branch
  const float* rbase = p.res ? p.res + p.res_c0 : reinterpret_cast<const float*>(p.w);
  const int rps = p.res ? p.res_ps : 0, rcout = p.res ? p.Cout : 0;
  f32x4 wc[TN];
  float4 gc = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
  for (int u = 0; u < TN; ++u) wc[u] = wfrag(0, u);
  if (AS) gc = gate(gb, 0);

  for (; blk < nblk;) {
    const int nxt = blk + nwv;
    const int bnx = nxt < nblk ? nxt : blk;  // last block: harmless re-read
    const int m = blk * 16 + j;
    // residual loads are issued unconditionally (a null residual reads the
    // first weight float4, an L2 hit) so the vmcnt of the A stages behind
    // them stays exact; the long-K instances, which are at the register
    // limit, request them three quarters through the K loop (RSTAGE)
    float4 R[TN];
    auto residual = [&]() {
      const int mr = m < M ? m : M - 1;
#pragma unroll
      for (int u = 0; u < TN; ++u) {
        const int n0 = 16 * u + 4 * g;
        R[u] = *reinterpret_cast<const float4*>(rbase + mr * rps + (n0 < rcout ? n0 : 0));
      }
    };
    const int gbn = AS ? (bnx * 16) / ohw : 0;
    f32x4 acc[TN];
#pragma unroll
    for (int u = 0; u < TN; ++u) acc[u] = (f32x4){bias[u].x, bias[u].y, bias[u].z, bias[u].w};
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      // this stage's LDS operands are in wc / gc already; each register is
      // refilled for the next stage (the next block's stage 0 after the
      // last) as soon as its last reader has issued
      const int kn = kc + 1 < KC ? kc + 1 : 0;
      const int gnx = kc + 1 < KC ? gb : gbn;
      if (kc == RSTAGE) residual();
      float4 a = A[kc];
      const int kq = kc * 16 + 4 * g;
      // the partial last stage and the skip source's ungated channels exist
      // only from KTAIL on (X2: the source boundary can be anywhere)
      if (kc >= KTAIL && kq >= Ktot) a = make_float4(0.f, 0.f, 0.f, 0.f);
      if (AS) {
        if (X2 || kc >= KTAIL) {
          const bool gk = kq < Cin;
          a.x *= gk ? gc.x : 1.f; a.y *= gk ? gc.y : 1.f;
          a.z *= gk ? gc.z : 1.f; a.w *= gk ? gc.w : 1.f;
        } else {
          a.x *= gc.x; a.y *= gc.y; a.z *= gc.z; a.w *= gc.w;
        }
      }
      if (FULL || kc < KC - 2) {
#pragma unroll
        for (int u = 0; u < TN; ++u)
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].x, a.x, acc[u], 0, 0, 0);
        if (AS) gc = gate(gnx, kn);
#pragma unroll
        for (int u = 0; u < TN; ++u)
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].y, a.y, acc[u], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < TN; ++u)
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].z, a.z, acc[u], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < TN; ++u) {
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].w, a.w, acc[u], 0, 0, 0);
          wc[u] = wfrag(kn, u);
        }
        // pin that order: x group, gate read, y and z groups, then the w
        // group with a fragment read behind each of its MFMAs
        __builtin_amdgcn_sched_group_barrier(0x8, TN, 0);
        if (AS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x8, 2 * TN, 0);
#pragma unroll
        for (int u = 0; u < TN; ++u) {
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
      } else {
        // !FULL, last two stages: p.Kc decides (wave-uniform branch)
        if (kc < Kc) {
#pragma unroll
          for (int u = 0; u < TN; ++u)
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].x, a.x, acc[u], 0, 0, 0);
#pragma unroll
          for (int u = 0; u < TN; ++u)
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].y, a.y, acc[u], 0, 0, 0);
#pragma unroll
          for (int u = 0; u < TN; ++u)
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].z, a.z, acc[u], 0, 0, 0);
#pragma unroll
          for (int u = 0; u < TN; ++u)
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].w, a.w, acc[u], 0, 0, 0);
        }
        if (AS) gc = gate(gnx, kn);
#pragma unroll
        for (int u = 0; u < TN; ++u) wc[u] = wfrag(kn, u);
      }
      // refill after the MFMAs have read the stage: the load can take the
      // stage's own registers (no loop-carried copy, which would wait vmcnt(0))
      A[kc] = issue(bnx, kc);
      // a stage's reads stay in that stage: without this the scheduler hoists
      // every stage's LDS reads to the top of the block and spills them
      __builtin_amdgcn_sched_barrier(0);
    }
    gb = gbn;
    // acc[u][r] = Y[pixel m][16u + 4g + r]
    if (m < M) {
#pragma unroll
      for (int u = 0; u < TN; ++u) {
        const int n0 = 16 * u + 4 * g;
        if (n0 < p.Cout) {
          float4 v = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
          if (p.res) {
            v.x += R[u].x; v.y += R[u].y; v.z += R[u].z; v.w += R[u].w;
          }
          v.x = cs_act(v.x, p.act, p.slope);
          v.y = cs_act(v.y, p.act, p.slope);
          v.z = cs_act(v.z, p.act, p.slope);
          v.w = cs_act(v.w, p.act, p.slope);
          *reinterpret_cast<float4*>(p.y + m * p.y_ps + p.y_c0 + n0) = v;
          if (ST) {
            const float4 d = make_float4(v.x - sh[u].x, v.y - sh[u].y, v.z - sh[u].z, v.w - sh[u].w);
            ss[u].x += d.x; ss[u].y += d.y; ss[u].z += d.z; ss[u].w += d.w;
            sq[u].x = fmaf(d.x, d.x, sq[u].x); sq[u].y = fmaf(d.y, d.y, sq[u].y);
            sq[u].z = fmaf(d.z, d.z, sq[u].z); sq[u].w = fmaf(d.w, d.w, sq[u].w);
          }
        }
      }
    }
    if (nxt >= nblk) break;
    blk = nxt;
  }
  if (ST) {
    // lanes j of a channel quad g: xor-tree over j (fixed order), then the
    // waves in order through LDS (the weights are dead by now)
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        ss[u].x += __shfl_xor(ss[u].x, off); ss[u].y += __shfl_xor(ss[u].y, off);
        ss[u].z += __shfl_xor(ss[u].z, off); ss[u].w += __shfl_xor(ss[u].w, off);
        sq[u].x += __shfl_xor(sq[u].x, off); sq[u].y += __shfl_xor(sq[u].y, off);
        sq[u].z += __shfl_xor(sq[u].z, off); sq[u].w += __shfl_xor(sq[u].w, off);
      }
    __syncthreads();
    float4* red = reinterpret_cast<float4*>(smem);  // [NW][2][TN * 4]
    if (j == 0) {
#pragma unroll
      for (int u = 0; u < TN; ++u) {
        red[(wave * 2 + 0) * TN * 4 + 4 * u + g] = ss[u];
        red[(wave * 2 + 1) * TN * 4 + 4 * u + g] = sq[u];
      }
    }
    __syncthreads();
    if (t < 2 * TN * 4) {
      const int which = t / (TN * 4), q = t - which * (TN * 4);  // q = 4u + g: channels 4q..
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int w = 0; w < NW; ++w) {
        const float4 a = red[(w * 2 + which) * TN * 4 + q];
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
      }
      if (4 * q < p.Cout)
        *reinterpret_cast<float4*>(stp + ((int64_t)blockIdx.x * 2 + which) * p.Cout + 4 * q) = v;
    }
  }
}

// JABD_CONV_STREAM=0 disables the streaming kernel (A/B).
static bool conv_stream_on() {
  static const bool on = env_digit("JABD_CONV_STREAM") != 0;
  return on;
}

static int stream_kc(int kc) {
  static const int ks[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 13, 16, 18};
  for (int k : ks)
    if (kc <= k) return k;
  return -1;
}

template <typename Kern>
static int stream_grid(Kern kern, int threads, size_t lds, int64_t nwg) {
  int dev = 0, ncu = 0, occ = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, threads, lds) != hipSuccess ||
      occ < 1)
    return -1;
  const int64_t cap = (int64_t)ncu * occ;
  return (int)(nwg < cap ? nwg : cap);
}

// The (TN, KC) instances of the plain form; the statistics form has those
// with KC <= 4.  One list for the predicate and the launcher.
#define CS_ROW(X, TN_) X(TN_, 1) X(TN_, 2) X(TN_, 3) X(TN_, 4) X(TN_, 5) X(TN_, 6) X(TN_, 8)
#define CS_INSTANCES(X)                                          \
  CS_ROW(X, 1) CS_ROW(X, 2) CS_ROW(X, 3) CS_ROW(X, 4) CS_ROW(X, 5) \
  X(2, 10) X(3, 10) X(3, 12) X(5, 10) X(5, 12) X(5, 13) X(5, 16) X(5, 18)
#define CS_STATS_INSTANCES(X)                                                           \
  X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(1, 2) X(2, 2) X(3, 2) X(4, 2) X(5, 2) \
  X(1, 3) X(2, 3) X(3, 3) X(4, 3) X(5, 3) X(1, 4) X(2, 4) X(3, 4) X(4, 4) X(5, 4)

// The KC that stream_kc rounds a smaller Kc up to: only these also have the
// !FULL form; every other KC is reached by Kc == KC alone.
static constexpr bool stream_kc_rounds(int kc) {
  return kc == 8 || kc == 10 || kc == 12 || kc == 16 || kc == 18;
}

template <int TN, int KC, int X2, bool AS, bool FULL>
static int stream_launch_form(const ConvArgs& a, hipStream_t st, size_t lds, int64_t nblk,
                              int64_t ohw) {
  auto kern = conv1x1_stream_kernel<TN, KC, X2, AS, false, FULL>;
  constexpr int nw = CsCfg<TN, KC>::NW;
  const int grid = stream_grid(kern, nw * 64, lds, cdiv(nblk, nw));
  if (grid < 1) return -1;
  kern<<<grid, nw * 64, lds, st>>>(a, (int)nblk, (int)ohw, nullptr, nullptr);
  return check_launch("conv1x1_stream", 100 * KC + TN);
}

template <int TN, int KC, int X2, bool AS>
static int stream_launch(const ConvArgs& a, hipStream_t st, size_t lds, int64_t nblk,
                         int64_t ohw) {
  if (a.Kc == KC) return stream_launch_form<TN, KC, X2, AS, true>(a, st, lds, nblk, ohw);
  if constexpr (stream_kc_rounds(KC))
    return stream_launch_form<TN, KC, X2, AS, false>(a, st, lds, nblk, ohw);
  return -1;
}

// Whether this kernel serves a layer of the fast-1x1 layouts (contiguous NHWC
// rows, v4 epilogue, x2 at the same resolution); stats: its statistics form
// (no gate, no second source, no residual).  The route (conv.hip) and the
// dispatch below both ask here; only the occupancy query of the launch can
// still turn a served layer away.
bool conv1x1_stream_serves(const ConvArgs& a, bool stats) {
  if (!conv_stream_on()) return false;
  if (stats && (a.x2 || a.ascale || a.res || stream_kc(a.Kc) > 4)) return false;
  const int TN = a.Ntiles, KC = stream_kc(a.Kc);
  if (TN < 1 || TN > 5 || KC < 0) return false;
  if (a.x2 && a.x2_stride != 1) return false;
  const int64_t ohw = (int64_t)a.OH * a.OW;
  if (a.ascale && (ohw % 16 || a.ascale_bs % 4)) return false;
  const size_t lds = (size_t)a.Kc * TN * 1024 + (a.ascale ? (size_t)a.B * a.Cin * 4 : 0);
  if (lds > (a.Kc * TN > 24 ? 150 : 40) * 1024) return false;
  if (cdiv(a.M, 16) >= ((int64_t)1 << 27)) return false;
  // the kernel forms pixel offsets m * ps in 32-bit ints (the caller's fast1x1
  // condition already bounds (M + 64) * (max ps + 16) < 2^31; kept here so the
  // kernel never relies on a caller's check)
  const int64_t maxps = std::max<int64_t>(std::max<int64_t>(a.x_ps, a.y_ps),
                                          std::max<int64_t>(a.res ? a.res_ps : 0,
                                                            a.x2 ? a.x2_ps : 0));
  if ((a.M + 16) * (maxps + 16) >= ((int64_t)1 << 31)) return false;
  // the instance's wave count (CsCfg, from the rounded KC) must be the one the
  // LDS bound above assumed (from Kc)
  if ((a.Kc * TN > 24) != (KC * TN > 24)) return false;
  // the !FULL form tests p.Kc on its last two stages only
  if (KC - a.Kc > 2 || (KC != a.Kc && !stream_kc_rounds(KC))) return false;
#define CS_HAS(TN_, KC_) \
  if (TN == TN_ && KC == KC_) return true;
  CS_INSTANCES(CS_HAS)
#undef CS_HAS
  return false;
}

// Called from jabd_conv2d_nhwc_f32 for the layers conv1x1_stream_serves takes.
// Returns -1 when the shape is not served.
// ss != nullptr: the statistics form (ST).  ss->query: only report the grid
// (= partial rows) in ss->nblk; otherwise launch and require ss->nblk to
// match it.
int conv1x1_stream_dispatch(const ConvArgs& a, hipStream_t st, StreamStats* ss) {
  if (!conv1x1_stream_serves(a, ss != nullptr)) return -1;
  const int TN = a.Ntiles, KC = stream_kc(a.Kc);
  const int64_t ohw = (int64_t)a.OH * a.OW;
  const size_t lds = (size_t)a.Kc * TN * 1024 + (a.ascale ? (size_t)a.B * a.Cin * 4 : 0);
  const int64_t nblk = cdiv(a.M, 16);
  const int x2 = a.x2 ? 1 : 0;
  const bool as = a.ascale != nullptr;
#define CS_LAUNCH(TN_, KC_, X2_, AS_)                                                       \
  return stream_launch<TN_, KC_, X2_, AS_>(a, st, lds, nblk, ohw)
#define CS_LAUNCH_ST(TN_, KC_)                                                              \
  do {                                                                                      \
    auto kern = conv1x1_stream_kernel<TN_, KC_, 0, false, true>;                            \
    constexpr int nw_ = CsCfg<TN_, KC_>::NW;                                                \
    const int grid = stream_grid(kern, nw_ * 64, lds, cdiv(nblk, nw_));                     \
    if (grid < 1) return -1;                                                                \
    if (ss->query) {                                                                        \
      ss->nblk = grid;                                                                      \
      return 0;                                                                             \
    }                                                                                       \
    JABD_REQUIRE(ss->nblk == grid && ss->part && ss->shift,                                 \
                 "conv1x1_bn_stats: %lld partial rows given, kernel grid %d",               \
                 (long long)ss->nblk, grid);                                                \
    kern<<<grid, nw_ * 64, lds, st>>>(a, (int)nblk, (int)ohw, ss->part, ss->shift);         \
    return check_launch("conv1x1_stream_stats", 100 * KC_ + TN_);                           \
  } while (0)
#define CS_FLAGS_ST(TN_, KC_) \
  if (ss && TN == TN_ && KC == KC_) CS_LAUNCH_ST(TN_, KC_);
  CS_STATS_INSTANCES(CS_FLAGS_ST)
  if (ss) return -1;
#undef CS_FLAGS_ST
#undef CS_LAUNCH_ST
#define CS_FLAGS(TN_, KC_)                      \
  if (TN == TN_ && KC == KC_) {                 \
    if (x2 == 0 && !as) CS_LAUNCH(TN_, KC_, 0, false); \
    if (x2 == 0 && as) CS_LAUNCH(TN_, KC_, 0, true);   \
    if (x2 == 1 && !as) CS_LAUNCH(TN_, KC_, 1, false); \
    CS_LAUNCH(TN_, KC_, 1, true);               \
  }
  CS_INSTANCES(CS_FLAGS)
#undef CS_FLAGS
#undef CS_LAUNCH
  return -1;
}

}  // namespace jabd

// Gaussian Soft-NMS on gfx950: the reference's softer_nms (utils/utils_bbox.py:
// 65-114), batched, one workgroup per image, bit-exact with the literal loop
// on the arithmetic of softnms_math.h (tests/_softnms_ref.c compiles the same
// header).  Instead of deleting the neighbours of a selected box, the rule
// decays their scores by exp(-IoU^2 / sigma) and drops a row only once its
// score falls below `prune`.
//
// The reference's loop, on rows (x1, y1, x2, y2, score) in input order:
//   for i = 0, 1, ... while i < N:
//     m = first position in [i, N) of the maximum score; swap rows m and i
//     for pos = i + 1 ... (N shrinking):
//       o = IoU(row i, row pos)                    fp32, "+offset" form
//       if o > 0: score[pos] = fp32(double(score[pos]) * exp(-(o * o) / sigma))
//                 if score[pos] < prune: swap rows pos and N - 1; N -= 1; stay
//   result: rows [0, N) in array order.
// The swaps decide the output order and which of two equal scores is selected
// first, so they are reproduced, not only the surviving set.  One inner loop
// (a sweep) decays every position in (i, N) exactly once; with N' the number
// of survivors, the dead positions below N', ascending, receive the surviving
// positions at or above N', descending, and nothing else moves.  A sweep is
// therefore: parallel decay, one workgroup scan of the dead flags (which ranks
// both sides: a survivor at p >= N' has (N - 1 - p) - (dead above p) survivors
// above it), and a scatter through a hole table.
//
// Per image the kernel
//   1. compacts the candidates (row < n_valid, score >= threshold; a NaN score
//      fails) in ascending row order;
//   2. top_k > 0 and more candidates: finds the top_k-th largest score key by a
//      bitwise radix select and compacts again, keeping larger keys and the
//      first equal ones (the stable descending order's cut);
//   3. stages the candidates' boxes as float4 and sets up the state, a
//      permutation of candidates and their working scores;
//   4. runs the loop above: workgroup argmax (key << 32 | ~position, so ties
//      go to the lowest position), decay, scan, relocation.  Position i is
//      final once selected and goes straight to keep / keep_scores.
// The outer variable rises strictly to a bound that only shrinks, every inner
// loop is counted, and no workgroup waits for another: the kernel ends
// whatever the data.
//
// Two forms, by the host-known bound on the candidates (n, or top_k when it
// cuts below n): the state (permutation, scores, hole table; 10 bytes per
// candidate) in LDS up to kSoftLdsRows, in the caller's workspace above.
//
// Compile with -ffp-contract=off (EXACT_SRCS).
#include <math.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "nms_internal.h"
#include "softnms_math.h"

namespace jabd {

static constexpr int kSoftT = 1024;  // one workgroup: 16 waves
static constexpr int kSoftWaves = kSoftT / 64;
// 10 bytes per candidate + the static slots within the 160 KiB of a CU
static constexpr int64_t kSoftLdsRows = 16000;
static constexpr int64_t kSoftMaxRows = int64_t(1) << 24;
static constexpr uint32_t kSoftDead = 0x80000000u;  // marks a permutation entry whose row died
static constexpr int kSoftBatch = 4;  // box gathers in flight per thread in the decay

static size_t soft_lds_bytes(int64_t cap) { return (size_t)(cap * 8 + (cap / 2 + 1) * 4); }
// the host-known bound on an image's candidates
static int64_t soft_cap(int64_t n, int64_t top_k) { return top_k > 0 && top_k < n ? top_k : n; }

struct SoftWs {
  float4* sbox;  // [B, n] candidate boxes
  int* crow;     // [B, n] candidate -> input row
  float* csc;    // [B, n] candidate scores (input values)
  int* perm;     // [B, n]   the state of the workspace form
  float* sc;     // [B, n]
  int* hole;     // [B, n / 2 + 1]
};

template <typename A>
static void carve_soft(A& a, int64_t batch, int64_t n, SoftWs* w) {
  SoftWs t;
  t.sbox = a.template take<float4>(batch * n);
  t.crow = a.template take<int>(batch * n);
  t.csc = a.template take<float>(batch * n);
  t.perm = a.template take<int>(batch * n);
  t.sc = a.template take<float>(batch * n);
  t.hole = a.template take<int>(batch * (n / 2 + 1));
  if (w) *w = t;
}

size_t soft_nms_ws_bytes(int64_t batch, int64_t n) {
  Sizer s;
  carve_soft(s, batch, n, (SoftWs*)nullptr);
  return s.used;
}

struct SoftSlots {
  unsigned long long best[kSoftWaves];
  int row[kSoftWaves];
  float sc[kSoftWaves];
  int cnt[kSoftWaves];
};

// every thread gets the sum of v over the workgroup (two barriers)
__device__ __forceinline__ int soft_block_sum(int v, int* cnt) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = v;
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int q = 0; q < kSoftWaves; ++q) all += cnt[q];
  __syncthreads();
  return all;
}

// Ordered compaction step: `flag` per thread (threads in position order) ->
// the number of flagged threads before this one; *all receives the total.
// One barrier before the counts are read and one after.
__device__ __forceinline__ int soft_rank(bool flag, int* cnt, int* all) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (l == 0) cnt[w] = __popcll(m);
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < kSoftWaves; ++q) {
    const int c = cnt[q];
    pre += q < w ? c : 0;
    tot += c;
  }
  __syncthreads();
  *all = tot;
  return pre + __popcll(m & ((1ull << l) - 1ull));
}

template <bool LDS>
__global__ __launch_bounds__(kSoftT) void soft_nms_kernel(
    const float* __restrict__ boxes, int64_t box_stride, int64_t box_bstride,
    const float* __restrict__ scores, int64_t score_stride, int64_t score_bstride,
    const int64_t* __restrict__ n_valid, int64_t n, int cap, double sigma, float offset,
    double prune, float score_thr, int64_t top_k, SoftWs ws, int64_t* __restrict__ keep,
    float* __restrict__ keep_scores, int64_t* __restrict__ n_keep) {
  extern __shared__ __align__(16) unsigned char soft_dyn[];
  __shared__ SoftSlots slots;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int64_t nv = n_valid ? n_valid[b] : n;
  nv = nv < 0 ? 0 : (nv > n ? n : nv);
  const float* bx_in = boxes + (int64_t)b * box_bstride;
  const float* sc_in = scores + (int64_t)b * score_bstride;
  float4* sbox = ws.sbox + (int64_t)b * n;
  int* crow = ws.crow + (int64_t)b * n;
  float* csc = ws.csc + (int64_t)b * n;
  int* perm;
  float* sc;
  int* hole;
  if constexpr (LDS) {
    perm = reinterpret_cast<int*>(soft_dyn);
    sc = reinterpret_cast<float*>(perm + cap);
    hole = reinterpret_cast<int*>(sc + cap);
  } else {
    perm = ws.perm + (int64_t)b * n;
    sc = ws.sc + (int64_t)b * n;
    hole = ws.hole + (int64_t)b * (n / 2 + 1);
  }
  keep += (int64_t)b * n;
  keep_scores += (int64_t)b * n;

  // 1. candidates, ascending rows
  int M = 0;
  for (int64_t r0 = 0; r0 < nv; r0 += kSoftT) {
    const int64_t r = r0 + t;
    float s = 0.f;
    bool valid = false;
    if (r < nv) {
      s = sc_in[r * score_stride];
      valid = s >= score_thr;  // a NaN fails; -inf keeps every other row
    }
    int all;
    const int k = soft_rank(valid, slots.cnt, &all);
    if (valid) {
      crow[M + k] = (int)r;
      csc[M + k] = s;
    }
    M += all;
  }
  __syncthreads();

  // 2. the top_k cut
  if (top_k > 0 && (int64_t)M > top_k) {
    uint32_t kth = 0;         // becomes the key of the top_k-th best candidate
    int krem = (int)top_k;    // how many candidates of exactly that key are taken
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t want = kth | (1u << bit);
      const uint32_t mask = ~((1u << bit) - 1u);
      int c = 0;
      for (int p = t; p < M; p += kSoftT) c += (jabd_sn_key(csc[p]) & mask) == want ? 1 : 0;
      c = soft_block_sum(c, slots.cnt);
      if (c >= krem) kth = want; else krem -= c;
    }
    int out = 0, eq_seen = 0;
    for (int c0 = 0; c0 < M; c0 += kSoftT) {
      const int c = c0 + t;
      int row = 0;
      float s = 0.f;
      uint32_t key = 0;
      const bool in = c < M;
      if (in) {
        row = crow[c];
        s = csc[c];
        key = jabd_sn_key(s);
      }
      const bool eq = in && key == kth;
      int all_eq, all_take;
      const int eq_rank = eq_seen + soft_rank(eq, slots.cnt, &all_eq);
      const bool take = in && (key > kth || (eq && eq_rank < krem));
      // every read of this chunk is done (barriers in soft_rank); the
      // destinations are at or below the sources
      const int d = out + soft_rank(take, slots.cnt, &all_take);
      if (take) {
        crow[d] = row;
        csc[d] = s;
      }
      out += all_take;
      eq_seen += all_eq;
      __syncthreads();
    }
    M = out;
  }

  // 3. boxes and state
  for (int c = t; c < M; c += kSoftT) {
    const float* bx = bx_in + (int64_t)crow[c] * box_stride;
    sbox[c] = make_float4(bx[0], bx[1], bx[2], bx[3]);
    perm[c] = c;
    sc[c] = csc[c];
  }
  __syncthreads();

  // 4. select, decay, relocate
  int N = M;
  for (int i = 0; i < N; ++i) {
    unsigned long long best = 0;  // no (key, position) pair packs to 0
    for (int p = i + t; p < N; p += kSoftT) {
      const unsigned long long v =
          ((unsigned long long)jabd_sn_key(sc[p]) << 32) | (unsigned long long)(~(uint32_t)p);
      best = v > best ? v : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long v = __shfl_xor(best, o);
      best = v > best ? v : best;
    }
    if (lane == 0) {
      slots.best[wv] = best;
      if (best != 0) {
        const int p = (int)(~(uint32_t)best);
        slots.row[wv] = (int)((uint32_t)perm[p] & ~kSoftDead);
        slots.sc[wv] = sc[p];
      }
    }
    __syncthreads();
    int win = 0;
    best = slots.best[0];
#pragma unroll
    for (int q = 1; q < kSoftWaves; ++q) {
      const unsigned long long v = slots.best[q];
      if (v > best) {
        best = v;
        win = q;
      }
    }
    const int m = (int)(~(uint32_t)best);  // i <= m < N
    const int rm = slots.row[win];
    const float sm = slots.sc[win];
    // row i moves to position m (the swap); position i is final and is not
    // read again, so the selected row goes straight to the output
    const int ri = (int)((uint32_t)perm[i] & ~kSoftDead);
    const float si = sc[i];
    if (t == 0) {
      keep[i] = (int64_t)crow[rm];
      keep_scores[i] = sm;
    }
    const int L = N - (i + 1);
    if (L == 0) break;
    const float4 bi = sbox[rm];
    // consecutive positions per thread (the scan ranks threads in position
    // order); an odd count keeps the LDS accesses of a wave off one bank
    const int C = ((L + kSoftT - 1) / kSoftT) | 1;
    const int p0 = min(N, i + 1 + t * C), p1 = min(N, p0 + C);
    int nd = 0;
    // kSoftBatch positions at a time: their state, then their boxes (the
    // gathers of a batch are in flight together), then decay and store
    for (int pb = p0; pb < p1; pb += kSoftBatch) {
      int c[kSoftBatch];
      float s[kSoftBatch];
      float4 bj[kSoftBatch];
#pragma unroll
      for (int u = 0; u < kSoftBatch; ++u) {
        const int p = pb + u;
        const bool own = p < p1 && p != m;  // position m holds row i's old state (the swap)
        c[u] = own ? (int)((uint32_t)perm[p] & ~kSoftDead) : (p < p1 ? ri : rm);
        s[u] = own ? sc[p] : si;
      }
#pragma unroll
      for (int u = 0; u < kSoftBatch; ++u) bj[u] = sbox[c[u]];
#pragma unroll
      for (int u = 0; u < kSoftBatch; ++u) {
        const int p = pb + u;
        if (p < p1) {
          const float o =
              jabd_sn_iou(bi.x, bi.y, bi.z, bi.w, bj[u].x, bj[u].y, bj[u].z, bj[u].w, offset);
          float v = s[u];
          bool dead = false;
          if (o > 0.f) {  // a NaN overlap decays nothing
            v = jabd_sn_decay(v, o, sigma);
            dead = (double)v < prune;
          }
          perm[p] = dead ? (int)((uint32_t)c[u] | kSoftDead) : c[u];
          sc[p] = v;
          nd += dead ? 1 : 0;
        }
      }
    }
    // dead rows before this thread's positions, and in all
    int incl = nd;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) slots.cnt[wv] = incl;
    __syncthreads();
    int before = incl - nd, D = 0;
#pragma unroll
    for (int q = 0; q < kSoftWaves; ++q) {
      const int c = slots.cnt[q];
      before += q < wv ? c : 0;
      D += c;
    }
    if (D > 0) {  // uniform
      const int Np = N - D;
      int dr = before, low = 0;  // low: this thread's dead rows below Np
      for (int p = p0; p < p1; ++p) {
        if ((uint32_t)perm[p] & kSoftDead) {
          if (p < Np) {
            hole[dr] = p;  // dr < (dead rows below Np) <= L / 2
            ++low;
          }
          ++dr;
        }
      }
      __syncthreads();
      // Only positions at or above Np are read from here on: the holes below
      // Np are being filled (by any thread) and no longer tell dead from alive.
      dr = before + low;
      for (int p = max(p0, Np); p < p1; ++p) {
        const uint32_t c = (uint32_t)perm[p];
        if (c & kSoftDead) {
          ++dr;
        } else {
          // survivors above p: (N - 1 - p) less the dead rows above p
          const int h = hole[(N - 1 - p) - (D - dr)];
          perm[h] = (int)c;
          sc[h] = sc[p];
        }
      }
      N = Np;
    }
    __syncthreads();
  }
  if (t == 0) n_keep[b] = (int64_t)N;
}

int soft_nms_core(const float* boxes, int64_t box_stride, int64_t box_bstride,
                  const float* scores, int64_t score_stride, int64_t score_bstride,
                  const int64_t* n_valid, int64_t batch, int64_t n, double sigma, float offset,
                  double prune, float score_thr, int64_t top_k, int64_t* keep,
                  float* keep_scores, int64_t* n_keep, void* ws, size_t ws_bytes,
                  hipStream_t st) {
  JABD_REQUIRE(n >= 0 && batch >= 0, "soft_nms: negative size");
  JABD_REQUIRE(sigma > 0.0 && std::isfinite(sigma),
               "soft_nms: sigma must be positive and finite, got %g", sigma);
  JABD_REQUIRE(std::isfinite(offset), "soft_nms: offset must be finite, got %g", (double)offset);
  JABD_REQUIRE(std::isfinite(prune), "soft_nms: prune must be finite, got %g", prune);
  JABD_REQUIRE(n < kSoftMaxRows, "soft_nms: n=%lld exceeds %lld rows per image", (long long)n,
               (long long)kSoftMaxRows);
  JABD_REQUIRE(batch <= 0x7fffffff, "soft_nms: batch=%lld too large", (long long)batch);
  if (batch == 0) return JABD_OK;
  JABD_REQUIRE(n_keep, "soft_nms: null n_keep");
  if (n == 0) {
    const FillRange fr{n_keep, (int64_t)sizeof(int64_t) * batch, 0u};
    return fill_ranges(&fr, 1, st);
  }
  JABD_REQUIRE(boxes && scores && keep && keep_scores, "soft_nms: null pointer");
  JABD_REQUIRE(ws && ws_bytes >= soft_nms_ws_bytes(batch, n), "soft_nms: workspace %zu < %zu",
               ws_bytes, soft_nms_ws_bytes(batch, n));
  Carve cv(ws, ws_bytes);
  SoftWs w;
  carve_soft(cv, batch, n, &w);
  if (!cv.ok()) {
    set_error("soft_nms: workspace carve overflow");
    return JABD_EWS;
  }
  const int64_t cap = soft_cap(n, top_k);
  if (cap <= kSoftLdsRows) {
    const size_t lds = soft_lds_bytes(cap);
    if (lds + sizeof(SoftSlots) > 64 * 1024) {
      JABD_HIP(hipFuncSetAttribute((const void*)soft_nms_kernel<true>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)soft_lds_bytes(kSoftLdsRows)));
    }
    soft_nms_kernel<true><<<(unsigned)batch, kSoftT, lds, st>>>(
        boxes, box_stride, box_bstride, scores, score_stride, score_bstride, n_valid, n, (int)cap,
        sigma, offset, prune, score_thr, top_k, w, keep, keep_scores, n_keep);
    return check_launch("soft_nms_lds", 1);
  }
  soft_nms_kernel<false><<<(unsigned)batch, kSoftT, 0, st>>>(
      boxes, box_stride, box_bstride, scores, score_stride, score_bstride, n_valid, n, (int)cap,
      sigma, offset, prune, score_thr, top_k, w, keep, keep_scores, n_keep);
  return check_launch("soft_nms_ws", 2);
}

}  // namespace jabd

extern "C" int jabd_soft_nms_workspace_size(int64_t batch, int64_t n, size_t* bytes) {
  JABD_REQUIRE(bytes && batch >= 0 && n >= 0, "soft_nms_workspace_size: bad args");
  *bytes = jabd::soft_nms_ws_bytes(batch, n);
  return JABD_OK;
}

extern "C" int jabd_batched_soft_nms_f32(const float* boxes, int64_t box_stride,
                                         int64_t box_bstride, const float* scores,
                                         int64_t score_stride, int64_t score_bstride,
                                         const int64_t* n_valid, int64_t batch, int64_t n,
                                         double sigma, float offset, double prune,
                                         float score_threshold, int64_t top_k, int64_t* keep,
                                         float* keep_scores, int64_t* n_keep, void* ws,
                                         size_t ws_bytes, jabd_stream_t stream) {
  JABD_REQUIRE(box_stride >= 4 && score_stride >= 1, "soft_nms: bad row stride");
  return jabd::soft_nms_core(boxes, box_stride, box_bstride, scores, score_stride, score_bstride,
                             n_valid, batch, n, sigma, offset, prune, score_threshold, top_k,
                             keep, keep_scores, n_keep, ws, ws_bytes, jabd::as_stream(stream));
}

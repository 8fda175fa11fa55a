// Box voting on gfx950: the merge step of multi-scale / flip test-time
// detection.  Each cluster of overlapping boxes is replaced by its
// score-weighted mean box; batched, one workgroup per image.
//
// Per image, on rows (x1, y1, x2, y2, score, extra...):
//   alive = rows r < n_valid with score >= threshold (a NaN score fails)
//   while a row is alive:
//     seed    = the alive row of the largest score (jabd_sn_key order; among
//               equal scores the lowest row)
//     members = { alive j : IoU(seed, j) >= (float)vote_threshold } + { seed }
//               (jabd_sn_iou: fp32, "+offset" form; a NaN overlap is no member)
//     alive  -= members
//     if |members| >= min_votes:
//       box = (float)(sum score_j * coord_j / sum score_j), products and sums
//             in double; score and the columns from 5 on are the seed row's
//       emit the row; stop after max_out rows
//
// Form: a workgroup argmax per seed, like the selection of soft_nms_kernel,
// over a state indexed by input row (no compaction: the seed is its own row
// index, and rows that are no candidates start dead).  The state is one
// float4 box, one score and one int per row:
//   own[r] = kAlive            still to be clustered
//            kNone             no candidate, or the seed of a dropped cluster
//            s >= 0            a member of the cluster seeded by row s
//            kSeedBase - k     the seed of result row k
// so the owner of a row is found at the end through its seed, whatever
// min_votes decided after the row was taken.  Thread t owns the rows
// congruent to t modulo the workgroup size in every pass, so own[] needs no
// barrier inside the loop.  A seed step is one sweep over the alive rows
// (membership test, kill, fp64 partial sums, and the argmax of the rows that
// stay alive: the next seed), wave butterflies, one barrier (the slots
// alternate between two sets), then the per-wave partials added in wave order.
// The butterfly adds the same two values in both lanes and the wave order is
// fixed, so the sums do not depend on scheduling: two runs agree bit for bit.
//
// The loop is counted by the row bound, every step kills at least its seed,
// and no workgroup waits for another: the kernel ends whatever the data.
//
// Two forms by the host-known n: the state (24 bytes per row) in LDS up to
// kVoteLdsRows rows, in the caller's workspace above.
//
// Compile with -ffp-contract=off (EXACT_SRCS): jabd_sn_iou rounds as in
// soft_nms.hip.
#include <math.h>

#include <cmath>

#include "common.h"
#include "softnms_math.h"

namespace jabd {

static constexpr int kVoteT = 1024;  // one workgroup: 16 waves
static constexpr int kVoteWaves = kVoteT / 64;
static constexpr int kVoteRowBytes = 24;  // float4 box + float score + int own
// (163840 - sizeof(VoteSlots)) / 24 = 6757 rows fit the 160 KiB of a CU; the
// bound is that rounded down to a multiple of half the workgroup
static constexpr int64_t kVoteLdsRows = 6656;
static constexpr int64_t kVoteMaxRows = int64_t(1) << 24;
static constexpr int kAlive = -2, kNone = -1, kSeedBase = -4;

struct VoteWs {
  float4* box;  // [B, n]
  float* sc;    // [B, n]
  int* own;     // [B, n]
};

template <typename A>
static void carve_vote(A& a, int64_t batch, int64_t n, VoteWs* w) {
  VoteWs t;
  t.box = a.template take<float4>(batch * n);
  t.sc = a.template take<float>(batch * n);
  t.own = a.template take<int>(batch * n);
  if (w) *w = t;
}

static size_t box_vote_ws_bytes(int64_t batch, int64_t n) {
  Sizer s;
  if (n > kVoteLdsRows) carve_vote(s, batch, n, (VoteWs*)nullptr);
  return s.used;
}

struct VoteSlots {  // two of each: a step writes one parity while the other is read
  unsigned long long best[2][kVoteWaves];
  double sum[2][kVoteWaves][5];  // score, score * x1, y1, x2, y2
  int cnt[2][kVoteWaves];
};

// (score key, row) as one u64 whose maximum is the next seed: the largest key
// (jabd_sn_key order), the lowest row among equal keys
__device__ __forceinline__ unsigned long long vote_pack(float s, int r) {
  return ((unsigned long long)jabd_sn_key(s) << 32) | (unsigned long long)(~(uint32_t)r);
}
__device__ __forceinline__ unsigned long long vote_max(unsigned long long a,
                                                       unsigned long long b) {
  return a > b ? a : b;
}
__device__ __forceinline__ unsigned long long vote_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = vote_max(v, __shfl_xor(v, o));
  return v;
}
static_assert(kVoteLdsRows * kVoteRowBytes + sizeof(VoteSlots) <= 160 * 1024,
              "the LDS form's state exceeds a CU's LDS");

template <bool LDS>
__global__ __launch_bounds__(kVoteT) void box_vote_kernel(
    const float* __restrict__ rows, int64_t row_stride, int64_t row_bstride, int cols,
    const int64_t* __restrict__ n_valid, int64_t n, float thr, float offset, float score_thr,
    int min_votes, int64_t max_out, VoteWs ws, float* __restrict__ out,
    int64_t* __restrict__ n_out, int64_t* __restrict__ seed_out, int* __restrict__ votes_out,
    int* __restrict__ owner) {
  extern __shared__ __align__(16) unsigned char vote_dyn[];
  __shared__ VoteSlots slots;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int64_t nv64 = n_valid ? n_valid[b] : n;
  nv64 = nv64 < 0 ? 0 : (nv64 > n ? n : nv64);
  const int nv = (int)nv64;  // n < 2^24
  const float* in = rows + (int64_t)b * row_bstride;
  float4* box;
  float* sc;
  int* own;
  if constexpr (LDS) {
    box = reinterpret_cast<float4*>(vote_dyn);
    sc = reinterpret_cast<float*>(box + n);
    own = reinterpret_cast<int*>(sc + n);
  } else {
    box = ws.box + (int64_t)b * n;
    sc = ws.sc + (int64_t)b * n;
    own = ws.own + (int64_t)b * n;
  }
  out += (int64_t)b * n * cols;
  seed_out += (int64_t)b * n;
  votes_out += (int64_t)b * n;

  // the state; thread t owns rows t, t + kVoteT, ... here and in every pass
  for (int r = t; r < nv; r += kVoteT) {
    const float* p = in + (int64_t)r * row_stride;
    const float s = p[4];
    box[r] = make_float4(p[0], p[1], p[2], p[3]);
    sc[r] = s;
    own[r] = s >= score_thr ? kAlive : kNone;  // a NaN fails; -inf keeps every other row
  }
  __syncthreads();

  // the first seed: a sweep of its own; every later one is found by the
  // membership sweep of the step before, among the rows that stay alive
  {
    unsigned long long best = 0;  // no (key, row) pair packs to 0
    for (int r = t; r < nv; r += kVoteT)
      if (own[r] == kAlive) best = vote_max(best, vote_pack(sc[r], r));
    best = vote_wave_max(best);
    if (lane == 0) slots.best[0][wv] = best;
  }
  __syncthreads();

  int emitted = 0;
  for (int step = 0; step < nv; ++step) {
    const int p = step & 1;  // the slots alternate: one barrier per step
    unsigned long long best = slots.best[p][0];
#pragma unroll
    for (int q = 1; q < kVoteWaves; ++q) best = vote_max(best, slots.best[p][q]);
    if (best == 0) break;  // uniform: nothing alive
    const int sd = (int)(~(uint32_t)best);  // 0 <= sd < nv, alive
    const float4 bs = box[sd];
    const float ss = sc[sd];

    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
    int cnt = 0;
    unsigned long long next = 0;
    for (int r = t; r < nv; r += kVoteT) {
      if (own[r] != kAlive) continue;
      const float4 bj = box[r];
      const float sj = sc[r];
      const float o = jabd_sn_iou(bs.x, bs.y, bs.z, bs.w, bj.x, bj.y, bj.z, bj.w, offset);
      if (o >= thr || r == sd) {  // a NaN overlap is no member
        const double s = (double)sj;
        a0 += s;
        a1 += s * (double)bj.x;  // the products are exact (24 x 24 bits)
        a2 += s * (double)bj.y;
        a3 += s * (double)bj.z;
        a4 += s * (double)bj.w;
        ++cnt;
        own[r] = sd;  // the seed's own entry is settled below, by this thread
      } else {
        next = vote_max(next, vote_pack(sj, r));
      }
    }
    if (__any(cnt)) {  // wave-uniform; most waves hold no member of a cluster
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
        a2 += __shfl_xor(a2, o);
        a3 += __shfl_xor(a3, o);
        a4 += __shfl_xor(a4, o);
        cnt += __shfl_xor(cnt, o);
      }
    }
    next = vote_wave_max(next);
    if (lane == 0) {
      slots.sum[p][wv][0] = a0;
      slots.sum[p][wv][1] = a1;
      slots.sum[p][wv][2] = a2;
      slots.sum[p][wv][3] = a3;
      slots.sum[p][wv][4] = a4;
      slots.cnt[p][wv] = cnt;
      slots.best[p ^ 1][wv] = next;
    }
    // Slots of parity p are read after this barrier and written again two
    // barriers later; best[p ^ 1] was last read before the previous barrier.
    __syncthreads();
    int votes = 0;
#pragma unroll
    for (int q = 0; q < kVoteWaves; ++q) votes += slots.cnt[p][q];
    const bool emit = votes >= min_votes;  // uniform
    if ((sd & (kVoteT - 1)) == t) own[sd] = emit ? kSeedBase - emitted : kNone;
    if (emit) {
      float* o = out + (int64_t)emitted * cols;
      if (t < 4) {
        double den = 0.0, num = 0.0;
        for (int q = 0; q < kVoteWaves; ++q) {  // the waves in order
          den += slots.sum[p][q][0];
          num += slots.sum[p][q][1 + t];
        }
        o[t] = (float)(num / den);
      } else if (t == 4) {
        o[4] = ss;
        seed_out[emitted] = (int64_t)sd;
        votes_out[emitted] = votes;
      }
      const uint32_t* src = reinterpret_cast<const uint32_t*>(in + (int64_t)sd * row_stride);
      for (int c = 5 + t; c < cols; c += kVoteT) reinterpret_cast<uint32_t*>(o)[c] = src[c];
      ++emitted;
      if (max_out > 0 && (int64_t)emitted >= max_out) break;  // uniform
    }
  }
  if (t == 0) n_out[b] = (int64_t)emitted;
  if (owner) {
    __syncthreads();  // own[] of other threads' rows is read
    owner += (int64_t)b * n;
    for (int64_t r = t; r < n; r += kVoteT) {
      int v = r < nv ? own[r] : kNone;
      if (v >= 0) v = own[v];  // a member: its seed's entry
      owner[r] = v <= kSeedBase ? kSeedBase - v : -1;
    }
  }
}

}  // namespace jabd

using namespace jabd;

extern "C" int jabd_box_vote_workspace_size(int64_t batch, int64_t n, size_t* bytes) {
  JABD_REQUIRE(bytes && batch >= 0 && n >= 0, "box_vote_workspace_size: bad args");
  *bytes = box_vote_ws_bytes(batch, n);
  return JABD_OK;
}

extern "C" int jabd_box_vote_f32(const float* rows, int64_t row_stride, int64_t row_bstride,
                                 int32_t cols, const int64_t* n_valid, int64_t batch, int64_t n,
                                 double vote_threshold, float offset, float score_threshold,
                                 int32_t min_votes, int64_t max_out, float* out, int64_t* n_out,
                                 int64_t* seed, int32_t* votes, int32_t* owner, void* ws,
                                 size_t ws_bytes, jabd_stream_t stream) {
  JABD_REQUIRE(n >= 0 && batch >= 0, "box_vote: negative size");
  JABD_REQUIRE(vote_threshold == vote_threshold, "box_vote: vote_threshold is NaN");
  JABD_REQUIRE(std::isfinite(offset), "box_vote: offset must be finite, got %g", (double)offset);
  JABD_REQUIRE(cols >= 5, "box_vote: rows need at least 5 columns, got %d", (int)cols);
  JABD_REQUIRE(min_votes >= 1, "box_vote: min_votes must be at least 1, got %d", (int)min_votes);
  JABD_REQUIRE(n < kVoteMaxRows, "box_vote: n=%lld exceeds %lld rows per image", (long long)n,
               (long long)kVoteMaxRows);
  JABD_REQUIRE(row_stride >= cols, "box_vote: row stride %lld < %d columns",
               (long long)row_stride, (int)cols);
  JABD_REQUIRE(batch <= 0x7fffffff, "box_vote: batch=%lld too large", (long long)batch);
  if (batch == 0) return JABD_OK;
  JABD_REQUIRE(n_out, "box_vote: null n_out");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    const FillRange fr{n_out, (int64_t)sizeof(int64_t) * batch, 0u};
    return fill_ranges(&fr, 1, st);
  }
  JABD_REQUIRE(rows && out && seed && votes, "box_vote: null pointer");
  const float thr = (float)vote_threshold;
  if (n <= kVoteLdsRows) {
    const size_t lds = (size_t)n * kVoteRowBytes;
    if (lds + sizeof(VoteSlots) > 64 * 1024) {
      JABD_HIP(hipFuncSetAttribute((const void*)box_vote_kernel<true>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(kVoteLdsRows * kVoteRowBytes)));
    }
    box_vote_kernel<true><<<(unsigned)batch, kVoteT, lds, st>>>(
        rows, row_stride, row_bstride, (int)cols, n_valid, n, thr, offset, score_threshold,
        (int)min_votes, max_out, VoteWs{nullptr, nullptr, nullptr}, out, n_out, seed, votes,
        owner);
    return check_launch("box_vote_lds", 1);
  }
  JABD_REQUIRE(ws && ws_bytes >= box_vote_ws_bytes(batch, n), "box_vote: workspace %zu < %zu",
               ws_bytes, box_vote_ws_bytes(batch, n));
  Carve cv(ws, ws_bytes);
  VoteWs w;
  carve_vote(cv, batch, n, &w);
  if (!cv.ok()) {
    set_error("box_vote: workspace carve overflow");
    return JABD_EWS;
  }
  box_vote_kernel<false><<<(unsigned)batch, kVoteT, 0, st>>>(
      rows, row_stride, row_bstride, (int)cols, n_valid, n, thr, offset, score_threshold,
      (int)min_votes, max_out, w, out, n_out, seed, votes, owner);
  return check_launch("box_vote_ws", 2);
}

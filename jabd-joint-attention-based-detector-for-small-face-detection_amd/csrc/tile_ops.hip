// Tiled (sliced) detection of large images on gfx950: the image -> tile-batch
// gather in front of the fixed-shape forward, and the tile -> image merge of
// the tiles' detect rows behind it.  Semantics: jabd_tile_gather_f32 and
// jabd_tile_collect_f32 in include/jabd.h.
//
// tile_gather: dst[t, c, y, x] = P - mean[c], P the source pixel
// (y0 + y, x0 + x) of an HWC image (float32 or uint8) or `fill` outside it.
// One thread per four output pixels of a row (x fastest): three 16-byte plane
// stores, and, when the four pixels lie inside the image and their first
// source element is 16-byte (float) or 4-byte (uint8) aligned, three 16-byte
// (4-byte) loads of the 12 contiguous HWC values; element loads otherwise.
// 3 * pixel_index is a multiple of 4 exactly when pixel_index is, so the test
// is ((y0 + y) * iw + x0 + x) % 4 == 0.  A tile width that is no multiple of
// 4 takes the one-pixel-per-thread form.  Memory-bound, no reuse, no LDS:
// n_tiles * tile_h * tile_w * (12 or 3 bytes read + 12 written).
//
// tile_collect: two launches, no atomics, no host synchronisation.
//   1. tile_rank_kernel, one workgroup per tile: the rows r < n_keep[t] in
//      chunks of 256; each row's keep flag (the edge filter), a wave ballot,
//      the four waves' counts through LDS and a running total give the row
//      its rank among the tile's survivors (-1: dropped) and the tile its
//      count, both written to the workspace.
//   2. tile_scatter_kernel, one thread per (row, column): a workgroup sums the
//      counts of the tiles before its own (every workgroup in the same order,
//      integers: the position is a function of the data alone), and survivor
//      k of tile t lands at merged[offsets[pass] + before(t) + k].
// Two runs give identical bytes.
//
// Compile with -ffp-contract=off (EXACT_SRCS): (double)v * tile + origin is a
// product and a sum, each rounded once, as the numpy restatement.
#include <math.h>

#include "common.h"

namespace jabd {

static constexpr int kTileT = 256;
static constexpr int kTileWaves = kTileT / 64;

__device__ __forceinline__ float tile_px(const float* p) { return *p; }
__device__ __forceinline__ float tile_px(const uint8_t* p) { return (float)*p; }

// the 12 values of 4 consecutive HWC pixels starting at element e (e % 4 == 0)
__device__ __forceinline__ void tile_load12(const float* src, int64_t e, float* v) {
  const float4* p = reinterpret_cast<const float4*>(src + e);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float4 f = p[q];
    v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
  }
}
__device__ __forceinline__ void tile_load12(const uint8_t* src, int64_t e, float* v) {
  const uint32_t* p = reinterpret_cast<const uint32_t*>(src + e);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const uint32_t w = p[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[4 * q + k] = (float)((w >> (8 * k)) & 0xffu);
  }
}

// VEC = 4: tile_w % 4 == 0, one thread per 4 pixels; VEC = 1: any tile_w
template <typename T, int VEC>
__global__ __launch_bounds__(kTileT) void tile_gather_kernel(
    const T* __restrict__ src, int ih, int iw, const int32_t* __restrict__ origins,
    int64_t total, int tile_h, int tile_w, float fill, float m0, float m1, float m2,
    float* __restrict__ dst) {
  const int64_t i = blockIdx.x * (int64_t)kTileT + threadIdx.x;
  if (i >= total) return;
  const int wq = tile_w / VEC;
  const int64_t row = i / wq;  // t * tile_h + y
  const int x = (int)(i - row * wq) * VEC;
  const int64_t t = row / tile_h;
  const int y = (int)(row - t * tile_h);
  const int64_t sy = (int64_t)origins[2 * t] + y;
  const int64_t sx = (int64_t)origins[2 * t + 1] + x;
  const int64_t plane = (int64_t)tile_h * tile_w;
  float* D = dst + t * 3 * plane + (int64_t)y * tile_w + x;
  const bool yin = sy >= 0 && sy < ih;
  if constexpr (VEC == 4) {
    float v[12];
    const int64_t pix = sy * iw + sx;  // meaningful only when inside
    if (yin && sx >= 0 && sx + 3 < iw && (pix & 3) == 0) {
      tile_load12(src, pix * 3, v);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = yin && sx + k >= 0 && sx + k < iw;
        const T* p = src + (in ? (pix + k) * 3 : 0);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * k + c] = in ? tile_px(p + c) : fill;
      }
    }
    *reinterpret_cast<float4*>(D) = make_float4(v[0] - m0, v[3] - m0, v[6] - m0, v[9] - m0);
    *reinterpret_cast<float4*>(D + plane) =
        make_float4(v[1] - m1, v[4] - m1, v[7] - m1, v[10] - m1);
    *reinterpret_cast<float4*>(D + 2 * plane) =
        make_float4(v[2] - m2, v[5] - m2, v[8] - m2, v[11] - m2);
  } else {
    const bool in = yin && sx >= 0 && sx < iw;
    const T* p = src + (in ? (sy * iw + sx) * 3 : 0);
    D[0] = (in ? tile_px(p) : fill) - m0;
    D[plane] = (in ? tile_px(p + 1) : fill) - m1;
    D[2 * plane] = (in ? tile_px(p + 2) : fill) - m2;
  }
}

struct TileGeom {
  int tile_h, tile_w, image_h, image_w;
  double border, hi_x, hi_y;  // hi = tile - border
};

struct TileWs {
  int* rank;   // [n_tiles, A]: a row's rank among its tile's survivors, -1: dropped
  int* count;  // [n_tiles]
};

template <typename A>
static void carve_tile(A& a, int64_t n_tiles, int64_t rows, TileWs* w) {
  TileWs t;
  t.rank = a.template take<int>(n_tiles * rows);
  t.count = a.template take<int>(n_tiles);
  if (w) *w = t;
}

static size_t tile_ws_bytes(int64_t n_tiles, int64_t rows) {
  Sizer s;
  carve_tile(s, n_tiles, rows, (TileWs*)nullptr);
  return s.used;
}

__device__ __forceinline__ int64_t tile_clamp(int64_t v, int64_t hi) {
  return v < 0 ? 0 : (v > hi ? hi : v);
}

__global__ __launch_bounds__(kTileT) void tile_rank_kernel(
    const float* __restrict__ rows, const int64_t* __restrict__ n_keep, int64_t A,
    const int32_t* __restrict__ origins, TileGeom g, TileWs ws) {
  __shared__ int wave_cnt[2][kTileWaves];  // two sets: one barrier per chunk
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nk = (int)tile_clamp(n_keep[t], A);  // A < 2^31
  const int64_t y0 = origins[2 * t], x0 = origins[2 * t + 1];
  // a side on or beyond the image boundary never filters
  const bool fl = x0 > 0, fr = x0 + g.tile_w < g.image_w;
  const bool ft = y0 > 0, fb = y0 + g.tile_h < g.image_h;
  const float* in = rows + (int64_t)t * A * 15;
  int* rank = ws.rank + (int64_t)t * A;
  int running = 0;
  for (int r0 = 0, it = 0; r0 < nk; r0 += kTileT, ++it) {
    const int r = r0 + tid;
    bool keep = false;
    if (r < nk) {
      const float* p = in + (int64_t)r * 15;
      const double bx1 = (double)p[0] * g.tile_w, by1 = (double)p[1] * g.tile_h;
      const double bx2 = (double)p[2] * g.tile_w, by2 = (double)p[3] * g.tile_h;
      // a NaN compares false: such a row is kept
      keep = !((fl && bx1 < g.border) || (fr && bx2 > g.hi_x) || (ft && by1 < g.border) ||
               (fb && by2 > g.hi_y));
    }
    const unsigned long long m = __ballot(keep);
    const int set = it & 1;
    if (lane == 0) wave_cnt[set][wv] = __popcll(m);
    // a set is read after this barrier and written again two barriers later
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < kTileWaves; ++q) {
      const int c = wave_cnt[set][q];
      before += q < wv ? c : 0;
      all += c;
    }
    if (r < nk)
      rank[r] = keep ? running + before + __popcll(m & ((1ull << lane) - 1ull)) : -1;
    running += all;
  }
  if (tid == 0) ws.count[t] = running;
}

__global__ __launch_bounds__(kTileT) void tile_scatter_kernel(
    const float* __restrict__ rows, const int64_t* __restrict__ n_keep, int64_t A,
    const int32_t* __restrict__ origins, TileGeom g, TileWs ws, float* __restrict__ merged,
    int64_t cap, int64_t* __restrict__ offsets, int pass) {
  __shared__ long long wave_sum[kTileWaves];
  const int t = blockIdx.y, n_tiles = gridDim.y, tid = threadIdx.x;
  const int64_t i = blockIdx.x * (int64_t)kTileT + tid;
  const int64_t nk = tile_clamp(n_keep[t], A);
  // the last tile's first workgroup stays: it writes offsets[pass + 1]
  const bool closes = t == n_tiles - 1 && blockIdx.x == 0;
  if (blockIdx.x * (int64_t)kTileT >= nk * 15 && !closes) return;  // uniform
  long long s = 0;  // survivors of the tiles before this one
  for (int q = tid; q < t; q += kTileT) s += ws.count[q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
  __syncthreads();
  long long before = 0;
#pragma unroll
  for (int q = 0; q < kTileWaves; ++q) before += wave_sum[q];
  const int64_t base = tile_clamp(offsets[pass], cap);
  if (closes && tid == 0) {
    const int64_t end = base + before + ws.count[t];
    offsets[pass + 1] = end < cap ? end : cap;  // a slot no thread reads
  }
  const int64_t r = i / 15;
  const int c = (int)(i - r * 15);
  if (r >= nk) return;
  const int k = ws.rank[(int64_t)t * A + r];
  if (k < 0) return;
  const int64_t d = base + before + k;
  if (d >= cap) return;
  const float v = rows[((int64_t)t * A + r) * 15 + c];
  float o = v;
  if (c != 4) {
    const bool isx = ((c < 4 ? c : c - 5) & 1) == 0;
    o = isx ? (float)((double)v * g.tile_w + (double)origins[2 * t + 1])
            : (float)((double)v * g.tile_h + (double)origins[2 * t]);
  }
  merged[d * 15 + c] = o;
}

// a pass without tiles or rows: offsets[pass + 1] = offsets[pass], clamped to [0, cap]
__global__ void tile_close_kernel(int64_t* __restrict__ offsets, int64_t cap, int pass) {
  if (blockIdx.x == 0 && threadIdx.x == 0) offsets[pass + 1] = tile_clamp(offsets[pass], cap);
}

template <typename T>
static int tile_gather_launch(const T* src, int ih, int iw, const int32_t* origins,
                              int64_t n_tiles, int tile_h, int tile_w, float fill,
                              const float* m, float* dst, hipStream_t st) {
  const bool vec = tile_w % 4 == 0;
  const int64_t total = n_tiles * tile_h * (vec ? tile_w / 4 : tile_w);
  const int64_t blocks = cdiv(total, kTileT);
  JABD_REQUIRE(blocks <= 0x7fffffff, "tile_gather: %lld tiles of %dx%d are too many",
               (long long)n_tiles, tile_h, tile_w);
  if (vec) {
    tile_gather_kernel<T, 4><<<(unsigned)blocks, kTileT, 0, st>>>(
        src, ih, iw, origins, total, tile_h, tile_w, fill, m[0], m[1], m[2], dst);
    return check_launch("tile_gather", 4);
  }
  tile_gather_kernel<T, 1><<<(unsigned)blocks, kTileT, 0, st>>>(
      src, ih, iw, origins, total, tile_h, tile_w, fill, m[0], m[1], m[2], dst);
  return check_launch("tile_gather", 1);
}

}  // namespace jabd

using namespace jabd;

extern "C" int jabd_tile_gather_f32(const void* src, int src_is_u8, int ih, int iw,
                                    const int32_t* origins, int64_t n_tiles, int tile_h,
                                    int tile_w, float fill, const float* mean3, float* dst,
                                    jabd_stream_t stream) {
  JABD_REQUIRE(n_tiles >= 0 && ih > 0 && iw > 0 && tile_h > 0 && tile_w > 0,
               "tile_gather: bad size");
  JABD_REQUIRE((int64_t)ih * iw < (int64_t(1) << 40), "tile_gather: image %dx%d too large", ih,
               iw);
  JABD_REQUIRE(n_tiles < (int64_t(1) << 31), "tile_gather: n_tiles=%lld too large",
               (long long)n_tiles);
  JABD_REQUIRE(mean3, "tile_gather: null channel means");
  if (n_tiles == 0) return JABD_OK;
  JABD_REQUIRE(src && origins && dst, "tile_gather: null pointer");
  // the wide loads assume the element alignment of the image's base
  JABD_REQUIRE(((uintptr_t)src & (src_is_u8 ? 3u : 15u)) == 0 && ((uintptr_t)dst & 15u) == 0,
               "tile_gather: src must be %d-byte and dst 16-byte aligned", src_is_u8 ? 4 : 16);
  hipStream_t st = as_stream(stream);
  if (src_is_u8)
    return tile_gather_launch(static_cast<const uint8_t*>(src), ih, iw, origins, n_tiles,
                              tile_h, tile_w, fill, mean3, dst, st);
  return tile_gather_launch(static_cast<const float*>(src), ih, iw, origins, n_tiles, tile_h,
                            tile_w, fill, mean3, dst, st);
}

extern "C" int jabd_tile_collect_workspace_size(int64_t n_tiles, int64_t A, size_t* bytes) {
  JABD_REQUIRE(bytes && n_tiles >= 0 && A >= 0, "tile_collect_workspace_size: bad args");
  *bytes = tile_ws_bytes(n_tiles, A);
  return JABD_OK;
}

extern "C" int jabd_tile_collect_f32(const float* rows, const int64_t* n_keep, int64_t n_tiles,
                                     int64_t A, const int32_t* origins, int tile_h, int tile_w,
                                     int image_h, int image_w, float border, float* merged,
                                     int64_t cap, int64_t* offsets, int32_t pass, void* ws,
                                     size_t ws_bytes, jabd_stream_t stream) {
  JABD_REQUIRE(n_tiles >= 0 && A >= 0 && cap >= 0 && pass >= 0, "tile_collect: bad size");
  JABD_REQUIRE(tile_h > 0 && tile_w > 0 && image_h > 0 && image_w > 0,
               "tile_collect: bad tile or image shape");
  JABD_REQUIRE(border == border, "tile_collect: border is NaN");
  JABD_REQUIRE(n_tiles <= 65535, "tile_collect: n_tiles=%lld exceeds 65535 per call",
               (long long)n_tiles);
  JABD_REQUIRE(A * 15 < (int64_t(1) << 31), "tile_collect: A=%lld too large", (long long)A);
  JABD_REQUIRE(offsets, "tile_collect: null offsets");
  JABD_REQUIRE(n_tiles == 0 || A == 0 || (rows && n_keep && origins),
               "tile_collect: null pointer");
  JABD_REQUIRE(merged || cap == 0, "tile_collect: null merged");
  hipStream_t st = as_stream(stream);
  const TileGeom g{tile_h, tile_w, image_h, image_w, (double)border,
                   (double)tile_w - (double)border, (double)tile_h - (double)border};
  const int64_t nt = (n_tiles == 0 || A == 0) ? 0 : n_tiles;
  JABD_REQUIRE(nt == 0 || (ws && ws_bytes >= tile_ws_bytes(nt, A)),
               "tile_collect: workspace %zu < %zu", ws_bytes, tile_ws_bytes(nt, A));
  if (nt == 0) {  // an empty pass
    tile_close_kernel<<<1, 64, 0, st>>>(offsets, cap, (int)pass);
    return check_launch("tile_collect_empty");
  }
  Carve cv(ws, ws_bytes);
  TileWs w;
  carve_tile(cv, nt, A, &w);
  if (!cv.ok()) {
    set_error("tile_collect: workspace carve overflow");
    return JABD_EWS;
  }
  tile_rank_kernel<<<(unsigned)nt, kTileT, 0, st>>>(rows, n_keep, A, origins, g, w);
  if (int e = check_launch("tile_rank")) return e;
  tile_scatter_kernel<<<dim3((unsigned)cdiv(A * 15, kTileT), (unsigned)nt), kTileT, 0, st>>>(
      rows, n_keep, A, origins, g, w, merged, cap, offsets, (int)pass);
  return check_launch("tile_scatter");
}

// Aligned face crops from the detector's five landmarks (jabd_align_faces_u8,
// semantics in include/jabd.h): per face a least-squares similarity from its
// landmarks to a five-point template, then an inverse warp of the image's
// bytes into a size x size crop, for every face of a chunk of mixed-size
// images in one launch.
//
// One workgroup per (face, band of kAlignT * VEC consecutive output pixels).
// The fit is five points, so every workgroup makes it again for its face
// (thread 0, in double, result through the LDS) instead of a launch in front
// that hands the matrices over; the band-0 workgroup writes the face's matrix.
// The owning image comes from a binary search of the offsets batch_collect
// wrote.  One thread makes VEC = 4 consecutive pixels of a crop row and stores
// whole dwords (uint8 HWC: 12 bytes, float NCHW: three 16-byte plane stores); a
// size that is no multiple of 4, or an output that is not aligned for those
// stores, takes the one-pixel form.  The source reads are byte gathers that do
// not coalesce for a rotated face; a small face's source footprint stays in the
// L2.  The kernel is bound by the latency of those gathers, not by bytes: the
// taps are loaded from clamped addresses and selected afterwards, so that the 48
// loads of a thread's four pixels are in flight together (with a branch around
// each pixel's taps the same work took 1.3x (one sample per pixel) to 5.5x (4 x 4
// sub-samples) as long).  No atomics, no memset, nothing read
// back: the call can be captured in a HIP graph and two runs give identical
// bytes.
//
// This file is built with -ffp-contract=off: tests/_align_ref.py restates the
// arithmetic below operation by operation in numpy.
#include <math.h>

#include "common.h"

namespace jabd {

static constexpr int kAlignT = 256;

struct AlignFit {
  double ia, ib, tx, ty;  // inverse rotation-scale rows (ia, ib), (-ib, ia); translation
  double o[4];            // sub-sample j lies at (x + o[j]) - 0.5, o[j] = (j + 0.5) / s
  int s;                  // sub-samples per axis; 0: the face is invalid
  float m[6];             // the forward matrix, each entry rounded once
};

// lm: the row's ten landmark floats, q: the template's ten.  False (f.s = 0,
// f.m all zero) for an invalid face.
__host__ __device__ inline bool align_fit(const float* lm, const float* q, int antialias,
                                          AlignFit& f) {
  f.ia = f.ib = f.tx = f.ty = 0.0;
  f.o[0] = f.o[1] = f.o[2] = f.o[3] = 0.0;
  f.s = 0;
  for (int k = 0; k < 6; ++k) f.m[k] = 0.f;
  for (int k = 0; k < 10; ++k)
    if (!isfinite(lm[k])) return false;
  double mpx = 0.0, mpy = 0.0, mqx = 0.0, mqy = 0.0;
  for (int i = 0; i < 5; ++i) {
    mpx = mpx + (double)lm[2 * i];
    mpy = mpy + (double)lm[2 * i + 1];
    mqx = mqx + (double)q[2 * i];
    mqy = mqy + (double)q[2 * i + 1];
  }
  mpx = mpx / 5.0;
  mpy = mpy / 5.0;
  mqx = mqx / 5.0;
  mqy = mqy / 5.0;
  double S = 0.0, A = 0.0, B = 0.0;
  for (int i = 0; i < 5; ++i) {
    const double px = (double)lm[2 * i] - mpx, py = (double)lm[2 * i + 1] - mpy;
    const double qx = (double)q[2 * i] - mqx, qy = (double)q[2 * i + 1] - mqy;
    S = S + (px * px + py * py);
    A = A + (px * qx + py * qy);
    B = B + (px * qy - py * qx);
  }
  if (!(S > 0.0)) return false;
  const double a = A / S, b = B / S;
  const double det = a * a + b * b;
  if ((a == 0.0 && b == 0.0) || !(det > 0.0) || !isfinite(det)) return false;
  f.tx = mqx - (a * mpx - b * mpy);
  f.ty = mqy - (b * mpx + a * mpy);
  f.ia = a / det;
  f.ib = b / det;
  int s = 1;
  if (antialias) {  // the smallest s with s * sqrt(det) >= 1, without the root
    s = 4;
    for (int k = 1; k < 4; ++k)
      if ((double)(k * k) * det >= 1.0) {
        s = k;
        break;
      }
  }
  f.s = s;
#pragma unroll
  for (int j = 0; j < 4; ++j) f.o[j] = ((double)j + 0.5) / (double)s;  // j >= s: not read
  f.m[0] = (float)a;
  f.m[1] = (float)(-b);
  f.m[2] = (float)f.tx;
  f.m[3] = (float)b;
  f.m[4] = (float)a;
  f.m[5] = (float)f.ty;
  return true;
}

// Crop pixels (x .. x + VEC - 1, y) of a valid face: each the mean of s x s
// bilinear sub-samples of the RGB HWC uint8 image S [ih, iw, 3]; v[k][c]
// unrounded.  The sub-sample loops are outside the pixels', so what a row of
// sub-samples shares (dv and its two products) is formed once; every pixel
// still adds its sub-samples rows outer, columns inner.
template <int VEC>
__host__ __device__ inline void align_pixels(const uint8_t* S, int ih, int iw, const AlignFit& f,
                                             int x, int y, float v[VEC][3]) {
  const int s = f.s;
  float acc[VEC][3];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.f;
  const double xmax = (double)(iw - 1), ymax = (double)(ih - 1);
  for (int jy = 0; jy < s; ++jy) {
    const double dv = (((double)y + f.o[jy]) - 0.5) - f.ty;
    const double av = f.ia * dv, bv = f.ib * dv;
    for (int jx = 0; jx < s; ++jx) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const double du = (((double)(x + k) + f.o[jx]) - 0.5) - f.tx;
        const double sx = f.ia * du + bv;
        const double sy = av - f.ib * du;
        const double fx = floor(sx), fy = floor(sy);
        // Outside this range (or NaN) all four taps are outside and the sub-sample is 0:
        // the position collapses to (0, 0) with weights 0 and no tap counts, so no int is
        // formed from a wild double.  Every tap is loaded from a clamped, valid address
        // and then selected, without a branch: the loads of a thread's pixels are
        // independent and overlap.
        const bool in = fx >= -1.0 && fx <= xmax && fy >= -1.0 && fy <= ymax;
        const float wx = (float)(in ? sx - fx : 0.0), wy = (float)(in ? sy - fy : 0.0);
        const float ax = 1.f - wx, ay = 1.f - wy;
        const int x0 = (int)(in ? fx : 0.0), y0 = (int)(in ? fy : 0.0);
        const bool xl = in && x0 >= 0, xr = in && x0 + 1 < iw;
        const bool yt = y0 >= 0, yb = y0 + 1 < ih;
        const int xa = x0 < 0 ? 0 : x0, xb = x0 + 1 < iw ? x0 + 1 : iw - 1;
        const int ya = y0 < 0 ? 0 : y0, yc = y0 + 1 < ih ? y0 + 1 : ih - 1;
        const uint8_t* r0 = S + (int64_t)ya * iw * 3;
        const uint8_t* r1 = S + (int64_t)yc * iw * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float q00 = (float)r0[(int64_t)xa * 3 + c], q01 = (float)r0[(int64_t)xb * 3 + c];
          const float q10 = (float)r1[(int64_t)xa * 3 + c], q11 = (float)r1[(int64_t)xb * 3 + c];
          const float p00 = (yt && xl) ? q00 : 0.f, p01 = (yt && xr) ? q01 : 0.f;
          const float p10 = (yb && xl) ? q10 : 0.f, p11 = (yb && xr) ? q11 : 0.f;
          const float top = p00 * ax + p01 * wx;
          const float bot = p10 * ax + p11 * wx;
          acc[k][c] = acc[k][c] + (top * ay + bot * wy);
        }
      }
    }
  }
  const float n = (float)(s * s);
#pragma unroll
  for (int k = 0; k < VEC; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[k][c] = acc[k][c] / n;
}

struct AlignParams {
  float q[10];             // the template
  float mean[3], std[3];   // per output plane (float output)
  int bgr;
};

struct AlignFace {
  const uint8_t* src;
  int ih, iw;
  AlignFit fit;
};

// VEC = 4: size % 4 == 0 and crops aligned for the wide stores; VEC = 1: any.
// F32 = false: uint8 HWC crops, true: float32 NCHW crops.
template <int VEC, bool F32>
__global__ __launch_bounds__(kAlignT) void align_faces_kernel(
    const uint8_t* __restrict__ pool, int64_t pool_bytes, const int64_t* __restrict__ desc,
    int64_t n_images, const float* __restrict__ rows, const int64_t* __restrict__ offsets,
    int64_t cap, AlignParams P, int size, int antialias, int bands, void* __restrict__ crops,
    float* __restrict__ matrices) {
  __shared__ AlignFace face;
  const int64_t r = blockIdx.x / (unsigned)bands;
  const int band = (int)(blockIdx.x - r * bands);
  int64_t count = offsets[n_images];
  if (count > cap) count = cap;
  if (r >= count) return;  // uniform
  if (threadIdx.x == 0) {
    AlignFace fc;
    fc.src = pool;
    fc.ih = fc.iw = 0;
    float lm[10];  // asked for first: the search below does not wait for them
    for (int k = 0; k < 10; ++k) lm[k] = rows[r * 15 + 5 + k];
    // the owning image: the last i with offsets[i] <= r (images without faces repeat an offset)
    int64_t lo = 0, hi = n_images - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (offsets[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int64_t off = desc[3 * lo], ih = desc[3 * lo + 1], iw = desc[3 * lo + 2];
    // the slot rules of jabd_letterbox_batch_u8; 3 * ih * iw <= pool_bytes - off without overflow
    const bool slot = ih > 0 && iw > 0 && ih <= 0x7fffffff && iw <= 0x7fffffff && off >= 0 &&
                      off <= pool_bytes && ih * iw <= (pool_bytes - off) / 3;
    if (align_fit(lm, P.q, antialias, fc.fit) && !slot) {
      fc.fit.s = 0;
      for (int k = 0; k < 6; ++k) fc.fit.m[k] = 0.f;
    }
    if (fc.fit.s > 0) {
      fc.src = pool + off;
      fc.ih = (int)ih;
      fc.iw = (int)iw;
    }
    if (band == 0 && matrices)
      for (int k = 0; k < 6; ++k) matrices[r * 6 + k] = fc.fit.m[k];
    face = fc;
  }
  __syncthreads();
  const int wq = size / VEC;
  const int i = band * kAlignT + (int)threadIdx.x;
  if (i >= size * wq) return;
  const int y = i / wq;
  const int x = (i - y * wq) * VEC;
  const bool valid = face.fit.s > 0;  // an invalid face reads nothing
  float v[VEC][3];
#pragma unroll
  for (int k = 0; k < VEC; ++k) v[k][0] = v[k][1] = v[k][2] = 0.f;
  if (valid) align_pixels<VEC>(face.src, face.ih, face.iw, face.fit, x, y, v);
  const int64_t plane = (int64_t)size * size;
  if constexpr (F32) {
    float* D = static_cast<float*>(crops) + r * 3 * plane + (int64_t)y * size + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int sc = P.bgr ? 2 - c : c;  // the source channel of output plane c
      const float m = P.mean[c], d = P.std[c];
      if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(D + c * plane) =
            make_float4((v[0][sc] - m) / d, (v[1][sc] - m) / d, (v[2][sc] - m) / d,
                        (v[3][sc] - m) / d);
      } else {
        D[c * plane] = (v[0][sc] - m) / d;
      }
    }
  } else {
    uint8_t* D = static_cast<uint8_t*>(crops) + (r * plane + (int64_t)y * size + x) * 3;
    uint32_t b[VEC * 3];
#pragma unroll
    for (int k = 0; k < VEC; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) b[k * 3 + c] = (uint32_t)(int)rintf(v[k][c]);  // 0 .. 255
    if constexpr (VEC == 4) {
      struct alignas(4) U3 {
        uint32_t a, b, c;
      };
      *reinterpret_cast<U3*>(D) = U3{b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24,
                                     b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24,
                                     b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24};
    } else {
      D[0] = (uint8_t)b[0];
      D[1] = (uint8_t)b[1];
      D[2] = (uint8_t)b[2];
    }
  }
}

}  // namespace jabd

using namespace jabd;

extern "C" int jabd_align_faces_u8(const uint8_t* pool, int64_t pool_bytes, const int64_t* desc,
                                   int64_t n_images, const float* rows, const int64_t* offsets,
                                   int64_t cap, const float* template10, int size, int antialias,
                                   int out_kind, const float* mean3, const float* std3, int bgr,
                                   void* crops, float* matrices, jabd_stream_t stream) {
  JABD_REQUIRE(n_images >= 0 && cap >= 0 && pool_bytes >= 0, "align_faces: bad size");
  JABD_REQUIRE(size >= 1 && size <= 1024, "align_faces: size %d outside [1, 1024]", size);
  JABD_REQUIRE(out_kind == JABD_ALIGN_U8_HWC || out_kind == JABD_ALIGN_F32_NCHW,
               "align_faces: unknown out_kind %d", out_kind);
  JABD_REQUIRE(template10, "align_faces: null template");
  AlignParams P{};
  for (int k = 0; k < 10; ++k) {
    JABD_REQUIRE(std::isfinite(template10[k]), "align_faces: template entry %d is not finite", k);
    P.q[k] = template10[k];
  }
  const bool f32 = out_kind == JABD_ALIGN_F32_NCHW;
  JABD_REQUIRE(!f32 || (mean3 && std3), "align_faces: float output needs mean3 and std3");
  for (int c = 0; c < 3; ++c) {
    P.mean[c] = mean3 ? mean3[c] : 0.f;
    P.std[c] = std3 ? std3[c] : 1.f;
    JABD_REQUIRE(std::isfinite(P.mean[c]), "align_faces: mean3[%d] is not finite", c);
    JABD_REQUIRE(std::isfinite(P.std[c]) && P.std[c] != 0.f,
                 "align_faces: std3[%d] is zero or not finite", c);
  }
  P.bgr = bgr ? 1 : 0;
  if (cap == 0 || n_images == 0) return JABD_OK;
  JABD_REQUIRE(desc && rows && offsets && crops && (pool || pool_bytes == 0),
               "align_faces: null pointer");
  const bool vec = size % 4 == 0 && ((uintptr_t)crops & (f32 ? 15u : 3u)) == 0;
  const int bands = (int)cdiv((int64_t)size * (vec ? size / 4 : size), kAlignT);
  JABD_REQUIRE(cap <= 0x7fffffff / bands, "align_faces: cap=%lld too large for size %d",
               (long long)cap, size);
  const unsigned g = (unsigned)(cap * bands);
  hipStream_t st = as_stream(stream);
  const int aa = antialias ? 1 : 0;
#define JABD_ALIGN_LAUNCH(V, F)                                                               \
  align_faces_kernel<V, F><<<g, kAlignT, 0, st>>>(pool, pool_bytes, desc, n_images, rows,     \
                                                  offsets, cap, P, size, aa, bands, crops,    \
                                                  matrices)
  if (vec) {
    if (f32) JABD_ALIGN_LAUNCH(4, true); else JABD_ALIGN_LAUNCH(4, false);
    return check_launch("align_faces", 4);
  }
  if (f32) JABD_ALIGN_LAUNCH(1, true); else JABD_ALIGN_LAUNCH(1, false);
#undef JABD_ALIGN_LAUNCH
  return check_launch("align_faces", 1);
}

// A6-A10 box work on gfx950: decode / decode_landm, the fused predict.py
// post-process, batched anchor matching + encoding, and MultiBoxLoss with
// on-device hard-negative mining.  All HBM-bound integer/fp32 elementwise
// work; compiled with -ffp-contract=off so every float op rounds like the
// reference's separate tensor ops.
#include <math.h>

#include <cmath>

#include "common.h"
#include "nms_internal.h"

namespace jabd {

// ---------------------------------------------------------------------------
// decode / decode_landm — utils/utils_bbox.py:29-46
// ---------------------------------------------------------------------------
struct Box4 {
  float x1, y1, x2, y2;
};

__device__ __forceinline__ Box4 decode_one(const float* l, const float4 p, float v0, float v1) {
  // boxes = cat(p_c + l[:2]*v0*p_wh, p_wh*exp(l[2:]*v1)); boxes[:2] -= boxes[2:]/2;
  // boxes[2:] += boxes[:2]   (each a separate fp32 op, left to right)
  float cx = p.x + (l[0] * v0) * p.z;
  float cy = p.y + (l[1] * v0) * p.w;
  float w = p.z * expf(l[2] * v1);
  float h = p.w * expf(l[3] * v1);
  Box4 b;
  b.x1 = cx - w / 2.f;
  b.y1 = cy - h / 2.f;
  b.x2 = w + b.x1;
  b.y2 = h + b.y1;
  return b;
}

__global__ void decode_kernel(const float* __restrict__ loc, const float4* __restrict__ pri,
                              int64_t A, int64_t total, float v0, float v1,
                              float* __restrict__ out) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  float l[4];
  float4 lv = reinterpret_cast<const float4*>(loc)[i];
  l[0] = lv.x; l[1] = lv.y; l[2] = lv.z; l[3] = lv.w;
  Box4 b = decode_one(l, pri[i % A], v0, v1);
  reinterpret_cast<float4*>(out)[i] = make_float4(b.x1, b.y1, b.x2, b.y2);
}

__global__ void decode_landm_kernel(const float* __restrict__ pre, const float4* __restrict__ pri,
                                    int64_t A, int64_t total, float v0, float* __restrict__ out) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  float4 p = pri[i % A];
  const float* q = pre + i * 10;
  float* o = out + i * 10;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    o[2 * k] = p.x + (q[2 * k] * v0) * p.z;
    o[2 * k + 1] = p.y + (q[2 * k + 1] * v0) * p.w;
  }
}

// predict.py:167-180: rows (x1,y1,x2,y2, conf[:,1], landmarks) per prior.
__global__ void detect_rows_kernel(const float* __restrict__ loc, const float* __restrict__ conf,
                                   const float* __restrict__ landm,
                                   const float4* __restrict__ pri, int64_t A, int64_t total,
                                   float v0, float v1, float* __restrict__ rows) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  float4 p = pri[i % A];
  float l[4];
  float4 lv = reinterpret_cast<const float4*>(loc)[i];
  l[0] = lv.x; l[1] = lv.y; l[2] = lv.z; l[3] = lv.w;
  Box4 b = decode_one(l, p, v0, v1);
  float* r = rows + i * 15;
  r[0] = b.x1; r[1] = b.y1; r[2] = b.x2; r[3] = b.y2;
  r[4] = conf[i * 2 + 1];
  const float* q = landm + i * 10;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    r[5 + 2 * k] = p.x + (q[2 * k] * v0) * p.z;
    r[6 + 2 * k] = p.y + (q[2 * k + 1] * v0) * p.w;
  }
}

__global__ void gather_rows_kernel(const float* __restrict__ rows, const int64_t* __restrict__ keep,
                                   const int64_t* __restrict__ n_keep, int64_t A,
                                   float* __restrict__ out) {
  int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int b = blockIdx.y;
  if (k >= n_keep[b]) return;
  int64_t src = keep[(int64_t)b * A + k];
  const float* r = rows + ((int64_t)b * A + src) * 15;
  float* o = out + ((int64_t)b * A + k) * 15;
#pragma unroll
  for (int c = 0; c < 15; ++c) o[c] = r[c];
}

// ---------------------------------------------------------------------------
// match / encode — nets/retinaface_training.py:8-162
// ---------------------------------------------------------------------------
__device__ __forceinline__ float nan_min(float a, float b) {  // torch.min(a, b)
  return (a != a || b != b) ? __int_as_float(0x7fc00000) : (b < a ? b : a);
}
__device__ __forceinline__ float nan_max(float a, float b) {  // torch.max(a, b)
  return (a != a || b != b) ? __int_as_float(0x7fc00000) : (a < b ? b : a);
}

// jaccard(truth, point_form(prior)) for one pair, reference op order (:20-59).
__device__ __forceinline__ float match_iou(float tx1, float ty1, float tx2, float ty2,
                                           float tarea, float px1, float py1, float px2,
                                           float py2, float parea) {
  float mx = nan_min(tx2, px2), my = nan_min(ty2, py2);
  float nx = nan_max(tx1, px1), ny = nan_max(ty1, py1);
  float iw = nan_max(mx - nx, 0.f), ih = nan_max(my - ny, 0.f);  // clamp(min=0)
  float inter = iw * ih;
  float uni = tarea + parea - inter;
  return inter / uni;
}

// torch max(): larger value wins, NaN beats numbers, ties -> lower index.
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ void prior_point_form(float4 p, float& x1, float& y1, float& x2,
                                                 float& y2, float& area) {
  x1 = p.x - p.z / 2.f;
  y1 = p.y - p.w / 2.f;
  x2 = p.x + p.z / 2.f;
  y2 = p.y + p.w / 2.f;
  area = (x2 - x1) * (y2 - y1);
}

// best_prior_idx per truth (:112-114) and the forced-match scatter (:128-130):
// forced[b][a] = max j with best_prior_idx[j] == a (the last writer of the
// reference's sequential loop).
__global__ __launch_bounds__(256) void match_best_prior_kernel(
    const float* __restrict__ targets, const int64_t* __restrict__ offsets,
    const float4* __restrict__ pri, int64_t A, int* __restrict__ forced) {
  const int b = blockIdx.y;
  const int64_t j = blockIdx.x;
  const int64_t t0 = offsets[b], t1 = offsets[b + 1];
  if (j >= t1 - t0) return;  // every block of an image without targets, too
  const float* tr = targets + (t0 + j) * 15;
  const float tx1 = tr[0], ty1 = tr[1], tx2 = tr[2], ty2 = tr[3];
  const float tarea = (tx2 - tx1) * (ty2 - ty1);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int64_t a = threadIdx.x; a < A; a += blockDim.x) {
    float px1, py1, px2, py2, pa;
    prior_point_form(pri[a], px1, py1, px2, py2, pa);
    float v = match_iou(tx1, ty1, tx2, ty2, tarea, px1, py1, px2, py2, pa);
    if (better(v, (int)a, bv, bi)) { bv = v; bi = (int)a; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    float ov = __shfl_xor(bv, off);
    int oi = __shfl_xor(bi, off);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  __shared__ float sv[4];
  __shared__ int si[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
      if (better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
    atomicMax(&forced[(int64_t)b * A + bi], (int)j);
  }
}

// best_truth per prior (:121-123), forced override (:127-130), threshold
// (:145), encode (:62-73) and encode_landm (:75-86).  kRaw is match_iou()
// (nets/retinaface_training_DIOU.py:176-246): the same assignment, but loc_t
// holds the matched truth box corners (:230-231 `loc = matches`).  An image
// without targets (the reference fails on it) reads no target row: conf_t 0,
// loc_t and landm_t zeros (include/jabd.h).
template <bool kRaw>
__global__ __launch_bounds__(256) void match_assign_kernel(
    const float* __restrict__ targets, const int64_t* __restrict__ offsets,
    const float4* __restrict__ pri, int64_t A, const int* __restrict__ forced,
    float thr, float v0, float v1, float* __restrict__ loc_t, int64_t* __restrict__ conf_t,
    float* __restrict__ landm_t) {
  extern __shared__ float st[];  // [ngt][5]: x1,y1,x2,y2,area
  const int b = blockIdx.y;
  const int64_t t0 = offsets[b];
  const int ngt = (int)(offsets[b + 1] - t0);
  for (int j = threadIdx.x; j < ngt; j += blockDim.x) {
    const float* tr = targets + (t0 + j) * 15;
    float x1 = tr[0], y1 = tr[1], x2 = tr[2], y2 = tr[3];
    st[j * 5 + 0] = x1; st[j * 5 + 1] = y1; st[j * 5 + 2] = x2; st[j * 5 + 3] = y2;
    st[j * 5 + 4] = (x2 - x1) * (y2 - y1);
  }
  __syncthreads();
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (a >= A) return;
  const int64_t ba = (int64_t)b * A + a;
  if (ngt <= 0) {  // an image without targets: all background, zero targets
    conf_t[ba] = 0;
    reinterpret_cast<float4*>(loc_t)[ba] = make_float4(0.f, 0.f, 0.f, 0.f);
    float* lm = landm_t + ba * 10;
#pragma unroll
    for (int k = 0; k < 10; ++k) lm[k] = 0.f;
    return;
  }
  const float4 p = pri[a];
  float px1, py1, px2, py2, pa;
  prior_point_form(p, px1, py1, px2, py2, pa);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int j = 0; j < ngt; ++j) {
    float v = match_iou(st[j * 5], st[j * 5 + 1], st[j * 5 + 2], st[j * 5 + 3], st[j * 5 + 4],
                        px1, py1, px2, py2, pa);
    if (better(v, j, bv, bi)) { bv = v; bi = j; }
  }
  const int f = forced[ba];
  if (f >= 0) { bv = 2.f; bi = f; }
  const float* tr = targets + (t0 + bi) * 15;
  float label = tr[14];
  if (bv < thr) label = 0.f;
  conf_t[ba] = (int64_t)label;
  // encode: ((m_lo+m_hi)/2 - p_c) / (v0*p_wh); log((m_hi-m_lo)/p_wh) / v1
  const float sw = v0 * p.z, sh = v0 * p.w;
  if (kRaw) {
    reinterpret_cast<float4*>(loc_t)[ba] = make_float4(tr[0], tr[1], tr[2], tr[3]);
  } else {
  float gx = (tr[0] + tr[2]) / 2.f - p.x;
  float gy = (tr[1] + tr[3]) / 2.f - p.y;
  gx /= sw;
  gy /= sh;
  float gw = logf((tr[2] - tr[0]) / p.z) / v1;
  float gh = logf((tr[3] - tr[1]) / p.w) / v1;
  reinterpret_cast<float4*>(loc_t)[ba] = make_float4(gx, gy, gw, gh);
  }
  float* lm = landm_t + ba * 10;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    lm[2 * k] = (tr[4 + 2 * k] - p.x) / sw;
    lm[2 * k + 1] = (tr[5 + 2 * k] - p.y) / sh;
  }
}

// ---------------------------------------------------------------------------
// MultiBoxLoss — nets/retinaface_training.py:183-303
// ---------------------------------------------------------------------------
constexpr int kLossBlock = 256;

__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int off = 32; off > 0; off >>= 1) {
    float o = __shfl_xor(v, off);
    v = (o > v || o != o) ? o : v;  // NaN propagates like torch max()
  }
  return v;
}

__device__ __forceinline__ float smooth_l1(float d) {
  float z = fabsf(d);
  return z < 1.f ? 0.5f * z * z : z - 0.5f;
}

// ---------------------------------------------------------------------------
// IoU-family box terms — nets/retinaface_training_DIOU.py: IouLoss (:491-522)
// over decode() (:319-337) and bbox_overlaps_iou/giou/diou/ciou (:339-490),
// paired rows, b1 = the prediction, b2 = the truth:
//   kBoxIou   I/U                                   clamp [0, 1]
//   kBoxGiou  I/U - (C - U)/C, C = ow*oh            clamp [-1, 1]
//   kBoxDiou  I/U - |c2-c1|^2 / |outer|^2           clamp [-1, 1]
//   kBoxCiou  I/U - (|c2-c1|^2/|outer|^2 + a*v)     clamp [-1, 1]
//             v = 4/pi^2 (atan(w2/h2) - atan(w1/h1))^2, a = v/((1 - I/U) + v),
//             a constant in the backward (the reference's no_grad block)
// and the per-row loss is 1 - clamp(value).  kBoxSmoothL1 names the base
// loss's box term in the fused kernels' template parameter.
// ---------------------------------------------------------------------------
constexpr int kBoxSmoothL1 = -1, kBoxIou = 0, kBoxGiou = 1, kBoxDiou = 2, kBoxCiou = 3;

struct IouTerms {
  Box4 b;                                  // prediction corners (bboxes1)
  float w1, h1, iwr, ihr, iw, ih, inter;   // iwr/ihr before clamp(min=0)
  float dcx, dcy, diag, owr, ohr, ow, oh, odiag, uni, d;
  float carea;                             // Giou: the closure's area
  float dat, alpha;                        // Ciou: atan(w2/h2) - atan(w1/h1), a
};

template <int kKind>
__device__ __forceinline__ IouTerms iou_terms(const Box4 b, const float4 t) {
  IouTerms r;
  r.b = b;
  r.w1 = b.x2 - b.x1;
  r.h1 = b.y2 - b.y1;
  const float w2 = t.z - t.x, h2 = t.w - t.y;
  const float area1 = r.w1 * r.h1, area2 = w2 * h2;
  r.iwr = nan_min(b.x2, t.z) - nan_max(b.x1, t.x);
  r.ihr = nan_min(b.y2, t.w) - nan_max(b.y1, t.y);
  r.iw = nan_max(r.iwr, 0.f);
  r.ih = nan_max(r.ihr, 0.f);
  r.inter = r.iw * r.ih;
  if (kKind != kBoxIou) {
    r.owr = nan_max(b.x2, t.z) - nan_min(b.x1, t.x);
    r.ohr = nan_max(b.y2, t.w) - nan_min(b.y1, t.y);
    r.ow = nan_max(r.owr, 0.f);
    r.oh = nan_max(r.ohr, 0.f);
  }
  if (kKind == kBoxDiou || kKind == kBoxCiou) {
    const float cx1 = (b.x2 + b.x1) / 2.f, cy1 = (b.y2 + b.y1) / 2.f;
    const float cx2 = (t.z + t.x) / 2.f, cy2 = (t.w + t.y) / 2.f;
    r.dcx = cx2 - cx1;
    r.dcy = cy2 - cy1;
    r.diag = r.dcx * r.dcx + r.dcy * r.dcy;
    r.odiag = r.ow * r.ow + r.oh * r.oh;
  }
  r.uni = area1 + area2 - r.inter;
  if (kKind == kBoxIou) {
    r.d = r.inter / r.uni;
  } else if (kKind == kBoxGiou) {
    r.carea = r.ow * r.oh;
    r.d = r.inter / r.uni - (r.carea - r.uni) / r.carea;
  } else if (kKind == kBoxDiou) {
    r.d = r.inter / r.uni - r.diag / r.odiag;
  } else {
    const float u = r.diag / r.odiag;
    const float iou = r.inter / r.uni;
    r.dat = atanf(w2 / h2) - atanf(r.w1 / r.h1);
    const float v = 0.40528473456935116f * (r.dat * r.dat);  // 4 / pi^2
    const float S = 1.f - iou;
    r.alpha = v / (S + v);
    r.d = iou - (u + r.alpha * v);
  }
  return r;
}

// torch.clamp(d, lo, 1): lo = 0 for Iou, -1 otherwise.  A NaN stays NaN, as
// torch's does; the DIoU instantiation keeps the form it shipped with.
template <int kKind>
__device__ __forceinline__ float iou_clamp(float d) {
  const float c = fminf(fmaxf(d, kKind == kBoxIou ? 0.f : -1.f), 1.f);
  return (kKind != kBoxDiou && d != d) ? d : c;
}

__device__ __forceinline__ Box4 decode_box(const float4 l, const float4 p, float v0, float v1) {
  const float la[4] = {l.x, l.y, l.z, l.w};
  return decode_one(la, p, v0, v1);
}

template <int kKind>
__device__ __forceinline__ float iou_loss(const float4 l, const float4 p, const float4 t,
                                          float v0, float v1) {
  const float d = iou_terms<kKind>(decode_box(l, p, v0, v1), t).d;
  return 1.f - iou_clamp<kKind>(d);
}

// torch.minimum/maximum backward: the whole gradient to the winner, half each on a tie.
__device__ __forceinline__ float pick_lo(float a, float b) { return a < b ? 1.f : (a == b ? .5f : 0.f); }
__device__ __forceinline__ float pick_hi(float a, float b) { return a > b ? 1.f : (a == b ? .5f : 0.f); }

// Gradient with respect to the prediction's corners (x1, y1, x2, y2) given
// gd = dL/d(clamped value).  clamp() passes the gradient on its closed interval.
template <int kKind>
__device__ __forceinline__ float4 iou_box_grad(const IouTerms& r, const float4 t, float gd) {
  const bool inside = r.d >= (kKind == kBoxIou ? 0.f : -1.f) && r.d <= 1.f;
  if (kKind == kBoxCiou) {
    // autograd's clamp backward zeroes gd outside the interval and the chain
    // goes on: with a = 0/0 (prediction == truth) 0 * a makes the gradient NaN
    gd = inside ? gd : 0.f;
  } else if (!inside) {
    return make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float U2 = r.uni * r.uni;
  float gI = gd * (1.f / r.uni + r.inter / U2);
  float gA1 = gd * (-r.inter / U2);
  const Box4 b = r.b;
  float gx1 = 0.f, gy1 = 0.f, gx2 = 0.f, gy2 = 0.f;
  float gow = 0.f, goh = 0.f;   // gradient of the clamped outer extents' raw values
  if (kKind == kBoxGiou) {
    // -(C - U)/C = U/C - 1: d/dU = 1/C (U = area1 + area2 - I), d/dC = -U/C^2
    const float gU = gd * (1.f / r.carea);
    gA1 += gU;
    gI -= gU;
    const float gC = gd * (-r.uni / (r.carea * r.carea));
    gow = r.owr >= 0.f ? gC * r.oh : 0.f;
    goh = r.ohr >= 0.f ? gC * r.ow : 0.f;
  }
  // area1 = w1*h1
  gx2 += gA1 * r.h1; gx1 -= gA1 * r.h1;
  gy2 += gA1 * r.w1; gy1 -= gA1 * r.w1;
  // inter = clamp(iw)*clamp(ih); iw = min(x2,tx2) - max(x1,tx1)
  const float giw = r.iwr >= 0.f ? gI * r.ih : 0.f;
  const float gih = r.ihr >= 0.f ? gI * r.iw : 0.f;
  gx2 += giw * pick_lo(b.x2, t.z); gx1 -= giw * pick_hi(b.x1, t.x);
  gy2 += gih * pick_lo(b.y2, t.w); gy1 -= gih * pick_hi(b.y1, t.y);
  if (kKind == kBoxDiou || kKind == kBoxCiou) {
    const float gD = gd * (-1.f / r.odiag);
    const float gO = gd * (r.diag / (r.odiag * r.odiag));
    // diag = (c2 - c1)^2, c1 = (x2 + x1)/2
    const float gcx1 = gD * -2.f * r.dcx, gcy1 = gD * -2.f * r.dcy;
    gx1 += gcx1 * .5f; gx2 += gcx1 * .5f;
    gy1 += gcy1 * .5f; gy2 += gcy1 * .5f;
    // odiag = clamp(ow)^2 + clamp(oh)^2; ow = max(x2,tx2) - min(x1,tx1)
    gow = r.owr >= 0.f ? gO * 2.f * r.ow : 0.f;
    goh = r.ohr >= 0.f ? gO * 2.f * r.oh : 0.f;
  }
  if (kKind != kBoxIou) {
    gx2 += gow * pick_hi(b.x2, t.z); gx1 -= gow * pick_lo(b.x1, t.x);
    gy2 += goh * pick_hi(b.y2, t.w); gy1 -= goh * pick_lo(b.y1, t.y);
  }
  if (kKind == kBoxCiou) {
    // -a*v, v = 4/pi^2 dat^2, dat = atan(w2/h2) - atan(q), q = w1/h1
    const float gv = gd * -r.alpha;
    const float gat1 = gv * (0.40528473456935116f * 2.f * r.dat) * -1.f;
    const float q = r.w1 / r.h1;
    const float gq = gat1 / (1.f + q * q);
    const float gw1 = gq / r.h1, gh1 = gq * (-r.w1 / (r.h1 * r.h1));
    gx2 += gw1; gx1 -= gw1;
    gy2 += gh1; gy1 -= gh1;
  }
  return make_float4(gx1, gy1, gx2, gy2);
}

// decode's chain: x1 = cx - W/2, x2 = x1 + W; cx = px + l0*v0*pw, W = pw*exp(l2*v1)
__device__ __forceinline__ float4 decode_grad(const float4 gb, const float4 l, const float4 p,
                                              float v0, float v1) {
  const float gx1 = gb.x, gy1 = gb.y, gx2 = gb.z, gy2 = gb.w;
  const float gcx = gx1 + gx2, gcy = gy1 + gy2;
  const float gW = (gx2 - gx1) * .5f, gH = (gy2 - gy1) * .5f;
  const float W = p.z * expf(l.z * v1);
  const float H = p.w * expf(l.w * v1);
  float4 g;
  g.x = gcx * v0 * p.z;
  g.y = gcy * v0 * p.w;
  g.z = gW * W * v1;
  g.w = gH * H * v1;
  return g;
}

// d(loss)/d(loc) for one positive, scaled by s (= dL/dloss_l / N).
template <int kKind>
__device__ __forceinline__ float4 iou_grad(const float4 l, const float4 p, const float4 t,
                                           float v0, float v1, float s) {
  const IouTerms r = iou_terms<kKind>(decode_box(l, p, v0, v1), t);
  return decode_grad(iou_box_grad<kKind>(r, t, -s), l, p, v0, v1);
}

// The stand-alone paired op (IouLoss / bbox_overlaps_* outside the fused loss):
// one row per thread, float4 in and out, no atomics.  pri == NULL: pred holds
// corner boxes; otherwise loc offsets decoded against pri[i].
template <int kKind>
__global__ void iou_rows_fwd_kernel(const float4* __restrict__ pred,
                                    const float4* __restrict__ pri,
                                    const float4* __restrict__ truth, int64_t n, float v0,
                                    float v1, float* __restrict__ val) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 l = pred[i];
  Box4 b;
  if (pri) {
    b = decode_box(l, pri[i], v0, v1);
  } else {
    b.x1 = l.x; b.y1 = l.y; b.x2 = l.z; b.y2 = l.w;
  }
  val[i] = iou_clamp<kKind>(iou_terms<kKind>(b, truth[i]).d);
}

template <int kKind>
__global__ void iou_rows_bwd_kernel(const float4* __restrict__ pred,
                                    const float4* __restrict__ pri,
                                    const float4* __restrict__ truth, int64_t n, float v0,
                                    float v1, const float* __restrict__ gval,
                                    float4* __restrict__ gpred) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 l = pred[i], t = truth[i];
  Box4 b;
  if (pri) {
    b = decode_box(l, pri[i], v0, v1);
  } else {
    b.x1 = l.x; b.y1 = l.y; b.x2 = l.z; b.y2 = l.w;
  }
  const float4 gb = iou_box_grad<kKind>(iou_terms<kKind>(b, t), t, gval[i]);
  gpred[i] = pri ? decode_grad(gb, l, pri[i], v0, v1) : gb;
}

// Global max of conf (log_sum_exp uses x.data.max(), :86-88): block partials.
__global__ __launch_bounds__(kLossBlock) void conf_max_partial(const float* __restrict__ conf,
                                                               int64_t total,
                                                               float* __restrict__ part) {
  float m = -INFINITY;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = conf[i];
    m = (v > m || v != v) ? v : m;
  }
  m = wave_max(m);
  __shared__ float s[kLossBlock / 64];
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kLossBlock / 64; ++w) m = (s[w] > m || s[w] != s[w]) ? s[w] : m;
    part[blockIdx.x] = m;
  }
}

// Per prior: box/landmark smooth-L1 partials, positive counts, and the
// hard-negative mining loss (lse(x) - x[t], positives zeroed, :256-262).
// kBox >= 0: the box term is that IoU-family loss of the decoded prediction
// against the raw matched truth (retinaface_training_DIOU.py:600-602);
// kBoxSmoothL1: the base loss's, pri/v0/v1 unused.
template <int kBox>
__global__ __launch_bounds__(kLossBlock) void loss_elem_kernel(
    const float* __restrict__ loc, const float* __restrict__ conf,
    const float* __restrict__ landm, const float* __restrict__ loc_t,
    const int64_t* __restrict__ conf_t, const float* __restrict__ landm_t, int64_t A,
    const float4* __restrict__ pri, float v0, float v1,
    const float* __restrict__ gmax_part, int n_gmax_part, float* __restrict__ mining,
    uint8_t* __restrict__ sel, float* __restrict__ part_l, float* __restrict__ part_lm,
    int* __restrict__ npos_img, int* __restrict__ npos1_img) {
  __shared__ float s_gmax;
  if (threadIdx.x == 0) {
    float m = -INFINITY;
    for (int i = 0; i < n_gmax_part; ++i) {
      float v = gmax_part[i];
      m = (v > m || v != v) ? v : m;
    }
    s_gmax = m;
  }
  __syncthreads();
  const float gmax = s_gmax;
  const int b = blockIdx.y;
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  float sl = 0.f, slm = 0.f;
  int p = 0, p1 = 0;
  if (a < A) {
    const int64_t i = (int64_t)b * A + a;
    const int64_t t = conf_t[i];
    const bool pos = t != 0, pos1 = t > 0;
    if (pos) {
      float4 x = reinterpret_cast<const float4*>(loc)[i];
      float4 y = reinterpret_cast<const float4*>(loc_t)[i];
      if constexpr (kBox != kBoxSmoothL1)
        sl = iou_loss<kBox>(x, pri[a], y, v0, v1);
      else
        sl = smooth_l1(x.x - y.x) + smooth_l1(x.y - y.y) + smooth_l1(x.z - y.z) +
             smooth_l1(x.w - y.w);
    }
    if (pos1) {
      const float* x = landm + i * 10;
      const float* y = landm_t + i * 10;
#pragma unroll
      for (int k = 0; k < 10; ++k) slm += smooth_l1(x[k] - y[k]);
    }
    const float c0 = conf[i * 2], c1 = conf[i * 2 + 1];
    const float lse = logf(expf(c0 - gmax) + expf(c1 - gmax)) + gmax;
    const float mine = pos ? 0.f : lse - c0;  // target is 0 for every non-positive
    mining[i] = mine;
    sel[i] = (uint8_t)((pos ? 1 : 0) | (pos1 ? 2 : 0));
    p = pos;
    p1 = pos1;
  }
  sl = wave_sum(sl);
  slm = wave_sum(slm);
  uint64_t bp = __ballot(p), bp1 = __ballot(p1);
  __shared__ float s_l[kLossBlock / 64], s_lm[kLossBlock / 64];
  __shared__ int s_p[kLossBlock / 64], s_p1[kLossBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_l[wave] = sl; s_lm[wave] = slm;
    s_p[wave] = __popcll(bp); s_p1[wave] = __popcll(bp1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tl = 0.f, tlm = 0.f;
    int tp = 0, tp1 = 0;
    for (int w = 0; w < kLossBlock / 64; ++w) {
      tl += s_l[w]; tlm += s_lm[w]; tp += s_p[w]; tp1 += s_p1[w];
    }
    const int64_t blk = (int64_t)b * gridDim.x + blockIdx.x;
    part_l[blk] = tl;
    part_lm[blk] = tlm;
    if (tp) atomicAdd(&npos_img[b], tp);
    if (tp1) atomicAdd(&npos1_img[b], tp1);
  }
}

__device__ __forceinline__ uint32_t fkey_asc(float v) {
  uint32_t f = __float_as_uint(v);
  if (v != v) f = 0x7fc00000u;
  if (f == 0x80000000u) f = 0u;
  return (f & 0x80000000u) ? ~f : (f | 0x80000000u);
}

constexpr int kSelBlock = 1024;

// Per image: radix-select the num_neg-th largest mining loss (:270-276),
// mark pos ∪ neg (bit 2) and sum the cross-entropy of the marked rows
// (:283-293).  Ties at the threshold are taken lowest index first.
__global__ __launch_bounds__(kSelBlock) void ohem_select_kernel(
    const float* __restrict__ mining, const float* __restrict__ conf, int64_t A, int neg_pos,
    const int* __restrict__ npos_img, uint8_t* __restrict__ sel, float* __restrict__ ce_img) {
  const int b = blockIdx.x;
  const float* m = mining + (int64_t)b * A;
  __shared__ int hist[256];
  __shared__ uint32_t s_prefix;
  __shared__ int s_need;
  __shared__ int s_wave[kSelBlock / 64];
  __shared__ float s_wsum[kSelBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t npos = npos_img[b];
  int64_t num_neg = (int64_t)neg_pos * npos;
  if (num_neg > A - 1) num_neg = A - 1;

  uint32_t prefix = 0;
  int need = (int)num_neg;  // still to take among keys matching prefix
  if (num_neg > 0) {
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const uint32_t pmask = pass == 0 ? 0u : (0xffffffffu << (32 - 8 * pass));
      for (int i = tid; i < 256; i += kSelBlock) hist[i] = 0;
      __syncthreads();
      for (int64_t i = tid; i < A; i += kSelBlock) {
        uint32_t k = fkey_asc(m[i]);
        if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int acc = 0, d = 255;
        for (; d > 0; --d) {
          if (acc + hist[d] >= need) break;
          acc += hist[d];
        }
        s_prefix = prefix | ((uint32_t)d << shift);
        s_need = need - acc;
      }
      __syncthreads();
      prefix = s_prefix;
      need = s_need;
      __syncthreads();
    }
  }
  // prefix = key of the num_neg-th largest; take every key > prefix and the
  // first `need` keys == prefix in index order.
  int taken_eq = 0;
  float ce = 0.f;
  for (int64_t base = 0; base < A; base += kSelBlock) {
    const int64_t i = base + tid;
    bool valid = i < A;
    uint32_t k = valid ? fkey_asc(m[i]) : 0u;
    bool gt = valid && num_neg > 0 && k > prefix;
    bool eq = valid && num_neg > 0 && k == prefix;
    uint64_t be = __ballot(eq);
    int rank_in_wave = __popcll(be & (((uint64_t)1 << lane) - 1));
    if (lane == 0) s_wave[wave] = __popcll(be);
    __syncthreads();
    int before = taken_eq;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    int tot = 0;
    for (int w = 0; w < kSelBlock / 64; ++w) tot += s_wave[w];
    bool take_eq = eq && (before + rank_in_wave) < need;
    if (valid) {
      const int64_t gi = (int64_t)b * A + i;
      uint8_t s = sel[gi];
      const bool pos = s & 1;
      if (pos || gt || take_eq) {
        s |= 4;
        sel[gi] = s;
        // F.cross_entropy row: -(x_t - max - log(sum exp(x - max)))
        const float c0 = conf[gi * 2], c1 = conf[gi * 2 + 1];
        const float mx = c0 < c1 ? c1 : c0;
        const float lsm = logf(expf(c0 - mx) + expf(c1 - mx));
        const float xt = pos ? c1 : c0;
        ce += -((xt - mx) - lsm);
      }
    }
    taken_eq += tot;
    __syncthreads();
  }
  ce = wave_sum(ce);
  if (lane == 0) s_wsum[wave] = ce;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < kSelBlock / 64; ++w) t += s_wsum[w];
    ce_img[b] = t;
  }
}

__global__ void loss_final_kernel(const float* __restrict__ part_l,
                                  const float* __restrict__ part_lm, int64_t nparts,
                                  const float* __restrict__ ce_img, const int* __restrict__ npos,
                                  const int* __restrict__ npos1, int batch,
                                  float* __restrict__ sums, int64_t* __restrict__ counts) {
  // one wave; fixed-order partial sums -> deterministic
  const int lane = threadIdx.x;
  float sl = 0.f, slm = 0.f, sc = 0.f;
  int64_t p = 0, p1 = 0;
  for (int64_t i = lane; i < nparts; i += 64) { sl += part_l[i]; slm += part_lm[i]; }
  for (int i = lane; i < batch; i += 64) { sc += ce_img[i]; p += npos[i]; p1 += npos1[i]; }
  sl = wave_sum(sl); slm = wave_sum(slm); sc = wave_sum(sc);
  for (int off = 32; off > 0; off >>= 1) {
    p += __shfl_xor(p, off);
    p1 += __shfl_xor(p1, off);
  }
  if (lane == 0) {
    sums[0] = sl; sums[1] = sc; sums[2] = slm;
    counts[0] = p; counts[1] = p1;
  }
}

__global__ void loss_normalize_kernel(const float* __restrict__ sums,
                                      const int64_t* __restrict__ counts,
                                      float* __restrict__ loss) {
  if (threadIdx.x != 0) return;
  const float n = (float)(counts[0] > 1 ? counts[0] : 1);
  const float n1 = (float)(counts[1] > 1 ? counts[1] : 1);
  loss[0] = sums[0] / n;
  loss[1] = sums[1] / n;
  loss[2] = sums[2] / n1;
}

__device__ __forceinline__ float sl1_grad(float d) { return d < -1.f ? -1.f : (d > 1.f ? 1.f : d); }

template <int kBox>
__global__ void loss_bwd_kernel(const float* __restrict__ loc, const float* __restrict__ conf,
                                const float* __restrict__ landm, const float* __restrict__ loc_t,
                                const int64_t* __restrict__ conf_t,
                                const float* __restrict__ landm_t,
                                const float4* __restrict__ pri, int64_t A, float v0, float v1,
                                const uint8_t* __restrict__ sel, int64_t total,
                                const float* __restrict__ gout,
                                const int64_t* __restrict__ counts, float* __restrict__ gl,
                                float* __restrict__ gc, float* __restrict__ glm) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float n = (float)(counts[0] > 1 ? counts[0] : 1);
  const float n1 = (float)(counts[1] > 1 ? counts[1] : 1);
  const float sl = gout[0] / n, sc = gout[1] / n, slm = gout[2] / n1;
  const uint8_t s = sel[i];
  const bool pos = s & 1, pos1 = s & 2, ce = s & 4;
  if (gl) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pos) {
      float4 x = reinterpret_cast<const float4*>(loc)[i];
      float4 y = reinterpret_cast<const float4*>(loc_t)[i];
      if constexpr (kBox != kBoxSmoothL1)
        g = iou_grad<kBox>(x, pri[i % A], y, v0, v1, sl);
      else
        g = make_float4(sl1_grad(x.x - y.x) * sl, sl1_grad(x.y - y.y) * sl,
                        sl1_grad(x.z - y.z) * sl, sl1_grad(x.w - y.w) * sl);
    }
    reinterpret_cast<float4*>(gl)[i] = g;
  }
  if (glm) {
#pragma unroll
    for (int k = 0; k < 10; ++k)
      glm[i * 10 + k] = pos1 ? sl1_grad(landm[i * 10 + k] - landm_t[i * 10 + k]) * slm : 0.f;
  }
  if (gc) {
    float g0 = 0.f, g1 = 0.f;
    if (ce) {
      const float c0 = conf[i * 2], c1 = conf[i * 2 + 1];
      const float mx = c0 < c1 ? c1 : c0;
      const float e0 = expf(c0 - mx), e1 = expf(c1 - mx);
      const float z = e0 + e1;
      const float t1 = pos ? 1.f : 0.f;
      g0 = (e0 / z - (1.f - t1)) * sc;
      g1 = (e1 / z - t1) * sc;
    }
    gc[i * 2] = g0;
    gc[i * 2 + 1] = g1;
  }
}

template <typename Al>
static void carve_loss(Al& a, int64_t B, int64_t A, int64_t ngmax) {
  const int64_t nblk = cdiv(A, kLossBlock);
  a.template take<float>(ngmax);       // gmax partials
  a.template take<float>(B * A);       // mining loss
  a.template take<float>(B * nblk);    // part_l
  a.template take<float>(B * nblk);    // part_lm
  a.template take<int>(B);             // npos
  a.template take<int>(B);             // npos1
  a.template take<float>(B);           // ce per image
}

static int64_t gmax_blocks(int64_t total) {
  int64_t g = cdiv(total, kLossBlock * 8);
  return g < 1 ? 1 : (g > 1024 ? 1024 : g);
}

// ---------------------------------------------------------------------------
// letterbox_image + preprocess_input — utils/utils.py:8-19,27-29 as predict.py
// calls them (:122,143-152): a float32 HWC image is cv2.resize'd (INTER_LINEAR,
// float path) to nw x nh, pasted at ((h-nh)//2, (w-nw)//2) on a canvas filled
// with `fill`, then (NCHW mode) the channel means are subtracted and the result
// transposed to [3, h, w].  cv2's float INTER_LINEAR restated (cv2 is absent
// here, parity unpinned against it): per axis f = (float)((d + .5) * scale - .5),
// s = floor(f), f -= s; s < 0 -> (s, f) = (0, 0); s >= n-1 -> (n-1, 0); taps
// combined as S0*(1-f) + S1*f in fp32 (separate products, -ffp-contract=off),
// horizontal pass first.  An exact 2x downscale is cv2's INTER_AREA fast path:
// (S00 + S01 + S10 + S11) * 0.25f.  One thread per canvas pixel, three channels.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void lin_tap(int d, double scale, int n, int& s0, int& s1, float& f) {
  float fx = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(fx);
  fx -= (float)s;
  if (s < 0) { s = 0; fx = 0.f; }
  if (s >= n - 1) { s = n - 1; fx = 0.f; }
  s0 = s;
  s1 = s + 1 < n ? s + 1 : n - 1;
  f = fx;
}

// The geometry of one letterbox: utils/utils.py:10-13 (scale = min(w/iw,
// h/ih); nw = int(iw*scale); nh = int(ih*scale), numpy float64) and cv2.resize's
// inv_scale = dsize/ssize, scale = 1/inv_scale; an exact 2x is INTER_AREA.
// ih, iw, h, w > 0.  Host and device evaluate the same IEEE double expressions.
struct LetterboxGeom {
  int nw, nh, top, left, area2x;
  double sx, sy;
};

__host__ __device__ inline LetterboxGeom letterbox_geom(int ih, int iw, int h, int w) {
  LetterboxGeom g;
  const double sc = fmin((double)w / iw, (double)h / ih);
  g.nw = (int)(iw * sc);
  g.nh = (int)(ih * sc);
  g.top = (h - g.nh) / 2;
  g.left = (w - g.nw) / 2;
  g.sx = 1.0 / ((double)g.nw / iw);  // inf when the side collapses: the callers reject it first
  g.sy = 1.0 / ((double)g.nh / ih);
  g.area2x = (iw == 2 * g.nw && ih == 2 * g.nh) ? 1 : 0;
  return g;
}

__device__ __forceinline__ float letterbox_px(const float* p) { return *p; }
__device__ __forceinline__ float letterbox_px(const uint8_t* p) { return (float)*p; }

// pixel (ry, rx) of the resized nw x nh image, 0 <= ry < nh, 0 <= rx < nw
template <typename T>
__device__ __forceinline__ void letterbox_sample(const T* __restrict__ S, int ih, int iw, int ry,
                                                 int rx, double sx, double sy, int area2x,
                                                 float* v) {
  if (area2x) {
    const T* r0 = S + ((int64_t)(2 * ry) * iw + 2 * rx) * 3;
    const T* r1 = r0 + (int64_t)iw * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      v[c] = (letterbox_px(r0 + c) + letterbox_px(r0 + c + 3) + letterbox_px(r1 + c) +
              letterbox_px(r1 + c + 3)) * 0.25f;
  } else {
    int x0, x1, y0, y1;
    float fx, fy;
    lin_tap(rx, sx, iw, x0, x1, fx);
    lin_tap(ry, sy, ih, y0, y1, fy);
    const float ax0 = 1.f - fx, ay0 = 1.f - fy;
    const T* p00 = S + ((int64_t)y0 * iw + x0) * 3;
    const T* p01 = S + ((int64_t)y0 * iw + x1) * 3;
    const T* p10 = S + ((int64_t)y1 * iw + x0) * 3;
    const T* p11 = S + ((int64_t)y1 * iw + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float h0 = letterbox_px(p00 + c) * ax0 + letterbox_px(p01 + c) * fx;
      const float h1 = letterbox_px(p10 + c) * ax0 + letterbox_px(p11 + c) * fx;
      v[c] = h0 * ay0 + h1 * fy;
    }
  }
}

__global__ __launch_bounds__(256) void letterbox_kernel(
    const float* __restrict__ src, int ih, int iw, float* __restrict__ dst, int h, int w,
    int nw, int nh, int top, int left, double sx, double sy, int area2x, float fill, float m0,
    float m1, float m2, int nchw) {
  const int b = blockIdx.y;
  const int64_t pix = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (pix >= (int64_t)h * w) return;
  const int y = (int)(pix / w), x = (int)(pix - (int64_t)y * w);
  const float* S = src + (int64_t)b * ih * iw * 3;
  float v[3] = {fill, fill, fill};
  const int ry = y - top, rx = x - left;
  if (ry >= 0 && ry < nh && rx >= 0 && rx < nw)
    letterbox_sample(S, ih, iw, ry, rx, sx, sy, area2x, v);
  if (nchw) {
    float* D = dst + (int64_t)b * 3 * h * w + pix;
    const int64_t plane = (int64_t)h * w;
    D[0] = v[0] - m0;
    D[plane] = v[1] - m1;
    D[2 * plane] = v[2] - m2;
  } else {
    float* D = dst + ((int64_t)b * h * w + pix) * 3;
    D[0] = v[0]; D[1] = v[1]; D[2] = v[2];
  }
}

// retinaface_correct_boxes (utils/utils_bbox.py:9-24) then predict.py's
// rescale to image pixels (:195-196) on detection rows [n, 15]: numpy does
// both in float64 and assigns back into the float32 rows, so each step is
// (float)((double)v - off) * sc) and (float)((double)v * dim).
struct CorrectArgs {
  int letterbox;
  double offx, offy, scx, scy, dimx, dimy;
};

// column c (not the score column 4) of a row
__device__ __forceinline__ float correct_value(float v, int c, const CorrectArgs& a) {
  const bool isx = ((c < 4 ? c : c - 5) & 1) == 0;
  if (a.letterbox) v = (float)(((double)v - (isx ? a.offx : a.offy)) * (isx ? a.scx : a.scy));
  return (float)((double)v * (isx ? a.dimx : a.dimy));  // x * 1.0 is exact when !to_pixels
}

__global__ void correct_rows_kernel(float* __restrict__ rows, int64_t n, CorrectArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n * 15) return;
  const int c = (int)(i % 15);
  if (c == 4) return;  // the score column is untouched
  rows[i] = correct_value(rows[i], c, a);
}

// One pass of a multi-scale / flip test-time detection joins the merged rows:
// the pass's first n_keep[0] detect rows (normalised canvas coordinates), if
// `flip` un-mirrored (x -> 1 - x, one fp32 subtraction; the box's x1 and x2
// change places, and so do the landmark pairs 0 <-> 1, the eyes, and 3 <-> 4,
// the mouth corners), corrected as correct_rows_kernel does, land at
// merged[offsets[pass] + i]; rows at or beyond cap are dropped.  One thread per
// (row, column); thread 0 writes offsets[pass + 1], a slot no thread reads.
__global__ void tta_collect_kernel(const float* __restrict__ rows,
                                   const int64_t* __restrict__ n_keep, int64_t n_max,
                                   float* __restrict__ merged, int64_t cap,
                                   int64_t* __restrict__ offsets, int pass, int flip,
                                   CorrectArgs a) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t nk = n_keep[0];
  nk = nk < 0 ? 0 : (nk > n_max ? n_max : nk);
  int64_t base = offsets[pass];
  base = base < 0 ? 0 : (base > cap ? cap : base);
  if (i == 0) offsets[pass + 1] = base + nk < cap ? base + nk : cap;
  const int64_t r = i / 15;
  const int c = (int)(i - r * 15);
  if (r >= nk || base + r >= cap) return;
  const float* src = rows + r * 15;
  float v;
  if (!flip || c == 4) {
    v = src[c];
  } else if (c < 4) {
    v = (c & 1) ? src[c] : 1.f - src[2 - c];
  } else {
    const int k = (c - 5) >> 1;  // landmark k takes its mirror partner's place
    const int ks = k == 0 ? 1 : (k == 1 ? 0 : (k == 3 ? 4 : (k == 4 ? 3 : 2)));
    const float s = src[5 + 2 * ks + ((c - 5) & 1)];
    v = ((c - 5) & 1) ? s : 1.f - s;
  }
  merged[(base + r) * 15 + c] = c == 4 ? v : correct_value(v, c, a);
}

// utils_bbox.py:10-12, numpy float64 over [h, w] pairs
__host__ __device__ static CorrectArgs correct_args(int input_h, int input_w, int image_h,
                                                    int image_w, int letterbox, int to_pixels) {
  CorrectArgs a{letterbox, 0, 0, 1, 1, to_pixels ? (double)image_w : 1.0,
                to_pixels ? (double)image_h : 1.0};
  if (letterbox) {
    const double r = fmin((double)input_h / image_h, (double)input_w / image_w);
    const double nh = image_h * r, nw = image_w * r;
    a.offy = (input_h - nh) / 2. / input_h;
    a.offx = (input_w - nw) / 2. / input_w;
    a.scy = input_h / nh;
    a.scx = input_w / nw;
  }
  return a;
}

// ---------------------------------------------------------------------------
// Batched detection of images of different sizes (predict.detect_images): the
// ragged letterbox in front of the fixed-shape forward and the per-image box
// correction + packing behind it.  Semantics: jabd_letterbox_batch_u8 and
// jabd_batch_collect_f32 in include/jabd.h.  Both read the slot table desc
// [n, 3] = (byte offset into the pool, ih, iw) on the device; blockIdx.y is the
// slot, so a workgroup's image is uniform and its geometry is derived once, in
// double, with the host expressions of jabd_letterbox_f32 / correct_args.
//
// letterbox_batch: letterbox_kernel's arithmetic (letterbox_sample) on uint8
// sources, NCHW output.  One thread per four canvas pixels of a row, three
// 16-byte plane stores (a w that is no multiple of 4: one pixel per thread);
// the four pixels are sampled one by one, so a group may straddle the
// bar / image boundary.  Memory-bound: 12 bytes written per canvas pixel, at
// most 4 taps x 3 source bytes read; the LDS holds the geometry record only.
//
// batch_collect: one launch, one thread per (row, column) of a slot.  Every
// workgroup sums the counts of the slots before its own (integers, every
// workgroup in the same order: the position is a function of the data alone);
// no atomics, no memset, two runs give identical bytes.
// ---------------------------------------------------------------------------
static constexpr int kBatchT = 256;
static constexpr int kBatchWaves = kBatchT / 64;

// Slot i of the table: its (ih, iw) and letterbox to h x w.  False for an empty
// slot: a side <= 0 or beyond int, or a letterbox that collapses (nw or nh 0).
__device__ __forceinline__ bool batch_slot(const int64_t* __restrict__ desc, int64_t i, int h,
                                           int w, int& ih, int& iw, LetterboxGeom& g) {
  const int64_t a = desc[3 * i + 1], b = desc[3 * i + 2];
  if (a <= 0 || b <= 0 || a > 0x7fffffff || b > 0x7fffffff) return false;
  ih = (int)a;
  iw = (int)b;
  g = letterbox_geom(ih, iw, h, w);
  return g.nw > 0 && g.nh > 0;
}

struct BatchSlot {
  const uint8_t* src;
  int ih, iw, empty;
  LetterboxGeom g;
};

// VEC = 4: w % 4 == 0, one thread per 4 pixels; VEC = 1: any w
template <int VEC>
__global__ __launch_bounds__(kBatchT) void letterbox_batch_kernel(
    const uint8_t* __restrict__ pool, int64_t pool_bytes, const int64_t* __restrict__ desc,
    float* __restrict__ dst, int h, int w, float fill, float m0, float m1, float m2) {
  __shared__ BatchSlot slot;
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    BatchSlot s{pool, 0, 0, 1, LetterboxGeom{0, 0, 0, 0, 0, 1.0, 1.0}};
    int ih, iw;
    LetterboxGeom g;
    if (batch_slot(desc, b, h, w, ih, iw, g)) {
      const int64_t off = desc[3 * b];
      // the range guard, 3 * ih * iw <= pool_bytes - off without overflow
      if (off >= 0 && off <= pool_bytes && (int64_t)ih * iw <= (pool_bytes - off) / 3)
        s = BatchSlot{pool + off, ih, iw, 0, g};
    }
    slot = s;
  }
  __syncthreads();
  const int wq = w / VEC;
  const int64_t i = blockIdx.x * (int64_t)kBatchT + threadIdx.x;
  if (i >= (int64_t)h * wq) return;
  const int y = (int)(i / wq);
  const int x = (int)(i - (int64_t)y * wq) * VEC;
  const uint8_t* S = slot.src;
  const int ih = slot.ih, iw = slot.iw;
  const LetterboxGeom g = slot.g;
  const int ry = y - g.top;
  const bool yin = !slot.empty && ry >= 0 && ry < g.nh;  // an empty slot reads nothing
  float v[VEC][3];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    v[k][0] = v[k][1] = v[k][2] = fill;
    const int rx = x + k - g.left;
    if (yin && rx >= 0 && rx < g.nw) letterbox_sample(S, ih, iw, ry, rx, g.sx, g.sy, g.area2x, v[k]);
  }
  const int64_t plane = (int64_t)h * w;
  float* D = dst + (int64_t)b * 3 * plane + (int64_t)y * w + x;
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(D) =
        make_float4(v[0][0] - m0, v[1][0] - m0, v[2][0] - m0, v[3][0] - m0);
    *reinterpret_cast<float4*>(D + plane) =
        make_float4(v[0][1] - m1, v[1][1] - m1, v[2][1] - m1, v[3][1] - m1);
    *reinterpret_cast<float4*>(D + 2 * plane) =
        make_float4(v[0][2] - m2, v[1][2] - m2, v[2][2] - m2, v[3][2] - m2);
  } else {
    D[0] = v[0][0] - m0;
    D[plane] = v[0][1] - m1;
    D[2 * plane] = v[0][2] - m2;
  }
}

// rows slot i contributes: clamp(n_keep[i], 0, A), cut to max_det > 0; 0 when empty
__device__ __forceinline__ int64_t batch_count(const int64_t* __restrict__ n_keep,
                                               const int64_t* __restrict__ desc, int64_t i,
                                               int64_t A, int h, int w, int64_t max_det, int& ih,
                                               int& iw) {
  LetterboxGeom g;
  if (!batch_slot(desc, i, h, w, ih, iw, g)) return 0;
  int64_t c = n_keep[i];
  c = c < 0 ? 0 : (c > A ? A : c);
  return (max_det > 0 && c > max_det) ? max_det : c;
}

__global__ __launch_bounds__(kBatchT) void batch_collect_kernel(
    const float* __restrict__ rows, const int64_t* __restrict__ n_keep, int64_t A,
    const int64_t* __restrict__ desc, int h, int w, int64_t max_det, float* __restrict__ out,
    int64_t cap, int64_t* __restrict__ offsets) {
  __shared__ long long wave_sum[kBatchWaves];
  __shared__ CorrectArgs args;
  const int t = blockIdx.y, tid = threadIdx.x;
  int ih = 1, iw = 1, qh, qw;
  const int64_t cnt = batch_count(n_keep, desc, t, A, h, w, max_det, ih, iw);
  // a slot's first workgroup stays: it writes offsets[t + 1]
  if (blockIdx.x > 0 && blockIdx.x * (int64_t)kBatchT >= cnt * 15) return;  // uniform
  long long s = 0;  // rows of the slots before this one
  for (int q = tid; q < t; q += kBatchT) s += batch_count(n_keep, desc, q, A, h, w, max_det, qh, qw);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
  if (tid == 0) args = correct_args(h, w, ih, iw, 1, 1);  // read only when cnt > 0
  __syncthreads();
  long long before = 0;
#pragma unroll
  for (int q = 0; q < kBatchWaves; ++q) before += wave_sum[q];
  if (blockIdx.x == 0 && tid == 0) {  // slots no thread reads
    if (t == 0) offsets[0] = 0;
    const int64_t end = before + cnt;
    offsets[t + 1] = end < cap ? end : cap;
  }
  const int64_t i = blockIdx.x * (int64_t)kBatchT + tid;
  const int64_t r = i / 15;
  const int c = (int)(i - r * 15);
  if (r >= cnt) return;
  const int64_t d = before + r;
  if (d >= cap) return;
  const float v = rows[((int64_t)t * A + r) * 15 + c];
  const CorrectArgs a = args;
  out[d * 15 + c] = c == 4 ? v : correct_value(v, c, a);
}

// no slots: offsets[0] is all there is to write
__global__ void batch_collect_empty_kernel(int64_t* __restrict__ offsets) {
  if (blockIdx.x == 0 && threadIdx.x == 0) offsets[0] = 0;
}

}  // namespace jabd

using namespace jabd;

extern "C" int jabd_correct_boxes_f32(float* rows, int64_t n, int input_h, int input_w,
                                      int image_h, int image_w, int letterbox,
                                      int to_pixels, jabd_stream_t stream) {
  JABD_REQUIRE(n >= 0 && image_h > 0 && image_w > 0, "correct_boxes: bad size");
  JABD_REQUIRE(!letterbox || (input_h > 0 && input_w > 0), "correct_boxes: bad input shape");
  if (n == 0) return JABD_OK;
  JABD_REQUIRE(rows, "correct_boxes: null pointer");
  correct_rows_kernel<<<(unsigned)cdiv(n * 15, 256), 256, 0, as_stream(stream)>>>(
      rows, n, correct_args(input_h, input_w, image_h, image_w, letterbox, to_pixels));
  return check_launch("correct_boxes");
}

extern "C" int jabd_tta_collect_f32(const float* rows, const int64_t* n_keep, int64_t n_max,
                                    float* merged, int64_t cap, int64_t* offsets, int32_t pass,
                                    int input_h, int input_w, int image_h, int image_w,
                                    int letterbox, int flip, jabd_stream_t stream) {
  JABD_REQUIRE(n_max >= 0 && cap >= 0 && pass >= 0, "tta_collect: bad size");
  JABD_REQUIRE(image_h > 0 && image_w > 0, "tta_collect: bad image shape");
  JABD_REQUIRE(!letterbox || (input_h > 0 && input_w > 0), "tta_collect: bad input shape");
  JABD_REQUIRE(n_max < (int64_t(1) << 31), "tta_collect: n_max=%lld too large",
               (long long)n_max);
  JABD_REQUIRE(n_keep && offsets, "tta_collect: null pointer");
  JABD_REQUIRE((rows || n_max == 0) && (merged || cap == 0), "tta_collect: null pointer");
  const int64_t blocks = cdiv(n_max * 15, 256);
  tta_collect_kernel<<<(unsigned)(blocks < 1 ? 1 : blocks), 256, 0, as_stream(stream)>>>(
      rows, n_keep, n_max, merged, cap, offsets, (int)pass, flip ? 1 : 0,
      correct_args(input_h, input_w, image_h, image_w, letterbox, 1));
  return check_launch("tta_collect");
}

extern "C" int jabd_letterbox_f32(const float* src, int64_t batch, int ih, int iw, float* dst,
                                  int h, int w, float fill, const float* mean3, int nchw,
                                  jabd_stream_t stream) {
  JABD_REQUIRE(batch >= 0 && ih > 0 && iw > 0 && h > 0 && w > 0, "letterbox: bad size");
  JABD_REQUIRE(!nchw || mean3, "letterbox: NCHW output needs the channel means");
  if (batch == 0) return JABD_OK;
  JABD_REQUIRE(src && dst, "letterbox: null pointer");
  const LetterboxGeom lg = letterbox_geom(ih, iw, h, w);
  JABD_REQUIRE(lg.nw > 0 && lg.nh > 0, "letterbox: image %dx%d collapses to %dx%d", iw, ih,
               lg.nw, lg.nh);
  const float m[3] = {nchw ? mean3[0] : 0.f, nchw ? mean3[1] : 0.f, nchw ? mean3[2] : 0.f};
  const int64_t npix = (int64_t)h * w;
  dim3 g((unsigned)cdiv(npix, 256), (unsigned)batch);
  letterbox_kernel<<<g, 256, 0, as_stream(stream)>>>(src, ih, iw, dst, h, w, lg.nw, lg.nh, lg.top,
                                                      lg.left, lg.sx, lg.sy, lg.area2x, fill,
                                                      m[0], m[1], m[2], nchw);
  return check_launch("letterbox");
}

extern "C" int jabd_letterbox_batch_u8(const uint8_t* pool, int64_t pool_bytes,
                                       const int64_t* desc, int64_t n, float* dst, int h, int w,
                                       float fill, const float* mean3, jabd_stream_t stream) {
  JABD_REQUIRE(n >= 0 && pool_bytes >= 0 && h > 0 && w > 0, "letterbox_batch: bad size");
  JABD_REQUIRE(mean3, "letterbox_batch: null channel means");
  if (n == 0) return JABD_OK;
  JABD_REQUIRE(n <= 65535, "letterbox_batch: n=%lld exceeds 65535 per call", (long long)n);
  JABD_REQUIRE(desc && dst && (pool || pool_bytes == 0), "letterbox_batch: null pointer");
  JABD_REQUIRE(((uintptr_t)dst & 15u) == 0, "letterbox_batch: dst must be 16-byte aligned");
  const bool vec = w % 4 == 0;
  const int64_t blocks = cdiv((int64_t)h * (vec ? w / 4 : w), kBatchT);
  JABD_REQUIRE(blocks <= 0x7fffffff, "letterbox_batch: canvas %dx%d too large", w, h);
  const dim3 g((unsigned)blocks, (unsigned)n);
  hipStream_t st = as_stream(stream);
  if (vec) {
    letterbox_batch_kernel<4><<<g, kBatchT, 0, st>>>(pool, pool_bytes, desc, dst, h, w, fill,
                                                     mean3[0], mean3[1], mean3[2]);
    return check_launch("letterbox_batch", 4);
  }
  letterbox_batch_kernel<1><<<g, kBatchT, 0, st>>>(pool, pool_bytes, desc, dst, h, w, fill,
                                                   mean3[0], mean3[1], mean3[2]);
  return check_launch("letterbox_batch", 1);
}

extern "C" int jabd_batch_collect_f32(const float* rows, const int64_t* n_keep, int64_t n,
                                      int64_t A, const int64_t* desc, int input_h, int input_w,
                                      int64_t max_det, float* out, int64_t cap,
                                      int64_t* offsets, jabd_stream_t stream) {
  JABD_REQUIRE(n >= 0 && A >= 0 && cap >= 0, "batch_collect: bad size");
  JABD_REQUIRE(input_h > 0 && input_w > 0, "batch_collect: bad input shape");
  JABD_REQUIRE(n <= 4096, "batch_collect: n=%lld exceeds 4096 per call", (long long)n);
  JABD_REQUIRE(A * 15 < (int64_t(1) << 31), "batch_collect: A=%lld too large", (long long)A);
  JABD_REQUIRE(offsets, "batch_collect: null offsets");
  JABD_REQUIRE(n == 0 || (n_keep && desc && (rows || A == 0)), "batch_collect: null pointer");
  JABD_REQUIRE(out || cap == 0, "batch_collect: null out");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    batch_collect_empty_kernel<<<1, 64, 0, st>>>(offsets);
    return check_launch("batch_collect_empty");
  }
  const int64_t bx = cdiv(A * 15, kBatchT);
  batch_collect_kernel<<<dim3((unsigned)(bx < 1 ? 1 : bx), (unsigned)n), kBatchT, 0, st>>>(
      rows, n_keep, A, desc, input_h, input_w, max_det, out, cap, offsets);
  return check_launch("batch_collect");
}

extern "C" int jabd_decode_f32(const float* loc, const float* priors, int64_t batch,
                               int64_t num_priors, float var0, float var1, float* boxes,
                               jabd_stream_t stream) {
  JABD_REQUIRE(batch >= 0 && num_priors >= 0, "decode: negative size");
  const int64_t total = batch * num_priors;
  if (total == 0) return JABD_OK;
  JABD_REQUIRE(loc && priors && boxes, "decode: null pointer");
  decode_kernel<<<(unsigned)cdiv(total, 256), 256, 0, as_stream(stream)>>>(
      loc, reinterpret_cast<const float4*>(priors), num_priors, total, var0, var1, boxes);
  return check_launch("decode");
}

extern "C" int jabd_decode_landm_f32(const float* pre, const float* priors, int64_t batch,
                                     int64_t num_priors, float var0, float* landms,
                                     jabd_stream_t stream) {
  JABD_REQUIRE(batch >= 0 && num_priors >= 0, "decode_landm: negative size");
  const int64_t total = batch * num_priors;
  if (total == 0) return JABD_OK;
  JABD_REQUIRE(pre && priors && landms, "decode_landm: null pointer");
  decode_landm_kernel<<<(unsigned)cdiv(total, 256), 256, 0, as_stream(stream)>>>(
      pre, reinterpret_cast<const float4*>(priors), num_priors, total, var0, landms);
  return check_launch("decode_landm");
}

static size_t detect_ws(int64_t B, int64_t A) {
  Sizer s;
  s.take<float>(B * A * 15);
  s.take<int64_t>(B * A);
  s.take<char>(nms_ws_bytes(B, A));
  return s.used;
}

extern "C" int jabd_detect_workspace_size(int64_t batch, int64_t num_priors, size_t* bytes) {
  JABD_REQUIRE(bytes && batch >= 0 && num_priors >= 0, "detect_workspace_size: bad args");
  *bytes = detect_ws(batch, num_priors);
  return JABD_OK;
}

extern "C" int jabd_detect_ex_f32(const float* loc, const float* conf, const float* landm,
                                  const float* priors, int64_t batch, int64_t num_priors,
                                  float var0, float var1, float conf_threshold,
                                  double nms_threshold, float* out, int64_t* n_keep, void* ws,
                                  size_t ws_bytes, jabd_stream_t stream, int32_t kind,
                                  double beta1, int64_t top_k) {
  JABD_REQUIRE(batch >= 0 && num_priors >= 0, "detect: negative size");
  if (batch == 0) return JABD_OK;
  hipStream_t st = as_stream(stream);
  if (num_priors == 0) {
    const FillRange fr{n_keep, (int64_t)sizeof(int64_t) * batch, 0u};
    if (int e = fill_ranges(&fr, 1, st)) return e;
    return JABD_OK;
  }
  JABD_REQUIRE(loc && conf && landm && priors && out && n_keep, "detect: null pointer");
  JABD_REQUIRE(ws_bytes >= detect_ws(batch, num_priors), "detect: workspace too small");
  Carve cv(ws, ws_bytes);
  float* rows = cv.take<float>(batch * num_priors * 15);
  int64_t* keep = cv.take<int64_t>(batch * num_priors);
  size_t nws = nms_ws_bytes(batch, num_priors);
  void* nmsws = cv.take<char>(nws);
  const int64_t total = batch * num_priors;
  detect_rows_kernel<<<(unsigned)cdiv(total, 256), 256, 0, st>>>(
      loc, conf, landm, reinterpret_cast<const float4*>(priors), num_priors, total, var0, var1,
      rows);
  if (int e = check_launch("detect_rows")) return e;
  if (int e = nms_core(rows, 15, num_priors * 15, rows + 4, 15, num_priors * 15, nullptr, batch,
                       num_priors, nms_threshold, conf_threshold, keep, n_keep, nmsws, nws, st,
                       kind, beta1, top_k))
    return e;
  dim3 g((unsigned)cdiv(num_priors, 256), (unsigned)batch);
  gather_rows_kernel<<<g, 256, 0, st>>>(rows, keep, n_keep, num_priors, out);
  return check_launch("detect_gather");
}

extern "C" int jabd_detect_f32(const float* loc, const float* conf, const float* landm,
                               const float* priors, int64_t batch, int64_t num_priors,
                               float var0, float var1, float conf_threshold,
                               double nms_threshold, float* out, int64_t* n_keep, void* ws,
                               size_t ws_bytes, jabd_stream_t stream) {
  return jabd_detect_ex_f32(loc, conf, landm, priors, batch, num_priors, var0, var1,
                            conf_threshold, nms_threshold, out, n_keep, ws, ws_bytes, stream,
                            kNmsIoU, 1.0, 0);
}

// gather_rows_kernel with column 4 taken from the Soft-NMS's decayed scores
__global__ void gather_rows_soft_kernel(const float* __restrict__ rows,
                                        const int64_t* __restrict__ keep,
                                        const float* __restrict__ keep_scores,
                                        const int64_t* __restrict__ n_keep, int64_t A,
                                        float* __restrict__ out) {
  int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int b = blockIdx.y;
  if (k >= n_keep[b]) return;
  int64_t src = keep[(int64_t)b * A + k];
  const float* r = rows + ((int64_t)b * A + src) * 15;
  float* o = out + ((int64_t)b * A + k) * 15;
#pragma unroll
  for (int c = 0; c < 15; ++c) o[c] = r[c];
  o[4] = keep_scores[(int64_t)b * A + k];
}

static size_t detect_soft_ws(int64_t B, int64_t A) {
  Sizer s;
  s.take<float>(B * A * 15);
  s.take<int64_t>(B * A);
  s.take<float>(B * A);
  s.take<char>(soft_nms_ws_bytes(B, A));
  return s.used;
}

extern "C" int jabd_detect_soft_workspace_size(int64_t batch, int64_t num_priors,
                                               size_t* bytes) {
  JABD_REQUIRE(bytes && batch >= 0 && num_priors >= 0, "detect_soft_workspace_size: bad args");
  *bytes = detect_soft_ws(batch, num_priors);
  return JABD_OK;
}

extern "C" int jabd_detect_soft_f32(const float* loc, const float* conf, const float* landm,
                                    const float* priors, int64_t batch, int64_t num_priors,
                                    float var0, float var1, float conf_threshold, double sigma,
                                    float offset, double prune, int64_t top_k, float* out,
                                    int64_t* n_keep, void* ws, size_t ws_bytes,
                                    jabd_stream_t stream) {
  JABD_REQUIRE(batch >= 0 && num_priors >= 0, "detect_soft: negative size");
  hipStream_t st = as_stream(stream);
  if (batch == 0 || num_priors == 0)  // the argument checks; n_keep = 0
    return soft_nms_core(nullptr, 15, 0, nullptr, 15, 0, nullptr, batch, 0, sigma, offset, prune,
                         conf_threshold, top_k, nullptr, nullptr, n_keep, nullptr, 0, st);
  JABD_REQUIRE(loc && conf && landm && priors && out && n_keep, "detect_soft: null pointer");
  JABD_REQUIRE(ws_bytes >= detect_soft_ws(batch, num_priors), "detect_soft: workspace too small");
  Carve cv(ws, ws_bytes);
  float* rows = cv.take<float>(batch * num_priors * 15);
  int64_t* keep = cv.take<int64_t>(batch * num_priors);
  float* keep_scores = cv.take<float>(batch * num_priors);
  size_t nws = soft_nms_ws_bytes(batch, num_priors);
  void* nmsws = cv.take<char>(nws);
  const int64_t total = batch * num_priors;
  // the Soft-NMS checks sigma / offset / prune; nothing may launch before it does
  JABD_REQUIRE(sigma > 0.0 && std::isfinite(sigma) && std::isfinite(offset) &&
                   std::isfinite(prune),
               "detect_soft: sigma must be positive and finite, offset and prune finite "
               "(got %g, %g, %g)", sigma, (double)offset, prune);
  detect_rows_kernel<<<(unsigned)cdiv(total, 256), 256, 0, st>>>(
      loc, conf, landm, reinterpret_cast<const float4*>(priors), num_priors, total, var0, var1,
      rows);
  if (int e = check_launch("detect_rows")) return e;
  if (int e = soft_nms_core(rows, 15, num_priors * 15, rows + 4, 15, num_priors * 15, nullptr,
                            batch, num_priors, sigma, offset, prune, conf_threshold, top_k, keep,
                            keep_scores, n_keep, nmsws, nws, st))
    return e;
  dim3 g((unsigned)cdiv(num_priors, 256), (unsigned)batch);
  gather_rows_soft_kernel<<<g, 256, 0, st>>>(rows, keep, keep_scores, n_keep, num_priors, out);
  return check_launch("detect_soft_gather");
}

static size_t match_ws(int64_t B, int64_t A) {
  Sizer s;
  s.take<int>(B * A);
  return s.used;
}

extern "C" int jabd_match_workspace_size(int64_t batch, int64_t num_priors, size_t* bytes) {
  JABD_REQUIRE(bytes && batch >= 0 && num_priors >= 0, "match_workspace_size: bad args");
  *bytes = match_ws(batch, num_priors);
  return JABD_OK;
}

static int match_impl(bool raw, const float* targets, const int64_t* offsets, int64_t batch,
                      int64_t max_gt, const float* priors, int64_t num_priors, float threshold,
                      float var0, float var1, float* loc_t, int64_t* conf_t, float* landm_t,
                      void* ws, size_t ws_bytes, jabd_stream_t stream) {
  JABD_REQUIRE(batch >= 0 && num_priors >= 0 && max_gt >= 0, "match: negative size");
  if (batch == 0 || num_priors == 0) return JABD_OK;
  JABD_REQUIRE(max_gt > 0, "match: an image has no targets (reference match() fails too)");
  JABD_REQUIRE(max_gt <= 3276, "match: max_gt=%lld > 3276 targets in one image", (long long)max_gt);
  JABD_REQUIRE(num_priors < 0x7fffffff, "match: too many priors");
  JABD_REQUIRE(targets && offsets && priors && loc_t && conf_t && landm_t, "match: null pointer");
  JABD_REQUIRE(ws_bytes >= match_ws(batch, num_priors), "match: workspace too small");
  hipStream_t st = as_stream(stream);
  Carve cv(ws, ws_bytes);
  int* forced = cv.take<int>(batch * num_priors);
  {
    const FillRange fr{forced, (int64_t)sizeof(int) * batch * num_priors, 0xFFFFFFFFu};  // -1
    if (int e = fill_ranges(&fr, 1, st)) return e;
  }
  const float4* pri = reinterpret_cast<const float4*>(priors);
  dim3 g1((unsigned)max_gt, (unsigned)batch);
  match_best_prior_kernel<<<g1, 256, 0, st>>>(targets, offsets, pri, num_priors, forced);
  if (int e = check_launch("match_best_prior")) return e;
  dim3 g2((unsigned)cdiv(num_priors, 256), (unsigned)batch);
  if (raw)
    match_assign_kernel<true><<<g2, 256, max_gt * 5 * sizeof(float), st>>>(
        targets, offsets, pri, num_priors, forced, threshold, var0, var1, loc_t, conf_t, landm_t);
  else
    match_assign_kernel<false><<<g2, 256, max_gt * 5 * sizeof(float), st>>>(
        targets, offsets, pri, num_priors, forced, threshold, var0, var1, loc_t, conf_t, landm_t);
  return check_launch("match_assign");
}

extern "C" int jabd_match_encode_f32(const float* targets, const int64_t* offsets,
                                     int64_t batch, int64_t max_gt, const float* priors,
                                     int64_t num_priors, float threshold, float var0,
                                     float var1, float* loc_t, int64_t* conf_t,
                                     float* landm_t, void* ws, size_t ws_bytes,
                                     jabd_stream_t stream) {
  return match_impl(false, targets, offsets, batch, max_gt, priors, num_priors, threshold, var0,
                    var1, loc_t, conf_t, landm_t, ws, ws_bytes, stream);
}

extern "C" int jabd_match_iou_f32(const float* targets, const int64_t* offsets, int64_t batch,
                                  int64_t max_gt, const float* priors, int64_t num_priors,
                                  float threshold, float var0, float var1, float* loc_t,
                                  int64_t* conf_t, float* landm_t, void* ws, size_t ws_bytes,
                                  jabd_stream_t stream) {
  return match_impl(true, targets, offsets, batch, max_gt, priors, num_priors, threshold, var0,
                    var1, loc_t, conf_t, landm_t, ws, ws_bytes, stream);
}

extern "C" int jabd_multibox_workspace_size(int64_t batch, int64_t num_priors, size_t* bytes) {
  JABD_REQUIRE(bytes && batch >= 0 && num_priors >= 0, "multibox_workspace_size: bad args");
  Sizer s;
  carve_loss(s, batch, num_priors, gmax_blocks(batch * num_priors * 2));
  *bytes = s.used;
  return JABD_OK;
}

// kind: kBoxSmoothL1 (priors unused) or one of the four IoU-family kinds.
static int loss_fwd_impl(int kind, const float* loc, const float* conf, const float* landm,
                         const float* loc_t, const int64_t* conf_t, const float* landm_t,
                         const float* priors, float v0, float v1, int64_t batch,
                         int64_t num_priors, int neg_pos, float* sums, int64_t* counts,
                         uint8_t* sel, void* ws, size_t ws_bytes, jabd_stream_t stream) {
  JABD_REQUIRE(batch > 0 && num_priors > 0, "multibox: empty batch");
  JABD_REQUIRE(num_priors < 0x7fffffff, "multibox: too many priors");
  JABD_REQUIRE(loc && conf && landm && loc_t && conf_t && landm_t && sums && counts && sel,
               "multibox: null pointer");
  hipStream_t st = as_stream(stream);
  const int64_t B = batch, A = num_priors;
  const int64_t ng = gmax_blocks(B * A * 2);
  Sizer sz;
  carve_loss(sz, B, A, ng);
  JABD_REQUIRE(ws_bytes >= sz.used, "multibox: workspace %zu < %zu", ws_bytes, sz.used);
  Carve cv(ws, ws_bytes);
  const int64_t nblk = cdiv(A, kLossBlock);
  float* gpart = cv.take<float>(ng);
  float* mining = cv.take<float>(B * A);
  float* part_l = cv.take<float>(B * nblk);
  float* part_lm = cv.take<float>(B * nblk);
  int* npos = cv.take<int>(B);
  int* npos1 = cv.take<int>(B);
  float* ce = cv.take<float>(B);
  {
    const FillRange fr[2] = {{npos, (int64_t)sizeof(int) * B, 0u},
                             {npos1, (int64_t)sizeof(int) * B, 0u}};
    if (int e = fill_ranges(fr, 2, st)) return e;
  }
  conf_max_partial<<<(unsigned)ng, kLossBlock, 0, st>>>(conf, B * A * 2, gpart);
  if (int e = check_launch("conf_max")) return e;
  dim3 g((unsigned)nblk, (unsigned)B);
  const float4* pri = reinterpret_cast<const float4*>(priors);
#define JABD_LOSS_ELEM(K)                                                                    \
  loss_elem_kernel<K><<<g, kLossBlock, 0, st>>>(loc, conf, landm, loc_t, conf_t, landm_t, A, \
                                                pri, v0, v1, gpart, (int)ng, mining, sel,    \
                                                part_l, part_lm, npos, npos1)
  switch (kind) {
    case kBoxIou: JABD_LOSS_ELEM(kBoxIou); break;
    case kBoxGiou: JABD_LOSS_ELEM(kBoxGiou); break;
    case kBoxDiou: JABD_LOSS_ELEM(kBoxDiou); break;
    case kBoxCiou: JABD_LOSS_ELEM(kBoxCiou); break;
    default: JABD_LOSS_ELEM(kBoxSmoothL1); break;
  }
#undef JABD_LOSS_ELEM
  if (int e = check_launch("loss_elem")) return e;
  ohem_select_kernel<<<(unsigned)B, kSelBlock, 0, st>>>(mining, conf, A, neg_pos, npos, sel, ce);
  if (int e = check_launch("ohem_select")) return e;
  loss_final_kernel<<<1, 64, 0, st>>>(part_l, part_lm, B * nblk, ce, npos, npos1, (int)B, sums,
                                      counts);
  return check_launch("loss_final");
}

extern "C" int jabd_multibox_loss_fwd_f32(const float* loc, const float* conf,
                                          const float* landm, const float* loc_t,
                                          const int64_t* conf_t, const float* landm_t,
                                          int64_t batch, int64_t num_priors, int neg_pos,
                                          float* sums, int64_t* counts, uint8_t* sel, void* ws,
                                          size_t ws_bytes, jabd_stream_t stream) {
  return loss_fwd_impl(kBoxSmoothL1, loc, conf, landm, loc_t, conf_t, landm_t, nullptr, 0.f, 0.f,
                       batch, num_priors, neg_pos, sums, counts, sel, ws, ws_bytes, stream);
}

extern "C" int jabd_multibox_iou_loss_fwd_f32(const float* loc, const float* conf,
                                              const float* landm, const float* loc_t,
                                              const int64_t* conf_t, const float* landm_t,
                                              const float* priors, float var0, float var1,
                                              int64_t batch, int64_t num_priors, int neg_pos,
                                              float* sums, int64_t* counts, uint8_t* sel,
                                              void* ws, size_t ws_bytes, int32_t kind,
                                              jabd_stream_t stream) {
  JABD_REQUIRE(kind >= kBoxIou && kind <= kBoxCiou,
               "multibox_iou: kind %d (0 Iou, 1 Giou, 2 Diou, 3 Ciou)", kind);
  JABD_REQUIRE(priors, "multibox_iou: null priors");
  return loss_fwd_impl(kind, loc, conf, landm, loc_t, conf_t, landm_t, priors, var0, var1, batch,
                       num_priors, neg_pos, sums, counts, sel, ws, ws_bytes, stream);
}

extern "C" int jabd_multibox_diou_loss_fwd_f32(const float* loc, const float* conf,
                                               const float* landm, const float* loc_t,
                                               const int64_t* conf_t, const float* landm_t,
                                               const float* priors, float var0, float var1,
                                               int64_t batch, int64_t num_priors, int neg_pos,
                                               float* sums, int64_t* counts, uint8_t* sel,
                                               void* ws, size_t ws_bytes,
                                               jabd_stream_t stream) {
  return jabd_multibox_iou_loss_fwd_f32(loc, conf, landm, loc_t, conf_t, landm_t, priors, var0,
                                        var1, batch, num_priors, neg_pos, sums, counts, sel, ws,
                                        ws_bytes, kBoxDiou, stream);
}

extern "C" int jabd_multibox_loss_finalize_f32(const float* sums, const int64_t* counts,
                                               float* loss, jabd_stream_t stream) {
  JABD_REQUIRE(sums && counts && loss, "multibox_finalize: null pointer");
  loss_normalize_kernel<<<1, 64, 0, as_stream(stream)>>>(sums, counts, loss);
  return check_launch("loss_finalize");
}

extern "C" int jabd_multibox_loss_bwd_f32(const float* loc, const float* conf,
                                          const float* landm, const float* loc_t,
                                          const int64_t* conf_t, const float* landm_t,
                                          const uint8_t* sel, int64_t batch,
                                          int64_t num_priors, const float* gout,
                                          const int64_t* counts, float* grad_loc,
                                          float* grad_conf, float* grad_landm,
                                          jabd_stream_t stream) {
  const int64_t total = batch * num_priors;
  if (total <= 0) return JABD_OK;
  JABD_REQUIRE(sel && gout && counts, "multibox_bwd: null pointer");
  loss_bwd_kernel<kBoxSmoothL1><<<(unsigned)cdiv(total, 256), 256, 0, as_stream(stream)>>>(
      loc, conf, landm, loc_t, conf_t, landm_t, nullptr, num_priors, 0.f, 0.f, sel, total, gout,
      counts, grad_loc, grad_conf, grad_landm);
  return check_launch("multibox_bwd");
}

extern "C" int jabd_multibox_iou_loss_bwd_f32(const float* loc, const float* conf,
                                              const float* landm, const float* loc_t,
                                              const int64_t* conf_t, const float* landm_t,
                                              const float* priors, float var0, float var1,
                                              const uint8_t* sel, int64_t batch,
                                              int64_t num_priors, const float* gout,
                                              const int64_t* counts, float* grad_loc,
                                              float* grad_conf, float* grad_landm, int32_t kind,
                                              jabd_stream_t stream) {
  JABD_REQUIRE(kind >= kBoxIou && kind <= kBoxCiou,
               "multibox_iou_bwd: kind %d (0 Iou, 1 Giou, 2 Diou, 3 Ciou)", kind);
  const int64_t total = batch * num_priors;
  if (total <= 0) return JABD_OK;
  JABD_REQUIRE(sel && gout && counts && priors, "multibox_iou_bwd: null pointer");
  const float4* pri = reinterpret_cast<const float4*>(priors);
  const unsigned grid = (unsigned)cdiv(total, 256);
  hipStream_t st = as_stream(stream);
#define JABD_LOSS_BWD(K)                                                                      \
  loss_bwd_kernel<K><<<grid, 256, 0, st>>>(loc, conf, landm, loc_t, conf_t, landm_t, pri,     \
                                           num_priors, var0, var1, sel, total, gout, counts, \
                                           grad_loc, grad_conf, grad_landm)
  switch (kind) {
    case kBoxIou: JABD_LOSS_BWD(kBoxIou); break;
    case kBoxGiou: JABD_LOSS_BWD(kBoxGiou); break;
    case kBoxDiou: JABD_LOSS_BWD(kBoxDiou); break;
    default: JABD_LOSS_BWD(kBoxCiou); break;
  }
#undef JABD_LOSS_BWD
  return check_launch("multibox_iou_bwd", kind);
}

extern "C" int jabd_multibox_diou_loss_bwd_f32(const float* loc, const float* conf,
                                               const float* landm, const float* loc_t,
                                               const int64_t* conf_t, const float* landm_t,
                                               const float* priors, float var0, float var1,
                                               const uint8_t* sel, int64_t batch,
                                               int64_t num_priors, const float* gout,
                                               const int64_t* counts, float* grad_loc,
                                               float* grad_conf, float* grad_landm,
                                               jabd_stream_t stream) {
  return jabd_multibox_iou_loss_bwd_f32(loc, conf, landm, loc_t, conf_t, landm_t, priors, var0,
                                        var1, sel, batch, num_priors, gout, counts, grad_loc,
                                        grad_conf, grad_landm, kBoxDiou, stream);
}

// The stand-alone paired overlaps (IouLoss, bbox_overlaps_*): val[i] = the
// clamped kind-overlap of row i; the backward maps dL/dval to dL/dpred.
extern "C" int jabd_iou_rows_fwd_f32(const float* pred, const float* priors, const float* truth,
                                     int64_t n, float var0, float var1, int32_t kind, float* val,
                                     jabd_stream_t stream) {
  JABD_REQUIRE(kind >= kBoxIou && kind <= kBoxCiou,
               "iou_rows: kind %d (0 Iou, 1 Giou, 2 Diou, 3 Ciou)", kind);
  JABD_REQUIRE(n >= 0, "iou_rows: n = %lld", (long long)n);
  if (n == 0) return JABD_OK;
  JABD_REQUIRE(pred && truth && val, "iou_rows: null pointer");
  const float4* p4 = reinterpret_cast<const float4*>(pred);
  const float4* pri = reinterpret_cast<const float4*>(priors);
  const float4* t4 = reinterpret_cast<const float4*>(truth);
  const unsigned grid = (unsigned)cdiv(n, 256);
  hipStream_t st = as_stream(stream);
#define JABD_ROWS_FWD(K) \
  iou_rows_fwd_kernel<K><<<grid, 256, 0, st>>>(p4, pri, t4, n, var0, var1, val)
  switch (kind) {
    case kBoxIou: JABD_ROWS_FWD(kBoxIou); break;
    case kBoxGiou: JABD_ROWS_FWD(kBoxGiou); break;
    case kBoxDiou: JABD_ROWS_FWD(kBoxDiou); break;
    default: JABD_ROWS_FWD(kBoxCiou); break;
  }
#undef JABD_ROWS_FWD
  return check_launch("iou_rows_fwd", kind);
}

extern "C" int jabd_iou_rows_bwd_f32(const float* pred, const float* priors, const float* truth,
                                     int64_t n, float var0, float var1, int32_t kind,
                                     const float* gval, float* gpred, jabd_stream_t stream) {
  JABD_REQUIRE(kind >= kBoxIou && kind <= kBoxCiou,
               "iou_rows_bwd: kind %d (0 Iou, 1 Giou, 2 Diou, 3 Ciou)", kind);
  JABD_REQUIRE(n >= 0, "iou_rows_bwd: n = %lld", (long long)n);
  if (n == 0) return JABD_OK;
  JABD_REQUIRE(pred && truth && gval && gpred, "iou_rows_bwd: null pointer");
  const float4* p4 = reinterpret_cast<const float4*>(pred);
  const float4* pri = reinterpret_cast<const float4*>(priors);
  const float4* t4 = reinterpret_cast<const float4*>(truth);
  float4* g4 = reinterpret_cast<float4*>(gpred);
  const unsigned grid = (unsigned)cdiv(n, 256);
  hipStream_t st = as_stream(stream);
#define JABD_ROWS_BWD(K) \
  iou_rows_bwd_kernel<K><<<grid, 256, 0, st>>>(p4, pri, t4, n, var0, var1, gval, g4)
  switch (kind) {
    case kBoxIou: JABD_ROWS_BWD(kBoxIou); break;
    case kBoxGiou: JABD_ROWS_BWD(kBoxGiou); break;
    case kBoxDiou: JABD_ROWS_BWD(kBoxDiou); break;
    default: JABD_ROWS_BWD(kBoxCiou); break;
  }
#undef JABD_ROWS_BWD
  return check_launch("iou_rows_bwd", kind);
}

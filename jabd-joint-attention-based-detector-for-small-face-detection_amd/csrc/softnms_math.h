/* Arithmetic of the Gaussian Soft-NMS (soft_nms.hip), in plain C so that the
 * kernel and the test-side C twin (tests/_softnms_ref.c) compile the very same
 * text: the "+offset" IoU in fp32, the score decay in double, the exp it
 * uses, and the total order of scores that the selection and the top_k cut
 * share.
 *
 * Every operation here is one IEEE add, multiply, divide, compare or
 * conversion; there is no library call and no fused multiply-add, so host and
 * device produce the same bits.  Compile with -ffp-contract=off (the EXACT
 * flags of the Makefile; the twin's build line): a contracted a*b+c would
 * round once where this text rounds twice.
 */
#ifndef JABD_SOFTNMS_MATH_H
#define JABD_SOFTNMS_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define JABD_SN_FN static __host__ __device__ __inline__
#else
#define JABD_SN_FN static inline
#endif

JABD_SN_FN double jabd_sn_from_bits(uint64_t u) {
  double d;
  __builtin_memcpy(&d, &u, sizeof(d));
  return d;
}

JABD_SN_FN uint32_t jabd_sn_float_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, sizeof(u));
  return u;
}

/* exp(x) for x <= 0 (NaN -> NaN; x > 0 is not used and not supported).
 * Argument reduction x = k ln2 + r, |r| <= ln2 / 2, with ln2 split in two so
 * that k * ln2_hi is exact; exp(r) = 1 + 2r / (R(r^2) - r) with the degree-5
 * Remez polynomial R of the classic freely distributable libm (fdlibm
 * e_exp.c), whose error bound is below one ulp; the scaling by 2^k is an exact
 * multiplication (two of them where the result is subnormal, the second one
 * the only rounding).  Results below the smallest subnormal are 0. */
JABD_SN_FN double jabd_sn_exp_nonpos(double x) {
  const double ln2_hi = 6.93147180369123816490e-01;  /* 0x3fe62e42fee00000 */
  const double ln2_lo = 1.90821492927058770002e-10;  /* 0x3dea39ef35793c76 */
  const double inv_ln2 = 1.44269504088896338700e+00;
  const double p1 = 1.66666666666666019037e-01;
  const double p2 = -2.77777777770155933842e-03;
  const double p3 = 6.61375632143793436117e-05;
  const double p4 = -1.65339022054652515390e-06;
  const double p5 = 4.13813679705723846039e-08;
  double hi, lo, r, t, c, y;
  int k;
  if (x != x) return x;
  if (x < -7.45133219101941108420e+02) return 0.0;
  if (x > -3.7252902984619140625e-09) return 1.0 + x; /* |x| < 2^-28 */
  if (x > -0.34657359027997264) {                     /* |x| <= ln2 / 2 */
    k = 0;
    hi = x;
    lo = 0.0;
    r = x;
  } else {
    k = (int)(inv_ln2 * x - 0.5);
    hi = x - (double)k * ln2_hi;
    lo = (double)k * ln2_lo;
    r = hi - lo;
  }
  t = r * r;
  c = r - t * (p1 + t * (p2 + t * (p3 + t * (p4 + t * p5))));
  if (k == 0) return 1.0 - ((r * c) / (c - 2.0) - r);
  y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
  if (k >= -1021) return y * jabd_sn_from_bits((uint64_t)(k + 1023) << 52);
  /* subnormal result: y 2^(k+1000) is exact, the last product rounds */
  return (y * jabd_sn_from_bits((uint64_t)(k + 1000 + 1023) << 52)) *
         jabd_sn_from_bits((uint64_t)(1023 - 1000) << 52);
}

/* max(0, v) as numpy.maximum(0.0, v): NaN stays NaN */
JABD_SN_FN float jabd_sn_relu(float v) { return (v > 0.f || v != v) ? v : 0.f; }

/* IoU of boxes (x1, y1, x2, y2) a and b in fp32, every operation rounded on
 * its own, in the order of the reference's softer_nms (utils/utils_bbox.py:
 * 73-85): areas and extents carry `offset` (1 for pixel boxes). */
JABD_SN_FN float jabd_sn_iou(float ax1, float ay1, float ax2, float ay2, float bx1, float by1,
                             float bx2, float by2, float offset) {
  const float area_a = ((ax2 - ax1) + offset) * ((ay2 - ay1) + offset);
  const float area_b = ((bx2 - bx1) + offset) * ((by2 - by1) + offset);
  const float xx1 = ax1 > bx1 ? ax1 : bx1, yy1 = ay1 > by1 ? ay1 : by1;
  const float xx2 = ax2 < bx2 ? ax2 : bx2, yy2 = ay2 < by2 ? ay2 : by2;
  const float w = jabd_sn_relu((xx2 - xx1) + offset);
  const float h = jabd_sn_relu((yy2 - yy1) + offset);
  const float inter = w * h;
  return inter / ((area_a + area_b) - inter);
}

/* score * exp(-o^2 / sigma): the product in double, rounded to fp32 once
 * (numpy's dets[pos, 4] *= np.exp(-(ovr * ovr) / sigma) on an fp32 row) */
JABD_SN_FN float jabd_sn_decay(float score, float o, double sigma) {
  const double od = (double)o;
  return (float)((double)score * jabd_sn_exp_nonpos(-(od * od) / sigma));
}

/* Ascending total order of scores as numpy.argmax sees them: a NaN is the
 * maximum, -0.0 equals +0.0.  The selection takes the first position of the
 * largest key; the top_k cut ranks by it. */
JABD_SN_FN uint32_t jabd_sn_key(float s) {
  uint32_t f = jabd_sn_float_bits(s);
  if (s != s) return 0xffffffffu;
  if (f == 0x80000000u) f = 0u;
  return (f & 0x80000000u) ? ~f : (f | 0x80000000u);
}

#endif /* JABD_SOFTNMS_MATH_H */

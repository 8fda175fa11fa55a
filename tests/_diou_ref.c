/* C twin of tests/_diou_ref.py's loop (the numpy restatement of the reference's
 * diounms, utils/box_utils.py:450-526), for the 24k-row cases: the same fp32
 * operations in the same order, one at a time (build with -ffp-contract=off),
 * the same NaN rule and the same margin.  Ordering and the top_k cut stay in
 * Python: the boxes arrive in ranked order and the kept ranks go back.
 * tests/test_diou_nms.py checks that the twins agree. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* np.maximum / np.minimum: a NaN operand gives NaN */
static float fmx(float a, float b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }
static float fmn(float a, float b) { return (a != a || b != b) ? NAN : (a < b ? a : b); }

/* b: n boxes (x1, y1, x2, y2) in ranked order; kind 0 = IoU (torchvision's
 * union order), 1 = DIoU.  Writes the kept ranks and the smallest
 * |value - thr| over the finite values compared (HUGE_VAL if none); returns
 * the kept count, -1 on allocation failure. */
int64_t diou_ref_nms(const float* b, int64_t n, double thr, double beta1, int kind,
                     int64_t* keep, double* margin) {
  float* area = (float*)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
  char* sup = (char*)calloc((size_t)(n > 0 ? n : 1), 1);
  int64_t nk = 0;
  double m = HUGE_VAL;
  if (!area || !sup) {
    free(area);
    free(sup);
    return -1;
  }
  for (int64_t i = 0; i < n; ++i) area[i] = (b[4 * i + 2] - b[4 * i]) * (b[4 * i + 3] - b[4 * i + 1]);
  for (int64_t i = 0; i < n; ++i) {
    if (sup[i]) continue;
    keep[nk++] = i;
    const float x1 = b[4 * i], y1 = b[4 * i + 1], x2 = b[4 * i + 2], y2 = b[4 * i + 3];
    const float cxi = (x1 + x2) / 2.0f, cyi = (y1 + y2) / 2.0f;
    for (int64_t j = i + 1; j < n; ++j) {
      if (sup[j]) continue;
      const float xx1 = b[4 * j], yy1 = b[4 * j + 1], xx2 = b[4 * j + 2], yy2 = b[4 * j + 3];
      const float w = fmx(fmn(xx2, x2) - fmx(xx1, x1), 0.0f);
      const float h = fmx(fmn(yy2, y2) - fmx(yy1, y1), 0.0f);
      const float inter = w * h;
      float val;
      if (kind == 0) {
        val = inter / ((area[i] + area[j]) - inter);
      } else {
        const float uni = (area[j] - inter) + area[i];
        const float dx = cxi - (xx1 + xx2) / 2.0f, dy = cyi - (yy1 + yy2) / 2.0f;
        const float d = dx * dx + dy * dy;
        const float ex = fmx(xx2, x2) - fmn(xx1, x1), ey = fmx(yy2, y2) - fmn(yy1, y1);
        const float c = ex * ex + ey * ey;
        float u = d / c;
        if (beta1 != 1.0) u = (float)pow((double)u, beta1);
        val = inter / uni - u;
      }
      const double v = (double)val;
      if (isfinite(v)) {
        const double a = fabs(v - thr);
        if (a < m) m = a;
      }
      if (v > thr) sup[j] = 1; /* NaN: not suppressed */
    }
  }
  *margin = m;
  free(area);
  free(sup);
  return nk;
}

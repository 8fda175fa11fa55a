/* C twin of the Gaussian Soft-NMS for tests/_softnms_ref.py: the literal loop
 * of the reference's softer_nms (utils/utils_bbox.py:88-114) with the swaps it
 * makes, on the arithmetic of csrc/softnms_math.h -- the very text the kernel
 * compiles.  Built by the host compiler with -O2 -ffp-contract=off. */
#include <stdint.h>
#include <stdlib.h>

#include "softnms_math.h"

/* larger as numpy.argmax sees it: a NaN beats every number */
static int sn_greater(float a, float b) { return a > b || (a != a && b == b); }

/* rows [n, 5] (x1, y1, x2, y2, score) are the candidates in input order and
 * are not modified.  Writes the result's positions into `rows` to keep[] and
 * their decayed scores to keep_scores[]; returns their number, or -1 when
 * memory runs out. */
int64_t softnms_ref(const float* rows, int64_t n, double sigma, float offset, double prune,
                    int64_t* keep, float* keep_scores) {
  float* d;
  int64_t* id;
  int64_t N = n, i, pos, p, c;
  if (n <= 0) return 0;
  d = (float*)malloc(sizeof(float) * 5 * (size_t)n);
  id = (int64_t*)malloc(sizeof(int64_t) * (size_t)n);
  if (!d || !id) {
    free(d);
    free(id);
    return -1;
  }
  for (i = 0; i < 5 * n; ++i) d[i] = rows[i];
  for (i = 0; i < n; ++i) id[i] = i;
#define SN_SWAP(a, b)                         \
  do {                                        \
    int64_t ti_ = id[a];                      \
    id[a] = id[b];                            \
    id[b] = ti_;                              \
    for (c = 0; c < 5; ++c) {                 \
      float tf_ = d[5 * (a) + c];             \
      d[5 * (a) + c] = d[5 * (b) + c];        \
      d[5 * (b) + c] = tf_;                   \
    }                                         \
  } while (0)
  for (i = 0; i < N; ++i) {
    int64_t m = i;
    for (p = i + 1; p < N; ++p)
      if (sn_greater(d[5 * p + 4], d[5 * m + 4])) m = p;
    SN_SWAP(m, i);
    pos = i + 1;
    while (pos < N) {
      const float o = jabd_sn_iou(d[5 * i], d[5 * i + 1], d[5 * i + 2], d[5 * i + 3], d[5 * pos],
                                  d[5 * pos + 1], d[5 * pos + 2], d[5 * pos + 3], offset);
      if (o > 0.f) {
        d[5 * pos + 4] = jabd_sn_decay(d[5 * pos + 4], o, sigma);
        if ((double)d[5 * pos + 4] < prune) {
          SN_SWAP(pos, N - 1);
          N -= 1;
          pos -= 1;
        }
      }
      pos += 1;
    }
  }
#undef SN_SWAP
  for (i = 0; i < N; ++i) {
    keep[i] = id[i];
    keep_scores[i] = d[5 * i + 4];
  }
  free(d);
  free(id);
  return N;
}

void softnms_ref_exp(const double* x, double* y, int64_t n) {
  int64_t i;
  for (i = 0; i < n; ++i) y[i] = jabd_sn_exp_nonpos(x[i]);
}

uint32_t softnms_ref_key(float s) { return jabd_sn_key(s); }

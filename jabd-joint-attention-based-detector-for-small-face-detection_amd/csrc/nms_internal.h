// Internal entry to the batched NMS pipeline (shared with jabd_detect_ex_f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jabd {
// suppression rule (the `kind` of jabd_batched_nms_ex_f32 / jabd_detect_ex_f32)
enum : int { kNmsIoU = 0, kNmsDIoU = 1 };
size_t nms_ws_bytes(int64_t batch, int64_t n);
// kind kNmsDIoU: IoU - (d/c)^beta1 > iou_thr, beta1 > 0 (ignored by kNmsIoU);
// top_k > 0: only each image's first top_k ranked rows are candidates.
int nms_core(const float* boxes, int64_t box_stride, int64_t box_bstride,
             const float* scores, int64_t score_stride, int64_t score_bstride,
             const int64_t* n_valid, int64_t batch, int64_t n, double iou_thr,
             float score_thr, int64_t* keep, int64_t* n_keep, void* ws,
             size_t ws_bytes, hipStream_t st, int kind, double beta1, int64_t top_k);

// Gaussian Soft-NMS (soft_nms.hip; shared with jabd_detect_soft_f32): the
// arguments of jabd_batched_soft_nms_f32, which also checks them.
size_t soft_nms_ws_bytes(int64_t batch, int64_t n);
int soft_nms_core(const float* boxes, int64_t box_stride, int64_t box_bstride,
                  const float* scores, int64_t score_stride, int64_t score_bstride,
                  const int64_t* n_valid, int64_t batch, int64_t n, double sigma, float offset,
                  double prune, float score_thr, int64_t top_k, int64_t* keep,
                  float* keep_scores, int64_t* n_keep, void* ws, size_t ws_bytes,
                  hipStream_t st);
}  // namespace jabd

// Person boxes around a caller-named detector (diffuman4d_amd/host/detect.py; the reference's detector step of predict_keypoints:
// scripts/preprocess/sapiens/lite/demo/vis_pose.py:425-440 with detector_utils.py process_one_image_bbox and pose_utils.py nms).  The
// network is the caller's; the two entries here are the arithmetic on either side of it.
//
//   dm4d_detect_input_u8_f32   composite over black through the mask, keep-ratio bilinear resize into the canvas' corner, pad, normalise
//   dm4d_detect_select_f32     threshold, rescale, exact top-k (radix select + bitonic sort), greedy NMS, one workgroup per image
//
// The resize and the composite are integer-only from the host's tables on; the normalisation and the NMS round every fp32 operation
// on its own (this file is compiled with -ffp-contract=off).  No global atomics, no float atomics, no workgroup waits on another, and
// an image's result does not depend on the batch around it.
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "dm4d.h"
#include "errors.h"
#include "image_common.h"
#include "pose_rows.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- network input
constexpr int kTileW = 64, kTileH = 4;  // a workgroup's tile of the canvas: one pixel per thread, a wave per row

struct DetectNorm {
  float mean[3], stdv[3];
};

// grid (ceil(W / kTileW), ceil(H / kTileH), n)
__global__ void __launch_bounds__(kTileW* kTileH) detect_input_kernel(const uint8_t* __restrict__ staging, const int64_t* __restrict__ desc,
                                                                      const int32_t* __restrict__ tab, float* __restrict__ out, int H, int W,
                                                                      int pad_value, int bgr, DetectNorm norm) {
  const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  if (x >= W || y >= H) return;
  const int img_k = blockIdx.z;
  const int64_t* d = desc + (int64_t)img_k * DM4D_POSE_FIELDS;
  const int32_t* t = tab + d[4];  // {nw, nh | xofs[nw] | yofs[nh] | alpha[nw] | beta[nh]}
  const int nw = t[0], nh = t[1];
  int v[3] = {pad_value, pad_value, pad_value};
  if (x < nw && y < nh) {
    const uint8_t* img = staging + d[0];
    const uint8_t* mask = d[1] >= 0 ? staging + d[1] : nullptr;
    const int h = (int)d[2], w = (int)d[3];
    const int sx = t[2 + x], sy = t[2 + nw + y];
    const int32_t ca = t[2 + nw + nh + x], cb = t[2 + 2 * nw + nh + y];
    const int a0 = (int16_t)(ca & 0xffff), a1 = (int16_t)(ca >> 16), b0 = (int16_t)(cb & 0xffff), b1 = (int16_t)(cb >> 16);
    const int px[2] = {sx, min(sx + 1, w - 1)}, py[2] = {sy, min(sy + 1, h - 1)};
    int S[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      uint32_t c[2][3];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int64_t at = (int64_t)py[r] * w + px[k];
        const uint8_t* p = img + at * 3;
        c[k][0] = p[0], c[k][1] = p[1], c[k][2] = p[2];
        if (mask) {
          const uint32_t m = mask[at];
          c[k][0] = muldiv255(c[k][0], m), c[k][1] = muldiv255(c[k][1], m), c[k][2] = muldiv255(c[k][2], m);
        }
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) S[r][ch] = (int)c[0][ch] * a0 + (int)c[1][ch] * a1;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = (((b0 * (S[0][ch] >> 4)) >> 16) + ((b1 * (S[1][ch] >> 4)) >> 16) + 2) >> 2;
  }
  float* o = out + (int64_t)img_k * 3 * H * W + (int64_t)y * W + x;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    o[(int64_t)c * H * W] = __fdiv_rn(__fsub_rn((float)v[bgr ? 2 - c : c], norm.mean[c]), norm.stdv[c]);
}

// -------------------------------------------------------------------------------------------------------------------------- select
constexpr int kSelThreads = 1024;
constexpr int kKeep = DM4D_DETECT_MAX_KEEP;
static_assert((kKeep & (kKeep - 1)) == 0 && kKeep <= kSelThreads, "DM4D_DETECT_MAX_KEEP: a power of two (bitonic sort), one key per thread");

struct ImageBox {
  float x1, y1, x2, y2;
};

// uint32 whose unsigned order is the float order (-0 taken as +0; NaN never gets here)
__device__ __forceinline__ uint32_t ordered_bits(float s) {
  const uint32_t b = __float_as_uint(s == 0.f ? 0.f : s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// An anchor's 64-bit key {ordered score bits << 32 | ~index}, 0 unless it is a candidate with a usable image box; what == 1: it is
// above the threshold but its box is dropped.  Keys are unique per anchor and never 0 for a candidate (index < 2^20).
__device__ __forceinline__ uint64_t anchor_key(const float* __restrict__ boxes, const float* __restrict__ scores, int a, int C, int cat,
                                               float score_thr, float inv_w, float inv_h, ImageBox& b, float& s, int& what) {
  s = scores[(int64_t)a * C + cat];
  what = 0;
  if (!(s > score_thr)) return 0;
  const float4 q = *reinterpret_cast<const float4*>(boxes + (int64_t)a * 4);
  b.x1 = q.x * inv_w, b.y1 = q.y * inv_h, b.x2 = q.z * inv_w, b.y2 = q.w * inv_h;
  const bool ok = isfinite(b.x1) && isfinite(b.y1) && isfinite(b.x2) && isfinite(b.y2) && b.x2 > b.x1 && b.y2 > b.y1;
  what = ok ? 2 : 1;
  return ok ? ((uint64_t)ordered_bits(s) << 32) | (uint32_t)~(uint32_t)a : 0;
}

// one workgroup per image
__global__ void __launch_bounds__(kSelThreads) detect_select_kernel(const float* __restrict__ boxes_all, const float* __restrict__ scores_all,
                                                                    const float* __restrict__ inv_scale, int A, int C, int cat,
                                                                    float score_thr, float nms_thr, int max_per_img,
                                                                    int32_t* __restrict__ counts, float* __restrict__ out_boxes,
                                                                    int32_t* __restrict__ out_idx) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint64_t s_key[kKeep];
  __shared__ float s_box[kKeep][4], s_area[kKeep], s_score[kKeep];
  __shared__ int s_alive[kKeep];
  __shared__ uint32_t s_above, s_dropped, s_fill;
  __shared__ uint64_t s_prefix;
  __shared__ int s_need, s_done;
  const int tid = threadIdx.x, img = blockIdx.x;
  const float* boxes = boxes_all + (int64_t)img * A * 4;
  const float* scores = scores_all + (int64_t)img * A * C;
  const float inv_w = inv_scale[2 * img], inv_h = inv_scale[2 * img + 1];
  ImageBox b;
  float s;
  int what;

  if (tid == 0) s_above = 0, s_dropped = 0, s_fill = 0, s_prefix = 0, s_need = max_per_img, s_done = 0;
  if (tid < kKeep) s_key[tid] = 0;
  __syncthreads();
  // pass 0: how many candidates, how many of them dropped
  uint32_t above = 0, dropped = 0;
  for (int a = tid; a < A; a += kSelThreads) {
    anchor_key(boxes, scores, a, C, cat, score_thr, inv_w, inv_h, b, s, what);
    above += what != 0, dropped += what == 1;
  }
  if (above) atomicAdd(&s_above, above);      // integer LDS atomics: the sums do not depend on the order
  if (dropped) atomicAdd(&s_dropped, dropped);
  __syncthreads();
  const int n_above = (int)s_above, n_dropped = (int)s_dropped, valid = n_above - n_dropped;
  const int m = min(valid, max_per_img);  // the boxes that reach the NMS

  // radix select, only with more candidates than places: the key of rank max_per_img, 8 bits a pass from the top.  s_prefix holds the
  // digits found so far; a pass counts the keys that share them by their next digit; walking the histogram from 255 down finds the
  // digit that holds the rank.  When the keys that share the new prefix are exactly the ones still needed, every one of them is
  // taken and the lower digits stay 0.
  uint64_t least = 0;  // keys >= least stay; there are exactly m of them
  if (valid > max_per_img) {
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) s_hist[tid] = 0;
      __syncthreads();
      const uint64_t prefix = s_prefix;
      for (int a = tid; a < A; a += kSelThreads) {
        const uint64_t key = anchor_key(boxes, scores, a, C, cat, score_thr, inv_w, inv_h, b, s, what);
        if (key && (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        int need = s_need, dgt = 255;
        for (; dgt > 0 && (int)s_hist[dgt] < need; --dgt) need -= (int)s_hist[dgt];
        s_prefix = prefix | ((uint64_t)dgt << shift);
        s_need = need;
        s_done = (int)s_hist[dgt] == need;
      }
      __syncthreads();
      if (s_done) break;  // uniform: read after the barrier by every thread
    }
    least = s_prefix;
  }
  // gather the m keys that stay (their slots depend on the order of arrival, the sort below does not)
  if (valid > 0) {
    for (int a = tid; a < A; a += kSelThreads) {
      const uint64_t key = anchor_key(boxes, scores, a, C, cat, score_thr, inv_w, inv_h, b, s, what);
      if (key && key >= least) {
        const uint32_t slot = atomicAdd(&s_fill, 1u);
        if (slot < (uint32_t)kKeep) s_key[slot] = key;  // never more than m <= kKeep; the guard keeps a wrong count inside the array
      }
    }
  }
  __syncthreads();
  // bitonic sort, descending, of kKeep keys (zeros behind the m real ones)
  for (int k = 2; k <= kKeep; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (tid < kKeep) {
        const int other = tid ^ j;
        if (other > tid) {
          const uint64_t u = s_key[tid], v = s_key[other];
          const bool desc = (tid & k) == 0;
          if (desc ? u < v : u > v) s_key[tid] = v, s_key[other] = u;
        }
      }
      __syncthreads();
    }
  }
  // the sorted candidates' image boxes, areas and scores
  if (tid < m) {
    const int a = (int)~(uint32_t)(s_key[tid] & 0xffffffffu);
    anchor_key(boxes, scores, a, C, cat, score_thr, inv_w, inv_h, b, s, what);
    s_box[tid][0] = b.x1, s_box[tid][1] = b.y1, s_box[tid][2] = b.x2, s_box[tid][3] = b.y2;
    s_area[tid] = ((b.x2 - b.x1) + 1.f) * ((b.y2 - b.y1) + 1.f);
    s_score[tid] = s;
    s_alive[tid] = 1;
  }
  __syncthreads();
  // greedy NMS: box i, if it still stands, removes every later box that overlaps it by more than nms_thr (or by NaN)
  for (int i = 0; i + 1 < m; ++i) {
    if (s_alive[i] && tid > i && tid < m && s_alive[tid]) {
      const float xx1 = fmaxf(s_box[i][0], s_box[tid][0]), yy1 = fmaxf(s_box[i][1], s_box[tid][1]);
      const float xx2 = fminf(s_box[i][2], s_box[tid][2]), yy2 = fminf(s_box[i][3], s_box[tid][3]);
      const float w = fmaxf(0.f, (xx2 - xx1) + 1.f), h = fmaxf(0.f, (yy2 - yy1) + 1.f);
      const float inter = w * h;
      const float ovr = __fdiv_rn(inter, (s_area[i] + s_area[tid]) - inter);
      if (!(ovr <= nms_thr)) s_alive[tid] = 0;
    }
    __syncthreads();
  }
  // kept order = sorted order without the removed: a kept box's place is the number of kept boxes before it
  int kept = 0, place = -1;
  for (int j = 0; j < m; ++j) {
    if (j == tid && s_alive[j]) place = kept;
    kept += s_alive[j];
  }
  float* ob = out_boxes + (int64_t)img * max_per_img * 5;
  int32_t* oi = out_idx + (int64_t)img * max_per_img;
  if (tid >= kept && tid < max_per_img) {
#pragma unroll
    for (int c = 0; c < 5; ++c) ob[tid * 5 + c] = 0.f;
    oi[tid] = -1;
  }
  if (place >= 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) ob[place * 5 + c] = s_box[tid][c];
    ob[place * 5 + 4] = s_score[tid];
    oi[place] = (int)~(uint32_t)(s_key[tid] & 0xffffffffu);
  }
  if (tid == 0) counts[3 * img] = kept, counts[3 * img + 1] = n_dropped, counts[3 * img + 2] = n_above;
}

}  // namespace

extern "C" int dm4d_detect_input_u8_f32(void* stream, const void* staging, int64_t staging_bytes, const int64_t* desc_host,
                                        const int64_t* desc_dev, int n, const int32_t* tab_host, const int32_t* tab_dev, int64_t tab_len,
                                        const float* norm_host, float* out, int H, int W, int pad_value, int bgr) {
  if (!staging || !desc_host || !desc_dev || !tab_host || !tab_dev || !norm_host || !out)
    return dm4d_set_error(DM4D_ERR_ARG, "detect_input: null pointer");
  if (n < 1 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "detect_input: n outside 1..65535");
  if (H < 1 || W < 1 || H > DM4D_DETECT_MAX_CANVAS || W > DM4D_DETECT_MAX_CANVAS)
    return dm4d_set_error(DM4D_ERR_ARG, "detect_input: canvas size outside 1..4096");
  if (pad_value < 0 || pad_value > 255) return dm4d_set_error(DM4D_ERR_ARG, "detect_input: pad_value outside 0..255");
  if (staging_bytes < 1 || tab_len < 1) return dm4d_set_error(DM4D_ERR_ARG, "detect_input: empty staging buffer or table");
  if (((uintptr_t)out & 3) || ((uintptr_t)tab_dev & 3) || ((uintptr_t)desc_dev & 7))
    return dm4d_set_error(DM4D_ERR_ARG, "detect_input: out, tab_dev (4 bytes) and desc_dev (8 bytes) must be aligned");
  DetectNorm norm;
  for (int c = 0; c < 3; ++c) {
    norm.mean[c] = norm_host[c], norm.stdv[c] = norm_host[3 + c];
    if (!isfinite(norm.mean[c]) || !isfinite(norm.stdv[c]) || norm.stdv[c] == 0.f)
      return dm4d_set_error(DM4D_ERR_ARG, "detect_input: mean must be finite and std finite and non-zero");
  }
  const int rc = pose_check_rows("detect_input", staging_bytes, desc_host, n, true, false, true);
  if (rc) return rc;
  for (int r = 0; r < n; ++r) {
    const int64_t* d = desc_host + (int64_t)r * DM4D_POSE_FIELDS;
    const int64_t h = d[2], w = d[3], off = d[4];
    if (off < 0 || off > tab_len || 2 > tab_len - off) return dm4d_set_error(DM4D_ERR_ARG, "detect_input: an image's resize table lies outside tab");
    const int32_t* t = tab_host + off;
    const int64_t nw = t[0], nh = t[1];
    if (nw < 1 || nh < 1 || nw > W || nh > H) return dm4d_set_error(DM4D_ERR_ARG, "detect_input: the resized image is empty or larger than the canvas");
    if (2 * (nw + nh) > tab_len - off - 2) return dm4d_set_error(DM4D_ERR_ARG, "detect_input: an image's resize table lies outside tab");
    const int32_t *ofs = t + 2, *coef = ofs + nw + nh;  // {xofs | yofs} and {alpha | beta}, each walked as one run
    for (int64_t k = 0; k < nw + nh; ++k) {
      if (ofs[k] < 0 || ofs[k] >= (k < nw ? w : h))
        return dm4d_set_error(DM4D_ERR_ARG, "detect_input: a resize table's tap window lies outside its image");
      const int c0 = (int16_t)(coef[k] & 0xffff), c1 = (int16_t)(coef[k] >> 16);
      if (c0 < 0 || c1 < 0 || c0 > DM4D_DETECT_COEF_ONE || c1 > DM4D_DETECT_COEF_ONE)
        return dm4d_set_error(DM4D_ERR_ARG, "detect_input: a resize weight is outside 0..2048");
    }
  }
  hipLaunchKernelGGL(detect_input_kernel, dim3((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, n), dim3(kTileW * kTileH), 0,
                     (hipStream_t)stream, (const uint8_t*)staging, desc_dev, tab_dev, out, H, W, pad_value, bgr ? 1 : 0, norm);
  return dm4d_check_launch("detect_input_kernel");
}

extern "C" int dm4d_detect_select_f32(void* stream, const float* boxes, const float* scores, const float* inv_scale, int n, int A, int C, int cat,
                                      float score_thr, float nms_thr, int max_per_img, int32_t* counts, float* out_boxes, int32_t* out_idx) {
  if (!boxes || !scores || !inv_scale || !counts || !out_boxes || !out_idx) return dm4d_set_error(DM4D_ERR_ARG, "detect_select: null pointer");
  if (n < 1 || n > 65535) return dm4d_set_error(DM4D_ERR_ARG, "detect_select: n outside 1..65535");
  if (A < 1 || A > DM4D_DETECT_MAX_ANCHORS) return dm4d_set_error(DM4D_ERR_ARG, "detect_select: A outside 1..2^20");
  if (C < 1 || C > DM4D_DETECT_MAX_CLASSES) return dm4d_set_error(DM4D_ERR_ARG, "detect_select: C outside 1..4096");
  if (cat < 0 || cat >= C) return dm4d_set_error(DM4D_ERR_ARG, "detect_select: cat outside 0..C - 1");
  if (max_per_img < 1 || max_per_img > DM4D_DETECT_MAX_KEEP) return dm4d_set_error(DM4D_ERR_ARG, "detect_select: max_per_img outside 1..256");
  if (!isfinite(score_thr) || !isfinite(nms_thr)) return dm4d_set_error(DM4D_ERR_ARG, "detect_select: score_thr and nms_thr must be finite");
  if (((uintptr_t)boxes & 15) || ((uintptr_t)scores & 3) || ((uintptr_t)inv_scale & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)out_boxes & 3) ||
      ((uintptr_t)out_idx & 3))
    return dm4d_set_error(DM4D_ERR_ARG, "detect_select: boxes (16 bytes) and the other pointers (4 bytes) must be aligned");
  hipLaunchKernelGGL(detect_select_kernel, dim3(n), dim3(kSelThreads), 0, (hipStream_t)stream, boxes, scores, inv_scale, A, C, cat, score_thr,
                     nms_thr, max_per_img, counts, out_boxes, out_idx);
  return dm4d_check_launch("detect_select_kernel");
}

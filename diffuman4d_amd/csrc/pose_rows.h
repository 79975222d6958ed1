// The host-side check of the DM4D_POSE_FIELDS descriptors that pose.hip and detect.hip take (include/dm4d.h, dm4d_pose_input_u8_f32):
// sizes, plane offsets against the staging buffer, spare fields.  Defined once; nothing here runs on the device.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "dm4d.h"
#include "errors.h"

// aligned16: the planes must start on 16-byte boundaries, as host/pose.py::plane_layout lays them out
inline int pose_check_rows(const char* what, int64_t staging_bytes, const int64_t* desc_host, int rows, bool need_image, bool need_mask,
                           bool aligned16) {
  static thread_local char msg[160];
  for (int r = 0; r < rows; ++r) {
    const int64_t* d = desc_host + (int64_t)r * DM4D_POSE_FIELDS;
    const int64_t h = d[2], w = d[3];
    const char* bad = nullptr;
    if (h < 1 || h > DM4D_POSE_MAX_SIDE || w < 1 || w > DM4D_POSE_MAX_SIDE)
      bad = "image size outside 1..16384";
    else if (need_image && (d[0] < 0 || d[0] > staging_bytes || h * w * 3 > staging_bytes - d[0]))
      bad = "image outside the staging buffer";
    else if (d[1] < (need_mask ? 0 : -1))
      bad = "mask offset is negative";
    else if (d[1] >= 0 && (d[1] > staging_bytes || h * w > staging_bytes - d[1]))
      bad = "mask outside the staging buffer";
    else if (aligned16 && (((need_image ? d[0] : 0) & 15) || (d[1] >= 0 && (d[1] & 15))))
      bad = "a plane offset is not 16-byte aligned";
    else if (d[5] || d[6] || d[7])
      bad = "spare fields must be 0";
    if (bad) {
      snprintf(msg, sizeof msg, "%s: row %d: %s", what, r, bad);
      return dm4d_set_error(DM4D_ERR_ARG, msg);
    }
  }
  return 0;
}

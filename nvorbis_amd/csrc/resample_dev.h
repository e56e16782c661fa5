// resample_dev.h -- what k_resample_rows (kernels_resample.hip) and its launcher (nvh_resample.hip) share: the kernel's argument
// block and its tile geometry.  include/nvorbis_hip.h states the rule (nvh_resample_rows).
#pragma once
#include <stdint.h>

#define NVH_RS_THREADS 256
#define NVH_RS_TILE 512           // consecutive outputs of one (row, channel) per workgroup step: NVH_RESAMPLE_TILE of the ABI
#define NVH_RS_TAP_FLOATS 16384   // LDS budget of the tap table, rows padded to an odd stride (else the taps are read through L2)
#define NVH_RS_SRC_FLOATS 4096    // LDS budget of a tile's source span (else the span is read through L2, bounds checked per tap)

struct NvhResampleArgs {
  const float* taps;  // [L][2 * half]
  const float* src;
  void* dst;
  // the per-row block, one upload: origin[rows], start[rows], valid[rows] (int64), then dst_row[rows] (int32)
  const long long* origin;
  const long long* start;
  const long long* valid;
  const int* dst_row;
  int* clipped;  // one word per destination row, or null
  long long length, src_length;
  long long src_row_stride, src_time_stride, src_chan_stride;
  long long dst_row_stride, dst_time_stride, dst_chan_stride;
  int L, M, half;
  int taps_in_lds;   // the table fits NVH_RS_TAP_FLOATS
  int tiles;         // ceil(length / NVH_RS_TILE)
};

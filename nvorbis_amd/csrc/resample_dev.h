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

// The launch route of one call, from integers alone: what nvh_resample_rows launches and nvh_resample_route reports.
struct NvhResampleRoute {
  int taps_in_lds;   // the table, rows padded to an odd stride, fits NVH_RS_TAP_FLOATS
  long long tiles;   // ceil(length / NVH_RS_TILE)
  int grid_y;        // workgroups per (row, channel): each walks tiles y, y + grid_y, ..
  int lds_bytes;     // the staged table (or nothing) and a tile's source span
};
// A workgroup stages the taps once and walks its tiles: four tiles each once there are workgroups enough to fill the chip.
static inline constexpr NvhResampleRoute nvh_resample_route_for(int L, int half, int rows, int channels, long long length) {
  const long long padded = (long long)L * ((2 * half) | 1);
  const bool in_lds = padded <= NVH_RS_TAP_FLOATS;
  const long long tiles = (length + NVH_RS_TILE - 1) / NVH_RS_TILE;
  const long long gy = (long long)rows * channels * tiles >= 4096 ? (tiles + 3) / 4 : tiles;
  return {in_lds ? 1 : 0, tiles, (int)(gy < 65535 ? gy : 65535), (int)(((in_lds ? padded : 0) + NVH_RS_SRC_FLOATS) * 4)};
}
static_assert(nvh_resample_route_for(160, 45, 6, 2, 1041).taps_in_lds == 1 && nvh_resample_route_for(160, 45, 6, 2, 1041).grid_y == 3, "44100 -> 16000");
static_assert(nvh_resample_route_for(160, 45, 6, 2, 1041).lds_bytes == (160 * 91 + NVH_RS_SRC_FLOATS) * 4, "... its table beside the span");
static_assert(nvh_resample_route_for(1, 16384, 1, 1, 5).taps_in_lds == 0 && nvh_resample_route_for(1, 16384, 1, 1, 5).lds_bytes == NVH_RS_SRC_FLOATS * 4, "1024 -> 1");
static_assert(nvh_resample_route_for(2, 16, 1, 1, 4000 * 512).grid_y == 4000 && nvh_resample_route_for(2, 16, 1, 1, 8192 * 512).grid_y == 2048, "four tiles each");
// (known cases away from the thresholds: tests/test_row_routes.py walks the thresholds' edges through nvh_resample_route's export)

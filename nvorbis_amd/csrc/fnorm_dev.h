// fnorm_dev.h -- what k_fnorm_rows (kernels_fnorm.hip) and its launcher (nvh_fnorm.hip) share: the kernel's argument block and its
// LDS geometry.  include/nvorbis_hip.h states the rule (nvh_fnorm_rows).
#pragma once
#include <stdint.h>

#define NVH_FNORM_WAVES 8  // wavefronts per workgroup: a wavefront owns a band at a time
#define NVH_FNORM_THREADS (64 * NVH_FNORM_WAVES)
#define NVH_FNORM_MAX_BANDS 256
#define NVH_FNORM_LDS_BYTES 81920  // a workgroup's LDS budget: two workgroups per CU (160 KB), as NVH_MEL_LDS_BYTES
#define NVH_FNORM_MAX_BLOCKS 2048  // workgroups of a launch: eight per CU; more work items are walked
#define NVH_FNORM_TILE 64          // frames per tile of the re-reading path (the 64 partials of a band are the tile's frames)

// The workgroup's LDS in floats: the bands' means (first their sums), the bands' deviations (first their sums of squares) and the
// wavefronts' maxima; then the data region.
#define NVH_FNORM_FIXED_FLOATS (2 * NVH_FNORM_MAX_BANDS + 16)
#define NVH_FNORM_DATA_FLOATS (NVH_FNORM_LDS_BYTES / 4 - NVH_FNORM_FIXED_FLOATS)
// Resident: the (row, channel)'s F x B floats lie in the data region band after band, a band's frames side by side, F rounded up to
// an odd count (a frame's bands then spread over the banks).
static inline constexpr int nvh_fnorm_band_pitch(int frames) { return frames | 1; }
static inline constexpr bool nvh_fnorm_resident(int frames, int bands) {
  return (long long)nvh_fnorm_band_pitch(frames) * bands <= NVH_FNORM_DATA_FLOATS;
}
// Re-reading: the data region holds the partials p[b][l] at b * 65 + l while a sum runs over a source whose band stride is the
// smaller one, and a tile of 64 frames x B at fl * (B | 1) + b while the last pass turns one layout into the other.
static inline constexpr int nvh_fnorm_reread_floats(int bands) {
  return bands * (NVH_FNORM_TILE + 1) > NVH_FNORM_TILE * (bands | 1) ? bands * (NVH_FNORM_TILE + 1) : NVH_FNORM_TILE * (bands | 1);
}

struct NvhFnormArgs {
  const float* src;
  float* dst;
  const long long* vf;  // counted frames per row (the per-row block, one upload), or null: frames
  long long src_row_stride, src_chan_stride, src_frame_stride, src_band_stride;
  long long dst_row_stride, dst_chan_stride, dst_frame_stride, dst_band_stride;
  long long total;  // rows * channels: the workgroups' work items
  int channels, frames, bands;
  int mode, axis;
  float eps, pad_value, range, offset, gain;
  int src_band_fast;  // the source's band stride is the smaller one: a frame's bands run along the lanes, else a band's frames
  int dst_band_fast;  // the same for the destination
};

// The launch route of one call, from integers alone: what nvh_fnorm_rows launches and nvh_fnorm_route reports.
struct NvhFnormRoute {
  int resident;   // nvh_fnorm_resident: read once and normalised out of LDS; else the source is re-read
  int lds_bytes;
  int blocks;     // workgroups: each walks items b, b + blocks, ..
};
static inline constexpr NvhFnormRoute nvh_fnorm_route_for(int frames, int bands, long long total_items) {
  const bool resident = nvh_fnorm_resident(frames, bands);
  const long long data = resident ? (long long)nvh_fnorm_band_pitch(frames) * bands : nvh_fnorm_reread_floats(bands);
  return {resident ? 1 : 0, (int)((NVH_FNORM_FIXED_FLOATS + data) * 4), (int)(total_items < NVH_FNORM_MAX_BLOCKS ? total_items : NVH_FNORM_MAX_BLOCKS)};
}
static_assert(nvh_fnorm_route_for(1244, 16, 12).resident == 1 && nvh_fnorm_route_for(1244, 16, 12).lds_bytes == 4 * (528 + 1245 * 16), "resident");
static_assert(nvh_fnorm_route_for(1248, 16, 5000).resident == 0 && nvh_fnorm_route_for(1248, 16, 5000).lds_bytes == 4 * (528 + 64 * 17), "re-reading");
static_assert(nvh_fnorm_route_for(1248, 16, 5000).blocks == NVH_FNORM_MAX_BLOCKS && nvh_fnorm_route_for(1244, 16, 12).blocks == 12, "");
// (known cases away from the threshold: tests/test_row_routes.py walks its edge, (1246, 16) to (1248, 16), through nvh_fnorm_route's export)

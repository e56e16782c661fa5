// cep_dev.h -- what k_cep_rows (kernels_cep.hip) and its launcher (nvh_cep.hip) share: the kernel's argument block, its LDS
// geometry and the launch route.  include/nvorbis_hip.h states the rule (nvh_cep_rows).
#pragma once
#include <stdint.h>

#define NVH_CEP_WAVES 4  // wavefronts per workgroup: the lanes run along the staged frames of a block of four cepstral indices
#define NVH_CEP_THREADS (64 * NVH_CEP_WAVES)
#define NVH_CEP_TILE 24  // output frames of a work item (the header's NVH_CEP_FRAMES): tile + the widest halo, 56 frames, fits the budget at 256 bands
#define NVH_CEP_KBLOCK 4          // cepstral indices a lane accumulates side by side: one 16-byte read of the table per band
#define NVH_CEP_MAX_BANDS 256
#define NVH_CEP_MAX_COLS 256      // Q, the output's columns: what nvh_fnorm_rows takes
#define NVH_CEP_WINDOW_MAX 8      // N
#define NVH_CEP_LDS_BYTES 81920   // a workgroup's LDS budget: two workgroups per CU (160 KB), as NVH_FNORM_LDS_BYTES
#define NVH_CEP_MAX_BLOCKS 2048   // workgroups of a launch: eight per CU; more work items are walked
// The delta scales in LDS and behind the DCT table in device memory: s_1[-N .. N] at 0, s_2[-2N .. 2N] at 17, zeros up to 64.
#define NVH_CEP_SCALE_FLOATS 64
#define NVH_CEP_S2_AT (2 * NVH_CEP_WINDOW_MAX + 1)

// A work item stages its tile's frames and `halo` frames on each side: `slots` frames, slot s holding frame f0 - halo + s of the
// (row, channel) -- or, outside the tile, that frame clamped into the counted ones.
static inline constexpr int nvh_cep_halo(int order, int window) { return order * window; }
static inline constexpr int nvh_cep_slots(int order, int window) { return NVH_CEP_TILE + 2 * nvh_cep_halo(order, window); }
// The DCT table as the kernel reads it: [b][kpad] floats, kpad = K rounded up to whole blocks (zeros behind K), so that the four
// weights of a block at one band are 16 aligned bytes.  No table without a transform.
static inline constexpr int nvh_cep_kpad(int ceps) { return (ceps + NVH_CEP_KBLOCK - 1) / NVH_CEP_KBLOCK * NVH_CEP_KBLOCK; }
static inline constexpr int nvh_cep_table_floats(int dct, int bands, int ceps) { return dct ? bands * nvh_cep_kpad(ceps) : 0; }
// The staged frames, slot s's band b at s * (B | 1) + b, and behind them their cepstra, slot s's index k at s * (K | 1) + k
// (odd pitches: lanes along the frames spread over the banks).  Without a transform the staged frames are the cepstra.
static inline constexpr int nvh_cep_tile_floats(int dct, int bands, int ceps, int order, int window) {
  return nvh_cep_slots(order, window) * ((bands | 1) + (dct ? (ceps | 1) : 0));
}
// the largest tiles of each order (K at its limit Q / (1 + o)) fit the budget without their table
static_assert((NVH_CEP_SCALE_FLOATS + nvh_cep_tile_floats(1, 256, 85, 2, 8)) * 4 <= NVH_CEP_LDS_BYTES, "");
static_assert((NVH_CEP_SCALE_FLOATS + nvh_cep_tile_floats(1, 256, 128, 1, 8)) * 4 <= NVH_CEP_LDS_BYTES, "");
static_assert((NVH_CEP_SCALE_FLOATS + nvh_cep_tile_floats(1, 256, 256, 0, 8)) * 4 <= NVH_CEP_LDS_BYTES, "");

struct NvhCepArgs {
  const float* src;
  float* dst;
  const long long* vf;  // counted frames per row (the per-row block, one upload), or null: frames
  const float* tab;     // the DCT table [b][kpad], then NVH_CEP_SCALE_FLOATS floats of delta scales
  long long src_row_stride, src_chan_stride, src_frame_stride, src_band_stride;
  long long dst_row_stride, dst_chan_stride, dst_frame_stride, dst_col_stride;
  long long total;  // rows * channels * tiles: the workgroups' work items
  long long tiles;  // per (row, channel)
  int channels, frames, bands, ceps;
  int dct;  // NVH_CEP_DCT2; 0: the cepstra are the input
  int order, window;
  int src_band_fast;  // the source's band stride is the smaller one: a frame's bands run along the lanes, else a band's frames
  int dst_col_fast;   // the same for the destination's columns
};

// The launch route of one call, from integers alone: what nvh_cep_rows launches and nvh_cep_route reports.
struct NvhCepRoute {
  int staged;  // the DCT table is copied into LDS once per workgroup; else every read of it goes through the caches
  int lds_bytes;
  int blocks;  // workgroups: each walks items b, b + blocks, ..
};
static inline constexpr NvhCepRoute nvh_cep_route_for(int dct, int bands, int ceps, int order, int window, long long total_items) {
  const int tile = NVH_CEP_SCALE_FLOATS + nvh_cep_tile_floats(dct, bands, ceps, order, window);
  const int table = nvh_cep_table_floats(dct, bands, ceps);
  const bool staged = table > 0 && (long long)(tile + table) * 4 <= NVH_CEP_LDS_BYTES;
  return {staged ? 1 : 0, (tile + (staged ? table : 0)) * 4, (int)(total_items < NVH_CEP_MAX_BLOCKS ? total_items : NVH_CEP_MAX_BLOCKS)};
}
// 80 bands -> 13 cepstra with deltas and delta-deltas over N = 2: 32 slots of 81 + 13 floats, and a table of 80 x 16
static_assert(nvh_cep_route_for(1, 80, 13, 2, 2, 7).staged == 1 && nvh_cep_route_for(1, 80, 13, 2, 2, 7).lds_bytes == 4 * (64 + 32 * 94 + 1280), "staged");
static_assert(nvh_cep_route_for(1, 256, 85, 2, 8, 5000).staged == 0 && nvh_cep_route_for(1, 256, 85, 2, 8, 5000).lds_bytes == 4 * (64 + 56 * 342), "through the caches");
static_assert(nvh_cep_route_for(0, 80, 80, 2, 2, 5000).staged == 0 && nvh_cep_route_for(0, 80, 80, 2, 2, 5000).lds_bytes == 4 * (64 + 32 * 81), "no table");
static_assert(nvh_cep_route_for(1, 256, 85, 2, 8, 5000).blocks == NVH_CEP_MAX_BLOCKS && nvh_cep_route_for(1, 80, 13, 2, 2, 7).blocks == 7, "");
// (known cases away from the threshold: tests/test_cep_routes.py walks its edge through nvh_cep_route's export)

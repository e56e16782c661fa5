// mel_dev.h -- what k_mel_rows (kernels_mel.hip) and its launcher (nvh_mel.hip) share: the kernel's argument block and its LDS
// geometry.  include/nvorbis_hip.h states the rule (nvh_mel_rows; nvh_mel_front for the front of a frame).
#pragma once
#include <stdint.h>

#define NVH_MEL_WAVES 4        // wavefronts per workgroup, one frame each: NVH_MEL_FRAMES of the ABI
#define NVH_MEL_THREADS (64 * NVH_MEL_WAVES)
#define NVH_MEL_MAX_BANDS 256
#define NVH_MEL_OUT_STRIDE (NVH_MEL_MAX_BANDS + 1)  // floats per frame of the workgroup's output tile (odd: band-major reads spread over the banks)
#define NVH_MEL_LDS_BYTES 81920  // a workgroup's LDS budget: two workgroups per CU (160 KB)

// Floats of one wavefront's transform slice: N/2 complex points at float2 slot c + 8 * (c >> 6), the padded layout of imdct_wave.h.
static inline constexpr int nvh_mel_slice_floats(int n_fft) { return 2 * ((n_fft >> 1) + (((n_fft >> 1) >> 6) << 3)); }
// float2 slots of the staged twiddles: pair k at slot k + (k >> 4), so that a pass's lanes, which read pairs a power of two
// apart, spread over the banks.
static inline constexpr int nvh_mel_tw_pad(int k) { return k + (k >> 4); }
static inline constexpr int nvh_mel_tw_slots(int n_fft) { return nvh_mel_tw_pad(n_fft >> 1) + 1; }
// The workgroup's LDS in floats: the four slices, the output tile, then (staged tables) the twiddles, the band records, the
// sparse weights, the window and the source span of the four frames.
static inline constexpr int nvh_mel_fixed_floats(int n_fft) { return NVH_MEL_WAVES * nvh_mel_slice_floats(n_fft) + NVH_MEL_WAVES * NVH_MEL_OUT_STRIDE; }

struct NvhMelArgs {
  const float* tw;    // [N/2 + 1] (cos, sin) pairs
  const float* win;   // [W]
  const float* fbw;   // the sparse bank's weights, band after band
  const int* band;    // [B][3]: first bin, bin count, offset of the band's weights in fbw
  const float* src;
  float* dst;
  const long long* valid;  // one per row (the per-row block, one upload), or null: src_length
  long long src_length, first, frames;
  long long src_row_stride, src_time_stride, src_chan_stride;
  long long dst_row_stride, dst_chan_stride, dst_frame_stride, dst_band_stride;
  long long groups;  // ceil(frames / NVH_MEL_WAVES)
  long long total;   // rows * channels * groups: the workgroups' work items
  int channels;
  int n_fft, ld;     // N = 1 << ld
  int win_length, hop, n_mels;
  int scale;
  float floor;
  int weights;       // floats of fbw
  int span;          // floats of the four frames' source span in LDS (3 * hop + W), 0: every frame reads the row through L2
  int band_fast;     // the band stride is the smaller one: a frame's bands are stored side by side, else a band's four frames
  // the front (nvh_mel_front), read by the FRONT instances of the kernel only; it takes no LDS of its own: the mean lives in
  // registers, so the staged layout above and the launcher's route choice are the same with and without it
  int reflect;       // NVH_PAD_REFLECT: a sample time outside [0, src_length) is mirrored once
  int remove_dc;
  float preemphasis; // p, 0: none
  float gain;        // g, 1: none
};

// The launch route of one call, from integers alone: what nvh_mel_rows[_front] launches and nvh_mel_route reports.
struct NvhMelRoute {
  int staged;        // twiddles, band records, weights, window and the four frames' span lie in LDS beside the slices and the tile
  int span;          // NvhMelArgs::span
  int lds_bytes;
  long long blocks;  // workgroups: each walks items b, b + blocks, ..
};
// Everything is staged where it fits the budget.  A workgroup stages the tables once and walks its items: several items each once
// there are workgroups enough to fill the chip.  weights: floats of the sparse bank; total_items: NvhMelArgs::total.
static inline constexpr NvhMelRoute nvh_mel_route_for(int n_fft, int win_length, int hop, int n_mels, int weights, long long total_items) {
  const long long span = (long long)(NVH_MEL_WAVES - 1) * hop + win_length;
  const long long fixed = nvh_mel_fixed_floats(n_fft);
  const long long staged = fixed + 2 * nvh_mel_tw_slots(n_fft) + 3 * n_mels + weights + win_length + span;
  const bool fits = staged * 4 <= NVH_MEL_LDS_BYTES;
  const long long blocks = total_items >= 16384 ? (total_items + 3) / 4 : total_items;
  return {fits ? 1 : 0, fits ? (int)span : 0, (int)((fits ? staged : fixed) * 4), blocks < (1 << 20) ? blocks : (1 << 20)};
}
// Which instance runs.  Windows and triangles change the tables alone, so such a front runs nvh_mel_rows' own instances; the
// FRONT instances run where the kernel itself has something to do.  (Today's front, and no front, have nothing of it.)
static inline constexpr bool nvh_mel_front_in_kernel(bool reflect, bool remove_dc, float preemphasis, float gain) {
  return reflect || remove_dc || preemphasis > 0.0f || gain != 1.0f;
}
static_assert(nvh_mel_route_for(4096, 4096, 5000, 128, 0, 7).staged == 0 && nvh_mel_route_for(4096, 4096, 5000, 128, 0, 7).lds_bytes == 4 * (4 * 4608 + 4 * 257), "n_fft = 4096");
static_assert(nvh_mel_route_for(512, 400, 160, 80, 1000, 20000).staged == 1 && nvh_mel_route_for(512, 400, 160, 80, 1000, 20000).span == 880, "Whisper's frames");
static_assert(nvh_mel_route_for(512, 400, 160, 80, 1000, 20000).blocks == 5000 && nvh_mel_route_for(512, 400, 160, 80, 1000, 1000).blocks == 1000, "four items each");
static_assert(!nvh_mel_front_in_kernel(false, false, 0.0f, 1.0f) && nvh_mel_front_in_kernel(false, false, 0.97f, 1.0f), "");
// (known cases away from the thresholds: tests/test_row_routes.py walks the thresholds' edges through nvh_mel_route's export)

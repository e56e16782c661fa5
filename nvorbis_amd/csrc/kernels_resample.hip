// kernels_resample.hip -- k_resample_rows: rows of f32 samples to another sample rate by a polyphase filter (include/nvorbis_hip.h
// states the rule under nvh_resample_rows; nvh_resample.hip builds the tap table and launches).
//
// A workgroup owns one (row, channel) and walks tiles of NVH_RS_TILE consecutive outputs of it (blockIdx.y, gridDim.y apart), two
// outputs per lane.  Per tile it stages the source span the tile's outputs read -- ((start + t0) * M) div L - half + 1 up to
// ((start + t_last) * M) div L + half, zeros where the span leaves the source row -- in LDS, and once per workgroup the tap table,
// its rows padded to an odd stride: lanes of one ds_read_b32 group read different phases, which then fall on different banks.  A
// table beyond NVH_RS_TAP_FLOATS is read through L2 instead, a span beyond NVH_RS_SRC_FLOATS (ratios beyond about 7 : 1) as well,
// with the row's bounds checked per tap.  Every output is the rule's serial chain -- acc = fl(acc + fl(x * h)) over the taps in
// order, one accumulator, the build has -ffp-contract=off -- and the throughput comes from the outputs in flight: two chains per
// lane, 256 lanes, two workgroups per CU at the full 80 KB of LDS.
#include <hip/hip_runtime.h>

#include "kernels_common.h"
#include "resample_dev.h"

#define NVH_RS_OUTS (NVH_RS_TILE / NVH_RS_THREADS)

// The chains of one lane.  TAPS_LDS / SRC_LDS: where taps and samples are read from.  `tap`: the lane's phases' rows (row stride
// folded in); `at`: per output the index of x[c - half + 1] -- in the staged span, or in the source row (bounds checked per tap).
template <bool TAPS_LDS, bool SRC_LDS>
__device__ __forceinline__ void resample_chains(const float* __restrict__ taps, const float* __restrict__ l_src,
                                                const float* __restrict__ src, long long src_time_stride, long long src_length,
                                                const int (&tap)[NVH_RS_OUTS], const long long (&at)[NVH_RS_OUTS], int ntaps,
                                                float (&acc)[NVH_RS_OUTS]) {
#pragma unroll
  for (int o = 0; o < NVH_RS_OUTS; ++o) acc[o] = 0.0f;
  for (int k = 0; k < ntaps; ++k) {
#pragma unroll
    for (int o = 0; o < NVH_RS_OUTS; ++o) {
      const float h = taps[tap[o] + k];
      float x;
      if (SRC_LDS) {
        x = l_src[(int)at[o] + k];
      } else {
        const long long s = at[o] + k;
        x = (s >= 0 && s < src_length) ? src[s * src_time_stride] : 0.0f;
      }
      const float prod = x * h;
      acc[o] = acc[o] + prod;
    }
  }
}

template <typename PCM>
__global__ void __launch_bounds__(NVH_RS_THREADS) k_resample_rows(NvhResampleArgs A) {
  extern __shared__ float rs_lds[];
  const int tid = (int)threadIdx.x;
  const long long row = (long long)blockIdx.x;
  const int ch = (int)blockIdx.z;
  const int ntaps = 2 * A.half;
  const int tstride = A.taps_in_lds ? (ntaps | 1) : ntaps;
  float* l_taps = rs_lds;
  float* l_src = rs_lds + (A.taps_in_lds ? A.L * tstride : 0);
  const long long valid = A.valid[row], start = A.start[row], origin = A.origin[row];
  const long long drow = A.dst_row ? (long long)A.dst_row[row] : row;
  PCM* __restrict__ dst = static_cast<PCM*>(A.dst) + drow * A.dst_row_stride + (long long)ch * A.dst_chan_stride;
  const float* __restrict__ src = A.src + row * A.src_row_stride + (long long)ch * A.src_chan_stride;
  const float* taps = A.taps_in_lds ? l_taps : A.taps;
  const long long L = A.L, M = A.M;
  bool taps_staged = false;
  int clipped = 0;

  for (long long tile = blockIdx.y; tile < A.tiles; tile += gridDim.y) {
    const long long t0 = tile * NVH_RS_TILE;
    const long long tend = t0 + NVH_RS_TILE < A.length ? t0 + NVH_RS_TILE : A.length;
    const long long vend = tend < valid ? tend : valid;  // outputs [t0, vend) are the clip's, [max(t0, vend), tend) the pad
    if (vend > t0) {                                     // (uniform over the workgroup)
      if (A.taps_in_lds && !taps_staged) {
        for (int i = tid; i < A.L * ntaps; i += NVH_RS_THREADS) {
          const int p = i / ntaps;
          l_taps[p * tstride + (i - p * ntaps)] = A.taps[i];
        }
        taps_staged = true;
      }
      const long long c_lo = ((start + t0) * M) / L - A.half + 1;  // the first source sample the tile reads ... (64-bit J * M)
      const long long c_hi = ((start + vend - 1) * M) / L + A.half;  // ... and the last
      const long long span = c_hi - c_lo + 1;
      const bool src_lds = span <= NVH_RS_SRC_FLOATS;
      __syncthreads();  // the tile before is done with the span
      if (src_lds) {
        for (int e = tid; e < (int)span; e += NVH_RS_THREADS) {
          const long long s = c_lo + e - origin;
          l_src[e] = (s >= 0 && s < A.src_length) ? src[s * A.src_time_stride] : 0.0f;
        }
      }
      __syncthreads();
      int tap[NVH_RS_OUTS];
      long long at[NVH_RS_OUTS];
#pragma unroll
      for (int o = 0; o < NVH_RS_OUTS; ++o) {
        const long long t = t0 + tid + o * NVH_RS_THREADS;
        const long long n = (start + (t < vend ? t : t0)) * M;  // (a lane without an output runs the tile's first one, unused)
        const long long c = n / L;
        tap[o] = (int)(n - c * L) * tstride;
        at[o] = c - A.half + 1 - (src_lds ? c_lo : origin);
      }
      float acc[NVH_RS_OUTS];
      if (A.taps_in_lds) {
        if (src_lds) resample_chains<true, true>(taps, l_src, src, A.src_time_stride, A.src_length, tap, at, ntaps, acc);
        else resample_chains<true, false>(taps, l_src, src, A.src_time_stride, A.src_length, tap, at, ntaps, acc);
      } else {
        if (src_lds) resample_chains<false, true>(taps, l_src, src, A.src_time_stride, A.src_length, tap, at, ntaps, acc);
        else resample_chains<false, false>(taps, l_src, src, A.src_time_stride, A.src_length, tap, at, ntaps, acc);
      }
#pragma unroll
      for (int o = 0; o < NVH_RS_OUTS; ++o) {
        const long long t = t0 + tid + o * NVH_RS_THREADS;
        if (t < vend) pcm_store1(dst + t * A.dst_time_stride, clip_value(acc[o], &clipped));
      }
    }
    for (long long t = (vend > t0 ? vend : t0) + tid; t < tend; t += NVH_RS_THREADS) pcm_store1(dst + t * A.dst_time_stride, 0.0f);
  }
  if (A.clipped) report_clipped(clipped, A.clipped + drow);
}

template __global__ void k_resample_rows<float>(NvhResampleArgs);
template __global__ void k_resample_rows<int16_t>(NvhResampleArgs);

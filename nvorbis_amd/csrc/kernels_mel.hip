// kernels_mel.hip -- k_mel_rows: log-mel features of rows of f32 samples (include/nvorbis_hip.h states the rule under nvh_mel_rows;
// nvh_mel.hip builds the tables and launches).
//
// A wavefront owns a frame, a workgroup of four wavefronts four consecutive frames of one (row, channel); a workgroup walks its
// work items (row, channel, frame group) gridDim.x apart.  A frame's life, all of it in the wavefront's own LDS slice (N/2 complex
// points in the padded layout of imdct_wave.h), so that the wavefront's program order is the only synchronisation inside it:
//   window    u = x * win, packed as z[n] = (u[2n], u[2n+1]) and stored at the bit-reversed index
//   transform the radix-2 decimation-in-time stages half = 1 .. N/4, up to three per register pass (a lane holds the 8 points
//             base + S k and runs the stages half = S, 2S, 4S on them; two per pass below N = 1024, where three would leave
//             lanes without a set), the rule's arithmetic per butterfly
//   split     the pair (k, N/2 - k) per lane: P[k] and P[N/2 - k] overwrite the real parts of Z[k] and Z[N/2 - k] (P[N/2] the
//             imaginary part of Z[0]): P never leaves LDS
//   mel       bands on lanes, one serial chain over the band's bins each; the scale; the value into the workgroup's output tile
// then the workgroup stores the tile: a frame's bands side by side where the band stride is the smaller one, else a band's four
// frames side by side (the tile is the transpose).  STAGED: the twiddles (in padded slots: a pass's lanes read pairs a power of two
// apart), the sparse bank (first bin, bin count, weights' offset per band -- never the dense table), the window and the source span
// the four frames share (3 H + W samples, zeros outside [0, valid)) lie in LDS, staged once per workgroup resp. per work item;
// otherwise (N = 4096, or a hop far beyond the window: the slices leave no room) they are read through L2.
// FRONT (the front of nvh_mel_front, stated under it in the header): the span staging also mirrors a sample time outside the row
// and applies the gain, the frame's wavefront sums its mean as the rule's sum64 (partial l in lane l, the halvings across lanes),
// and the window step reads s[n] and s[n-1], subtracts the mean from both and pre-emphasises.  No LDS of its own.
// Every operation of the rule is one f32 instruction: the build has -ffp-contract=off, and nothing here calls fmaf or a library
// logarithm.
#include <hip/hip_runtime.h>

#include "imdct_wave.h"
#include "mel_dev.h"

namespace {

// One register pass over R radix-2 stages whose smallest distance is S complex points (half = S, 2S, .., S << (R - 1)).
// tws = (N/2) / S: the twiddle step of the stage half = S (tw[j * N / (2 half)] with N / (2 half) = (N/2) / half).
// TWL: the twiddles are the staged ones, in their padded slots.
template <int R, bool TWL>
__device__ __forceinline__ void mel_pass(float2* __restrict__ l2, const float2* __restrict__ tw, int points, int S, int tws, int lane) {
  constexpr int K = 1 << R;
  const int nsets = points >> R;
#pragma unroll 1
  for (int s = lane; s < nsets; s += 64) {
    const int r = s & (S - 1);
    const int base = ((s - r) << R) + r;
    float2 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = l2[phys(base + S * k)];
#pragma unroll
    for (int t = 0; t < R; ++t) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (k & (1 << t)) continue;
        const int lo = k, hi = k | (1 << t);
        const int j = r + S * (lo & ((1 << t) - 1));  // a's index inside its group of 2 * half
        const int at = j * (tws >> t);
        const float2 cs = tw[TWL ? nvh_mel_tw_pad(at) : at];
        const float2 a = v[lo], b = v[hi];
        const float p0 = b.x * cs.x, p1 = b.y * cs.y, p2 = b.y * cs.x, p3 = b.x * cs.y;
        const float tr = p0 + p1;
        const float ti = p2 - p3;
        v[lo] = make_float2(a.x + tr, a.y + ti);
        v[hi] = make_float2(a.x - tr, a.y - ti);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) l2[phys(base + S * k)] = v[k];
  }
}

// P[k] of the split: a = Z[k mod N/2], b = conj(Z[(N/2 - k) mod N/2]) (already conjugated here), (c, s) = tw[k]
__device__ __forceinline__ float mel_power(float2 a, float2 b, float2 cs) {
  const float er = a.x + b.x, ei = a.y + b.y, dr = a.x - b.x, di = a.y - b.y;
  const float q0 = cs.x * di, q1 = cs.y * dr, q2 = cs.x * dr, q3 = cs.y * di;
  const float tr = q0 - q1;
  const float ti = -(q2 + q3);
  const float xr = er + tr, xi = ei + ti;
  const float rr = xr * xr, ii = xi * xi;
  return 0.25f * (rr + ii);
}

// the rule's logarithm
__device__ __forceinline__ float mel_ln(float v) {
  const unsigned bits = __float_as_uint(v);
  int e = (int)(bits >> 23) - 126;
  float g = __uint_as_float((bits & 0x007fffffu) | 0x3f000000u);  // v = g * 2^e, g in [0.5, 1)
  if (g < 0.70710678f) {
    g = g + g;
    e -= 1;
  }
  const float num = g - 1.0f, den = g + 1.0f;
  const float s = num / den;
  const float z = s * s;
  float p = (float)(1.0 / 11.0);
  p = p * z;
  p = p + (float)(1.0 / 9.0);
  p = p * z;
  p = p + (float)(1.0 / 7.0);
  p = p * z;
  p = p + (float)(1.0 / 5.0);
  p = p * z;
  p = p + (float)(1.0 / 3.0);
  p = p * z;
  p = p + 1.0f;
  const float hi = (float)e * (float)0.6931471805599453;
  const float s2 = s + s;
  const float lo = s2 * p;
  return hi + lo;
}

// s of the front's rule at sample time t of the row: the reflection (one is enough for every frame of the call: the launcher has
// checked it; a dead frame of the last group may map outside the row and reads 0), the zeroing at and behind `valid`, the gain
__device__ __forceinline__ float front_sample(const NvhMelArgs& A, const float* __restrict__ src, long long valid, long long t) {
  if (A.reflect) {
    if (t < 0) t = -t;
    else if (t >= A.src_length) t = 2 * (A.src_length - 1) - t;
  }
  float x = (t >= 0 && t < valid) ? src[t * A.src_time_stride] : 0.0f;
  if (A.gain != 1.0f) x = x * A.gain;
  return x;
}

// the frame's mean by the rule's sum64: partial l in lane l over the elements l, l + 64, .. in rising order, the six halvings
// (lane l < d takes p[l + d]), the division in lane 0's value; every lane returns it
template <bool STAGED>
__device__ __forceinline__ float front_mean(const NvhMelArgs& A, const float* __restrict__ span, const float* __restrict__ src,
                                            long long valid, long long t_frame, int W, int lane) {
  float p = 0.0f;
#pragma unroll 1
  for (int e = lane; e < W; e += 64) p = p + (STAGED ? span[e] : front_sample(A, src, valid, t_frame + e));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) p = p + __shfl_down(p, d, 64);
  return __shfl(p / (float)W, 0, 64);
}

}  // namespace

// FRONT: the front of nvh_mel_front (reflection, gain, DC removal, pre-emphasis) between the row and the window; the instances
// without it are nvh_mel_rows' own and read none of the front's arguments.
template <bool STAGED, bool FRONT>
__global__ void __launch_bounds__(NVH_MEL_THREADS) k_mel_rows(NvhMelArgs A) {
  extern __shared__ float mel_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = A.n_fft, points = N >> 1, W = A.win_length, B = A.n_mels;
  const int slice = nvh_mel_slice_floats(N);
  float* my = mel_lds + wave * slice;
  float2* my2 = reinterpret_cast<float2*>(my);
  float* l_out = mel_lds + NVH_MEL_WAVES * slice;
  float2* l_tw = reinterpret_cast<float2*>(l_out + NVH_MEL_WAVES * NVH_MEL_OUT_STRIDE);  // (an even count of floats in front of it)
  int* l_band = reinterpret_cast<int*>(l_tw + nvh_mel_tw_slots(N));
  float* l_fbw = reinterpret_cast<float*>(l_band + 3 * B);
  float* l_win = l_fbw + A.weights;
  float* l_span = l_win + W;
  const float2* __restrict__ g_tw = reinterpret_cast<const float2*>(A.tw);
  const float2* tw = STAGED ? l_tw : g_tw;

  if (STAGED) {  // once per workgroup (the first barrier of the walk below stands between these stores and their readers)
    for (int i = tid; i <= points; i += NVH_MEL_THREADS) l_tw[nvh_mel_tw_pad(i)] = g_tw[i];
    for (int i = tid; i < 3 * B; i += NVH_MEL_THREADS) l_band[i] = A.band[i];
    for (int i = tid; i < A.weights; i += NVH_MEL_THREADS) l_fbw[i] = A.fbw[i];
    for (int i = tid; i < W; i += NVH_MEL_THREADS) l_win[i] = A.win[i];
  }
  const int pad = (N - W) >> 1;

  for (long long item = blockIdx.x; item < A.total; item += gridDim.x) {
    const long long group = item % A.groups, rc = item / A.groups;
    const int ch = (int)(rc % A.channels);
    const long long row = rc / A.channels;
    const long long f0 = group * NVH_MEL_WAVES, f = f0 + wave;
    const bool live = f < A.frames;
    long long valid = A.valid ? A.valid[row] : A.src_length;
    const float* __restrict__ src = A.src + row * A.src_row_stride + (long long)ch * A.src_chan_stride;
    const long long t_group = f0 * A.hop + A.first;  // the row's sample under window sample 0 of the group's first frame
    if (STAGED) {
      for (int e = tid; e < A.span; e += NVH_MEL_THREADS) {
        const long long t = t_group + e;
        if (FRONT) l_span[e] = front_sample(A, src, valid, t);
        else l_span[e] = (t >= 0 && t < valid) ? src[t * A.src_time_stride] : 0.0f;
      }
    }
    __syncthreads();  // the span (and, the first time, the tables) are staged; the item before is done with the output tile

    if (live) {
      // ---- window: z[n] = (u[2n], u[2n+1]) at the bit-reversed index ----
      const long long t_frame = t_group + (long long)wave * A.hop;
      float mean = 0.0f;
      if (FRONT && A.remove_dc) mean = front_mean<STAGED>(A, l_span + wave * A.hop, src, valid, t_frame, W, lane);
#pragma unroll 1
      for (int n = lane; n < points; n += 64) {
        float u[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int i = 2 * n + h - pad;  // the window sample
          float v = 0.0f;
          if (i >= 0 && i < W) {
            float x, w;
            if (FRONT) {  // x: s[i]; xp: s[i-1], recomputed (s[0] under window sample 0)
              const int ip = i > 0 ? i - 1 : 0;
              float xp;
              if (STAGED) {
                x = l_span[wave * A.hop + i];
                xp = l_span[wave * A.hop + ip];
                w = l_win[i];
              } else {
                x = front_sample(A, src, valid, t_frame + i);
                xp = front_sample(A, src, valid, t_frame + ip);
                w = A.win[i];
              }
              if (A.remove_dc) {
                x = x - mean;
                xp = xp - mean;
              }
              if (A.preemphasis > 0.0f) {
                const float q = A.preemphasis * xp;
                x = x - q;
              }
            } else if (STAGED) {
              x = l_span[wave * A.hop + i];
              w = l_win[i];
            } else {
              const long long t = t_frame + i;
              x = (t >= 0 && t < valid) ? src[t * A.src_time_stride] : 0.0f;
              w = A.win[i];
            }
            v = x * w;
          }
          u[h] = v;
        }
        const int rev = (int)(__brev((unsigned)n) >> (32 - (A.ld - 1)));
        my2[phys(rev)] = make_float2(u[0], u[1]);
      }
      wave_sync();

      // ---- transform: stages half = 1 .. N/4, three per pass where that leaves a set for every lane (N >= 1024), else two;
      // the remainder last (the grouping changes no operation) ----
      int S = 1, left = A.ld - 1;
      if (points >= 512) {
        while (left >= 3) {
          mel_pass<3, STAGED>(my2, tw, points, S, points / S, lane);
          wave_sync();
          S <<= 3;
          left -= 3;
        }
      }
      while (left >= 2) {
        mel_pass<2, STAGED>(my2, tw, points, S, points / S, lane);
        wave_sync();
        S <<= 2;
        left -= 2;
      }
      if (left == 1) {
        mel_pass<1, STAGED>(my2, tw, points, S, points / S, lane);
        wave_sync();
      }

      // ---- split and power, in place: P[k] -> Re Z[k] (k < N/2), P[N/2] -> Im Z[0] ----
#pragma unroll 1
      for (int k = lane; k <= (points >> 1); k += 64) {
        const int k2 = (points - k) & (points - 1);
        const float2 za = my2[phys(k)], zb = my2[phys(k2)];
        const float pa = mel_power(za, make_float2(zb.x, -zb.y), tw[STAGED ? nvh_mel_tw_pad(k) : k]);
        const float pb = mel_power(zb, make_float2(za.x, -za.y), tw[STAGED ? nvh_mel_tw_pad(points - k) : points - k]);
        if (k == 0) {
          my2[phys(0)] = make_float2(pa, pb);  // P[0], P[N/2]
        } else {
          my[2 * phys(k)] = pa;
          my[2 * phys(k2)] = pb;
        }
      }
      wave_sync();

      // ---- mel and scale: bands on lanes, one chain per band ----
#pragma unroll 1
      for (int b = lane; b < B; b += 64) {
        const int* rec = (STAGED ? l_band : A.band) + 3 * b;
        const int k0 = rec[0], count = rec[1];
        const float* wts = (STAGED ? l_fbw : A.fbw) + rec[2];
        float acc = 0.0f;
        for (int i = 0; i < count; ++i) {
          const int k = k0 + i;
          const float p = k < points ? my[2 * phys(k)] : my[1];
          const float prod = p * wts[i];
          acc = acc + prod;
        }
        if (A.scale != 0) {  // NVH_MEL_LN, NVH_MEL_DB
          acc = mel_ln(fmaxf(acc, A.floor));
          if (A.scale == 2) acc = acc * (float)(10.0 / 2.302585092994046);
        }
        l_out[wave * NVH_MEL_OUT_STRIDE + b] = acc;
      }
    }
    __syncthreads();  // the tile is whole

    // ---- store: the smaller of the two strides runs along the lanes ----
    const long long rest = A.frames - f0;
    const int nf = rest < NVH_MEL_WAVES ? (int)rest : NVH_MEL_WAVES;
    float* __restrict__ dst = A.dst + row * A.dst_row_stride + (long long)ch * A.dst_chan_stride + f0 * A.dst_frame_stride;
    if (A.band_fast) {
      for (int i = tid; i < nf * B; i += NVH_MEL_THREADS) {
        const int j = i / B, b = i - j * B;
        dst[j * A.dst_frame_stride + b * A.dst_band_stride] = l_out[j * NVH_MEL_OUT_STRIDE + b];
      }
    } else {
      for (int i = tid; i < NVH_MEL_WAVES * B; i += NVH_MEL_THREADS) {
        const int b = i >> 2, j = i & (NVH_MEL_WAVES - 1);
        if (j < nf) dst[j * A.dst_frame_stride + b * A.dst_band_stride] = l_out[j * NVH_MEL_OUT_STRIDE + b];
      }
    }
  }
}

template __global__ void k_mel_rows<true, false>(NvhMelArgs);
template __global__ void k_mel_rows<false, false>(NvhMelArgs);
template __global__ void k_mel_rows<true, true>(NvhMelArgs);
template __global__ void k_mel_rows<false, true>(NvhMelArgs);

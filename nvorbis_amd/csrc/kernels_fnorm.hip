// kernels_fnorm.hip -- k_fnorm_rows: per-row normalisation of features x[row, channel, frame, band] (include/nvorbis_hip.h states
// the rule under nvh_fnorm_rows; nvh_fnorm.hip checks the descriptor and launches).
//
// A workgroup of eight wavefronts owns one (row, channel) and walks its work items gridDim.x apart.  The rule's sum64 of a band is
// held the way the rule states it: partial p[l] in lane l of the wavefront that owns the band (or, over a source whose band stride
// is the smaller one, at p[b][l] in LDS, always added to by the same thread), the six halvings as cross-lane adds d = 32 .. 1.  The
// sums over all bands (NVH_FNORM_ALL) are one thread's serial chain over the bands' results.
//   RESIDENT   the counted frames are read once into LDS, band after band (pitch F | 1), in the order of the source's smaller
//              stride; every sum and the last pass read LDS.
//   otherwise  every sum reads the source again (L2 holds it): a wavefront per band where a band's frames lie side by side, the
//              LDS partials where a frame's bands do.  The last pass reads and writes element by element where source and
//              destination run the same way, else through a tile of 64 frames x B.
// The last pass is the only one that writes, in the order of the destination's smaller stride, so that dst == src with the same
// strides is the in-place form.  Every operation of the rule is one f32 instruction (-ffp-contract=off); division and square root
// are the compiler's correctly rounded ones.
#include <hip/hip_runtime.h>

#include "fnorm_dev.h"

namespace {

constexpr int T = NVH_FNORM_THREADS;
constexpr int TILE = NVH_FNORM_TILE;

// Element i = tid, tid + T, .. of an (outer, inner) block whose inner index runs fastest, without a division per element.
struct Walk {
  int out, in, d_out, d_in, inner;
  __device__ __forceinline__ Walk(int tid, int inner_) : inner(inner_) {
    out = tid / inner;
    in = tid - out * inner;
    d_out = T / inner;
    d_in = T - d_out * inner;
  }
  __device__ __forceinline__ void next() {
    out += d_out;
    in += d_in;
    if (in >= inner) {
      in -= inner;
      ++out;
    }
  }
};

// the six halvings of sum64: lane l < d takes p[l + d]; lane 0 ends with the rule's result
__device__ __forceinline__ float halve64(float p) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) p = p + __shfl_down(p, d, 64);
  return p;
}

// the rule's value of a counted element
__device__ __forceinline__ float fnorm_value(const NvhFnormArgs& A, float x, float mean, float sd, float t) {
  if (A.mode == 1) return x - mean;
  if (A.mode == 2) {
    const float d = x - mean;
    return d / sd;
  }
  if (A.mode == 3) {
    const float m = fmaxf(x, t);
    const float s = m + A.offset;
    return s * A.gain;
  }
  return x;
}

// sum64 per band over the counted frames of x (SQ: of fl(d d), d = fl(x - mean[b])) into l_out[b]
template <bool RESIDENT, bool SQ>
__device__ __forceinline__ void band_sums(const NvhFnormArgs& A, const float* __restrict__ src, float* l_data, const float* l_mean,
                                          float* l_out, int vf, int tid) {
  const int lane = tid & 63, wave = tid >> 6, B = A.bands;
  if (RESIDENT || !A.src_band_fast) {
    const int pitch = nvh_fnorm_band_pitch(A.frames);
    for (int b = wave; b < B; b += NVH_FNORM_WAVES) {
      const float mean = SQ ? l_mean[b] : 0.0f;
      const float* __restrict__ gb = src + (long long)b * A.src_band_stride;
      float p = 0.0f;
#pragma unroll 4
      for (int f = lane; f < vf; f += 64) {
        float x = RESIDENT ? l_data[b * pitch + f] : gb[(long long)f * A.src_frame_stride];
        if (SQ) {
          const float d = x - mean;
          x = d * d;
        }
        p = p + x;
      }
      p = halve64(p);
      if (lane == 0) l_out[b] = p;
    }
  } else {
    // a frame's bands lie side by side: partial p[b][l] at b * 65 + l; element e = fl * B + b of every tile belongs to thread
    // e mod T, so a partial has one owner from the zero to the last add and no barrier stands between the tiles
    for (Walk w(tid, B); w.out < TILE; w.next()) l_data[w.in * (TILE + 1) + w.out] = 0.0f;
    for (int f0 = 0; f0 < vf; f0 += TILE) {
      const int nf = vf - f0 < TILE ? vf - f0 : TILE;
      const float* __restrict__ g = src + (long long)f0 * A.src_frame_stride;
      for (Walk w(tid, B); w.out < nf; w.next()) {
        float x = g[(long long)w.out * A.src_frame_stride + (long long)w.in * A.src_band_stride];
        if (SQ) {
          const float d = x - l_mean[w.in];
          x = d * d;
        }
        float* p = l_data + w.in * (TILE + 1) + w.out;
        *p = *p + x;
      }
    }
    __syncthreads();
    for (int b = wave; b < B; b += NVH_FNORM_WAVES) {
      const float p = halve64(l_data[b * (TILE + 1) + lane]);
      if (lane == 0) l_out[b] = p;
    }
  }
}

// l_v[b] holds S_b: afterwards fl(S / fl32(n)) of the band's group (SD: sqrt(fl(that + eps))).  Ends behind a barrier.
template <bool SD>
__device__ __forceinline__ void group_stats(const NvhFnormArgs& A, float* l_v, float* l_red, int vf, int tid) {
  const int B = A.bands;
  __syncthreads();  // the bands' sums are whole
  float all = 0.0f;
  if (A.axis == 1) {
    if (tid == 0) {
      float acc = 0.0f;
      for (int b = 0; b < B; ++b) acc = acc + l_v[b];
      l_red[NVH_FNORM_WAVES] = acc;
    }
    __syncthreads();
    all = l_red[NVH_FNORM_WAVES];  // (the next chain writes it behind the barrier below)
  }
  const float n = A.axis == 1 ? (float)((long long)vf * B) : (float)vf;
  for (int b = tid; b < B; b += T) {
    float v = (A.axis == 1 ? all : l_v[b]) / n;
    if (SD) {
      v = v + A.eps;
      v = __builtin_sqrtf(v);
    }
    l_v[b] = v;
  }
  __syncthreads();
}

}  // namespace

template <bool RESIDENT>
__global__ void __launch_bounds__(NVH_FNORM_THREADS) k_fnorm_rows(NvhFnormArgs A) {
  extern __shared__ float fnorm_lds[];
  float* l_mean = fnorm_lds;
  float* l_sd = fnorm_lds + NVH_FNORM_MAX_BANDS;
  float* l_red = fnorm_lds + 2 * NVH_FNORM_MAX_BANDS;
  float* l_data = fnorm_lds + NVH_FNORM_FIXED_FLOATS;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F = A.frames, B = A.bands;
  const int pitch = nvh_fnorm_band_pitch(F);
  const long long sf = A.src_frame_stride, sb = A.src_band_stride, df = A.dst_frame_stride, db = A.dst_band_stride;

  for (long long item = blockIdx.x; item < A.total; item += gridDim.x) {
    const int ch = (int)(item % A.channels);
    const long long row = item / A.channels;
    const int vf = A.vf ? (int)A.vf[row] : F;
    const float* src = A.src + row * A.src_row_stride + (long long)ch * A.src_chan_stride;
    float* dst = A.dst + row * A.dst_row_stride + (long long)ch * A.dst_chan_stride;
    __syncthreads();  // the item before is done with the LDS

    // ---- the counted frames into LDS (RESIDENT), and their maximum ----
    float mx = -__builtin_inff();
    if (vf > 0 && (RESIDENT || A.mode == 3)) {
      if (A.src_band_fast) {
        for (Walk w(tid, B); w.out < vf; w.next()) {
          const float x = src[(long long)w.out * sf + (long long)w.in * sb];
          if (RESIDENT) l_data[w.in * pitch + w.out] = x;
          mx = fmaxf(mx, x);
        }
      } else {
        for (Walk w(tid, vf); w.out < B; w.next()) {
          const float x = src[(long long)w.in * sf + (long long)w.out * sb];
          if (RESIDENT) l_data[w.out * pitch + w.in] = x;
          mx = fmaxf(mx, x);
        }
      }
    }
    float t = 0.0f;
    if (A.mode == 3) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
      if (lane == 0) l_red[wave] = mx;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < NVH_FNORM_WAVES; ++w) mx = fmaxf(mx, l_red[w]);
      t = mx - A.range;
    }
    __syncthreads();  // the data is whole

    // ---- the statistics ----
    if (vf > 0 && (A.mode == 1 || A.mode == 2)) {
      band_sums<RESIDENT, false>(A, src, l_data, l_mean, l_mean, vf, tid);
      group_stats<false>(A, l_mean, l_red, vf, tid);
      if (A.mode == 2) {
        band_sums<RESIDENT, true>(A, src, l_data, l_mean, l_sd, vf, tid);
        group_stats<true>(A, l_sd, l_red, vf, tid);
      }
    }

    // ---- the last pass: every frame, in the order of the destination's smaller stride ----
    if (RESIDENT) {
      if (A.dst_band_fast) {
        for (Walk w(tid, B); w.out < F; w.next()) {
          const int f = w.out, b = w.in;
          dst[(long long)f * df + (long long)b * db] = f < vf ? fnorm_value(A, l_data[b * pitch + f], l_mean[b], l_sd[b], t) : A.pad_value;
        }
      } else {
        for (Walk w(tid, F); w.out < B; w.next()) {
          const int f = w.in, b = w.out;
          dst[(long long)f * df + (long long)b * db] = f < vf ? fnorm_value(A, l_data[b * pitch + f], l_mean[b], l_sd[b], t) : A.pad_value;
        }
      }
    } else if (A.src_band_fast == A.dst_band_fast) {
      // the same thread reads and writes an element: in place as well
      if (A.dst_band_fast) {
        for (Walk w(tid, B); w.out < F; w.next()) {
          const int f = w.out, b = w.in;
          float y = A.pad_value;
          if (f < vf) y = fnorm_value(A, src[(long long)f * sf + (long long)b * sb], l_mean[b], l_sd[b], t);
          dst[(long long)f * df + (long long)b * db] = y;
        }
      } else {
        for (Walk w(tid, F); w.out < B; w.next()) {
          const int f = w.in, b = w.out;
          float y = A.pad_value;
          if (f < vf) y = fnorm_value(A, src[(long long)f * sf + (long long)b * sb], l_mean[b], l_sd[b], t);
          dst[(long long)f * df + (long long)b * db] = y;
        }
      }
    } else {
      // one layout into the other: a tile of 64 frames x B, frame fl's band b at fl * (B | 1) + b
      const int tp = B | 1;
      for (int f0 = 0; f0 < F; f0 += TILE) {
        const int nf = F - f0 < TILE ? F - f0 : TILE;
        const int counted = vf - f0 < 0 ? 0 : (vf - f0 < nf ? vf - f0 : nf);
        const float* g = src + (long long)f0 * sf;
        float* o = dst + (long long)f0 * df;
        if (f0) __syncthreads();  // the tile before is written out
        if (counted > 0) {
          if (A.src_band_fast) {
            for (Walk w(tid, B); w.out < counted; w.next()) l_data[w.out * tp + w.in] = g[(long long)w.out * sf + (long long)w.in * sb];
          } else {
            for (Walk w(tid, counted); w.out < B; w.next()) l_data[w.in * tp + w.out] = g[(long long)w.in * sf + (long long)w.out * sb];
          }
        }
        __syncthreads();
        if (A.dst_band_fast) {
          for (Walk w(tid, B); w.out < nf; w.next()) {
            const int fl = w.out, b = w.in;
            o[(long long)fl * df + (long long)b * db] = fl < counted ? fnorm_value(A, l_data[fl * tp + b], l_mean[b], l_sd[b], t) : A.pad_value;
          }
        } else {
          for (Walk w(tid, nf); w.out < B; w.next()) {
            const int fl = w.in, b = w.out;
            o[(long long)fl * df + (long long)b * db] = fl < counted ? fnorm_value(A, l_data[fl * tp + b], l_mean[b], l_sd[b], t) : A.pad_value;
          }
        }
      }
    }
  }
}

template __global__ void k_fnorm_rows<true>(NvhFnormArgs);
template __global__ void k_fnorm_rows<false>(NvhFnormArgs);

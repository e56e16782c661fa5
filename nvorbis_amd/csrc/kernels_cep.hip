// kernels_cep.hip -- k_cep_rows: cepstra (a DCT-II over the bands, the lifter folded into its table) and delta / delta-delta
// columns of features x[row, channel, frame, band] (include/nvorbis_hip.h states the rule under nvh_cep_rows; nvh_cep.hip checks
// the descriptor, builds the tables and launches).
//
// A workgroup of four wavefronts takes work items gridDim.x apart: NVH_CEP_TILE consecutive frames of one (row, channel).
//   stage    the tile's frames and o * N halo frames on each side into LDS, slot s's bands at s * (B | 1): read in the order of
//            the source's smaller stride.  A halo slot holds its frame clamped into [0, vf - 1], as the rule clamps; a tile slot
//            holds its own frame whatever vf is (its statics are written).
//   cepstra  lanes along the slots of a block of four indices k, block behind block (a wavefront spans at most three blocks: the
//            slots are at least 24): per band one LDS read of x (conflict-free at the odd pitch) and one 16-byte read of
//            D[k .. k + 4)[b], one address per block -- from LDS (STAGED) or through the caches.  acc = acc + x * d with product
//            and sum rounded separately (-ffp-contract=off), b rising: the rule's chain.
//   write    every (frame, column) of the tile in the order of the destination's smaller stride: a static column is its cepstrum,
//            a delta column the rule's chain over the cepstra in LDS.
// Without a transform (NVH_CEP_NONE) the staged frames are the cepstra and the second step is left out.
#include <hip/hip_runtime.h>

#include "cep_dev.h"

namespace {

constexpr int T = NVH_CEP_THREADS;
constexpr int TILE = NVH_CEP_TILE;

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

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace

template <bool STAGED>
__global__ void __launch_bounds__(NVH_CEP_THREADS) k_cep_rows(NvhCepArgs A) {
  extern __shared__ float4 cep_lds[];
  float* l_sc = reinterpret_cast<float*>(cep_lds);
  const int tid = (int)threadIdx.x;
  const int F = A.frames, B = A.bands, K = A.ceps, N = A.window;
  const int halo = nvh_cep_halo(A.order, N), S = TILE + 2 * halo, Q = (1 + A.order) * K;
  const int kpad = nvh_cep_kpad(K), tabf = nvh_cep_table_floats(A.dct, B, K), units = kpad / NVH_CEP_KBLOCK * S;
  const int xp = B | 1, cp = A.dct ? (K | 1) : xp;
  float* l_tab = l_sc + NVH_CEP_SCALE_FLOATS;
  float* l_x = l_tab + (STAGED ? tabf : 0);
  float* l_c = A.dct ? l_x + S * xp : l_x;
  const float* __restrict__ tab = A.tab;
  const long long sf = A.src_frame_stride, sb = A.src_band_stride, df = A.dst_frame_stride, dq = A.dst_col_stride;

  // once per workgroup: the delta scales, and the table where it is staged (the first item's barrier stands behind them)
  if (tid < NVH_CEP_SCALE_FLOATS) l_sc[tid] = tab[tabf + tid];
  if (STAGED) {
    for (int i = tid; i < tabf; i += T) l_tab[i] = tab[i];
  }

  for (long long item = blockIdx.x; item < A.total; item += gridDim.x) {
    const long long rc = item / A.tiles;
    const int f0 = (int)(item - rc * A.tiles) * TILE;
    const int ch = (int)(rc % A.channels);
    const long long row = rc / A.channels;
    const int n = A.vf ? (int)A.vf[row] : F;
    const int last = n > 0 ? n - 1 : 0;        // (no counted frame: the halo reads frame 0, and nobody reads the halo)
    const int nf = F - f0 < TILE ? F - f0 : TILE;  // the tile's frames
    const float* __restrict__ src = A.src + row * A.src_row_stride + (long long)ch * A.src_chan_stride;
    float* __restrict__ dst = A.dst + row * A.dst_row_stride + (long long)ch * A.dst_chan_stride;
    __syncthreads();  // the item before is done with the LDS

    // ---- stage: slot s holds frame g = f0 - halo + s inside the tile, clamp(g, 0, n - 1) outside it (always a frame below F) ----
    if (A.src_band_fast) {
      for (Walk w(tid, B); w.out < S; w.next()) {
        const int t = w.out - halo;
        const int g = t >= 0 && t < nf ? f0 + t : clampi(f0 + t, 0, last);
        l_x[w.out * xp + w.in] = src[(long long)g * sf + (long long)w.in * sb];
      }
    } else {
      for (Walk w(tid, S); w.out < B; w.next()) {
        const int t = w.in - halo;
        const int g = t >= 0 && t < nf ? f0 + t : clampi(f0 + t, 0, last);
        l_x[w.in * xp + w.out] = src[(long long)g * sf + (long long)w.out * sb];
      }
    }
    __syncthreads();

    // ---- cepstra: c[s][k] = the chain over b of x[s][b] * D[k][b] ----
    if (A.dct) {
      // unit u = block * S + slot: the slots of a block of four indices side by side in the lanes, the blocks one behind the other
      for (int u = tid; u < units; u += T) {
        const int kb = u / S, s = u - kb * S, k0 = kb * NVH_CEP_KBLOCK;
        const float* xs = l_x + s * xp;
        float* cs = l_c + s * cp;
        const float4* __restrict__ d4 = reinterpret_cast<const float4*>((STAGED ? l_tab : tab) + k0);
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 4
        for (int b = 0; b < B; ++b) {
          const float4 d = d4[(b * kpad) >> 2];
          const float x = xs[b];
          a0 = a0 + x * d.x;
          a1 = a1 + x * d.y;
          a2 = a2 + x * d.z;
          a3 = a3 + x * d.w;
        }
        cs[k0] = a0;
        if (k0 + 1 < K) cs[k0 + 1] = a1;
        if (k0 + 2 < K) cs[k0 + 2] = a2;
        if (k0 + 3 < K) cs[k0 + 3] = a3;
      }
      __syncthreads();
    }

    // ---- write: statics, deltas, delta-deltas, in the order of the destination's smaller stride ----
    const int elems = nf * Q;
    Walk w(tid, A.dst_col_fast ? Q : nf);
    for (int e = tid; e < elems; e += T, w.next()) {
      const int fl = A.dst_col_fast ? w.out : w.in, q = A.dst_col_fast ? w.in : w.out;
      const int m = q >= 2 * K ? 2 : (q >= K ? 1 : 0), k = q - m * K, f = f0 + fl;
      float y = 0.0f;
      if (m == 0) {
        y = l_c[(fl + halo) * cp + k];
      } else if (f < n) {
        const int reach = m * N;
        const float* sc = l_sc + (m == 1 ? 0 : NVH_CEP_S2_AT) + reach;
        const float* ck = l_c + k;  // frame g's cepstrum in slot g - f0 + halo: within halo of fl + halo, as the clamp moves towards f
        for (int j = -reach; j <= reach; ++j) {
          const float s = sc[j];
          if (s != 0.0f) y = y + ck[(clampi(f + j, 0, n - 1) - f0 + halo) * cp] * s;
        }
      }
      dst[(long long)f * df + (long long)q * dq] = y;
    }
  }
}

template __global__ void k_cep_rows<true>(NvhCepArgs);
template __global__ void k_cep_rows<false>(NvhCepArgs);

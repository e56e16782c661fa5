// kernels_common.h -- device-side parameter blocks for the gfx950 synthesis kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifdef __HIPCC__
#include <type_traits>
#endif

#include "nvh_format.h"

// Pointers into the per-stream device arena that holds the setup (uploaded once).
struct NvhDevSetup {
  int32_t channels, block0, block1, nbooks;
  const float* vq;                // VQ lookup tables of every codebook
  const uint32_t* lattice;        // lattice pool (NvhDevBook::lat_off), lattice_words entries
  int32_t lattice_words;
  int32_t fused_tail_ok;          // <= 2 channels, Floor1 only, every mapping has <= 1 coupling step (k_spectrum's fused tail)
  const NvhDevBook* books;
  const NvhDevFloor* floors;
  const NvhDevResidue* residues;
  const NvhDevMapping* mappings;
  const uint8_t* coupling;        // (magnitude, angle) byte pairs
  const float* windows;           // window pool (Mode.cs:69-100)
  const int32_t* ipool;           // Floor0 Bark maps
  const float* fpool;             // Floor0 wdel maps
  const float* mdct_a[2];         // Mdct.cs:40-55 tables for block0 / block1
  const float* mdct_b[2];
  const float* mdct_c[2];
  const uint16_t* mdct_br[2];
  const float* mdct_tw[2];        // lane-ordered copies of _a for the wavefront IMDCT (host_setup.cpp)
  const uint32_t* recip;          // recip[d] = floor((2^32 - 1) / d) for 1 <= d <= block1 / 2 (segment lengths of a floor curve)
};

// One uploaded frame batch.
struct NvhDevBatch {
  const NvhFrame* frames;
  const NvhChan* chans;
  const NvhResPass* passes;
  const NvhResOp* ops;
  const uint16_t* op_link;        // per op: next op of the same partition/channel (host_parse.h FrameBatch::op_link)
  const uint16_t* entries;
  const uint16_t* posts;
  const float* coeffs;
  int32_t nframes, pad;
};

// LDS words of one per-channel floor scratch block of k_spectrum (kernels_spectrum.hip: FloorScratch)
#define NVH_SP_FLOOR_SCRATCH_WORDS 332

// Profiling aids of the spectrum kernels (per-workgroup phase timestamps, phases masked out one at a time) exist only in
// the debug build of the library (python -m nvorbis_amd.build --debug -> libnvorbis_hip_dbg.so, -DNVH_DEBUG); the release
// kernels take neither parameter, so nothing in the shipped .so can skip work.
#ifdef NVH_DEBUG
#define NVH_DBG_PARAMS , long long* dbg, int phase_mask
#define NVH_DBG_ARGS , dbg, phase_mask
#else
#define NVH_DBG_PARAMS
#define NVH_DBG_ARGS
#endif

// error word written by kernels when the reference would have thrown (index out of range)
enum { NVH_DEVERR_FLOOR1_Y = 1, NVH_DEVERR_FLOOR0_W = 2 };

// Arguments of the slab synthesis kernel (kernels_synth.hip).
// groups of four sample times per workgroup of k_ola_compact's LDS-interleaving path (more than two channels)
#define NVH_OLA_GW 64

struct NvhSynthArgs {
  const uint4* consts;      // inverse_dB_table (256 floats) followed by the lattice pool, const_vecs 16-byte units
  const uint4* slabs;       // nframes slabs at stride_vecs
  float* work;              // [frame][channel][block1] planes: receives the compact IMDCT output k_ola_compact reads
  int* err;                 // device error word
  const float* mdct_a[2];
  const float* mdct_b[2];
  const float* mdct_c[2];
  const float* mdct_tw[2];
  const int32_t* ipool;     // Floor0 Bark maps (NvhDevSetup::ipool)
  const float* vq;          // the VQ pool (NvhDevSetup::vq): books with an explicit table are gathered from it (kernels_synth.hip: table_value)
  const NvhFrame* frames;   // the batch's frame records (k_synth8_emit reads the overlaps' windows and output positions from them)
  int const_vecs, stride_vecs, cap_vecs;  // cap_vecs: largest slab of the batch
  int lds_vecs;             // the LDS slab area (>= cap_vecs; paired emission stages the neighbours' quarters over constants + slab)
  int channels, block1;
  int f0, fstep;            // workgroup b synthesises frame f0 + b * fstep (paired emission: odd frames, then even frames)
  int nframes;              // frames of the batch (frame groups: a group's frames beyond the batch's end are skipped)
  int xcd_map;              // frames in eight contiguous runs, one per XCD (kernels_synth.hip: synth_body)
  int walk_two;             // frame groups of two: bit 0 = the two frames' residue walks in one loop (kernels_synth.hip: residue_walk_two),
                            // bit 1 = steady groups take the lean body (synth_group_steady; only with bit 0)
  int prefetch_prev;        // paired emission, odd launch: workgroup b touches the slab of frame f - 1, which workgroup b of the even
                            // launch fetches next -- on the same XCD (workgroups go round the XCDs by index), so from that XCD's L2
  // paired emission (nvh_format.h: NVH_EMIT_*); pcm == nullptr: off, every frame leaves its plane for k_ola_compact
  float* pcm;               // (the _s16 twins: int16_t samples)
  const float* windows;
  int clip;
  int plane_stride;         // the _planar twins: samples between the channels' planes (time t of channel c at pcm + c * plane_stride + t).
                            // (The _mono twins write one plane and read no stride.)
                            // (In the padding in front of clipped_flag, not at the end: a larger struct moves the implicit kernel
                            // arguments behind it, which changes an s_load offset in every kernel that takes NvhSynthArgs.)
  int* clipped_flag;
  const float* carry;       // the carried tail this batch's first frame overlaps with (fully windowed), NVH_EMIT_SELF_CARRY
  float* carry_out;         // receives the last decoded block, fully windowed (NVH_EMIT_CARRY_OUT); nullptr: k_ola_compact writes it
};

// The layouts of PCM: every channel's sample of one time side by side, one plane per channel, or ONE plane that holds the mean of
// the channels (the mono down-mix: mono_mix below).
// (plain ints, not an enum: the layout is part of the k_ola_* kernels' signatures, and an unnamed type in a mangled name is quoted)
constexpr int NVH_LAYOUT_INTERLEAVED = 0, NVH_LAYOUT_PLANAR = 1, NVH_LAYOUT_MONO = 2;
// ... and the two layouts of a channel map (NvhChanMap below): OC output slots per sample time, slot j holding source channel
// map[j] -- interleaved (time t of slot j at pcm + t * OC + j) or one plane per slot (pcm + j * plane_stride + t).
constexpr int NVH_LAYOUT_INTERLEAVED_MAP = 3, NVH_LAYOUT_PLANAR_MAP = 4;
constexpr bool nvh_layout_mapped(int layout) { return layout == NVH_LAYOUT_INTERLEAVED_MAP || layout == NVH_LAYOUT_PLANAR_MAP; }
constexpr bool nvh_layout_planes(int layout) { return layout == NVH_LAYOUT_PLANAR || layout == NVH_LAYOUT_PLANAR_MAP; }

// A channel map as the mapped kernels take it: eight nibbles each way (a map is refused on streams of more than eight channels).
// fwd: nibble j = the source channel of output slot j (j < oc); inv: nibble c = the output slot of source channel c, 0xF = the map
// drops it.  It is an argument of the mapped forms alone (k_synth8_emit*_map: behind NvhSynthArgs; k_ola_*: the last one) and NOT
// a member of NvhSynthArgs: a larger struct moves the implicit kernel arguments of every kernel that takes it (see plane_stride).
struct NvhChanMap {
  uint32_t fwd, inv;
  int32_t oc;
};
// the k_ola_* planar mapped forms' last argument: the planes' stride and the map
struct NvhStrideMap {
  long long plane_stride;
  NvhChanMap map;
};

// The forms of PCM the emitting kernels write: M(sample type, layout, suffix of the kernels' names).  Every such kernel
// exists once per entry, written by its own file through this list and declared through it in nvh_internal.h; the host picks one
// by the same pair (nvh_launch.hip: with_pcm_twins), so one more form is one more entry here.
#define NVH_FOR_PCM_TWINS(M)                                                                                             \
  M(float, NVH_LAYOUT_INTERLEAVED, ) M(int16_t, NVH_LAYOUT_INTERLEAVED, _s16) M(float, NVH_LAYOUT_PLANAR, _planar)       \
  M(int16_t, NVH_LAYOUT_PLANAR, _s16_planar) M(float, NVH_LAYOUT_MONO, _mono) M(int16_t, NVH_LAYOUT_MONO, _s16_mono)
// The mapped forms, of the families that have them: k_synth8_emit (the steady path of three to eight channels) and the three
// k_ola_* templates.  The narrow families (k_synth_emit, k_synth_group2 / 4) have none: a mono or stereo stream with a map that is
// not the identity runs without paired emission (nvh_launch.hip).
#define NVH_FOR_PCM_MAP_TWINS(M)                                                                          \
  M(float, NVH_LAYOUT_INTERLEAVED_MAP, _map) M(int16_t, NVH_LAYOUT_INTERLEAVED_MAP, _s16_map)             \
  M(float, NVH_LAYOUT_PLANAR_MAP, _planar_map) M(int16_t, NVH_LAYOUT_PLANAR_MAP, _s16_planar_map)

#ifdef __HIPCC__
// The last argument of the k_ola_* kernels: the samples between the channels' planes, of the channel-planar forms only.  The
// interleaved and the mono forms take an empty struct in its place, which leaves their kernel-argument layout what it was without the argument
// (k_ola_compact reads the grid's shape from the implicit arguments behind it).
struct NvhNoStride {};
// The mapped forms take the map there (NvhChanMap), the planar mapped forms the stride and the map (NvhStrideMap).
template <int LAYOUT> using pcm_stride_t =
    std::conditional_t<LAYOUT == NVH_LAYOUT_PLANAR, long long,
    std::conditional_t<LAYOUT == NVH_LAYOUT_INTERLEAVED_MAP, NvhChanMap,
    std::conditional_t<LAYOUT == NVH_LAYOUT_PLANAR_MAP, NvhStrideMap, NvhNoStride>>>;
// the stride and the map out of that argument (0 / the empty map where the form has none)
__device__ __forceinline__ long long pcm_stride_of(long long s) { return s; }
__device__ __forceinline__ long long pcm_stride_of(const NvhStrideMap& s) { return s.plane_stride; }
__device__ __forceinline__ long long pcm_stride_of(const NvhChanMap&) { return 0; }
__device__ __forceinline__ long long pcm_stride_of(const NvhNoStride&) { return 0; }
__device__ __forceinline__ NvhChanMap pcm_map_of(const NvhChanMap& m) { return m; }
__device__ __forceinline__ NvhChanMap pcm_map_of(const NvhStrideMap& s) { return s.map; }
__device__ __forceinline__ NvhChanMap pcm_map_of(long long) { return NvhChanMap{0u, 0u, 0}; }
__device__ __forceinline__ NvhChanMap pcm_map_of(const NvhNoStride&) { return NvhChanMap{0u, 0u, 0}; }
// source channel of output slot j / output slot of source channel c (15: dropped)
__device__ __forceinline__ int map_src(uint32_t fwd, int j) { return (int)((fwd >> (4 * j)) & 15u); }
__device__ __forceinline__ int map_slot(uint32_t inv, int c) { return (int)((inv >> (4 * c)) & 15u); }

// PCM leaves the chip (a copy engine or the gather reads it next) and no kernel reads it again: streaming stores (`nt`), which do
// not displace what the kernels do re-read -- the odd frames' planes, the slabs the odd launch touched for the even one -- from
// the L2 / Infinity Cache.  Same box, three streams, working set past the Infinity Cache: 24.0 -> 22.2 us per 4096-frame pass.
__device__ __forceinline__ void pcm_store4(float4* p, float a, float b, float c, float d) {
  typedef float nvh_v4f __attribute__((ext_vector_type(4)));
  const nvh_v4f v = {a, b, c, d};
#ifdef NVH_PCM_POLICY
#define NVH_STR2(x) #x
#define NVH_STR(x) NVH_STR2(x)
  asm volatile("global_store_dwordx4 %0, %1, off " NVH_STR(NVH_PCM_POLICY) : : "v"(p), "v"(v) : "memory");
#else
  __builtin_nontemporal_store(v, reinterpret_cast<nvh_v4f*>(p));
#endif
}
__device__ __forceinline__ void pcm_store1(float* p, float v) { __builtin_nontemporal_store(v, p); }

// ---- 16-bit PCM (NVH_PCM_S16): the emitting kernels' twins (<name>_s16) are the same bodies instantiated with int16_t
// samples; only these helpers differ.  The rule is ov_read's: s16 = clamp(rint(x * 32768), -32768, 32767), on the float the
// float path would have stored (after the clip).  x * 32768 is exact; v_rndne_f32 rounds ties to even; v_cvt_i32_f32
// saturates out-of-range values and maps NaN to 0 -- written as asm because a C conversion of NaN is undefined (a float clamp
// in front of it would turn NaN into -32768).
__device__ __forceinline__ int pcm_s16_value(float x) {
  const float r = __builtin_rintf(x * 32768.0f);
  int i;
  asm("v_cvt_i32_f32 %0, %1" : "=v"(i) : "v"(r));
  return i < -32768 ? -32768 : (i > 32767 ? 32767 : i);
}
__device__ __forceinline__ unsigned pcm_s16_pair(float lo, float hi) {
  return ((unsigned)pcm_s16_value(lo) & 0xFFFFu) | ((unsigned)pcm_s16_value(hi) << 16);
}

// four consecutive 16-bit samples: what a float4 of float PCM becomes (8 bytes)
struct __attribute__((aligned(8))) nvh_s16x4 { int16_t v[4]; };
template <typename T> struct PcmVec4;
template <> struct PcmVec4<float> { typedef float4 type; };
template <> struct PcmVec4<int16_t> { typedef nvh_s16x4 type; };
template <typename T> using pcm4_t = typename PcmVec4<T>::type;

__device__ __forceinline__ void pcm_store4(nvh_s16x4* p, float a, float b, float c, float d) {
  typedef unsigned nvh_v2u __attribute__((ext_vector_type(2)));
  const nvh_v2u v = {pcm_s16_pair(a, b), pcm_s16_pair(c, d)};
#ifdef NVH_PCM_POLICY
  asm volatile("global_store_dwordx2 %0, %1, off " NVH_STR(NVH_PCM_POLICY) : : "v"(p), "v"(v) : "memory");
#else
  __builtin_nontemporal_store(v, reinterpret_cast<nvh_v2u*>(p));
#endif
}
__device__ __forceinline__ void pcm_store1(int16_t* p, float v) { __builtin_nontemporal_store((int16_t)pcm_s16_value(v), p); }
// Two groups of four stereo sample times (p[0], p[1]) from eight interleaved values -- two 16-byte stores of float PCM -- as one
// 16-byte store of 16-bit PCM where p is 16-byte aligned.  The vector paths only guarantee an element offset that is a multiple of 4
// (8 bytes of s16), so the other frames take two 8-byte stores (uniform per frame: p moves by 16 bytes per lane).  (The float
// kernels keep their own two calls of pcm_store4: through this helper their code comes out differently.)
__device__ __forceinline__ void pcm_store4x2(nvh_s16x4* p, const float (&v)[8]) {
  if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    typedef unsigned nvh_v4u __attribute__((ext_vector_type(4)));
    const nvh_v4u u = {pcm_s16_pair(v[0], v[1]), pcm_s16_pair(v[2], v[3]), pcm_s16_pair(v[4], v[5]), pcm_s16_pair(v[6], v[7])};
#ifdef NVH_PCM_POLICY
    asm volatile("global_store_dwordx4 %0, %1, off " NVH_STR(NVH_PCM_POLICY) : : "v"(p), "v"(u) : "memory");
#else
    __builtin_nontemporal_store(u, reinterpret_cast<nvh_v4u*>(p));
#endif
  } else {
    pcm_store4(p, v[0], v[1], v[2], v[3]);
    pcm_store4(p + 1, v[4], v[5], v[6], v[7]);
  }
}
// plain (not streaming) store of four 16-bit samples: synth_emit8_direct's partial-line stores, which the L2 merges
__device__ __forceinline__ void pcm_plain4(nvh_s16x4* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pcm_s16_pair(a, b), pcm_s16_pair(c, d));
}
// ---- channel-planar PCM (the _planar twins: sample time t of channel c at pcm + c * plane_stride + out_pos + t).  The narrow
// emission's lane computes four forward sample times i0 .. i0 + 3 (v) and four mirrored ones n/2 - 4 - i0 .. n/2 - 1 - i0 (u, already
// in time order) of one channel: they leave as one vector each (16 bytes of float, 8 of int16_t) as soon as the channel is done.
// `plane`: the frame's first sample in the channel's plane; g / gm: the two vectors' indices in units of four samples.
template <typename PCM>
__device__ __forceinline__ void pcm_store_plane(PCM* plane, long long g, long long gm, const float4& v, const float4& u) {
  pcm4_t<PCM>* p = reinterpret_cast<pcm4_t<PCM>*>(plane);
  pcm_store4(p + g, v.x, v.y, v.z, v.w);
  pcm_store4(p + gm, u.x, u.y, u.z, u.w);
}
// ... and the streaming load of 16 bytes that exactly one lane reads exactly once (a neighbour frame's quarter)
__device__ __forceinline__ float4 stream_load4(const float* p) {
  typedef float nvh_v4f __attribute__((ext_vector_type(4)));
  const nvh_v4f v = __builtin_nontemporal_load(reinterpret_cast<const nvh_v4f*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

// Utils.cs:30-43, without branches (two compares, two selects; the flag is an OR of the compare masks): the early-return form
// compiles to two exec-mask regions per sample.  A NaN compares false twice and passes through, as in the reference.
// `bit`: what a clamped sample ORs into the lane's flag.  A lane that emits for more than one frame gives each frame a bit of its
// own (report_clipped<NB>: bit k belongs to frame + k), so that the flag still costs one select and one OR per sample.
__device__ __forceinline__ float clip_value(float v, int* clipped, int bit = 1) {
  const bool hi = v > .99999994f, lo = v < -.99999994f;
  *clipped |= (hi | lo) ? bit : 0;
  return hi ? 0.99999994f : (lo ? -0.99999994f : v);
}

__device__ __forceinline__ void clip_value4(float4& v, int* clipped, int bit = 1) {
  v.x = clip_value(v.x, clipped, bit); v.y = clip_value(v.y, clipped, bit);
  v.z = clip_value(v.z, clipped, bit); v.w = clip_value(v.w, clipped, bit);
}

// ---- the symmetric overlap-add tail ------------------------------------------------------------------------------------------
// The steady state of a stream: a block whose whole first half overlaps the whole second half of a predecessor of the same size.
// Sample times i0 .. i0 + 3 (v) and n/2 - 4 - i0 .. n/2 - 1 - i0 (u, in time order) of the overlap need exactly a = the later
// block's first quarter and b = the earlier block's third quarter at i0 .. i0 + 3 (Mdct.cs:275-303: y[n/2-1-x] = -y[x],
// y[n-1-x] = y[n/2+x]), times the later block's window at i0 (wf) and n/2 - 4 - i0 (wm) and the earlier block's at n/2 + i0 (pf) and
// n - 4 - i0 (pm): Mode.cs:160-166 windows, StreamDecoder.cs:532-541 adds, as separately rounded products and sums in this order
// (the build has -ffp-contract=off; -a.w * wm.x is the product of the negated value, as the reference's mirrored read gives it).
// k_ola_compact's read-once forms (kernels.hip: ola_sym, ola_sym_lds, ola_sym_planar) share it.  The emitting synthesis kernels
// (kernels_synth.hip: synth_emit, synth_group_body, synth_emit8_direct) spell the same lines out in place: routed through a
// shared helper, k_synth_emit and the frame-group kernels come out with another register allocation (profiles/pcm_twins_isa.txt).
__device__ __forceinline__ void ola_sym_mul_add(const float4& a, const float4& b, const float4& wf, const float4& wm, const float4& pf,
                                                const float4& pm, float4& v, float4& u) {
  v = make_float4(a.x * wf.x, a.y * wf.y, a.z * wf.z, a.w * wf.w);
  const float4 tt = make_float4(b.x * pf.x, b.y * pf.y, b.z * pf.z, b.w * pf.w);
  v.x = v.x + tt.x; v.y = v.y + tt.y; v.z = v.z + tt.z; v.w = v.w + tt.w;
  u = make_float4(-a.w * wm.x, -a.z * wm.y, -a.y * wm.z, -a.x * wm.w);
  const float4 r = make_float4(b.w * pm.x, b.z * pm.y, b.y * pm.z, b.x * pm.w);
  u.x = u.x + r.x; u.y = u.y + r.y; u.z = u.z + r.z; u.w = u.w + r.w;
}

// Four consecutive positions idx0 .. idx0+3 of a block (idx0 a multiple of 4: a group never straddles a quarter) from its compact
// plane -- the two independent quarters y[0, n/4) and y[n/2, 3n/4) of the inverse MDCT, the others follow from
// y[n/2-1-x] = -y[x] and y[n-1-x] = y[n/2+x] (Mdct.cs:275-303); a channel that does not execute keeps its residue in
// [0, n/2) and zeros behind it (Mapping.cs:192-196) -- times the window (Mode.cs:160-166).
__device__ __forceinline__ float4 compact_value4(const float* __restrict__ plane, const float* __restrict__ w, int n,
                                                 int exec, int idx0) {
  const int n2 = n >> 1, n4 = n >> 2;
  float4 y;
  if (exec) {
    if (idx0 < n4 || (idx0 >= n2 && idx0 < n2 + n4)) {
      y = *reinterpret_cast<const float4*>(plane + idx0);
    } else if (idx0 < n2) {
      const float4 r = *reinterpret_cast<const float4*>(plane + (n2 - 4 - idx0));
      y = make_float4(-r.w, -r.z, -r.y, -r.x);
    } else {
      const float4 r = *reinterpret_cast<const float4*>(plane + (n + n2 - 4 - idx0));
      y = make_float4(r.w, r.z, r.y, r.x);
    }
  } else {
    y = idx0 < n2 ? *reinterpret_cast<const float4*>(plane + idx0) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float4 ww = *reinterpret_cast<const float4*>(w + idx0);
  return make_float4(y.x * ww.x, y.y * ww.y, y.z * ww.z, y.w * ww.w);
}

// ---- the mono down-mix (the _mono twins: one plane, sample time t at pcm + out_pos + t) --------------------------------------
// m = (((x_0 + x_1) + x_2) + ... + x_{C-1}) / (float)C on the channels' samples BEFORE ClipSamples' clip: C - 1 additions in
// channel order, each rounded once, then one correctly rounded division; the clip (and, for 16-bit PCM, pcm_s16_value) is applied
// once, to the mix.  The division is IEEE's: the build has neither fast-math nor a reciprocal flag, so `s / 3.0f` is the v_div_scale /
// v_div_fmas / v_div_fixup sequence, and for C a power of two the compiler's own x / C -> x * (1 / C) is exact.  The narrow
// kernels (at most two channels, k_synth_emit at its 64-VGPR cap) spell the stereo case out as a multiply by 0.5f.
__device__ __forceinline__ float mono_scale(float s, int nch) { return s / (float)nch; }
// the narrow emission's eight values per half (sample time k of channel c at v[2 k + c], nch <= 2) -> the four mixed sample times
__device__ __forceinline__ float4 mono_mix2(const float (&v)[8], int nch, int clip, int* clipped, int bit = 1) {
  float4 m = nch == 2 ? make_float4((v[0] + v[1]) * 0.5f, (v[2] + v[3]) * 0.5f, (v[4] + v[5]) * 0.5f, (v[6] + v[7]) * 0.5f)
                      : make_float4(v[0], v[2], v[4], v[6]);
  if (clip) clip_value4(m, clipped, bit);
  return m;
}
// CH channels per lane (sample time k of channel c at v[k * CH + c]) -> the four mixed sample times
template <int CH>
__device__ __forceinline__ float4 mono_mix(const float (&v)[4 * CH], int clip, int* clipped, int bit = 1) {
  float m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float s = v[k * CH];
#pragma unroll
    for (int c = 1; c < CH; ++c) s = s + v[k * CH + c];
    m[k] = s / (float)CH;
  }
  float4 r = make_float4(m[0], m[1], m[2], m[3]);
  if (clip) clip_value4(r, clipped, bit);
  return r;
}

// HasClipped (StreamDecoder.cs:728) is sticky: one lane per wavefront that clipped looks at the flag and only sets it
// while it is still clear.  A stream that clips everywhere (loud material; Floor0 curves on random bits) otherwise
// serialises one atomic per lane -- or still 8192 per launch with one per wavefront, ~35 us -- on a single address.
__device__ __forceinline__ void set_clipped_word(int* w) {
  if (__atomic_load_n(w, __ATOMIC_RELAXED) == 0) atomicOr(w, 1);
}
// (the stand-alone form: a flag word of the caller's, nothing behind it -- k_copy_buffer)
__device__ __forceinline__ void report_clipped(int clipped, int* __restrict__ clipped_flag) {
  const unsigned long long any = __ballot(clipped != 0);
  if (any && (int)(threadIdx.x & 63u) == __ffsll((long long)any) - 1) set_clipped_word(clipped_flag);
}
// The emitting kernels of a batch: `clipped_flag` is word 1 of the stream's flag block (nvh_internal.h: nvh_stream::flags), and
// words 2-3 of that block hold the device address of the batch's segment-flag table, or null (a batch of one segment, a resident
// batch: the sticky word alone, which is then that segment's flag).  The table is one int32 per frame -- the index, from the
// table's base, of the flag word of the segment the frame's PCM belongs to -- followed by those flag words, zeroed at upload.
// `frame` is uniform over the wavefront, and bit k of a lane's `clipped << shift` says that the lane clamped a sample of
// frame + k (`shift`: for a lane whose every sample belongs to one frame, known without a bit of its own; applied behind `any`).
// Everything new is behind `any`: a wavefront that did not clip executes what it executed before.  The segment words keep the
// sticky word's discipline (one lane per wavefront and frame, a load in front of the atomic).
template <int NB = 1>
__device__ __forceinline__ void report_clipped(int clipped, int* __restrict__ clipped_flag, int frame, int shift = 0) {
  const unsigned long long any = __ballot(clipped != 0);
  if (any) {
    const int lane = (int)(threadIdx.x & 63u);
    if (lane == __ffsll((long long)any) - 1) set_clipped_word(clipped_flag);
    int* tab = *reinterpret_cast<int* const*>(clipped_flag + 1);
    if (tab) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const unsigned long long m = NB == 1 ? any : __ballot((((clipped << shift) >> k) & 1) != 0);
        if (m && lane == __ffsll((long long)m) - 1) set_clipped_word(tab + tab[frame + k]);
      }
    }
  }
}
#endif

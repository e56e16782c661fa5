// nvh_fnorm.hip -- per-row normalisation of features (include/nvorbis_hip.h: nvh_fnorm_check / _rows): the descriptor's check, the
// upload of the per-row frame counts and the launch of k_fnorm_rows (kernels_fnorm.hip).
#include "nvh_internal.h"

namespace {

static_assert(NVH_FNORM_RESIDENT_FLOATS == NVH_FNORM_DATA_FLOATS, "the header states the resident path's limit");

bool finite32(float v) { return v >= -3.40282347e+38f && v <= 3.40282347e+38f; }  // (NaN fails both)

int fnorm_check(const nvh_fnorm_desc& D) {
  if (D.mode != NVH_FNORM_NONE && D.mode != NVH_FNORM_MEAN && D.mode != NVH_FNORM_MEAN_VAR && D.mode != NVH_FNORM_PEAK) return NVH_ERR_ARGUMENT;
  if (D.axis != NVH_FNORM_PER_BAND && D.axis != NVH_FNORM_ALL) return NVH_ERR_ARGUMENT;
  if (D.rows < 0 || D.channels < 1 || D.channels > 65535 || D.frames < 0 || D.frames > (1 << 24) || D.bands < 1 || D.bands > NVH_FNORM_MAX_BANDS)
    return NVH_ERR_ARGUMENT;
  if (!finite32(D.pad_value)) return NVH_ERR_ARGUMENT;
  if (D.mode == NVH_FNORM_MEAN_VAR && (!(D.eps >= 1.17549435e-38f) || !finite32(D.eps))) return NVH_ERR_ARGUMENT;
  if (D.mode == NVH_FNORM_PEAK && (!(D.range >= 0.0f) || !finite32(D.offset) || !finite32(D.gain))) return NVH_ERR_ARGUMENT;  // (+inf is a range)
  return NVH_OK;
}

long long magnitude(long long v) { return v < 0 ? -v : v; }

// Every check of nvh_fnorm_rows in front of its context's, in the header's order, and what the launch follows from.  io: the call
// has its buffers (nvh_fnorm_route has none and checks the descriptor alone).
struct FnormPrep {
  bool work = false;
  long long total = 0;  // rows * channels (the work items are counted in 64 bits)
  NvhFnormRoute route;
};
int fnorm_prepare(const nvh_fnorm_desc* desc, bool io, const int64_t* valid_frames, FnormPrep* out) {
  if (!desc) return NVH_ERR_ARGUMENT;
  const nvh_fnorm_desc& D = *desc;
  const int rc = fnorm_check(D);
  if (rc != NVH_OK) return rc;
  out->work = D.rows > 0 && D.frames > 0;
  if (out->work && !io) return NVH_ERR_ARGUMENT;
  for (int i = 0; valid_frames && i < D.rows; ++i) {
    if (valid_frames[i] < 0 || valid_frames[i] > D.frames) return NVH_ERR_ARGUMENT;
  }
  out->total = (long long)D.rows * D.channels;
  out->route = nvh_fnorm_route_for(D.frames, D.bands, out->total);
  return NVH_OK;
}

}  // namespace

extern "C" int nvh_fnorm_route(const nvh_fnorm_desc* desc, int64_t* out) {
  return nvh_guard([&]() -> int {
    if (!out) return NVH_ERR_ARGUMENT;
    FnormPrep P;
    const int rc = fnorm_prepare(desc, true, nullptr, &P);
    if (rc != NVH_OK) return rc;
    const int64_t v[3] = {P.route.resident, P.route.lds_bytes, P.route.blocks};
    std::copy(v, v + 3, out);
    return NVH_OK;
  });
}

extern "C" int nvh_fnorm_check(const nvh_fnorm_desc* desc) {
  return nvh_guard([&]() -> int { return desc ? fnorm_check(*desc) : NVH_ERR_ARGUMENT; });
}

extern "C" int nvh_fnorm_rows(nvh_ctx* c, const nvh_fnorm_desc* desc, const float* d_src, float* d_dst, const int64_t* valid_frames) {
  return nvh_guard([&]() -> int {
    FnormPrep P;
    int rc = fnorm_prepare(desc, d_src && d_dst, valid_frames, &P);
    if (rc != NVH_OK) return rc;
    if (!c) return NVH_ERR_NO_GPU;
    if (!P.work) return NVH_OK;
    const nvh_fnorm_desc& D = *desc;
    HIP_TRY(hipSetDevice(c->device));
    rc = lds_opt_in(c->fnorm_lds_attr_set, NVH_FNORM_LDS_BYTES, {(const void*)k_fnorm_rows<true>, (const void*)k_fnorm_rows<false>});
    if (rc != NVH_OK) return rc;
    NvhFnormArgs A{};
    if (valid_frames) {  // the per-row block: the rows' counted frames
      const size_t bytes = (size_t)D.rows * sizeof(int64_t);
      void* image = nullptr;
      const void* d_block = nullptr;
      rc = c->fnorm_rows.begin(c, bytes, &image);
      if (rc != NVH_OK) return rc;
      std::memcpy(image, valid_frames, bytes);
      rc = c->fnorm_rows.send(c, bytes, &d_block);
      if (rc != NVH_OK) return rc;
      A.vf = static_cast<const long long*>(d_block);
    }
    A.src = d_src;
    A.dst = d_dst;
    A.src_row_stride = D.src_row_stride;
    A.src_chan_stride = D.src_chan_stride;
    A.src_frame_stride = D.src_frame_stride;
    A.src_band_stride = D.src_band_stride;
    A.dst_row_stride = D.dst_row_stride;
    A.dst_chan_stride = D.dst_chan_stride;
    A.dst_frame_stride = D.dst_frame_stride;
    A.dst_band_stride = D.dst_band_stride;
    A.total = P.total;
    A.channels = D.channels;
    A.frames = D.frames;
    A.bands = D.bands;
    A.mode = D.mode;
    A.axis = D.axis;
    A.eps = D.eps;
    A.pad_value = D.pad_value;
    A.range = D.range;
    A.offset = D.offset;
    A.gain = D.gain;
    A.src_band_fast = magnitude(D.src_band_stride) <= magnitude(D.src_frame_stride) ? 1 : 0;
    A.dst_band_fast = magnitude(D.dst_band_stride) <= magnitude(D.dst_frame_stride) ? 1 : 0;
    // a (row, channel) that fits the budget is read once and normalised out of LDS; a larger one re-reads its source
    const dim3 grid((unsigned)P.route.blocks), block(NVH_FNORM_THREADS);
    const size_t lds = (size_t)P.route.lds_bytes;
    if (P.route.resident) hipLaunchKernelGGL(k_fnorm_rows<true>, grid, block, lds, c->stream, A);
    else hipLaunchKernelGGL(k_fnorm_rows<false>, grid, block, lds, c->stream, A);
    HIP_TRY(hipGetLastError());
    return NVH_OK;
  });
}

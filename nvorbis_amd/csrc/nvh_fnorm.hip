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

}  // namespace

extern "C" int nvh_fnorm_check(const nvh_fnorm_desc* desc) {
  return nvh_guard([&]() -> int { return desc ? fnorm_check(*desc) : NVH_ERR_ARGUMENT; });
}

extern "C" int nvh_fnorm_rows(nvh_ctx* c, const nvh_fnorm_desc* desc, const float* d_src, float* d_dst, const int64_t* valid_frames) {
  return nvh_guard([&]() -> int {
    if (!desc) return NVH_ERR_ARGUMENT;
    const nvh_fnorm_desc& D = *desc;
    int rc = fnorm_check(D);
    if (rc != NVH_OK) return rc;
    const bool work = D.rows > 0 && D.frames > 0;
    if (work && (!d_src || !d_dst)) return NVH_ERR_ARGUMENT;
    for (int i = 0; valid_frames && i < D.rows; ++i) {
      if (valid_frames[i] < 0 || valid_frames[i] > D.frames) return NVH_ERR_ARGUMENT;
    }
    if (!c) return NVH_ERR_NO_GPU;
    if (!work) return NVH_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->fnorm_lds_attr_set) {
      HIP_TRY(hipFuncSetAttribute((const void*)k_fnorm_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize, NVH_FNORM_LDS_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)k_fnorm_rows<false>, hipFuncAttributeMaxDynamicSharedMemorySize, NVH_FNORM_LDS_BYTES));
      c->fnorm_lds_attr_set = true;
    }
    NvhFnormArgs A{};
    if (valid_frames) {
      // the per-row block, one copy out of page-locked memory; the block of the call before may still be on its way: its copy
      // is waited for (the kernel behind it is not) before the staging is written again
      const size_t bytes = (size_t)D.rows * sizeof(int64_t);
      if (!c->fnorm_copied) HIP_TRY(hipEventCreateWithFlags(&c->fnorm_copied, hipEventDisableTiming));
      else HIP_TRY(hipEventSynchronize(c->fnorm_copied));
      c->fnorm_rows_host.host = true;
      c->fnorm_rows_host.pool = &c->hpool;
      c->fnorm_rows_dev.pool = &c->pool;
      rc = c->fnorm_rows_host.reserve(bytes);
      if (rc == NVH_OK) rc = c->fnorm_rows_dev.reserve(bytes);
      if (rc != NVH_OK) return rc;
      std::memcpy(c->fnorm_rows_host.p, valid_frames, bytes);
      HIP_TRY(hipMemcpyAsync(c->fnorm_rows_dev.p, c->fnorm_rows_host.p, bytes, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipEventRecord(c->fnorm_copied, c->stream));
      A.vf = static_cast<const long long*>(c->fnorm_rows_dev.p);
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
    A.total = (long long)D.rows * D.channels;  // (the work items are counted in 64 bits)
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
    const bool resident = nvh_fnorm_resident(D.frames, D.bands);
    const size_t data = resident ? (size_t)nvh_fnorm_band_pitch(D.frames) * D.bands : (size_t)nvh_fnorm_reread_floats(D.bands);
    const size_t lds = (NVH_FNORM_FIXED_FLOATS + data) * sizeof(float);
    const long long blocks = std::min<long long>(A.total, NVH_FNORM_MAX_BLOCKS);
    const dim3 grid((unsigned)blocks), block(NVH_FNORM_THREADS);
    if (resident) hipLaunchKernelGGL(k_fnorm_rows<true>, grid, block, lds, c->stream, A);
    else hipLaunchKernelGGL(k_fnorm_rows<false>, grid, block, lds, c->stream, A);
    HIP_TRY(hipGetLastError());
    return NVH_OK;
  });
}

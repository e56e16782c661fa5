// nvh_mel.hip -- log-mel features of rows (include/nvorbis_hip.h: nvh_mel_plan / _tables / _rows): the parameter check, the tables
// in double on the host, the per-context cache of device tables, and the launch of k_mel_rows (kernels_mel.hip).
#include <cmath>

#include "nvh_internal.h"

namespace {

constexpr double kPi = 3.14159265358979323846;

// The rule's parameters (everything the three calls share); *ld = log2(n_fft).
int mel_check(const nvh_mel_desc& D, int* ld) {
  if (D.rate < 1 || D.n_fft < 64 || D.n_fft > 4096 || (D.n_fft & (D.n_fft - 1))) return NVH_ERR_ARGUMENT;
  if (D.win_length < 1 || D.win_length > D.n_fft || D.hop < 1 || D.hop > 65536 || D.n_mels < 1 || D.n_mels > NVH_MEL_MAX_BANDS) return NVH_ERR_ARGUMENT;
  if (!(D.f_min >= 0.0) || !(D.f_min < D.f_max) || !(D.f_max <= (double)D.rate / 2.0)) return NVH_ERR_ARGUMENT;  // (NaN fails each)
  if ((D.mel_scale != NVH_MEL_HTK && D.mel_scale != NVH_MEL_SLANEY) || (D.norm != NVH_MEL_NORM_NONE && D.norm != NVH_MEL_NORM_SLANEY))
    return NVH_ERR_ARGUMENT;
  if (D.scale != NVH_MEL_POWER && D.scale != NVH_MEL_LN && D.scale != NVH_MEL_DB) return NVH_ERR_ARGUMENT;
  if (!(D.floor >= 1.17549435e-38f) || !(D.floor <= 3.40282347e+38f)) return NVH_ERR_ARGUMENT;
  constexpr int64_t kMaxFrames = (int64_t)1 << 40, kMaxFirst = (int64_t)1 << 60;  // f * hop + first stays inside 64 bits
  if (D.frames < 0 || D.frames > kMaxFrames || D.first > kMaxFirst || D.first < -kMaxFirst) return NVH_ERR_ARGUMENT;
  int l = 0;
  while ((1 << l) < D.n_fft) ++l;
  *ld = l;
  return NVH_OK;
}

double hz_to_mel(double f, int scale) {
  if (scale == NVH_MEL_HTK) return 2595.0 * std::log10(1.0 + f / 700.0);
  if (f < 1000.0) return 3.0 * f / 200.0;
  return 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0);
}

double mel_to_hz(double m, int scale) {
  if (scale == NVH_MEL_HTK) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
  if (m < 15.0) return 200.0 * m / 3.0;
  return 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0));
}

void mel_twiddles(const nvh_mel_desc& D, float* tw) {
  for (int k = 0; k <= D.n_fft / 2; ++k) {
    const double a = 2.0 * kPi * (double)k / (double)D.n_fft;
    tw[2 * k] = (float)std::cos(a);
    tw[2 * k + 1] = (float)std::sin(a);
  }
}

void mel_window(const nvh_mel_desc& D, float* win) {
  for (int n = 0; n < D.win_length; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * (double)n / (double)D.win_length));
}

// the dense bank, [B][N/2 + 1]
void mel_bank(const nvh_mel_desc& D, float* fb) {
  const int bins = D.n_fft / 2 + 1, B = D.n_mels;
  const double m_lo = hz_to_mel(D.f_min, D.mel_scale), m_hi = hz_to_mel(D.f_max, D.mel_scale);
  std::vector<double> pt((size_t)B + 2);
  for (int i = 0; i < B + 2; ++i) pt[(size_t)i] = mel_to_hz(m_lo + (m_hi - m_lo) * (double)i / (double)(B + 1), D.mel_scale);
  for (int b = 0; b < B; ++b) {
    const double l = pt[(size_t)b], c = pt[(size_t)b + 1], r = pt[(size_t)b + 2];
    for (int k = 0; k < bins; ++k) {
      const double f = (double)k * (double)D.rate / (double)D.n_fft;
      const double up = (f - l) / (c - l), down = (r - f) / (r - c);
      double v = up < down ? up : down;
      if (!(v > 0.0)) v = 0.0;
      if (D.norm == NVH_MEL_NORM_SLANEY) v *= 2.0 / (r - l);
      fb[(size_t)b * bins + k] = (float)v;
    }
  }
}

int upload(void** dst, const void* src, size_t bytes) {
  HIP_TRY(hipMalloc(dst, bytes ? bytes : 4));
  if (!bytes) return NVH_OK;
  const hipError_t e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    g_last_hip_error = (int)e;
    return NVH_ERR_DEVICE;
  }
  return NVH_OK;
}

int get_mel(nvh_ctx* c, const nvh_mel_desc& D, MelDev** out) {
  const MelKey key(D.rate, D.n_fft, D.win_length, D.n_mels, D.mel_scale, D.norm, D.f_min, D.f_max);
  auto it = c->mel_cache.find(key);
  if (it != c->mel_cache.end()) {
    *out = &it->second;
    return NVH_OK;
  }
  const int bins = D.n_fft / 2 + 1, B = D.n_mels;
  std::vector<float> tw((size_t)2 * bins), win((size_t)D.win_length), fb((size_t)B * bins), wts;
  mel_twiddles(D, tw.data());
  mel_window(D, win.data());
  mel_bank(D, fb.data());
  // the sparse bank: per band its first non-zero bin, the bins up to its last non-zero one, and where their weights begin
  std::vector<int> band((size_t)3 * B);
  for (int b = 0; b < B; ++b) {
    const float* rowp = fb.data() + (size_t)b * bins;
    int k0 = 0, k1 = bins;
    while (k0 < bins && rowp[k0] == 0.0f) ++k0;
    while (k1 > k0 && rowp[k1 - 1] == 0.0f) --k1;
    band[(size_t)3 * b] = k0 < bins ? k0 : 0;
    band[(size_t)3 * b + 1] = k1 - k0;
    band[(size_t)3 * b + 2] = (int)wts.size();
    wts.insert(wts.end(), rowp + k0, rowp + k1);
  }
  MelDev d;
  d.weights = (int)wts.size();
  int rc = upload((void**)&d.tw, tw.data(), tw.size() * sizeof(float));
  if (rc == NVH_OK) rc = upload((void**)&d.win, win.data(), win.size() * sizeof(float));
  if (rc == NVH_OK) rc = upload((void**)&d.fbw, wts.data(), wts.size() * sizeof(float));
  if (rc == NVH_OK) rc = upload((void**)&d.band, band.data(), band.size() * sizeof(int));
  if (rc != NVH_OK) {
    (void)hipFree(d.tw);
    (void)hipFree(d.win);
    (void)hipFree(d.fbw);
    (void)hipFree(d.band);
    return rc;
  }
  auto ins = c->mel_cache.emplace(key, d);
  *out = &ins.first->second;
  return NVH_OK;
}

}  // namespace

extern "C" int nvh_mel_plan(const nvh_mel_desc* desc, int64_t* twiddle_count, int64_t* window_count, int64_t* bank_count) {
  return nvh_guard([&]() -> int {
    if (!desc || !twiddle_count || !window_count || !bank_count) return NVH_ERR_ARGUMENT;
    int ld = 0;
    const int rc = mel_check(*desc, &ld);
    if (rc != NVH_OK) return rc;
    const int64_t bins = desc->n_fft / 2 + 1;
    *twiddle_count = 2 * bins;
    *window_count = desc->win_length;
    *bank_count = (int64_t)desc->n_mels * bins;
    return NVH_OK;
  });
}

extern "C" int nvh_mel_tables(const nvh_mel_desc* desc, float* twiddle, float* window, float* bank, int64_t twiddle_cap,
                              int64_t window_cap, int64_t bank_cap, int64_t* twiddle_count, int64_t* window_count, int64_t* bank_count) {
  return nvh_guard([&]() -> int {
    if (twiddle_cap < 0 || window_cap < 0 || bank_cap < 0 || (twiddle_cap > 0 && !twiddle) || (window_cap > 0 && !window) || (bank_cap > 0 && !bank))
      return NVH_ERR_ARGUMENT;
    const int rc = nvh_mel_plan(desc, twiddle_count, window_count, bank_count);
    if (rc != NVH_OK) return rc;
    if ((twiddle && *twiddle_count > twiddle_cap) || (window && *window_count > window_cap) || (bank && *bank_count > bank_cap)) return NVH_ERR_ARGUMENT;
    if (twiddle) mel_twiddles(*desc, twiddle);
    if (window) mel_window(*desc, window);
    if (bank) mel_bank(*desc, bank);
    return NVH_OK;
  });
}

extern "C" int nvh_mel_rows(nvh_ctx* c, const nvh_mel_desc* desc, const float* d_src, float* d_dst, const int64_t* valid) {
  return nvh_guard([&]() -> int {
    if (!desc) return NVH_ERR_ARGUMENT;
    const nvh_mel_desc& D = *desc;
    int ld = 0;
    int rc = mel_check(D, &ld);
    if (rc != NVH_OK) return rc;
    if (D.rows < 0 || D.src_length < 0 || D.channels < 1 || D.channels > 65535) return NVH_ERR_ARGUMENT;
    const bool work = D.rows > 0 && D.frames > 0;
    if (work && (!d_src || !d_dst)) return NVH_ERR_ARGUMENT;
    for (int i = 0; valid && i < D.rows; ++i) {
      if (valid[i] < 0 || valid[i] > D.src_length) return NVH_ERR_ARGUMENT;
    }
    const int64_t groups = (D.frames + NVH_MEL_WAVES - 1) / NVH_MEL_WAVES;
    if (work && (int64_t)D.rows * D.channels > INT64_MAX / groups) return NVH_ERR_ARGUMENT;  // (the work items are counted in 64 bits)
    if (!c) return NVH_ERR_NO_GPU;
    if (!work) return NVH_OK;
    HIP_TRY(hipSetDevice(c->device));
    MelDev* tab = nullptr;
    rc = get_mel(c, D, &tab);
    if (rc != NVH_OK) return rc;
    if (!c->mel_lds_attr_set) {
      HIP_TRY(hipFuncSetAttribute((const void*)k_mel_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize, NVH_MEL_LDS_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)k_mel_rows<false>, hipFuncAttributeMaxDynamicSharedMemorySize, NVH_MEL_LDS_BYTES));
      c->mel_lds_attr_set = true;
    }
    NvhMelArgs A{};
    if (valid) {
      // the per-row block, one copy out of page-locked memory; the block of the call before may still be on its way: its copy
      // is waited for (the kernel behind it is not) before the staging is written again
      const size_t bytes = (size_t)D.rows * sizeof(int64_t);
      if (!c->mel_copied) HIP_TRY(hipEventCreateWithFlags(&c->mel_copied, hipEventDisableTiming));
      else HIP_TRY(hipEventSynchronize(c->mel_copied));
      c->mel_rows_host.host = true;
      c->mel_rows_host.pool = &c->hpool;
      c->mel_rows_dev.pool = &c->pool;
      rc = c->mel_rows_host.reserve(bytes);
      if (rc == NVH_OK) rc = c->mel_rows_dev.reserve(bytes);
      if (rc != NVH_OK) return rc;
      std::memcpy(c->mel_rows_host.p, valid, bytes);
      HIP_TRY(hipMemcpyAsync(c->mel_rows_dev.p, c->mel_rows_host.p, bytes, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipEventRecord(c->mel_copied, c->stream));
      A.valid = static_cast<const long long*>(c->mel_rows_dev.p);
    }
    A.tw = tab->tw;
    A.win = tab->win;
    A.fbw = tab->fbw;
    A.band = tab->band;
    A.src = d_src;
    A.dst = d_dst;
    A.src_length = D.src_length;
    A.first = D.first;
    A.frames = D.frames;
    A.src_row_stride = D.src_row_stride;
    A.src_time_stride = D.src_time_stride;
    A.src_chan_stride = D.src_chan_stride;
    A.dst_row_stride = D.dst_row_stride;
    A.dst_chan_stride = D.dst_chan_stride;
    A.dst_frame_stride = D.dst_frame_stride;
    A.dst_band_stride = D.dst_band_stride;
    A.groups = groups;
    A.total = (long long)D.rows * D.channels * groups;
    A.channels = D.channels;
    A.n_fft = D.n_fft;
    A.ld = ld;
    A.win_length = D.win_length;
    A.hop = D.hop;
    A.n_mels = D.n_mels;
    A.scale = D.scale;
    A.floor = D.floor;
    A.weights = tab->weights;
    const long long abs_f = D.dst_frame_stride < 0 ? -D.dst_frame_stride : D.dst_frame_stride;
    const long long abs_b = D.dst_band_stride < 0 ? -D.dst_band_stride : D.dst_band_stride;
    A.band_fast = abs_b <= abs_f ? 1 : 0;
    // everything staged -- twiddles, band records, weights, window, the four frames' span -- where it fits beside the slices and
    // the tile
    const long long span = (long long)(NVH_MEL_WAVES - 1) * D.hop + D.win_length;
    const long long staged = (long long)nvh_mel_fixed_floats(D.n_fft) + 2 * nvh_mel_tw_slots(D.n_fft) + 3 * D.n_mels + tab->weights + D.win_length + span;
    const bool fits = staged * (long long)sizeof(float) <= NVH_MEL_LDS_BYTES;
    A.span = fits ? (int)span : 0;
    const size_t lds = (size_t)(fits ? staged : nvh_mel_fixed_floats(D.n_fft)) * sizeof(float);
    // a workgroup stages the tables once and walks its items: several items each once there are workgroups enough to fill the chip
    long long blocks = A.total;
    if (blocks >= 16384) blocks = (blocks + 3) / 4;
    blocks = std::min<long long>(blocks, 1 << 20);
    const dim3 grid((unsigned)blocks), block(NVH_MEL_THREADS);
    if (fits) hipLaunchKernelGGL(k_mel_rows<true>, grid, block, lds, c->stream, A);
    else hipLaunchKernelGGL(k_mel_rows<false>, grid, block, lds, c->stream, A);
    HIP_TRY(hipGetLastError());
    return NVH_OK;
  });
}

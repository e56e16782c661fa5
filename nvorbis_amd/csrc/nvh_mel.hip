// nvh_mel.hip -- log-mel features of rows (include/nvorbis_hip.h: nvh_mel_plan / _tables / _rows and their _front forms): the
// parameter check, the tables in double on the host, the per-context cache of device tables, and the launch of k_mel_rows
// (kernels_mel.hip).
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

// The front's fields (nvh_mel_front) and, under NVH_PAD_REFLECT, that one reflection is enough for every frame of D.
int front_check(const nvh_mel_desc& D, const nvh_mel_front& Fr) {
  if (Fr.window < NVH_WIN_HANN || Fr.window > NVH_WIN_RECT || (Fr.triangles != NVH_TRI_HZ && Fr.triangles != NVH_TRI_MEL)) return NVH_ERR_ARGUMENT;
  if ((Fr.pad_mode != NVH_PAD_ZERO && Fr.pad_mode != NVH_PAD_REFLECT) || (Fr.remove_dc != 0 && Fr.remove_dc != 1)) return NVH_ERR_ARGUMENT;
  if (!(Fr.preemphasis >= 0.0f) || !(Fr.preemphasis <= 1.0f)) return NVH_ERR_ARGUMENT;  // (NaN fails each)
  if (!(Fr.gain > 0.0f) || !(Fr.gain <= 3.40282347e+38f)) return NVH_ERR_ARGUMENT;
  if (Fr.reserved[0] != 0 || Fr.reserved[1] != 0) return NVH_ERR_ARGUMENT;
  if (Fr.pad_mode == NVH_PAD_REFLECT && D.frames > 0) {  // (mel_check has bounded frames, hop and first: no overflow below)
    const int64_t L = D.src_length;
    if (L < 2 || -D.first > L - 1) return NVH_ERR_ARGUMENT;
    const int64_t last = (D.frames - 1) * D.hop + D.first + D.win_length - 1;  // below 2^61
    if (L - 1 < ((int64_t)1 << 61) && last > 2 * (L - 1)) return NVH_ERR_ARGUMENT;
  }
  return NVH_OK;
}

void mel_window(const nvh_mel_desc& D, int kind, float* win) {
  const int W = D.win_length;
  const double den = kind == NVH_WIN_HANN ? (double)W : (W > 1 ? (double)(W - 1) : 1.0);
  for (int n = 0; n < W; ++n) {
    const double c = std::cos(2.0 * kPi * (double)n / den);
    double v = 0.5 - 0.5 * c;  // NVH_WIN_HANN (periodic), NVH_WIN_HANN_SYM
    if (kind == NVH_WIN_HAMMING) v = 0.54 - 0.46 * c;
    else if (kind == NVH_WIN_POVEY) v = std::pow(v, 0.85);
    else if (kind == NVH_WIN_RECT) v = 1.0;
    win[n] = (float)v;
  }
}

// the dense bank, [B][N/2 + 1]; triangles linear in Hz (NVH_TRI_HZ) or in mel (NVH_TRI_MEL)
void mel_bank(const nvh_mel_desc& D, int triangles, float* fb) {
  const int bins = D.n_fft / 2 + 1, B = D.n_mels;
  const double m_lo = hz_to_mel(D.f_min, D.mel_scale), m_hi = hz_to_mel(D.f_max, D.mel_scale);
  std::vector<double> pt((size_t)B + 2), hz((size_t)B + 2);
  for (int i = 0; i < B + 2; ++i) {
    const double m = m_lo + (m_hi - m_lo) * (double)i / (double)(B + 1);
    hz[(size_t)i] = mel_to_hz(m, D.mel_scale);
    pt[(size_t)i] = triangles == NVH_TRI_MEL ? m : hz[(size_t)i];
  }
  for (int b = 0; b < B; ++b) {
    const double l = pt[(size_t)b], c = pt[(size_t)b + 1], r = pt[(size_t)b + 2];
    for (int k = 0; k < bins; ++k) {
      double f = (double)k * (double)D.rate / (double)D.n_fft;
      if (triangles == NVH_TRI_MEL) f = hz_to_mel(f, D.mel_scale);
      const double up = (f - l) / (c - l), down = (r - f) / (r - c);
      double v = up < down ? up : down;
      if (!(v > 0.0)) v = 0.0;
      if (D.norm == NVH_MEL_NORM_SLANEY) v *= 2.0 / (hz[(size_t)b + 2] - hz[(size_t)b]);
      fb[(size_t)b * bins + k] = (float)v;
    }
  }
}

// What k_mel_rows reads of one parameter set, on the host: twiddles, window, and the sparse bank -- per band its first non-zero
// bin, the bins up to its last non-zero one, and where their weights begin.  wts.size() is the `weights` of the route.
struct MelTables {
  std::vector<float> tw, win, wts;
  std::vector<int> band;
};

MelTables mel_build(const nvh_mel_desc& D, int window, int triangles) {
  const int bins = D.n_fft / 2 + 1, B = D.n_mels;
  MelTables t;
  t.tw.resize((size_t)2 * bins);
  t.win.resize((size_t)D.win_length);
  t.band.resize((size_t)3 * B);
  std::vector<float> fb((size_t)B * bins);
  mel_twiddles(D, t.tw.data());
  mel_window(D, window, t.win.data());
  mel_bank(D, triangles, fb.data());
  for (int b = 0; b < B; ++b) {
    const float* rowp = fb.data() + (size_t)b * bins;
    int k0 = 0, k1 = bins;
    while (k0 < bins && rowp[k0] == 0.0f) ++k0;
    while (k1 > k0 && rowp[k1 - 1] == 0.0f) --k1;
    t.band[(size_t)3 * b] = k0 < bins ? k0 : 0;
    t.band[(size_t)3 * b + 1] = k1 - k0;
    t.band[(size_t)3 * b + 2] = (int)t.wts.size();
    t.wts.insert(t.wts.end(), rowp + k0, rowp + k1);
  }
  return t;
}

int get_mel(nvh_ctx* c, const nvh_mel_desc& D, int window, int triangles, MelDev** out) {
  const MelKey key(D.rate, D.n_fft, D.win_length, D.n_mels, D.mel_scale, D.norm, D.f_min, D.f_max, window, triangles);
  auto it = c->mel_cache.find(key);
  if (it != c->mel_cache.end()) {
    *out = &it->second;
    return NVH_OK;
  }
  const MelTables t = mel_build(D, window, triangles);
  MelDev d;
  d.weights = (int)t.wts.size();
  int rc = upload_table(&d.tw, t.tw);
  if (rc == NVH_OK) rc = upload_table(&d.win, t.win);
  if (rc == NVH_OK) rc = upload_table(&d.fbw, t.wts);  // (a bank of zeros alone is an empty table)
  if (rc == NVH_OK) rc = upload_table(&d.band, t.band);
  if (rc != NVH_OK) {
    d.free_tables();
    return rc;
  }
  auto ins = c->mel_cache.emplace(key, d);
  *out = &ins.first->second;
  return NVH_OK;
}

// Every check of nvh_mel_rows[_front] in front of its context's, in the header's order, and what the launch follows from.  The
// route itself waits for the sparse bank's size (route()): the cached tables have it, nvh_mel_route builds the bank for it.
// io: the call has its buffers (nvh_mel_route has none and checks the descriptors alone).
struct MelPrep {
  int ld = 0, window = NVH_WIN_HANN, triangles = NVH_TRI_HZ;
  bool work = false, front_in_kernel = false;
  long long groups = 0, total = 0;
  NvhMelRoute route(const nvh_mel_desc& D, int weights) const { return nvh_mel_route_for(D.n_fft, D.win_length, D.hop, D.n_mels, weights, total); }
};
int mel_prepare(const nvh_mel_desc* desc, const nvh_mel_front* front, bool io, const int64_t* valid, MelPrep* out) {
  if (!desc) return NVH_ERR_ARGUMENT;
  const nvh_mel_desc& D = *desc;
  int rc = mel_check(D, &out->ld);
  if (rc == NVH_OK && front) rc = front_check(D, *front);
  if (rc != NVH_OK) return rc;
  if (front) {
    out->window = front->window;
    out->triangles = front->triangles;
    out->front_in_kernel = nvh_mel_front_in_kernel(front->pad_mode == NVH_PAD_REFLECT, front->remove_dc != 0, front->preemphasis, front->gain);
  }
  if (D.rows < 0 || D.src_length < 0 || D.channels < 1 || D.channels > 65535) return NVH_ERR_ARGUMENT;
  out->work = D.rows > 0 && D.frames > 0;
  if (out->work && !io) return NVH_ERR_ARGUMENT;
  for (int i = 0; valid && i < D.rows; ++i) {
    if (valid[i] < 0 || valid[i] > D.src_length) return NVH_ERR_ARGUMENT;
  }
  out->groups = (D.frames + NVH_MEL_WAVES - 1) / NVH_MEL_WAVES;
  if (out->work && (int64_t)D.rows * D.channels > INT64_MAX / out->groups) return NVH_ERR_ARGUMENT;  // (the work items are counted in 64 bits)
  out->total = out->work ? (long long)D.rows * D.channels * out->groups : 0;
  return NVH_OK;
}

}  // namespace

extern "C" int nvh_mel_route(const nvh_mel_desc* desc, const nvh_mel_front* front, int64_t* out) {
  return nvh_guard([&]() -> int {
    if (!out) return NVH_ERR_ARGUMENT;
    MelPrep P;
    const int rc = mel_prepare(desc, front, true, nullptr, &P);
    if (rc != NVH_OK) return rc;
    const int64_t weights = (int64_t)mel_build(*desc, P.window, P.triangles).wts.size();
    const NvhMelRoute r = P.route(*desc, (int)weights);
    const int64_t v[6] = {r.staged, r.span, r.lds_bytes, r.blocks, P.front_in_kernel ? 1 : 0, weights};
    std::copy(v, v + 6, out);
    return NVH_OK;
  });
}

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

extern "C" int nvh_mel_front_check(const nvh_mel_desc* desc, const nvh_mel_front* front) {
  return nvh_guard([&]() -> int {
    if (!desc) return NVH_ERR_ARGUMENT;
    int ld = 0;
    const int rc = mel_check(*desc, &ld);
    if (rc != NVH_OK || !front) return rc;
    return front_check(*desc, *front);
  });
}

extern "C" int nvh_mel_tables(const nvh_mel_desc* desc, float* twiddle, float* window, float* bank, int64_t twiddle_cap,
                              int64_t window_cap, int64_t bank_cap, int64_t* twiddle_count, int64_t* window_count, int64_t* bank_count) {
  return nvh_mel_tables_front(desc, nullptr, twiddle, window, bank, twiddle_cap, window_cap, bank_cap, twiddle_count, window_count, bank_count);
}

extern "C" int nvh_mel_tables_front(const nvh_mel_desc* desc, const nvh_mel_front* front, float* twiddle, float* window, float* bank,
                                    int64_t twiddle_cap, int64_t window_cap, int64_t bank_cap, int64_t* twiddle_count,
                                    int64_t* window_count, int64_t* bank_count) {
  return nvh_guard([&]() -> int {
    if (twiddle_cap < 0 || window_cap < 0 || bank_cap < 0 || (twiddle_cap > 0 && !twiddle) || (window_cap > 0 && !window) || (bank_cap > 0 && !bank))
      return NVH_ERR_ARGUMENT;
    int rc = nvh_mel_plan(desc, twiddle_count, window_count, bank_count);
    if (rc == NVH_OK && front) rc = front_check(*desc, *front);
    if (rc != NVH_OK) return rc;
    if ((twiddle && *twiddle_count > twiddle_cap) || (window && *window_count > window_cap) || (bank && *bank_count > bank_cap)) return NVH_ERR_ARGUMENT;
    if (twiddle) mel_twiddles(*desc, twiddle);
    if (window) mel_window(*desc, front ? front->window : NVH_WIN_HANN, window);
    if (bank) mel_bank(*desc, front ? front->triangles : NVH_TRI_HZ, bank);
    return NVH_OK;
  });
}

extern "C" int nvh_mel_rows(nvh_ctx* c, const nvh_mel_desc* desc, const float* d_src, float* d_dst, const int64_t* valid) {
  return nvh_mel_rows_front(c, desc, nullptr, d_src, d_dst, valid);
}

extern "C" int nvh_mel_rows_front(nvh_ctx* c, const nvh_mel_desc* desc, const nvh_mel_front* front, const float* d_src, float* d_dst,
                                  const int64_t* valid) {
  return nvh_guard([&]() -> int {
    MelPrep P;
    int rc = mel_prepare(desc, front, d_src && d_dst, valid, &P);
    if (rc != NVH_OK) return rc;
    if (!c) return NVH_ERR_NO_GPU;
    if (!P.work) return NVH_OK;
    const nvh_mel_desc& D = *desc;
    HIP_TRY(hipSetDevice(c->device));
    MelDev* tab = nullptr;
    rc = get_mel(c, D, P.window, P.triangles, &tab);
    if (rc == NVH_OK)
      rc = lds_opt_in(c->mel_lds_attr_set, NVH_MEL_LDS_BYTES, {(const void*)k_mel_rows<true, false>, (const void*)k_mel_rows<false, false>,
                                                                (const void*)k_mel_rows<true, true>, (const void*)k_mel_rows<false, true>});
    if (rc != NVH_OK) return rc;
    NvhMelArgs A{};
    if (valid) {  // the per-row block: the rows' counts
      const size_t bytes = (size_t)D.rows * sizeof(int64_t);
      void* image = nullptr;
      const void* d_block = nullptr;
      rc = c->mel_rows.begin(c, bytes, &image);
      if (rc != NVH_OK) return rc;
      std::memcpy(image, valid, bytes);
      rc = c->mel_rows.send(c, bytes, &d_block);
      if (rc != NVH_OK) return rc;
      A.valid = static_cast<const long long*>(d_block);
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
    A.groups = P.groups;
    A.total = P.total;
    A.channels = D.channels;
    A.n_fft = D.n_fft;
    A.ld = P.ld;
    A.win_length = D.win_length;
    A.hop = D.hop;
    A.n_mels = D.n_mels;
    A.scale = D.scale;
    A.floor = D.floor;
    A.weights = tab->weights;
    A.gain = 1.0f;
    if (front) {
      A.reflect = front->pad_mode == NVH_PAD_REFLECT ? 1 : 0;
      A.remove_dc = front->remove_dc;
      A.preemphasis = front->preemphasis;
      A.gain = front->gain;
    }
    const long long abs_f = D.dst_frame_stride < 0 ? -D.dst_frame_stride : D.dst_frame_stride;
    const long long abs_b = D.dst_band_stride < 0 ? -D.dst_band_stride : D.dst_band_stride;
    A.band_fast = abs_b <= abs_f ? 1 : 0;
    const NvhMelRoute route = P.route(D, tab->weights);
    A.span = route.span;
    const size_t lds = (size_t)route.lds_bytes;
    const dim3 grid((unsigned)route.blocks), block(NVH_MEL_THREADS);
    if (!P.front_in_kernel) {
      if (route.staged) hipLaunchKernelGGL((k_mel_rows<true, false>), grid, block, lds, c->stream, A);
      else hipLaunchKernelGGL((k_mel_rows<false, false>), grid, block, lds, c->stream, A);
    } else {
      if (route.staged) hipLaunchKernelGGL((k_mel_rows<true, true>), grid, block, lds, c->stream, A);
      else hipLaunchKernelGGL((k_mel_rows<false, true>), grid, block, lds, c->stream, A);
    }
    HIP_TRY(hipGetLastError());
    return NVH_OK;
  });
}

// nvh_resample.hip -- rows at one sample rate (include/nvorbis_hip.h: nvh_resample_plan / _taps / _rows): the plan and the tap
// table in double on the host, the per-context cache of device tables, and the launch of k_resample_rows (kernels_resample.hip).
#include <cmath>
#include <numeric>

#include "nvh_internal.h"

namespace {

struct ResamplePlan {
  int L = 0, M = 0, half = 0;
  int64_t tap_count = 0;
};

int resample_plan(int in_rate, int out_rate, ResamplePlan* out) {
  if (in_rate < 1 || out_rate < 1) return NVH_ERR_ARGUMENT;
  const int g = std::gcd(in_rate, out_rate);
  ResamplePlan p;
  p.L = out_rate / g;
  p.M = in_rate / g;
  if (p.L > 4096) return NVH_ERR_UNSUPPORTED;
  const int64_t half = p.L >= p.M ? 16 : ((int64_t)16 * p.M + p.L - 1) / p.L;
  if ((int64_t)p.L * 2 * half > 262144) return NVH_ERR_UNSUPPORTED;
  p.half = (int)half;
  p.tap_count = (int64_t)p.L * 2 * half;
  *out = p;
  return NVH_OK;
}

// I0 by its power series, sum over k of ((x / 2)^k / k!)^2, until a term no longer changes the sum
double bessel_i0(double x) {
  const double q = x * x / 4.0;
  double sum = 1.0, term = 1.0;
  for (int k = 1; k < 1000; ++k) {
    term *= q / ((double)k * (double)k);
    const double next = sum + term;
    if (next == sum) break;
    sum = next;
  }
  return sum;
}

void resample_taps(const ResamplePlan& p, float* h) {
  const double pi = 3.14159265358979323846;
  const double ratio = (double)p.M / (double)p.L, inv = (double)p.L / (double)p.M;
  const double W = 16.0 * (ratio > 1.0 ? ratio : 1.0);
  const double sc = 0.94 * (inv < 1.0 ? inv : 1.0);
  const double i0_beta = bessel_i0(9.0);
  const int ntaps = 2 * p.half;
  for (int ph = 0; ph < p.L; ++ph) {
    for (int k = 0; k < ntaps; ++k) {
      const double t = (double)(k - p.half + 1) - (double)ph / (double)p.L;
      const double u = t / W;
      double v = 0.0;
      if (std::fabs(u) < 1.0) {
        const double x = sc * t;
        const double sinc = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
        v = sc * sinc * bessel_i0(9.0 * std::sqrt(1.0 - u * u)) / i0_beta;
      }
      h[(size_t)ph * ntaps + k] = (float)v;
    }
  }
}

constexpr size_t kResampleLdsBytes = (size_t)(NVH_RS_TAP_FLOATS + NVH_RS_SRC_FLOATS) * sizeof(float);

int get_resample(nvh_ctx* c, const ResamplePlan& p, ResampleDev** out) {
  const auto key = std::make_pair(p.L, p.M);
  auto it = c->resample_cache.find(key);
  if (it != c->resample_cache.end()) {
    *out = &it->second;
    return NVH_OK;
  }
  std::vector<float> h((size_t)p.tap_count);
  resample_taps(p, h.data());
  ResampleDev d;
  d.L = p.L;
  d.M = p.M;
  d.half = p.half;
  const int rc = upload_table(&d.taps, h);
  if (rc != NVH_OK) return rc;
  auto ins = c->resample_cache.emplace(key, d);
  *out = &ins.first->second;
  return NVH_OK;
}

// The per-row arrays of a call, on the host (dst_row may be null: the identity).
struct ResampleRows {
  const int64_t *origin, *start, *valid;
  const int32_t* dst_row;
};

// Every check of nvh_resample_rows in front of its context's, in the header's order, and what the launch follows from: the plan
// and the route.  io: the call has its buffers and arrays (nvh_resample_route has none and checks the descriptor alone).
struct ResamplePrep {
  ResamplePlan plan;
  NvhResampleRoute route;
  bool work = false;
};
int resample_prepare(const nvh_resample_desc* desc, bool io, const ResampleRows& R, ResamplePrep* out) {
  if (!desc) return NVH_ERR_ARGUMENT;
  const nvh_resample_desc& D = *desc;
  if (D.in_rate < 1 || D.out_rate < 1 || D.rows < 0 || D.length < 0 || D.src_length < 0 || D.channels < 1 || D.channels > 65535 ||
      !PcmOut::format_ok(D.format))
    return NVH_ERR_ARGUMENT;
  out->work = D.rows > 0 && D.length > 0;
  if (out->work && !io) return NVH_ERR_ARGUMENT;
  constexpr int64_t kMaxTime = (int64_t)1 << 48;  // J * M stays inside 64 bits (M <= 8192 inside the limits)
  if (D.length > kMaxTime || D.src_length > kMaxTime) return NVH_ERR_ARGUMENT;
  for (int i = 0; out->work && R.origin && i < D.rows; ++i) {
    if (R.origin[i] < 0 || R.origin[i] > kMaxTime || R.start[i] < 0 || R.start[i] > kMaxTime - D.length || R.valid[i] < 0 ||
        R.valid[i] > D.length || (R.dst_row && R.dst_row[i] < 0))
      return NVH_ERR_ARGUMENT;
  }
  const int rc = resample_plan(D.in_rate, D.out_rate, &out->plan);
  if (rc != NVH_OK) return rc;
  out->route = nvh_resample_route_for(out->plan.L, out->plan.half, D.rows, D.channels, D.length);
  return NVH_OK;
}

}  // namespace

extern "C" int nvh_resample_route(const nvh_resample_desc* desc, int64_t* out) {
  return nvh_guard([&]() -> int {
    if (!out) return NVH_ERR_ARGUMENT;
    ResamplePrep P;
    const int rc = resample_prepare(desc, true, ResampleRows{}, &P);
    if (rc != NVH_OK) return rc;
    const int64_t v[4] = {P.route.taps_in_lds, P.route.tiles, P.route.grid_y, P.route.lds_bytes};
    std::copy(v, v + 4, out);
    return NVH_OK;
  });
}

extern "C" int nvh_resample_plan(int in_rate, int out_rate, int* up, int* down, int* half, int64_t* tap_count) {
  return nvh_guard([&]() -> int {
    if (!up || !down || !half || !tap_count) return NVH_ERR_ARGUMENT;
    ResamplePlan p;
    const int rc = resample_plan(in_rate, out_rate, &p);
    if (rc != NVH_OK) return rc;
    *up = p.L;
    *down = p.M;
    *half = p.half;
    *tap_count = p.tap_count;
    return NVH_OK;
  });
}

extern "C" int nvh_resample_taps(int in_rate, int out_rate, float* taps, int64_t cap, int64_t* count) {
  return nvh_guard([&]() -> int {
    if (!count || cap < 0 || (cap > 0 && !taps)) return NVH_ERR_ARGUMENT;
    ResamplePlan p;
    const int rc = resample_plan(in_rate, out_rate, &p);
    if (rc != NVH_OK) return rc;
    *count = p.tap_count;
    if (*count > cap) return NVH_ERR_ARGUMENT;
    resample_taps(p, taps);
    return NVH_OK;
  });
}

extern "C" int nvh_resample_rows(nvh_ctx* c, const nvh_resample_desc* desc, const float* d_src, void* d_dst, const int64_t* origin,
                                 const int64_t* start, const int64_t* valid, const int32_t* dst_row, int32_t* d_clipped) {
  return nvh_guard([&]() -> int {
    ResamplePrep P;
    int rc = resample_prepare(desc, d_src && d_dst && origin && start && valid, ResampleRows{origin, start, valid, dst_row}, &P);
    if (rc != NVH_OK) return rc;
    if (!c) return NVH_ERR_NO_GPU;
    if (!P.work) return NVH_OK;
    const nvh_resample_desc& D = *desc;
    const ResamplePlan& p = P.plan;
    HIP_TRY(hipSetDevice(c->device));
    ResampleDev* tab = nullptr;
    rc = get_resample(c, p, &tab);
    if (rc == NVH_OK)
      rc = lds_opt_in(c->resample_lds_attr_set, (int)kResampleLdsBytes, {(const void*)k_resample_rows<float>, (const void*)k_resample_rows<int16_t>});
    if (rc != NVH_OK) return rc;
    // the per-row block: three int64 arrays, then the int32 one
    const size_t n = (size_t)D.rows;
    const size_t bytes = n * (3 * sizeof(int64_t) + sizeof(int32_t));
    void* image = nullptr;
    rc = c->resample_rows.begin(c, bytes, &image);
    if (rc != NVH_OK) return rc;
    int64_t* h64 = static_cast<int64_t*>(image);
    std::memcpy(h64, origin, n * sizeof(int64_t));
    std::memcpy(h64 + n, start, n * sizeof(int64_t));
    std::memcpy(h64 + 2 * n, valid, n * sizeof(int64_t));
    int32_t* h32 = reinterpret_cast<int32_t*>(h64 + 3 * n);
    if (dst_row) std::memcpy(h32, dst_row, n * sizeof(int32_t));
    else for (size_t i = 0; i < n; ++i) h32[i] = (int32_t)i;
    const void* d_block = nullptr;
    rc = c->resample_rows.send(c, bytes, &d_block);
    if (rc != NVH_OK) return rc;

    NvhResampleArgs A{};
    const long long* d64 = static_cast<const long long*>(d_block);
    A.taps = tab->taps;
    A.src = d_src;
    A.dst = d_dst;
    A.origin = d64;
    A.start = d64 + n;
    A.valid = d64 + 2 * n;
    A.dst_row = reinterpret_cast<const int*>(d64 + 3 * n);
    A.clipped = d_clipped;
    A.length = D.length;
    A.src_length = D.src_length;
    A.src_row_stride = D.src_row_stride;
    A.src_time_stride = D.src_time_stride;
    A.src_chan_stride = D.src_chan_stride;
    A.dst_row_stride = D.dst_row_stride;
    A.dst_time_stride = D.dst_time_stride;
    A.dst_chan_stride = D.dst_chan_stride;
    A.L = p.L;
    A.M = p.M;
    A.half = p.half;
    A.taps_in_lds = P.route.taps_in_lds;
    // The kernel counts tiles in an int: that holds a length below 2^40 (2^31 tiles of 512), not every length the checks let
    // through (up to 2^48, 2^39 tiles).  Nothing refuses the lengths between; such a row would be 4 TiB of f32.
    A.tiles = (int)P.route.tiles;
    const dim3 grid((unsigned)D.rows, (unsigned)P.route.grid_y, (unsigned)D.channels), block(NVH_RS_THREADS);
    const size_t lds = (size_t)P.route.lds_bytes;
    if (D.format == NVH_PCM_S16) hipLaunchKernelGGL(k_resample_rows<int16_t>, grid, block, lds, c->stream, A);
    else hipLaunchKernelGGL(k_resample_rows<float>, grid, block, lds, c->stream, A);
    HIP_TRY(hipGetLastError());
    return NVH_OK;
  });
}

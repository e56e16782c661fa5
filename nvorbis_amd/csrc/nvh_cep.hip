// nvh_cep.hip -- cepstra and deltas of features (include/nvorbis_hip.h: nvh_cep_check / _plan / _tables / _rows): the descriptor's
// check, the tables in double on the host, the per-context cache of device tables, the upload of the per-row frame counts and
// the launch of k_cep_rows (kernels_cep.hip).
#include <cmath>

#include "nvh_internal.h"

namespace {

static_assert(NVH_CEP_FRAMES == NVH_CEP_TILE, "the header names the tile");
static_assert(NVH_CEP_MAX_WINDOW == NVH_CEP_WINDOW_MAX, "the header names the widest window");

constexpr double kPi = 3.14159265358979323846;

bool finite32(float v) { return v >= -3.40282347e+38f && v <= 3.40282347e+38f; }  // (NaN fails both)

int cep_check(const nvh_cep_desc& D) {
  if ((D.transform != NVH_CEP_NONE && D.transform != NVH_CEP_DCT2) || (D.dct_norm != NVH_CEP_ORTHO && D.dct_norm != NVH_CEP_PLAIN)) return NVH_ERR_ARGUMENT;
  if (D.order < 0 || D.order > 2 || D.window < 1 || D.window > NVH_CEP_MAX_WINDOW) return NVH_ERR_ARGUMENT;
  if (D.rows < 0 || D.channels < 1 || D.channels > 65535 || D.frames < 0 || D.frames > (1 << 24) || D.bands < 1 || D.bands > NVH_CEP_MAX_BANDS)
    return NVH_ERR_ARGUMENT;
  if (D.ceps < 1 || D.ceps > D.bands || (D.transform == NVH_CEP_NONE && D.ceps != D.bands)) return NVH_ERR_ARGUMENT;
  if ((1 + D.order) * D.ceps > NVH_CEP_MAX_COLS) return NVH_ERR_ARGUMENT;
  if (!(D.lifter >= 0.0f) || !finite32(D.lifter)) return NVH_ERR_ARGUMENT;
  if (D.reserved[0] != 0 || D.reserved[1] != 0) return NVH_ERR_ARGUMENT;
  return NVH_OK;
}

// D[k][b], row after row: the rule's table
void cep_dct(const nvh_cep_desc& D, float* out) {
  const int B = D.bands, K = D.ceps;
  const double Lf = (double)D.lifter;
  for (int k = 0; k < K; ++k) {
    const double w = D.dct_norm == NVH_CEP_PLAIN ? 2.0 : (k == 0 ? std::sqrt(1.0 / (double)B) : std::sqrt(2.0 / (double)B));
    const double lift = D.lifter > 0.0f ? 1.0 + (0.5 * Lf) * std::sin((kPi * (double)k) / Lf) : 1.0;
    const double wl = w * lift;
    for (int b = 0; b < B; ++b) out[(size_t)k * B + b] = (float)(wl * std::cos(((kPi * ((double)b + 0.5)) * (double)k) / (double)B));
  }
}

// s_1[-N .. N], then s_2[-2N .. 2N]: 6 N + 2 floats
void cep_scales(int N, float* out) {
  long long d = 0;
  for (int i = 1; i <= N; ++i) d += 2LL * i * i;
  for (int j = -N; j <= N; ++j) out[j + N] = (float)((double)j / (double)d);
  for (int j = -2 * N; j <= 2 * N; ++j) {
    long long num = 0;
    for (int i = -N; i <= N; ++i) {
      if (j - i >= -N && j - i <= N) num += (long long)i * (j - i);
    }
    out[2 * N + 1 + j + 2 * N] = (float)((double)num / (double)(d * d));
  }
}

// What k_cep_rows reads of one parameter set, on the host: the table as [b][kpad] (cep_dev.h), then the scales at their places.
std::vector<float> cep_build(const nvh_cep_desc& D) {
  const int dct = D.transform == NVH_CEP_DCT2 ? 1 : 0, B = D.bands, K = D.ceps, N = D.window;
  const int kpad = nvh_cep_kpad(K), tabf = nvh_cep_table_floats(dct, B, K);
  std::vector<float> t((size_t)tabf + NVH_CEP_SCALE_FLOATS, 0.0f);
  if (dct) {
    std::vector<float> rows((size_t)K * B);
    cep_dct(D, rows.data());
    for (int k = 0; k < K; ++k) {
      for (int b = 0; b < B; ++b) t[(size_t)b * kpad + k] = rows[(size_t)k * B + b];
    }
  }
  float s[6 * NVH_CEP_WINDOW_MAX + 2];
  cep_scales(N, s);
  std::copy(s, s + 2 * N + 1, t.begin() + tabf);
  std::copy(s + 2 * N + 1, s + 6 * N + 2, t.begin() + tabf + NVH_CEP_S2_AT);
  return t;
}

int get_cep(nvh_ctx* c, const nvh_cep_desc& D, CepDev** out) {
  uint32_t lifter_bits = 0;
  std::memcpy(&lifter_bits, &D.lifter, sizeof lifter_bits);
  const bool dct = D.transform == NVH_CEP_DCT2;  // (without a transform the table is the scales alone)
  const CepKey key(D.transform, dct ? D.bands : 0, dct ? D.ceps : 0, dct ? D.dct_norm : 0, dct ? lifter_bits : 0u, D.window);
  auto it = c->cep_cache.find(key);
  if (it != c->cep_cache.end()) {
    *out = &it->second;
    return NVH_OK;
  }
  CepDev d;
  const int rc = upload_table(&d.tab, cep_build(D));
  if (rc != NVH_OK) return rc;
  auto ins = c->cep_cache.emplace(key, d);
  *out = &ins.first->second;
  return NVH_OK;
}

long long magnitude(long long v) { return v < 0 ? -v : v; }

// Every check of nvh_cep_rows in front of its context's, in the header's order, and what the launch follows from.  io: the call
// has its buffers (nvh_cep_route has none and checks the descriptor alone).
struct CepPrep {
  bool work = false;
  int dct = 0;
  long long tiles = 0, total = 0;  // tiles per (row, channel); rows * channels * tiles (the work items are counted in 64 bits)
  NvhCepRoute route;
};
int cep_prepare(const nvh_cep_desc* desc, bool io, const int64_t* valid_frames, CepPrep* out) {
  if (!desc) return NVH_ERR_ARGUMENT;
  const nvh_cep_desc& D = *desc;
  const int rc = cep_check(D);
  if (rc != NVH_OK) return rc;
  out->work = D.rows > 0 && D.frames > 0;
  if (out->work && !io) return NVH_ERR_ARGUMENT;
  for (int i = 0; valid_frames && i < D.rows; ++i) {
    if (valid_frames[i] < 0 || valid_frames[i] > D.frames) return NVH_ERR_ARGUMENT;
  }
  out->dct = D.transform == NVH_CEP_DCT2 ? 1 : 0;
  out->tiles = (D.frames + NVH_CEP_TILE - 1) / NVH_CEP_TILE;
  if (out->work && (int64_t)D.rows * D.channels > INT64_MAX / out->tiles) return NVH_ERR_ARGUMENT;
  out->total = out->work ? (long long)D.rows * D.channels * out->tiles : 0;
  out->route = nvh_cep_route_for(out->dct, D.bands, D.ceps, D.order, D.window, out->total);
  return NVH_OK;
}

}  // namespace

extern "C" int nvh_cep_route(const nvh_cep_desc* desc, int64_t* out) {
  return nvh_guard([&]() -> int {
    if (!out) return NVH_ERR_ARGUMENT;
    CepPrep P;
    const int rc = cep_prepare(desc, true, nullptr, &P);
    if (rc != NVH_OK) return rc;
    const int64_t v[4] = {P.route.staged, P.route.lds_bytes, P.route.blocks, P.tiles};
    std::copy(v, v + 4, out);
    return NVH_OK;
  });
}

extern "C" int nvh_cep_check(const nvh_cep_desc* desc) {
  return nvh_guard([&]() -> int { return desc ? cep_check(*desc) : NVH_ERR_ARGUMENT; });
}

extern "C" int nvh_cep_plan(const nvh_cep_desc* desc, int64_t* dct_count, int64_t* scale_count) {
  return nvh_guard([&]() -> int {
    if (!desc || !dct_count || !scale_count) return NVH_ERR_ARGUMENT;
    const int rc = cep_check(*desc);
    if (rc != NVH_OK) return rc;
    *dct_count = desc->transform == NVH_CEP_DCT2 ? (int64_t)desc->ceps * desc->bands : 0;
    *scale_count = 6 * (int64_t)desc->window + 2;
    return NVH_OK;
  });
}

extern "C" int nvh_cep_tables(const nvh_cep_desc* desc, float* dct, float* scales, int64_t dct_cap, int64_t scale_cap, int64_t* dct_count,
                              int64_t* scale_count) {
  return nvh_guard([&]() -> int {
    if (dct_cap < 0 || scale_cap < 0 || (dct_cap > 0 && !dct) || (scale_cap > 0 && !scales)) return NVH_ERR_ARGUMENT;
    const int rc = nvh_cep_plan(desc, dct_count, scale_count);
    if (rc != NVH_OK) return rc;
    if ((dct && *dct_count > dct_cap) || (scales && *scale_count > scale_cap)) return NVH_ERR_ARGUMENT;
    if (dct && *dct_count > 0) cep_dct(*desc, dct);
    if (scales) cep_scales(desc->window, scales);
    return NVH_OK;
  });
}

extern "C" int nvh_cep_rows(nvh_ctx* c, const nvh_cep_desc* desc, const float* d_src, float* d_dst, const int64_t* valid_frames) {
  return nvh_guard([&]() -> int {
    CepPrep P;
    int rc = cep_prepare(desc, d_src && d_dst, valid_frames, &P);
    if (rc != NVH_OK) return rc;
    if (!c) return NVH_ERR_NO_GPU;
    if (!P.work) return NVH_OK;
    const nvh_cep_desc& D = *desc;
    if (P.route.lds_bytes > NVH_CEP_LDS_BYTES) return NVH_ERR_RUNTIME;  // (cep_dev.h asserts the largest tiles: not reached)
    HIP_TRY(hipSetDevice(c->device));
    CepDev* tab = nullptr;
    rc = get_cep(c, D, &tab);
    if (rc == NVH_OK) rc = lds_opt_in(c->cep_lds_attr_set, NVH_CEP_LDS_BYTES, {(const void*)k_cep_rows<true>, (const void*)k_cep_rows<false>});
    if (rc != NVH_OK) return rc;
    NvhCepArgs A{};
    if (valid_frames) {  // the per-row block: the rows' counted frames
      const size_t bytes = (size_t)D.rows * sizeof(int64_t);
      void* image = nullptr;
      const void* d_block = nullptr;
      rc = c->cep_rows.begin(c, bytes, &image);
      if (rc != NVH_OK) return rc;
      std::memcpy(image, valid_frames, bytes);
      rc = c->cep_rows.send(c, bytes, &d_block);
      if (rc != NVH_OK) return rc;
      A.vf = static_cast<const long long*>(d_block);
    }
    A.src = d_src;
    A.dst = d_dst;
    A.tab = tab->tab;
    A.src_row_stride = D.src_row_stride;
    A.src_chan_stride = D.src_chan_stride;
    A.src_frame_stride = D.src_frame_stride;
    A.src_band_stride = D.src_band_stride;
    A.dst_row_stride = D.dst_row_stride;
    A.dst_chan_stride = D.dst_chan_stride;
    A.dst_frame_stride = D.dst_frame_stride;
    A.dst_col_stride = D.dst_col_stride;
    A.total = P.total;
    A.tiles = P.tiles;
    A.channels = D.channels;
    A.frames = D.frames;
    A.bands = D.bands;
    A.ceps = D.ceps;
    A.dct = P.dct;
    A.order = D.order;
    A.window = D.window;
    A.src_band_fast = magnitude(D.src_band_stride) <= magnitude(D.src_frame_stride) ? 1 : 0;
    A.dst_col_fast = magnitude(D.dst_col_stride) <= magnitude(D.dst_frame_stride) ? 1 : 0;
    // a table that fits the budget beside the tile is copied into LDS once per workgroup; a larger one is read through the caches
    const dim3 grid((unsigned)P.route.blocks), block(NVH_CEP_THREADS);
    const size_t lds = (size_t)P.route.lds_bytes;
    if (P.route.staged) hipLaunchKernelGGL(k_cep_rows<true>, grid, block, lds, c->stream, A);
    else hipLaunchKernelGGL(k_cep_rows<false>, grid, block, lds, c->stream, A);
    HIP_TRY(hipGetLastError());
    return NVH_OK;
  });
}

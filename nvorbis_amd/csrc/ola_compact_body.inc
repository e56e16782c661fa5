// ola_compact_body.inc -- the body of k_ola_compact, k_ola_compact_s16 and their _planar twins (kernels.hip), included inside
// each kernel with `PCM` (float / int16_t) typedef'd and `PLANAR` (and, interleaved, a zero `plane_stride`) declared in front:
// the float kernel's code is exactly what it was before the 16-bit twin existed (the same body as an inlined template function
// compiles to a different register allocation).
  // list: the frames paired emission left to this kernel (nvh_launch.hip); emitted: k_synth wrote the PCM of every frame with
  // NVH_EMIT_DONE (such a frame is on the list only as the block that becomes the carried tail)
  const int f = list ? list[blockIdx.x] : (int)blockIdx.x;
  const NvhFrame fr = Bt.frames[f];
  const int ch = S.channels;
  if (f == last_decoded && carry_out) {
    // this block becomes the carried tail of the next batch (StreamDecoder's _prevPacketBuf), stored fully windowed
    const float* __restrict__ wl = S.windows + fr.window_off;
    for (int o = NVH_OLA_TID; o < (fr.n >> 2) * ch; o += NVH_OLA_THREADS) {
      int c = o / (fr.n >> 2), g = o - c * (fr.n >> 2);
      const float* plane = work + ((long long)f * ch + c) * S.block1;
      *reinterpret_cast<float4*>(carry_out + (long long)c * S.block1 + 4 * g) =
          compact_value4(plane, wl, fr.n, Bt.chans[fr.chan_off + c].exec, 4 * g);
    }
  }
  const int total = fr.emit_count * ch;
  if (total <= 0) return;
  if (emitted && (fr.emit_flags & NVH_EMIT_DONE)) return;
  const float* cur = work + (long long)f * ch * S.block1;
  const float* prev = nullptr;
  if (fr.ov_len > 0) prev = (fr.ov_frame == -2) ? carry : (fr.ov_frame >= 0 ? work + (long long)fr.ov_frame * ch * S.block1 : nullptr);
  const float* __restrict__ w = S.windows + fr.window_off;
  const float* __restrict__ wp = S.windows + fr.ov_window_off;
  const NvhChan* chans = Bt.chans + fr.chan_off;
  PCM* out = pcm + fr.out_pos * (PLANAR ? 1 : ch);
  int clipped = 0;
  // the carried block (ov_frame == -2) is always stored fully windowed (k_expand_carry); blocks of this batch are compact
  const bool prev_full = fr.ov_frame == -2;

  // fast path: everything in units of four samples (true for every frame of a well-formed stream except an
  // EOS-trimmed last one), up to 8 channels
  const bool vec = !PLANAR && fr.n != 0 && ch <= 8 && ((fr.emit_start | fr.emit_count | fr.start | fr.ov_src | fr.ov_len) & 3) == 0 &&
                   ((fr.out_pos * ch) & 3) == 0;
  // steady state: whole first half over the whole second half of an executing predecessor of the same size
  const unsigned all_ch = ch >= 32 ? 0xFFFFFFFFu : ((1u << ch) - 1u);
  if constexpr (PLANAR) {
    // channel-planar: every plane's first sample of the frame on a 16-byte boundary (an aligned base, a plane stride and an
    // output position in whole groups of four), up to 32 channels (the execute flags of the frame record's masks); else the
    // per-sample form below
    const bool pvec = fr.n != 0 && ch <= 32 && ((fr.emit_start | fr.emit_count | fr.start | fr.ov_src | fr.ov_len) & 3) == 0 &&
                      ((fr.out_pos | plane_stride) & 3) == 0 && (reinterpret_cast<uintptr_t>(pcm) & 15u) == 0;
    const unsigned pall = ch >= 32 ? 0xFFFFFFFFu : ((1u << ch) - 1u);
    const bool psym = pvec && prev && !prev_full && fr.ov_n == fr.n && fr.start == 0 && fr.emit_start == 0 &&
                      fr.emit_count == (fr.n >> 1) && fr.ov_src == (fr.n >> 1) && fr.ov_len == (fr.n >> 1) &&
                      (fr.exec_mask & pall) == pall && (fr.ov_exec_mask & pall) == pall && !nosym;
    if (psym || pvec) {
      clipped = psym ? ola_sym_planar<PCM>(S, fr, cur, prev, w, wp, out, plane_stride, ch, clip, NVH_OLA_TID, NVH_OLA_THREADS)
                     : ola_vec_planar<PCM>(S, fr, cur, prev, prev_full, w, wp, out, plane_stride, ch, clip, NVH_OLA_TID, NVH_OLA_THREADS);
      report_clipped(clipped, clipped_flag);
      return;
    }
  }
  const bool sym = vec && prev && !prev_full && fr.ov_n == fr.n && fr.start == 0 && fr.emit_start == 0 && fr.emit_count == (fr.n >> 1) &&
                   fr.ov_src == (fr.n >> 1) && fr.ov_len == (fr.n >> 1) && (fr.exec_mask & all_ch) == all_ch &&
                   (fr.ov_exec_mask & all_ch) == all_ch && !nosym;
  if (sym && ch > 2 && gridDim.y * NVH_OLA_GW >= (unsigned)(fr.n >> 4)) {
    // more than two channels: per-(group, channel) lanes, interleave through LDS (the launch gives every frame gridDim.y
    // workgroups of NVH_OLA_GW groups each: nvh_launch.hip)
    __shared__ __attribute__((aligned(16))) float s_run[2 * 8 * 4 * NVH_OLA_GW];
    switch (ch) {
      case 3: clipped = ola_sym_lds<3, PCM>(S, fr, cur, prev, w, wp, out, clip, s_run); break;
      case 4: clipped = ola_sym_lds<4, PCM>(S, fr, cur, prev, w, wp, out, clip, s_run); break;
      case 5: clipped = ola_sym_lds<5, PCM>(S, fr, cur, prev, w, wp, out, clip, s_run); break;
      case 6: clipped = ola_sym_lds<6, PCM>(S, fr, cur, prev, w, wp, out, clip, s_run); break;
      case 7: clipped = ola_sym_lds<7, PCM>(S, fr, cur, prev, w, wp, out, clip, s_run); break;
      default: clipped = ola_sym_lds<8, PCM>(S, fr, cur, prev, w, wp, out, clip, s_run); break;
    }
    report_clipped(clipped, clipped_flag);
    return;
  }
  if (sym) {
    switch (ch) {
      case 1: clipped = ola_sym<1, PCM>(S, fr, cur, prev, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 2: clipped = ola_sym<2, PCM>(S, fr, cur, prev, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 3: clipped = ola_sym<3, PCM>(S, fr, cur, prev, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 4: clipped = ola_sym<4, PCM>(S, fr, cur, prev, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 5: clipped = ola_sym<5, PCM>(S, fr, cur, prev, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 6: clipped = ola_sym<6, PCM>(S, fr, cur, prev, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 7: clipped = ola_sym<7, PCM>(S, fr, cur, prev, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      default: clipped = ola_sym<8, PCM>(S, fr, cur, prev, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
    }
    report_clipped(clipped, clipped_flag);
    return;
  }
  if (vec) {
    switch (ch) {
      case 1: clipped = ola_vec<1, PCM>(S, fr, cur, prev, prev_full, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 2: clipped = ola_vec<2, PCM>(S, fr, cur, prev, prev_full, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 3: clipped = ola_vec<3, PCM>(S, fr, cur, prev, prev_full, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 4: clipped = ola_vec<4, PCM>(S, fr, cur, prev, prev_full, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 5: clipped = ola_vec<5, PCM>(S, fr, cur, prev, prev_full, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 6: clipped = ola_vec<6, PCM>(S, fr, cur, prev, prev_full, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      case 7: clipped = ola_vec<7, PCM>(S, fr, cur, prev, prev_full, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
      default: clipped = ola_vec<8, PCM>(S, fr, cur, prev, prev_full, w, wp, out, clip, NVH_OLA_TID, NVH_OLA_THREADS); break;
    }
    report_clipped(clipped, clipped_flag);
    return;
  }

  for (int o = NVH_OLA_TID; o < total; o += NVH_OLA_THREADS) {
    int t = o / ch, c = o - t * ch;
    if constexpr (PLANAR) c = o / fr.emit_count, t = o - c * fr.emit_count;  // plane-major: consecutive lanes, one plane
    int idx = fr.emit_start + t;
    const NvhChan cn = chans[c];
    float v;
    if (fr.n == 0) {
      // drained carried tail (StreamDecoder.cs:352-356): the previous block's windowed samples as they are
      v = prev[(long long)c * S.block1 + fr.ov_src + t];
    } else {
      v = compact_value(cur + (long long)c * S.block1, w, fr.n, cn.exec, idx);
      int j = idx - fr.start;
      if (prev && j >= 0 && j < fr.ov_len) {  // OverlapBuffers: next[start + j] += previous[prevStart + j]
        const float* pp = prev + (long long)c * S.block1;
        v = v + (prev_full ? pp[fr.ov_src + j] : compact_value(pp, wp, fr.ov_n, cn.ov_exec, fr.ov_src + j));
      }
    }
    if (clip) v = clip_value(v, &clipped);
    if constexpr (PLANAR) pcm_store1(out + c * plane_stride + t, v);
    else pcm_store1(out + o, v);
  }
  report_clipped(clipped, clipped_flag);

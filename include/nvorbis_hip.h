/*
 * nvorbis_hip.h -- C ABI of libnvorbis_hip.so, the MI355X (gfx950) back end for NVorbis'
 * per-packet synthesis path.
 *
 * The reference (NVorbis 0.10.5, managed C#) has no native boundary; its synthesis plug-ins sit
 * behind the internal interfaces IMdct / IFloor / IResidue / IMapping / IMode created by IFactory
 * (NVorbis/Contracts/I*.cs, NVorbis/Factory.cs:5-59) and are driven once per packet by
 * StreamDecoder.DecodeNextPacket (NVorbis/StreamDecoder.cs:497-506).  This header declares what a
 * P/Invoke binding for that path binds to (see INTEGRATION.md for the C# side):
 *
 *   level 1  batched, device-pointer entry points that mirror the interface methods one to one
 *            (unit parity tests, GpuMdct / GpuFloor / GpuResidue / GpuMapping shims);
 *   level 2  a stream object that takes raw Vorbis packets exactly as IPacketProvider hands them
 *            to StreamDecoder (bytes + granule position + end-of-stream / resync flags), parses
 *            them on the host, synthesises whole batches of frames on the GPU and returns
 *            interleaved float PCM with VorbisReader.ReadSamples semantics.
 *
 * Conventions: every function returns an int status (NVH_OK == 0, negative = error, never throws or
 * unwinds across the ABI); handles are opaque; `d_` pointers are device (HBM) addresses, all other
 * pointers are host addresses owned by the caller for the duration of the call.  A handle must not
 * be used from two threads at once; distinct handles are independent.
 */
#ifndef NVORBIS_HIP_H
#define NVORBIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (C# shim maps them back to the reference's exception types) ---- */
#define NVH_OK 0
#define NVH_ERR_INVALID_DATA (-1) /* System.IO.InvalidDataException (Mapping.cs:40-77, Floor1.cs:122, Residue0.cs:64,73, Codebook.cs:63,161, Factory.cs:29,38,56) */
#define NVH_ERR_ARGUMENT (-2)     /* ArgumentOutOfRangeException / ArgumentException (StreamDecoder.cs:322-325, Floor1.cs:188) */
#define NVH_ERR_RUNTIME (-3)      /* IndexOutOfRange / NullReference / DivideByZero class faults of the managed code */
#define NVH_ERR_NOMEM (-4)
#define NVH_ERR_NOT_VORBIS (-5)   /* header signature mismatch (StreamDecoder.cs:145-155) */
#define NVH_ERR_DEVICE (-6)       /* HIP runtime error; nvh_last_hip_error() has the code */
#define NVH_ERR_UNSUPPORTED (-7)  /* legal stream outside the documented limits of this build */
#define NVH_ERR_NO_GPU (-8)       /* no gfx950 device visible: there is NO CPU fallback */

typedef struct nvh_ctx nvh_ctx;       /* device + HIP stream + per-n IMDCT table cache */
typedef struct nvh_stream nvh_stream; /* one logical Vorbis stream: setup tables in HBM + overlap state */
typedef struct nvh_batch nvh_batch;   /* one parsed batch of frames resident in HBM */

/* packet flags, as IPacket exposes them (Contracts/IPacket.cs: IsEndOfStream, IsResync) */
#define NVH_PKT_EOS 1
#define NVH_PKT_RESYNC 2

const char *nvh_version(void);
int nvh_last_hip_error(void);
int nvh_device_count(void);

/* ---- context ---- */
int nvh_ctx_create(int device, nvh_ctx **out);
void nvh_ctx_destroy(nvh_ctx *ctx);
/* Launch on an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream. */
int nvh_ctx_set_hip_stream(nvh_ctx *ctx, void *hip_stream);
int nvh_ctx_synchronize(nvh_ctx *ctx);
/* Launch shape of the GPU packet parser (nvh_stream_set_gpu_parse) for the streams of this context: packets per wavefront,
 * a power of two 1..64, 0 = automatic (one packet per wavefront up to 4096 packets per batch: the lowest latency for a lone
 * stream).  A host that keeps many contexts busy at once -- a corpus worker pool, one context per thread -- gives each
 * of them 32 (an upper limit for batches below a thousand packets, which keep at least 256 wavefronts: short files parse
 * one packet per wavefront all the same): where packets share wavefronts every lane walks its own packet (k_parse_slab_f;
 * a wavefront costs the same at 8 or 64 packets), a parse is a few dozen wavefronts, and the parses of all workers fit the
 * chip side by side (the corpus of BASELINE configs[4]: decode pass 0.82 -> 0.51 s with 8 packets per wavefront and 16
 * workers in round 5, 0.35 s with 32 and 32; with the process started under GPU_MAX_HW_QUEUES=16, the HIP runtime's
 * default of 4 hardware queues lets only four kernels run at once).
 * No counterpart in the reference (its decoder is one thread per stream); results do not depend on it. */
int nvh_ctx_set_parse_lanes(nvh_ctx *ctx, int lanes);

/* ---- level 1: batched mirrors of the plug-in interface methods (device pointers) ----
 * nvh_inverse_couple, nvh_mdct_reverse, nvh_window_apply and nvh_overlap_buffers only enqueue their kernel on the
 * context's stream (nvh_ctx_synchronize, or work queued on the same HIP stream, orders against them); the entry points
 * that return per-item status or read packets (nvh_floor*_apply, nvh_residue_decode, nvh_copy_buffer, nvh_mode_decode)
 * are synchronous. */

/* One inverse square-polar coupling step over two device vectors of `count` floats, in place (Mapping.cs:150-178). */
int nvh_inverse_couple(nvh_ctx *c, float *d_magnitude, float *d_angle, int count);

/* IFloor.Apply(IFloorData, int blockSize, float[] residue) for a Floor1 (Contracts/IFloor.cs, Floor1.cs:186-341:
 * UnwrapPosts, the walk over the sorted posts, RenderLineMulti) of stream `s`, on `batch` device vectors:
 * item b multiplies d_residue[b*stride .. +block_size/2) by the curve its posts describe, or clears it when
 * post_counts[b] == 0 (:218-221).  posts: host, [batch][64] raw values as Floor1.Unpack leaves them in
 * Data.Posts (:135-184), each 0..65535; post_counts[b] is 0 or the floor's post count (nvh_stream_floor_info).
 * status (host, [batch], may be NULL): NVH_OK, or NVH_ERR_RUNTIME where the reference would index
 * inverse_dB_table out of range (the item's vector is then unspecified, as after the managed exception);
 * with status == NULL the first such code is the return value.  Synchronous. */
int nvh_floor1_apply(nvh_stream *s, int floor_index, int block_size, int batch, const int32_t *posts,
                     const int32_t *post_counts, float *d_residue, int64_t stride, int32_t *status);
/* IFloor.Apply for a Floor0 (Floor0.cs:152-212): item b scales d_residue[b*stride .. +block_size/2) by the curve of
 * its LSP coefficients (coeffs: host, [batch][coeff_stride], the first `order` of each row as Floor0.Unpack leaves
 * them in Data.Coeff, :98-150) and amplitude amps[b] (Data.Amp), or clears it when amps[b] <= 0 (:208-211).
 * Floating point: the curve's value per Bark section (cos / sqrt / exp in double, rounded to float, Floor0.cs:167,198,201) is
 * evaluated on the calling thread with the host's math library and only gathered and multiplied on the device; values
 * differ from the managed reference only where the two platforms' libm differ in the last ulp of a double.  status as for
 * nvh_floor1_apply. */
int nvh_floor0_apply(nvh_stream *s, int floor_index, int block_size, int batch, const float *amps, const float *coeffs,
                     int coeff_stride, float *d_residue, int64_t stride, int32_t *status);
/* type (0/1), number of posts (Floor1: _xList.Length, Floor1.cs:93-107; Floor0: _order) and _range (Floor1.cs:76)
 * of floor `floor_index`. */
int nvh_stream_floor_info(const nvh_stream *s, int floor_index, int *type, int *post_count, int *range);

/* Mode.cs:24-50 of mode `mode_index`: its block flag, block size and mapping index (NVH_ERR_ARGUMENT past the last mode). */
int nvh_stream_mode_info(const nvh_stream *s, int mode_index, int *block_flag, int *block_size, int *mapping);
/* ICodebook (Contracts/ICodebook.cs:5-13) of the stream's codebook `book_index`, as Codebook.Init built it
 * (Codebook.cs:59-283) with Huffman.GenerateTable's decode tables (Huffman.cs:15-76): Dimensions, Entries, MapType, and the
 * sizes of the tables nvh_stream_codebook_tables copies out.  n_prefix = 1 << prefix_bits slots (0: the tree was never
 * built), n_overflow = -1 for the reference's null overflow list. */
int nvh_stream_codebook_info(const nvh_stream *s, int book_index, int *dimensions, int *entries, int *map_type, int *prefix_bits,
                             int *max_bits, int *n_prefix, int *n_overflow);
/* lengths[entries] (Codebook.cs:76-160; -1 = unused entry), lookup[entries * dimensions] = the indexer's table
 * (Codebook.cs:222-283, :322; untouched for map type 0), prefix[n_prefix * 5] and overflow[n_overflow * 5] = the Huffman nodes
 * as (present, value, length, bits, mask) (Huffman.cs:15-76).  Any pointer may be NULL. */
int nvh_stream_codebook_tables(const nvh_stream *s, int book_index, int32_t *lengths, float *lookup, int32_t *prefix,
                               int32_t *overflow);
/* Read-only: the route a symbol of codebook `book_index` takes through the two packet parsers, as decided per book at stream
 * open.  GPU parser (nvh_stream_set_gpu_parse): gpu_parse_ok = the stream shape is inside its limits (the other four are 0
 * when it is not); prefix_in_lds / overflow_in_lds = the book's prefix table / its overflow nodes, grouped by prefix slot, are
 * held in LDS (else read from global memory); second_level = its long codes are looked up in second-level tables (else their
 * slot's group is scanned); scan_all_slots = prefix slots whose long codes are found by scanning the book's whole overflow
 * list.  Host parser: host_scan_slots = prefix slots for which it scans the whole list.  A slot counts only if no short code
 * fills it.  A stream with a context reports what it uploaded, a host-only stream the same decisions made without a device.
 * Any pointer may be NULL. */
int nvh_stream_parse_book_info(const nvh_stream *s, int book_index, int *gpu_parse_ok, int *prefix_in_lds, int *overflow_in_lds,
                               int *second_level, int *scan_all_slots, int *host_scan_slots);

/* IResidue.Decode(IPacket, bool[] doNotDecodeChannel, int blockSize, float[][] buffer) (Contracts/IResidue.cs:6;
 * Residue0.cs:119-201, Residue1.cs:8-26, Residue2.cs:10-47) for residue `residue_index` of stream `s`: reads the
 * classifications and codebook entries from `pkt` starting at bit `bit_offset` and adds the decoded vectors into
 * d_buffer, device planes [channels][block1] (the reference's float[channels][block1Size] working buffer).
 * any_channel_decodes = doNotDecodeChannel contains a false (:125; otherwise the call reads nothing).
 * *bits_consumed: how far the packet cursor moved.  The stream must have nothing pending.  Synchronous. */
int nvh_residue_decode(nvh_stream *s, int residue_index, const uint8_t *pkt, int len, int bit_offset,
                       int any_channel_decodes, int block_size, float *d_buffer, int *bits_consumed);

/* Mode.Decode's window loop (Mode.cs:160-166) for mode `mode_index`: d_buf[b*stride + i] *= window[i], i < the
 * mode's block size, b < batch; the window is the one the packet's previous/next flag bits select (Mode.cs:135). */
int nvh_window_apply(nvh_stream *s, int mode_index, int prev_flag, int next_flag, int batch, float *d_buf,
                     int64_t stride);
/* StreamDecoder.OverlapBuffers (StreamDecoder.cs:532-541) on device planes [channels][plane_stride]:
 * next[c][next_start + j] += previous[c][prev_start + j] for j < prev_stop - prev_start. */
int nvh_overlap_buffers(nvh_ctx *c, const float *d_previous, float *d_next, int prev_start, int prev_stop,
                        int next_start, int channels, int64_t plane_stride);
/* ClippingCopyBuffer / CopyBuffer (StreamDecoder.cs:391-415, Utils.ClipValue Utils.cs:30-43): `count` samples per
 * channel from index `start` of device planes [channels][plane_stride], interleaved into d_target[count*channels];
 * clip != 0 clamps to +-0.99999994f and reports in *clipped whether any value was (HasClipped).  Synchronous. */
int nvh_copy_buffer(nvh_ctx *c, const float *d_planes, int start, int count, int channels, int64_t plane_stride,
                    float *d_target, int clip, int *clipped);

/* Device memory for callers without a HIP binding of their own (csharp/GpuFactory.cs stages the managed float[] arrays of
 * the plug-in interfaces through these).  Copies complete before the call returns. */
int nvh_dev_alloc(nvh_ctx *c, size_t bytes, void **out);
void nvh_dev_free(nvh_ctx *c, void *d_ptr);
int nvh_dev_upload(nvh_ctx *c, void *d_dst, const void *h_src, size_t bytes);
int nvh_dev_download(nvh_ctx *c, void *h_dst, const void *d_src, size_t bytes);

/* Measurement helper (no reference counterpart): `iters` passes of a float4 copy kernel over `bytes` bytes (a multiple
 * of 16) from d_src to d_dst, timed with HIP events on the context's stream; *ms = total.  bench.py reports
 * 2 * bytes * iters / ms as the measured HBM ceiling next to the roofline figure. */
int nvh_measure_copy(nvh_ctx *c, const void *d_src, void *d_dst, size_t bytes, int iters, float *ms);

/* IMdct.Reverse(float[] samples, int sampleCount) (Contracts/IMdct.cs:5, Mdct.cs:13-21) on `batch`
 * buffers: buffer b = d_buf + b*stride holds n floats, reads [0,n/2), writes [0,n).  n = 64..8192. */
int nvh_mdct_reverse(nvh_ctx *ctx, int n, int batch, float *d_buf, int64_t stride);

/* Table builders (host, exact reference typing): Mdct.cs:30-63, Mode.cs:69-117. */
int nvh_mdct_tables(int n, float *a /*n/2*/, float *b /*n/2*/, float *c /*n/4*/, uint16_t *bitrev /*n/8*/);
int nvh_calc_window(int prev_block, int block, int next_block, float *out /*block*/);
int nvh_calc_overlap(int prev_block, int block, int next_block, int *start, int *valid, int *total);

/* ---- level 2: stream ---- */

/* StreamDecoder..ctor -> ProcessHeaderPackets (StreamDecoder.cs:50-127): the three Vorbis header
 * packets.  Builds every table of LoadBooks (:226-289) and uploads it once.  ctx == NULL creates a
 * host-only stream that can parse packets but returns NVH_ERR_NO_GPU from every synthesis call. */
int nvh_stream_open(nvh_ctx *ctx, const uint8_t *id_pkt, int id_len, const uint8_t *comment_pkt, int comment_len,
                    const uint8_t *setup_pkt, int setup_len, nvh_stream **out);
void nvh_stream_close(nvh_stream *s);
/* IStreamDecoder.UpperBitrate / NominalBitrate / LowerBitrate (Contracts/IStreamDecoder.cs; the three 32-bit fields
 * of the identification header, StreamDecoder.cs:191-193). */
int nvh_stream_bitrates(const nvh_stream *s, int *upper, int *nominal, int *lower);
int nvh_stream_info(const nvh_stream *s, int *channels, int *sample_rate, int *block0, int *block1);
/* IStreamDecoder.ClipSamples (StreamDecoder.cs:723, default on) / HasClipped (:728) */
/* Page-locked host memory for PCM destinations: nvh_stream_synth writes a pinned pcm_host directly with the copy
 * engine (no bounce buffer, no memcpy on the calling thread).  Any other pinned allocation works as well. */
int nvh_pinned_alloc(size_t bytes, void **out);
void nvh_pinned_free(void *p);
int nvh_stream_set_clip(nvh_stream *s, int on);
/* Parse audio packets on the GPU (kernels_parse.hip: floors, residue classification and VQ entry decode, one lane per
 * packet) instead of on the calling thread; the host then only reads each packet's mode number and window flags.
 * Same PCM.  Difference in error behaviour: a packet the managed decoder would have thrown on (NVH_ERR_RUNTIME) is
 * reported by nvh_stream_synth for the whole look-ahead batch instead of by nvh_stream_push_packet for that packet.
 * NVH_ERR_UNSUPPORTED for stream shapes outside the GPU parser's limits (Floor0, > 8 channels); call between batches.
 * The environment variable NVH_GPU_PARSE=1 turns it on for every eligible stream. */
int nvh_stream_set_gpu_parse(nvh_stream *s, int on);
int nvh_stream_has_clipped(nvh_stream *s, int *clipped);
/* IStreamDecoder.SamplePosition after everything parsed so far has been read (StreamDecoder.cs:718) */
int nvh_stream_position(const nvh_stream *s, int64_t *position, int64_t *emitted, int *eos);

/* Host parse of one audio packet into the pending batch (DecodeNextPacket, StreamDecoder.cs:465-530,
 * bit-consuming half).  granule < 0 = packet carries no granule position. */
int nvh_stream_push_packet(nvh_stream *s, const uint8_t *data, int len, int64_t granule, int flags);
/* nvh_stream_push_packet over a packet array in one call (packet i = bytes[offsets[i], offsets[i+1]); granules / flags
 * may be NULL): the look-ahead loop of a batched caller without one FFI transition per packet.  Stops after
 * max_packets, at the first error, or once the stream has seen its end-of-stream packet; *consumed = packets taken. */
int nvh_stream_push_packets(nvh_stream *s, const uint8_t *bytes, const int64_t *offsets, const int64_t *granules,
                            const uint8_t *flags, int n, int max_packets, int *consumed);
/* _hasPosition / _currentPosition (StreamDecoder.cs:35-39) after everything pushed so far was read.  Setting them is
 * what a caller does that starts a decoder in the middle of a stream (the state SeekTo leaves behind, :562-628):
 * nvorbis_amd/corpus.py's chunked decode pushes one lead-in packet, then sets the state the serial decoder has there. */
int nvh_stream_position_state(const nvh_stream *s, int *has_position, int64_t *position);
int nvh_stream_set_position_state(nvh_stream *s, int has_position, int64_t position);
/* Index of a run of `n` audio packets (packet i = bytes[offsets[i] .. offsets[i+1]), granule -1 = none, flags NVH_PKT_*;
 * granules / flags may be NULL) as a serial decoder that starts with packet 0 of the run sees them -- the integer half of
 * ReadNextPacket (StreamDecoder.cs:417-463) and Mode.GetPacketInfo (Mode.cs:119-151) only, no floor / residue bits:
 *   position_after[i]  _currentPosition once everything packet i lets the decoder emit was read
 *   emitted_after[i]   samples per channel emitted so far
 *   state_after[i]     bit 0: the packet decodes; bit 1: and its overlap stays out of its own tail (a decoder may start
 *                      right after it with this packet as its only lead-in); bit 2: _hasPosition; bit 3: _eosFound
 * *total_emitted: samples per channel the whole run yields, including the drain of the last block's tail when the run
 * ends without an end-of-stream packet (StreamDecoder.cs:352-356).  Any output pointer may be NULL.
 * Host only; does not touch the stream's own state.  Callers: seeking and the chunked decode of nvorbis_amd. */
int nvh_stream_index_packets(const nvh_stream *s, const uint8_t *bytes, const int64_t *offsets, const int64_t *granules,
                             const uint8_t *flags, int n, int64_t *position_after, int64_t *emitted_after,
                             uint8_t *state_after, int64_t *total_emitted);
/* StreamDecoder.GetPacketGranules (StreamDecoder.cs:630-647): the sample count a packet stands for in the reference's
 * page granule arithmetic (Mode.GetPacketSampleCount, Mode.cs:172-176); 0 for resync, non-audio and short packets and
 * for an invalid mode number.  What a binding passes to IPacketProvider.SeekTo as its GetPacketGranuleCount delegate. */
int nvh_stream_packet_sample_count(const nvh_stream *s, const uint8_t *pkt, int len, int is_resync, int *count);
/* ResetDecoder (StreamDecoder.cs:295-305): previous block, position, end-of-stream and clipped flag forgotten, pending
 * frames dropped; the next packet pushed is a first packet again (emits nothing, :446-450).  SeekTo = reset, push the
 * pre-roll packet, nvh_stream_set_position_state(1, position of the packet that follows), carry on, discard the
 * roll-forward samples (:596-627). */
int nvh_stream_reset(nvh_stream *s);
/* Forget the pending (parsed, not yet synthesised) frames without synthesising them: for callers that only want the
 * integer geometry (positions, sample counts) of a stretch of packets. */
int nvh_stream_drop_pending(nvh_stream *s);
/* The packet provider returned null (StreamDecoder.cs:472-475). */
int nvh_stream_push_end(nvh_stream *s);
/* Pending (parsed, not yet synthesised) work. */
/* Frame geometry of the pending batch, 8 int32 per frame: block size, start, valid, total
 * (Mode.GetPacketInfo, Mode.cs:119-151, valid after the EOS trim of StreamDecoder.cs:429-437),
 * emit_start, emit_count, overlap source frame (-1 none, -2 carried tail), overlap length. */
int nvh_stream_pending_geometry(const nvh_stream *s, int32_t *out, int cap_frames);
int nvh_stream_pending(const nvh_stream *s, int *frames, int64_t *pcm_samples_per_channel);
/* ---- segments: many short runs of packets under one setup in one batch ----
 * A segment is one independent run of audio packets decoded under the stream's setup: it decodes exactly as a freshly opened
 * stream of the same three headers would decode it.  Several segments may share one pending batch (one upload, one parse, one
 * set of launches); a segment may also run across batch boundaries, carried like any stream.
 *
 * nvh_stream_next_segment ends the current segment as nvh_stream_push_end would (the previous block's tail is drained unless
 * an NVH_PKT_EOS packet ended the segment already) and puts the packet state machine into the state nvh_stream_reset leaves:
 * previous block, position and end of stream forgotten, the next packet a first packet again.  It KEEPS the pending frames,
 * the sticky HasClipped flag, ClipSamples, the parser choice and outstanding flights.  Then the batch's running output
 * position (samples per channel) is rounded up to a multiple of `align`, a power of two in [1, 65536] (anything else, or no
 * stream: NVH_ERR_ARGUMENT).  align = 4 is what the kernels' vector paths ask for (out_pos * channels in whole groups of
 * four; out_pos itself for planar, mono and mapped PCM): with it a segment that ends on an odd sample does not push every
 * later segment of the batch onto the per-frame fall-back.  Larger values are for callers who tile.  Segments are numbered
 * from 0 since nvh_stream_open or the last nvh_stream_reset; two calls in a row make an empty segment.
 *
 * nvh_stream_pending_segments describes the pending batch -- read it before the synthesis call that consumes the batch: one
 * entry per segment that was current while the batch was pending, in order.  The first is the segment that was open when the
 * batch began (it may contribute nothing to this batch), the last is the current segment.  index[i] is the segment's number,
 * [begin[i], end[i]) its range in the batch's output in samples per channel, the unit of nvh_stream_pending's count.  A stream
 * that never calls nvh_stream_next_segment reports the one entry {0, 0, pending samples}.  *count is set even when `cap` is
 * too small (NVH_ERR_ARGUMENT then).  Host state only: works on a host-only stream.
 *
 * nvh_stream_synth_segments is the same table for the batch the last synthesis call CONSUMED (nvh_stream_synth_* of any form;
 * for a pipelined batch, from its nvh_stream_synth_end on), as that call finally parsed it.  It equals what
 * nvh_stream_pending_segments said before the call -- except in GPU-parse mode for a batch with a packet the parser fails on
 * (the call returns that error code together with *written > 0): the look-ahead counted the packet, the batch was parsed again
 * without it, boundaries and gaps included, and the ranges behind it lie where THIS table says (each begin re-rounded to its
 * align).  The rule below holds for these ranges.  No entries before the first synthesis call and after nvh_stream_reset.
 *
 * THE RULE.  For every output form, the samples of segment k in the batch outputs, taken over its ranges in batch order, are
 * bit for bit the samples a fresh stream over the same headers and the same packets, granules and flags emits in that form.
 * Samples in the gaps that `align` opens are zero.  *written, *expected and extents count gaps as samples.
 * nvh_stream_position reports the current segment.  nvh_stream_parse_errors' samples_before stays an offset into the batch's
 * output, gaps included.  HasClipped has two calls: nvh_stream_has_clipped is the sticky OR over every segment since the last
 * reset, nvh_stream_synth_segments_clipped says which segments of the last batch set it.
 *
 * THE RULE, HasClipped.  For the batch the last synthesis call consumed, entry i of nvh_stream_synth_segments_clipped belongs
 * to entry i of nvh_stream_synth_segments.  It is 1 exactly when ClipSamples clamped at least one of the samples THIS BATCH
 * emitted inside that segment's range, in the output form of the call; otherwise 0.  ORed over the batches a segment runs
 * through, it is the HasClipped a fresh stream over the same headers, packets, granules and flags reports after emitting the
 * same samples in the same form.  With NVH_MIX_MONO the mix decides the flag; with a channel map only the emitted channels
 * count; with a window only the emitted samples count; gaps and pads never set a flag; with ClipSamples off every entry is 0.
 * In GPU-parse mode a batch that was parsed again reports by the table as finally parsed.  nvh_stream_has_clipped keeps its
 * meaning and its value in every case (it is the OR of every entry since the last reset).
 * The call follows nvh_stream_synth_segments' conventions: *count is set even when `cap` is too small (NVH_ERR_ARGUMENT
 * then); no entries before the first synthesis call and after nvh_stream_reset; host state only once the synthesis call has
 * returned (works on a host-only stream: no entries); for a pipelined batch valid from that batch's nvh_stream_synth_end on.
 * A batch of one segment -- every stream that never calls nvh_stream_next_segment -- launches exactly what it launched before
 * there was this call: its one entry is what the batch added to the sticky flag.  Resident batches (nvh_batch_*) have no
 * table: they are launched repeatedly and report through nvh_stream_has_clipped alone.
 * Python: Stream.synth_segments_clipped, decode_clips(..., return_clipped=True). */
int nvh_stream_next_segment(nvh_stream *s, int align);
/* ---- windowed segments: crop and pad a segment into a fixed-length row ----
 * nvh_stream_segment_window applies to the CURRENT segment and is legal only while that segment has seen no packet and no
 * nvh_stream_push_end -- after nvh_stream_open, nvh_stream_reset or nvh_stream_next_segment; a second call before the first
 * packet replaces the first.  NVH_ERR_ARGUMENT otherwise, and for: no stream, skip < 0, take < -1, pitch < 0, pitch > 0 with
 * take < 0 or take > pitch.  nvh_stream_next_segment and nvh_stream_reset restore the default (0, -1, 0), with which
 * everything is as without the call, bit for bit, the kernels launched included.
 *
 * THE RULE, windowed.  Number the samples per channel that a fresh stream over the same headers, packets, granules and flags
 * emits from 0.  The segment emits exactly those with skip <= e < skip + take (take = -1: no upper end; fewer if the stream
 * emits fewer), in every output form, bit for bit.  Its ranges in nvh_stream_pending_segments / nvh_stream_synth_segments
 * cover emitted samples only; HasClipped follows the emitted samples.  nvh_stream_position: `position` keeps counting
 * un-windowed stream time (the end-of-stream trim needs it), `emitted` counts what was emitted.
 *
 * Full window.  Once skip + take samples have been accounted for, the segment takes no more packets, as after an end-of-stream
 * packet: nvh_stream_push_packet returns NVH_OK without parsing, nvh_stream_push_packets stops there (*consumed excludes such
 * packets), and in GPU-parse mode they never reach the parser.  The packet that fills the window is parsed whole, only its
 * emission is cut; the drain at the next boundary emits nothing.
 *
 * Pitch.  With pitch > 0, nvh_stream_next_segment -- before its `align` rounding -- advances the output position to the
 * segment's first output position plus `pitch`: a pad of pitch minus everything the segment emitted, in this batch and in
 * earlier ones.  The pad is a gap: zeros, outside the segment's range, counted in *written / *expected / extents (pads longer
 * than a chunk are written by k_zero_rows, one bounded chunk per workgroup).  nvh_stream_push_end does not pad: the last row
 * is closed with nvh_stream_next_segment.  An empty segment with a pitch is a row of zeros.  For a segment with a pitch the
 * `align` rounding is applied to the pitch (the next segment begins pitch rounded up to `align` behind this one's first
 * sample, also where that sample lies in an earlier batch at an odd position), so that with a pitch that `align` divides,
 * the batch outputs of a run of rows, concatenated, ARE the dense [N, pitch] buffer.
 *
 * Two limits.  (1) A pending batch of pads alone (segments that emit nothing) is written by the nvh_stream_synth_* calls; the
 * pipelined nvh_stream_synth_begin treats a batch without frames as empty, as before, and leaves the pads pending: they join the
 * next batch that has frames, or are flushed by a synchronous synthesis call.  (2) GPU-parse mode, a segment with a bounded take
 * that holds a packet the parser fails on: the look-ahead counts that packet's samples towards the window, so the window may be
 * declared full one or more packets earlier than in host-parse mode; the replay emits nothing for the failing packet and the
 * packets that were kept out are not there to fill the window: the segment comes out shorter than the host parser's (never
 * different in the samples it has; nvh_stream_synth_segments tells its true range).  A caller who needs the host parser's
 * count pushes such a clip with take = -1, or in host-parse mode.
 *
 * A frame whose emission the window cuts is emitted by the per-frame overlap kernel; a skip and a take in whole groups of four
 * samples keep its vector paths, and with them every later frame of the row on paired emission (frame starts lie on multiples
 * of 64 samples of stream time for blocks of 256 and more).  Python: Stream.segment_window, nv.decode_clip_rows. */
int nvh_stream_segment_window(nvh_stream *s, int64_t skip, int64_t take, int64_t pitch);
int nvh_stream_pending_segments(const nvh_stream *s, int64_t *index, int64_t *begin, int64_t *end, int cap, int *count);
int nvh_stream_synth_segments(const nvh_stream *s, int64_t *index, int64_t *begin, int64_t *end, int cap, int *count);
int nvh_stream_synth_segments_clipped(const nvh_stream *s, int32_t *clipped, int cap, int *count);
/* The pending frames in the form the synthesis kernels fetch (per-frame slabs: the integer half of Floor1.Apply --
 * UnwrapPosts and the walk over the sorted posts, Floor1.cs:196-297 -- as line segments, the vector writes of
 * Residue0.cs:132-175 / Residue2.cs:23-47 as chain-major records; the entry section in DIGIT form for setups whose residue books
 * have at most 63 lattice values (nvh_format.h: NVH_SLAB_RGEOM_DIGITS -- one byte per vector component, the byte offset of its
 * float from the book's first word in the value pool; a record's x then counts 2-byte units of that section, its y holds the
 * book's value-pool offset), else as uint16 entry numbers), written by the host parser's thread.  Host only, for
 * tests and tools: buf receives the slabs back to back, first_unit[f] the first 16-byte unit of frame f's slab
 * (first_unit[frames] = total units).  NVH_ERR_UNSUPPORTED: the stream shape is outside the slab kernels' contract.
 * *bytes is set even when cap is too small (NVH_ERR_ARGUMENT then). */
int nvh_stream_pending_slabs(const nvh_stream *s, uint8_t *buf, int64_t cap, int64_t *bytes, uint32_t *first_unit,
                             int cap_frames);
/* The setup's lattice pool as the synthesis kernels hold it: per lattice codebook (Codebook.cs:222-283, lookup type 1 without
 * sequence_p) its distinct component values as float bits, then the reciprocals ceil(2^32 / lat_values^i) for i < dimensions;
 * a slab record of the ENTRY form points at a book's first value there.  Behind it -- only for setups that take the digit form --
 * the VALUE pool: per book its distinct values again, then +0.0f (where the bytes of a vector that was never added point); a slab
 * record of the DIGIT form holds the offset of the book's first value-pool word, counted from the lattice pool's start.  Host only,
 * for tests and tools.  *words is set even when cap_words is too small (NVH_ERR_ARGUMENT then). */
int nvh_stream_lattice_pool(const nvh_stream *s, uint32_t *out, int64_t cap_words, int64_t *words);
/* The setup's VQ table pool (Codebook.cs:222-283: every book's lookup table, entries x dimensions floats, book after book).  A
 * slab record that names a book with an EXPLICIT table (lookup type 2, or type 1 with sequence_p: lat_values = 0 in the record)
 * points at one word of the lattice pool, that book's offset in this pool; component d of entry e is float offset + e * dim + d.
 * Host only, for tests and tools.  *floats is set even when cap_floats is too small (NVH_ERR_ARGUMENT then). */
int nvh_stream_vq_pool(const nvh_stream *s, float *out, int64_t cap_floats, int64_t *floats);

/* ---- synthesis: one PCM output descriptor, three calls that take it ----
 * What a synthesis call writes is said by ONE descriptor: the sample format, the down-mix, the layout, the channel map and
 * the room the destination has.  nvh_stream_synth_out synthesises the pending batch (H2D descriptors -> kernels -> PCM) into
 * exactly one of pcm_host / d_pcm and advances the overlap state; nvh_stream_synth_begin_out is its pipelined form for a
 * page-locked pcm_host (nvh_stream_synth_end retires it); nvh_batch_synth_out launches a device-resident batch.  Every
 * named synthesis call below (nvh_stream_synth*, nvh_stream_synth_begin*, nvh_batch_synth*) is shorthand for one of the three
 * with a descriptor filled from its arguments, and keeps the comment that explains its form; a further output form is a
 * further field here, not a further set of calls.
 *   format        NVH_PCM_F32 / NVH_PCM_S16 (see nvh_stream_synth_pcm)
 *   mix           NVH_MIX_NONE / NVH_MIX_MONO (see nvh_stream_synth_mix); not together with planar or a map
 *   planar        0: interleaved; 1: channel-planar (see nvh_stream_synth_planar).  A field of its own: a planar call with a
 *                 stride of 0 and nothing to write is legal, so a positive stride cannot be what marks the layout
 *   out_channels  0: no channel map; else the number of entries of map (see nvh_stream_synth_map)
 *   map           out_channels entries, read during the call only; ignored when out_channels == 0
 *   extent        interleaved / mixed: the destination's capacity in output samples; planar: the plane stride in samples per
 *                 channel.  *written and *expected count in the same unit.
 * Errors, in this order: NVH_ERR_ARGUMENT for no stream or no descriptor, a planar flag other than 0 / 1, a mix together with
 * planar or a map; the map's errors (NVH_ERR_ARGUMENT / NVH_ERR_UNSUPPORTED, see nvh_stream_synth_map); NVH_ERR_ARGUMENT for an
 * unknown format or mix, both destinations (begin: no pcm_host), a misaligned device base; from here on *written / *expected
 * is 0; NVH_ERR_ARGUMENT for an extent below the pending samples or no destination with PCM to write; NVH_ERR_NO_GPU for a
 * host-only stream.  (Interleaved unmixed un-mapped PCM -- the descriptor of nvh_stream_synth_pcm -- compares its capacity only
 * after the device was found and an empty batch returned NVH_OK.) */
typedef struct nvh_pcm_out {
  int32_t format;       /* NVH_PCM_* */
  int32_t mix;          /* NVH_MIX_* */
  int32_t planar;       /* 0: interleaved; 1: channel-planar (extent is then the plane stride) */
  int32_t out_channels; /* 0: no channel map; else the number of entries of map */
  const int32_t *map;   /* out_channels entries, or NULL */
  int64_t extent;       /* capacity in output samples, or plane stride in samples per channel */
} nvh_pcm_out;
int nvh_stream_synth_out(nvh_stream *s, const nvh_pcm_out *out, void *pcm_host, void *d_pcm, int64_t *written);
int nvh_stream_synth_begin_out(nvh_stream *s, const nvh_pcm_out *out, void *pcm_host, int64_t *expected);

/* Synthesise the pending batch: H2D descriptors -> kernels -> interleaved PCM.  Exactly one of
 * pcm_host / d_pcm is non-NULL; capacity is in floats and must hold pending samples * channels.
 * Advances the overlap state (the last block's tail is carried to the next batch).
 * Shorthand for nvh_stream_synth_out with {NVH_PCM_F32, extent = capacity}. */
int nvh_stream_synth(nvh_stream *s, float *pcm_host, float *d_pcm, int64_t capacity, int64_t *written);
/* Pipelined form for a destination in page-locked host memory (nvh_pinned_alloc): nvh_stream_synth_begin queues the upload, the
 * synthesis and -- on a copy stream of its own -- the transfer of the PCM and returns (*expected = floats the batch will
 * deliver); nvh_stream_synth_end waits for the OLDEST outstanding batch and reports what nvh_stream_synth would have (error
 * codes, *written, nvh_stream_parse_errors).  Up to two batches may be outstanding: the PCIe transfer of batch i overlaps the
 * upload, the parse and the kernels of batch i+1 (begin itself first waits for the kernels of the batch before it -- both flights
 * share one scratch batch -- so what overlaps batch i's kernels is the pushing of batch i+1, which happens before its begin);
 * each needs its own destination buffer until its end call returns.  No counterpart in the
 * reference (its Read is synchronous); nvh_stream_synth must not be mixed in while batches are outstanding (NVH_ERR_ARGUMENT).
 * nvh_stream_synth_begin is shorthand for nvh_stream_synth_begin_out with {NVH_PCM_F32, extent = capacity}. */
int nvh_stream_synth_begin(nvh_stream *s, float *pcm_host, int64_t capacity, int64_t *expected);
int nvh_stream_synth_end(nvh_stream *s, int64_t *written);
/* Output formats of the *_pcm forms of the synthesis calls.  NVH_PCM_S16 is libvorbis ov_read's conversion, done inside the
 * kernels on the float the float path emits (after ClipSamples' clip): s16 = clamp(rint(x * 32768), -32768, 32767), ties to even,
 * NaN -> 0; out-of-range values saturate without touching HasClipped.  No counterpart in the reference.  The format belongs to
 * the call, not the stream (batches of one stream may alternate).  Capacities, *written and *expected count samples; a 16-bit
 * d_pcm must be 16-byte aligned.  An unknown format, or a misaligned 16-bit d_pcm: NVH_ERR_ARGUMENT.  The float forms above are
 * these with NVH_PCM_F32; nvh_stream_synth_end serves both.  Shorthand for the descriptor calls with {format, extent = capacity}. */
#define NVH_PCM_F32 0
#define NVH_PCM_S16 1
int nvh_stream_synth_pcm(nvh_stream *s, int format, void *pcm_host, void *d_pcm, int64_t capacity, int64_t *written);
int nvh_stream_synth_begin_pcm(nvh_stream *s, int format, void *pcm_host, int64_t capacity, int64_t *expected);
/* Planar forms of nvh_stream_synth_pcm / nvh_stream_synth_begin_pcm / nvh_batch_synth_pcm: channel c's samples go to
 * base + c * plane_stride (in samples of the format); plane_stride >= the batch's samples per channel; *written and
 * *expected count samples PER CHANNEL.  Nothing outside [c*plane_stride, c*plane_stride + written) is written.  The emitting
 * kernels' _planar twins write the planes themselves (a device base aligned to its sample size; the vector stores run where the
 * base is 16-byte aligned and plane_stride a multiple of 4).  A host destination is read back as one 2-D copy (one plain copy
 * when plane_stride equals the batch's length); pinned memory takes it without a bounce.  nvh_stream_synth_end retires planar
 * flights too; planar and interleaved batches of one stream may alternate.  NVH_ERR_ARGUMENT: an unknown format, both
 * destinations or neither (with PCM to write), plane_stride too small, a misaligned device base, batches outstanding.
 * No counterpart in the reference (libvorbis' ov_read_float hands out planes).  Shorthand for the descriptor calls with
 * {format, planar = 1, extent = plane_stride}. */
int nvh_stream_synth_planar(nvh_stream *s, int format, void *pcm_host, void *d_pcm, int64_t plane_stride, int64_t *written);
int nvh_stream_synth_begin_planar(nvh_stream *s, int format, void *pcm_host, int64_t plane_stride, int64_t *expected);
/* Mixing forms of nvh_stream_synth_pcm / nvh_stream_synth_begin_pcm / nvh_batch_synth_pcm: the channels of a sample time are
 * mixed into ONE output sample inside the emitting kernels (their _mono twins).  NVH_MIX_NONE is the *_pcm call.  NVH_MIX_MONO,
 * for a stream of C channels, with x_c(t) the float sample the float path produces for channel c at time t BEFORE ClipSamples'
 * clip (what it emits with clipping off; a channel that does not execute contributes the +0.0f it contributes today):
 *     s = x_0;  s = s + x_1;  ...  s = s + x_{C-1}     (C - 1 fp32 additions, in channel order, each rounded once)
 *     m = s / (float)C                                  (one correctly rounded fp32 division)
 *     y = ClipSamples ? clip(m) : m                     (the clip every emitter applies, Utils.cs:30-43, applied ONCE, to the mix)
 * NVH_PCM_S16 then converts y as it converts every float.  HasClipped becomes true when the MIX clips: a channel that alone
 * leaves [-1, 1] does not set it in a mixed batch.  C = 1 is the identity (the existing kernels run).  Capacities, *written
 * and *expected count output samples (NVH_MIX_MONO: samples per channel); nvh_stream_parse_errors' samples_before is per
 * channel already, which for a mix is the output position.  A device base must be aligned to its sample size; the vector
 * stores run where it is 16-byte aligned and every frame of the batch starts on a multiple of four samples, else the batch
 * falls back to the per-frame overlap kernel (same bits).  nvh_stream_synth_end retires these flights too; mixed and unmixed
 * batches, and formats, may alternate on one stream (the carried tail stays per-channel float planes).  NVH_ERR_ARGUMENT: an
 * unknown mix or format, both destinations or neither (with PCM to write), a capacity below the pending samples, a misaligned
 * device base, batches outstanding.  No counterpart in the reference (NVorbis emits channels as they are).  Shorthand for the
 * descriptor calls with {format, mix, extent = capacity}; with NVH_MIX_NONE these calls still compare the capacity before
 * they look for the device, as they do for every mix, where the *_pcm calls compare it after. */
#define NVH_MIX_NONE 0
#define NVH_MIX_MONO 1
int nvh_stream_synth_mix(nvh_stream *s, int format, int mix, void *pcm_host, void *d_pcm, int64_t capacity, int64_t *written);
int nvh_stream_synth_begin_mix(nvh_stream *s, int format, int mix, void *pcm_host, int64_t capacity, int64_t *expected);
/* Channel-map forms of the *_pcm and *_planar calls: the emitting kernels (their _map twins) write `out_channels` output slots
 * per sample time, and output slot j holds source channel map[j] -- a permutation (WAVE order), a selection ("front pair only",
 * "drop the LFE", "channel 3 as a mono plane"), or both.  THE RULE: output slot j at time t is exactly the sample the un-mapped call
 * of the same format emits for channel map[j] at time t, ClipSamples' clip and the 16-bit conversion included; a map has no
 * arithmetic of its own.  1 <= out_channels <= channels; the entries are distinct and in [0, channels).  The map belongs to the
 * call, like format and layout: mapped and un-mapped batches (and formats, layouts, mixes) of one stream may alternate, because
 * the carried tail stays per-channel float planes.  HasClipped follows the EMITTED samples: a channel the map drops does not set
 * it in that batch.  The identity map (out_channels == channels, map[j] == j) IS the un-mapped call: the existing kernels run
 * (nvh_stream_kernels shows their names) under that call's own rules.  Interleaved (*_map): out_channels samples per sample
 * time; capacities, *written and *expected count output samples.  Planar (*_planar_map): output slot j at
 * base + j * plane_stride; counts per channel, as in the planar calls.  A device base must be aligned to its sample size; the
 * vector stores run where it is 16-byte aligned and every frame of the batch starts on a multiple of four samples per channel
 * (planar: and the stride is a multiple of four), else the batch falls back to the per-frame overlap kernel (same bits).
 * Streams of three to eight channels keep paired emission under a map (k_synth8_emit*_map).  The mono / stereo emitting kernels
 * have no mapped forms: there a map that is not the identity is a swap or a single channel, and its batch runs without paired
 * emission (k_synth + the mapped k_ola_compact) -- the route of a planar call with a misaligned destination; blocks beyond
 * 2048 take the wide kernel and keep it.
 * Errors, in this order: NVH_ERR_ARGUMENT for no stream, a null map, out_channels outside [1, channels], an entry out of range
 * or named twice; NVH_ERR_UNSUPPORTED for a map other than the identity on a stream of more than 8 channels (the map travels
 * as eight nibbles); then the un-mapped twin's own argument errors in its own order.  A map cannot be combined with a mix.
 * No counterpart in the reference (NVorbis emits channels in Vorbis order).  Shorthand for the descriptor calls with
 * {format, planar, out_channels, map, extent = capacity or plane_stride}; these calls always ask for a map (a count of 0 is
 * refused here, where a descriptor with out_channels == 0 has none).
 *
 * nvh_channel_map_wave fills map[0 .. channels) with the Vorbis-to-WAVE permutation for 1 to 8 channels (other counts:
 * NVH_ERR_ARGUMENT).  Derivation: Vorbis I 4.3.9 fixes the order of a stream's channels --
 *   1: M | 2: L R | 3: L C R | 4: FL FR RL RR | 5: FL C FR RL RR | 6: FL C FR RL RR LFE | 7: FL C FR SL SR RC LFE |
 *   8: FL C FR SL SR RL RR LFE
 * -- and WAVE_FORMAT_EXTENSIBLE orders the channels present by the bit order of dwChannelMask: FL FR FC LFE BL BR (FLC FRC) BC
 * SL SR.  Sorting each Vorbis layout by those bits (rear = back) gives, by output slot with the source channel as value,
 *   1: {0}  2: {0,1}  3: {0,2,1}  4: {0,1,2,3}  5: {0,2,1,3,4}  6: {0,2,1,5,3,4}  7: {0,2,1,6,5,3,4}  8: {0,2,1,7,5,6,3,4}
 * (7: FL FR FC LFE BC SL SR; 8: FL FR FC LFE BL BR SL SR). */
int nvh_channel_map_wave(int channels, int32_t *map);
int nvh_stream_synth_map(nvh_stream *s, int format, const int32_t *map, int out_channels, void *pcm_host, void *d_pcm, int64_t capacity, int64_t *written);
int nvh_stream_synth_begin_map(nvh_stream *s, int format, const int32_t *map, int out_channels, void *pcm_host, int64_t capacity, int64_t *expected);
int nvh_stream_synth_planar_map(nvh_stream *s, int format, const int32_t *map, int out_channels, void *pcm_host, void *d_pcm, int64_t plane_stride, int64_t *written);
int nvh_stream_synth_begin_planar_map(nvh_stream *s, int format, const int32_t *map, int out_channels, void *pcm_host, int64_t plane_stride, int64_t *expected);
/* After nvh_stream_synth returned an error code together with *written > 0 (GPU-parse mode: packets of the batch made
 * the parser fail -- with the codes nvh_stream_push_packet returns for them in host-parse mode -- and the batch was
 * parsed again on the host without them): every such packet in stream order, codes[i] and samples_before[i] = the
 * samples per channel of that batch's PCM that precede it, i.e. where the reference's exception would have surfaced.
 * *count = how many there are (0 when the last synthesis reported none); at most `cap` are written. */
int nvh_stream_parse_errors(const nvh_stream *s, int32_t *codes, int64_t *samples_before, int cap, int *count);

/* ---- device-resident batches (benchmarks, pipelined callers) ---- */
/* Move the pending batch into HBM as an object of its own; the stream's pending batch becomes empty
 * and its overlap state advances as if the batch had been synthesised. */
/* IMode.Decode (Mode.cs:153-170) on ONE audio packet: the bit-consuming half on the host, then floors, residue adds, inverse
 * coupling, floor apply, IMDCT and window on the GPU -- the windowed block before any overlap -- into d_block
 * [channels][block1] (device).  Independent of the stream's decode state (needs an empty pending batch); *decoded = 0
 * when the reference returns without decoding the packet.  Geometry as Mode.GetPacketInfo reports it. */
int nvh_mode_decode(nvh_stream *s, const uint8_t *pkt, int len, float *d_block, int *decoded, int *block_size, int *start,
                    int *valid, int *total);

int nvh_batch_upload(nvh_stream *s, nvh_batch **out);
int nvh_batch_info(const nvh_batch *b, int *frames, int *chan_frames, int64_t *pcm_samples_per_channel,
                   int64_t *descriptor_bytes);
/* Descriptor element counts: frames, channel-frames, residue passes, residue ops, VQ entries, floor1 posts,
 * floor0 coefficients, nanoseconds the descriptor -> slab conversion of this upload took on the GPU (0: none). */
int nvh_batch_stats(const nvh_batch *b, int64_t *out8);
/* Names of the kernels behind the four timing slots of nvh_batch_time, as launched last (comma separated,
 * "-" = empty slot): which of the kernel variants ran depends on the stream shape. */
int nvh_batch_kernels(const nvh_batch *b, char *buf, int cap);
/* The same for the batch nvh_stream_synth / nvh_stream_synth_begin launched last (the stream's own look-ahead batch). */
int nvh_stream_kernels(const nvh_stream *s, char *buf, int cap);
/* Diagnostics (like nvh_batch_kernels; the values are not part of the ABI): how many of the batch's groups of two frames the
 * frame-group synthesis takes through its steady body -- two long stereo blocks between neighbours of the same size, both
 * channels executing, nothing carried in or out -- instead of the general one.  Counted at upload from the slab headers by the
 * test the kernel itself applies; 0 for batches the GPU parser wrote, and with NVH_NO_STEADY=1. */
int nvh_batch_steady_groups(const nvh_batch *b, int *groups);
/* The same for the batch nvh_stream_synth / nvh_stream_synth_begin launched last. */
int nvh_stream_steady_groups(const nvh_stream *s, int *groups);
/* The same for the stream's pending frames as an upload would lay them out; host-parsing streams only, needs no GPU. */
int nvh_stream_pending_steady(const nvh_stream *s, int *groups);
/* The same test on `frames` slab headers of sixteen 32-bit words each (groups are frames 2 g and 2 g + 1) of a stream of
 * `channels` channels whose larger block size is block1: no stream, no GPU. */
int nvh_steady_count(const uint32_t *headers, int frames, int channels, int block1, int *groups);
/* Launch the synthesis kernels for a resident batch (asynchronous on the context's stream) into the destination `out`
 * describes (nvh_pcm_out, above); may be repeated, results are identical each time. */
int nvh_batch_synth_out(nvh_batch *b, const nvh_pcm_out *out, void *d_pcm);
/* Shorthands for nvh_batch_synth_out, as the stream's named calls are for theirs: interleaved float PCM, d_pcm holds
 * samples*channels floats ... */
int nvh_batch_synth(nvh_batch *b, float *d_pcm, int64_t capacity);
/* ... the same in an output format (NVH_PCM_*; see nvh_stream_synth_pcm) ... */
int nvh_batch_synth_pcm(nvh_batch *b, int format, void *d_pcm, int64_t capacity);
/* ... and channel-planar (see nvh_stream_synth_planar). */
int nvh_batch_synth_planar(nvh_batch *b, int format, void *d_pcm, int64_t plane_stride);
/* ... and mixed (see nvh_stream_synth_mix); capacity in output samples. */
int nvh_batch_synth_mix(nvh_batch *b, int format, int mix, void *d_pcm, int64_t capacity);
/* ... and with a channel map (see nvh_stream_synth_map); capacity in output samples, plane_stride per channel. */
int nvh_batch_synth_map(nvh_batch *b, int format, const int32_t *map, int out_channels, void *d_pcm, int64_t capacity);
int nvh_batch_synth_planar_map(nvh_batch *b, int format, const int32_t *map, int out_channels, void *d_pcm, int64_t plane_stride);
/* Time `iters` repetitions with hipEvents on the launch stream: total milliseconds for the whole
 * pipeline, and per timing slot (spectrum: residue | couple+floor, or fused in slot 1; imdct+window; overlap+emit;
 * see nvh_batch_kernels).  A slot brackets its launches with event records, which costs ~2 us per slot. */
int nvh_batch_time(nvh_batch *b, float *d_pcm, int64_t capacity, int iters, float *total_ms, float *kernel_ms /*[4]*/);
void nvh_batch_free(nvh_batch *b);

/* ---- container helper (minimal forward-only demux so .ogg files can feed the path) ----
 * Splits the first logical stream of an Ogg file into packets the way NVorbis' seekable reader
 * delivers them (Ogg/PageReader.cs:27-93, Ogg/PacketProvider.cs:324-438).  Call with NULL outputs to
 * size, then again with buffers: the sizing call keeps its result for the fill call that follows on the same
 * thread with the same bytes (the file is demultiplexed once; any other call sequence simply demultiplexes again). */
int nvh_ogg_demux(const uint8_t *bytes, size_t len, uint8_t *pkt_bytes, int64_t pkt_bytes_cap, int64_t *offsets,
                  int64_t *granules, uint8_t *flags, int pkt_cap, int *npackets, int64_t *total_bytes);
/* The same for logical stream `stream_index` of a multiplexed or chained file; *nstreams (may be NULL) = number of
 * logical streams in the file.  A stream begins with the first page of a serial number that has no open stream, ends with
 * its end-of-stream page (a later page with the same serial number starts another one); a page without packets is refused
 * and its serial number ignored from then on (Ogg/PageReader.cs:126-158, Ogg/PageReaderBase.cs:72-85).  Streams that are
 * not Vorbis are listed too: nvh_stream_open refuses them (NVH_ERR_NOT_VORBIS), as VorbisReader's new-stream callback
 * does (VorbisReader.cs:74-87).  NVH_ERR_ARGUMENT for a stream_index past the last stream. */
int nvh_ogg_demux_stream(const uint8_t *bytes, size_t len, int stream_index, uint8_t *pkt_bytes, int64_t pkt_bytes_cap,
                         int64_t *offsets, int64_t *granules, uint8_t *flags, int pkt_cap, int *npackets,
                         int64_t *total_bytes, int *nstreams);

/* The index form of nvh_ogg_demux_stream, for a pass that only asks what the stream decodes to (a corpus transcoder sizing its
 * output before the first kernel runs): the same page walk and packet rules (Ogg/PageReaderBase.cs:227-292 header + lacing
 * values, Ogg/PacketProvider.cs:324-438) WITHOUT the page checksums and without the packets' bodies.  The first three packets
 * (the Vorbis headers) are delivered whole, every other packet as its first (up to) 8 bytes -- packet type, mode number and window
 * flags, all nvh_stream_index_packets reads, are in the first two; *payload_bytes = the bytes the packets really have.  One call,
 * caller's buffers (pkt_bytes_cap >= len and pkt_cap >= len / 27 + 8 always suffice); NVH_ERR_ARGUMENT when they are too small.
 * A damaged page passes unnoticed here: the pass that decodes the file demultiplexes it with the checksums and compares the
 * packet count and the payload size with this call's (a refused page changes both). */
int nvh_ogg_index_packets(const uint8_t *bytes, size_t len, int stream_index, uint8_t *pkt_bytes, int64_t pkt_bytes_cap,
                          int64_t *offsets, int64_t *granules, uint8_t *flags, int pkt_cap, int *npackets,
                          int64_t *total_bytes, int64_t *payload_bytes, int *nstreams);

/* The packet list of a source that cannot seek: ForwardOnlyPageReader + ForwardOnlyPacketProvider
 * (Ogg/ForwardOnlyPageReader.cs:21-52, Ogg/ForwardOnlyPacketProvider.cs:36-67, 119-290), same calling convention.  It differs from
 * the seekable reader's list in the resync marks (the first page always carries one, sequence numbers are checked without the
 * exemption for 0), in zero-length packets (delivered), in pages that start with the tail of a lost packet (their packets are cut
 * from the wrong bytes, as the reference cuts them) and in continued packets (no granule position, no end-of-stream mark). */
int nvh_ogg_demux_forward(const uint8_t *bytes, size_t len, int stream_index, uint8_t *pkt_bytes, int64_t pkt_bytes_cap,
                          int64_t *offsets, int64_t *granules, uint8_t *flags, int pkt_cap, int *npackets,
                          int64_t *total_bytes, int *nstreams);

/* ---- seeking ----
 * Page table of one logical stream plus the reference's seek search over it:
 *   StreamPageReader.FindPage / FindPageBisection / FindPageForward   Ogg/StreamPageReader.cs:122-264
 *   PacketProvider.SeekTo / FindPacket / granule-bug workaround        Ogg/PacketProvider.cs:56-260
 *   PacketProvider.NormalizePacketIndex                                 Ogg/PacketProvider.cs:262-295
 * in the state the reference's reader is in once it has read every page of the stream.  The index copies what it needs;
 * `bytes` may be released after nvh_ogg_index_open returns. */
typedef struct nvh_ogg_index nvh_ogg_index;
int nvh_ogg_index_open(const uint8_t *bytes, size_t len, int stream_index, nvh_ogg_index **out);
void nvh_ogg_index_close(nvh_ogg_index *ix);
/* pages and packets of the stream, StreamPageReader.FirstDataPageIndex (-1: none), MaxGranulePosition, HasAllPages */
int nvh_ogg_index_info(const nvh_ogg_index *ix, int *npages, int *npackets, int *first_data_page, int64_t *max_granule,
                       int *has_all_pages);
/* StreamPageReader.GetPage (Ogg/StreamPageReader.cs:292-377): granule position, flags (1 resync, 2 continuation, 4 continued),
 * packet count, and the index (in nvh_ogg_demux_stream's packet list) of the first packet that starts on the page (-1: none) */
int nvh_ogg_index_page(const nvh_ogg_index *ix, int page, int64_t *granule, int *flags, int *packet_count, int *first_packet);
/* IPacketProvider.SeekTo(granulePos, preRoll, getPacketGranuleCount) (Ogg/PacketProvider.cs:56-72) with the stream's
 * StreamDecoder.GetPacketGranules (StreamDecoder.cs:630-647) as the callback: *packet_index = position in the packet list of the
 * packet GetNextPacket returns next, *granule_out = the method's return value.  NVH_ERR_ARGUMENT where the reference throws
 * ArgumentOutOfRangeException, NVH_ERR_INVALID_DATA for its InvalidDataExceptions, NVH_ERR_RUNTIME for an index fault. */
int nvh_ogg_seek(const nvh_ogg_index *ix, const nvh_stream *s, int64_t granule_pos, int pre_roll, int64_t *packet_index,
                 int64_t *granule_out);

/* ---- rows at one sample rate: a stateless polyphase resampler over rows of f32 samples ----
 * Every output row is a pure function of a window of source samples; nothing is carried from call to call, and no synthesis
 * call, emitting kernel or parser takes part.  THE RULE (a dozen lines of numpy reproduce it bit for bit):
 *   Ratio and width.  Source rate fi, target rate fo, g = gcd(fi, fo), L = fo / g (up), M = fi / g (down).
 *     half = 16 when L >= M, else (16 * M + L - 1) / L in integers; W = 16 * max(1, M / L) and sc = 0.94 * min(1, L / M) in reals.
 *   Taps.  A table h[L][2 * half] of f32: tap k of phase p lies at t = (k - half + 1) - p / L, with u = t / W, and
 *     h = sc * sinc(sc * t) * I0(9 * sqrt(1 - u * u)) / I0(9) for |u| < 1, else 0; sinc(x) = sin(pi x) / (pi x), 1 at 0; I0 by its
 *     power series to convergence.  Everything in double on the host, rounded once to f32.
 *   Output sample J of a clip (J counts from 0 in the clip resampled as a whole): n = J * M in 64 bits, c = n div L, p = n mod L;
 *     acc = +0.0f; for k = 0 .. 2 * half - 1 in this order: acc = fl(acc + fl(x[c - half + 1 + k] * h[p][k])) -- product and sum
 *     rounded separately, one accumulator.  x is the clip's f32 sample in the requested output form (after the mono mix or the
 *     channel map, after ClipSamples' clip, per output channel) and 0 outside [0, total).  (Skipping the terms whose x lies
 *     outside the clip gives the same bits.)
 *   Clip and format.  The result goes through ClipSamples' clip again (a band-limited filter overshoots), then, for NVH_PCM_S16,
 *     through the 16-bit conversion of nvh_stream_synth_pcm.
 *   Length.  total_out = (total * L + M - 1) / M.  A row [start, start + T) counts target-rate samples;
 *     valid = clamp(total_out - start, 0, T); the samples at and behind `valid` are zeros, as pads are, not filter ringing.
 *   Limits.  NVH_ERR_ARGUMENT for a rate below 1; NVH_ERR_UNSUPPORTED for L > 4096 or L * 2 * half > 262144.
 *
 * nvh_resample_plan: *up = L, *down = M, *half, *tap_count = L * 2 * half.  Host only; every output pointer is required.
 * nvh_resample_taps: the table exactly as the kernel uses it, phase after phase.  Host only.  *count is set even when `cap` is
 *   too small (NVH_ERR_ARGUMENT then).
 * nvh_resample_rows: `rows` rows of `length` (T) output samples per channel, asynchronous on the context's HIP stream.
 *   Element (row i, sample time e, channel c) of the source lies at d_src + i * src_row_stride + e * src_time_stride +
 *   c * src_chan_stride (f32), for e in [0, src_length); of the destination at d_dst + dst_row[i] * dst_row_stride + t *
 *   dst_time_stride + c * dst_chan_stride in elements of `format` -- interleaved, planar (C, N, T) and mono are stride choices.
 *   origin[i]: the source-sample index that element 0 of source row i holds; reads outside the row are 0.  start[i], valid[i]: as
 *   in the rule (0 <= valid[i] <= length; the row's samples from valid[i] on are written as zeros).  dst_row: the destination
 *   row of row i, or NULL for i.  d_clipped: NULL, or one int32 per DESTINATION row, zeroed by the caller; word dst_row[i]
 *   becomes non-zero when the second clip clamped a sample of that row (one lane per wavefront looks and sets, as HasClipped's
 *   word is set).  The four per-row arrays are host arrays, read during the call and uploaded in one copy; the device tap table
 *   is cached per context and (L, M).  Errors, before any device is touched: NVH_ERR_ARGUMENT for no descriptor, a rate below 1,
 *   rows / length / src_length below 0, channels below 1, an unknown format, a missing array or buffer with rows and length
 *   above 0, a start or an origin below 0 or with start + length above 2^48, a valid outside [0, length], a dst_row below 0;
 *   NVH_ERR_UNSUPPORTED as nvh_resample_plan; NVH_ERR_NO_GPU for no context.  The kernel owns NVH_RESAMPLE_TILE consecutive
 *   outputs of one (row, channel) per workgroup step. */
#define NVH_RESAMPLE_TILE 512
typedef struct nvh_resample_desc {
  int32_t in_rate, out_rate;
  int32_t rows;     /* N */
  int32_t channels; /* output channels per row (1 for the mono mix) */
  int32_t format;   /* NVH_PCM_* of the destination; the source is f32 */
  int32_t reserved; /* 0 */
  int64_t length;     /* T: output samples per row and channel */
  int64_t src_length; /* source samples per row and channel */
  int64_t src_row_stride, src_time_stride, src_chan_stride; /* in f32 elements */
  int64_t dst_row_stride, dst_time_stride, dst_chan_stride; /* in elements of `format` */
} nvh_resample_desc;
int nvh_resample_plan(int in_rate, int out_rate, int *up, int *down, int *half, int64_t *tap_count);
int nvh_resample_taps(int in_rate, int out_rate, float *taps, int64_t cap, int64_t *count);
int nvh_resample_rows(nvh_ctx *ctx, const nvh_resample_desc *desc, const float *d_src, void *d_dst, const int64_t *origin,
                      const int64_t *start, const int64_t *valid, const int32_t *dst_row, int32_t *d_clipped);
/* Diagnostics (like nvh_batch_kernels: which route a launch takes depends on the shape; the values are not part of the ABI):
 * what nvh_resample_rows would launch for `desc`, computed on the host by the code that launches it -- no context, no GPU.
 * out[4]: the tap table staged in LDS (0 | 1), tiles per row, workgroups per (row, channel), bytes of dynamic LDS.  Returns
 * what nvh_resample_rows returns for the descriptor alone (no buffer or array is looked at). */
int nvh_resample_route(const nvh_resample_desc *desc, int64_t *out);

/* ---- log-mel features of rows: a short-time transform, a mel filter bank and a logarithm over rows of f32 samples ----
 * Rows in, features out: every value is a pure function of one frame of one (row, channel); nothing is carried from call to
 * call, and no synthesis call, emitting kernel, parser or the resampler takes part.  Everything on the device is f32 with
 * separately rounded operations (fl(.) below; no fused multiply-add, IEEE division); every table is computed in double on the
 * host and rounded once to f32 (fl32(.)).  THE RULE (about 60 lines of numpy reproduce it bit for bit):
 *   Parameters.  rate R >= 1; n_fft N a power of two in [64, 4096]; win_length W in [1, N]; hop H in [1, 65536]; n_mels B in
 *     [1, 256]; doubles 0 <= f_min < f_max <= R / 2; mel_scale NVH_MEL_HTK or NVH_MEL_SLANEY; norm NVH_MEL_NORM_NONE or
 *     NVH_MEL_NORM_SLANEY; scale NVH_MEL_POWER, NVH_MEL_LN or NVH_MEL_DB; floor an f32 >= 2^-126 (1e-10 is the usual one);
 *     frames F >= 0; first an int64 that may be negative.  NVH_ERR_ARGUMENT for anything outside these (and, so that f * H +
 *     first stays inside 64 bits, for F above 2^40 or |first| above 2^60); there is no NVH_ERR_UNSUPPORTED case.
 *   Tables.  tw[k] = (cos(2 pi k / N), sin(2 pi k / N)) for k = 0 .. N/2.  win[n] = 0.5 - 0.5 cos(2 pi n / W) for n < W, the
 *     periodic Hann window (W = 1: the one sample is 0, taken as it is).  fb[b][k], b < B, k = 0 .. N/2: B + 2 points
 *     pt[i] = hz(m_lo + (m_hi - m_lo) * i / (B + 1)), equally spaced on the mel scale between m_lo = mel(f_min) and m_hi =
 *     mel(f_max); with l = pt[b], c = pt[b+1], r = pt[b+2] and f = k * R / N: fb = max(0, min((f - l) / (c - l), (r - f) /
 *     (r - c))), times 2 / (r - l) for NVH_MEL_NORM_SLANEY.  HTK: mel(f) = 2595 log10(1 + f / 700), hz(m) = 700 (10^(m / 2595)
 *     - 1).  Slaney: mel(f) = 3 f / 200 below 1000 Hz, 15 + ln(f / 1000) / (ln(6.4) / 27) from there on, hz its inverse.  A
 *     band that no bin falls into has an all-zero row: its value is 0, the floor in the log scales; that is not an error.
 *   Frame f of a (row, channel).  u = N zeros, then u[(N - W) div 2 + n] = fl(x[f * H + first + n] * win[n]) for n < W, x the
 *     row's f32 sample and 0 outside [0, valid) of the row.
 *   Transform.  z[n] = u[2n] + i u[2n+1], n < N/2, through an N/2-point radix-2 decimation-in-time FFT: input in bit-reversed
 *     order, then stages with half = 1, 2, .., N/4; in each the pair (a, b) at distance `half`, a at index j inside its group
 *     of 2 * half, takes (c, s) = tw[j * N / (2 * half)]:  tr = fl(fl(br c) + fl(bi s)), ti = fl(fl(bi c) - fl(br s)),
 *     a' = (fl(ar + tr), fl(ai + ti)), b' = (fl(ar - tr), fl(ai - ti)).
 *   Split, k = 0 .. N/2.  a = Z[k mod N/2], b = conj(Z[(N/2 - k) mod N/2]); er = fl(ar + br), ei = fl(ai + bi), dr = fl(ar -
 *     br), di = fl(ai - bi); with (c, s) = tw[k]: tr = fl(fl(c di) - fl(s dr)), ti = -fl(fl(c dr) + fl(s di)), xr = fl(er +
 *     tr), xi = fl(ei + ti); P[k] = fl(0.25 fl(fl(xr xr) + fl(xi xi))) -- the power of bin k of the frame's N-point transform.
 *   Mel.  m[b]: acc = +0; for k rising over the bins with fb[b][k] != 0: acc = fl(acc + fl(P[k] fb[b][k])).  One accumulator.
 *     (The non-zero bins of a band are consecutive; the kernel reads them as first bin, count and weights.)
 *   Scale.  NVH_MEL_POWER: m.  NVH_MEL_LN: ln_r(max(m, floor)).  NVH_MEL_DB: fl(ln_r(max(m, floor)) * fl32(10 / ln 10)).
 *     ln_r(v), the rule's own logarithm (a device library's logf is not reproducible): v = g 2^e with g in [0.5, 1); if g <
 *     fl32(0.70710678) then g = 2 g, e = e - 1; s = fl(fl(g - 1) / fl(g + 1)), z = fl(s s); p = fl32(1/11), then for c in
 *     fl32(1/9), fl32(1/7), fl32(1/5), fl32(1/3), 1: p = fl(fl(p z) + c); ln_r = fl(fl(float(e) * fl32(0.6931471805599453)) +
 *     fl(fl(s + s) * p)).  Within 4 ulp of the logarithm over [1e-10, 1e8] (tests/test_mel_plan.py).
 *
 * nvh_mel_plan: validates the parameters and returns the table sizes: *twiddle_count = 2 * (N/2 + 1), *window_count = W,
 *   *bank_count = B * (N/2 + 1).  Host only; every pointer is required.
 * nvh_mel_tables: the tables exactly as the kernel uses their values -- twiddles as (cos, sin) pairs, the window, the bank
 *   dense, band after band.  Host only.  The three counts are set even when a cap is too small (NVH_ERR_ARGUMENT then); a
 *   table whose pointer is NULL with cap 0 is left out.
 * nvh_mel_rows: `rows` rows of `channels` channels, F frames each, asynchronous on the context's HIP stream.  Element (row i,
 *   sample time e, channel c) of the source lies at d_src + i * src_row_stride + e * src_time_stride + c * src_chan_stride
 *   (f32), for e in [0, src_length) -- interleaved, planar and mono are stride choices, as in nvh_resample_desc; value (row i,
 *   channel c, frame f, band b) is written to d_dst + i * dst_row_stride + c * dst_chan_stride + f * dst_frame_stride + b *
 *   dst_band_stride (f32), so that [N, C, F, B] and [N, C, B, F] are stride choices too.  valid: NULL (every row counts
 *   src_length samples), or a host array of one int64 per row in [0, src_length], read during the call and uploaded in one
 *   copy: reads at and behind valid[i] are 0.  The device tables are cached per context and parameter set.  Errors, before
 *   any device is touched: NVH_ERR_ARGUMENT for no descriptor, a parameter outside the rule's, rows / src_length below 0,
 *   channels outside [1, 65535], a missing buffer with rows and F above 0, a valid[i] outside [0, src_length]; then
 *   NVH_ERR_NO_GPU for no context.  The kernel: one wavefront per frame, NVH_MEL_FRAMES consecutive frames of one (row,
 *   channel) per workgroup. */
#define NVH_MEL_HTK 0
#define NVH_MEL_SLANEY 1
#define NVH_MEL_NORM_NONE 0
#define NVH_MEL_NORM_SLANEY 1
#define NVH_MEL_POWER 0
#define NVH_MEL_LN 1
#define NVH_MEL_DB 2
#define NVH_MEL_FRAMES 4
typedef struct nvh_mel_desc {
  int32_t rate, n_fft, win_length, hop, n_mels;
  int32_t mel_scale, norm, scale; /* NVH_MEL_* */
  float floor;
  int32_t rows;     /* N */
  int32_t channels; /* channels per row (1 for the mono mix) */
  int32_t reserved; /* 0 */
  double f_min, f_max;
  int64_t frames; /* F: frames per row and channel */
  int64_t first;  /* frame f begins at sample f * hop + first of its row */
  int64_t src_length; /* source samples per row and channel */
  int64_t src_row_stride, src_time_stride, src_chan_stride;                    /* in f32 elements */
  int64_t dst_row_stride, dst_chan_stride, dst_frame_stride, dst_band_stride; /* in f32 elements */
} nvh_mel_desc;
int nvh_mel_plan(const nvh_mel_desc *desc, int64_t *twiddle_count, int64_t *window_count, int64_t *bank_count);
int nvh_mel_tables(const nvh_mel_desc *desc, float *twiddle, float *window, float *bank, int64_t twiddle_cap, int64_t window_cap,
                   int64_t bank_cap, int64_t *twiddle_count, int64_t *window_count, int64_t *bank_count);
int nvh_mel_rows(nvh_ctx *ctx, const nvh_mel_desc *desc, const float *d_src, float *d_dst, const int64_t *valid);

/* ---- the front of a frame: DC removal, pre-emphasis, other windows, reflect padding, triangles linear in mel ----
 * The front of a frame is everything between the row's samples and u[0 .. N) of nvh_mel_rows' rule; a second descriptor,
 * nvh_mel_front, chooses it.  Every field at today's value (NVH_WIN_HANN, NVH_TRI_HZ, NVH_PAD_ZERO, remove_dc 0, preemphasis 0,
 * gain 1), or no nvh_mel_front at all, is nvh_mel_rows' rule and nvh_mel_rows' kernel.  As there: every operation is a separately
 * rounded f32 instruction (fl(.)), every table is computed in double and rounded once (fl32(.)).  THE RULE OF THE FRONT (about 40
 * more lines of numpy):
 *   Parameters.  window one of NVH_WIN_*; triangles NVH_TRI_HZ or NVH_TRI_MEL; pad_mode NVH_PAD_ZERO or NVH_PAD_REFLECT; remove_dc
 *     0 or 1; preemphasis p a finite f32 in [0, 1] (0: none); gain g a finite f32 > 0 (1: none); reserved 0.  NVH_ERR_ARGUMENT
 *     for anything else.
 *   Tables.  win[n], n < W.  NVH_WIN_HANN: nvh_mel_rows' periodic Hann, 0.5 - 0.5 cos(2 pi n / W).  The others are symmetric, with
 *     the denominator D = W - 1 (W = 1: D = 1): NVH_WIN_HANN_SYM 0.5 - 0.5 cos(2 pi n / D); NVH_WIN_HAMMING 0.54 - 0.46 cos(2 pi n
 *     / D); NVH_WIN_POVEY (0.5 - 0.5 cos(2 pi n / D))^0.85, the power taken in double on the host; NVH_WIN_RECT 1.
 *     fb[b][k] under NVH_TRI_MEL: B + 2 points pm[i] = m_lo + (m_hi - m_lo) * i / (B + 1), equally spaced on the mel scale
 *     between m_lo = mel(f_min) and m_hi = mel(f_max) and NOT mapped back to Hz; with l = pm[b], c = pm[b+1], r = pm[b+2] and m =
 *     mel(k * R / N): fb = max(0, min((m - l) / (c - l), (r - m) / (r - c))), times 2 / (hz(r) - hz(l)) for NVH_MEL_NORM_SLANEY
 *     (the normalisation keeps its Hz definition).  mel and hz are those of mel_scale.  The non-zero bins of a band are
 *     consecutive here too.  NVH_TRI_HZ: nvh_mel_rows' bank.  The twiddles do not depend on the front.
 *   Frame f of a (row, channel).  For n < W, t = f * H + first + n is mapped first:
 *     NVH_PAD_REFLECT, with L = src_length: t < 0 -> -t; t >= L -> 2 (L - 1) - t.  One reflection must be enough for every frame
 *       of the call: L >= 2, -first <= L - 1 and (F - 1) H + first + W - 1 <= 2 (L - 1), else NVH_ERR_ARGUMENT (a call with F = 0
 *       has no frame and passes).  NVH_PAD_ZERO: t stays.
 *     x[n] = the row's f32 sample at the mapped t, and 0 where the mapped t lies outside [0, valid) of the row: the zeroing comes
 *       after the reflection, so a reflected read can land in the zeros behind `valid`.
 *     s[n] = fl(x[n] * g); with g == 1, s[n] = x[n] (which is the same bits).
 *     remove_dc: mean = fl(sum64(s[0 .. W)) / fl32(W)), then s[n] = fl(s[n] - mean) for every n < W.  sum64 is the summation of
 *       nvh_fnorm_rows' rule below: 64 partials, element e into partial e mod 64 in rising e, then the six halvings.
 *     y[n] = s[n] with p == 0.  With p > 0: y[n] = fl(s[n] - fl(p * s[n-1])) for 1 <= n < W, and y[0] = fl(s[0] - fl(p * s[0]))
 *       -- Kaldi's pre-emphasis.  It reads the values s (after the DC removal), never y: it is not recursive.
 *     u = N zeros, then u[(N - W) div 2 + n] = fl(y[n] * win[n]) for n < W.  (The window stays centred in N; Kaldi puts it at the
 *     start of the buffer, which changes the phase of the transform and not its power.)
 *   Transform, Split, Mel and Scale are nvh_mel_rows' text, unchanged.
 *   Kaldi's fbank (dither 0, no energy column) is: g = 32768, remove_dc, p = 0.97, NVH_WIN_POVEY, NVH_TRI_MEL with NVH_MEL_HTK
 *   (Kaldi's 1127 ln(1 + f / 700) is the HTK scale, and the bank holds only ratios of mel differences), NVH_MEL_LN with floor =
 *   2^-23, first = 0 and F = (L - W) div H + 1.  torch.stft's default padding and Whisper's front end are NVH_PAD_REFLECT with
 *   first = (N - W) div 2 - N div 2.
 *
 * nvh_mel_front_check: NVH_OK or NVH_ERR_ARGUMENT for the pair (desc's rule parameters as nvh_mel_plan checks them, the front's
 *   fields, and under NVH_PAD_REFLECT with F > 0 the three conditions above from desc's src_length, first, frames, hop and
 *   win_length).  front == NULL checks desc alone.  Host only.
 * nvh_mel_tables_front: nvh_mel_tables with the front's window and triangles (front == NULL: nvh_mel_tables).  Host only.
 * nvh_mel_rows_front: nvh_mel_rows with the front.  front == NULL or a front with every field at today's value IS nvh_mel_rows:
 *   the same kernel instance, LDS, grid and bits.  Errors as nvh_mel_rows, nvh_mel_front_check's among the argument errors, all
 *   before NVH_ERR_NO_GPU.  The kernel: a front variant of k_mel_rows; the span staging applies the reflection, the zeroing and
 *   the gain, the frame's wavefront sums its mean (partial l in lane l, the halvings across lanes) and the window step recomputes
 *   s[n-1] from the span.  No LDS is added, so a parameter set is staged with a front exactly when it is without. */
#define NVH_WIN_HANN 0
#define NVH_WIN_HANN_SYM 1
#define NVH_WIN_HAMMING 2
#define NVH_WIN_POVEY 3
#define NVH_WIN_RECT 4
#define NVH_TRI_HZ 0
#define NVH_TRI_MEL 1
#define NVH_PAD_ZERO 0
#define NVH_PAD_REFLECT 1
typedef struct nvh_mel_front {
  int32_t window;      /* NVH_WIN_* */
  int32_t triangles;   /* NVH_TRI_* */
  int32_t pad_mode;    /* NVH_PAD_* */
  int32_t remove_dc;   /* 0 | 1 */
  float preemphasis;   /* p, a finite f32 in [0, 1]; 0: none */
  float gain;          /* g, a finite f32 > 0; 1: none */
  int32_t reserved[2]; /* 0 */
} nvh_mel_front;
int nvh_mel_front_check(const nvh_mel_desc *desc, const nvh_mel_front *front);
int nvh_mel_tables_front(const nvh_mel_desc *desc, const nvh_mel_front *front, float *twiddle, float *window, float *bank,
                         int64_t twiddle_cap, int64_t window_cap, int64_t bank_cap, int64_t *twiddle_count, int64_t *window_count,
                         int64_t *bank_count);
int nvh_mel_rows_front(nvh_ctx *ctx, const nvh_mel_desc *desc, const nvh_mel_front *front, const float *d_src, float *d_dst,
                       const int64_t *valid);
/* Diagnostics (like nvh_resample_route; the values are not part of the ABI): what nvh_mel_rows_front would launch for `desc`
 * and `front` (NULL: nvh_mel_rows), on the host -- no context, no GPU; the bank is built for its size.  out[6]: tables and span
 * staged in LDS (0 | 1), floats of the staged span (0: none), bytes of dynamic LDS, workgroups, whether the kernel instance with
 * the front runs (0: nvh_mel_rows' own, the tables alone differ), floats of the sparse bank.  Returns what nvh_mel_rows_front
 * returns for the two descriptors alone (no buffer or array is looked at). */
int nvh_mel_route(const nvh_mel_desc *desc, const nvh_mel_front *front, int64_t *out);

/* ---- per-row normalisation of features: mean, variance or peak of each (row, channel), and the fill of its padded frames ----
 * Features in, features out: every value is a pure function of one (row, channel) of the input and of that row's frame count;
 * nothing is carried from call to call, and nvh_mel_rows takes no part.  (fnorm: NVH_MEL_NORM_* is the bank's normalisation.)
 * Everything on the device is f32 with separately rounded operations (fl(.) below; no fused multiply-add); division and square
 * root are the correctly rounded ones.  THE RULE (about 40 lines of numpy reproduce it bit for bit):
 *   Input.  x[i, c, f, b] for row i < rows, channel c < channels, frame f < F, band b < B, and vf[i] in [0, F], the number of
 *     counted frames of row i: valid_frames[i], or F for every row when valid_frames is NULL.  B in [1, 256], F in [0, 2^24],
 *     channels in [1, 65535], rows >= 0.  Inputs are finite or +-inf; a NaN makes the values of its group unspecified (it is
 *     not an error, and nothing faults).
 *   sum64(v[0 .. n)), the one summation.  64 partials p[l] = +0; for e = l, l + 64, l + 128, .. < n, rising: p[l] = fl(p[l] +
 *     v[e]); then for d = 32, 16, 8, 4, 2, 1: p[l] = fl(p[l] + p[l + d]) for every l < d; the result is p[0].  (numpy: pad to a
 *     multiple of 64 with zeros, reshape to (-1, 64), add the rows in order, then six halvings.)  Within (ceil(n / 64) + 6) *
 *     2^-24 * sum |v| of the exact sum (tests/test_fnorm_plan.py).
 *   Groups, by axis.  NVH_FNORM_PER_BAND: one group per (i, c, b); S1 = sum64 over f < vf[i] of x[i, c, f, b], n = vf[i].
 *     NVH_FNORM_ALL: one group per (i, c); the per-band sum64 results S_b are added in rising b into one accumulator, acc = +0,
 *     acc = fl(acc + S_b); S1 = acc, n = vf[i] * B.  (The order does not depend on the memory layout.)
 *   Modes.  mean = fl(S1 / fl32(n)), fl32(n) the integer rounded to nearest.
 *     NVH_FNORM_NONE: y = x.  NVH_FNORM_MEAN: y = fl(x - mean).
 *     NVH_FNORM_MEAN_VAR: d = fl(x - mean), q = fl(d d); S2 the same sums over q (per band, and for NVH_FNORM_ALL the bands'
 *       results added in rising b); var = fl(S2 / fl32(n)), the population variance; sd = sqrt(fl(var + eps)); y = fl(d / sd).
 *       eps is an f32 >= 2^-126.
 *     NVH_FNORM_PEAK: the group is (i, c) whatever the axis.  mx = the maximum of x over the counted frames and all bands
 *       (exact: its order is free); t = fl(mx - range); y = fl(fl(max(x, t) + offset) * gain).  range an f32 >= 0 or +inf,
 *       offset and gain finite.  On dB features range = 80, offset = 40, gain = fl32(1 / 40) is Whisper's normalisation.
 *   Pad.  Every (i, c, f >= vf[i], b) gets pad_value, a finite f32; a row with vf = 0 is all pad_value.
 *
 * nvh_fnorm_check: NVH_OK or NVH_ERR_ARGUMENT for the descriptor's numbers (below).  Host only.
 * nvh_fnorm_rows: asynchronous on the context's HIP stream.  x[i, c, f, b] lies at d_src + i * src_row_stride + c *
 *   src_chan_stride + f * src_frame_stride + b * src_band_stride, y at d_dst with the dst strides (f32 elements): [N, C, B, F]
 *   and [N, C, F, B] are stride choices, on each side independently.  d_dst == d_src with identical strides is the in-place
 *   form (only the last pass writes); any other overlap of the two is the caller's error and gives unspecified values.
 *   valid_frames: NULL, or a host array of one int64 per row, read during the call and uploaded in one copy.  Errors, before any
 *   device is touched: NVH_ERR_ARGUMENT for no descriptor; a mode or axis that is none of the constants (the axis is checked in
 *   every mode); rows, channels, F or B outside the limits above; a pad_value that is not finite (in every mode, with or without
 *   valid_frames); in NVH_FNORM_MEAN_VAR an eps that is not a finite f32 >= 2^-126; in NVH_FNORM_PEAK a range that is negative or
 *   NaN, an offset or gain that is not finite (a field its mode does not use is not looked at); a missing buffer with rows and F
 *   above 0; a valid_frames[i] outside [0, F].  Then NVH_ERR_NO_GPU for no context.  There is no NVH_ERR_UNSUPPORTED case.
 *   The kernel: a workgroup per (row, channel), a wavefront per band, partial p[l] in lane l.  A (row, channel) of at most
 *   NVH_FNORM_RESIDENT_FLOATS floats, counted as (F | 1) * B, is read once and normalised out of LDS; a larger one re-reads its
 *   source for the second sum and for the last pass. */
#define NVH_FNORM_NONE 0
#define NVH_FNORM_MEAN 1
#define NVH_FNORM_MEAN_VAR 2
#define NVH_FNORM_PEAK 3
#define NVH_FNORM_PER_BAND 0
#define NVH_FNORM_ALL 1
#define NVH_FNORM_RESIDENT_FLOATS 19952
typedef struct nvh_fnorm_desc {
  int32_t mode, axis; /* NVH_FNORM_* */
  int32_t rows;       /* N */
  int32_t channels;   /* channels per row */
  int32_t frames;     /* F: frames per row and channel */
  int32_t bands;      /* B */
  float eps;          /* NVH_FNORM_MEAN_VAR */
  float pad_value;
  float range, offset, gain; /* NVH_FNORM_PEAK */
  int32_t reserved;          /* 0 */
  int64_t src_row_stride, src_chan_stride, src_frame_stride, src_band_stride; /* in f32 elements */
  int64_t dst_row_stride, dst_chan_stride, dst_frame_stride, dst_band_stride; /* in f32 elements */
} nvh_fnorm_desc;
int nvh_fnorm_check(const nvh_fnorm_desc *desc);
int nvh_fnorm_rows(nvh_ctx *ctx, const nvh_fnorm_desc *desc, const float *d_src, float *d_dst, const int64_t *valid_frames);
/* Diagnostics (like nvh_resample_route; the values are not part of the ABI): what nvh_fnorm_rows would launch for `desc`, on the
 * host -- no context, no GPU.  out[3]: normalised out of LDS (0: re-reading), bytes of dynamic LDS, workgroups.  Returns what
 * nvh_fnorm_rows returns for the descriptor alone (no buffer or array is looked at). */
int nvh_fnorm_route(const nvh_fnorm_desc *desc, int64_t *out);

/* ---- cepstra and deltas of features: a DCT-II over the bands with an optional lifter, and delta / delta-delta columns ----
 * Features in, features out: every value is a pure function of a few frames of one (row, channel) of the input and of that row's
 * frame count; nothing is carried from call to call, and neither nvh_mel_rows nor nvh_fnorm_rows takes part (the stage sits
 * between them: MFCCs as Kaldi's compute-mfcc-feats and torchaudio.transforms.MFCC make them, deltas as Kaldi's add-deltas and
 * torchaudio.functional.compute_deltas).  Everything on the device is f32 with separately rounded operations (fl(.) below; no
 * fused multiply-add); every table is computed in double on the host and rounded once to f32 (fl32(.)).  THE RULE (about 40
 * lines of numpy reproduce it bit for bit):
 *   Input.  x[i, c, f, b] for row i < rows, channel c < channels, frame f < F, band b < B, and vf[i] in [0, F], the number of
 *     counted frames of row i: valid_frames[i], or F for every row when valid_frames is NULL.  B in [1, 256], F in [0, 2^24],
 *     channels in [1, 65535], rows >= 0.  Inputs are finite; anything else gives unspecified values (it is not an error, and
 *     nothing faults).
 *   Parameters.  transform: NVH_CEP_NONE (then K = B, `ceps` must say so, and c = x, the input's bits) or NVH_CEP_DCT2 with
 *     ceps K in [1, B].  dct_norm: NVH_CEP_ORTHO or NVH_CEP_PLAIN.  lifter Lf: a finite f32 >= 0; 0: none.  order o in {0, 1, 2}.
 *     window N in [1, 8].  dct_norm, lifter and window are checked whatever transform and order are.  The output has
 *     Q = (1 + o) * K columns, and Q <= 256 (so that nvh_fnorm_rows takes the result).  reserved is 0.  NVH_ERR_ARGUMENT for
 *     anything else; there is no NVH_ERR_UNSUPPORTED case.
 *   Tables.  D[k][b] = fl32(w_k * lift_k * cos(pi * (b + 0.5) * k / B)) for k < K, b < B, in double and in this order of
 *     operations: the product (w_k * lift_k) times the cosine of ((pi * (b + 0.5)) * k) / B.  NVH_CEP_ORTHO: w_0 = sqrt(1 / B),
 *     w_k = sqrt(2 / B) for k > 0 -- Kaldi's DCT matrix, torchaudio's norm="ortho".  NVH_CEP_PLAIN: w_k = 2 for every k --
 *     torchaudio's norm=None.  lift_k = 1 + (0.5 * Lf) * sin((pi * k) / Lf), Kaldi's cepstral_lifter; 1 when Lf = 0.  The lifter
 *     is folded into the table: Kaldi multiplies the cepstra by lift_k afterwards, which is the same mathematics and one more
 *     rounding.
 *     Delta scales, with d = 2 * sum_{i = 1 .. N} i^2 (an integer):  s_1[j] = fl32(j / d) for j = -N .. N;  s_2[j] = fl32(n_j /
 *     d^2) for j = -2N .. 2N, n_j = the sum over i of i * (j - i) with both |i| <= N and |j - i| <= N (an integer): the full
 *     convolution of s_1 with itself, taken in double as one division of integers and rounded once.
 *   Cepstra.  c[f][k] for every f < F: acc = +0; for b rising over all B: acc = fl(acc + fl(x[f][b] * D[k][b])).  One
 *     accumulator.
 *   Deltas.  For order m = 1 .. o and frame f < n = vf[i]: acc = +0; for j rising over the j in [-m N, m N] with s_m[j] != 0:
 *     acc = fl(acc + fl(c[clamp(f + j, 0, n - 1)][k] * s_m[j])).  This is Kaldi's composite filter with the edge frames repeated:
 *     one pass over the cepstra, never a delta of computed deltas.  First-order values are compute_deltas' with its replicate
 *     padding; second-order values differ from torchaudio's twice-applied form only in the 2N frames at each end (there the
 *     second application sees deltas of repeated frames, the composite filter repeated cepstra).  For f >= n the delta columns
 *     are +0.
 *   Output.  y[i, c, f, m * K + k], m = 0 .. o: the statics first, then the deltas, then the delta-deltas -- Kaldi's column
 *     order.  The static columns are written for every f < F: the pad frames' statics are the transform of whatever x holds there.
 *
 * nvh_cep_check: NVH_OK or NVH_ERR_ARGUMENT for the descriptor's numbers.  Host only.
 * nvh_cep_plan: nvh_cep_check, and the table sizes: *dct_count = K * B (0 under NVH_CEP_NONE), *scale_count = 6 N + 2.  Host
 *   only; every pointer is required.
 * nvh_cep_tables: the tables exactly as the kernel uses their values -- D row after row (k, then b), and the scales, s_1's 2 N + 1
 *   then s_2's 4 N + 1.  Host only.  Both counts are set even when a cap is too small (NVH_ERR_ARGUMENT then); a table whose
 *   pointer is NULL with cap 0 is left out.
 * nvh_cep_rows: asynchronous on the context's HIP stream.  x[i, c, f, b] lies at d_src + i * src_row_stride + c *
 *   src_chan_stride + f * src_frame_stride + b * src_band_stride, y[i, c, f, q] at d_dst + i * dst_row_stride + c *
 *   dst_chan_stride + f * dst_frame_stride + q * dst_col_stride (f32 elements): [N, C, Q, F] and [N, C, F, Q] are stride
 *   choices, on each side independently.  Out of place only: any overlap of the two buffers is the caller's error and gives
 *   unspecified values.  valid_frames: NULL, or a host array of one int64 per row, read during the call and uploaded in one
 *   copy.  The device tables are cached per context and parameter set.  Errors, before any device is touched and in this order:
 *   NVH_ERR_ARGUMENT for no descriptor; a transform, dct_norm, order or window that is none of the above; rows, channels, F or B
 *   outside the limits; a K outside [1, B], or other than B under NVH_CEP_NONE; Q above 256; a lifter that is negative or not
 *   finite; a reserved word that is not 0; a missing buffer with rows and F above 0; a valid_frames[i] outside [0, F]; more than
 *   2^63 - 1 work items (rows * channels * tiles).  Then NVH_ERR_NO_GPU for no context.
 *   The kernel: a workgroup takes NVH_CEP_FRAMES consecutive frames of one (row, channel) at a time, with o * N more frames on
 *   each side (clamped as the rule clamps); it stages them in LDS, computes their cepstra into LDS, forms the deltas from there
 *   and writes the Q columns along the destination's smaller stride.  The DCT table lies in LDS where it fits the workgroup's
 *   80 KB beside the frames, and is read through the caches where it does not. */
#define NVH_CEP_NONE 0
#define NVH_CEP_DCT2 1
#define NVH_CEP_ORTHO 0
#define NVH_CEP_PLAIN 1
#define NVH_CEP_FRAMES 24
#define NVH_CEP_MAX_WINDOW 8
typedef struct nvh_cep_desc {
  int32_t transform, dct_norm; /* NVH_CEP_* */
  int32_t order;               /* o: 0 statics alone, 1 + deltas, 2 + delta-deltas */
  int32_t window;              /* N */
  int32_t rows;                /* rows of the batch */
  int32_t channels;            /* channels per row */
  int32_t frames;              /* F: frames per row and channel */
  int32_t bands;               /* B */
  int32_t ceps;                /* K */
  float lifter;                /* Lf; 0: none */
  int32_t reserved[2];         /* 0 */
  int64_t src_row_stride, src_chan_stride, src_frame_stride, src_band_stride; /* in f32 elements */
  int64_t dst_row_stride, dst_chan_stride, dst_frame_stride, dst_col_stride;  /* in f32 elements */
} nvh_cep_desc;
int nvh_cep_check(const nvh_cep_desc *desc);
int nvh_cep_plan(const nvh_cep_desc *desc, int64_t *dct_count, int64_t *scale_count);
int nvh_cep_tables(const nvh_cep_desc *desc, float *dct, float *scales, int64_t dct_cap, int64_t scale_cap, int64_t *dct_count,
                   int64_t *scale_count);
int nvh_cep_rows(nvh_ctx *ctx, const nvh_cep_desc *desc, const float *d_src, float *d_dst, const int64_t *valid_frames);
/* Diagnostics (like nvh_resample_route; the values are not part of the ABI): what nvh_cep_rows would launch for `desc`, on the
 * host -- no context, no GPU.  out[4]: the DCT table staged in LDS (0: read through the caches, or no table at all under
 * NVH_CEP_NONE), bytes of dynamic LDS, workgroups, tiles per (row, channel).  Returns what nvh_cep_rows returns for the
 * descriptor alone (no buffer or array is looked at). */
int nvh_cep_route(const nvh_cep_desc *desc, int64_t *out);

/* ---- multi-GPU: the gather of the file-parallel corpus transcode (SURVEY 8 e) ----
 * StreamDecoder holds per-stream state only (StreamDecoder.cs:35-39), so a corpus shards by file: every process decodes its
 * files on its own GPU (one nvh_ctx per process) and the PCM is gathered on one of them -- the path's one collective, through
 * RCCL over xGMI.  Python callers have nvorbis_amd.corpus (torch.distributed); these entry points are the same exchange for a
 * host without it (the C# host: INTEGRATION.md, "Eight GPUs").  RCCL is loaded on first use (dlopen); NVH_ERR_UNSUPPORTED when
 * it is not installed, NVH_ERR_DEVICE for an RCCL failure (nvh_last_hip_error() = 10000 + its ncclResult_t).
 *   nvh_comm_unique_id   rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other processes by whatever
 *                        means the host has (a file, a socket, its job launcher);
 *   nvh_comm_create      every rank, with the same id (ncclCommInitRank on the context's device; collective: returns when
 *                        all `world` ranks have called it);
 *   nvh_comm_allgather_i64  `n` 64-bit words per rank -- e.g. the number of floats of each file it decoded -- to every rank
 *                        (host arrays: mine[n], all[world * n], rank-major);
 *   nvh_comm_gather_pcm  rank r's `send_count` floats at d_send (HBM) arrive at d_recv + sum(counts[0..r-1]) on `root`
 *                        (d_recv: HBM, sum(counts) floats, ignored elsewhere); counts[world] = every rank's total, the same on every rank.  One
 *                        group of point-to-point transfers on the context's stream, waited for.  The root's own part is a
 *                        device copy; NVH_GATHER_SELF_P2P sends it through RCCL as well (a one-rank check of the
 *                        point-to-point path on a single GPU). */
#define NVH_COMM_ID_BYTES 128
#define NVH_GATHER_SELF_P2P 1
typedef struct nvh_comm nvh_comm;
int nvh_comm_unique_id(uint8_t *id);
int nvh_comm_create(nvh_ctx *ctx, const uint8_t *id, int rank, int world, nvh_comm **out);
void nvh_comm_destroy(nvh_comm *comm);
int nvh_comm_info(const nvh_comm *comm, int *rank, int *world);
int nvh_comm_allgather_i64(nvh_comm *comm, const int64_t *mine, int n, int64_t *all);
int nvh_comm_gather_pcm(nvh_comm *comm, const float *d_send, int64_t send_count, float *d_recv, const int64_t *counts,
                        int root, int flags);

#ifdef __cplusplus
}
#endif
#endif /* NVORBIS_HIP_H */

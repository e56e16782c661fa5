"""Clip batches: many short Ogg Vorbis files of one encoder setup, decoded as segments of shared batches.

A sound-effect bank, a set of speech clips or a dataset shard is thousands of short streams with byte-identical
identification and setup headers.  One stream per clip pays for its setup upload, at least two launches, a synchronisation and
a read-back per clip; here every group of clips with the same setup is ONE stream, each clip a segment of it
(Stream.next_segment, include/nvorbis_hip.h), and a batch of `batch_frames` frames -- however many clips that is -- goes
through one upload, one parse and one set of launches.

decode_clip_rows is the fixed-length form a dataset loader wants: a crop [start, start + length) of every clip, zero-padded
where the clip is shorter, N rows in one tensor.  Every row is a WINDOWED segment (Stream.segment_window): only the packets the
crop needs are pushed, the parser cuts the first and the last frame's emission, and the pad is written with the batch.
"""
import collections
import contextlib
import ctypes as C
import dataclasses

import numpy as np

from . import native
from .reader import (Context, Stream, _channel_map, _enable_gpu_parse, _layout, _mix, _pcm_format, _pcm_out, _sample_format,
                     demux_ogg_array)


def _return_clipped(value):
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError("return_clipped must be True or False, not %r" % (value,))
    return bool(value)


def _length(value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
        raise ValueError("length must be an int >= 0, not %r" % (value,))
    return int(value)


def _batch_frames(value):
    if int(value) < 1:
        raise ValueError("batch_frames must be at least 1")
    return int(value)


def _starts(starts, n):
    """One start per clip as a list of ints; None: 0 for every clip."""
    if starts is None:
        return [0] * n
    starts = list(starts)
    if len(starts) != n:
        raise ValueError("starts must name one start per clip (%d for %d clips)" % (len(starts), n))
    for v in starts:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("starts must be ints >= 0, not %r" % (v,))
    return [int(v) for v in starts]


@contextlib.contextmanager
def _context(ctx, device):
    """The caller's Context, or one of its own on `device` that is closed on every way out of the block."""
    if ctx is not None:
        yield ctx
        return
    ctx = Context(device)
    try:
        yield ctx
    finally:
        ctx.close()


@dataclasses.dataclass
class _Form:
    """The output form of one public call: what every batch is synthesised as and where it goes."""
    dtype: np.dtype  # of a sample: float32 or int16
    planar: bool
    mix: object
    channel_map: object
    batch_frames: int
    gpu_parse: bool
    device_out: bool
    device: int
    align: int = None  # clip batches only
    clipped: object = None  # the caller's bool array over all clips or rows, or None: not asked for

    def map(self, ch):
        """The map of a stream of `ch` channels ("wave" depends on the count)."""
        return _channel_map(self.channel_map, ch, self.mix)

    def och(self, ch):
        """The samples per sample time that a stream of `ch` channels leaves."""
        return _pcm_out(self.dtype, self.planar, self.mix, self.channel_map, ch)[2]

    def torch_dtype(self):
        import torch
        return torch.int16 if self.dtype == np.dtype(np.int16) else torch.float32

    def row_shape(self, rows, t, och):
        return (och, rows, t) if self.planar else (rows, t) if self.mix is not None else (rows, t, och)

    def row_strides(self, rows, t, och):
        """(row, sample time, channel) in elements."""
        return (t, 1, rows * t) if self.planar else (t, 1, 0) if self.mix is not None else (t * och, och, 1)

    def f32(self):
        """The same form in float32: the resampler's source rows."""
        return dataclasses.replace(self, dtype=np.dtype(np.float32))


_Clip = collections.namedtuple("_Clip", "packets key channels rate index")


def _load_clips(clips, call, sample_rate=None, want_index=False, form=None):
    """One _Clip per clip (bytes or a path), on the host: its PacketArray, its setup key (identification and setup packet), the
    stream's channels and rate, and with want_index what Stream.index_packets says of its audio packets (else None).  Clip by
    clip, before the next one is looked at: NvhError for its headers as clip i of `call`, then, with a form, ValueError for a
    channel map that does not fit it, then ValueError for a rate the resampler does not take to `sample_rate`."""
    recs = []
    for i, src in enumerate(clips):
        if isinstance(src, (bytes, bytearray, memoryview)):
            data = bytes(src)
        else:
            with open(src, "rb") as fh:
                data = fh.read()
        try:
            pa = demux_ogg_array(data, 0)
            if len(pa) < 3:
                raise native.NvhError(native.ERR_NOT_VORBIS, call)
            # every clip's own three headers are looked at, on the host (a setup seen before on this thread is not parsed again)
            key = (pa[0], pa[2])
            probe = Stream(None, key[0], pa[1], key[1])
            try:
                rec = _Clip(pa, key, probe.channels, probe.sample_rate, probe.index_packets(pa, 3) if want_index else None)
            finally:
                probe.close()
        except native.NvhError as e:
            raise _clip_error(i, e, "headers", call)
        if form is not None:
            form.och(rec.channels)
        if sample_rate is not None and rec.rate != sample_rate:
            resample_plan(rec.rate, sample_rate)
        recs.append(rec)
    return recs


def _note_clipped(st, members, clipped):
    """OR the last batch's per-segment flags (Stream.synth_segments_clipped) into `clipped`, segment k being clip members[k]."""
    for k, hit in zip(st.synth_segments()[:, 0], st.synth_segments_clipped()):
        if hit:
            clipped[members[int(k)]] = True


def _clip_error(index, err, where=None, call="decode_clips"):
    """`err` (an NvhError) as the error of clip `index`."""
    e = native.NvhError(err.code, "%s: clip %d: %s" % (call, index, where or "decode"))
    e.clip = index
    return e


class _Group:
    """One setup's clips on one Stream: pushes them as segments, synthesises whenever batch_frames frames are pending and
    routes every batch through its segment table."""

    def __init__(self, ctx, members, recs, form):
        self.members, self.recs, self.form = members, recs, form
        pa = recs[members[0]].packets
        self.stream = Stream(ctx, pa[0], pa[1], pa[2])
        self.pieces = {i: [] for i in members}

    def run(self):
        o, st = self.form, self.stream
        if o.gpu_parse:
            _enable_gpu_parse(st)
        for i in self.members:
            pa, nxt = self.recs[i].packets, 3
            while nxt < len(pa):
                room = o.batch_frames - st.pending()[0]
                if room <= 0:
                    self.flush()
                    continue
                try:
                    took = st.push_packets(pa, nxt, room)
                except native.NvhError as e:
                    raise _clip_error(i, e, "nvh_stream_push_packets")
                nxt += took
                if took < room and nxt < len(pa):
                    break  # the clip's end-of-stream packet: nothing behind it is pulled
            st.next_segment(o.align)
        self.flush()

    def flush(self):
        o, st = self.form, self.stream
        frames, samples = st.pending()
        if not frames:
            return
        table = st.pending_segments()
        och, planar = o.och(st.channels), o.planar
        if o.device_out:
            import torch
            dev = "cuda:%d" % o.device
            if planar:
                stride = max((samples + 3) & ~3, 4)
                out = torch.empty((och, stride), dtype=o.torch_dtype(), device=dev)
                st.synth_device(out.data_ptr(), 0, dtype=o.dtype, plane_stride=stride, channel_map=o.map(st.channels))
            else:
                out = torch.empty(max(samples * och, 1), dtype=o.torch_dtype(), device=dev)
                st.synth_device(out.data_ptr(), out.numel(), dtype=o.dtype, mix=o.mix, channel_map=o.map(st.channels))
        else:
            out = st.synth_host(pinned=True, dtype=o.dtype, planar=planar, mix=o.mix, channel_map=o.map(st.channels))
        if st.parse_errors:  # GPU-parse mode: a packet of this batch made the parser fail; positions up to it are the table's
            err, at = st.parse_errors[0]
            at //= 1 if (planar or o.mix is not None) else och
            # the segment whose range holds the position; a packet that leaves no samples there (a clip's first): the first
            # non-empty segment that begins at it, else the last one that begins before it
            inside = np.nonzero((table[:, 1] <= at) & (at < table[:, 2]))[0]
            row = inside[0] if inside.size else max(int(np.searchsorted(table[:, 1], at, side="right")) - 1, 0)
            k = int(table[row, 0])
            raise _clip_error(self.members[k], err, "a packet the parser fails on")
        if o.clipped is not None:
            _note_clipped(st, self.members, o.clipped)
        for k, b, e in table:
            if e > b:
                piece = out[:, b:e] if planar else out[b * och:e * och]
                # (a host batch lies in the stream's page-locked buffer, which the next batch overwrites)
                self.pieces[self.members[int(k)]].append(piece if o.device_out else piece.copy())

    def results(self, into):
        o, st = self.form, self.stream
        och = o.och(st.channels)
        for i in self.members:
            ps = self.pieces[i]
            if o.device_out:
                import torch
                if not ps:
                    ps = [torch.empty((och, 0) if o.planar else (0,), dtype=o.torch_dtype(), device="cuda:%d" % o.device)]
                into[i] = ps[0] if len(ps) == 1 else torch.cat(ps, dim=-1)  # (a clip inside one batch: a view of that batch's output)
            else:
                if not ps:
                    ps = [np.zeros((och, 0) if o.planar else (0,), dtype=o.dtype)]
                into[i] = ps[0] if len(ps) == 1 else np.concatenate(ps, axis=-1)


def decode_clips(clips, ctx=None, device=0, batch_frames=4096, gpu_parse=True, sample_format="f32", layout="interleaved", mix=None,
                 channel_map=None, align=4, device_out=False, return_clipped=False):
    """Decode a list of Ogg Vorbis clips (bytes or paths; logical stream 0 of each) and return one array per clip, in input
    order: what VorbisReader(clip, <the same options>).read_all() returns for it, bit for bit.

    Clips are grouped by identical identification and setup packets (the comment packet may differ).  Every group is one Stream;
    each clip's packets are pushed with their granules and flags and closed with next_segment(align); synthesis runs whenever
    `batch_frames` frames are pending -- in the middle of a clip if need be -- and every batch is taken apart by its segment
    table.  align=4 keeps every clip of a batch on the kernels' vector paths (include/nvorbis_hip.h).

    Host results are numpy arrays: (T * channels,) interleaved, (channels, T) for layout="planar", (T,) for mix="mono".
    device_out=True: torch tensors on the device instead -- views of the batch outputs for clips that lie inside one batch.

    return_clipped=True: returns (results, clipped) instead, `clipped` a numpy bool array with one entry per clip: that clip's
    VorbisReader.HasClipped after read_all() in the same output form (the per-segment flags of every batch the clip ran through,
    ORed: Stream.synth_segments_clipped).

    A clip whose headers or packets make the library return an error raises NvhError with the clip's index in the message (and
    as its `clip` attribute); there are no partial results."""
    dtype = _sample_format(sample_format)
    planar = _layout(layout)
    _mix(mix, planar)
    return_clipped = _return_clipped(return_clipped)
    if channel_map is not None:
        _channel_map(channel_map, None, mix)
    if isinstance(align, bool) or not isinstance(align, (int, np.integer)) or align < 1 or align > 65536 or align & (align - 1):
        raise ValueError("align must be a power of two in [1, 65536], not %r" % (align,))
    form = _Form(dtype, planar, mix, channel_map, _batch_frames(batch_frames), bool(gpu_parse), bool(device_out),
                 int(device) if ctx is None else ctx.device, int(align))
    recs = _load_clips(clips, "decode_clips")
    groups = {}
    for i, r in enumerate(recs):
        groups.setdefault(r.key, []).append(i)
    results = [None] * len(recs)
    clipped = np.zeros(len(recs), dtype=bool)
    if return_clipped:
        form.clipped = clipped
    if groups:
        with _context(ctx, device) as ctx:
            for members in groups.values():
                try:
                    g = _Group(ctx, members, recs, form)
                except native.NvhError as e:
                    raise _clip_error(members[0], e, "nvh_stream_open")
                try:
                    g.run()
                    g.results(results)
                finally:
                    g.stream.close()
    return (results, clipped) if return_clipped else results


# ---------------------------------------------------------------------------------------------------------------------------
# rows: crop and pad every clip into a fixed length
# ---------------------------------------------------------------------------------------------------------------------------

def plan_clip_window(position_after, emitted_after, state_after, total, start, length):
    """Which packets of a clip a row [start, start + length) needs, from Stream.index_packets' arrays over the clip's audio
    packets (indices below count audio packets from 0).  Host arithmetic only.  Returns a dict:
      valid         samples of the row that are the clip's: min(length, max(0, total - start))
      lead          the lead-in packet, pushed first without granule or flags (it emits nothing: a first packet), or None: the
                    run starts with the clip's first audio packet as a fresh stream does
      has_position, position   the serial decoder's position state behind the lead-in (set_position_state), None without one
      first, last   packets [first, last) follow with their granules and flags
      skip          the window's skip: `start` minus what the serial decoder had emitted behind the lead-in
    The first packet to emit is the first whose emitted_after exceeds `start`; the lead-in is the nearest packet before it that
    decodes with its overlap out of its own tail (state bit 1, value 2: where plan_stream_chunks cuts); the last packet pushed is
    the first whose emitted_after reaches start + length.  A row with valid == 0 needs no packet at all."""
    em, state = np.asarray(emitted_after), np.asarray(state_after)
    n = int(em.size)
    valid = int(min(length, max(0, total - start)))
    if valid == 0:
        return {"valid": 0, "lead": None, "has_position": None, "position": None, "first": 0, "last": 0, "skip": 0}
    f = int(np.searchsorted(em, start, side="right"))  # the first packet with emitted_after > start (n: only the final drain emits)
    safe = np.nonzero(state[:f] & 2)[0]
    lead = int(safe[-1]) if safe.size else None
    reach = int(np.searchsorted(em, start + length, side="left"))  # the first packet with emitted_after >= start + length
    last = min(reach + 1, n)
    if lead is None:
        return {"valid": valid, "lead": None, "has_position": None, "position": None, "first": 0, "last": last, "skip": int(start)}
    return {"valid": valid, "lead": lead, "has_position": bool(state[lead] & 4), "position": int(position_after[lead]),
            "first": lead + 1, "last": max(last, lead + 1), "skip": int(start - em[lead])}


def push_clip_window(st, pa, plan, length, room=None, flush=None):
    """Push one planned row into the current segment of `st` (the caller closes it with next_segment): the window, the lead-in,
    the position state, the packets.  room() -> how many more frames the pending batch takes, flush() synthesises it; without
    them everything is pushed at once.  `pa` is the clip's PacketArray (three headers first).  A plan with a "take" emits that
    many samples at most and pads the row to `length` (the resampler's source rows: a window of the row's own)."""
    st.segment_window(plan["skip"], plan.get("take", length), length)
    if plan["valid"] == 0:
        return
    if plan["lead"] is not None:
        if room is not None and room() <= 0:
            flush()
        st.push_packet(pa[3 + plan["lead"]], -1, 0)
        st.set_position_state(plan["has_position"], plan["position"])
    nxt, last = 3 + plan["first"], 3 + plan["last"]
    while nxt < last:
        take = last - nxt
        if room is not None:
            r = room()
            if r <= 0:
                flush()
                continue
            take = min(take, r)
        took = st.push_packets(pa, nxt, take)
        nxt += took
        if took < take:
            break  # the window is full, or the clip's end-of-stream packet: nothing behind it is pulled


class _RowGroup:
    """One setup's rows on one Stream, written into `buf` -- rows [row0, row0 + len(members)) of the dense buffer -- batch by
    batch: every batch's destination is the buffer's base plus what the batches before it wrote."""

    def __init__(self, ctx, members, recs, plans, form, length):
        self.members, self.recs, self.plans, self.form, self.length = members, recs, plans, form, length
        pa = recs[members[0]].packets
        self.stream = Stream(ctx, pa[0], pa[1], pa[2])
        self.done = 0  # samples per channel written so far: whole rows and the part of the open one
        self.dests = []  # the destination of every batch

    def run(self, base_ptr, row0, rows_total):
        """base_ptr: address of the dense buffer (device or host); rows_total: its rows (the planes' stride is rows_total * length)."""
        o, st = self.form, self.stream
        self.base, self.row0, self.rows_total = base_ptr, row0, rows_total
        if o.gpu_parse:
            _enable_gpu_parse(st)
        align = 4 if self.length % 4 == 0 else 1
        # Batches end on row boundaries -- once batch_frames frames are pending and the next batch's destination is one the
        # kernels take (interleaved 16-bit PCM: 16-byte aligned, which every eighth row boundary is at the latest) -- so that
        # every row of a batch lies where the vector paths want it; only a row of more than batch_frames frames is cut inside.
        och, isz = o.och(st.channels), o.dtype.itemsize
        strict = isz == 2 and not o.planar and o.mix is None and o.map(st.channels) is None
        for i in self.members:
            # a row is cut inside only after 2 * batch_frames frames of its own (what earlier rows left pending does not count
            # against it; behind a cut inside the row the count starts again)
            own = [st.pending()[0]]

            def cut_inside():
                self.flush()
                own[0] = 0
            try:
                push_clip_window(st, self.recs[i].packets, self.plans[i], self.length,
                                 lambda: own[0] + 2 * o.batch_frames - st.pending()[0], cut_inside)
            except native.NvhError as e:
                if getattr(e, "clip", None) is not None:
                    raise
                raise _clip_error(i, e, "nvh_stream_push_packets", "decode_clip_rows")
            st.next_segment(align)
            frames, samples = st.pending()
            if frames >= o.batch_frames and (not strict or (self.base + (self.row0 * self.length + self.done + samples) * och * isz) % 16 == 0):
                self.flush()
        self.flush()
        if self.done != len(self.members) * self.length:
            raise RuntimeError("decode_clip_rows: %d samples written, %d rows of %d planned" % (self.done, len(self.members), self.length))

    def flush(self):
        o, st = self.form, self.stream
        frames, samples = st.pending()
        if not frames and not samples:
            return
        och, planar, isz = o.och(st.channels), o.planar, o.dtype.itemsize
        if self.done + samples > len(self.members) * self.length:  # (never write behind the group's rows)
            raise RuntimeError("decode_clip_rows: a batch of %d samples behind %d does not fit %d rows of %d" %
                               (samples, self.done, len(self.members), self.length))
        stride = self.rows_total * self.length
        at = self.row0 * self.length + self.done  # samples per channel in front of this batch
        d, _, _, per = _pcm_out(o.dtype, planar, o.mix, o.map(st.channels), st.channels)
        if planar:
            ptr, d.extent = self.base + at * isz, stride
        else:
            ptr, d.extent = self.base + at * och * isz, samples * och
        self.dests.append(ptr)
        wr = C.c_int64(0)
        if o.device_out:
            rc = native.lib().nvh_stream_synth_out(st._h, C.byref(d), None, C.c_void_p(ptr), C.byref(wr))
        else:
            rc = native.lib().nvh_stream_synth_out(st._h, C.byref(d), C.c_void_p(ptr), None, C.byref(wr))
        st._note_parse_error(rc, wr.value, "nvh_stream_synth_out", planar=per, channels=och)
        if st.parse_errors:  # GPU-parse mode: a packet of this batch made the parser fail; rows lie `length` apart
            err, pos = st.parse_errors[0]
            pos //= 1 if per else och
            k = min((self.done + pos) // max(self.length, 1), len(self.members) - 1)
            raise _clip_error(self.members[int(k)], err, "a packet the parser fails on", "decode_clip_rows")
        if o.clipped is not None:
            _note_clipped(st, self.members, o.clipped)
        self.done += wr.value if per else wr.value // och


def resample_plan(in_rate, out_rate):
    """(L, M, half, tap_count) of nvh_resample_plan for a source and a target rate; ValueError for a pair outside its limits."""
    up, down, half, count = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    rc = native.lib().nvh_resample_plan(int(in_rate), int(out_rate), C.byref(up), C.byref(down), C.byref(half), C.byref(count))
    if rc in (native.ERR_UNSUPPORTED, native.ERR_ARGUMENT):
        raise ValueError("no resampler from %d Hz to %d Hz: the ratio is outside the limits (include/nvorbis_hip.h)" % (in_rate, out_rate))
    native.check(rc, "nvh_resample_plan")
    return up.value, down.value, half.value, count.value


def resample_taps(in_rate, out_rate):
    """The tap table of nvh_resample_taps as a float32 array (L, 2 * half): exactly what k_resample_rows reads."""
    L, _, half, count = resample_plan(in_rate, out_rate)
    h = np.zeros(count, np.float32)
    got = C.c_int64(0)
    native.check(native.lib().nvh_resample_taps(int(in_rate), int(out_rate), h.ctypes.data, count, C.byref(got)), "nvh_resample_taps")
    return h.reshape(L, 2 * half)


def _sample_rate(value):
    if value is None:
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 1 or value > 2 ** 31 - 1:
        raise ValueError("sample_rate must be None or an int in [1, 2**31), not %r" % (value,))
    return int(value)


def _output_channels(recs, form, call):
    """The one output channel count of the clips in `form` (1 without clips); ValueError of `call` if they differ."""
    ochs = sorted(set(form.och(ch) for ch in set(r.channels for r in recs)))
    if len(ochs) > 1:
        raise ValueError("%s: the clips' output channel counts differ (%s)" % (call, ochs))
    return ochs[0] if ochs else 1


def _run_row_groups(ctx, members, recs, plans, form, length, base, rows_total):
    """Clips `members` as rows [0, len(members)) of the buffer at `base` (of rows_total rows), grouped by setup, one _RowGroup
    after the other.  Returns the clips in the order of their rows."""
    groups = {}
    for i in members:
        groups.setdefault(recs[i].key, []).append(i)
    placed, row0 = [], 0
    for group in groups.values():
        try:
            g = _RowGroup(ctx, group, recs, plans, form, length)
        except native.NvhError as e:
            raise _clip_error(group[0], e, "nvh_stream_open", "decode_clip_rows")
        try:
            g.run(base, row0, rows_total)
        finally:
            g.stream.close()
        row0 += len(group)
        placed += group
    return placed, len(groups)


def _resampled_rows(ctx, recs, plans, starts, length, sample_rate, form):
    """decode_clip_rows with at least one clip at another rate than `sample_rate`: (buf, valid) on the device, rows in input
    order.  Clips at the target rate go through the row path as they are and are copied to their rows; the others are classed by
    source rate, every class decodes f32 source rows [origin, origin + S) into a temporary buffer through the same row path,
    and k_resample_rows writes the class's rows of the returned buffer.  `form`: the call's, with device_out set."""
    import torch
    n = len(recs)
    dev = "cuda:%d" % form.device
    tdt, och = form.torch_dtype(), form.och(recs[0].channels)
    buf = torch.empty(form.row_shape(n, length, och), dtype=tdt, device=dev)
    flags = torch.zeros(n, dtype=torch.int32, device=dev) if form.clipped is not None else None
    valid = np.asarray([p["valid"] for p in plans], dtype=np.int64)
    classes, setups = {}, {}
    for i, r in enumerate(recs):
        if r.rate != sample_rate:
            classes.setdefault(r.rate, []).append(i)
        else:
            setups.setdefault(r.key, []).append(i)
    keep = []  # the temporaries, until the context's stream has run
    for group in setups.values():  # (a buffer per setup: every group begins on an allocation's alignment, whatever the length)
        tmp = torch.empty(form.row_shape(len(group), length, och), dtype=tdt, device=dev)
        placed, _ = _run_row_groups(ctx, group, recs, plans, form, length, tmp.data_ptr(), len(group))
        buf.index_copy_(1 if form.planar else 0, torch.as_tensor(placed, dtype=torch.int64, device=dev), tmp)
        keep.append(tmp)
    for rate, members in classes.items():
        L, M, half, _ = resample_plan(rate, sample_rate)
        origin, take = {}, {}
        for i in members:
            total = recs[i].index[3]
            total_out = (total * L + M - 1) // M
            valid[i] = min(length, max(0, total_out - starts[i]))
            origin[i] = take[i] = 0  # (nothing of the clip in the row: no packet is decoded, the source row is a pad)
            if valid[i]:
                c_first, c_last = (starts[i] * M) // L, ((starts[i] + int(valid[i]) - 1) * M) // L
                origin[i] = max(0, c_first - half + 1) & ~3
                take[i] = (c_last + half + 1 - origin[i] + 3) & ~3
        S = max(4, max(take.values()))  # the source rows' pitch; row i holds source samples [origin, origin + take) and a pad
        src_plans = {}
        for i in members:
            pos, em, state, total = recs[i].index
            src_plans[i] = plan_clip_window(pos, em, state, total, origin[i] if take[i] else total, take[i])
            if take[i]:
                src_plans[i]["take"] = take[i]
        tmp = torch.empty(form.row_shape(len(members), S, och), dtype=torch.float32, device=dev)
        placed, _ = _run_row_groups(ctx, members, recs, src_plans, form.f32(), S, tmp.data_ptr(), len(members))
        torch.cuda.current_stream(dev).synchronize()  # (the flag words are zeroed on torch's stream)
        sr, st, sc = form.row_strides(len(members), S, och)
        dr, dt, dc = form.row_strides(n, length, och)
        desc = native.ResampleDesc(in_rate=rate, out_rate=sample_rate, rows=len(members), channels=och,
                                   format=_pcm_format(form.dtype)[0], length=length, src_length=S,
                                   src_row_stride=sr, src_time_stride=st, src_chan_stride=sc, dst_row_stride=dr,
                                   dst_time_stride=dt, dst_chan_stride=dc)
        ctx.resample_rows(desc, tmp.data_ptr(), buf.data_ptr(), [origin[i] for i in placed], [starts[i] for i in placed],
                          [valid[i] for i in placed], placed, None if flags is None else flags.data_ptr())
        keep.append(tmp)
    ctx.synchronize()
    if flags is not None:
        form.clipped |= flags.cpu().numpy() != 0
    del keep
    return buf, valid


def decode_clip_rows(clips, length, starts=None, ctx=None, device=0, batch_frames=4096, gpu_parse=True, sample_format="f32",
                     layout="interleaved", mix=None, channel_map=None, device_out=False, return_clipped=False, sample_rate=None):
    """Crop and pad a list of Ogg Vorbis clips (bytes or paths; logical stream 0 of each) into N rows of exactly `length` samples:
    returns (rows, valid).  Row i holds samples [starts[i], starts[i] + length) of what VorbisReader(clips[i], <the same
    options>).read_all() returns, per channel, bit for bit, and zeros behind the clip's end; valid[i] (an int64 numpy array) says
    how many of the row's samples are the clip's -- 0 for a start at or beyond its end.  starts=None: 0 for every clip; starts
    are ints >= 0, length >= 0.

    Shapes: (N, length, channels) interleaved; (N, length) for mix="mono"; layout="planar": (N, channels, length), returned as a
    PERMUTED VIEW of the (channels, N, length) buffer the planar kernels write (not contiguous: call .contiguous() /
    np.ascontiguousarray where that matters).  channels = the output channels (len(channel_map) with a map).  device_out=True: a
    torch tensor on the device, else a numpy array.  Clips whose output channel counts differ raise ValueError.

    Only the packets a row needs are decoded: per clip the host plans (plan_clip_window, from Stream.index_packets) a one-packet
    lead-in, the serial decoder's position state behind it and the packets up to the row's end, and pushes them as a windowed
    segment (Stream.segment_window: skip, take = pitch = length).  Clips are grouped by setup as in decode_clips.  With one
    group the kernels write the returned buffer itself, batch behind batch; with several, rows are written group by group and
    returned through one gather.

    Rows are aligned to 4 samples when length % 4 == 0 (else to 1).  Starts and lengths that are multiples of 4 keep the
    kernels' vector paths and paired emission for the frames inside a row; any other start or length gives the same bits through
    the per-frame fall-back, slower.

    return_clipped=True: returns ((rows, valid), clipped) instead, `clipped` a numpy bool array with one entry per row: whether
    ClipSamples clamped one of the samples the row holds (HasClipped of a reader that emitted exactly those samples in the same
    output form; the pad never counts).

    sample_rate=R: every row at R Hz.  None, or a clip whose own rate is R: that clip's row is what it is without the keyword,
    bit for bit, and if every clip is at R so are the launches.  A clip at another rate is resampled by the rule of
    include/nvorbis_hip.h (nvh_resample_rows: a polyphase filter of 2 * half taps per output, reproducible bit for bit): `starts`,
    `length` and `valid` then count samples at R -- valid = clamp(ceil(total * R / rate) - start, 0, length) -- and the row holds
    outputs [start, start + length) of the clip resampled as a whole, zeros from `valid` on.  Such clips are classed by source
    rate; per class the row path above decodes f32 SOURCE rows into a temporary device buffer in the requested mix, map and
    layout -- the source window of a row is what its outputs read, which includes up to `half` samples of margin on each side:
    [origin, origin + take) with origin = max(0, c_first - half + 1) rounded down and take rounded up to a multiple of 4 samples, so
    that paired emission is kept, c_first = start * M div L -- and k_resample_rows writes the rows into the
    returned buffer at their final indices, clipping again and converting to 16 bits there for sample_format="s16".  Host
    results are that device buffer read back.  return_clipped: a resampled row's flag is the decode stage's flag for its source
    window, margins included, ORed with the resampler's.  ValueError for a rate that is no int >= 1 and for a pair of rates
    outside the resampler's limits (up factor above 4096, or more than 262144 taps), before any device is touched.

    Batches end on row boundaries once `batch_frames` frames are pending; only a row of more than 2 * batch_frames frames of
    its own is cut inside, every 2 * batch_frames frames.  LIMIT: such a cut falls on whatever sample the frames end on, and
    interleaved 16-bit PCM asks for a 16-byte aligned destination (nvh_stream_synth_pcm's rule), so sample_format="s16" with
    layout="interleaved" and rows that long can fail with NVH_ERR_ARGUMENT: raise batch_frames above half a row's frames
    (length / 64 + 12 is an upper bound of a row's frames), or use the planar layout, which has no such rule.

    A clip whose headers or packets make the library return an error raises NvhError with the clip's index in the message (and
    as its `clip` attribute); there are no partial results."""
    dtype = _sample_format(sample_format)
    planar = _layout(layout)
    _mix(mix, planar)
    return_clipped = _return_clipped(return_clipped)
    sample_rate = _sample_rate(sample_rate)
    if channel_map is not None:
        _channel_map(channel_map, None, mix)
    length = _length(length)
    batch_frames = _batch_frames(batch_frames)
    clips = list(clips)
    starts = _starts(starts, len(clips))
    form = _Form(dtype, planar, mix, channel_map, batch_frames, bool(gpu_parse), bool(device_out),
                 int(device) if ctx is None else ctx.device, clipped=np.zeros(len(clips), dtype=bool) if return_clipped else None)
    recs = _load_clips(clips, "decode_clip_rows", sample_rate, True, form)
    return _clip_rows(ctx, recs, starts, length, sample_rate, form)


def _clip_rows(ctx, recs, starts, length, sample_rate, form):
    """decode_clip_rows behind its argument checks and the load: `recs` from _load_clips with the index, `form` with the
    `clipped` array of return_clipped (what is returned says so: ((rows, valid), clipped))."""
    n, och = len(recs), _output_channels(recs, form, "decode_clip_rows")
    plans = [plan_clip_window(*r.index, starts[i], length) for i, r in enumerate(recs)]
    valid = np.asarray([p["valid"] for p in plans], dtype=np.int64)
    if sample_rate is not None and n and length and any(r.rate != sample_rate for r in recs):
        with _context(ctx, form.device) as ctx:
            buf, valid = _resampled_rows(ctx, recs, plans, starts, length, sample_rate, dataclasses.replace(form, device_out=True))
        if not form.device_out:
            buf = buf.cpu().numpy()
    else:
        if form.device_out:
            import torch
            buf = torch.empty(form.row_shape(n, length, och), dtype=form.torch_dtype(), device="cuda:%d" % form.device)
            base = buf.data_ptr()
        else:
            buf = np.empty(form.row_shape(n, length, och), dtype=form.dtype)
            base = buf.ctypes.data
        placed, groups = list(range(n)), 1
        if n and length:
            with _context(ctx, form.device) as ctx:
                placed, groups = _run_row_groups(ctx, range(n), recs, plans, form, length, base, n)
        elif n:
            groups = len(set(r.key for r in recs))
        if groups > 1:  # rows lie group by group: one gather puts them into input order
            order = np.empty(n, dtype=np.int64)
            order[np.asarray(placed, dtype=np.int64)] = np.arange(n)
            if form.device_out:
                buf = buf.index_select(1 if form.planar else 0, torch.as_tensor(order, device=buf.device))
            else:
                buf = np.take(buf, order, axis=1 if form.planar else 0)
    if form.planar:
        buf = buf.permute(1, 0, 2) if form.device_out else buf.transpose(1, 0, 2)
    return ((buf, valid), form.clipped) if form.clipped is not None else (buf, valid)


# ---------------------------------------------------------------------------------------------------------------------------
# features: log-mel spectrograms of the rows
# ---------------------------------------------------------------------------------------------------------------------------

_MEL_SCALES = {"htk": native.MEL_HTK, "slaney": native.MEL_SLANEY}
_MEL_NORMS = {None: native.MEL_NORM_NONE, "slaney": native.MEL_NORM_SLANEY}
_MEL_OUT = {"power": native.MEL_POWER, "ln": native.MEL_LN, "db": native.MEL_DB}


def _int_in(name, value, lo, hi):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < lo or value > hi:
        raise ValueError("%s must be an int in [%d, %d], not %r" % (name, lo, hi, value))
    return int(value)


def _real(name, value, finite):
    """`value` if it is a real number: no bool, no NaN and, with `finite`, no infinity."""
    if (isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating))
            or (not np.isfinite(value) if finite else np.isnan(value))):
        raise ValueError("%s must be a %s, not %r" % (name, "finite number" if finite else "number", value))
    return value


def mel_desc(rate, n_fft=512, win_length=400, hop=160, n_mels=80, f_min=0.0, f_max=None, mel_scale="htk", norm=None, scale="ln",
             floor=1e-10):
    """A native.MelDesc with the rule's parameters filled in (include/nvorbis_hip.h: nvh_mel_rows), checked on the host: ValueError
    for anything outside the rule's limits.  f_max=None: rate / 2.  Shape and strides are left 0 for the caller."""
    rate = _int_in("the sample rate", rate, 1, 2 ** 31 - 1)
    n_fft = _int_in("n_fft", n_fft, 64, 4096)
    if n_fft & (n_fft - 1):
        raise ValueError("n_fft must be a power of two in [64, 4096], not %r (other transforms are out of scope)" % (n_fft,))
    win_length = _int_in("win_length", win_length, 1, n_fft)
    hop = _int_in("hop", hop, 1, 65536)
    n_mels = _int_in("n_mels", n_mels, 1, 256)
    if not isinstance(mel_scale, str) or mel_scale not in _MEL_SCALES:
        raise ValueError("mel_scale must be 'htk' or 'slaney', not %r" % (mel_scale,))
    if norm is not None and (not isinstance(norm, str) or norm not in _MEL_NORMS):
        raise ValueError("norm must be None or 'slaney', not %r" % (norm,))
    if not isinstance(scale, str) or scale not in _MEL_OUT:
        raise ValueError("scale must be 'power', 'ln' or 'db', not %r" % (scale,))
    f_min, f_max, floor = (float(_real(name, v, True)) for name, v in
                           (("f_min", f_min), ("f_max", rate / 2.0 if f_max is None else f_max), ("floor", floor)))
    if not 0.0 <= f_min < f_max <= rate / 2.0:
        raise ValueError("f_min and f_max must satisfy 0 <= f_min < f_max <= rate / 2 (%r, %r at %d Hz)" % (f_min, f_max, rate))
    with np.errstate(over="ignore"):
        floor32 = np.float32(floor)
    if not np.isfinite(floor32) or floor32 < np.float32(2.0 ** -126):
        raise ValueError("floor must be an f32 >= 2**-126, not %r" % (floor,))
    d = native.MelDesc(rate=rate, n_fft=n_fft, win_length=win_length, hop=hop, n_mels=n_mels, mel_scale=_MEL_SCALES[mel_scale],
                       norm=_MEL_NORMS[norm], scale=_MEL_OUT[scale], floor=float(floor32), f_min=f_min, f_max=f_max)
    counts = [C.c_int64(0) for _ in range(3)]
    rc = native.lib().nvh_mel_plan(C.byref(d), *[C.byref(c) for c in counts])
    if rc == native.ERR_ARGUMENT:
        raise ValueError("the mel parameters are outside the rule's limits (include/nvorbis_hip.h)")
    native.check(rc, "nvh_mel_plan")
    return d


_MEL_WINDOWS = {"hann": native.WIN_HANN, "hann_symmetric": native.WIN_HANN_SYM, "hamming": native.WIN_HAMMING, "povey": native.WIN_POVEY,
                "rectangular": native.WIN_RECT}
_MEL_TRIANGLES = {"hz": native.TRI_HZ, "mel": native.TRI_MEL}
_MEL_PADS = {"constant": native.PAD_ZERO, "reflect": native.PAD_REFLECT}


def mel_front(window="hann", mel_triangles="hz", pad_mode="constant", remove_dc=False, preemphasis=0.0, sample_gain=1.0):
    """A native.MelFront (include/nvorbis_hip.h: nvh_mel_front), checked on the host with ValueError -- or None where every
    argument has today's value: the caller then goes through nvh_mel_rows itself."""
    if not isinstance(window, str) or window not in _MEL_WINDOWS:
        raise ValueError("window must be one of %s, not %r" % (", ".join(repr(k) for k in _MEL_WINDOWS), window))
    if not isinstance(mel_triangles, str) or mel_triangles not in _MEL_TRIANGLES:
        raise ValueError("mel_triangles must be 'hz' or 'mel', not %r" % (mel_triangles,))
    if not isinstance(pad_mode, str) or pad_mode not in _MEL_PADS:
        raise ValueError("pad_mode must be 'constant' or 'reflect', not %r" % (pad_mode,))
    if not isinstance(remove_dc, (bool, np.bool_)):
        raise ValueError("remove_dc must be True or False, not %r" % (remove_dc,))
    with np.errstate(over="ignore"):
        p32 = np.float32(_real("preemphasis", preemphasis, False))
        g32 = np.float32(_real("sample_gain", sample_gain, False))
    if not 0.0 <= p32 <= 1.0:
        raise ValueError("preemphasis must be in [0, 1], not %r" % (preemphasis,))
    if not np.isfinite(g32) or not g32 > 0:
        raise ValueError("sample_gain must be a finite f32 > 0, not %r" % (sample_gain,))
    f = native.MelFront(_MEL_WINDOWS[window], _MEL_TRIANGLES[mel_triangles], _MEL_PADS[pad_mode], int(bool(remove_dc)), float(p32), float(g32))
    if (f.window, f.triangles, f.pad_mode, f.remove_dc) == (native.WIN_HANN, native.TRI_HZ, native.PAD_ZERO, 0) and p32 == 0 and g32 == 1:
        return None
    return f


def mel_tables(rate, n_fft=512, win_length=400, n_mels=80, f_min=0.0, f_max=None, mel_scale="htk", norm=None, window="hann",
               mel_triangles="hz"):
    """The tables of nvh_mel_tables (nvh_mel_tables_front with a window or triangles of one's own) as float32 arrays, exactly the
    values k_mel_rows uses: (twiddles (n_fft / 2 + 1, 2) as (cos, sin), window (win_length,), bank (n_mels, n_fft / 2 + 1))."""
    d = mel_desc(rate, n_fft, win_length, 1, n_mels, f_min, f_max, mel_scale, norm)
    front = mel_front(window, mel_triangles)
    bins = n_fft // 2 + 1
    tw, win, fb = np.zeros(2 * bins, np.float32), np.zeros(win_length, np.float32), np.zeros(n_mels * bins, np.float32)
    counts = [C.c_int64(0) for _ in range(3)]
    if front is None:
        native.check(native.lib().nvh_mel_tables(C.byref(d), tw.ctypes.data, win.ctypes.data, fb.ctypes.data, tw.size, win.size, fb.size,
                                                 *[C.byref(c) for c in counts]), "nvh_mel_tables")
    else:
        native.check(native.lib().nvh_mel_tables_front(C.byref(d), C.byref(front), tw.ctypes.data, win.ctypes.data, fb.ctypes.data, tw.size,
                                                       win.size, fb.size, *[C.byref(c) for c in counts]), "nvh_mel_tables_front")
    return tw.reshape(bins, 2), win, fb.reshape(n_mels, bins)


def kaldi_fbank_keywords(rate, frame_length_ms=25.0, frame_shift_ms=10.0, num_mel_bins=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97,
                         remove_dc=True, window="povey"):
    """The keywords that make decode_clip_features compute Kaldi's fbank (compute-fbank-feats, torchaudio.compliance.kaldi.fbank)
    at `rate` Hz, under Kaldi's own option names: decode_clip_features(clips, length, sample_rate=rate,
    **kaldi_fbank_keywords(rate)).  win_length and hop are the milliseconds in samples (truncated, as Kaldi does), n_fft the next
    power of two (at least 64: round_to_power_of_two), f_min = low_freq, f_max = high_freq, or rate / 2 + high_freq for high_freq
    <= 0; mel_scale="htk" with mel_triangles="mel" (Kaldi's bank), scale="ln" with floor = the f32 epsilon, center=False with
    frame_count="window" (snip_edges) and sample_gain=32768 (Kaldi reads 16-bit sample values).  What differs from Kaldi: the
    window is centred in n_fft, not at its start (the power spectrum is the same), and the arithmetic is the rule's f32
    (tests/test_mel_front_plan.py measures the distance).  Dither (dither=0 in Kaldi's terms) and the energy column (use_energy)
    are out of scope; so is snip_edges=false.  The dict does not hold sample_rate: pass it beside the dict where the clips are
    at other rates."""
    rate = _int_in("rate", rate, 1, 2 ** 31 - 1)
    for name, v in (("frame_length_ms", frame_length_ms), ("frame_shift_ms", frame_shift_ms), ("low_freq", low_freq), ("high_freq", high_freq)):
        _real(name, v, True)
    win_length, hop = int(rate * 0.001 * frame_length_ms), int(rate * 0.001 * frame_shift_ms)
    if win_length < 1 or win_length > 4096 or hop < 1:
        raise ValueError("frame_length_ms and frame_shift_ms must give a window in [1, 4096] samples and a hop >= 1 (%d, %d)" % (win_length, hop))
    n_fft = 64
    while n_fft < win_length:
        n_fft *= 2
    return dict(n_fft=n_fft, win_length=win_length, hop=hop, n_mels=num_mel_bins, f_min=float(low_freq),
                f_max=float(high_freq) if high_freq > 0 else rate / 2.0 + float(high_freq), mel_scale="htk", mel_triangles="mel",
                scale="ln", floor=float(np.finfo(np.float32).eps), center=False, frame_count="window", sample_gain=32768.0,
                preemphasis=preemphasis, remove_dc=remove_dc, window=window)


_FNORM_MODES = {None: native.FNORM_NONE, "mean": native.FNORM_MEAN, "mean_var": native.FNORM_MEAN_VAR, "peak": native.FNORM_PEAK}
_FNORM_AXES = {"band": native.FNORM_PER_BAND, "all": native.FNORM_ALL}


class _DefaultPad(float):
    """decode_clip_features' pad_value default: 0.0, and an object of its own, so that `pad_value=0.0` given by the caller is not it."""
    __slots__ = ()

    def __repr__(self):
        return "0.0"


_PAD_DEFAULT = _DefaultPad(0.0)


def fnorm_desc(normalize=None, normalize_axis="band", norm_eps=1e-5, pad_value=0.0, peak_range=80.0, peak_offset=40.0, peak_gain=1 / 40,
               frames=0, bands=1):
    """A native.FnormDesc with the rule's numbers filled in (include/nvorbis_hip.h: nvh_fnorm_rows), checked on the host: ValueError
    for anything outside the rule's limits.  Every number is checked whatever the mode (the C call looks only at those its mode
    uses).  rows, channels and the strides are left 0 for the caller."""
    if normalize is not None and (not isinstance(normalize, str) or normalize not in _FNORM_MODES):
        raise ValueError("normalize must be None, 'mean', 'mean_var' or 'peak', not %r" % (normalize,))
    if not isinstance(normalize_axis, str) or normalize_axis not in _FNORM_AXES:
        raise ValueError("normalize_axis must be 'band' or 'all', not %r" % (normalize_axis,))
    frames = _int_in("frames", frames, 0, 2 ** 24)
    bands = _int_in("bands", bands, 1, 256)
    vals = {}
    for name, v in (("norm_eps", norm_eps), ("pad_value", pad_value), ("peak_range", peak_range), ("peak_offset", peak_offset),
                    ("peak_gain", peak_gain)):
        with np.errstate(over="ignore"):
            vals[name] = np.float32(_real(name, v, False))
    if not np.isfinite(vals["norm_eps"]) or vals["norm_eps"] < np.float32(2.0 ** -126):
        raise ValueError("norm_eps must be an f32 >= 2**-126, not %r" % (norm_eps,))
    if not vals["peak_range"] >= 0:
        raise ValueError("peak_range must be >= 0 (inf: no clamp), not %r" % (peak_range,))
    for name in ("pad_value", "peak_offset", "peak_gain"):
        if not np.isfinite(vals[name]):
            raise ValueError("%s must be a finite f32, not %r" % (name, {"pad_value": pad_value, "peak_offset": peak_offset, "peak_gain": peak_gain}[name]))
    d = native.FnormDesc(mode=_FNORM_MODES[normalize], axis=_FNORM_AXES[normalize_axis], frames=frames, bands=bands, channels=1,
                         eps=float(vals["norm_eps"]), pad_value=float(vals["pad_value"]), range=float(vals["peak_range"]),
                         offset=float(vals["peak_offset"]), gain=float(vals["peak_gain"]))
    rc = native.lib().nvh_fnorm_check(C.byref(d))
    if rc == native.ERR_ARGUMENT:
        raise ValueError("the normalisation parameters are outside the rule's limits (include/nvorbis_hip.h)")
    native.check(rc, "nvh_fnorm_check")
    d.channels = 0
    return d


_CEP_NORMS = {"ortho": native.CEP_ORTHO, None: native.CEP_PLAIN}


def cep_desc(cepstra=None, dct_norm="ortho", lifter=0.0, deltas=0, delta_window=2, frames=0, bands=1):
    """A native.CepDesc with the rule's numbers filled in (include/nvorbis_hip.h: nvh_cep_rows), checked on the host: ValueError for
    anything outside the rule's limits.  cepstra: None (no transform: the bands themselves are the static columns) or the number K
    of DCT-II coefficients, 1 <= K <= bands.  dct_norm: "ortho" (Kaldi's matrix, torchaudio's norm="ortho") or None (torchaudio's
    norm=None).  lifter: Kaldi's cepstral_lifter, 0 for none.  deltas: 0, 1 or 2 orders of delta columns over a window of
    delta_window frames on each side (1 .. 8).  (1 + deltas) * K columns come out, at most 256.  Every number is checked whatever
    the others are.  rows, channels and the strides are left 0 for the caller."""
    bands = _int_in("bands", bands, 1, 256)
    frames = _int_in("frames", frames, 0, 2 ** 24)
    ceps = bands if cepstra is None else _int_in("cepstra", cepstra, 1, bands)
    if dct_norm is not None and (not isinstance(dct_norm, str) or dct_norm not in _CEP_NORMS):
        raise ValueError("dct_norm must be 'ortho' or None, not %r" % (dct_norm,))
    with np.errstate(over="ignore"):
        l32 = np.float32(_real("lifter", lifter, False))
    if not np.isfinite(l32) or not l32 >= 0:
        raise ValueError("lifter must be a finite f32 >= 0 (0: none), not %r" % (lifter,))
    deltas = _int_in("deltas", deltas, 0, 2)
    delta_window = _int_in("delta_window", delta_window, 1, native.CEP_MAX_WINDOW)
    if (1 + deltas) * ceps > 256:
        raise ValueError("(1 + deltas) * %d columns are more than 256" % ceps)
    d = native.CepDesc(transform=native.CEP_NONE if cepstra is None else native.CEP_DCT2, dct_norm=_CEP_NORMS[dct_norm], order=deltas,
                       window=delta_window, channels=1, frames=frames, bands=bands, ceps=ceps, lifter=float(l32))
    rc = native.lib().nvh_cep_check(C.byref(d))
    if rc == native.ERR_ARGUMENT:
        raise ValueError("the cepstral parameters are outside the rule's limits (include/nvorbis_hip.h)")
    native.check(rc, "nvh_cep_check")
    d.channels = 0
    return d


def cep_tables(bands, cepstra=None, dct_norm="ortho", lifter=0.0, delta_window=2):
    """The tables of nvh_cep_tables as float32 arrays, exactly the values k_cep_rows uses: (D (K, bands), or None without a
    transform; s_1 (2 N + 1,); s_2 (4 N + 1,))."""
    d = cep_desc(cepstra, dct_norm, lifter, 0, delta_window, 0, bands)
    d.channels = 1
    n = d.window
    dct = np.zeros(d.ceps * d.bands if cepstra is not None else 0, np.float32)
    scales = np.zeros(6 * n + 2, np.float32)
    counts = [C.c_int64(0), C.c_int64(0)]
    native.check(native.lib().nvh_cep_tables(C.byref(d), dct.ctypes.data if dct.size else None, scales.ctypes.data, dct.size, scales.size,
                                             C.byref(counts[0]), C.byref(counts[1])), "nvh_cep_tables")
    return (dct.reshape(d.ceps, d.bands) if cepstra is not None else None), scales[:2 * n + 1], scales[2 * n + 1:]


def kaldi_mfcc_keywords(rate, num_ceps=13, num_mel_bins=23, cepstral_lifter=22.0, frame_length_ms=25.0, frame_shift_ms=10.0, low_freq=20.0,
                        high_freq=0.0, preemphasis=0.97, remove_dc=True, window="povey"):
    """The keywords that make decode_clip_features compute Kaldi's MFCCs (compute-mfcc-feats --use-energy=false,
    torchaudio.compliance.kaldi.mfcc with use_energy=False) at `rate` Hz, under Kaldi's own option names: kaldi_fbank_keywords(rate,
    ...) with Kaldi's MFCC defaults (23 mel bins), plus cepstra=num_ceps, dct_norm="ortho" (Kaldi's DCT matrix) and
    lifter=cepstral_lifter.  The lifter is folded into the DCT table where Kaldi multiplies afterwards (one rounding apart).
    C0 is the DCT's coefficient 0: the energy column (use_energy, Kaldi's default) is out of scope, because the mel stage does
    not emit the frame's raw energy; so is dither.  add-deltas is deltas=2, delta_window=2 beside the dict."""
    kw = kaldi_fbank_keywords(rate, frame_length_ms, frame_shift_ms, num_mel_bins, low_freq, high_freq, preemphasis, remove_dc, window)
    num_ceps = _int_in("num_ceps", num_ceps, 1, _int_in("num_mel_bins", num_mel_bins, 1, 256))
    with np.errstate(over="ignore"):
        l32 = np.float32(_real("cepstral_lifter", cepstral_lifter, False))
    if not np.isfinite(l32) or not l32 >= 0:
        raise ValueError("cepstral_lifter must be a finite f32 >= 0 (0: none), not %r" % (cepstral_lifter,))
    kw.update(cepstra=num_ceps, dct_norm="ortho", lifter=float(cepstral_lifter))
    return kw


def decode_clip_features(clips, length, starts=None, *, sample_rate=None, n_fft=512, win_length=400, hop=160, n_mels=80, f_min=0.0,
                         f_max=None, mel_scale="htk", norm=None, scale="ln", floor=1e-10, center=True, band_major=True, mix=None,
                         channel_map=None, ctx=None, device=0, batch_frames=4096, gpu_parse=True, device_out=True,
                         return_clipped=False, normalize=None, normalize_axis="band", norm_eps=1e-5, pad_value=_PAD_DEFAULT,
                         peak_range=80.0, peak_offset=40.0, peak_gain=1 / 40, mask_padding=True, window="hann", remove_dc=False,
                         preemphasis=0.0, sample_gain=1.0, pad_mode="constant", mel_triangles="hz", frame_count="n_fft", cepstra=None,
                         dct_norm="ortho", lifter=0.0, deltas=0, delta_window=2):
    """Log-mel features of fixed-length rows: decode_clip_rows(clips, length, starts, sample_format="f32", layout="planar",
    device_out=True, sample_rate=sample_rate, ...) as it is, then nvh_mel_rows over the buffer the planar kernels wrote (the one
    plane of mix="mono").  Returns (features, valid, valid_frames); with return_clipped=True ((features, valid, valid_frames),
    clipped), `clipped` being decode_clip_rows' per-row flags.

    features: float32, (N, C, n_mels, F), or (N, C, F, n_mels) with band_major=False; the C axis is absent with mix="mono".  A
    torch tensor on the device, or a numpy array with device_out=False.  Every value follows the rule of include/nvorbis_hip.h
    (nvh_mel_rows) bit for bit: a periodic Hann window of win_length samples centred in n_fft, the power spectrum, a triangular
    mel bank (mel_scale "htk" or "slaney", norm None or "slaney", f_max=None: half the rate), then scale "power", "ln" or "db"
    of max(value, floor).  Samples outside [0, valid[i]) of a row count as zeros.

    center=True is torch.stft's center=True with pad_mode="constant": frame f is centred on sample f * hop, F = length // hop + 1.
    center=False: frame f begins at sample f * hop, F = (length - n_fft) // hop + 1; ValueError for length < n_fft.  n_fft must
    be a power of two in [64, 4096]: other transform lengths are out of scope (Whisper's own 400-point bins, for example, are
    not what n_fft=512, win_length=400 gives).

    The front of a frame (include/nvorbis_hip.h: nvh_mel_front; with every keyword of this paragraph left away the call goes
    through nvh_mel_rows exactly as before).  window: "hann" (periodic), "hann_symmetric", "hamming", "povey" or "rectangular".
    sample_gain: every sample is multiplied by it first (32768: 16-bit sample values).  remove_dc: the mean of the frame's
    win_length samples is subtracted.  preemphasis p in [0, 1]: y[n] = s[n] - p s[n-1], y[0] = s[0] - p s[0] (Kaldi's).
    mel_triangles="mel": the bank's triangles are linear in mel, not in Hz (Kaldi's bank).  pad_mode="reflect" (torch.stft's
    default, Whisper's front end) needs center=True: samples in front of the row and behind `length` are the row mirrored at
    its first and last sample; ValueError unless one reflection is enough for every frame (length >= 2, n_fft // 2 -
    (n_fft - win_length) // 2 <= length - 1, and the last frame's last sample at most 2 (length - 1)).  The mirror is at
    `length`, not at valid[i]: samples at and behind valid[i] are zeros, and a mirrored read can land in them.
    frame_count="window" (Kaldi's snip_edges) needs center=False: frame f begins at sample f * hop, F = (length - win_length)
    // hop + 1; ValueError for length < win_length.  kaldi_fbank_keywords() returns the whole Kaldi set.

    valid: decode_clip_rows' valid.  valid_frames[i] (int64): how many of the row's frames have one of their win_length samples
    inside [0, valid[i]) -- under pad_mode="reflect" too, where the formula looks at the UNREFLECTED positions (a frame counts by
    where its window lies, not by what the mirror shows it: with valid[i] == length - win_length / 2 and hop dividing length, the
    frame behind the last counted one reads one counted sample through the mirror; the counted frames stay a prefix).  Without
    sample_rate all clips must share one rate (ValueError otherwise); with it, clips at other
    rates are resampled as decode_clip_rows does.  Every keyword is checked, with ValueError, before any device is touched.

    cepstra, deltas: a stage between the mel bank and the normalisation, nvh_cep_rows (include/nvorbis_hip.h states its rule; with
    the five keywords of this paragraph left away nothing new runs).  cepstra=K: the first K coefficients of a DCT-II over the
    bands replace them (MFCCs where scale is "ln" or "db"), with dct_norm "ortho" (Kaldi, torchaudio's norm="ortho") or None
    (torchaudio's norm=None) and lifter = Kaldi's cepstral_lifter folded into the table (0: none).  deltas=1 or 2: delta and
    delta-delta columns over delta_window frames on each side (Kaldi's add-deltas; order 1 is torchaudio's compute_deltas), from
    the row's counted frames alone with the edge frames repeated -- the counted frames are the first valid_frames[i] with
    mask_padding=True, all of them without -- and +0 behind them.  The features then have Q = (1 + deltas) * K columns in place
    of n_mels (K = n_mels without cepstra), statics first; Q is at most 256.  The mel stage writes a temporary (N, C, n_mels, F)
    tensor, and the normalisation runs over the Q columns as it does over bands.  kaldi_mfcc_keywords() returns Kaldi's set.

    normalize: the last stage, nvh_fnorm_rows in place on the features (include/nvorbis_hip.h states its rule).  "mean": the mean
    over the row's counted frames is subtracted, per band with normalize_axis="band" (utterance CMVN, NeMo's per_feature) or one
    mean of all bands with "all" (all_features).  "mean_var": then divided by sqrt(population variance + norm_eps).  "peak":
    (max(x, peak - peak_range) + peak_offset) * peak_gain, `peak` the maximum over the row's counted frames and all bands
    (normalize_axis is not used); with scale="db" the defaults 80, 40, 1/40 are Whisper's.  mask_padding=True: the counted frames
    of row i are its first valid_frames[i] ones, and every frame behind them is set to pad_value.  mask_padding=False: every frame
    counts and none is filled (the exact Whisper form).
    With normalize=None the stage runs only as the fill-only form, which needs mask_padding=True and a pad_value GIVEN BY THE
    CALLER: the default of pad_value is a marker object equal to 0.0, and the stage is told to run by `pad_value is not that
    object`, so that pad_value=0.0 written out fills with zeros while leaving the keyword away keeps today's frames (ln(floor) and
    the like) and launches nothing new.  normalize=None with mask_padding=False has nothing to do and launches nothing either."""
    for name, v in (("center", center), ("band_major", band_major), ("device_out", device_out)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("%s must be True or False, not %r" % (name, v))
    return_clipped = _return_clipped(return_clipped)
    sample_rate = _sample_rate(sample_rate)
    _mix(mix, False)
    if channel_map is not None:
        _channel_map(channel_map, None, mix)
    length = _length(length)
    batch_frames = _batch_frames(batch_frames)
    clips = list(clips)
    starts = _starts(starts, len(clips))
    # the rows' form: f32 on the device, the planes of the planar kernels or the one plane of the mix
    form = _Form(np.dtype(np.float32), mix is None, mix, channel_map, batch_frames, bool(gpu_parse), True,
                 int(device) if ctx is None else ctx.device, clipped=np.zeros(len(clips), dtype=bool) if return_clipped else None)
    recs = _load_clips(clips, "decode_clip_features", sample_rate, True, form)  # (every clip is read once per call)
    _output_channels(recs, form, "decode_clip_features")
    rate = sample_rate
    if rate is None:
        rates = sorted(set(r.rate for r in recs))
        if len(rates) != 1:
            raise ValueError("decode_clip_features: without sample_rate all clips must share one rate (found %s)" % rates)
        rate = rates[0]
    desc = mel_desc(rate, n_fft, win_length, hop, n_mels, f_min, f_max, mel_scale, norm, scale, floor)
    N_, W, H, B = desc.n_fft, desc.win_length, desc.hop, desc.n_mels
    front = mel_front(window, mel_triangles, pad_mode, remove_dc, preemphasis, sample_gain)
    if not isinstance(frame_count, str) or frame_count not in ("n_fft", "window"):
        raise ValueError("frame_count must be 'n_fft' or 'window', not %r" % (frame_count,))
    if frame_count == "window" and center:
        raise ValueError("frame_count='window' needs center=False")
    if pad_mode == "reflect" and not center:
        raise ValueError("pad_mode='reflect' needs center=True")
    if not isinstance(mask_padding, (bool, np.bool_)):
        raise ValueError("mask_padding must be True or False, not %r" % (mask_padding,))
    pad_given = pad_value is not _PAD_DEFAULT
    cdesc = cep_desc(cepstra, dct_norm, lifter, deltas, delta_window, 0, B)  # (checked whether the stage runs or not)
    run_cep = cepstra is not None or cdesc.order > 0
    Q = (1 + cdesc.order) * cdesc.ceps if run_cep else B
    ndesc = fnorm_desc(normalize, normalize_axis, norm_eps, pad_value, peak_range, peak_offset, peak_gain, 0, Q)
    run_fnorm = normalize is not None or (bool(mask_padding) and pad_given)
    if center:
        first, F = (N_ - W) // 2 - N_ // 2, length // H + 1
        if pad_mode == "reflect" and (length < 2 or -first > length - 1 or (F - 1) * H + first + W - 1 > 2 * (length - 1)):
            raise ValueError("pad_mode='reflect' needs one reflection to be enough for every frame: length >= 2, %d <= length - 1 and "
                             "%d <= 2 * (length - 1) (length %d)" % (-first, (F - 1) * H + first + W - 1, length))
    elif frame_count == "window":
        if length < W:
            raise ValueError("frame_count='window' needs length >= win_length (%d < %d)" % (length, W))
        first, F = 0, (length - W) // H + 1
    else:
        if length < N_:
            raise ValueError("center=False needs length >= n_fft (%d < %d)" % (length, N_))
        first, F = (N_ - W) // 2, (length - N_) // H + 1
    if run_fnorm and F > 2 ** 24:
        raise ValueError("normalize takes at most 2**24 frames per row (%d)" % F)
    if run_cep and F > 2 ** 24:
        raise ValueError("cepstra and deltas take at most 2**24 frames per row (%d)" % F)
    begins = np.arange(F, dtype=np.int64) * H + first
    import torch
    with _context(ctx, device) as ctx:
        out = _clip_rows(ctx, recs, starts, length, sample_rate, form)
        (rows, valid), clipped = out if return_clipped else (out, None)
        mono = mix is not None
        n = rows.shape[0]
        och = 1 if mono else rows.shape[1]
        shape = (n, och, Q, F) if band_major else (n, och, F, Q)
        feats = torch.empty(shape, dtype=torch.float32, device=rows.device)
        mel_out, mel_major = (torch.empty((n, och, B, F), dtype=torch.float32, device=rows.device), True) if run_cep else (feats, band_major)
        if n and och:
            desc.rows, desc.channels, desc.frames, desc.first, desc.src_length = n, och, F, first, length
            if length:
                desc.src_row_stride, desc.src_time_stride = rows.stride(0), rows.stride(-1)
                desc.src_chan_stride = 0 if mono else rows.stride(1)
            else:  # no samples at all: every frame is the transform of zeros (the source is never read)
                rows = torch.zeros(1, dtype=torch.float32, device=rows.device)
            desc.dst_row_stride, desc.dst_chan_stride = mel_out.stride(0), mel_out.stride(1)
            desc.dst_band_stride, desc.dst_frame_stride = (mel_out.stride(2), mel_out.stride(3)) if mel_major else (mel_out.stride(3), mel_out.stride(2))
            torch.cuda.current_stream(rows.device).synchronize()  # (a gather of several setups' rows runs on torch's stream)
            ctx.mel_rows(desc, rows.data_ptr(), mel_out.data_ptr(), valid, front)
        valid_frames = (np.maximum(begins, 0)[None, :] < np.minimum(begins[None, :] + W, valid[:, None])).sum(axis=1).astype(np.int64)
        if n and och:
            col_stride, frame_stride = (feats.stride(2), feats.stride(3)) if band_major else (feats.stride(3), feats.stride(2))
            if run_cep:  # behind k_mel_rows on the context's stream, out of the temporary tensor
                cdesc.rows, cdesc.channels, cdesc.frames = n, och, F
                cdesc.src_row_stride, cdesc.src_chan_stride = desc.dst_row_stride, desc.dst_chan_stride
                cdesc.src_frame_stride, cdesc.src_band_stride = desc.dst_frame_stride, desc.dst_band_stride
                cdesc.dst_row_stride, cdesc.dst_chan_stride = feats.stride(0), feats.stride(1)
                cdesc.dst_frame_stride, cdesc.dst_col_stride = frame_stride, col_stride
                ctx.cep_rows(cdesc, mel_out.data_ptr(), feats.data_ptr(), valid_frames if mask_padding else None)
            if run_fnorm:  # behind the kernels before it on the context's stream, in place
                ndesc.rows, ndesc.channels, ndesc.frames = n, och, F
                ndesc.src_row_stride = ndesc.dst_row_stride = feats.stride(0)
                ndesc.src_chan_stride = ndesc.dst_chan_stride = feats.stride(1)
                ndesc.src_frame_stride = ndesc.dst_frame_stride = frame_stride
                ndesc.src_band_stride = ndesc.dst_band_stride = col_stride
                ctx.fnorm_rows(ndesc, feats.data_ptr(), feats.data_ptr(), valid_frames if mask_padding else None)
            ctx.synchronize()
    if mono:
        feats = feats[:, 0]
    if not device_out:
        feats = feats.cpu().numpy()
    res = (feats, valid, valid_frames)
    return (res, clipped) if return_clipped else res

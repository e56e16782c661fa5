"""Clip batches: many short Ogg Vorbis files of one encoder setup, decoded as segments of shared batches.

A sound-effect bank, a set of speech clips or a dataset shard is thousands of short streams with byte-identical
identification and setup headers.  One stream per clip pays for its setup upload, at least two launches, a synchronisation and
a read-back per clip; here every group of clips with the same setup is ONE stream, each clip a segment of it
(Stream.next_segment, include/nvorbis_hip.h), and a batch of `batch_frames` frames -- however many clips that is -- goes
through one upload, one parse and one set of launches.
"""
import numpy as np

from . import native
from .reader import (Context, Stream, _channel_map, _layout, _mix, _pcm_out, _sample_format, demux_ogg_array)


def _clip_error(index, err, where=None):
    """`err` (an NvhError) as the error of clip `index`."""
    e = native.NvhError(err.code, "decode_clips: clip %d: %s" % (index, where or "decode"))
    e.clip = index
    return e


class _Group:
    """One setup's clips on one Stream: pushes them as segments, synthesises whenever batch_frames frames are pending and
    routes every batch through its segment table."""

    def __init__(self, ctx, first, members, packets, opts):
        self.members, self.packets, self.opts = members, packets, opts
        pa = packets[first]
        self.stream = Stream(ctx, pa[0], pa[1], pa[2])
        self.pieces = {i: [] for i in members}

    def run(self):
        o, st = self.opts, self.stream
        if o["gpu_parse"]:  # stream shapes outside the GPU parser's limits keep the host parser, as in VorbisReader
            try:
                st.set_gpu_parse(True)
            except native.NvhError as e:
                if e.code != native.ERR_UNSUPPORTED:
                    raise
        for i in self.members:
            pa, nxt = self.packets[i], 3
            while nxt < len(pa):
                room = o["batch_frames"] - st.pending()[0]
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
            st.next_segment(o["align"])
        self.flush()

    def flush(self):
        o, st = self.opts, self.stream
        frames, samples = st.pending()
        if not frames:
            return
        table = st.pending_segments()
        och, planar = o["och"](st.channels), o["planar"]
        if o["device_out"]:
            import torch
            dev = "cuda:%d" % o["device"]
            tdt = torch.int16 if o["dtype"] == np.dtype(np.int16) else torch.float32
            if planar:
                stride = max((samples + 3) & ~3, 4)
                out = torch.empty((och, stride), dtype=tdt, device=dev)
                st.synth_device(out.data_ptr(), 0, dtype=o["dtype"], plane_stride=stride, channel_map=o["map"](st.channels))
            else:
                out = torch.empty(max(samples * och, 1), dtype=tdt, device=dev)
                st.synth_device(out.data_ptr(), out.numel(), dtype=o["dtype"], mix=o["mix"], channel_map=o["map"](st.channels))
        else:
            out = st.synth_host(pinned=True, dtype=o["dtype"], planar=planar, mix=o["mix"], channel_map=o["map"](st.channels))
        if st.parse_errors:  # GPU-parse mode: a packet of this batch made the parser fail; positions up to it are the table's
            err, at = st.parse_errors[0]
            at //= 1 if (planar or o["mix"] is not None) else och
            # the segment whose range holds the position; a packet that leaves no samples there (a clip's first): the first
            # non-empty segment that begins at it, else the last one that begins before it
            inside = np.nonzero((table[:, 1] <= at) & (at < table[:, 2]))[0]
            row = inside[0] if inside.size else max(int(np.searchsorted(table[:, 1], at, side="right")) - 1, 0)
            k = int(table[row, 0])
            raise _clip_error(self.members[k], err, "a packet the parser fails on")
        for k, b, e in table:
            if e > b:
                piece = out[:, b:e] if planar else out[b * och:e * och]
                # (a host batch lies in the stream's page-locked buffer, which the next batch overwrites)
                self.pieces[self.members[int(k)]].append(piece if o["device_out"] else piece.copy())

    def results(self, into):
        o, st = self.opts, self.stream
        och = o["och"](st.channels)
        for i in self.members:
            ps = self.pieces[i]
            if o["device_out"]:
                import torch
                if not ps:
                    tdt = torch.int16 if o["dtype"] == np.dtype(np.int16) else torch.float32
                    ps = [torch.empty((och, 0) if o["planar"] else (0,), dtype=tdt, device="cuda:%d" % o["device"])]
                into[i] = ps[0] if len(ps) == 1 else torch.cat(ps, dim=-1)  # (a clip inside one batch: a view of that batch's output)
            else:
                if not ps:
                    ps = [np.zeros((och, 0) if o["planar"] else (0,), dtype=o["dtype"])]
                into[i] = ps[0] if len(ps) == 1 else np.concatenate(ps, axis=-1)


def decode_clips(clips, ctx=None, device=0, batch_frames=4096, gpu_parse=True, sample_format="f32", layout="interleaved", mix=None,
                 channel_map=None, align=4, device_out=False):
    """Decode a list of Ogg Vorbis clips (bytes or paths; logical stream 0 of each) and return one array per clip, in input
    order: what VorbisReader(clip, <the same options>).read_all() returns for it, bit for bit.

    Clips are grouped by identical identification and setup packets (the comment packet may differ).  Every group is one Stream;
    each clip's packets are pushed with their granules and flags and closed with next_segment(align); synthesis runs whenever
    `batch_frames` frames are pending -- in the middle of a clip if need be -- and every batch is taken apart by its segment
    table.  align=4 keeps every clip of a batch on the kernels' vector paths (include/nvorbis_hip.h).

    Host results are numpy arrays: (T * channels,) interleaved, (channels, T) for layout="planar", (T,) for mix="mono".
    device_out=True: torch tensors on the device instead -- views of the batch outputs for clips that lie inside one batch.

    A clip whose headers or packets make the library return an error raises NvhError with the clip's index in the message (and
    as its `clip` attribute); there are no partial results."""
    dtype = _sample_format(sample_format)
    planar = _layout(layout)
    _mix(mix, planar)
    if channel_map is not None:
        _channel_map(channel_map, None, mix)
    if isinstance(align, bool) or not isinstance(align, (int, np.integer)) or align < 1 or align > 65536 or align & (align - 1):
        raise ValueError("align must be a power of two in [1, 65536], not %r" % (align,))
    if int(batch_frames) < 1:
        raise ValueError("batch_frames must be at least 1")
    packets, groups = [], {}
    for i, src in enumerate(clips):
        if isinstance(src, (bytes, bytearray, memoryview)):
            data = bytes(src)
        else:
            with open(src, "rb") as fh:
                data = fh.read()
        try:
            pa = demux_ogg_array(data, 0)
            if len(pa) < 3:
                raise native.NvhError(native.ERR_NOT_VORBIS, "decode_clips")
            key = (pa[0], pa[2])
            # every clip's own three headers are looked at, on the host (a setup seen before on this thread is not parsed again)
            Stream(None, pa[0], pa[1], pa[2]).close()
        except native.NvhError as e:
            raise _clip_error(i, e, "headers")
        packets.append(pa)
        groups.setdefault(key, []).append(i)
    own_ctx = ctx is None and bool(groups)
    if own_ctx:
        ctx = Context(device)
    opts = {
        "batch_frames": int(batch_frames), "gpu_parse": bool(gpu_parse), "dtype": dtype, "planar": planar, "mix": mix,
        "align": int(align), "device_out": bool(device_out), "device": ctx.device if ctx is not None else int(device),
        # the map of a stream of `ch` channels ("wave" depends on the count), and the samples per sample time it leaves
        "map": lambda ch: _channel_map(channel_map, ch, mix),
        "och": lambda ch: _pcm_out(dtype, planar, mix, channel_map, ch)[2],
    }
    results = [None] * len(packets)
    try:
        for members in groups.values():
            try:
                g = _Group(ctx, members[0], members, packets, opts)
            except native.NvhError as e:
                raise _clip_error(members[0], e, "nvh_stream_open")
            try:
                g.run()
                g.results(results)
            finally:
                g.stream.close()
    finally:
        if own_ctx:
            ctx.close()
    return results

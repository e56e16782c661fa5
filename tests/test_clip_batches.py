"""Clip batches: many short runs of packets under one setup as SEGMENTS of one stream (nvh_stream_next_segment,
nvh_stream_pending_segments, nv.decode_clips; include/nvorbis_hip.h states the rule).

A clip is a run of consecutive audio packets of one stream behind that stream's three headers.  The reference of every
comparison is the oracle run on ONE clip alone -- oracle.decode_packets(headers + run, granules, flags) -- never the library's own
single-stream output (the one exception is the existing suites': Floor0 under the descriptor-kernel toggles).  No tolerance
anywhere: a segment's samples are the fresh stream's samples, bit for bit, and the gaps the alignment opens are zeros."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKT_EOS = 1

# (first packet, run length, ending): "none" = no end-of-stream packet (next_segment drains the tail), "eos" = NVH_PKT_EOS on the
# last packet without a granule (T0 samples), an int k = NVH_PKT_EOS with granule T0 - k (the clip is trimmed to T0 - k samples).
# Run lengths {1, 2, 3, 5, 24} and one empty clip (two boundaries in a row).  Frames add up to 13 after clip 4 and to 39 after
# clip 7: with batches of 13 frames a batch boundary falls exactly on those clip boundaries (test_core_parity and the host-only
# test_batches_of_13_meet_clip_boundaries assert that this happened, for every setup).
SHAPES = [(40, 2, "eos"), (40, 2, "none"), (40, 2, 1), (41, 5, "eos"), (40, 2, 2), (60, 24, "eos"), (40, 1, "eos"), (40, 1, "none"),
          (40, 2, 3), (41, 5, "none"), (60, 24, 1), (40, 2, 5), (0, 0, "none"), (43, 3, "none"), (60, 24, 5), (60, 24, "none")]
SENTINEL = {np.dtype(np.float32): np.float32(-1234.5), np.dtype(np.int16): np.int16(-7777)}
CLIP = np.float32(0.99999994)


def to_s16(x):
    """ov_read's conversion (test_pcm_s16.py): float32 multiply, round half to even, clamp, NaN -> 0."""
    y = np.rint(np.asarray(x, np.float32) * np.float32(32768.0))
    y = np.where(np.isnan(y), np.float32(0.0), y)
    return np.clip(y, -32768, 32767).astype(np.int16)


def mix_rule(x, ch, clip):
    """The mono mix's rule (include/nvorbis_hip.h, test_pcm_mix.py) on interleaved UNCLIPPED float32 PCM."""
    p = np.asarray(x, np.float32).reshape(-1, ch)
    s = p[:, 0].copy()
    for c in range(1, ch):
        s = (s + p[:, c]).astype(np.float32)
    with np.errstate(all="ignore"):
        m = (s / np.float32(ch)).astype(np.float32)
    if clip:
        m = np.where(m > CLIP, CLIP, np.where(m < -CLIP, -CLIP, m)).astype(np.float32)
    return m


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# clips and their references (computed once per stream, shared, never modified)
# ---------------------------------------------------------------------------------------------------------------------------

_STREAMS, _CLIPS, _REFS = {}, {}, {}


def stream_packets(oracle, name):
    """The packet list every clip of a test is cut from: a shipped file, or ONE filtered_stream of a synthetic setup."""
    if name not in _STREAMS:
        import nvorbis_amd as nv
        if name.endswith(".ogg"):
            pk, _, _ = nv.demux_ogg(open(os.path.join(GOLDEN, name), "rb").read())
        else:
            from tests import synth_stream as ss
            pk, _, _ = ss.filtered_stream(oracle, name, 100, 11)
        _STREAMS[name] = list(pk)
    return _STREAMS[name]


def make_clips(oracle, name, shapes=SHAPES):
    """[(run, granules, flags)] of `shapes` cut from stream `name`."""
    key = (name, tuple(shapes))
    if key not in _CLIPS:
        pk = stream_packets(oracle, name)
        hdr, clips = pk[:3], []
        for first, n, end in shapes:
            assert first + n <= len(pk), (name, first, n)
            run, g, f = list(pk[first:first + n]), [-1] * n, [0] * n
            if end != "none" and n:
                f[-1] = PKT_EOS
            if isinstance(end, int):
                pcm, info = oracle.decode_packets(hdr + run, [-1] * (3 + n), [0] * 3 + f)
                t0 = pcm.size // info["channels"]
                assert t0 > end, (name, first, n, t0)
                g[-1] = t0 - end
            clips.append((run, g, f))
        _CLIPS[key] = clips
    return _CLIPS[key]


def oracle_clips(oracle, name, clip=True, shapes=SHAPES):
    """The oracle on each clip alone: [(interleaved float32 PCM, HasClipped)], and the channel count."""
    key = (name, bool(clip), tuple(shapes))
    if key not in _REFS:
        hdr = stream_packets(oracle, name)[:3]
        out, ch = [], None
        for run, g, f in make_clips(oracle, name, shapes):
            pcm, info = oracle.decode_packets(hdr + run, [-1] * 3 + g, [0] * 3 + f, clip=clip)
            pcm.setflags(write=False)
            ch = info["channels"]
            out.append((pcm, info["has_clipped"]))
        _REFS[key] = (out, ch)
    return _REFS[key]


class Segmented:
    """One stream fed clips as segments.  Batches are flushed at `bf` pending frames: for clips with an even index when the next
    packet finds the batch full (so a clip that ends exactly there gets its boundary BEFORE the synthesis: the next batch's first
    frame has no overlap source), for clips with an odd index as soon as it is full (the boundary comes after the synthesis, and
    drains the carried tail into the next batch).  synth(st, table, n) synthesises the pending batch and returns its samples as
    rows [n, output channels] -- gaps included -- or None when it delivers them later through route()."""

    def __init__(self, st, nclips, bf, align, synth):
        self.st, self.bf, self.align, self.synth = st, bf, align, synth
        self.pieces = [[] for _ in range(nclips + 1)]  # (+ the segment left open behind the last clip: always empty)
        self.tables, self.kernels = [], []

    def flush(self):
        st = self.st
        frames, n = st.pending()
        if not frames:
            return
        table = st.pending_segments()
        assert table[-1, 2] == n and (table[:, 1] <= table[:, 2]).all() and (table[1:, 1] >= table[:-1, 2]).all(), table
        assert (table[1:, 1] % self.align == 0).all(), (self.align, table)
        self.tables.append(table)
        rows = self.synth(st, table, n)
        if st._ctx is not None:
            self.kernels.append(st.kernels())
        if rows is not None:
            self.route(table, rows)

    def route(self, table, rows):
        covered = np.zeros(rows.shape[0], bool)
        for k, b, e in table:
            self.pieces[int(k)].append(rows[b:e].copy())
            covered[b:e] = True
        assert not rows[~covered].any(), "a gap holds something other than zeros"  # (+0.0 / 0: all bits clear)
        assert not rows[~covered].view(np.uint8).any()

    def run(self, clips):
        st = self.st
        for i, (run, g, f) in enumerate(clips):
            for p, gr, fl in zip(run, g, f):
                if st.pending()[0] >= self.bf:
                    self.flush()
                st.push_packet(p, gr, fl)
                if i % 2 == 1 and st.pending()[0] >= self.bf:
                    self.flush()
            st.next_segment(self.align)
        self.flush()
        assert not any(p.size for p in self.pieces[-1])
        return self

    def clip_rows(self, i, och, dt):
        ps = self.pieces[i]
        return np.concatenate(ps) if ps else np.zeros((0, och), dt)


def boundary_on_batch_boundary(tables):
    """Some batch ended exactly on a clip boundary that was passed BEFORE its synthesis: its table ends in an empty open segment,
    and the next batch's table begins with that segment, at 0, with samples in it."""
    return any(p[-1, 1] == p[-1, 2] and len(p) > 1 and t[0, 0] == p[-1, 0] and t[0, 1] == 0 and t[0, 2] > 0
               for p, t in zip(tables, tables[1:]))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: host-only streams
# ---------------------------------------------------------------------------------------------------------------------------

NAMES = ("nvh_stream_next_segment", "nvh_stream_pending_segments", "nvh_stream_synth_segments")
CPU_STREAMS = ["stereo_res1_coupled", "3test.ogg"]


def test_segment_entry_points_are_exported_and_declared():
    from nvorbis_amd import native
    L = native.lib()
    hdr = open(os.path.join(ROOT, "include", "nvorbis_hip.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "NativeMethods.cs")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in native.SIGNATURES, name
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern (?:unsafe )?int %s\(" % name, cs), name


def test_segment_entry_points_refuse_bad_arguments(oracle):
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    n = C.c_int(-1)
    a = (C.c_int64 * 3 * 4)()
    assert L.nvh_stream_next_segment(None, 4) == native.ERR_ARGUMENT
    assert L.nvh_stream_pending_segments(None, a[0], a[1], a[2], 4, C.byref(n)) == native.ERR_ARGUMENT
    pk = stream_packets(oracle, "3test.ogg")
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for bad in (0, 3, 131072, -4, 6):
            assert L.nvh_stream_next_segment(st._h, bad) == native.ERR_ARGUMENT, bad
            with pytest.raises(native.NvhError):
                st.next_segment(bad)
        assert np.array_equal(st.pending_segments(), [[0, 0, 0]])  # the refused calls made no segment
        for ok in (1, 2, 4, 65536):
            st.next_segment(ok)
        assert L.nvh_stream_pending_segments(st._h, a[0], a[1], a[2], 4, None) == native.ERR_ARGUMENT
        assert L.nvh_stream_pending_segments(st._h, None, a[1], a[2], 4, C.byref(n)) == native.ERR_ARGUMENT
        n.value = -1
        assert L.nvh_stream_pending_segments(st._h, a[0], a[1], a[2], 4, C.byref(n)) == native.ERR_ARGUMENT  # five entries
        assert n.value == 5
        n.value = -1
        assert L.nvh_stream_pending_segments(st._h, None, None, None, 0, C.byref(n)) == native.ERR_ARGUMENT and n.value == 5
        assert np.array_equal(st.pending_segments(), [[k, 0, 0] for k in range(5)])  # empty segments, numbered from 0
    finally:
        st.close()


def _own_geometry(nv, hdr, clip):
    """A fresh host-only stream over one clip: (geometry, samples, slab words, first unit of every slab)."""
    run, g, f = clip
    st = nv.Stream(None, hdr[0], hdr[1], hdr[2])
    try:
        for p, gr, fl in zip(run, g, f):
            st.push_packet(p, gr, fl)
        st.push_end()
        geo, n = st.pending_geometry().copy(), st.pending()[1]
        words, first = st.pending_slabs()
        return geo, n, words.copy(), first.copy()
    finally:
        st.close()


SLAB_FRAME_WORD = 6  # NvhSlabHdr::frame (nvh_format.h): the frame a slab belongs to -- an index into the batch


@pytest.mark.parametrize("name", CPU_STREAMS)
def test_segment_table_and_geometry_are_the_clips_own(oracle, name):
    """The segmented batch is the concatenation of the clips' own batches: table lengths = the oracle's per-clip sample counts
    (align 1, 4, 64; begins on multiples of align), geometry = each clip's own with in-batch overlap sources shifted by the frame
    offset (emit counts add up to the table's lengths: out_pos shifted by begin), slabs = each clip's own bytes (the slab header's
    frame index, an index into the batch, shifted by the frame offset like the overlap sources)."""
    import nvorbis_amd as nv
    pk = stream_packets(oracle, name)
    hdr = pk[:3]
    clips = make_clips(oracle, name)
    assert len(clips) >= 12
    refs, ch = oracle_clips(oracle, name)
    want = [r.size // ch for r, _ in refs]
    own = [_own_geometry(nv, hdr, c) for c in clips]
    assert [o[1] for o in own] == want  # (a fresh stream of the library agrees with the oracle on the counts)
    for align in (1, 4, 64):
        st = nv.Stream(None, hdr[0], hdr[1], hdr[2])
        try:
            for run, g, f in clips:
                for p, gr, fl in zip(run, g, f):
                    st.push_packet(p, gr, fl)
                st.next_segment(align)
            table = st.pending_segments()
            assert table.dtype == np.int64 and table.shape == (len(clips) + 1, 3)
            assert np.array_equal(table[:, 0], np.arange(len(clips) + 1))
            assert [int(e - b) for _, b, e in table[:-1]] == want, (align, table)
            assert (table[:, 1] % align == 0).all() and table[0, 1] == 0
            assert (table[1:, 1] - table[:-1, 2] >= 0).all() and (table[1:, 1] - table[:-1, 2] < align).all()
            assert table[-1, 1] == table[-1, 2] == st.pending()[1]  # the open segment is empty; gaps count as samples
            if align == 1:  # the trims put later segments on every residue mod 4
                assert set(int(b) % 4 for b in table[:-1, 1]) == {0, 1, 2, 3}, table[:, 1] % 4
            geo = st.pending_geometry()
            words, first = st.pending_slabs()
            cat, cat_words, cat_first, off, unit = [], [], [0], 0, 0
            for (g1, n1, w1, f1), (_, b, e) in zip(own, table):
                g1, w1 = g1.copy(), w1.copy()
                g1[g1[:, 6] >= 0, 6] += off
                assert g1[:, 5].sum() == e - b
                for s in f1[:-1]:
                    w1[int(s) * 4 + SLAB_FRAME_WORD] += off
                cat.append(g1)
                cat_words.append(w1)
                cat_first += [int(s) + unit for s in f1[1:]]
                off += g1.shape[0]
                unit += int(f1[-1])
            assert np.array_equal(geo, np.concatenate(cat)), align
            assert np.array_equal(first, np.asarray(cat_first, np.uint32)), align
            assert np.array_equal(words, np.concatenate(cat_words)), align
        finally:
            st.close()


@pytest.mark.parametrize("name", CPU_STREAMS)
def test_a_stream_without_segments_is_unchanged(oracle, name):
    """A stream that never calls next_segment: the table is {0, 0, pending}, and a stream driven by the old calls alone reports
    the geometry and the table of one that is also asked for its segments between the pushes."""
    import nvorbis_amd as nv
    pk = stream_packets(oracle, name)
    a, b = nv.Stream(None, pk[0], pk[1], pk[2]), nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for k, i in enumerate(range(3, 3 + 60)):
            for st in (a, b):
                st.push_packet(pk[i], -1, 0)
            assert np.array_equal(a.pending_segments(), [[0, 0, a.pending()[1]]])
            if k == 30:  # a batch boundary by the old calls
                assert np.array_equal(a.pending_geometry(), b.pending_geometry())
                a.drop_pending()
                b.drop_pending()
                assert np.array_equal(a.pending_segments(), [[0, 0, 0]])
        for st in (a, b):
            st.push_end()
        assert np.array_equal(a.pending_geometry(), b.pending_geometry()) and a.pending() == b.pending()
        assert a.pending_geometry()[0, 6] == -2  # carried across the boundary as ever
        assert np.array_equal(a.pending_segments(), [[0, 0, a.pending()[1]]])
        assert np.array_equal(b.pending_segments(), [[0, 0, b.pending()[1]]])
        assert a.position() == b.position()
    finally:
        a.close()
        b.close()


def test_boundaries_at_and_across_batch_boundaries(oracle):
    """A segment boundary exactly at a batch boundary: the next batch's first frame has no overlap source (-1, not the carried
    tail's -2).  A segment across a batch boundary: -2, and the table's first entry repeats the index.  nvh_stream_reset restarts
    the numbering; nvh_stream_position reports the current segment."""
    import nvorbis_amd as nv
    pk = stream_packets(oracle, "3test.ogg")
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for i in range(40, 45):
            st.push_packet(pk[i], -1, 0)
        st.next_segment(4)
        assert np.array_equal(st.pending_segments()[:, 0], [0, 1])
        st.drop_pending()  # the batch boundary, exactly on the segment boundary
        assert np.array_equal(st.pending_segments(), [[1, 0, 0]])
        assert st.position() == (0, 0, False)
        for i in range(60, 64):
            st.push_packet(pk[i], -1, 0)
        geo = st.pending_geometry()
        assert geo[0, 6] == -1 and geo[0, 5] == 0 and geo[0, 7] == 0, geo[0]  # a first packet: no overlap, emits nothing
        assert geo[1, 6] == 0
        emitted = st.pending()[1]
        assert st.position()[1] == emitted  # this segment's samples, not the stream's
        st.drop_pending()  # a batch boundary inside segment 1
        assert np.array_equal(st.pending_segments(), [[1, 0, 0]])
        st.push_packet(pk[64], -1, 0)
        assert st.pending_geometry()[0, 6] == -2
        st.next_segment(4)
        st.push_packet(pk[70], -1, 0)
        t = st.pending_segments()
        assert np.array_equal(t[:, 0], [1, 2]) and t[0, 1] == 0 and t[0, 2] > 0 and t[1, 1] == t[1, 2], t
        # the boundary right behind a batch boundary drains the carried tail into the new batch
        st.push_packet(pk[71], -1, 0)
        st.drop_pending()
        st.next_segment(1)
        geo = st.pending_geometry()
        assert geo.shape[0] == 1 and geo[0, 0] == 0 and geo[0, 6] == -2 and geo[0, 5] == geo[0, 7] > 0, geo
        tail = int(geo[0, 5])
        assert np.array_equal(st.pending_segments(), [[2, 0, tail], [3, tail, tail]])
        st.reset()
        assert np.array_equal(st.pending_segments(), [[0, 0, 0]])
        st.next_segment(1)
        assert np.array_equal(st.pending_segments(), [[0, 0, 0], [1, 0, 0]])
    finally:
        st.close()


@pytest.mark.parametrize("name", ["stereo_res1_coupled", "mono_res0_small_blocks", "six_ch_res2_4096", "stereo_8192", "floor0_slab",
                                  "3test.ogg"])
def test_batches_of_13_meet_clip_boundaries(oracle, name):
    """The driver of the GPU tests on a host-only stream (the batch is dropped instead of synthesised): with batches of 13 frames
    every setup has a batch boundary exactly on a clip boundary, one inside a clip, and a boundary that drains the carried tail."""
    import nvorbis_amd as nv
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name)
    firsts = []

    def drop(st, table, n):
        firsts.append(st.pending_geometry()[0].copy())
        st.drop_pending()
        return None
    st = nv.Stream(None, hdr[0], hdr[1], hdr[2])
    try:
        seg = Segmented(st, len(clips), 13, 4, drop).run(clips)
    finally:
        st.close()
    assert boundary_on_batch_boundary(seg.tables), seg.tables
    assert any(t[0, 0] == p[-1, 0] and p[-1, 2] > p[-1, 1] for p, t in zip(seg.tables, seg.tables[1:]))
    assert any(f[0] != 0 and f[6] == -1 for f in firsts[1:])  # a batch that begins with a first packet: no overlap source
    assert any(f[6] == -2 for f in firsts[1:])                # ... and one that begins over the carried tail


def exec_share(nv, hdr, clip_packets):
    """Of one clip alone (host-only stream, slab headers: NvhSlabHdr::exec_mask): frames, and frames in which every channel
    executes in the frame and in the frame before it -- the most that paired emission can take."""
    run, g, f = clip_packets
    st = nv.Stream(None, hdr[0], hdr[1], hdr[2])
    try:
        for p, gr, fl in zip(run, g, f):
            st.push_packet(p, gr, fl)
        st.push_end()
        words, first = st.pending_slabs()
        full = [((int(words[int(u) * 4]) >> 16) & 0xFF) & ((1 << st.channels) - 1) == (1 << st.channels) - 1 for u in first[:-1]]
        return len(full), sum(1 for i in range(1, len(full)) if full[i] and full[i - 1])
    finally:
        st.close()


ROUTING_SHAPES = {n: tuple((4 + step * k, 24, ("none", 1, "eos", 3, 2, 5)[k % 6]) for k in range(12))
                  for n, step in (("3test.ogg", 25), ("stereo_res1_coupled", 6))}


def test_routing_streams_and_the_emission_threshold(oracle):
    """Why test_routing_keeps_paired_emission names k_synth_group2 on 3test.ogg only: in every 24-frame clip cut from
    stereo_res1_coupled (random packets) fewer than 7/8 of the frames have all channels executing in the frame and the one before,
    so assign_emission's threshold keeps such a batch off paired emission, segmented or not; 3test.ogg's clips are above it."""
    import nvorbis_amd as nv
    for name, above in (("3test.ogg", True), ("stereo_res1_coupled", False)):
        hdr = stream_packets(oracle, name)[:3]
        shares = [exec_share(nv, hdr, c) for c in make_clips(oracle, name, ROUTING_SHAPES[name])]
        assert all(n == 24 for n, _ in shares)
        if above:
            assert all((k - 1) * 8 >= n * 7 for n, k in shares), shares  # (k - 1: the clip's last frame is a drained tail or a trim)
        else:
            assert all(k * 8 < n * 7 for n, k in shares), shares
            assert shares[0] == (24, 11)


def test_decode_clips_checks_its_arguments_before_a_device():
    import nvorbis_amd as nv
    from nvorbis_amd import native
    assert nv.decode_clips([]) == []
    for kw in ({"sample_format": "s24"}, {"layout": "tiled"}, {"mix": "stereo"}, {"mix": "mono", "layout": "planar"}, {"align": 3},
               {"align": 0}, {"align": 131072}, {"channel_map": (0, 0)}, {"batch_frames": 0}):
        with pytest.raises(ValueError):
            nv.decode_clips([b"x"], **kw)
    good = open(os.path.join(GOLDEN, "3test.ogg"), "rb").read()
    with pytest.raises(native.NvhError) as e:
        nv.decode_clips([good[:40000], b"not an ogg file at all, and long enough to be looked at" * 4])
    assert "clip 1" in str(e.value) and e.value.clip == 1


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _descriptor_toggle():
    return any(os.environ.get(t) for t in ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB"))


def _device_synth(torch, dt=np.float32, och=None, planar=False, pad=64, **form):
    """synth(st, table, n) into a device destination pre-filled with a sentinel: the call writes `n` sample times and nothing
    else -- nothing behind them, and in the planar layout (a stride larger than the batch) nothing between the planes."""
    dt = np.dtype(dt)
    tdt = torch.int16 if dt == np.int16 else torch.float32
    sent = SENTINEL[dt]

    def synth(st, table, n):
        oc = och or st.channels
        if planar:
            stride = ((n + 3) & ~3) + pad
            buf = torch.full((oc * stride + pad,), float(sent) if dt != np.int16 else int(sent), dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            wr = st.synth_device(buf.data_ptr(), 0, dtype=dt, plane_stride=stride, **form)
            host = buf.cpu().numpy()
            assert wr == n
            planes = host[:oc * stride].reshape(oc, stride)
            assert (planes[:, n:] == sent).all() and (host[oc * stride:] == sent).all()
            return np.ascontiguousarray(planes[:, :n].T)
        buf = torch.full((n * oc + pad,), float(sent) if dt != np.int16 else int(sent), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        wr = st.synth_device(buf.data_ptr(), n * oc, dtype=dt, **form)
        host = buf.cpu().numpy()
        assert wr == n * oc
        assert (host[n * oc:] == sent).all()
        return host[:n * oc].reshape(n, oc).copy()
    return synth


def _open(nv, ctx, hdr, gpu_parse, clip=True):
    st = nv.Stream(ctx, hdr[0], hdr[1], hdr[2])
    if gpu_parse:
        st.set_gpu_parse(True)
    st.set_clip(clip)
    return st


def _own_output(nv, ctx, hdr, clip_packets, clip):
    """The library's own fresh stream over one clip (only where the existing suites hold Floor0 to it: the descriptor toggles)."""
    run, g, f = clip_packets
    st = _open(nv, ctx, hdr, False, clip)
    try:
        for p, gr, fl in zip(run, g, f):
            st.push_packet(p, gr, fl)
        st.push_end()
        return st.synth_host().copy() if st.pending()[0] else np.zeros(0, np.float32)
    finally:
        st.close()


CORE = [(n, g) for n in ("stereo_res1_coupled", "mono_res0_small_blocks", "six_ch_res2_4096", "stereo_8192", "floor0_slab", "3test.ogg")
        for g in (False, True) if not (n == "floor0_slab" and g)]  # Floor0: the host parser only (the GPU parser refuses it)


@pytest.mark.gpu
@pytest.mark.parametrize("name,gpu_parse", CORE)
def test_core_parity(oracle, gpu_ctx, name, gpu_parse):
    """16 clips of every shape as segments of one stream, batches of 13 frames (boundaries inside clips and exactly on clip
    boundaries) and of 1024, align 1 and 4, ClipSamples on and off: every clip's samples are the oracle's for that clip alone,
    the gaps are zeros, nothing past `written` is touched, HasClipped is the OR of the oracle's per-clip flags."""
    torch = _torch()
    import nvorbis_amd as nv
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name)
    exact_ref = not (name.startswith("floor0") and _descriptor_toggle())
    for clip in (True, False):
        refs, ch = oracle_clips(oracle, name, clip)
        if not exact_ref:
            refs = [(_own_output(nv, gpu_ctx, hdr, c, clip), hc) for c, (_, hc) in zip(clips, refs)]
        for bf in (13, 1024):
            for align in (1, 4):
                st = _open(nv, gpu_ctx, hdr, gpu_parse, clip)
                try:
                    seg = Segmented(st, len(clips), bf, align, _device_synth(torch)).run(clips)
                    for i, (ref, _) in enumerate(refs):
                        got = seg.clip_rows(i, ch, np.float32).reshape(-1)
                        assert same_bits(got, ref), (name, gpu_parse, clip, bf, align, i, got.size, ref.size)
                    assert st.has_clipped() == any(hc for _, hc in refs), (name, gpu_parse, clip, bf, align)
                    if bf == 13:
                        assert len(seg.tables) > 4
                        # a segment across a batch boundary: the table's first entry repeats the index
                        assert any(t[0, 0] == p[-1, 0] and t[0, 2] > 0 and p[-1, 2] > p[-1, 1] for p, t in zip(seg.tables, seg.tables[1:]))
                        assert boundary_on_batch_boundary(seg.tables), (name, seg.tables)  # ... and one exactly on a clip boundary
                    if align == 1 and bf == 1024:
                        assert set(int(b) % 4 for b in seg.tables[0][:-1, 1]) == {0, 1, 2, 3}
                finally:
                    st.close()


def _route_alone(nv, ctx, hdr, clip_packets):
    """The synthesis slot a fresh stream over one clip names."""
    run, g, f = clip_packets
    st = _open(nv, ctx, hdr, False)
    try:
        for p, gr, fl in zip(run, g, f):
            st.push_packet(p, gr, fl)
        st.push_end()
        st.synth_host()
        return st.kernels()[1]
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["3test.ogg", "stereo_res1_coupled"])
def test_routing_keeps_paired_emission(oracle, gpu_ctx, name):
    """Twelve 24-frame clips, one batch.  align 4: the batch takes the route each of its clips takes alone, although the trimmed
    clips end on odd samples -- on 3test.ogg that is the emitting family, k_synth_group2 (22 of a clip's 24 frames emit: above the
    7/8 threshold of assign_emission).  align 1: the same bits, whatever ran.

    stereo_res1_coupled never reaches that threshold, segmented or not: its packets are random bits, and in the clips used here
    fewer than 7/8 of the frames have every channel executing in the frame and in the one before it
    (test_routing_streams_and_the_emission_threshold counts them: 11 of 24 in the first clip), so a fresh stream over such a clip runs k_synth + k_ola_compact as well.  The family's name is therefore
    asserted on the real packets, and the unchanged route on both."""
    torch = _torch()
    import nvorbis_amd as nv
    shapes = ROUTING_SHAPES[name]
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name, shapes)
    refs, ch = oracle_clips(oracle, name, True, shapes)
    alone = {_route_alone(nv, gpu_ctx, hdr, c) for c in clips}
    assert len(alone) == 1, alone
    named = {}
    for align in (4, 1):
        st = _open(nv, gpu_ctx, hdr, False)
        try:
            seg = Segmented(st, len(clips), 1024, align, _device_synth(torch)).run(clips)
            assert len(seg.tables) == 1
            named[align] = seg.kernels[0]
            if align == 1:
                assert (seg.tables[0][:-1, 1] % 4 != 0).any()
            for i, (ref, _) in enumerate(refs):
                assert same_bits(seg.clip_rows(i, ch, np.float32).reshape(-1), ref), (align, i)
        finally:
            st.close()
    assert named[4][1] in alone, (named, alone)
    if name.endswith(".ogg") and not any(os.environ.get(t) for t in ("NVH_NO_EMIT", "NVH_NO_SLAB", "NVH_FPW", "NVH_UNFUSED",
                                                                    "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_GPU_PARSE")):
        assert named[4][1] == "k_synth_group2", named


# (the selecting map {0, 2} needs the six channels)
FORMS = [(n, f) for n in ("stereo_res1_coupled", "six_ch_res2_4096") for f in ("s16", "planar", "mono", "map", "pipelined")
         if not (f == "map" and n == "stereo_res1_coupled")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", FORMS)
def test_forms(oracle, gpu_ctx, name, form):
    """One run per output form, device destination (the pipelined pair: page-locked host memory), batches of 13 frames, align 4:
    every clip equals the form's own rule (include/nvorbis_hip.h) applied to the oracle's PCM of that clip, gaps zero."""
    torch = _torch()
    import nvorbis_amd as nv
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name)
    refs, ch = oracle_clips(oracle, name, True)
    raw, _ = oracle_clips(oracle, name, False)
    rows = [r.reshape(-1, ch) for r, _ in refs]
    st = _open(nv, gpu_ctx, hdr, form == "pipelined")
    try:
        if form == "s16":
            want, dt, och, synth = [to_s16(r) for r in rows], np.int16, ch, _device_synth(torch, np.int16)
        elif form == "planar":
            want, dt, och, synth = rows, np.float32, ch, _device_synth(torch, planar=True)
        elif form == "mono":
            want = [mix_rule(r, ch, True).reshape(-1, 1) for r, _ in raw]
            dt, och, synth = np.float32, 1, _device_synth(torch, och=1, mix="mono")
        elif form == "map":
            want, dt, och = [np.ascontiguousarray(r[:, (0, 2)]) for r in rows], np.float32, 2
            synth = _device_synth(torch, och=2, channel_map=(0, 2))
        else:
            want, dt, och = rows, np.float32, ch
            flights = []

            def synth(st, table, n):  # begin this batch, end the one before: two flights overlap
                assert st.synth_begin() == n * ch
                flights.append((table, n))
                if len(flights) == 2:
                    t, m = flights.pop(0)
                    seg.route(t, st.synth_end().reshape(m, ch))
                return None
        seg = Segmented(st, len(clips), 13, 4, synth)
        seg.run(clips)
        if form == "pipelined":
            while flights:
                t, m = flights.pop(0)
                seg.route(t, st.synth_end().reshape(m, ch))
        for i, w in enumerate(want):
            assert same_bits(seg.clip_rows(i, och, dt), w), (name, form, i)
    finally:
        st.close()


@pytest.mark.gpu
def test_throwing_packet_is_replayed_with_its_boundaries(oracle, gpu_ctx):
    """GPU-parse mode, one clip in the middle of the batch holds packets the reference throws on (the IncompleteBook construction
    of test_pcm_s16.py): the batch is parsed again on the host WITH its boundaries and gaps.  The whole output -- every other
    clip's PCM, the gaps, the count -- and the positions of the errors equal the host-parser run's, and so does the segment table
    of the batch as finally parsed (synth_segments); the table read before the call is the look-ahead's and agrees up to the
    throwing clip."""
    torch = _torch()
    import nvorbis_amd as nv
    from nvorbis_amd import native
    from tests import synth_stream as ss
    cfg = ss.config("stereo_res1_coupled")
    old = cfg["books"][3]
    cfg["books"][3] = ss.IncompleteBook(old.bits, dims=old.dims, lookup=old.lookup, min_me=old.min_me, delta_me=old.delta_me,
                                        value_bits=old.value_bits, sequence_p=old.sequence_p, mults=old.mults)
    pk, _, _ = ss.make_stream(cfg, 200, 1)
    hdr = pk[:3]
    # which packets throw: the host parser says
    probe = nv.Stream(None, hdr[0], hdr[1], hdr[2])
    bad = []
    for i in range(3, len(pk)):
        try:
            probe.push_packet(pk[i], -1, 0)
        except native.NvhError:
            bad.append(i)
    probe.close()
    good = [i for i in range(3, len(pk)) if i not in bad]
    assert len(bad) > 0 and len(good) >= 20
    # five clips put together from packets that parse; the third has one that throws in its middle
    runs = [good[0:5], good[5:8], good[8:10] + [bad[len(bad) // 2]] + good[10:12], good[12:18], good[18:20]]
    res = {}
    for gpu_parse in (False, True):
        st = _open(nv, gpu_ctx, hdr, gpu_parse)
        host_errors = []
        for k, run in enumerate(runs):
            for i in run:
                try:
                    st.push_packet(pk[i], -1, PKT_EOS if (k % 2 and i == run[-1]) else 0)
                except native.NvhError as e:
                    host_errors.append((e.code, st.pending()[1]))
            st.next_segment(4096)  # (every block size is a multiple of 64: a large step, so that there are gaps)
        assert st.synth_segments().shape == (0, 3)  # nothing synthesised yet
        table = st.pending_segments()
        n = st.pending()[1]
        buf = torch.full((n * 2 + 64,), float(SENTINEL[np.dtype(np.float32)]), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        wr = st.synth_device(buf.data_ptr(), n * 2)
        final = st.synth_segments()
        errors = [(e.code, at // 2) for e, at in st.parse_errors] if gpu_parse else host_errors
        res[gpu_parse] = (table, final, wr, buf.cpu().numpy(), errors)
        st.close()
    (th, fh, wh, ph, eh), (tg, fg, wg, pg, eg) = res[False], res[True]
    assert len(eh) == 1 and eg == eh, (eh, eg)
    assert wg == wh and wh == th[-1, 2] * 2
    assert same_bits(pg[:wg], ph[:wh]) and (pg[wg:] == SENTINEL[np.dtype(np.float32)]).all()
    covered = np.zeros(wh // 2, bool)
    for _, b, e in th:
        covered[b:e] = True
    assert (~covered).any() and not ph[:wh].reshape(-1, 2)[~covered].any()  # there are gaps, and they are zeros in both runs
    # the table of the batch as it was finally parsed: the host-parser run's, whole; there it is the one read before the call
    assert np.array_equal(fg, th) and np.array_equal(fh, th), (th, fh, fg)
    assert np.array_equal(tg[:3, :2], th[:3, :2]) and np.array_equal(tg[:2], th[:2]), (th, tg)  # (the look-ahead's: up to the throwing clip)
    assert tg[2, 2] > th[2, 2]  # the look-ahead counted the packet that throws


_OGG_CLIPS = []


def _cut_ogg_clips(nv, oracle, ogg_bytes):
    """40 clips cut from 3test.ogg and 1test.ogg (two setups), each rewritten as an Ogg file of its own: (files, the oracle's
    decode of each)."""
    from tests import ogg_py
    if _OGG_CLIPS:
        return _OGG_CLIPS[0]
    rng = np.random.default_rng(5)
    files = []
    for k in range(40):
        name = ("3test", "1test")[k % 3 == 1]
        pk, _, _ = nv.demux_ogg(ogg_bytes[name])
        n = int(rng.choice([1, 2, 3, 5, 24]))
        first = int(rng.integers(3, len(pk) - n))
        run = list(pk[first:first + n])
        # granule positions as an encoder writes them: the samples the clip has delivered after each packet; every third clip
        # ends a few samples early (the end-of-stream trim)
        d = nv.Stream(None, pk[0], pk[1], pk[2])
        _, em, _, total = d.index_packets(nv.PacketArray.from_list(pk[:3] + run))
        d.close()
        gran = [0, 0, 0] + [int(v) for v in em]
        if k % 3 == 0 and n > 1 and gran[-1] > 8:
            gran[-1] -= int(rng.integers(1, 6))
        files.append(ogg_py.write_ogg(pk[:3] + run, gran, serial=0x1000 + k))
    _OGG_CLIPS.append((files, [oracle.decode_ogg(f) for f in files]))
    return _OGG_CLIPS[0]


@pytest.mark.gpu
@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_decode_clips(oracle, gpu_ctx, ogg_bytes, fmt, layout, device_out):
    """40 clips of two setups, as Ogg files: every result is the oracle's decode of that file (converted / laid out by the form's
    rule), in input order."""
    _torch()
    import nvorbis_amd as nv
    files, refs = _cut_ogg_clips(nv, oracle, ogg_bytes)
    assert len({r.size for r, _ in refs}) > 5 and len({f[:200] for f in files}) > 1
    for bf in (64, 4096):
        got = nv.decode_clips(files, ctx=gpu_ctx, batch_frames=bf, sample_format=fmt, layout=layout, device_out=device_out)
        assert len(got) == len(files)
        for i, ((ref, info), g) in enumerate(zip(refs, got)):
            if device_out:
                g = g.cpu().numpy()
            want = to_s16(ref) if fmt == "s16" else ref
            if layout == "planar":
                want = np.ascontiguousarray(want.reshape(-1, info["channels"]).T)
            assert same_bits(np.ascontiguousarray(g), want), (fmt, layout, device_out, bf, i, g.shape, want.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["mono", "map", "planar_map_s16"])
def test_decode_clips_mix_and_map(oracle, gpu_ctx, ogg_bytes, form):
    """The stereo clips of the same 40 with the mono mix and with a channel map (a swap), host results: the form's rule
    (include/nvorbis_hip.h) applied to the oracle's decode of each file."""
    _torch()
    import nvorbis_amd as nv
    files, refs = _cut_ogg_clips(nv, oracle, ogg_bytes)
    stereo = [i for i, (_, info) in enumerate(refs) if info["channels"] == 2]  # (1test.ogg is mono: a swap is no map of it)
    assert len(stereo) > 20
    files, refs = [files[i] for i in stereo], [refs[i] for i in stereo]
    kw = {"mono": dict(mix="mono"), "map": dict(channel_map=(1, 0)),
          "planar_map_s16": dict(channel_map=(1, 0), layout="planar", sample_format="s16")}[form]
    got = nv.decode_clips(files, ctx=gpu_ctx, batch_frames=64, **kw)
    for i, (f, (ref, info), g) in enumerate(zip(files, refs, got)):
        ch = info["channels"]
        assert ch == 2
        if form == "mono":
            raw, _ = oracle.decode_ogg(f, clip=False)
            want = mix_rule(raw, ch, True)
        else:
            want = np.ascontiguousarray(ref.reshape(-1, ch)[:, (1, 0)])
            want = np.ascontiguousarray(to_s16(want).T) if form == "planar_map_s16" else want.reshape(-1)
        assert same_bits(np.ascontiguousarray(g), want), (form, i, g.shape, want.shape)


@pytest.mark.gpu
def test_core_parity_under_the_toggles():
    """The core parity test once more in child processes under the kernel-variant toggles (three children at a time).  With
    poisoned planes a frame that read a plane of the segment before it -- which nothing of its own segment wrote -- shows as NaN."""
    if os.environ.get("NVH_TEST_CHILD"):
        return  # inside a replay
    from tests.replay import run_children
    children = []
    for toggle in ["NVH_FPW=1", "NVH_FPW=4", "NVH_NO_EMIT", "NVH_NO_SLAB", "NVH_POISON_PLANES+NVH_GPU_PARSE"]:
        env = dict(os.environ)
        for t in toggle.split("+"):
            key, _, val = t.partition("=")
            env[key] = val or "1"
        env["NVH_TEST_CHILD"] = "1"
        children.append((["test_clip_batches.py"], env, ["-k", "test_core_parity and not toggles"]))
    for k in range(0, len(children), 3):
        run_children(children[k:k + 3], timeout=900)

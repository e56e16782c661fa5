"""Windowed segments: crop and pad a clip into a fixed-length row (nvh_stream_segment_window, Stream.segment_window,
nv.decode_clip_rows; include/nvorbis_hip.h states the rule).

A windowed segment emits the samples [skip, skip + take) of what a fresh stream over the same packets emits, and -- with a pitch --
is padded with zeros so that the next segment begins `pitch` samples behind it.  The reference of the segment tests is the oracle
run on the clip alone, sliced; of decode_clip_rows, oracle.decode_ogg of the whole file, sliced.  No tolerance anywhere: floats
are compared as uint32, gaps and pads byte-wise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_clip_batches import (CLIP, GOLDEN, PKT_EOS, ROOT, SENTINEL, SHAPES, _device_synth, _open, _torch, make_clips, mix_rule,
                                     oracle_clips, same_bits, stream_packets, to_s16)

FILES = ("1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg")
STREAMS = ["3test.ogg", "1test.ogg"]
# 1test.ogg has 25 audio packets: the same shapes, cut from its beginning, the long runs 20 packets
SHAPES_SHORT = [({40: 5, 41: 6, 43: 7, 60: 4, 0: 0}[f], min(n, 20), e) for f, n, e in SHAPES]


def shapes_of(name):
    return tuple(SHAPES_SHORT if name == "1test.ogg" else SHAPES)


FIXED_WINDOWS = [(0, -1), (0, 0), (1, 1), (4, 1024), (129, 777)]


def cut(rows, skip, take):
    """Samples [skip, skip + take) of `rows` ([T, ...]); take = -1: to the end."""
    return rows[skip:] if take < 0 else rows[skip:skip + take]


def emitted_len(t0, skip, take):
    return max(0, t0 - skip) if take < 0 else min(take, max(0, t0 - skip))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: host-only streams
# ---------------------------------------------------------------------------------------------------------------------------

def test_window_entry_point_is_exported_and_declared():
    import nvorbis_amd as nv
    from nvorbis_amd import native
    name = "nvh_stream_segment_window"
    assert hasattr(native.lib(), name) and name in native.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "nvorbis_hip.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "NativeMethods.cs")).read()
    assert re.search(r"\bint %s\s*\(" % name, hdr)
    assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern (?:unsafe )?int %s\(" % name, cs)
    assert callable(nv.decode_clip_rows) and callable(nv.Stream.segment_window)


def test_window_refuses_bad_arguments(oracle):
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    assert L.nvh_stream_segment_window(None, 0, -1, 0) == native.ERR_ARGUMENT
    pk = stream_packets(oracle, "3test.ogg")
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for bad in ((-1, -1, 0), (0, -2, 0), (0, -1, -1), (0, -1, 8), (0, 9, 8), (-5, 4, 8)):
            assert L.nvh_stream_segment_window(st._h, *bad) == native.ERR_ARGUMENT, bad
            with pytest.raises(native.NvhError):
                st.segment_window(*bad)
        for ok in ((0, -1, 0), (7, 0, 0), (0, 8, 8), (3, 5, 8), (1 << 40, 1 << 40, 0)):
            st.segment_window(*ok)  # a second call before the first packet replaces the first
        st.segment_window(4, 100, 0)
        st.push_packet(pk[40], -1, 0)
        assert L.nvh_stream_segment_window(st._h, 0, -1, 0) == native.ERR_ARGUMENT  # the segment has seen a packet
        st.next_segment(1)
        st.segment_window(0, 4, 4)  # legal again behind a boundary
        st.push_end()
        assert L.nvh_stream_segment_window(st._h, 0, -1, 0) == native.ERR_ARGUMENT  # ... and not after push_end
        st.reset()
        st.segment_window(0, 4, 4)  # ... and after a reset
        st.next_segment(1)
        assert np.array_equal(st.pending_segments(), [[0, 0, 0], [1, 4, 4]])  # an empty segment with a pitch: a row
    finally:
        st.close()


def _push_all(st, clip, window=None, drop_before_end=False):
    run, g, f = clip
    if window is not None:
        st.segment_window(window[0], window[1], 0)
    for p, gr, fl in zip(run, g, f):
        st.push_packet(p, gr, fl)
    if drop_before_end:
        st.drop_pending()
    st.push_end()
    return st.pending_geometry().copy(), st.pending()[1]


@pytest.mark.parametrize("name", STREAMS)
def test_windowed_geometry_is_the_twins_intersected(oracle, name):
    """A windowed stream next to an un-windowed twin, every clip of SHAPES: the windowed geometry is a prefix of the twin's, the
    emit fields are the twin's intersected with the window, every other field is equal.  Also with the batch dropped before the
    end, so that the carried-tail pseudo-frame is the frame that is cut."""
    import nvorbis_amd as nv
    hdr = stream_packets(oracle, name)[:3]
    seen = set()
    for clip, (_, npk, ending) in zip(make_clips(oracle, name, shapes_of(name)), shapes_of(name)):
        tw = nv.Stream(None, hdr[0], hdr[1], hdr[2])
        try:
            geo_t, t0 = _push_all(tw, clip)
        finally:
            tw.close()
        if npk == 0:
            geo_t = geo_t[:0]
        cnt = geo_t[:, 5].astype(np.int64)
        raw = np.concatenate([[0], np.cumsum(cnt)])  # frame i emits the stream's samples [raw[i], raw[i + 1])
        assert raw[-1] == t0
        windows = list(FIXED_WINDOWS) + [(t0 + 5, 10), (max(t0 - 3, 0), 100)]
        emitting = [i for i in range(1, len(cnt)) if cnt[i] > 8]
        if emitting:
            i = emitting[len(emitting) // 2]
            windows += [(int(raw[i]), 100), (int(raw[i]) + 3, 5)]
        if npk and t0 > 4:
            windows.append((1, t0 - 3))  # ends inside the last frame: its drained tail, or what an end-of-stream trim left of it
        for skip, take in windows:
            hi_w = t0 if take < 0 else min(skip + take, t0)
            for drop in (False, True):
                ws = nv.Stream(None, hdr[0], hdr[1], hdr[2])
                try:
                    geo_w, n = _push_all(ws, clip, (skip, take), drop)
                    pos_w, em_w, _ = ws.position()
                finally:
                    ws.close()
                assert n == emitted_len(t0, skip, take) or drop, (name, clip[1:], skip, take, n, t0)
                assert em_w == emitted_len(t0, skip, take)
                if drop:
                    # only the drained carried tail is pending: the twin's last frame's tail, cut
                    if npk == 0 or geo_t[-1, 5] == 0:
                        continue
                    last = len(cnt) - 1
                    own = int(geo_t[last, 2] - geo_t[last, 4]) if ending == "none" else int(cnt[last])
                    lo, hi = max(skip, int(raw[last]) + own), min(hi_w, int(raw[last + 1]))
                    if ending != "none" or hi <= lo:
                        assert geo_w.shape[0] == 0 or geo_w[:, 5].sum() == 0, (name, skip, take, geo_w)
                    else:
                        assert geo_w.shape[0] == 1 and geo_w[0, 0] == 0 and geo_w[0, 6] == -2, geo_w
                        assert geo_w[0, 4] == 0 and geo_w[0, 5] == geo_w[0, 7] == hi - lo, (geo_w, lo, hi)
                        seen.add("carried tail cut")
                    continue
                m = geo_w.shape[0] if npk else 0
                assert m <= len(cnt)
                other = [0, 1, 2, 3, 6, 7]
                assert np.array_equal(geo_w[:m][:, other], geo_t[:m][:, other]), (name, skip, take)
                for i in range(len(cnt)):
                    lo, hi = max(skip, int(raw[i])), min(hi_w, int(raw[i + 1]))
                    if i >= m:
                        assert hi <= lo, (name, skip, take, i, m)  # a frame the full window kept out emits nothing in it
                        continue
                    if hi > lo:
                        assert geo_w[i, 5] == hi - lo and geo_w[i, 4] == geo_t[i, 4] + (lo - raw[i]), (name, skip, take, i, geo_w[i], geo_t[i])
                    else:
                        assert geo_w[i, 5] == 0, (name, skip, take, i, geo_w[i])
                if m < len(cnt):
                    seen.add("full window dropped packets")
                if skip >= t0:
                    seen.add("skip beyond the end")
                elif take >= 0 and skip + take > t0:
                    seen.add("take beyond the end")
                if skip > 0 and skip in raw[1:-1]:
                    seen.add("skip on an emit boundary")
                if take > 0 and any(raw[i] < skip and skip + take < raw[i + 1] for i in range(len(cnt))):
                    seen.add("inside one frame")
                if len(cnt) and take >= 0 and skip + take < t0:
                    last = len(cnt) - 1
                    if ending == "none" and skip + take > raw[last] + (geo_t[last, 2] - geo_t[last, 4]):
                        seen.add("ends inside a drained tail")
                    if isinstance(ending, int) and skip + take > raw[last]:
                        seen.add("ends inside an end-of-stream trim")
    assert seen >= {"full window dropped packets", "skip beyond the end", "take beyond the end", "skip on an emit boundary",
                    "inside one frame", "ends inside a drained tail", "ends inside an end-of-stream trim", "carried tail cut"}, seen


def row_windows(refs, ch, pitch):
    """One window per clip of SHAPES (skip, take <= pitch), the fixed ones first."""
    fixed = [(0, pitch), (0, 0), (1, 1), (4, 1024), (129, 777), (64, pitch), (5, 2000), (3000, 100)]
    out = []
    for i, (r, _) in enumerate(refs):
        t0 = r.size // ch
        skip, take = fixed[i] if i < len(fixed) else (((i * 37) % 200) * (4 if i % 2 else 1), pitch - (i % 3))
        if i == 9:
            skip = t0 + 3  # a skip beyond the end: a row of zeros
        out.append((skip, min(take, pitch), pitch))
    return out


class Rows:
    """One stream fed clips as WINDOWED segments; batches flushed at `bf` pending frames as tests.test_clip_batches.Segmented
    flushes them.  Collects every batch's rows (gaps and pads included) and its table, shifted to the position in the
    concatenation of all batch outputs."""

    def __init__(self, st, bf, align, synth):
        self.st, self.bf, self.align, self.synth = st, bf, align, synth
        self.out, self.tables, self.kernels, self.base, self.geos = [], [], [], 0, []

    def flush(self):
        st = self.st
        frames, n = st.pending()
        if not n and not frames:
            return
        table = st.pending_segments().copy()
        assert table[-1, 2] == n and (table[:, 1] <= table[:, 2]).all() and (table[1:, 1] >= table[:-1, 2]).all(), table
        self.geos.append(st.pending_geometry().copy() if frames else np.zeros((0, 8), np.int32))
        rows = self.synth(st, table, n)
        if st._ctx is not None:
            self.kernels.append(st.kernels())
            final = st.synth_segments()
            if final.shape[0]:
                table = final.copy()
        if rows is not None:
            self.out.append(rows)
            n = rows.shape[0]
        table[:, 1:] += self.base
        self.tables.append(table)
        self.base += n

    def run(self, clips, windows):
        st = self.st
        for i, ((run, g, f), w) in enumerate(zip(clips, windows)):
            st.segment_window(*w)
            for p, gr, fl in zip(run, g, f):
                if st.pending()[0] >= self.bf:
                    self.flush()
                st.push_packet(p, gr, fl)
                if i % 2 == 1 and st.pending()[0] >= self.bf:
                    self.flush()
            st.next_segment(self.align)
        self.flush()
        return self

    def ranges(self, k):
        """Segment k's ranges over all batches, in the concatenated output."""
        return [(int(b), int(e)) for t in self.tables for s, b, e in t if s == k and e > b]

    def check(self, wants, windows, och, dt):
        """Rows lie where pitch and align put them, hold `wants`, and everything outside the ranges is zero bytes."""
        out = np.concatenate(self.out) if self.out else np.zeros((0, och), dt)
        covered = np.zeros(out.shape[0], bool)
        cur = 0
        for k, (want, (skip, take, pitch)) in enumerate(zip(wants, windows)):
            rs = self.ranges(k)
            assert sum(e - b for b, e in rs) == want.shape[0], (k, rs, want.shape)
            at = cur
            for b, e in rs:
                assert b == at, (k, rs, cur)  # contiguous from the row's start, across batches
                at = e
            got = out[cur:cur + want.shape[0]]
            assert same_bits(got, want), (k, skip, take, got.shape)
            covered[cur:cur + want.shape[0]] = True
            cur += max(want.shape[0], pitch)
            cur = (cur + self.align - 1) & ~(self.align - 1)
        assert out.shape[0] == cur == self.base, (out.shape, cur, self.base)
        assert not out[~covered].view(np.uint8).any(), "a pad or a gap holds something other than zeros"
        return out


def crossed(tables):
    """A row was open across a batch boundary with samples in the earlier batch: its pad has to count from the row's start."""
    return any(t[0, 0] == p[-1, 0] and p[-1, 2] > p[-1, 1] and len(t) > 1 for p, t in zip(tables, tables[1:]))


def _drop(st, table, n):
    st.drop_pending()
    return None


def test_pitch_and_tables(oracle):
    """Rows begin `pitch` apart, the batch outputs add up to rows x pitch, every range has the emitted length and no pad lies in
    one.  Batches of 13 frames: a row crosses a batch boundary and its pad counts from the row's start."""
    import nvorbis_amd as nv
    name, pitch = "3test.ogg", 2048
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name)
    refs, ch = oracle_clips(oracle, name)
    wins = row_windows(refs, ch, pitch)
    lens = [emitted_len(r.size // ch, s, t) for (r, _), (s, t, _) in zip(refs, wins)]
    assert 0 in lens and pitch in lens and any(0 < v < pitch for v in lens)
    for bf in (13, 1 << 20):
        st = nv.Stream(None, hdr[0], hdr[1], hdr[2])
        try:
            rows = Rows(st, bf, 4, _drop).run(clips, wins)
            assert rows.base == len(clips) * pitch
            for k, want in enumerate(lens):
                rs = rows.ranges(k)
                assert sum(e - b for b, e in rs) == want, (k, rs, want)
                assert all(k * pitch <= b and e <= k * pitch + want for b, e in rs), (k, rs)
                assert not rs or rs[0][0] == k * pitch
            if bf == 13:
                assert len(rows.tables) > 2 and crossed(rows.tables), "no row crossed a batch boundary"
            else:
                assert len(rows.tables) == 1 and rows.tables[0][-1, 1] == len(clips) * pitch
        finally:
            st.close()


def test_a_full_window_takes_no_more_packets(oracle):
    """push_packets stops behind the packet that fills the window; `position` counts un-windowed stream time, `emitted` the window."""
    import nvorbis_amd as nv
    pk = stream_packets(oracle, "3test.ogg")
    pa = nv.PacketArray.from_list(pk)

    def twin(count):
        t = nv.Stream(None, pk[0], pk[1], pk[2])
        try:
            assert t.push_packets(pa, 40, count) == count
            return t.position()
        finally:
            t.close()
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        st.segment_window(129, 777, 0)
        took = st.push_packets(pa, 40, 30)
        assert 1 < took < 30
        assert st.push_packets(pa, 40 + took, 30) == 0  # *consumed excludes the packets behind a full window
        frames = st.pending()[0]
        st.push_packet(pk[40 + took], -1, 0)  # NVH_OK, not parsed
        assert st.pending() == (frames, 777)
        pos, em, eos = st.position()
        assert em == 777 and not eos
        assert (pos, pos) == twin(took)[:2] and pos >= 129 + 777  # un-windowed stream time
        assert twin(took - 1)[1] < 129 + 777  # the packet that filled the window was needed
        st.next_segment(1)  # the drain at the boundary emits nothing
        assert np.array_equal(st.pending_segments(), [[0, 0, 777], [1, 777, 777]])
    finally:
        st.close()


_INDEX = {}


def file_index(nv, name):
    if name not in _INDEX:
        pa = nv.demux_ogg_array(open(os.path.join(GOLDEN, name), "rb").read(), 0)
        st = nv.Stream(None, pa[0], pa[1], pa[2])
        try:
            _INDEX[name] = (pa,) + tuple(st.index_packets(pa, 3))
        finally:
            st.close()
    return _INDEX[name]


def file_windows(total, seed):
    """Eight (start, length is the caller's) starts per file: 0, 4, 1001, the middle, the last 3000 samples, beyond the end, two
    seeded ones (one a multiple of 4)."""
    rng = np.random.default_rng(seed)
    return [0, 4, 1001, (total // 2) & ~3, total - 3000, total + 7, int(rng.integers(0, total // 4)) * 4, int(rng.integers(0, total)) | 1]


@pytest.mark.parametrize("name", FILES)
def test_planner_runs_emit_the_row(name):
    """plan_clip_window + push_clip_window on a host-only stream: the pushed run's geometry emits exactly
    min(length, max(0, total - start)), for the fixed starts and 50 seeded random windows."""
    import nvorbis_amd as nv
    from nvorbis_amd.clips import plan_clip_window, push_clip_window
    pa, pos, em, state, total = file_index(nv, name)
    rng = np.random.default_rng(FILES.index(name))
    cases = [(s, n) for s in file_windows(total, 3) for n in (4096, 4095)]
    cases += [(int(rng.integers(0, total + 2000)), int(rng.integers(0, 9000))) for _ in range(50)]
    for start, length in cases:
        plan = plan_clip_window(pos, em, state, total, start, length)
        want = min(length, max(0, total - start))
        assert plan["valid"] == want
        st = nv.Stream(None, pa[0], pa[1], pa[2])
        try:
            push_clip_window(st, pa, plan, length)
            st.next_segment(1)
            table, geo = st.pending_segments(), st.pending_geometry()
            assert table[0, 2] - table[0, 1] == want and table[1, 1] == length, (name, start, length, plan, table)
            assert (geo[:, 5].sum() if st.pending()[0] else 0) == want
            assert st.pending()[0] <= 12 + length // 64, (name, start, length, st.pending())  # only the packets the row needs
        finally:
            st.close()


@pytest.mark.parametrize("name", ["1test.ogg", "2test.ogg", "3test.ogg"])
def test_the_end_of_stream_trim_needs_the_position_state(name):
    """The last 3000 samples of a file, from the planned lead-in to the end: with the serial decoder's position state the run
    emits what the serial decoder emits there; without it the end-of-stream trim is computed from a wrong position."""
    import nvorbis_amd as nv
    from nvorbis_amd.clips import plan_clip_window
    pa, pos, em, state, total = file_index(nv, name)
    plan = plan_clip_window(pos, em, state, total, total - 3000, 3000)
    counts = {}
    for with_state in (True, False):
        st = nv.Stream(None, pa[0], pa[1], pa[2])
        try:
            st.push_packet(pa[3 + plan["lead"]], -1, 0)
            if with_state:
                st.set_position_state(plan["has_position"], plan["position"])
            st.push_packets(pa, 3 + plan["first"], len(pa))
            st.push_end()
            counts[with_state] = st.pending()[1]
        finally:
            st.close()
    assert counts[True] == total - em[plan["lead"]] == 3000 + plan["skip"], (counts, plan)
    assert counts == {True: {"1test.ogg": 3558, "2test.ogg": 3918, "3test.ogg": 3102}[name], False: 4096}, counts


def test_decode_clip_rows_checks_its_arguments_before_a_device(ogg_bytes):
    import nvorbis_amd as nv
    good = ogg_bytes["3test"]
    for kw in ({"sample_format": "s24"}, {"layout": "tiled"}, {"mix": "stereo"}, {"mix": "mono", "layout": "planar"},
               {"channel_map": (0, 0)}, {"batch_frames": 0}, {"starts": [0, 1]}, {"starts": [-1]}, {"starts": [1.5]}):
        with pytest.raises(ValueError):
            nv.decode_clip_rows([good], 16, **kw)
    for bad in (-1, 2.0, None):
        with pytest.raises(ValueError):
            nv.decode_clip_rows([good], bad)
    with pytest.raises(ValueError):
        nv.decode_clip_rows([good, ogg_bytes["1test"]], 16)  # stereo and mono
    from nvorbis_amd import native
    with pytest.raises(native.NvhError) as e:
        nv.decode_clip_rows([good, b"not an ogg file at all, and long enough to be looked at" * 4], 16)
    assert "clip 1" in str(e.value) and e.value.clip == 1
    rows, valid = nv.decode_clip_rows([good, good], 0)  # no samples asked for: no device needed
    assert rows.shape == (2, 0, 2) and np.array_equal(valid, [0, 0]) and valid.dtype == np.int64


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

def form_case(torch, form, refs, raw, ch):
    """(per-clip reference rows [T, och] in the form's rule, dtype, och, synth) of an output form."""
    rows = [r.reshape(-1, ch) for r, _ in refs]
    if form == "f32":
        return rows, np.float32, ch, _device_synth(torch)
    if form == "s16":
        return [to_s16(r) for r in rows], np.int16, ch, _device_synth(torch, np.int16)
    if form == "planar":
        return rows, np.float32, ch, _device_synth(torch, planar=True)
    if form == "mono":
        return [mix_rule(r, ch, True).reshape(-1, 1) for r, _ in raw], np.float32, 1, _device_synth(torch, och=1, mix="mono")
    assert form == "swap" and ch == 2
    return [np.ascontiguousarray(r[:, (1, 0)]) for r in rows], np.float32, 2, _device_synth(torch, och=2, channel_map=(1, 0))


def forms_of(ch):
    return ("f32", "s16", "planar", "mono") + (("swap",) if ch == 2 else ())


def slice_clips(raw, ch, wins, form):
    """HasClipped of the emitted samples, from the oracle's unclipped PCM."""
    for (r, _), (skip, take, _) in zip(raw, wins):
        x = r.reshape(-1, ch)
        x = mix_rule(x, ch, False).reshape(-1, 1) if form == "mono" and ch > 1 else x
        x = cut(x, skip, take)
        if ((x > CLIP) | (x < -CLIP)).any():
            return True
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
@pytest.mark.parametrize("name", STREAMS)
def test_core_parity(oracle, gpu_ctx, name, gpu_parse):
    """16 windowed segments, batches of 13 frames, both parsers, every output form: rows equal the oracle's slices, pads and align
    gaps are zero, a sentinel behind the output is untouched (_device_synth), HasClipped is the unclipped slices'."""
    torch = _torch()
    import nvorbis_amd as nv
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name, shapes_of(name))
    refs, ch = oracle_clips(oracle, name, True, shapes_of(name))
    raw, _ = oracle_clips(oracle, name, False, shapes_of(name))
    for form in forms_of(ch):
        for pitch, align in ((2048, 4),) + (((2047, 1),) if form == "f32" else ()):
            wins = row_windows(refs, ch, pitch)
            full, dt, och, synth = form_case(torch, form, refs, raw, ch)
            wants = [cut(r, s, t) for r, (s, t, _) in zip(full, wins)]
            st = _open(nv, gpu_ctx, hdr, gpu_parse)
            try:
                rows = Rows(st, 13, align, synth).run(clips, wins)
                rows.check(wants, wins, och, dt)
                assert crossed(rows.tables)  # a row across a batch boundary
                assert st.has_clipped() == slice_clips(raw, ch, wins, form), (name, form)
            finally:
                st.close()


_FILE_REFS = {}


def host_item(rows, device_out):
    return rows.element_size() if device_out else rows.dtype.itemsize


def file_ref(oracle, ogg_bytes, name, clip=True):
    key = (name, clip)
    if key not in _FILE_REFS:
        pcm, info = oracle.decode_ogg(ogg_bytes[name[:-4]], clip=clip)
        pcm = pcm.reshape(-1, info["channels"])
        pcm.setflags(write=False)
        _FILE_REFS[key] = pcm
    return _FILE_REFS[key]


def want_rows(oracle, ogg_bytes, names, starts, length, layout, mix, fmt):
    out, valid = [], []
    for name, start in zip(names, starts):
        ref = file_ref(oracle, ogg_bytes, name, mix is None)
        ch = ref.shape[1]
        x = mix_rule(ref, ch, True).reshape(-1, 1) if mix else ref
        x = x[start:start + length]
        valid.append(x.shape[0])
        row = np.zeros((length, x.shape[1]), np.float32)
        row[:x.shape[0]] = x
        out.append(to_s16(row) if fmt == "s16" else row)
    rows = np.stack(out)
    if mix:
        rows = rows[:, :, 0]
    elif layout == "planar":
        rows = rows.transpose(0, 2, 1)
    return rows, np.asarray(valid, np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("form", ["interleaved", "planar", "mono", "planar_s16", "interleaved_s16"])
def test_decode_clip_rows(oracle, gpu_ctx, ogg_bytes, monkeypatch, form, device_out):
    """Eight windows of each file, length 4096 and 4095.  The four files as one call (four setups) under the mono mix; in the other
    forms the two stereo files and the two mono files as a call each (two setups; files whose channel counts differ cannot share
    a tensor); and 3test.ogg alone: one group, the kernels write the returned buffer.  Rows equal oracle.decode_ogg sliced."""
    _torch()
    import nvorbis_amd as nv
    from nvorbis_amd import clips as clips_mod
    layout = "planar" if form.startswith("planar") else "interleaved"
    mix = "mono" if form == "mono" else None
    fmt = "s16" if form.endswith("s16") else "f32"
    bases = []  # the destination of every batch: the pointer handed to nvh_stream_synth_out
    flush = clips_mod._RowGroup.flush

    def spy(self):
        flush(self)
        bases[:] = self.dests
    monkeypatch.setattr(clips_mod._RowGroup, "flush", spy)
    sets = ([list(FILES)] if mix else [["3test.ogg", "issue6test.ogg"], ["1test.ogg", "2test.ogg"]]) + [["3test.ogg"]]
    for names in sets:
        files, starts = [], []
        for k in range(8):  # interleave the files, so that the gather has work to do
            for n in names:
                files.append(ogg_bytes[n[:-4]])
                starts.append(file_windows(file_index(nv, n)[4], 3)[k])
        nm = [n for _ in range(8) for n in names]
        assert any(s % 4 for s in starts) and any(s % 4 == 0 and s for s in starts)
        for length in (4096, 4095):
            del bases[:]
            rows, valid = nv.decode_clip_rows(files, length, starts, ctx=gpu_ctx, batch_frames=16, sample_format=fmt, layout=layout,
                                              mix=mix, device_out=device_out)
            want, want_valid = want_rows(oracle, ogg_bytes, nm, starts, length, layout, mix, fmt)
            assert np.array_equal(valid, want_valid) and valid.dtype == np.int64
            assert (valid == 0).any() and (valid == length).any() and ((valid > 0) & (valid < length)).any()
            if len(names) == 1:  # one group: the returned storage is the buffer every batch wrote into
                dense = rows.permute(1, 0, 2) if layout == "planar" and device_out else rows.transpose(1, 0, 2) if layout == "planar" else rows
                ptr = dense.data_ptr() if device_out else dense.ctypes.data
                # (batches end on row boundaries: every batch begins at the base plus whole rows, behind the batch before it)
                row_bytes = length * host_item(rows, device_out) * (1 if layout == "planar" else int(np.prod(dense.shape[2:])))
                assert len(bases) > 1 and bases[0] == ptr and all(b > a for a, b in zip(bases, bases[1:])), (bases, ptr)
                assert all((b - ptr) % row_bytes == 0 and (b - ptr) // row_bytes < 8 for b in bases), (bases, ptr, row_bytes)
                assert dense.is_contiguous() if device_out else dense.flags["C_CONTIGUOUS"]
            host = rows.cpu().numpy() if device_out else rows
            assert tuple(host.shape) == want.shape, (host.shape, want.shape)
            assert same_bits(np.ascontiguousarray(host), np.ascontiguousarray(want)), (form, device_out, names, length)


ROUTE_SHAPES = tuple((4 + 25 * k, 40, "none") for k in range(12))


@pytest.mark.gpu
def test_routing_keeps_paired_emission(oracle, gpu_ctx):
    """Rows of 40 packets from the stretch of 3test.ogg the clip-batch routing test uses, starts and lengths multiples of 4: at
    least 7/8 of the decoded frames are untrimmed and fully emitting, and the batch runs the emitting family.  Shifted by one
    sample the rows are still bit-exact (whatever ran)."""
    torch = _torch()
    import nvorbis_amd as nv
    name = "3test.ogg"
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name, ROUTE_SHAPES)
    refs, ch = oracle_clips(oracle, name, True, ROUTE_SHAPES)
    pitch = 40960  # (no clip is longer: a row is its clip from `skip` on, 40 frames of which three are not whole)
    for shift in (0, 1):
        wins = [(256 + 4 * k + shift, pitch, pitch) for k in range(len(clips))]
        wants = [cut(r.reshape(-1, ch), s, t) for (r, _), (s, t, _) in zip(refs, wins)]
        assert all(19000 < w.shape[0] <= pitch for w in wants)
        st = _open(nv, gpu_ctx, hdr, False)
        try:
            rows = Rows(st, 1 << 20, 4, _device_synth(torch)).run(clips, wins)
            rows.check(wants, wins, ch, np.float32)
            assert len(rows.geos) == 1
            geo = rows.geos[0]
            decoded = geo[geo[:, 0] != 0]
            whole = (decoded[:, 4] == decoded[:, 1]) & (decoded[:, 5] == decoded[:, 2] - decoded[:, 1]) & (decoded[:, 5] > 0)
            if shift == 0:
                assert whole.sum() * 8 >= decoded.shape[0] * 7, (whole.sum(), decoded.shape[0])
                if not any(os.environ.get(t) for t in ("NVH_NO_EMIT", "NVH_NO_SLAB", "NVH_FPW", "NVH_UNFUSED", "NVH_NO_FUSED_IMDCT",
                                                       "NVH_NO_COMPACT", "NVH_GPU_PARSE")):
                    assert rows.kernels[0][1] == "k_synth_group2", rows.kernels
        finally:
            st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAMS)
def test_a_long_pad_goes_through_the_row_fill(oracle, gpu_ctx, name):
    """One row of 1000 real samples with a pitch of 262144 among ordinary rows, every output form: the batch names k_zero_rows,
    the pad is zeros, the sentinel behind the output untouched.  A batch without windows names what it names without the feature."""
    torch = _torch()
    import nvorbis_amd as nv
    hdr = stream_packets(oracle, name)[:3]
    shapes = shapes_of(name)[:8]
    clips = make_clips(oracle, name, shapes)
    refs, ch = oracle_clips(oracle, name, True, shapes)
    raw, _ = oracle_clips(oracle, name, False, shapes)
    wins = [(4 * k, 1024, 1024) for k in range(len(clips))]
    wins[5] = (8, 1000, 262144)  # (clip 5: 24 packets)
    for form in forms_of(ch):
        full, dt, och, synth = form_case(torch, form, refs, raw, ch)
        wants = [cut(r, s, t) for r, (s, t, _) in zip(full, wins)]
        assert wants[5].shape[0] == 1000
        st = _open(nv, gpu_ctx, hdr, False)
        try:
            rows = Rows(st, 1 << 20, 4, synth).run(clips, wins)
            rows.check(wants, wins, och, dt)
            assert len(rows.kernels) == 1 and "k_zero_rows" in rows.kernels[0][3], rows.kernels
        finally:
            st.close()
    st = _open(nv, gpu_ctx, hdr, False)
    try:
        plain = Rows(st, 1 << 20, 4, _device_synth(torch)).run(clips, [(0, -1, 0)] * len(clips))
        assert len(plain.kernels) == 1 and "k_zero_rows" not in ",".join(plain.kernels[0]), plain.kernels
        assert re.fullmatch(r"-|k_ola_compact\w*|k_ola_emit\w*", plain.kernels[0][3]), plain.kernels
    finally:
        st.close()


@pytest.mark.gpu
def test_a_batch_of_pads_alone(oracle, gpu_ctx, ogg_bytes):
    """Segments that emit nothing, with a pitch, and no frame in the batch: the synthesis call writes the rows of zeros (short pads
    by k_zero_gaps, the long one by k_zero_rows, which is named), nothing behind them, in every output form; and decode_clip_rows
    with every start beyond the end returns zeros, also where only the LAST rows are empty."""
    torch = _torch()
    import nvorbis_amd as nv
    name = "3test.ogg"
    hdr = stream_packets(oracle, name)[:3]
    empty = [([], [], [])] * 3
    wins = [(0, 0, 1024), (5, 7, 262144), (0, 0, 8)]
    raw = refs = [(np.zeros(0, np.float32), False)] * 3
    for form in forms_of(2):
        _, dt, och, synth = form_case(torch, form, refs, raw, 2)
        st = _open(nv, gpu_ctx, hdr, form == "planar")
        try:
            rows = Rows(st, 13, 4, synth).run(empty, wins)
            out = rows.check([np.zeros((0, och), dt)] * 3, wins, och, dt)
            assert out.shape[0] == 1024 + 262144 + 8 and len(rows.kernels) == 1
            assert rows.kernels[0] == ["-", "-", "-", "k_zero_rows"], rows.kernels
            assert not st.has_clipped()
        finally:
            st.close()
    data = ogg_bytes["3test"]
    total = file_index(nv, name)[4]
    for starts in ([total, total + 1, total + 4096], [0, 4, total + 9, total]):
        for device_out in (False, True):
            got, valid = nv.decode_clip_rows([data] * len(starts), 4096, starts, ctx=gpu_ctx, batch_frames=4, device_out=device_out)
            want, want_valid = want_rows(oracle, ogg_bytes, [name] * len(starts), starts, 4096, "interleaved", None, "f32")
            assert np.array_equal(valid, want_valid)
            assert same_bits(got.cpu().numpy() if device_out else got, want), (starts, device_out)


@pytest.mark.gpu
def test_a_throwing_packet_is_replayed_with_its_windows(oracle, gpu_ctx):
    """GPU-parse mode, a windowed batch in which one clip holds a packet the parser fails on (built as test_clip_batches.py builds
    it): the batch is parsed again on the host with the same windows and pads.  The output equals the host-parser run's, the final
    table (synth_segments) is the host-parser run's, and over it every clip holds the oracle's slice.  The clip with the throwing
    packet has no upper end (take = -1): with a bounded take the look-ahead, which counts the throwing packet's samples, may
    declare the window full earlier than the host parser does, and the replayed segment then comes out shorter than the
    host-parser run's -- the limit include/nvorbis_hip.h states; its samples are still the oracle's."""
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
    runs = [good[0:5], good[5:8], good[8:10] + [bad[len(bad) // 2]] + good[10:12], good[12:18], good[18:20]]
    wins = [(4, 200, 512), (1, 77, 512), (3, -1, 0), (130, 300, 512), (0, 512, 512)]
    res = {}
    for gpu_parse in (False, True):
        st = _open(nv, gpu_ctx, hdr, gpu_parse)
        try:
            errors = 0
            for run, w in zip(runs, wins):
                st.segment_window(*w)
                for i in run:
                    try:
                        st.push_packet(pk[i], -1, 0)
                    except native.NvhError:
                        errors += 1
                st.next_segment(4)
            n = st.pending()[1]
            buf = torch.full((n * 2 + 64,), float(SENTINEL[np.dtype(np.float32)]), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            wr = st.synth_device(buf.data_ptr(), n * 2)
            errors += len(st.parse_errors)
            res[gpu_parse] = (st.synth_segments().copy(), wr, buf.cpu().numpy(), errors)
        finally:
            st.close()
    (th, wh, ph, eh), (tg, wg, pg, eg) = res[False], res[True]
    assert eh == eg == 1
    assert np.array_equal(tg, th) and wg == wh == th[-1, 2] * 2
    assert same_bits(pg[:wg], ph[:wh]) and (pg[wg:] == SENTINEL[np.dtype(np.float32)]).all()
    out = pg[:wg].reshape(-1, 2)
    covered = np.zeros(out.shape[0], bool)
    for k, (run, (skip, take, pitch)) in enumerate(zip(runs, wins)):
        b, e = int(tg[k, 1]), int(tg[k, 2])
        covered[b:e] = True
        kept = [i for i in run if i not in bad]
        ref, _ = oracle.decode_packets(hdr + [pk[i] for i in kept], [-1] * (3 + len(kept)), [0] * (3 + len(kept)))
        assert same_bits(out[b:e], cut(ref.reshape(-1, 2), skip, take)), (k, b, e)
        if pitch:
            assert int(tg[k + 1, 1]) == b + pitch
    assert (~covered).any() and not out[~covered].view(np.uint8).any()


@pytest.mark.gpu
def test_gpu_tests_under_the_toggles():
    """This file's GPU tests once more in child processes under the kernel-variant toggles, one child at a time, each under a
    time limit of its own; the first child that fails ends the test."""
    if os.environ.get("NVH_TEST_CHILD"):
        return  # inside a replay
    from tests.replay import run_children
    for toggle in ["NVH_FPW=1", "NVH_NO_EMIT", "NVH_NO_SLAB", "NVH_POISON_PLANES+NVH_GPU_PARSE"]:
        env = dict(os.environ)
        for t in toggle.split("+"):
            key, _, val = t.partition("=")
            env[key] = val or "1"
        env["NVH_TEST_CHILD"] = "1"
        run_children([(["test_segment_windows.py"], env, ["-k", "not toggles"])], timeout=300)

"""Per-segment HasClipped: which clip of a batch clipped (nvh_stream_synth_segments_clipped, Stream.synth_segments_clipped,
decode_clips / decode_clip_rows with return_clipped=True; include/nvorbis_hip.h states the rule).

The reference of every flag is the CPU oracle on that clip ALONE, never the library's own output: oracle.decode_packets with
clip=False, the output form's rule applied on the CPU (tests/test_clip_batches.py: mix_rule; a map selects columns; a window
cuts rows), and the test |y| > 0.99999994f.  Every comparison is exact.  Every test first asserts that its reference vector
holds BOTH values: a vector of one value would let the sticky word pass for a per-segment flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_clip_batches import (CLIP, GOLDEN, ROOT, Segmented, _descriptor_toggle, _device_synth, _open, _own_output, _torch,
                                     make_clips, mix_rule, oracle_clips, same_bits, stream_packets, to_s16)

NAME = "nvh_stream_synth_segments_clipped"
# 3test.ogg: 45 clips of 8 consecutive packets from packet 3 on; the synthetic setups: 50 clips of 2 packets (the smallest clips
# that emit anything).  No end-of-stream flags, no granules.
SHAPES_OGG = tuple((3 + 8 * k, 8, "none") for k in range(45))
SHAPES_SYN = tuple((3 + 2 * k, 2, "none") for k in range(50))
SETUPS = ("stereo_res1_coupled", "mono_res0_small_blocks", "six_ch_res2_4096", "stereo_8192", "floor0_slab")
# the oracle's flagged clips (checked on the CPU when the inputs were chosen; asserted again below)
FLAGGED = {"3test.ogg": 4, "stereo_res1_coupled": 18, "mono_res0_small_blocks": 9, "six_ch_res2_4096": 40, "stereo_8192": 22,
           "floor0_slab": 22}
CORE = [(n, g) for n in SETUPS + ("3test.ogg",) for g in (False, True) if not (n == "floor0_slab" and g)]  # Floor0: host parser only


def shapes_of(name):
    return SHAPES_OGG if name.endswith(".ogg") else SHAPES_SYN


def over(x):
    """ClipSamples clamps at least one of these samples (Utils.cs:30-43: a NaN compares false twice and passes)."""
    x = np.asarray(x, np.float32)
    return bool(((x > CLIP) | (x < -CLIP)).any())


def form_rows(raw, ch, form=None):
    """The unclipped samples an output form emits, as rows [T, output channels]: "mono" -> the mix, a tuple -> the map's
    channels, anything else (f32, s16, planar: the clip comes before the conversion and the layout) -> every channel."""
    x = np.asarray(raw, np.float32).reshape(-1, ch)
    if form == "mono":
        return mix_rule(x, ch, False).reshape(-1, 1) if ch > 1 else x
    if isinstance(form, tuple):
        return x[:, list(form)]
    return x


def oracle_flags(oracle, name, form=None):
    """The oracle's per-clip flag vector for an output form, from its UNCLIPPED PCM of each clip alone."""
    raw, ch = oracle_clips(oracle, name, False, shapes_of(name))
    return np.array([over(form_rows(r, ch, form)) for r, _ in raw], bool)


def both_values(v):
    v = np.asarray(v, bool)
    return bool(v.any() and not v.all())


class Flagged(Segmented):
    """tests.test_clip_batches.Segmented, which also collects every batch's (synth_segments, synth_segments_clipped) pair."""

    def __init__(self, st, nclips, bf, align, synth, pipelined=False):
        self.batches, self.pipelined = [], pipelined

        def wrapped(st_, table, n):
            rows = synth(st_, table, n)
            if not self.pipelined:  # (a pipelined batch's pair is valid from its synth_end on: note() is called there)
                self.note(table)
            return rows
        Segmented.__init__(self, st, nclips, bf, align, wrapped)

    def note(self, pending_table):
        final, flags = self.st.synth_segments(), self.st.synth_segments_clipped()
        assert flags.dtype == np.bool_ and flags.shape == (final.shape[0],), (flags.dtype, flags.shape, final.shape)
        if not self.st.parse_errors:  # (no replay: the look-ahead's table is the batch's)
            assert np.array_equal(final, pending_table), (final, pending_table)
        self.batches.append((final.copy(), flags.copy()))

    def per_clip(self, nclips):
        out = np.zeros(nclips + 1, bool)
        for table, flags in self.batches:
            for (k, b, e), hit in zip(table, flags):
                assert not (hit and e == b), "a segment without samples in the batch is flagged"
                out[int(k)] |= bool(hit)
        assert not out[nclips]  # the segment left open behind the last clip
        return out[:nclips]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_exported_and_declared():
    from nvorbis_amd import native
    hdr = open(os.path.join(ROOT, "include", "nvorbis_hip.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "NativeMethods.cs")).read()
    assert hasattr(native.lib(), NAME)
    assert NAME in native.SIGNATURES
    assert re.search(r"\bint %s\s*\(" % NAME, hdr)
    assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern (?:unsafe )?int %s\(" % NAME, cs)
    assert "HasClipped is the OR over every segment since the last reset" not in hdr  # the sentence names both calls now


def test_the_entry_point_refuses_bad_arguments(oracle):
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    n = C.c_int(-1)
    a = (C.c_int * 4)()
    assert L.nvh_stream_synth_segments_clipped(None, a, 4, C.byref(n)) == native.ERR_ARGUMENT
    pk = stream_packets(oracle, "3test.ogg")
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        assert L.nvh_stream_synth_segments_clipped(st._h, a, 4, None) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_segments_clipped(st._h, None, 4, C.byref(n)) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_segments_clipped(st._h, a, -1, C.byref(n)) == native.ERR_ARGUMENT
        # a host-only stream never synthesises: no entries, whatever was pushed
        for p in pk[3:12]:
            st.push_packet(p, -1, 0)
        st.next_segment(4)
        n.value = -1
        assert L.nvh_stream_synth_segments_clipped(st._h, None, 0, C.byref(n)) == native.OK and n.value == 0
        got = st.synth_segments_clipped()
        assert got.dtype == np.bool_ and got.shape == (0,)
        assert st.synth_segments().shape == (0, 3)
        st.reset()
        assert st.synth_segments_clipped().shape == (0,)
    finally:
        st.close()


def test_return_clipped_is_checked_before_a_device(ogg_bytes):
    import nvorbis_amd as nv
    for bad in (1, 0, None, "yes", [True]):
        with pytest.raises(ValueError):
            nv.decode_clips([b"x"], return_clipped=bad)
        with pytest.raises(ValueError):
            nv.decode_clip_rows([b"x"], 64, return_clipped=bad)
    res, clipped = nv.decode_clips([], return_clipped=True)
    assert res == [] and clipped.dtype == np.bool_ and clipped.shape == (0,)
    assert nv.decode_clips([], return_clipped=False) == []
    (rows, valid), clipped = nv.decode_clip_rows([], 64, return_clipped=True)
    assert rows.shape == (0, 64, 1) and valid.shape == (0,) and clipped.dtype == np.bool_ and clipped.shape == (0,)
    # a row of no samples has nothing to clamp (no device is opened for length 0)
    (rows, valid), clipped = nv.decode_clip_rows([ogg_bytes["3test"]], 0, return_clipped=True)
    assert rows.shape[:2] == (1, 0) and not clipped.any() and clipped.shape == (1,)


@pytest.mark.parametrize("name", SETUPS + ("3test.ogg",))
def test_the_inputs_hold_both_values(oracle, name):
    """The condition on the inputs every GPU test rests on, for every form it is used with."""
    plain = oracle_flags(oracle, name)
    assert int(plain.sum()) == FLAGGED[name] and both_values(plain), (name, plain.sum())
    raw, ch = oracle_clips(oracle, name, False, shapes_of(name))
    ref, _ = oracle_clips(oracle, name, True, shapes_of(name))
    assert [bool(hc) for _, hc in ref] == list(plain)  # the oracle's own HasClipped per clip is this vector
    if name == "3test.ogg":
        assert list(np.nonzero(plain)[0]) == [2, 19, 25, 39]
        assert list(np.nonzero(oracle_flags(oracle, name, "mono"))[0]) == [2, 19]
    if name in ("stereo_res1_coupled", "six_ch_res2_4096"):
        for form in ("mono", (0,)):
            v = oracle_flags(oracle, name, form)
            assert both_values(v) and (v != plain).any(), (name, form)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,gpu_parse", CORE)
def test_core(oracle, gpu_ctx, name, gpu_parse):
    """Every input, both parsers, batches of 1024, 13 and 2 frames (13 and 2 put batch boundaries inside clips and exactly on clip
    boundaries): per clip the OR of its entries over the batches is the oracle's flag, every batch's flags are aligned with its
    synth_segments(), has_clipped() is the OR of everything, and the PCM is still the oracle's bit for bit."""
    torch = _torch()
    import nvorbis_amd as nv
    shapes = shapes_of(name)
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name, shapes)
    refs, ch = oracle_clips(oracle, name, True, shapes)
    want = oracle_flags(oracle, name)
    assert both_values(want), name
    if name.startswith("floor0") and _descriptor_toggle():  # (the existing suites' one exception: Floor0 on the descriptor kernels)
        refs = [(_own_output(nv, gpu_ctx, hdr, c, True), hc) for c, (_, hc) in zip(clips, refs)]
    for bf in (1024, 13, 2):
        st = _open(nv, gpu_ctx, hdr, gpu_parse, True)
        try:
            seg = Flagged(st, len(clips), bf, 4, _device_synth(torch)).run(clips)
            got = seg.per_clip(len(clips))
            assert np.array_equal(got, want), (name, gpu_parse, bf, np.nonzero(got != want)[0])
            assert st.has_clipped() == bool(got.any())
            for i, (ref, _) in enumerate(refs):
                assert same_bits(seg.clip_rows(i, ch, np.float32).reshape(-1), ref), (name, gpu_parse, bf, i)
            if bf == 1024:
                assert len(seg.batches) == 1 and seg.batches[0][0].shape[0] == len(clips) + 1
            else:
                assert len(seg.batches) > 4
                # a clip across a batch boundary, and a batch that ends exactly on a clip boundary
                assert any(t[0, 0] == p[-1, 0] and t[0, 2] > 0 and p[-1, 2] > p[-1, 1] for p, t in zip(seg.tables, seg.tables[1:]))
                assert any(p[-1, 1] == p[-1, 2] and len(p) > 1 for p in seg.tables)
        finally:
            st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,gpu_parse", CORE)
def test_clip_samples_off(oracle, gpu_ctx, name, gpu_parse):
    """ClipSamples off: nothing is clamped, every entry is 0 -- on inputs that would flag clips."""
    torch = _torch()
    import nvorbis_amd as nv
    shapes = shapes_of(name)
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name, shapes)
    assert both_values(oracle_flags(oracle, name))
    st = _open(nv, gpu_ctx, hdr, gpu_parse, False)
    try:
        seg = Flagged(st, len(clips), 13, 4, _device_synth(torch)).run(clips)
        assert len(seg.batches) > 4 and sum(f.size for _, f in seg.batches) > len(clips)
        assert not any(f.any() for _, f in seg.batches) and not st.has_clipped()
    finally:
        st.close()


FORMS = [(n, f) for n in ("stereo_res1_coupled", "six_ch_res2_4096") for f in ("s16", "planar", "mono", "map0", "wave", "pipelined")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", FORMS)
def test_forms(oracle, gpu_ctx, name, form):
    """One run per output form, batches of 13 frames: the flags are the form's rule on the oracle's unclipped PCM -- the mix
    decides with "mono", only the emitted channel counts with the map (0,) -- and the PCM is the form's rule on the oracle's."""
    torch = _torch()
    import nvorbis_amd as nv
    shapes = shapes_of(name)
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name, shapes)
    refs, ch = oracle_clips(oracle, name, True, shapes)
    raw, _ = oracle_clips(oracle, name, False, shapes)
    rows = [r.reshape(-1, ch) for r, _ in refs]
    plain = oracle_flags(oracle, name)
    from nvorbis_amd.reader import wave_channel_map
    if form == "s16":
        want, pcm, dt, och, synth = plain, [to_s16(r) for r in rows], np.int16, ch, _device_synth(torch, np.int16)
    elif form == "planar":
        want, pcm, dt, och, synth = plain, rows, np.float32, ch, _device_synth(torch, planar=True)
    elif form == "mono":
        want = oracle_flags(oracle, name, "mono")
        pcm, dt, och, synth = [mix_rule(r, ch, True).reshape(-1, 1) for r, _ in raw], np.float32, 1, _device_synth(torch, och=1, mix="mono")
        assert (want != plain).any()
    elif form == "map0":
        want = oracle_flags(oracle, name, (0,))
        pcm, dt, och, synth = [np.ascontiguousarray(r[:, :1]) for r in rows], np.float32, 1, _device_synth(torch, och=1, channel_map=(0,))
        assert (want != plain).any()
    elif form == "wave":  # a permutation of every channel: the un-mixed vector (the identity for two channels)
        want, dt, och, synth = plain, np.float32, ch, _device_synth(torch, och=ch, channel_map="wave")
        pcm = [np.ascontiguousarray(r[:, list(wave_channel_map(ch))]) for r in rows]
    else:
        want, pcm, dt, och = plain, rows, np.float32, ch
    assert both_values(want), (name, form)
    st = _open(nv, gpu_ctx, hdr, form == "pipelined")
    try:
        if form == "pipelined":
            flights = []

            def end_one():
                t, m = flights.pop(0)
                out = st.synth_end().reshape(m, ch)
                seg.note(t)  # valid from this batch's synth_end on: the flight carried its flags
                seg.route(t, out)

            def synth(st_, table, n):  # begin this batch, end the one before: two flights are outstanding in between
                assert st_.synth_begin() == n * ch
                flights.append((table, n))
                if len(flights) == 2:
                    end_one()
                return None
            seg = Flagged(st, len(clips), 13, 4, synth, pipelined=True)
            seg.run(clips)
            while flights:
                end_one()
        else:
            seg = Flagged(st, len(clips), 13, 4, synth).run(clips)
        got = seg.per_clip(len(clips))
        assert np.array_equal(got, want), (name, form, np.nonzero(got != want)[0])
        assert st.has_clipped() == bool(got.any())
        assert len(seg.batches) > 4
        for i, w in enumerate(pcm):
            assert same_bits(seg.clip_rows(i, och, dt), w), (name, form, i)
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_windows(oracle, gpu_ctx, gpu_parse):
    """Only the emitted samples count.  Clip 2 of 3test.ogg as three rows -- a window that ends in front of its first sample
    outside +-1, one of eight samples around it, one that begins behind its last -- among rows of clips 0, 1 and 3, one batch,
    with a pitch, so that pads lie between the rows.  The indices come from the oracle's unclipped PCM."""
    torch = _torch()
    import nvorbis_amd as nv
    name = "3test.ogg"
    hdr = stream_packets(oracle, name)[:3]
    clips = make_clips(oracle, name, SHAPES_OGG)
    raw, ch = oracle_clips(oracle, name, False, SHAPES_OGG)
    refs, _ = oracle_clips(oracle, name, True, SHAPES_OGG)
    x2 = raw[2][0].reshape(-1, ch)
    bad = np.nonzero(((x2 > CLIP) | (x2 < -CLIP)).any(axis=1))[0]
    total, first, last = x2.shape[0], int(bad[0]), int(bad[-1])
    before = first & ~3              # [0, before) ends in front of the first offending sample
    behind = (last + 4) & ~3         # [behind, end) begins behind the last one
    assert before >= 4 and before <= first < before + 8 and last < behind < total - 4, (first, last, total)
    pitch = (max(r.size // ch for r, _ in raw[:4]) + 67) & ~3
    order = [0, 2, 1, 2, 3, 2]
    wins = [(0, pitch, pitch), (0, before, pitch), (0, pitch, pitch), (before, 8, pitch), (0, pitch, pitch), (behind, pitch, pitch)]
    cut = [r[0].reshape(-1, ch)[s:s + t] for r, (s, t, _) in zip((raw[i] for i in order), wins)]
    want = np.array([over(c) for c in cut], bool)
    assert list(want) == [False, False, False, True, False, False]
    st = _open(nv, gpu_ctx, hdr, gpu_parse)
    try:
        for i, w in zip(order, wins):
            st.segment_window(*w)
            for p, g, f in zip(*clips[i]):
                st.push_packet(p, g, f)
            st.next_segment(4)
        n = st.pending()[1]
        assert n == len(order) * pitch
        out = _device_synth(torch)(st, None, n)
        table, flags = st.synth_segments(), st.synth_segments_clipped()
        assert table.shape == (len(order) + 1, 3) and flags.shape == (len(order) + 1,)
        assert np.array_equal(flags[:-1], want) and not flags[-1], (flags, want)
        assert st.has_clipped()
        covered = np.zeros(n, bool)
        for k, ((_, b, e), i, (s, t, _)) in enumerate(zip(table, order, wins)):
            assert b == k * pitch
            assert same_bits(out[b:e], refs[i][0].reshape(-1, ch)[s:s + t]), k
            covered[b:e] = True
        assert (~covered).sum() > 0 and not out[~covered].view(np.uint8).any()  # the pads: zeros, and they set no flag
    finally:
        st.close()


@pytest.mark.gpu
def test_a_replayed_batch_reports_by_its_final_table(oracle, gpu_ctx):
    """GPU-parse mode, one clip in the middle of the batch holds a packet the parser fails on (tests/test_clip_batches.py's
    damaged packet): the batch is parsed again, and the flags follow the table as finally parsed, for the segments in front of
    and behind the failure.  The reference is the oracle on each clip alone, the failing packet left out (it leaves no frame)."""
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
    nclips, middle = len(good) // 2, 24  # (few of these clips clip: every pair of packets that parses, the failure between two that do)
    assert bad and nclips >= 36
    runs = [good[2 * k:2 * k + 2] for k in range(nclips)]
    want = []
    for run in runs:
        raw, info = oracle.decode_packets(hdr + [pk[i] for i in run], [-1] * (3 + len(run)), [0] * (3 + len(run)), clip=False)
        want.append(over(raw))
    want = np.array(want, bool)
    assert both_values(want[:middle]) and both_values(want[middle + 1:]), want  # in front of and behind the failure
    runs[middle] = [runs[middle][0], bad[len(bad) // 2], runs[middle][1]]
    res = {}
    for gpu_parse in (False, True):
        st = _open(nv, gpu_ctx, hdr, gpu_parse)
        try:
            for run in runs:
                for i in run:
                    try:
                        st.push_packet(pk[i], -1, 0)
                    except native.NvhError:
                        assert not gpu_parse
                st.next_segment(4)
            look = st.pending_segments()
            n = st.pending()[1]
            buf = torch.zeros(max(n * 2, 1), dtype=torch.float32, device="cuda")
            st.synth_device(buf.data_ptr(), n * 2)
            assert bool(st.parse_errors) == gpu_parse
            table, flags = st.synth_segments(), st.synth_segments_clipped()
            assert flags.shape == (table.shape[0],) and table.shape[0] == nclips + 1
            assert np.array_equal(flags[:-1], want) and not flags[-1], (gpu_parse, np.nonzero(flags[:-1] != want)[0])
            assert st.has_clipped()
            res[gpu_parse] = (look, table)
        finally:
            st.close()
    assert np.array_equal(res[True][1], res[False][1])          # the table as finally parsed is the host parser's
    assert not np.array_equal(res[True][0], res[True][1])       # ... and not the look-ahead's: the batch was parsed again


@pytest.mark.gpu
def test_a_stream_without_segments_launches_what_it_launched(oracle, gpu_ctx):
    """A plain Stream over 3test.ogg, never a next_segment, four batches of 64 packets: every batch names the kernels a resident
    batch of the same packets names (resident batches have no table at all), the default route is still the frame-group kernel,
    and the one entry is what the batch adds to has_clipped() -- the oracle's flag for the batch's samples, cut out of its
    unclipped decode of the 256 packets by the batches' sample counts."""
    torch = _torch()
    import nvorbis_amd as nv
    pk = stream_packets(oracle, "3test.ogg")
    run = list(pk[3:3 + 256])
    raw, info = oracle.decode_packets(pk[:3] + run, [-1] * (3 + len(run)), [0] * (3 + len(run)), clip=False)
    ref, _ = oracle.decode_packets(pk[:3] + run, [-1] * (3 + len(run)), [0] * (3 + len(run)), clip=True)
    toggled = any(os.environ.get(t) for t in ("NVH_NO_EMIT", "NVH_NO_SLAB", "NVH_FPW", "NVH_UNFUSED", "NVH_NO_FUSED_IMDCT",
                                              "NVH_NO_COMPACT", "NVH_GPU_PARSE", "NVH_EMIT_ALWAYS"))
    st, twin = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2]), nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    try:
        at, want, got = 0, [], []
        for first in range(0, 256, 64):
            for p in run[first:first + 64]:
                st.push_packet(p, -1, 0)
                twin.push_packet(p, -1, 0)
            pcm = st.synth_host().copy()
            flags, table = st.synth_segments_clipped(), st.synth_segments()
            assert table.shape == (1, 3) and flags.shape == (1,) and table[0, 2] * st.channels == pcm.size
            assert same_bits(pcm, ref[at:at + pcm.size]), first
            want.append(over(raw[at:at + pcm.size]))
            got.append(bool(flags[0]))
            at += pcm.size
            assert st.has_clipped() == any(got), (first, got)  # the sticky flag: the OR of every entry so far
            b = twin.upload_batch()
            dev = torch.empty(max(b.samples * twin.channels, 1), dtype=torch.float32, device="cuda")
            b.synth(dev.data_ptr(), dev.numel())
            assert list(st.kernels()) == list(b.kernels()), (first, st.kernels(), b.kernels())
            b.free()
            if not toggled and first > 0:
                assert st.kernels()[1] == "k_synth_group2", st.kernels()
        assert both_values(want), want
        assert got == want
    finally:
        st.close()
        twin.close()


_OGG45 = []


def ogg_clips(nv, oracle):
    """The 45 clips of 3test.ogg re-wrapped as Ogg files of their own (granules as an encoder writes them), and the oracle's
    clipped and unclipped decode of each FILE."""
    from tests import ogg_py
    if not _OGG45:
        pk = stream_packets(oracle, "3test.ogg")
        files = []
        for k, (first, n, _) in enumerate(SHAPES_OGG):
            run = list(pk[first:first + n])
            d = nv.Stream(None, pk[0], pk[1], pk[2])
            _, em, _, _ = d.index_packets(nv.PacketArray.from_list(pk[:3] + run))
            d.close()
            files.append(ogg_py.write_ogg(pk[:3] + run, [0, 0, 0] + [int(v) for v in em], serial=0x3000 + k))
        _OGG45.append((files, [oracle.decode_ogg(f) for f in files], [oracle.decode_ogg(f, clip=False) for f in files]))
    return _OGG45[0]


@pytest.mark.gpu
@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_decode_clips_and_rows_return_clipped(oracle, gpu_ctx, fmt, device_out):
    """decode_clips and decode_clip_rows with return_clipped=True over the 45 clips as Ogg files: the array is the oracle's
    vector (rows: of the samples the row holds), and without the keyword the return value has the old shape and the same bits."""
    _torch()
    import nvorbis_amd as nv
    files, refs, raws = ogg_clips(nv, oracle)
    ch = refs[0][1]["channels"]
    want = np.array([over(r) for r, _ in raws], bool)
    assert both_values(want) and [bool(i["has_clipped"]) for _, i in refs] == list(want)
    host = (lambda g: g.cpu().numpy()) if device_out else (lambda g: np.asarray(g))
    for bf in (64, 4096):
        got, clipped = nv.decode_clips(files, ctx=gpu_ctx, batch_frames=bf, sample_format=fmt, device_out=device_out, return_clipped=True)
        old = nv.decode_clips(files, ctx=gpu_ctx, batch_frames=bf, sample_format=fmt, device_out=device_out)
        assert clipped.dtype == np.bool_ and np.array_equal(clipped, want), (fmt, device_out, bf, np.nonzero(clipped != want)[0])
        assert isinstance(old, list) and len(old) == len(got) == len(files)
        for i, ((ref, _), g, o) in enumerate(zip(refs, got, old)):
            w = to_s16(ref) if fmt == "s16" else ref
            assert same_bits(host(g), w) and same_bits(host(o), w), (fmt, device_out, bf, i)
    # rows: [start, start + length) of every clip; the flags are those samples'
    length = 512
    starts = [(37 * i) % 1900 // 4 * 4 for i in range(len(files))]
    rwant = np.array([over(r.reshape(-1, ch)[s:s + length]) for (r, _), s in zip(raws, starts)], bool)
    assert both_values(rwant)
    assert (rwant != want).any()  # some clip clips only outside its row
    (rows, valid), rclipped = nv.decode_clip_rows(files, length, starts=starts, ctx=gpu_ctx, batch_frames=64, sample_format=fmt,
                                                   device_out=device_out, return_clipped=True)
    orows, ovalid = nv.decode_clip_rows(files, length, starts=starts, ctx=gpu_ctx, batch_frames=64, sample_format=fmt,
                                        device_out=device_out)
    assert rclipped.dtype == np.bool_ and np.array_equal(rclipped, rwant), np.nonzero(rclipped != rwant)[0]
    assert np.array_equal(valid, ovalid) and same_bits(host(rows), host(orows))
    for i, ((ref, _), s) in enumerate(zip(refs, starts)):
        w = ref.reshape(-1, ch)[s:s + length]
        w = to_s16(w) if fmt == "s16" else w
        assert valid[i] == w.shape[0] and same_bits(host(rows)[i, :w.shape[0]], w), i
        assert not host(rows)[i, w.shape[0]:].any()


@pytest.mark.gpu
def test_core_and_forms_under_the_toggles():
    """test_core and test_forms once more in child processes under the kernel-variant toggles, two children at a time: with
    these, every emitting family's report site runs (k_synth_emit, k_synth_group4, k_synth8_emit's staged and direct forms,
    k_ola_compact alone, the descriptor kernels' k_ola_emit)."""
    if os.environ.get("NVH_TEST_CHILD"):
        return  # inside a replay
    from tests.replay import run_children
    children = []
    for toggle in ["NVH_FPW=1", "NVH_FPW=4", "NVH_EMIT_ALWAYS", "NVH_NO_EMIT8", "NVH_NO_SLAB", "NVH_NO_COMPACT"]:
        env = dict(os.environ)
        key, _, val = toggle.partition("=")
        env[key] = val or "1"
        env["NVH_TEST_CHILD"] = "1"
        children.append((["test_segment_clipped.py"], env, ["-k", "test_core or test_forms"]))
    for k in range(0, len(children), 2):
        run_children(children[k:k + 2], timeout=900)

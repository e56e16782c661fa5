"""Frame groups (kernels_synth.hip: synth_group_body -- k_synth_group2, k_synth_group4) and one frame per workgroup (k_synth +
k_synth_emit / k_synth_tail) at their edges: block-size switches at every offset inside a group and at the boundaries between the
groups of the two launches, short runs, partly filled last groups, batch boundaries on switches, silent channels, the end-of-stream
trim, the 7/8 threshold that sends a batch back to k_synth + k_ola_compact, clip on and off, and the automatic fall-back from groups
to one frame per workgroup when a group's LDS does not fit (nvh_launch.hip: slab_size_ok).

Every stream is written by the structured encoder (tests/vorbis_encode.py: full-depth packets) with block kinds placed at chosen
frame indices.  Every GPU decode is bit-exact against the oracle; the switch patterns of the stereo and the mono setup also agree
with the spec-derived decoder (tests/vorbis_spec.py) within 1e-6 of the peak, and a CPU test pins oracle against spec on the same
streams, so that a mismatch can be put down to the product or to the oracle.

The frames per workgroup come from the process's NVH_FPW (default 2); tests/test_gpu_parity.py replays this file under NVH_FPW=1
and NVH_FPW=4, and the last test here replays it itself and checks that every float PCM-writing synthesis variant was reached."""
import functools
import json
import os

import numpy as np
import pytest

from tests import vorbis_encode as ve
from tests import vorbis_spec
from tests.synth_stream import BitWriter, comment_header, ilog, write_floor1, write_mapping, write_residue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the synthesis slot's name of a batch with paired emission, by frames per workgroup
EMIT_NAME = {1: "k_synth+k_synth_emit", 2: "k_synth_group2", 4: "k_synth_group4"}
# toggles that change which kernels run: under any of them the name assertions are skipped, never the PCM ones
_KERNEL_TOGGLES = ("NVH_EMIT_ALWAYS", "NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_GPU_PARSE", "NVH_COPY_UPLOAD",
                   "NVH_NO_EMIT", "NVH_NO_EMIT8", "NVH_NO_SLAB", "NVH_POISON_PLANES")
_SEEN = set()   # synthesis-slot names of batches whose PCM was compared bit-exact in this process
_TAIL = [0]     # of them: FPW = 1 batches with paired emission whose last decoded frame is odd (k_synth_tail, nvh_launch.hip)


def _fpw():
    v = os.environ.get("NVH_FPW", "2")
    return int(v) if v in ("1", "2", "4") else 2


def _names_checked():
    return not any(os.environ.get(t) for t in _KERNEL_TOGGLES)


# ---------------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------------

def switch_kinds():
    """Block kinds (True = long) with every case at a known frame index: a long->short and a short->long switch at every
    offset modulo 8 (so at every offset inside groups of 2 and 4, and on both kinds of boundary between the groups of the two
    launches), isolated short blocks, runs of 2..5 short blocks, a short first and a short last block.  109 frames."""
    runs = [(False, 2)]
    longs = [3, 6, 4, 7, 5, 9, 2, 8, 3, 5, 7, 4, 6, 1, 5]
    shorts = [1, 2, 3, 4, 5, 1, 3, 2, 1, 4, 5, 2, 1, 3]
    for k in range(len(shorts)):
        runs.append((True, longs[k]))
        runs.append((False, shorts[k]))
    kinds = np.concatenate([np.full(n, k, dtype=bool) for k, n in runs])
    return kinds


def switches(kinds, to_short):
    """Frame indices where the kind changes: the first short block after a long one (to_short) or the first long after a short."""
    k = np.asarray(kinds)
    i = np.nonzero(k[1:] != k[:-1])[0] + 1
    return [int(j) for j in i if bool(k[j]) != to_short]


def short_runs(kinds):
    """Lengths of the runs of short blocks that have a long block on both sides."""
    out, i, k = [], 0, list(kinds)
    while i < len(k):
        if not k[i]:
            j = i
            while j < len(k) and not k[j]:
                j += 1
            if i > 0 and j < len(k):
                out.append(j - i)
            i = j
        else:
            i += 1
    return out


@functools.lru_cache(maxsize=None)
def _shipped(name):
    return ve.shipped_headers(open(os.path.join(GOLDEN, name + ".ogg"), "rb").read())


def deep_slab_headers():
    """3test.ogg's books and floors, stereo 256/2048, coupling (0, 1); the long blocks' Residue2 has partitions of 4 bins and
    six cascade stages in every class, each a dim-2 lattice book: a full-depth frame's slab is ~40 KB -- too big for four frames
    in the CU's LDS, small enough for one (the window of nvh_launch.hip: slab_size_ok at NVH_FPW=4)."""
    base = ve.setup_of(_shipped("3test"))
    long_mode = next(i for i, (f, _) in enumerate(base.modes) if f)
    short_mode = next(i for i, (f, _) in enumerate(base.modes) if not f)
    bm_long, bm_short = base.mappings[base.modes[long_mode][1]], base.mappings[base.modes[short_mode][1]]
    dim2 = [i for i, b in enumerate(base.books) if b.dims == 2 and b.lookup_type == 1]
    w = BitWriter()
    for b in b"\x05vorbis":
        w.write(b, 8)
    base.copy_book_bits(w)
    w.write(0, 6)
    w.write(0, 16)
    w.write(1, 6)  # two floors: the file's own
    for fl in (base.floors[bm_short.submap_floor[0]], base.floors[bm_long.submap_floor[0]]):
        ncls = max(fl.partition_class) + 1
        write_floor1(w, fl.partition_class, {c: fl.class_dims[c] for c in range(ncls)}, {c: fl.class_subs[c] for c in range(ncls)},
                     {c: fl.class_master[c] for c in range(ncls)}, {c: fl.sub_books[c] for c in range(ncls)}, fl.multiplier,
                     ilog(fl.xs[1]) - 1, fl.xs[2:])
    w.write(1, 6)  # two residues: the file's short one, the deep long one
    rs = base.residues[bm_short.submap_residue[0]]
    write_residue(w, 2, rs.begin, rs.end, rs.psize, rs.classbook, rs.cascade, [b for row in rs.books for b in row if b >= 0])
    rl = base.residues[bm_long.submap_residue[0]]
    stages = 6
    write_residue(w, 2, 0, 2 * 1024, 4, rl.classbook, [(1 << stages) - 1] * rl.nclass,
                  [dim2[(c + s) % len(dim2)] for c in range(rl.nclass) for s in range(stages)])
    w.write(1, 6)  # two mappings, two modes
    write_mapping(w, 2, 1, [(0, 1)], None, [(0, 0)])
    write_mapping(w, 2, 1, [(0, 1)], None, [(1, 1)])
    w.write(1, 6)
    for flag, mp in ((0, 0), (1, 1)):
        w.write(flag, 1)
        w.write(0, 16)
        w.write(0, 16)
        w.write(mp, 8)
    w.write(1, 1)
    return [_shipped("3test")[0], comment_header(), w.bytes()]


@functools.lru_cache(maxsize=None)
def headers(setup):
    """stereo: 3test.ogg (256/2048, Floor1, Residue2, coupling); mono: 1test.ogg (256/2048); equal: stereo 1024/1024 (both modes
    one block size: never a size switch); deep: deep_slab_headers."""
    if setup == "stereo":
        return tuple(_shipped("3test"))
    if setup == "mono":
        return tuple(_shipped("1test"))
    if setup == "equal":
        return tuple(ve.c4_headers(_shipped("3test"), psize=48, channels=2, block0=1024, block1=1024, end_per_channel=384))
    if setup == "deep":
        return tuple(deep_slab_headers())
    raise KeyError(setup)


def encode(setup, kinds, seed, silent=None):
    """Full-depth packets for `kinds` with consistent window flags; silent: {frame index: channels with an unused floor}.
    Returns (packets, granules, flags) as lists."""
    hdr = list(headers(setup))
    S = ve.setup_of(hdr)
    rng = np.random.default_rng(seed)
    enc = ve.PacketEncoder(S)
    long_mode = next(i for i, (f, _) in enumerate(S.modes) if f)
    short_mode = next((i for i, (f, _) in enumerate(S.modes) if not f), long_mode)
    pk, n = list(hdr), len(kinds)
    for i in range(n):
        sil = (silent or {}).get(i, ())
        if kinds[i]:
            pk.append(enc.packet(rng, long_mode, 1 if (i == 0 or kinds[i - 1]) else 0, 1 if (i + 1 >= n or kinds[i + 1]) else 0, silent=sil))
        else:
            pk.append(enc.packet(rng, short_mode, silent=sil))
    gr = [-1, -1, -1] + ve.granules_for(S, kinds)
    return pk, gr, [0] * len(pk)


def trimmed(pk, gr, fl, d):
    """The stream ending d samples early: the last packet's granule lowered and marked end of stream."""
    gr, fl = list(gr), list(fl)
    gr[-1] -= d
    fl[-1] = 1
    return pk, gr, fl


# Streams of the tests below: (setup, kinds, seed, silent, trim).  N0 frames of the pattern; N0 - 1 .. N0 - 3 leave last groups of
# 3, 2 and 1 frames at FPW = 4 (of 1 and 2 at FPW = 2).
_KINDS = switch_kinds()
N0 = len(_KINDS) - len(_KINDS) % 4


def _trim_kinds():
    k = switch_kinds()[:40].copy()
    k[-3:] = True  # ends on three long blocks: the last emits [0, 1024) before the trim
    return k


STREAMS = {
    "stereo_switches": ("stereo", _KINDS, 11, None, 0),
    "mono_switches": ("mono", _KINDS, 12, None, 0),
    "equal_switches": ("equal", _KINDS, 13, None, 0),
    "stereo_last_group_3": ("stereo", _KINDS[:N0 - 1], 14, None, 0),
    "stereo_last_group_2": ("stereo", _KINDS[:N0 - 2], 15, None, 0),
    "stereo_last_group_1": ("stereo", _KINDS[:N0 - 3], 16, None, 0),
    "mono_last_group_1": ("mono", _KINDS[:N0 - 3], 17, None, 0),
    # silent channels at chosen group offsets (one channel, the other, both), inside and at the edges of groups of 2 and 4
    "stereo_silent": ("stereo", np.ones(48, dtype=bool), 18, {5: {0}, 8: {1}, 9: {0, 1}, 14: {0}, 15: {1}, 22: {0, 1}, 31: {1}}, 0),
    "stereo_switches_silent": ("stereo", _KINDS[:64], 19, {int(i): {int(i) % 2} for i in switches(_KINDS[:64], True)[::2]}, 0),
    "mono_silent": ("mono", _KINDS[:48], 20, {3: {0}, 4: {0}, 12: {0}, 17: {0}}, 0),
    # end-of-stream trim: the last frame's valid a multiple of 64 (704) and not (691)
    "stereo_trim_64": ("stereo", _trim_kinds(), 21, None, 320),
    "stereo_trim_odd": ("stereo", _trim_kinds(), 22, None, 333),
    "mono_trim_odd": ("mono", _trim_kinds(), 23, None, 333),
}
SPEC_STREAMS = [k for k in STREAMS if k.startswith(("stereo", "mono"))]


@functools.lru_cache(maxsize=None)
def stream(name):
    setup, kinds, seed, silent, trim = STREAMS[name]
    pk, gr, fl = encode(setup, kinds, seed, silent)
    if trim:
        pk, gr, fl = trimmed(pk, gr, fl, trim)
    return pk, gr, fl


@functools.lru_cache(maxsize=None)
def oracle_pcm(oracle, name, clip):
    pk, gr, fl = stream(name)
    return oracle.decode_packets(pk, gr, fl, clip=clip)[0]


@functools.lru_cache(maxsize=None)
def spec_pcm(name):
    pk, gr, fl = stream(name)
    return vorbis_spec.decode_ogg_packets(pk, final_granule=gr[-1] if fl[-1] & 1 else None)[0]


def _spec_close(got, spec, clip):
    """Within test_spec_pin.py::test_c2_grand_full_depth_spec_vs_oracle's bound: 1e-6 of the peak (of the unclipped spec PCM)."""
    ref = np.clip(spec, -1.0, 1.0) if clip else spec
    n = min(got.size, ref.size)
    assert n > 0 and abs(got.size - ref.size) <= 2 * 2048
    err = float(np.abs(got[:n].astype(np.float64) - ref[:n]).max())
    assert err <= 1e-6 * float(np.abs(spec).max()), err


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fpw", [2, 4])
def test_switch_pattern_positions(fpw):
    """The pattern holds what the GPU tests rely on: at FPW = fpw, a long->short and a short->long switch at every offset inside a
    group, on the boundary from an odd-index group to the even-index group behind it and the reverse, isolated shorts, runs of 2..5
    shorts, a short first and last block; the truncated streams leave last groups of 3, 2 and 1 frames."""
    k = _KINDS
    for to_short in (True, False):
        at = switches(k[:N0 - 3], to_short)  # (inside the shortest truncation)
        assert {i % fpw for i in at} == set(range(fpw)), (fpw, to_short, at)
        # group g = i // fpw starts here; i % (2 fpw) == 0: g even (second launch), g - 1 odd; == fpw: g odd, g - 1 even
        assert any(i % (2 * fpw) == 0 for i in at) and any(i % (2 * fpw) == fpw for i in at), (fpw, to_short, at)
    runs = short_runs(k)
    assert set(runs) >= {1, 2, 3, 4, 5}, runs
    assert not k[0] and not k[-1] and k[1:].any()
    assert {(N0 - d) % 4 for d in (1, 2, 3)} == {3, 2, 1} and N0 % 4 == 0
    assert {(N0 - d) % 2 for d in (1, 2, 3)} == {0, 1}


def test_trim_streams_end_where_intended():
    """The trimmed streams' last frame: valid = 704 (a multiple of 64) and 691 (not), the granule lowered, the EOS flag set."""
    import nvorbis_amd as nv
    for name, want in (("stereo_trim_64", 704), ("stereo_trim_odd", 691), ("mono_trim_odd", 691)):
        pk, gr, fl = stream(name)
        st = nv.Stream(None, pk[0], pk[1], pk[2])
        try:
            for i in range(3, len(pk)):
                st.push_packet(pk[i], gr[i], fl[i])
            st.push_end()
            geo = st.pending_geometry()
        finally:
            st.close()
        last = geo[geo[:, 0] != 0][-1]
        assert last[0] == 2048 and last[2] == want, (name, last.tolist())


@pytest.mark.parametrize("name", SPEC_STREAMS)
def test_streams_oracle_against_spec(oracle, name):
    """Oracle against the spec-derived decoder on exactly the streams the GPU tests decode (clip off, 1e-6 of the peak)."""
    ref = oracle_pcm(oracle, name, False)
    spec = spec_pcm(name)
    assert float(np.abs(spec).max()) > 1.0  # the structured encoder's streams are loud: clip matters
    # (the oracle drains the last block's tail when the packets run out, StreamDecoder.cs:352-356; the spec stops before it)
    assert 0 <= ref.size - spec.size <= 2 * 1024, (ref.size, spec.size)
    _spec_close(ref, spec, False)


def test_equal_blocks_oracle_against_spec(oracle):
    ref = oracle_pcm(oracle, "equal_switches", False)
    spec = spec_pcm("equal_switches")
    assert 0 <= ref.size - spec.size <= 2 * 512, (ref.size, spec.size)
    _spec_close(ref, spec, False)


# The fall-back window at NVH_FPW=4 for stereo n = 2048 (nvh_launch.hip: slab_lds_bytes / slab_size_ok; C = the synthesis
# constants, synth_const_vecs * 16 bytes = 1 KB of dB table + the lattice and value pools; S = the slab area, the largest slab
# rounded up to 64 bytes): four frames need C + 4 S + 4 x 8 KB of spectra + 288 B <= 159 KB, one frame C + S + 8 KB + 512 B
# <= 64 KB.  So a group of four does not fit and one frame does for 32440 - C / 4 < S <= 56832 - C bytes.
def fallback_window(const_bytes):
    return 32440 - const_bytes / 4.0, 56832 - const_bytes


def test_deep_slabs_land_in_the_fpw4_fallback_window():
    """deep_slab_headers' full-depth frames: the largest slab lies inside the window with a margin of 4 KB on both sides."""
    import nvorbis_amd as nv
    pk, gr, fl = encode("deep", np.ones(12, dtype=bool), 31)
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for i in range(3, len(pk)):
            st.push_packet(pk[i], gr[i], fl[i])
        words, first = st.pending_slabs()
        lat = st.lattice_pool()
    finally:
        st.close()
    sizes = np.diff(first.astype(np.int64)) * 16
    # the constants block: the dB table (256 words), the lattice pool and the value pool; the lattice pool alone is a lower bound
    # of its size, 4 KB an upper one for this setup's books (nine dim-2 books of <= 21 values, a value pool of 21 + 1 words each)
    c_lo, c_hi = (256 + lat.size) * 4, (256 + lat.size + 9 * 22) * 4 + 16
    lo, hi = fallback_window(c_lo)[0], fallback_window(c_hi)[1]
    s = int(sizes.max() + 63) // 64 * 64
    assert lo + 4096 < s < hi - 4096, (sizes.tolist(), lo, hi)
    assert sizes.min() > lo + 4096


def test_fallback_never_fires_at_two_frames_per_workgroup():
    """At FPW = 2 the fall-back cannot fire: a group of two needs C + 2 S + ch * n words of walk map (the transforms' map is
    smaller), and whenever one frame fits k_synth's 64 KB -- C + S + ch * n / 2 + n / 16 <= 16384 words -- twice that is
    2 C + 2 S + ch * n + n / 8 <= 32768 words, below the group's 159 KB (40704 words, less its 40-word table)."""
    for ch in (1, 2):
        for n in (256, 512, 1024, 2048):
            for c in range(256, 16384, 64):
                s_max = 16384 - c - ch * n // 2 - n // 16
                if s_max < 0:
                    continue
                walk = c + 2 * (s_max + ch * n // 2)
                xform = ch * n // 2 + 2 * ch * (n // 2 + n // 16)
                assert max(walk, xform) + 8 * 5 <= 40704, (ch, n, c)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

def _assert_same(got, ref, what):
    assert got.size == ref.size, (what, got.size, ref.size)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (what, float(np.abs(got - ref).max()))


def _decode(nv, ctx, pk, gr, fl, clip, batch_frames, gpu_parse=False):
    dec = nv.StreamDecoder(ctx, pk, gr, fl, batch_frames=batch_frames, gpu_parse=gpu_parse)
    dec.ClipSamples = clip
    buf = np.zeros((1 << 20) - (1 << 20) % dec.Channels, np.float32)
    chunks = []
    while True:
        n = dec.Read(buf, 0, buf.size)
        if n == 0:
            break
        chunks.append(buf[:n].copy())
    dec.close()
    return np.concatenate(chunks) if chunks else np.zeros(0, np.float32)


def _batches(nv, ctx, pk, gr, fl, bounds, clip=True, gpu_parse=False):
    """The Stream path, batch by batch: frames [bounds[k], bounds[k + 1]) pushed, then synth_host.  Returns (PCM, [(frames,
    last decoded frame, synthesis-slot name)])."""
    st = nv.Stream(ctx, pk[0], pk[1], pk[2])
    st.set_clip(clip)
    if gpu_parse:
        st.set_gpu_parse(True)
    nfr = len(pk) - 3
    out, info = [], []
    try:
        for a, b in zip(bounds[:-1], bounds[1:]):
            for j in range(a, b):
                st.push_packet(pk[3 + j], gr[3 + j], fl[3 + j])
            if b >= nfr:
                st.push_end()
            fr = st.pending()[0]
            if fr == 0:
                continue
            geo = st.pending_geometry()
            dec = np.nonzero(geo[:, 0])[0]
            out.append(st.synth_host().copy())
            info.append((fr, int(dec[-1]) if dec.size else -1, st.kernels()[1]))
    finally:
        st.close()
    return (np.concatenate(out) if out else np.zeros(0, np.float32)), info


def _note(info):
    """Record what the bit-exact comparison just made saw; under NVH_FPW = f no batch may name the other groups' kernel."""
    f = _fpw()
    for fr, last, name in info:
        _SEEN.add(name)
        if name == EMIT_NAME[1] and last >= 0 and last % 2 == 1:
            _TAIL[0] += 1
        if f == 4:
            assert name != "k_synth_group2", info
        if f == 2:
            assert name != "k_synth_group4", info
        if f == 1:
            assert name not in ("k_synth_group2", "k_synth_group4"), info


def _bounds(nfr, bf):
    return list(range(0, nfr, bf)) + [nfr]



@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STREAMS))
def test_streams_bit_exact(oracle, gpu_ctx, name):
    """Every stream through the StreamDecoder at batch sizes 1 .. 1024, clip on and off, the host parser and (at 7 and 1024 frames)
    the GPU parser: bit-exact against the oracle and within 1e-6 of the peak of the spec decode."""
    import nvorbis_amd as nv
    pk, gr, fl = stream(name)
    spec = spec_pcm(name) if name in SPEC_STREAMS else None
    for clip in (True, False):
        ref = oracle_pcm(oracle, name, clip)
        if spec is not None:
            _spec_close(ref, spec, clip)
        for bf in (1, 2, 3, 4, 5, 7, 8, 13, 64, 1024):
            _assert_same(_decode(nv, gpu_ctx, pk, gr, fl, clip, bf), ref, (name, clip, bf))
        for bf in (7, 1024):
            _assert_same(_decode(nv, gpu_ctx, pk, gr, fl, clip, bf, gpu_parse=True), ref, (name, clip, bf, "gpu_parse"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stereo_switches", "mono_switches", "equal_switches", "stereo_last_group_3", "stereo_last_group_2",
                                  "stereo_last_group_1", "stereo_switches_silent"])
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_stream_batches_bit_exact(oracle, gpu_ctx, name, gpu_parse):
    """The Stream path batch by batch at every batch size, and with batch boundaries placed on every long->short switch (the batch
    ends on a long block followed by a short one), on every short->long switch, and one frame behind each: bit-exact against
    the oracle, each batch's synthesis slot the variant the rules promise (a batch of >= 8 frames of a stream without silence or
    trim has every frame pairable but its first: frame groups emit through switches at FPW 2 and 4)."""
    import nvorbis_amd as nv
    pk, gr, fl = stream(name)
    nfr = len(pk) - 3
    kinds = STREAMS[name][1]
    ref = oracle_pcm(oracle, name, True)
    ls, sl = switches(kinds, True), switches(kinds, False)
    layouts = [("bf%d" % bf, _bounds(nfr, bf)) for bf in (1, 2, 3, 4, 5, 7, 8, 13, 64, 1024)]
    layouts += [("at_long_short", [0] + ls + [nfr]), ("at_short_long", [0] + sl + [nfr]),
                ("behind_switch", sorted(set([0] + [i + 1 for i in ls + sl if i + 1 < nfr] + [nfr])))]
    names_ok = _names_checked() and not gpu_parse and STREAMS[name][3] is None
    for what, bounds in layouts:
        got, info = _batches(nv, gpu_ctx, pk, gr, fl, bounds, gpu_parse=gpu_parse)
        _assert_same(got, ref, (name, what, gpu_parse))
        _note(info)
        if names_ok and _fpw() > 1:
            for k, (fr, last, kname) in enumerate(info[:-1]):  # (the last batch holds the end of the stream)
                if fr >= 8:
                    assert kname == EMIT_NAME[_fpw()], (name, what, k, fr, kname)


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_all_long_batches_name_the_fpw_variant(oracle, gpu_ctx, gpu_parse):
    """Batches of >= 8 all-long, non-silent frames take the FPW's emitting variant; at FPW = 1 the batches of an even frame count
    end on an odd frame (k_synth_tail carries the tail out) and those of an odd count on an even one (k_synth)."""
    import nvorbis_amd as nv
    kinds = np.ones(200, dtype=bool)
    pk, gr, fl = encode("stereo", kinds, 41)
    ref = oracle.decode_packets(pk, gr, fl)[0]
    bounds = [0]
    for bf in (8, 9, 16, 17, 32, 33, 13, 12):
        bounds.append(bounds[-1] + bf)
    bounds.append(200)
    got, info = _batches(nv, gpu_ctx, pk, gr, fl, bounds, gpu_parse=gpu_parse)
    _assert_same(got, ref, ("all_long", gpu_parse))
    _note(info)
    assert [fr for fr, _, _ in info][:8] == [8, 9, 16, 17, 32, 33, 13, 12]
    assert all(last == fr - 1 for fr, last, _ in info[:8])
    if _names_checked() and not gpu_parse:
        for fr, last, kname in info[:8]:
            if fr >= 8:
                assert kname == EMIT_NAME[_fpw()], info
        if _fpw() == 1:
            assert {last % 2 for fr, last, _ in info[:8]} == {0, 1}


@pytest.mark.gpu
def test_seven_eighths_threshold_alternates_variants(oracle, gpu_ctx):
    """One stream, consecutive batches of 32 long frames whose emitting fraction sits at 28/32 = 7/8 (two silent frames: each
    takes itself and the frame behind it out of the steady state) and just below it, 27/32 (three, the last at the batch's end): the batches
    alternate between the emitting variant and k_synth + k_ola_compact, and the carried tail passes between them.  (The stream's
    first frame emits nothing: the first batch has one silent frame.  A silent last frame of a batch takes only itself out: 27/32.)"""
    import nvorbis_amd as nv
    nb, bf = 8, 32
    silent = {}
    for b in range(nb):
        offs = ((5,) if b == 0 else (5, 17)) if b % 2 == 0 else (4, 13, 31)
        for o in offs:
            silent[b * bf + o] = {0, 1}
    kinds = np.ones(nb * bf, dtype=bool)
    pk, gr, fl = encode("stereo", kinds, 42, silent)
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        got, info = _batches(nv, gpu_ctx, pk, gr, fl, _bounds(nb * bf, bf), clip=clip)
        _assert_same(got, ref, ("threshold", clip))
        _note(info)
        if _names_checked():
            names = [kname for _, _, kname in info]
            want = [EMIT_NAME[_fpw()] if b % 2 == 0 else "k_synth" for b in range(nb)]
            assert names == want, names


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_fallback_to_one_frame_per_workgroup(oracle, gpu_ctx, gpu_parse):
    """deep_slab_headers (~40 KB slabs): at NVH_FPW=4 a group of four frames does not fit the CU's LDS and the batch goes to one
    frame per workgroup (nvh_launch.hip: the host parser's re-layout, or the GPU parser's worst case) -- k_synth + k_synth_emit,
    bit-exact; at FPW 2 the group of two fits."""
    import nvorbis_amd as nv
    kinds = np.ones(40, dtype=bool)
    kinds[21:23] = False
    pk, gr, fl = encode("deep", kinds, 43)
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        got, info = _batches(nv, gpu_ctx, pk, gr, fl, [0, 16, 40], clip=clip, gpu_parse=gpu_parse)
        _assert_same(got, ref, ("deep", clip, gpu_parse))
        _note(info)
        _assert_same(_decode(nv, gpu_ctx, pk, gr, fl, clip, 1024, gpu_parse=gpu_parse), ref, ("deep", clip, gpu_parse, 1024))
        if _names_checked():
            assert info[0][2] == (EMIT_NAME[1] if _fpw() in (1, 4) else EMIT_NAME[2]), info


@pytest.mark.gpu
def test_float_variants_reached(tmp_path_factory):
    """(Last in this file.)  This file's GPU tests replayed under NVH_FPW=1 and NVH_FPW=4 in child processes; with this process's
    own (NVH_FPW=2 by default) the batches that were compared bit-exact must have named k_synth_group2, k_synth_group4 and
    k_synth + k_synth_emit, and some FPW = 1 batch with paired emission must have ended on an odd frame (k_synth_tail)."""
    if os.environ.get("NVH_TEST_CHILD"):
        out = os.environ.get("NVH_FG_SEEN")
        if out:
            with open(out, "w") as fh:
                json.dump({"seen": sorted(_SEEN), "tail": _TAIL[0]}, fh)
        pytest.skip("inside a replay: the parent checks the union")
    from tests.replay import run_children
    d = tmp_path_factory.mktemp("fg_seen")
    children, files = [], []
    for k, fpw in enumerate(("1", "4")):
        env = dict(os.environ)
        env["NVH_FPW"] = fpw
        env["NVH_TEST_CHILD"] = "1"
        env["NVH_FG_SEEN"] = str(d / ("%d.json" % k))
        files.append(env["NVH_FG_SEEN"])
        children.append((["test_frame_groups.py"], env, []))
    run_children(children, timeout=1500)
    seen, tail = set(_SEEN), _TAIL[0]
    for f in files:
        r = json.load(open(f))
        seen |= set(r["seen"])
        tail += r["tail"]
    missing = sorted({"k_synth_group2", "k_synth_group4", "k_synth+k_synth_emit"} - seen)
    assert not missing, "no bit-exact comparison reached %s (seen: %s)" % (missing, sorted(seen))
    assert tail > 0, "no FPW = 1 batch with paired emission ended on an odd frame (k_synth_tail)"

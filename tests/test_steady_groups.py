"""Steady frame groups (kernels_synth.hip: synth_group_steady; nvh_format.h: nvh_steady_pair): a group of two long stereo blocks
between neighbours of the same size takes a lean body, every other group the general one.  The predicate exists once and is
evaluated by the kernel on the two slab headers and by the host at upload (nvh_batch_steady_groups: the counter these tests read).

CPU: the count on 3test.ogg's first nine long/long packets and on hand-made header rows, each of which breaks exactly one clause of
the predicate.  GPU: uint32-exact against the oracle on streams that mix steady and general groups in the same two launches, on
chains of one, two and more cascade stages, on the 1024-sample instantiation, on every PCM twin, and with NVH_NO_STEADY=1.

The GPU parser writes the entry form of the slabs, which the steady body does not take (nor does the two-frame walk): its batches
count no steady group and stay exact through the general body."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import vorbis_encode as ve
from tests.test_frame_groups import _assert_same, _shipped, encode, headers
from tests.test_pcm_mix import mix_rule, same_bits
from tests.test_pcm_s16 import to_s16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_TOGGLED = any(os.environ.get(t) for t in ("NVH_NO_STEADY", "NVH_NO_WALK_TWO", "NVH_FPW", "NVH_NO_EMIT", "NVH_NO_SLAB", "NVH_GPU_PARSE",
                                           "NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_EMIT_ALWAYS"))
T7 = {}  # measured run time of each GPU test (printed by the last test)

# NvhSlabHdr (nvh_format.h) as sixteen words
F_FAULT, F_SLOT, F_FUSE, F_SELF, F_NEXT = 8, 16, 32, 64, 128
X_DONE, X_SELF_CARRY, X_CARRY_OUT = 0x20, 0x40, 0x80


def geo(prev_n, next_n, start, valid):
    return (prev_n >> 6) | ((next_n >> 6) << 8) | ((start >> 6) << 16) | ((valid >> 6) << 24)


def header(n, first, imp, **kw):
    """A steady frame's header: frame `first` (0) or second (1) of a group of the second launch (imp) or the first."""
    ef = (F_NEXT | (F_SELF if imp else 0)) if first else (F_SELF | (F_NEXT if imp else 0))
    nxt = n if ef & F_NEXT else 0
    f = dict(blk=n, xm=3 | X_DONE, flags=1 | F_SLOT | F_FUSE | ef, nheads=56, lpc=4, rgeom=2 | 8 | (2 << 4), group=8,
             md0=1, md1=1, geo=geo(n, nxt, 0, n >> 1))
    f.update(kw)
    h = np.zeros(16, np.uint32)
    h[0] = f["blk"] | (f["xm"] << 16) | (f["flags"] << 24)
    h[1] = f["nheads"] | (100 << 16)
    h[2] = 20 | (24 << 16)
    h[3] = 60 | (200 << 16)
    h[4] = f["lpc"] | (f["rgeom"] << 16) | (f["group"] << 24)
    h[5] = (1 << 30) + 1
    h[8] = f["md0"] | (3 << 8) | (4 << 16)
    h[9] = f["md1"] | (3 << 8) | (12 << 16)
    h[13] = f["geo"]
    return h


def count(rows, channels=2, block1=2048):
    import ctypes as C
    import nvorbis_amd as nv
    from nvorbis_amd import native
    hdr = np.ascontiguousarray(np.concatenate(rows).astype(np.uint32))
    n = C.c_int(-1)
    native.check(nv.lib().nvh_steady_count(hdr.ctypes.data, len(rows), channels, block1, C.byref(n)), "nvh_steady_count")
    return n.value


def pair(n, imp, k=None, **kw):
    """A steady pair with frame k's fields changed."""
    a, b = header(n, True, imp, **(kw if k == 0 else {})), header(n, False, imp, **(kw if k == 1 else {}))
    return [a, b]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_hand_made_rows_one_broken_clause_each():
    if os.environ.get("NVH_NO_STEADY") or os.environ.get("NVH_NO_WALK_TWO"):
        pytest.skip("the switch under test elsewhere")
    for n in (2048, 1024):
        for imp in (False, True):
            assert count(pair(n, imp), block1=n) == 1, (n, imp)
            assert count(pair(n, imp) + pair(n, not imp) + [header(n, True, imp)], block1=n) == 2  # (an odd frame is no group)
            broken = {
                "other block size": dict(blk=n >> 1),
                "one channel executes": dict(xm=1 | X_DONE),
                "self carry": dict(xm=3 | X_DONE | X_SELF_CARRY),
                "carry out": dict(xm=3 | X_DONE | X_CARRY_OUT),
                "k_ola_compact emits it": dict(xm=3),
                "floor not fused": None, "floor fault": None, "coupling pass": None,  # (the frame's own flags byte, below)
                "entry form": dict(rgeom=2 | (2 << 4)),
                "residue 1": dict(rgeom=1 | 8 | (2 << 4)),
                "two components per lane": dict(group=2),
                "no chain": dict(nheads=0),
                "floor 0 unused": dict(md0=2),
                "floor 1 unused": dict(md1=2),
                "floor 1 none": dict(md1=0),
                "short predecessor": None, "start": None, "valid": None,  # (with the frame's own successor field, below)
            }
            for what, kw in broken.items():
                for k in (0, 1):
                    if what in ("floor not fused", "floor fault", "coupling pass"):  # (the flags byte of that frame)
                        base = int(header(n, k == 0, imp)[0] >> 24)
                        kw = dict(flags={"floor not fused": base & ~F_FUSE, "floor fault": base | F_FAULT, "coupling pass": base | 4}[what])
                    if what in ("short predecessor", "start", "valid"):
                        nxt = n if (int(header(n, k == 0, imp)[0] >> 24) & F_NEXT) else 0
                        kw = dict(geo={"short predecessor": geo(256, nxt, 0, n >> 1), "start": geo(n, nxt, 64, n >> 1),
                                       "valid": geo(n, nxt, 0, (n >> 1) + 64)}[what])
                    assert count(pair(n, imp, k, **kw), block1=n) == 0, (n, imp, what, k)
            # a short successor, where one is named
            assert count(pair(n, imp, 0, geo=geo(n, 256, 0, n >> 1)), block1=n) == 0
            if imp:
                assert count(pair(n, imp, 1, geo=geo(n, 256, 0, n >> 1)), block1=n) == 0
            # emission flags that are not the position's: an inner overlap nobody emits, outer overlaps on one side only
            fl0, fl1 = int(header(n, True, imp)[0] >> 24), int(header(n, False, imp)[0] >> 24)
            assert count(pair(n, imp, 0, flags=fl0 & ~F_NEXT), block1=n) == 0
            assert count(pair(n, imp, 1, flags=fl1 & ~F_SELF), block1=n) == 0
            assert count(pair(n, imp, 0, flags=fl0 ^ F_SELF), block1=n) == 0
            assert count(pair(n, imp, 1, flags=fl1 ^ F_NEXT), block1=n) == 0
            # the launch's arguments: mono, a larger block1 (the group's blocks are then the short ones), sizes without a twin
            assert count(pair(n, imp), channels=1, block1=n) == 0
            assert count(pair(n, imp), block1=2 * n) == 0
    assert count(pair(512, True), block1=512) == 0 and count(pair(4096, True), block1=4096) == 0


def _ll(nv, k):
    import bench
    hdr, ll, ch = bench.ll_packets(nv, os.path.join(GOLDEN, "3test.ogg"))
    assert ch == 2 and len(ll) >= k
    return list(hdr), ll[:k]


def test_host_count_3test_first_nine_long_packets():
    """Nine n = 2048 frames in one batch, the first at the stream's start (it emits nothing): groups (2, 3), (4, 5), (6, 7) are
    steady; (0, 1) begins the stream, frame 8 is alone and writes the carried tail."""
    import nvorbis_amd as nv
    hdr, ll = _ll(nv, 9)
    st = nv.Stream(None, hdr[0], hdr[1], hdr[2])
    try:
        for p in ll:
            st.push_packet(p, -1, 0)
        assert st.pending()[0] == 9
        got = st.pending_steady()
    finally:
        st.close()
    if os.environ.get("NVH_NO_STEADY") or os.environ.get("NVH_NO_WALK_TWO") or os.environ.get("NVH_FPW", "2") != "2" or os.environ.get("NVH_NO_EMIT"):
        assert got == 0
    else:
        assert got == 3


def _chains(words, first, f):
    """Cascade stages of every chain of frame f's slab (heads -> records, `more` in bit 31 of a record's second word)."""
    w = words[int(first[f]) * 4:int(first[f + 1]) * 4]
    nheads, off_heads, off_rec = int(w[1] & 0xFFFF), int(w[2] & 0xFFFF), int(w[2] >> 16)
    out = []
    for k in range(nheads):
        o, d = int(w[off_heads * 4 + k] & 0xFFFF), 1
        while w[off_rec * 4 + 2 * o + 1] >> 31:
            o, d = o + 1, d + 1
        out.append(d)
    return out, int(w[4] & 0xFFFF)


@functools.lru_cache(maxsize=None)
def deep_stream():
    return encode("stereo", np.ones(9, dtype=bool), 51)


def test_full_depth_frames_have_the_chains_the_walk_tests_need():
    """The structured encoder's long frames: chains of one, two and three or more stages inside one wavefront's 64 lanes, and
    lanes behind the last chain (fewer than 256 lane groups)."""
    import nvorbis_amd as nv
    pk, gr, fl = deep_stream()
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for i in range(3, len(pk)):
            st.push_packet(pk[i], gr[i], fl[i])
        words, first = st.pending_slabs()
    finally:
        st.close()
    seen = False
    for f in (5, 6):  # batch frames (4, 5) of the GPU test below, a steady group
        depth, lpc = _chains(words, first, f)
        lanes = np.repeat(depth, lpc)
        assert lanes.size < 256, lanes.size
        for w0 in range(0, lanes.size, 64):
            d = set(lanes[w0:w0 + 64].tolist())
            seen = seen or (1 in d and 2 in d and max(d) >= 3)
    assert seen


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

def _run(nv, ctx, pk, gr, fl, bounds, clip=True, gpu_parse=False, **synth):
    """Frames [bounds[k], bounds[k + 1]) per batch through the Stream path: ([PCM per batch], [steady groups per batch],
    [host count of the pending frames per batch, host parser only], [synthesis slot names], HasClipped)."""
    st = nv.Stream(ctx, pk[0], pk[1], pk[2])
    st.set_clip(clip)
    if gpu_parse:
        st.set_gpu_parse(True)
    nfr = len(pk) - 3
    out, steady, pending, names = [], [], [], []
    try:
        for a, b in zip(bounds[:-1], bounds[1:]):
            for j in range(a, b):
                st.push_packet(pk[3 + j], gr[3 + j], fl[3 + j])
            if b >= nfr:
                st.push_end()
            pending.append(None if gpu_parse else st.pending_steady())
            out.append(st.synth_host(**synth).copy())
            steady.append(st.steady_groups())
            names.append(st.kernels()[1])
        clipped = st.has_clipped()
    finally:
        st.close()
    return out, steady, pending, names, clipped


def _timed(name, t0):
    T7[name] = T7.get(name, 0.0) + time.time() - t0


def _want(steady):
    return [0] * len(steady) if _TOGGLED else steady


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_nine_frames_3test(oracle, gpu_ctx, gpu_parse):
    """Nine stereo n = 2048 frames behind the stream's first: a first group over the carried tail, three steady groups (one of the
    first launch between two of the second), a last frame alone that writes the tail."""
    import nvorbis_amd as nv
    t0 = time.time()
    hdr, ll = _ll(nv, 10)
    pk, gr, fl = hdr + ll, [-1] * 13, [0] * 13
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        out, steady, pending, names, _ = _run(nv, gpu_ctx, pk, gr, fl, [0, 1, 10], clip=clip, gpu_parse=gpu_parse)
        _assert_same(np.concatenate(out), ref, ("3test", clip, gpu_parse))
        if gpu_parse:
            assert steady == [0, 0]
        else:
            assert steady == pending == _want([0, 3]), (steady, pending)
            if not _TOGGLED:
                assert names[1] == "k_synth_group2"
    _timed("nine_frames_3test[%s]" % gpu_parse, t0)


@pytest.mark.gpu
def test_full_depth_chains(oracle, gpu_ctx):
    """Eight full-depth frames behind the stream's first (six leave one steady group, whose wavefronts see two of the three chain
    depths each; of eight, the second steady group has all three in one): the peeled stage, the ballot loop and its masks."""
    import nvorbis_amd as nv
    t0 = time.time()
    pk, gr, fl = deep_stream()
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        out, steady, pending, _, _ = _run(nv, gpu_ctx, pk, gr, fl, [0, 1, 9], clip=clip)
        _assert_same(np.concatenate(out), ref, ("deep", clip))
        assert steady == pending == _want([0, 2]), (steady, pending)
    _timed("full_depth_chains", t0)


@pytest.mark.gpu
def test_steady_and_general_groups_trade_quarters(oracle, gpu_ctx):
    """L | L L | L S | S L | L L | L L | L at 2048 / 256 behind the stream's first frame: steady groups of both launches next to
    general ones, the quarters between them through the planes in both directions."""
    import nvorbis_amd as nv
    t0 = time.time()
    kinds = np.array([1] + [1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1], dtype=bool)
    pk, gr, fl = encode("stereo", kinds, 52)
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        out, steady, pending, _, _ = _run(nv, gpu_ctx, pk, gr, fl, [0, 1, len(kinds)], clip=clip)
        _assert_same(np.concatenate(out), ref, ("switches", clip))
        # batch frames 0..12: (0, 1) carried tail, (2, 3) steady, (4, 5) = L S, (6, 7) = S L, (8, 9) and (10, 11) steady, 12 last
        assert steady == pending == _want([0, 3]), (steady, pending)
    _timed("steady_and_general", t0)


@pytest.mark.gpu
@pytest.mark.parametrize("silent", [{0, 1}, {0}])
def test_steady_looking_groups_that_are_not(oracle, gpu_ctx, silent):
    """A silent frame ({0, 1}: no channel executes) and an unused floor on one channel of a coupled pair ({0}) inside what would be
    the steady group (2, 3) of the batch: that group takes the general body."""
    import nvorbis_amd as nv
    t0 = time.time()
    kinds = np.ones(10, dtype=bool)
    pk, gr, fl = encode("stereo", kinds, 53, {4: silent})  # batch frame 3
    base = encode("stereo", kinds, 53)
    ref = oracle.decode_packets(pk, gr, fl, clip=True)[0]
    out, steady, pending, _, _ = _run(nv, gpu_ctx, pk, gr, fl, [0, 1, 10])
    _assert_same(np.concatenate(out), ref, ("silent", sorted(silent)))
    _, steady0, _, _, _ = _run(nv, gpu_ctx, base[0], base[1], base[2], [0, 1, 10])
    assert steady == pending and steady0 == _want([0, 3]), (steady, steady0)
    assert steady[1] < steady0[1] or _TOGGLED, (steady, steady0)
    _timed("not_steady[%s]" % sorted(silent), t0)


@functools.lru_cache(maxsize=None)
def _headers_1024():
    return tuple(ve.c4_headers(_shipped("3test"), psize=48, channels=2, block0=256, block1=1024, end_per_channel=384))


@pytest.mark.gpu
def test_block_1024_instantiation(oracle, gpu_ctx):
    """A 256 / 1024 setup, nine long frames behind the stream's first: the n = 1024 body.  (Nine, not five: the stream's last frame
    drains its tail and is left to k_ola_compact, and a batch emits in frame groups only when 7/8 of its frames do.)"""
    import nvorbis_amd as nv
    t0 = time.time()
    hdr = list(_headers_1024())
    S = ve.setup_of(hdr)
    rng = np.random.default_rng(54)
    enc = ve.PacketEncoder(S)
    long_mode = next(i for i, (f, _) in enumerate(S.modes) if f)
    pk = hdr + [enc.packet(rng, long_mode, 1, 1) for _ in range(10)]
    gr, fl = [-1, -1, -1] + ve.granules_for(S, [True] * 10), [0] * 13
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        out, steady, pending, _, _ = _run(nv, gpu_ctx, pk, gr, fl, [0, 1, 10], clip=clip)
        _assert_same(np.concatenate(out), ref, ("1024", clip))
        assert steady == pending == _want([0, 3]), (steady, pending)
    _timed("block_1024", t0)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [True, False])
def test_every_pcm_twin(oracle, gpu_ctx, clip):
    """float, s16, planar, planar s16, mono and mono s16 on the nine-frame stream (made loud, so that clipping happens)."""
    import nvorbis_amd as nv
    t0 = time.time()
    pk, gr, fl = encode("stereo", np.ones(10, dtype=bool), 55)  # full-depth packets: louder than 1.0
    ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
    raw = oracle.decode_packets(pk, gr, fl, clip=False)[0]
    assert float(np.abs(raw).max()) > 1.0
    for dt in (np.float32, np.int16):
        conv = to_s16 if dt == np.int16 else (lambda x: x)
        out, steady, _, _, hc = _run(nv, gpu_ctx, pk, gr, fl, [0, 1, 10], clip=clip, dtype=dt)
        assert same_bits(np.concatenate(out), conv(ref)), ("interleaved", dt)
        assert steady == _want([0, 3]) and hc == clip  # (HasClipped is the clip's by-product: nothing is looked at with it off)
        out, steady, _, _, hc = _run(nv, gpu_ctx, pk, gr, fl, [0, 1, 10], clip=clip, dtype=dt, planar=True)
        assert same_bits(np.concatenate(out, axis=1), np.ascontiguousarray(conv(ref).reshape(-1, 2).T)), ("planar", dt)
        assert steady == _want([0, 3]) and hc == clip  # (HasClipped is the clip's by-product: nothing is looked at with it off)
        want, wc = mix_rule(raw, 2, clip, dt)
        out, steady, _, _, hc = _run(nv, gpu_ctx, pk, gr, fl, [0, 1, 10], clip=clip, dtype=dt, mix="mono")
        assert same_bits(np.concatenate(out), want), ("mono", dt)
        assert steady == _want([0, 3]) and hc == (clip and wc)
    _timed("every_pcm_twin[%s]" % clip, t0)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import nvorbis_amd as nv
from tests.test_steady_groups import _run, _ll
hdr, ll = _ll(nv, 10)
pk = hdr + ll
ctx = nv.Context(0)
out, steady, pending, names, _ = _run(nv, ctx, pk, [-1] * 13, [0] * 13, [0, 1, 10])
ctx.close()
np.concatenate(out).tofile(sys.argv[1])
print("STEADY", steady, pending, names)
"""


@pytest.mark.gpu
def test_no_steady_switch_same_bytes(oracle, gpu_ctx, tmp_path):
    """A child process with NVH_NO_STEADY=1: no steady group is counted, the PCM bytes are those of this process."""
    import nvorbis_amd as nv
    if _TOGGLED:
        pytest.skip("a kernel toggle is set: the default run is not the steady one")
    t0 = time.time()
    hdr, ll = _ll(nv, 10)
    pk = hdr + ll
    out, steady, _, _, _ = _run(nv, gpu_ctx, pk, [-1] * 13, [0] * 13, [0, 1, 10])
    assert steady == [0, 3]
    env = dict(os.environ)
    env["NVH_NO_STEADY"] = "1"
    dst = str(tmp_path / "pcm.f32")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, dst], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "STEADY [0, 0] [0, 0]" in r.stdout, r.stdout
    assert np.array_equal(np.fromfile(dst, np.uint32), np.concatenate(out).view(np.uint32))
    _timed("no_steady_switch", t0)


@pytest.mark.gpu
def test_t7_run_times():
    """(Last.)  T7: the measured run time of each GPU test of this file, against the budget of a few seconds each."""
    for k, v in sorted(T7.items()):
        print("T7 %-40s %6.2f s" % (k, v))
    assert all(v < 10.0 for v in T7.values()), T7

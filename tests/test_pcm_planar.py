"""Channel-planar PCM (nvh_*_planar): channel c's samples at base + c * plane_stride, written by the emitting kernels' _planar
twins.  No tolerance anywhere: planar output equals the interleaved output of the same call sequence reshaped to (T, C) and
transposed, in both formats -- and so, for float, the oracle's PCM transposed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the 14 planar twins (as the launcher names them in the timing slots); every one must be reached by this file's runs
PLANAR_TWINS = ["k_synth+k_synth_emit_planar", "k_synth+k_synth_emit_s16_planar",
                "k_synth8+k_synth8_emit_planar", "k_synth8+k_synth8_emit_s16_planar",
                "k_synth_group2_planar", "k_synth_group2_s16_planar", "k_synth_group4_planar", "k_synth_group4_s16_planar",
                "k_ola_compact_planar", "k_ola_compact_s16_planar", "k_ola_emit_planar", "k_ola_emit_s16_planar",
                "k_ola_emit_seq_planar", "k_ola_emit_seq_s16_planar"]
_SEEN = set()  # twins this process ran
SENTINEL = {np.dtype(np.float32): np.float32(-1234.5), np.dtype(np.int16): np.int16(-7777)}


def planes_of(x, ch):
    """Interleaved PCM -> (ch, T) planes."""
    return np.ascontiguousarray(np.asarray(x).reshape(-1, ch).T)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_planar_entry_points():
    from nvorbis_amd import native
    L = native.lib()
    for name in ("nvh_stream_synth_planar", "nvh_stream_synth_begin_planar", "nvh_batch_synth_planar"):
        assert hasattr(L, name), name


def test_planar_entry_points_refuse_bad_arguments():
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    wr = C.c_int64(0)
    buf = np.zeros(1 << 16, np.float32)
    for fmt in (native.PCM_F32, native.PCM_S16):
        assert L.nvh_stream_synth_planar(None, fmt, buf.ctypes.data, None, 16, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_begin_planar(None, fmt, buf.ctypes.data, 16, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_batch_synth_planar(None, fmt, None, 16) == native.ERR_ARGUMENT
    pk, _, _ = nv.demux_ogg(open(os.path.join(GOLDEN, "3test.ogg"), "rb").read())
    st = nv.Stream(None, pk[0], pk[1], pk[2])  # host-only: the arguments are checked before anything needs a device
    try:
        for fmt in (2, -1, 7):
            assert L.nvh_stream_synth_planar(st._h, fmt, buf.ctypes.data, None, 16, C.byref(wr)) == native.ERR_ARGUMENT
            assert L.nvh_stream_synth_begin_planar(st._h, fmt, buf.ctypes.data, 16, C.byref(wr)) == native.ERR_ARGUMENT
        for i in range(3, 12):
            st.push_packet(pk[i], -1, 0)
        _, n = st.pending()
        assert n > 0
        for fmt in (native.PCM_F32, native.PCM_S16):
            # a plane stride below the pending samples per channel
            assert L.nvh_stream_synth_planar(st._h, fmt, buf.ctypes.data, None, n - 1, C.byref(wr)) == native.ERR_ARGUMENT
            assert L.nvh_stream_synth_begin_planar(st._h, fmt, buf.ctypes.data, n - 1, C.byref(wr)) == native.ERR_ARGUMENT
            # both destinations, or neither with PCM to write
            assert L.nvh_stream_synth_planar(st._h, fmt, buf.ctypes.data, buf.ctypes.data, n, C.byref(wr)) == native.ERR_ARGUMENT
            assert L.nvh_stream_synth_planar(st._h, fmt, None, None, n, C.byref(wr)) == native.ERR_ARGUMENT
        # a device base not aligned to its sample size
        assert L.nvh_stream_synth_planar(st._h, native.PCM_F32, None, C.c_void_p(4096 + 2), n, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_planar(st._h, native.PCM_S16, None, C.c_void_p(4096 + 1), n, C.byref(wr)) == native.ERR_ARGUMENT
        # the Python surface: out arrays of the wrong shape or dtype
        ch = st.channels
        for bad in (np.zeros((ch, n), np.int16), np.zeros(ch * n, np.float32), np.zeros((ch + 1, n), np.float32),
                    np.zeros((ch, n - 1), np.float32), np.zeros((n, ch), np.float32).T):
            with pytest.raises(ValueError):
                st.synth_host(out=bad, planar=True)
    finally:
        st.close()


def test_reader_and_decoder_reject_unknown_layouts():
    import nvorbis_amd as nv
    data = open(os.path.join(GOLDEN, "3test.ogg"), "rb").read()
    for bad in ("Planar", "channels_first", "", None, 1):
        with pytest.raises(ValueError):
            nv.VorbisReader(data, layout=bad)  # before a context is created
        with pytest.raises(ValueError):
            nv.StreamDecoder(None, [b"", b"", b""], layout=bad)


def test_corpus_planar_refusals():
    from nvorbis_amd import corpus
    with pytest.raises(ValueError):
        corpus.decode_files_to_device([], layout="rows")
    with pytest.raises(ValueError):
        corpus.transcode([b""], layout="planar")
    with pytest.raises(ValueError):
        corpus.gather_pcm({0: np.zeros((2, 4), np.float32)}, 1, 0, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

_OPEN = []  # streams a GPU test opened: closed behind every test, also when it failed (not at interpreter exit, behind the context)


@pytest.fixture(autouse=True)
def _close_streams():
    yield
    while _OPEN:
        x = _OPEN.pop()
        (x.free if hasattr(x, "free") else x.close)()  # (batches before their stream: last in, first out)


def _stream(nv, ctx, pk):
    st = nv.Stream(ctx, pk[0], pk[1], pk[2])
    _OPEN.append(st)
    return st


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _note(names):
    for k in names:
        if k.endswith("_planar"):
            _SEEN.add(k)


def _descriptor_toggle():
    return any(os.environ.get(t) for t in ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB"))


# device destinations: (extra samples of plane stride, base offset in samples); a batch takes them in turn
VARIANTS = [(0, 0), (4, 0), (1, 0), (0, 1)]


def _synth_planar_device(torch, st, dt, variant):
    """The pending batch of `st` into a sentinel-filled device buffer as planes (variant: stride extra, base offset): (ch, n)
    planes; asserts that nothing outside the planes was written."""
    extra, off = variant
    ch = st.channels
    _, n = st.pending()
    stride = n + extra
    size = off + ch * stride + 64
    tdt = torch.float32 if dt == np.float32 else torch.int16
    buf = torch.full((size,), float(SENTINEL[np.dtype(dt)]), dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    got = st.synth_device(buf.data_ptr() + off * np.dtype(dt).itemsize, 0, dtype=dt, plane_stride=stride)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    planes = np.stack([h[off + c * stride: off + c * stride + got] for c in range(ch)]) if ch else np.zeros((0, got), dt)
    keep = np.ones(size, bool)
    for c in range(ch):
        keep[off + c * stride: off + c * stride + got] = False
    assert (h[keep] == SENTINEL[np.dtype(dt)]).all(), ("written outside the planes", variant, n, got)
    return planes, got


def _lockstep_planar(nv, torch, ctx, pk, gr, fl, clip, batch_frames, dt, v0):
    """Two streams over the same packets, batch by batch: interleaved synth_host and planar synth_device (device destinations
    rotating through VARIANTS from v0).  Returns (interleaved PCM, planar PCM (ch, T), kernel names of the planar batches,
    has_clipped of each)."""
    si, sp = _stream(nv, ctx, pk), _stream(nv, ctx, pk)
    si.set_clip(clip)
    sp.set_clip(clip)
    ch = si.channels
    outi, outp, kern = [], [], []
    i, k = 3, v0
    while i < len(pk):
        for st in (si, sp):
            for j in range(i, min(i + batch_frames, len(pk))):
                st.push_packet(pk[j], gr[j], fl[j])
        i += batch_frames
        if i >= len(pk):
            si.push_end()
            sp.push_end()
        if si.pending()[0] == 0:
            continue
        a = si.synth_host(dtype=dt).copy()
        p, got = _synth_planar_device(torch, sp, dt, VARIANTS[k % len(VARIANTS)])
        k += 1
        assert got * ch == a.size
        ks = sp.kernels()
        kern.append(ks)
        _note(ks)
        outi.append(a)
        outp.append(p)
    hc = (si.has_clipped(), sp.has_clipped())
    si.close()
    sp.close()
    cat = np.concatenate(outi) if outi else np.zeros(0, dt)
    catp = np.concatenate(outp, axis=1) if outp else np.zeros((ch, 0), dt)
    return cat, catp, kern, hc


CONFIGS = ["mono_res0_small_blocks", "stereo_res1_coupled", "three_ch_res2_misaligned", "six_ch_res2_4096", "two_submaps",
           "equal_blocks_overrun", "mono_8192", "stereo_8192", "mono_res1_2048", "floor0_slab", "floor0_stereo",
           "res0_slab", "odd_dims_slab", "res2_alias_stereo", "two_pass_slab", "res0_3ch",
           "table_books_pair", "table_books_general", "table_books_b1", "ch4_res1", "ch5_res2", "ch7_res1", "ch8_res2",
           "ch9_res2", "ch16_res1_4096", "ch40_res1"]


def test_configs_match_the_s16_suite():
    from tests import test_pcm_s16
    assert CONFIGS == test_pcm_s16.CONFIGS


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
@pytest.mark.parametrize("consistent", [True, False])
def test_synthetic_configs_planar(oracle, gpu_ctx, name, consistent):
    """Every synthetic config of the parity suite, clip on and off, batches of 1024 and 13 frames, float and s16: the planar
    device output (plane stride n, n + 4, n + 1, a base one sample off) equals the interleaved output transposed, the float one
    the oracle's PCM transposed; nothing between or behind the planes is written; HasClipped agrees."""
    torch = _torch()
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 150, 11 + int(consistent), consistent_windows=consistent)
    exact_ref = not (name.startswith("floor0") and _descriptor_toggle())
    v0 = 0
    for clip in (True, False):
        ref, _ = oracle.decode_packets(pk, gr, fl, clip=clip)
        for bf in (1024, 13):
            for dt in (np.float32, np.int16):
                a, p, _, (hci, hcp) = _lockstep_planar(nv, torch, gpu_ctx, pk, gr, fl, clip, bf, dt, v0)
                v0 += 1
                ch = p.shape[0]
                assert p.dtype == np.dtype(dt) and p.size == a.size, (name, clip, bf, dt)
                assert np.array_equal(p, planes_of(a, ch)), (name, clip, bf, dt)
                if dt == np.float32 and exact_ref:
                    assert a.size == ref.size and np.array_equal(p.view(np.uint32), planes_of(ref, ch).view(np.uint32)), (name, clip, bf)
                assert hci == hcp, (name, clip, bf, dt)


def _ogg_reader_cases():
    return [(n, g) for n in ("1test", "2test", "3test", "issue6test") for g in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,gpu_parse", _ogg_reader_cases())
def test_reader_planar_files(gpu_ctx, ogg_bytes, name, gpu_parse):
    """VorbisReader(layout="planar") on the shipped files, both parsers, float and s16: read_all, odd-sized partial reads and
    reads after seeks (from the beginning and from the current position) equal the interleaved reader's output transposed."""
    import nvorbis_amd as nv
    data = ogg_bytes[name]
    opened = []

    def reader(**kw):
        r = nv.VorbisReader(data, ctx=gpu_ctx, gpu_parse=gpu_parse, **kw)
        opened.append(r)
        return r
    try:
        _reader_planar_files(reader, name)
    finally:
        for r in opened:
            r.close()


def _reader_planar_files(reader, name):
    for fmt, dt in (("f32", np.float32), ("s16", np.int16)):
        ri = reader(batch_frames=64, sample_format=fmt)
        rp = reader(batch_frames=64, sample_format=fmt, layout="planar")
        ch = ri.Channels
        with pytest.raises(ValueError):
            rp.ReadSamples(np.zeros(64 * ch, dt))  # interleaved-shaped buffer
        with pytest.raises(ValueError):
            rp.ReadSamples(np.zeros((ch + 1, 64), dt))
        with pytest.raises(TypeError):
            rp.ReadSamples(np.zeros((ch, 64), np.float64))
        full = ri.read_all()
        p = rp.read_all()
        assert p.shape == (ch, full.size // ch) and p.dtype == np.dtype(dt)
        assert np.array_equal(p, planes_of(full, ch)), (name, fmt)
        # odd-sized partial reads at odd offsets of the buffer
        rp = reader(batch_frames=7, sample_format=fmt, layout="planar")
        rng = np.random.default_rng(5)
        parts, buf = [], np.zeros((ch, 5000), dt)
        while True:
            off = int(rng.integers(0, 100))
            k = int(rng.integers(1, 4899))
            n = rp.ReadSamples(buf, off, k)
            if n <= 0:
                break
            parts.append(buf[:, off:off + n].copy())
        assert np.array_equal(np.concatenate(parts, axis=1), planes_of(full, ch)), (name, fmt)
        # seeks
        ri = reader(batch_frames=64, sample_format=fmt)
        rp = reader(batch_frames=64, sample_format=fmt, layout="planar")
        total = ri.TotalSamples

        def outcome(r, planar, t, origin):
            try:
                r.SeekTo(t, origin)
                if planar:
                    b = np.zeros((ch, 777), dt)
                    n = r.ReadSamples(b)
                    return "ok", b[:, :n].copy(), r.SamplePosition
                b = np.zeros(777 * ch, dt)
                n = r.ReadSamples(b)
                return "ok", planes_of(b[:n], ch), r.SamplePosition
            except Exception as e:
                return type(e).__name__, None, None
        for t, origin in [(0, "begin"), (1, "begin"), (1000, "begin"), (total // 3, "begin"), (300, "current"),
                          (max(total - 700, 0), "begin"), (-500, "current")]:
            ci, pi, posi = outcome(ri, False, t, origin)
            cp, pp, posp = outcome(rp, True, t, origin)
            assert cp == ci and posp == posi, (name, fmt, t, origin, ci, cp)
            if cp == "ok":
                assert np.array_equal(pp, pi), (name, fmt, t, origin)


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_pipelined_planar_alternating(gpu_ctx, ogg_bytes, gpu_parse):
    """synth_begin / synth_end with planar and interleaved flights, float and s16, alternating on one stream: every flight equals
    the blocking interleaved synth_host of the same batch on a second stream (transposed where planar)."""
    import nvorbis_amd as nv
    pk, _, _ = nv.demux_ogg(ogg_bytes["3test"])

    def streams():
        st = _stream(nv, gpu_ctx, pk)
        if gpu_parse:
            st.set_gpu_parse(True)
        return st
    plan = [(np.float32, True), (np.int16, False), (np.int16, True), (np.float32, False), (np.float32, True), (np.int16, True)]
    a, b = streams(), streams()
    ch = a.channels
    cuts = np.linspace(3, len(pk), len(plan) + 1).astype(int)
    want, got = [], []
    out = 0
    for k, (dt, planar) in enumerate(plan):
        for st in (a, b):
            for i in range(cuts[k], cuts[k + 1]):
                st.push_packet(pk[i], -1, 0)
        w = a.synth_host(dtype=dt).copy()
        want.append(planes_of(w, ch) if planar else w)
        exp = b.synth_begin(dtype=dt, planar=planar)
        assert exp == (w.size // ch if planar else w.size)
        out += 1
        if out == 2:
            got.append(b.synth_end().copy())
            out -= 1
    while out:
        got.append(b.synth_end().copy())
        out -= 1
    for k, (w, g) in enumerate(zip(want, got)):
        assert g.dtype == np.dtype(plan[k][0]) and g.shape == w.shape and np.array_equal(w, g), k
    # host destinations of the blocking call: a pageable (ch, m) array with m > n
    a.close()
    b.close()
    a, b = streams(), streams()
    for st in (a, b):
        for i in range(3, len(pk)):
            st.push_packet(pk[i], -1, 0)
        st.push_end()
    w = a.synth_host().copy()
    n = w.size // ch
    dst = np.full((ch, n + 5), SENTINEL[np.dtype(np.float32)], np.float32)
    p = b.synth_host(out=dst, planar=True)
    assert p.shape == (ch, n) and np.array_equal(p, planes_of(w, ch))
    assert (dst[:, n:] == SENTINEL[np.dtype(np.float32)]).all()
    _note(b.kernels())
    a.close()
    b.close()


@pytest.mark.gpu
def test_resident_batch_planar(gpu_ctx):
    """A resident Batch at the bench shape (4096 stereo n = 2048 frames), planar, launched repeatedly: identical results, equal to
    the interleaved batch transposed, in float and s16; the planes' gap and tail keep the sentinel."""
    torch = _torch()
    import bench
    import nvorbis_amd as nv
    from nvorbis_amd import native
    headers, ll, ch = bench.ll_packets(nv, os.path.join(GOLDEN, "3test.ogg"))
    st = _stream(nv, gpu_ctx, headers)
    st.push_packet(ll[0], -1, 0)
    assert st.synth_host().size == 0
    for i in range(4096):
        st.push_packet(ll[(1 + i) % len(ll)], -1, 0)
    b = st.upload_batch()
    _OPEN.append(b)
    n = b.samples
    for dt, tdt in ((np.float32, torch.float32), (np.int16, torch.int16)):
        pi = torch.zeros(n * ch, dtype=tdt, device="cuda")
        stride = n + 8
        pp = torch.full((ch * stride + 8,), float(SENTINEL[np.dtype(dt)]), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        b.synth(pi.data_ptr(), n * ch, dtype=dt)
        gpu_ctx.synchronize()
        want = planes_of(pi.cpu().numpy(), ch)
        first = None
        for rep in range(3):
            b.synth(pp.data_ptr(), 0, dtype=dt, plane_stride=stride)
            ks = b.kernels()
            _note(ks)
            assert any(k.endswith("_planar") for k in ks), ks
            gpu_ctx.synchronize()
            h = pp.cpu().numpy()
            got = np.stack([h[c * stride: c * stride + n] for c in range(ch)])
            assert np.array_equal(got, want), (dt, rep)
            gaps = np.concatenate([h[c * stride + n: (c + 1) * stride] for c in range(ch)] + [h[ch * stride:]])
            assert (gaps == SENTINEL[np.dtype(dt)]).all()
            if first is None:
                first = h.copy()
            assert np.array_equal(h, first)
        with pytest.raises(native.NvhError) as e:
            b.synth(pp.data_ptr(), 0, dtype=dt, plane_stride=n - 1)
        assert e.value.code == native.ERR_ARGUMENT
    b.free()
    st.close()


@pytest.mark.gpu
def test_throwing_packet_gpu_parse_planar(gpu_ctx):
    """GPU-parse mode with a throwing packet in the batch: the planar call writes the interleaved call's PCM transposed, up to the
    error, and reports the error at its position in samples per channel."""
    import nvorbis_amd as nv
    from nvorbis_amd import native
    from tests import synth_stream as ss
    cfg = ss.config("stereo_res1_coupled")
    old = cfg["books"][3]
    cfg["books"][3] = ss.IncompleteBook(old.bits, dims=old.dims, lookup=old.lookup, min_me=old.min_me, delta_me=old.delta_me,
                                        value_bits=old.value_bits, sequence_p=old.sequence_p, mults=old.mults)
    pk, gr, fl = ss.make_stream(cfg, 200, 1)
    for dt in (np.float32, np.int16):
        res = {}
        for planar in (False, True):
            st = _stream(nv, gpu_ctx, pk)
            st.set_gpu_parse(True)
            for i in range(3, 40):
                st.push_packet(pk[i], gr[i], fl[i])
            pcm = st.synth_host(dtype=dt, planar=planar).copy()
            res[planar] = (pcm, [(e.code, at) for e, at in st.parse_errors], st.channels)
            _note(st.kernels())
            st.close()
        (a, ea, ch), (p, ep, _) = res[False], res[True]
        assert ea and all(c == native.ERR_RUNTIME for c, _ in ea)
        assert ep == [(c, at // ch) for c, at in ea]
        assert p.shape == (ch, a.size // ch) and np.array_equal(p, planes_of(a, ch))


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_corpus_planar_views(gpu_parse):
    """decode_files_to_device(layout="planar") on corpus-style files, one with a damaged page (the redo path): views[i] has shape
    (C_i, T_i), strided in the arena, and equals the interleaved run's view transposed."""
    from nvorbis_amd import corpus
    from tests import c5_corpus, ogg_py
    ws = c5_corpus.writer_setup()
    files = [c5_corpus.corpus_file(ws, i, 0.05) for i in range(5)]
    files.append(open(os.path.join(GOLDEN, "1test.ogg"), "rb").read())  # mono
    pages = ogg_py.read_pages(files[2])
    bad = bytearray(files[2])
    pg = pages[len(pages) // 2]
    bad[pg["offset"] + pg["length"] - 3] ^= 0x11
    files[2] = bytes(bad)
    _, vi = corpus.decode_files_to_device(files, device=0, workers=4, gpu_parse=gpu_parse)
    want = [v.cpu().numpy() for v in vi]
    del vi
    t = {}
    arena, vp = corpus.decode_files_to_device(files, device=0, workers=4, gpu_parse=gpu_parse, timings=t, layout="planar")
    assert t.get("files_reindexed") == [2]
    for i, (v, w) in enumerate(zip(vp, want)):
        ch = v.shape[0]
        assert v.dim() == 2 and v.shape[1] * ch == w.size, (i, tuple(v.shape))
        assert v.stride(1) == 1 and v.stride(0) % 4 == 0 and v.stride(0) >= v.shape[1]
        assert np.array_equal(v.cpu().numpy().view(np.uint32), planes_of(w, ch).view(np.uint32)), i
    del arena, vp


@pytest.mark.gpu
def test_planar_twins_reached(tmp_path_factory):
    """(Last in this file: a replay child reports what its tests ran from here.)  Replays of this file's GPU tests in child
    processes under the kernel-variant toggles; then every one of the 14 planar twins must have run somewhere."""
    seen = set(_SEEN)
    if os.environ.get("NVH_TEST_CHILD"):
        out = os.environ.get("NVH_PLANAR_SEEN")
        if out:
            with open(out, "w") as fh:
                json.dump(sorted(seen), fh)
        pytest.skip("inside a replay: the parent checks the union")
    from tests.replay import run_children
    d = tmp_path_factory.mktemp("planar_seen")
    children, files = [], []
    # (three children at a time beside this process: at most four processes with the GPU open)
    for k, toggle in enumerate(["NVH_FPW=1", "NVH_FPW=4", "NVH_EMIT_ALWAYS", "NVH_NO_EMIT", "NVH_NO_EMIT8", "NVH_NO_SLAB",
                                "NVH_NO_COMPACT", "NVH_GPU_PARSE", "NVH_POISON_PLANES+NVH_GPU_PARSE"]):
        env = dict(os.environ)
        for t in toggle.split("+"):
            key, _, val = t.partition("=")
            env[key] = val or "1"
        env["NVH_TEST_CHILD"] = "1"
        env["NVH_PLANAR_SEEN"] = str(d / ("%d.json" % k))
        files.append(env["NVH_PLANAR_SEEN"])
        children.append((["test_pcm_planar.py"], env, ["-k", "synthetic_configs_planar or resident_batch_planar or throwing or twins_reached"]))
    for k in range(0, len(children), 3):
        run_children(children[k:k + 3], timeout=1500)
    for f in files:
        seen |= set(json.load(open(f)))
    missing = sorted(set(PLANAR_TWINS) - seen)
    assert not missing, (missing, sorted(seen))

"""16-bit integer PCM (NVH_PCM_S16): the emitting kernels' _s16 twins convert inside the kernels with libvorbis ov_read's rule,
s16 = clamp(rint(x * 32768), -32768, 32767) (ties to even, NaN -> 0), on the float the float path emits.  No tolerance anywhere:
the s16 output equals that function of the float output -- and so of the oracle's PCM -- exactly."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the kernels that write PCM and their twins; every twin must be reached by this file's runs (the replays included)
TWINS = {
    "k_synth+k_synth_emit": "k_synth+k_synth_emit_s16",
    "k_synth8+k_synth8_emit": "k_synth8+k_synth8_emit_s16",
    "k_synth_group2": "k_synth_group2_s16",
    "k_synth_group4": "k_synth_group4_s16",
    "k_ola_compact": "k_ola_compact_s16",
    "k_ola_emit": "k_ola_emit_s16",
    "k_ola_emit_seq": "k_ola_emit_seq_s16",
}
_SEEN = set()  # twins this process ran


def to_s16(x):
    """ov_read's conversion in numpy: float32 multiply (exact), round half to even, clamp, NaN -> 0."""
    y = np.rint(np.asarray(x, np.float32) * np.float32(32768.0))
    y = np.where(np.isnan(y), np.float32(0.0), y)
    return np.clip(y, -32768, 32767).astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_to_s16_known_answers():
    h = 0.5 / 32768.0  # half a step: ties go to even
    x = np.array([1.0, -1.0, 0.5, -0.5, h, -h, 3 * h, -3 * h, 0.99999994, -0.99999994, 1.0000001, -1.0000001,
                  np.nan, np.inf, -np.inf, -0.0, 0.0, 2.0, -2.0], np.float32)
    want = np.array([32767, -32768, 16384, -16384, 0, 0, 2, -2, 32767, -32768, 32767, -32768,
                     0, 32767, -32768, 0, 0, 32767, -32768], np.int16)
    got = to_s16(x)
    assert got.dtype == np.int16
    assert np.array_equal(got, want), list(zip(x.tolist(), got.tolist(), want.tolist()))


def test_new_entry_points_refuse_bad_arguments():
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    wr = C.c_int64(0)
    assert L.nvh_stream_synth_pcm(None, native.PCM_S16, None, None, 0, C.byref(wr)) == native.ERR_ARGUMENT
    assert L.nvh_stream_synth_begin_pcm(None, native.PCM_S16, None, 0, C.byref(wr)) == native.ERR_ARGUMENT
    assert L.nvh_batch_synth_pcm(None, native.PCM_S16, None, 0) == native.ERR_ARGUMENT
    buf = np.zeros(16, np.int16)
    pk, _, _ = nv.demux_ogg(open(os.path.join(GOLDEN, "3test.ogg"), "rb").read())
    st = nv.Stream(None, pk[0], pk[1], pk[2])  # host-only: the format is checked before anything needs a device
    try:
        for fmt in (2, -1, 7):
            assert L.nvh_stream_synth_pcm(st._h, fmt, buf.ctypes.data, None, buf.size, C.byref(wr)) == native.ERR_ARGUMENT
            assert L.nvh_stream_synth_begin_pcm(st._h, fmt, buf.ctypes.data, buf.size, C.byref(wr)) == native.ERR_ARGUMENT
        for dt in (np.float64, np.int32, np.uint16):
            with pytest.raises(ValueError):
                st.synth_host(dtype=dt)
    finally:
        st.close()


def test_reader_rejects_unknown_sample_format():
    import nvorbis_amd as nv
    data = open(os.path.join(GOLDEN, "3test.ogg"), "rb").read()
    for bad in ("s24", "u8", "float", None, 16):
        with pytest.raises(ValueError):
            nv.VorbisReader(data, sample_format=bad)  # before a context is created
        with pytest.raises(ValueError):
            nv.StreamDecoder(None, [b"", b"", b""], sample_format=bad)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _note(names):
    for k in names:
        if k.endswith("_s16"):
            _SEEN.add(k)


def _descriptor_toggle():
    return any(os.environ.get(t) for t in ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB"))


def _lockstep(nv, ctx, pk, gr, fl, clip, batch_frames):
    """Two streams over the same packets, one synthesised as float, one as s16, batch by batch: (float PCM, s16 PCM,
    [(float kernels, s16 kernels)], has_clipped of each)."""
    sf, ss_ = nv.Stream(ctx, pk[0], pk[1], pk[2]), nv.Stream(ctx, pk[0], pk[1], pk[2])
    sf.set_clip(clip)
    ss_.set_clip(clip)
    outf, outs, kern = [], [], []
    i = 3
    while i < len(pk):
        for st in (sf, ss_):
            for j in range(i, min(i + batch_frames, len(pk))):
                st.push_packet(pk[j], gr[j], fl[j])
        i += batch_frames
        if i >= len(pk):
            sf.push_end()
            ss_.push_end()
        if sf.pending()[0] == 0:
            continue
        f = sf.synth_host().copy()
        s = ss_.synth_host(dtype=np.int16).copy()
        assert s.dtype == np.int16 and s.size == f.size
        kf, ks = sf.kernels(), ss_.kernels()
        kern.append((kf, ks))
        outf.append(f)
        outs.append(s)
    hc = (sf.has_clipped(), ss_.has_clipped())
    sf.close()
    ss_.close()
    cat = lambda a, dt: np.concatenate(a) if a else np.zeros(0, dt)  # noqa: E731
    return cat(outf, np.float32), cat(outs, np.int16), kern, hc


def _decode(nv, ctx, pk, gr, fl, clip, batch_frames, fmt):
    dec = nv.StreamDecoder(ctx, pk, gr, fl, batch_frames=batch_frames, sample_format=fmt)
    dec.ClipSamples = clip
    dt = np.int16 if fmt == "s16" else np.float32
    buf = np.zeros((1 << 20) - (1 << 20) % dec.Channels, dt)
    chunks = []
    while True:
        n = dec.Read(buf, 0, buf.size)
        if n == 0:
            break
        chunks.append(buf[:n].copy())
    hc = dec.HasClipped
    dec.close()
    return (np.concatenate(chunks) if chunks else np.zeros(0, dt)), hc


CONFIGS = ["mono_res0_small_blocks", "stereo_res1_coupled", "three_ch_res2_misaligned", "six_ch_res2_4096", "two_submaps",
           "equal_blocks_overrun", "mono_8192", "stereo_8192", "mono_res1_2048", "floor0_slab", "floor0_stereo",
           "res0_slab", "odd_dims_slab", "res2_alias_stereo", "two_pass_slab", "res0_3ch",
           "table_books_pair", "table_books_general", "table_books_b1", "ch4_res1", "ch5_res2", "ch7_res1", "ch8_res2",
           "ch9_res2", "ch16_res1_4096", "ch40_res1"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
@pytest.mark.parametrize("consistent", [True, False])
def test_synthetic_configs_s16(oracle, gpu_ctx, name, consistent):
    """Every synthetic config the float parity suite decodes, clip on and off, batches of 1024 and 13 frames: the s16 stream
    equals to_s16 of the oracle's PCM, with the float run's counts and HasClipped; the s16 batches ran the float batches' kernels
    with the twins in the emitting slots."""
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 150, 11 + int(consistent), consistent_windows=consistent)
    # Floor0 under the descriptor kernels is not bit-exact to the oracle (device libm): held to the same process's float output
    exact_ref = not (name.startswith("floor0") and _descriptor_toggle())
    saturated = False
    for clip in (True, False):
        ref, _ = oracle.decode_packets(pk, gr, fl, clip=clip)
        for bf in (1024, 13):
            # the reader surface: s16 == to_s16(oracle), the float run's counts and HasClipped
            s, hcs = _decode(nv, gpu_ctx, pk, gr, fl, clip, bf, "s16")
            f, hcf = _decode(nv, gpu_ctx, pk, gr, fl, clip, bf, "f32")
            assert s.dtype == np.int16 and s.size == f.size, (name, clip, bf)
            assert np.array_equal(s, to_s16(f)), (name, clip, bf)
            if exact_ref:
                assert s.size == ref.size and np.array_equal(s, to_s16(ref)), (name, clip, bf)
            assert hcs == hcf, (name, clip, bf)
            if not clip and (np.abs(f) > 1.0).any():
                saturated = True
                assert (s[f >= 1.0] == 32767).all() and (s[f <= -1.0] == -32768).all()
            # batch by batch: the same counts, the float batch's kernels with the twins in the emitting slots
            lf, ls, kern, (kcf, kcs) = _lockstep(nv, gpu_ctx, pk, gr, fl, clip, bf)
            assert ls.size == lf.size and np.array_equal(ls, to_s16(lf)) and kcf == kcs, (name, clip, bf)
            for kf, ks in kern:
                assert ks == [TWINS.get(k, k) for k in kf], (name, kf, ks)
                _note(ks)
    if name in ("floor0_slab", "floor0_stereo"):  # Floor0 curves on random bits are loud: out-of-range samples with clip off
        assert saturated, name


def _ogg_reader_cases():
    return [(n, g) for n in ("1test", "2test", "3test", "issue6test") for g in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,gpu_parse", _ogg_reader_cases())
def test_reader_s16_files(oracle, gpu_ctx, ogg_bytes, name, gpu_parse):
    """VorbisReader(sample_format="s16") on the shipped files, both parsers: read_all, odd-sized partial reads and reads after
    seeks equal the float reader's output and the oracle's, converted; a float buffer is refused."""
    import nvorbis_amd as nv
    data = ogg_bytes[name]
    ref, _ = oracle.decode_ogg(data)
    rf = nv.VorbisReader(data, ctx=gpu_ctx, batch_frames=64, gpu_parse=gpu_parse)
    rs = nv.VorbisReader(data, ctx=gpu_ctx, batch_frames=64, gpu_parse=gpu_parse, sample_format="s16")
    with pytest.raises(TypeError):
        rs.ReadSamples(np.zeros(64, np.float32))
    with pytest.raises(TypeError):
        rf.ReadSamples(np.zeros(64, np.int16))
    f = rf.read_all()
    s = rs.read_all()
    assert s.dtype == np.int16 and np.array_equal(s, to_s16(f)) and np.array_equal(s, to_s16(ref)), name
    rf.close()
    rs.close()
    # odd-sized partial reads
    probe = nv.VorbisReader(data, ctx=gpu_ctx)
    ch = probe.Channels
    probe.close()
    rs = nv.VorbisReader(data, ctx=gpu_ctx, batch_frames=7, gpu_parse=gpu_parse, sample_format="s16")
    rng = np.random.default_rng(3)
    parts, buf = [], np.zeros(5000 * ch, np.int16)
    while True:
        k = int(rng.integers(1, 4999)) * ch
        n = rs.ReadSamples(buf, 0, k)
        if n <= 0:
            break
        parts.append(buf[:n].copy())
    assert np.array_equal(np.concatenate(parts), to_s16(ref)), name
    # seeks: the float reader's output and the oracle's, converted
    rs.close()
    rf = nv.VorbisReader(data, ctx=gpu_ctx, batch_frames=64, gpu_parse=gpu_parse)
    rs = nv.VorbisReader(data, ctx=gpu_ctx, batch_frames=64, gpu_parse=gpu_parse, sample_format="s16")
    d = oracle.open_ogg(data)
    total = rf.TotalSamples
    def outcome(r, buf, t):
        try:
            r.SeekTo(t)
            n = r.ReadSamples(buf)
            return "ok", buf[:n].copy(), r.SamplePosition
        except Exception as e:  # the float reader must fail the same way
            return type(e).__name__, None, None
    for t in [0, 1, 127, 1000, total // 3, total // 2, max(total - 700, 0)]:
        cf, pf, posf = outcome(rf, np.zeros(777 * ch, np.float32), t)
        cs, ps, poss = outcome(rs, np.zeros(777 * ch, np.int16), t)
        assert cs == cf and poss == posf, (name, t, cf, cs)
        if cs != "ok":
            continue
        assert ps.size == pf.size and np.array_equal(ps, to_s16(pf)), (name, t)
        rc, smp, _ = oracle.seek_and_read(d, t, 777 * ch)
        if rc == 0 and not isinstance(smp, int) and smp.size == ps.size:
            assert np.array_equal(ps, to_s16(smp)), (name, t)
    rf.close()
    rs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_pipelined_s16_alternating_formats(gpu_ctx, ogg_bytes, gpu_parse):
    """synth_begin / synth_end in s16 equal blocking synth_host in s16, with float batches in between on the same stream (the
    format is the call's; the carried tail is float planes either way)."""
    import nvorbis_amd as nv
    pk, _, _ = nv.demux_ogg(ogg_bytes["3test"])

    def streams():
        st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
        if gpu_parse:
            st.set_gpu_parse(True)
        return st
    fmts = [np.int16, np.float32, np.int16, np.int16, np.float32, np.int16]
    a, b = streams(), streams()
    cuts = np.linspace(3, len(pk), len(fmts) + 1).astype(int)
    want, got = [], []
    out = 0
    for k, dt in enumerate(fmts):
        for st in (a, b):
            for i in range(cuts[k], cuts[k + 1]):
                st.push_packet(pk[i], -1, 0)
        want.append(a.synth_host(dtype=dt).copy())
        b.synth_begin(dtype=dt)
        out += 1
        if out == 2:
            got.append(b.synth_end().copy())
            out -= 1
    while out:
        got.append(b.synth_end().copy())
        out -= 1
    for k, (w, g) in enumerate(zip(want, got)):
        assert g.dtype == np.dtype(fmts[k]) and np.array_equal(w, g), k
    a.close()
    b.close()


@pytest.mark.gpu
def test_resident_batch_s16(gpu_ctx):
    """Batch.synth into a torch.int16 device tensor at the bench shape (4096 stereo n = 2048 frames) equals to_s16 of the float
    batch; a d_pcm that is not 16-byte aligned is refused."""
    torch = _torch()
    import bench
    import nvorbis_amd as nv
    from nvorbis_amd import native
    headers, ll, ch = bench.ll_packets(nv, os.path.join(GOLDEN, "3test.ogg"))
    st = nv.Stream(gpu_ctx, headers[0], headers[1], headers[2])
    st.push_packet(ll[0], -1, 0)
    assert st.synth_host().size == 0
    for i in range(4096):
        st.push_packet(ll[(1 + i) % len(ll)], -1, 0)
    b = st.upload_batch()
    n = b.samples * ch
    pf = torch.zeros(n, dtype=torch.float32, device="cuda")
    ps = torch.full((n + 8,), 7, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    b.synth(pf.data_ptr(), n)
    kf = b.kernels()
    b.synth(ps.data_ptr(), n, dtype=np.int16)
    ks = b.kernels()
    _note(ks)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    f = pf.cpu().numpy()
    s = ps.cpu().numpy()
    assert ks == [TWINS.get(k, k) for k in kf], (kf, ks)
    assert np.array_equal(s[:n], to_s16(f))
    assert (s[n:] == 7).all()  # nothing past the batch
    with pytest.raises(native.NvhError) as e:
        b.synth(ps.data_ptr() + 2, n, dtype=np.int16)
    assert e.value.code == native.ERR_ARGUMENT
    b.free()
    st.close()


@pytest.mark.gpu
def test_throwing_packet_gpu_parse_s16(gpu_ctx):
    """GPU-parse mode with a throwing packet in the batch (the batch is parsed again on the host): the s16 call reports the float
    call's written count and parse-error positions, and its PCM is the float PCM converted."""
    import nvorbis_amd as nv
    from nvorbis_amd import native
    from tests import synth_stream as ss
    cfg = ss.config("stereo_res1_coupled")
    old = cfg["books"][3]
    cfg["books"][3] = ss.IncompleteBook(old.bits, dims=old.dims, lookup=old.lookup, min_me=old.min_me, delta_me=old.delta_me,
                                        value_bits=old.value_bits, sequence_p=old.sequence_p, mults=old.mults)
    pk, gr, fl = ss.make_stream(cfg, 200, 1)
    res = {}
    for dt in (np.float32, np.int16):
        st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
        st.set_gpu_parse(True)
        for i in range(3, 40):
            st.push_packet(pk[i], gr[i], fl[i])
        pcm = st.synth_host(dtype=dt).copy()
        res[np.dtype(dt).name] = (pcm, [(e.code, at) for e, at in st.parse_errors])
        st.close()
    (f, ef), (s, es) = res["float32"], res["int16"]
    assert ef and all(c == native.ERR_RUNTIME for c, _ in ef)
    assert es == ef and s.size == f.size and np.array_equal(s, to_s16(f))


@pytest.mark.gpu
def test_twins_reached(tmp_path_factory):
    """(Last in this file: a replay child reports what its tests ran from here.)  Replays of this file's GPU tests in child processes under the kernel-variant toggles (frame groups of 1 and 4, paired
    emission always / never / never for wide frames, the descriptor kernels, no compact hand-over, GPU parse, poisoned planes);
    then every emitting kernel's twin must have run somewhere -- a kernel nothing reaches fails here."""
    seen = set(_SEEN)
    if os.environ.get("NVH_TEST_CHILD"):
        out = os.environ.get("NVH_S16_SEEN")
        if out:
            with open(out, "w") as fh:
                json.dump(sorted(seen), fh)
        pytest.skip("inside a replay: the parent checks the union")
    from tests.replay import run_children
    d = tmp_path_factory.mktemp("s16_seen")
    children, files = [], []
    # (three children at a time beside this process: at most four processes with the GPU open)
    for k, toggle in enumerate(["NVH_FPW=1", "NVH_FPW=4", "NVH_EMIT_ALWAYS", "NVH_NO_EMIT", "NVH_NO_EMIT8", "NVH_NO_SLAB",
                                "NVH_NO_COMPACT", "NVH_GPU_PARSE", "NVH_POISON_PLANES+NVH_GPU_PARSE"]):
        env = dict(os.environ)
        for t in toggle.split("+"):
            key, _, val = t.partition("=")
            env[key] = val or "1"
        env["NVH_TEST_CHILD"] = "1"
        env["NVH_S16_SEEN"] = str(d / ("%d.json" % k))
        files.append(env["NVH_S16_SEEN"])
        children.append((["test_pcm_s16.py"], env, ["-k", "synthetic_configs_s16 or resident_batch_s16 or throwing or twins_reached"]))
    for k in range(0, len(children), 3):
        run_children(children[k:k + 3], timeout=1500)
    for f in files:
        seen |= set(json.load(open(f)))
    missing = sorted(set(TWINS.values()) - seen)
    assert not missing, "no run of this file reached %s (seen: %s)" % (missing, sorted(seen))

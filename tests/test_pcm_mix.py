"""The mono down-mix (nvh_*_mix with NVH_MIX_MONO), summed inside the emitting kernels' _mono twins.

The rule (include/nvorbis_hip.h), for a stream of C channels, with x_c(t) the float sample the float path produces for channel c
at time t BEFORE ClipSamples' clip:

    s = x_0;  s = s + x_1;  ...  s = s + x_{C-1}      (C - 1 fp32 additions, in channel order, each rounded once)
    m = s / (float)C                                   (one correctly rounded fp32 division)
    y = ClipSamples ? clip(m) : m                      (Utils.cs:30-43, applied ONCE, to the mix)

NVH_PCM_S16 converts y with ov_read's conversion (tests/test_pcm_s16.py: to_s16).  HasClipped follows the mix.  C = 1 is the
identity and runs the existing kernels.  The expected value is always computed here, on the CPU, from the ORACLE's unclipped float
PCM in numpy float32 (mix_rule below); every comparison is bit for bit."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests.test_pcm_s16 import to_s16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the 14 mono twins (as the launcher names them in the timing slots); every one must be reached by this file's runs
MONO_TWINS = ["k_synth+k_synth_emit_mono", "k_synth+k_synth_emit_s16_mono",
              "k_synth8+k_synth8_emit_mono", "k_synth8+k_synth8_emit_s16_mono",
              "k_synth_group2_mono", "k_synth_group2_s16_mono", "k_synth_group4_mono", "k_synth_group4_s16_mono",
              "k_ola_compact_mono", "k_ola_compact_s16_mono", "k_ola_emit_mono", "k_ola_emit_s16_mono",
              "k_ola_emit_seq_mono", "k_ola_emit_seq_s16_mono"]
_SEEN = set()  # twins a bit-exact comparison of this process named
SENTINEL = {np.dtype(np.float32): np.float32(-1234.5), np.dtype(np.int16): np.int16(-7777)}
CLIP = np.float32(0.99999994)


def mix_rule(x, ch, clip, dt=np.float32):
    """The rule above on interleaved UNCLIPPED float32 PCM: (mixed samples of dtype dt, whether the mix clipped)."""
    p = np.asarray(x, np.float32).reshape(-1, ch)
    s = p[:, 0].copy()
    for c in range(1, ch):
        s = (s + p[:, c]).astype(np.float32)  # one fp32 addition per channel, in channel order
    with np.errstate(all="ignore"):
        m = (s / np.float32(ch)).astype(np.float32)  # one correctly rounded fp32 division
    hi, lo = m > CLIP, m < -CLIP  # (a NaN compares false twice and passes through, as in the reference)
    clipped = bool(hi.any() or lo.any())
    if clip:
        m = np.where(hi, CLIP, np.where(lo, -CLIP, m)).astype(np.float32)
    return (to_s16(m) if np.dtype(dt) == np.int16 else m), clipped


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

NAMES = ("nvh_stream_synth_mix", "nvh_stream_synth_begin_mix", "nvh_batch_synth_mix")


def test_mix_entry_points_are_exported_and_declared():
    from nvorbis_amd import native
    L = native.lib()
    hdr = open(os.path.join(ROOT, "include", "nvorbis_hip.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "NativeMethods.cs")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in native.SIGNATURES, name
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern (?:unsafe )?int %s\(" % name, cs), name
    assert (native.MIX_NONE, native.MIX_MONO) == (0, 1)
    assert re.search(r"#define NVH_MIX_NONE 0\b", hdr) and re.search(r"#define NVH_MIX_MONO 1\b", hdr)
    assert "NVH_MIX_NONE = 0, NVH_MIX_MONO = 1" in cs


def test_mix_entry_points_refuse_bad_arguments():
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    wr = C.c_int64(0)
    buf = np.zeros(1 << 16, np.float32)
    F32, S16, NONE, MONO = native.PCM_F32, native.PCM_S16, native.MIX_NONE, native.MIX_MONO
    for fmt in (F32, S16):
        assert L.nvh_stream_synth_mix(None, fmt, MONO, buf.ctypes.data, None, 16, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_begin_mix(None, fmt, MONO, buf.ctypes.data, 16, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_batch_synth_mix(None, fmt, MONO, None, 16) == native.ERR_ARGUMENT
    pk, _, _ = nv.demux_ogg(open(os.path.join(GOLDEN, "3test.ogg"), "rb").read())
    st = nv.Stream(None, pk[0], pk[1], pk[2])  # host-only: the arguments are checked before anything needs a device
    try:
        assert st.channels == 2
        for i in range(3, 12):
            st.push_packet(pk[i], -1, 0)
        _, n = st.pending()
        assert n > 0
        for fmt in (2, -1, 7):  # unknown formats (the mix is not a format: these stay refused)
            assert L.nvh_stream_synth_mix(st._h, fmt, MONO, buf.ctypes.data, None, n, C.byref(wr)) == native.ERR_ARGUMENT
            assert L.nvh_stream_synth_begin_mix(st._h, fmt, MONO, buf.ctypes.data, n, C.byref(wr)) == native.ERR_ARGUMENT
            assert L.nvh_batch_synth_mix(None, fmt, MONO, None, n) == native.ERR_ARGUMENT
        for mix in (2, -1, 9):  # unknown mixes
            for fmt in (F32, S16):
                assert L.nvh_stream_synth_mix(st._h, fmt, mix, buf.ctypes.data, None, n, C.byref(wr)) == native.ERR_ARGUMENT
                assert L.nvh_stream_synth_begin_mix(st._h, fmt, mix, buf.ctypes.data, n, C.byref(wr)) == native.ERR_ARGUMENT
        for fmt in (F32, S16):
            for mix in (NONE, MONO):
                # both destinations, or neither with PCM to write
                assert L.nvh_stream_synth_mix(st._h, fmt, mix, buf.ctypes.data, buf.ctypes.data, 2 * n, C.byref(wr)) == native.ERR_ARGUMENT
                assert L.nvh_stream_synth_mix(st._h, fmt, mix, None, None, 2 * n, C.byref(wr)) == native.ERR_ARGUMENT
            # a capacity below the pending samples: n for the mix, n * channels without it
            assert L.nvh_stream_synth_mix(st._h, fmt, MONO, buf.ctypes.data, None, n - 1, C.byref(wr)) == native.ERR_ARGUMENT
            assert L.nvh_stream_synth_mix(st._h, fmt, NONE, buf.ctypes.data, None, 2 * n - 1, C.byref(wr)) == native.ERR_ARGUMENT
        # a device base not aligned to its sample size (the mix), not 16-byte aligned (unmixed 16-bit PCM: the *_pcm rule)
        assert L.nvh_stream_synth_mix(st._h, F32, MONO, None, C.c_void_p(4096 + 2), n, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_mix(st._h, S16, MONO, None, C.c_void_p(4096 + 1), n, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_mix(st._h, S16, NONE, None, C.c_void_p(4096 + 8), 2 * n, C.byref(wr)) == native.ERR_ARGUMENT
        # NVH_MIX_NONE is accepted where the *_pcm call is: past the argument checks both report the missing device
        for fmt in (F32, S16):
            a = L.nvh_stream_synth_pcm(st._h, fmt, buf.ctypes.data, None, 2 * n, C.byref(wr))
            b = L.nvh_stream_synth_mix(st._h, fmt, NONE, buf.ctypes.data, None, 2 * n, C.byref(wr))
            c = L.nvh_stream_synth_mix(st._h, fmt, MONO, buf.ctypes.data, None, n, C.byref(wr))
            assert a == b == c == native.ERR_NO_GPU
        # the Python surface
        with pytest.raises(ValueError):
            st.synth_host(mix="stereo")
        with pytest.raises(ValueError):
            st.synth_host(mix="mono", planar=True)
        with pytest.raises(ValueError):
            st.synth_begin(mix="mono", planar=True)
        with pytest.raises(ValueError):
            st.synth_device(0, 0, mix="mono", plane_stride=n)
        with pytest.raises(ValueError):
            st.synth_host(out=np.zeros(n - 1, np.float32), mix="mono")
    finally:
        st.close()


def test_reader_and_decoder_reject_unknown_mixes():
    import nvorbis_amd as nv
    data = open(os.path.join(GOLDEN, "3test.ogg"), "rb").read()
    for bad in ("Mono", "stereo", "", 1, "left"):
        with pytest.raises(ValueError):
            nv.VorbisReader(data, mix=bad)  # before a context is created
        with pytest.raises(ValueError):
            nv.StreamDecoder(None, [b"", b"", b""], mix=bad)
    with pytest.raises(ValueError):
        nv.VorbisReader(data, mix="mono", layout="planar")
    with pytest.raises(ValueError):
        nv.StreamDecoder(None, [b"", b"", b""], mix="mono", layout="planar")


def test_division_by_a_power_of_two_is_a_multiply():
    """What licenses `* 0.5f` in the stereo kernels (and the compiler's x / 4, x / 8 -> multiply): for C = 2, 4, 8,
    s / C == s * (1 / C) bit for bit over random and edge float32 values."""
    rng = np.random.default_rng(1)
    tiny = np.float32(1.4e-45)
    edge = np.array([0.0, -0.0, 1.0, -1.0, 0.99999994, -0.99999994, 1.0000001, -1.0000001, np.inf, -np.inf, np.nan,
                     tiny, -tiny, 3 * tiny, 5 * tiny, 7 * tiny, 1.1754942e-38, 1.1754944e-38, 2.3509887e-38, 3.4028235e38, -3.4028235e38],
                    np.float32)
    bits = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)  # every exponent, denormals, NaNs
    near = (np.float32(1.0) + rng.integers(-64, 64, 4096).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    x = np.concatenate([edge, bits, near, -near, rng.standard_normal(1 << 16).astype(np.float32)])
    with np.errstate(all="ignore"):
        for c in (2, 4, 8):
            d = (x / np.float32(c)).astype(np.float32)
            m = (x * np.float32(1.0 / c)).astype(np.float32)
            nan = np.isnan(d)
            assert np.array_equal(nan, np.isnan(m))
            assert np.array_equal(d[~nan].view(np.uint32), m[~nan].view(np.uint32)), c
        # ... and that this is NOT so for the other channel counts: the kernels divide
        for c in (3, 5, 6, 7):
            d = (x / np.float32(c)).astype(np.float32)
            m = (x * np.float32(1.0 / c)).astype(np.float32)
            ok = ~np.isnan(d)
            assert not np.array_equal(d[ok].view(np.uint32), m[ok].view(np.uint32)), c


def test_mix_rule_known_answers():
    x = np.array([0.5, 0.25, 1.5, 1.0, -2.0, -1.0, 1.5, -1.5], np.float32)  # stereo: (l, r) pairs
    m, clipped = mix_rule(x, 2, True)
    assert np.array_equal(m, np.array([0.375, CLIP, -CLIP, 0.0], np.float32)) and clipped
    m, clipped = mix_rule(x, 2, False)
    assert np.array_equal(m, np.array([0.375, 1.25, -1.5, 0.0], np.float32)) and clipped
    m, clipped = mix_rule(np.array([1.5, -1.5, 0.25, 0.25], np.float32), 2, True)  # one channel alone leaves [-1, 1]: the mix does not
    assert np.array_equal(m, np.array([0.0, 0.25], np.float32)) and not clipped
    m, _ = mix_rule(np.array([1.0, 1.0, 1.0], np.float32), 3, True, np.int16)
    assert m.dtype == np.int16 and m[0] == 32767
    m, _ = mix_rule(np.array([0.1, 0.2, 0.3], np.float32), 3, False)
    assert m[0] == np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.3)) / np.float32(3)


def test_corpus_refuses_unknown_mixes():
    from nvorbis_amd import corpus
    with pytest.raises(ValueError):
        corpus.decode_files_to_device([], mix="stereo")
    with pytest.raises(ValueError):
        corpus.decode_files_to_device([], mix="mono", layout="planar")
    with pytest.raises(ValueError):
        corpus.transcode([b""], mix="mono")


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

_OPEN = []


@pytest.fixture(autouse=True)
def _close_streams():
    yield
    while _OPEN:
        x = _OPEN.pop()
        (x.free if hasattr(x, "free") else x.close)()


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
        if k.endswith("_mono"):
            _SEEN.add(k)


def _descriptor_toggle():
    return any(os.environ.get(t) for t in ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB"))


def _toggled():
    return _descriptor_toggle() or any(os.environ.get(t) for t in ("NVH_FPW", "NVH_NO_EMIT", "NVH_NO_EMIT8", "NVH_EMIT_ALWAYS", "NVH_GPU_PARSE"))


def _synth_mono_device(torch, st, dt, off):
    """The pending batch of `st`, mixed, into a guard-filled device buffer at a base `off` samples in: the samples written;
    asserts that nothing outside [0, written) was written."""
    _, n = st.pending()
    size = off + n + 64
    tdt = torch.float32 if dt == np.float32 else torch.int16
    buf = torch.full((size,), float(SENTINEL[np.dtype(dt)]), dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    got = st.synth_device(buf.data_ptr() + off * np.dtype(dt).itemsize, n, dtype=dt, mix="mono")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert got <= n
    keep = np.ones(size, bool)
    keep[off:off + got] = False
    assert (h[keep] == SENTINEL[np.dtype(dt)]).all(), ("written outside [0, written)", off, n, got)
    return h[off:off + got].copy()


def _decode_mono(nv, torch, ctx, pk, gr, fl, clip, batch_frames, dt, gpu_parse=False, offs=(0,), first=None):
    """A stream over the packets, batch by batch (the first batch of `first` frames when given), mixed into device memory with the
    base offsets `offs` in turn: (mixed PCM, kernel names per batch, has_clipped)."""
    st = _stream(nv, ctx, pk)
    if gpu_parse:
        st.set_gpu_parse(True)
    st.set_clip(clip)
    out, kern = [], []
    i, k = 3, 0
    while i < len(pk):
        step = first if (first and i == 3) else batch_frames
        for j in range(i, min(i + step, len(pk))):
            st.push_packet(pk[j], gr[j], fl[j])
        i += step
        if i >= len(pk):
            st.push_end()
        if st.pending()[0] == 0:
            continue
        out.append(_synth_mono_device(torch, st, dt, offs[k % len(offs)]))
        k += 1
        kern.append(st.kernels())
    hc = st.has_clipped()
    st.close()
    return (np.concatenate(out) if out else np.zeros(0, dt)), kern, hc


# the synthetic setups (tests/synth_stream.py) and the kernel family each must name with the default toggles (None: no claim);
# together with the replays of test_mono_twins_reached they reach every emitting family
# (random packets stay below the share of steady-state frames that paired emission asks for: the stereo setup is the batch that runs
# k_synth + k_ola_compact_mono; the frame groups are reached by the long blocks of test_resident_batch_mono)
CONFIGS = [("stereo_res1_coupled", "k_ola_compact"), ("stereo_8192", None), ("floor0_stereo", None), ("res2_alias_stereo", None),
           ("three_ch_res2_misaligned", None), ("res0_3ch", None), ("ch4_res1", None),
           ("ch5_res2", None), ("six_ch_res2_4096", None), ("ch7_res1", None),
           ("ch8_res2", None), ("ch9_res2", None), ("ch16_res1_4096", None), ("ch40_res1", None),
           ("two_submaps", None), ("mono_res1_2048", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,family", CONFIGS)
@pytest.mark.parametrize("consistent", [True, False])
def test_synthetic_configs_mono(oracle, gpu_ctx, name, family, consistent):
    """The synthetic setups, consistent and inconsistent window flags, clip on and off, batches of 1024 and 13 frames and a first
    batch of 3, float and s16, device bases aligned and one sample off: the mixed output equals the rule applied to the oracle's
    unclipped PCM; HasClipped follows the mix; nothing outside [0, written) is written; a one-channel stream names no _mono kernel."""
    torch = _torch()
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 150, 11 + int(consistent), consistent_windows=consistent)
    ref, info = oracle.decode_packets(pk, gr, fl, clip=False)
    ch = info["channels"]
    if name.startswith("floor0") and _descriptor_toggle():
        # (the descriptor kernels' Floor0 curve is not the oracle's to the bit -- the existing suites drop the oracle comparison
        # for these setups under these toggles (test_pcm_s16 / test_pcm_planar: exact_ref).  In those replays only, and for the
        # floor0 setups only, the rule is applied to the library's own unclipped interleaved output, which cannot be held to the
        # oracle: a consistency check of the mix, not a parity check.  Every other case of this test is held to the oracle.)
        dec = nv.StreamDecoder(gpu_ctx, pk, gr, fl, batch_frames=1024)
        dec.ClipSamples = False
        buf = np.zeros(ref.size + 64 * ch, np.float32)
        got = dec.Read(buf, 0, buf.size - buf.size % ch)
        dec.close()
        assert got == ref.size
        ref = buf[:got].copy()
    # (Destinations: every batch goes to a base of its own.  Inside a batch a frame's out_pos is the sum of the emit counts before
    # it, multiples of 16 for blocks of 64 and more; only a frame trimmed by the end-of-stream granule has another count, and it is
    # the stream's last.  So an odd position reaches the kernels as the BASE of a later batch in a contiguous destination: the
    # base one sample off below, which takes the host's fall-back and the per-sample branch.)
    for clip in (True, False):
        for dt in (np.float32, np.int16):
            want, want_clipped = mix_rule(ref, ch, clip, dt)
            for bf, offs, first in ((1024, (0,), None), (13, (0, 1), None), (16, (0,), 3)):
                if ch == 1:
                    offs = (0,)  # (one channel is the *_pcm call, with that call's alignment rule)
                got, kern, hc = _decode_mono(nv, torch, gpu_ctx, pk, gr, fl, clip, bf, dt, offs=offs, first=first)
                assert same_bits(got, want), (name, consistent, clip, dt, bf, got.size, want.size)
                _note(k for ks in kern for k in ks)
                if clip:
                    assert hc == want_clipped, (name, consistent, dt, bf)
                sfx = "_s16_mono" if dt == np.int16 else "_mono"
                if ch == 1:
                    assert not any(k.endswith("_mono") for ks in kern for k in ks), kern
                else:
                    assert all(any(k.endswith(sfx) for k in ks) for ks in kern), kern
                if family and bf == 1024 and consistent and not _toggled():
                    assert any(family + sfx in ks for ks in kern), (name, family + sfx, kern)


def _ogg_reader_cases():
    return [(n, g) for n in ("1test", "2test", "3test", "issue6test") for g in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,gpu_parse", _ogg_reader_cases())
def test_reader_mono_files(oracle, gpu_ctx, ogg_bytes, name, gpu_parse):
    """VorbisReader(mix="mono") on the shipped files, both parsers, clip on and off, float and s16: read_all with two batch sizes,
    odd-sized partial reads, and seeks followed by reads equal the rule applied to the oracle's unclipped PCM from that position."""
    import nvorbis_amd as nv
    data = ogg_bytes[name]
    ref, info = oracle.decode_ogg(data, clip=False)
    ch = info["channels"]
    opened = []

    def reader(**kw):
        r = nv.VorbisReader(data, ctx=gpu_ctx, gpu_parse=gpu_parse, **kw)
        opened.append(r)
        return r
    try:
        for clip in (True, False):
            for fmt, dt in (("f32", np.float32), ("s16", np.int16)):
                want, want_clipped = mix_rule(ref, ch, clip, dt)
                for bf in (64, 4096):
                    r = reader(batch_frames=bf, sample_format=fmt, mix="mono")
                    r.ClipSamples = clip
                    assert r.Channels == ch and r.OutputChannels == (1 if ch > 1 else ch)
                    got = r.read_all()
                    assert got.ndim == 1 and same_bits(got, want), (name, clip, fmt, bf)
                    assert r.SamplePosition == info["position"]
                    if clip:
                        assert r.HasClipped == want_clipped
                with pytest.raises(TypeError):
                    r.ReadSamples(np.zeros(64, np.float64))
                # odd-sized partial reads at odd offsets of the buffer
                r = reader(batch_frames=7, sample_format=fmt, mix="mono")
                r.ClipSamples = clip
                rng = np.random.default_rng(5)
                parts, buf = [], np.zeros(5000, dt)
                while True:
                    off = int(rng.integers(0, 100))
                    k = int(rng.integers(1, 4899)) | 1
                    n = r.ReadSamples(buf, off, k)
                    if n <= 0:
                        break
                    parts.append(buf[off:off + n].copy())
                assert same_bits(np.concatenate(parts), want), (name, clip, fmt)
                # seeks: the oracle's own seek and read from the same position, unclipped, through the rule
                r = reader(batch_frames=64, sample_format=fmt, mix="mono")
                r.ClipSamples = clip
                total = r.TotalSamples
                d = oracle.open_ogg(data)
                try:
                    for t in (0, 1, 1000, total // 3, max(total - 700, 0)):
                        rc, o, opos = oracle.seek_and_read(d, t, 777 * ch, clip=False)
                        try:
                            r.SeekTo(t)
                            b = np.zeros(777, dt)
                            n = r.ReadSamples(b)
                            mine = ("ok", b[:n].copy(), r.SamplePosition)
                        except Exception as e:  # noqa: BLE001
                            mine = (type(e).__name__, None, None)
                        if rc != 0 or not isinstance(o, np.ndarray):
                            assert mine[0] != "ok", (name, fmt, t, rc)
                            break  # (the oracle's decoder is in its failed state)
                        assert mine[0] == "ok", (name, fmt, t, mine[0])
                        w, _ = mix_rule(o, ch, clip, dt)
                        assert same_bits(mine[1], w) and mine[2] == opos, (name, clip, fmt, t)
                finally:
                    oracle.L.orc_close(d)
    finally:
        for r in opened:
            r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_pipelined_mono_alternating(oracle, gpu_ctx, ogg_bytes, gpu_parse):
    """synth_begin / synth_end with pinned destinations alternating mono-f32, interleaved-f32, mono-s16 and planar flights on one
    stream, so that the carried tail crosses every pair of forms: each flight equals its form of the oracle's PCM of that batch."""
    import nvorbis_amd as nv
    pk, gr, fl = nv.demux_ogg(ogg_bytes["3test"])
    st = _stream(nv, gpu_ctx, pk)
    if gpu_parse:
        st.set_gpu_parse(True)
    ch = st.channels
    forms = ["mono_f32", "il_f32", "mono_s16", "planar_f32"]
    plan = [f for a in forms for b in forms if a != b for f in (a, b)]  # every ordered pair of neighbours occurs
    pairs = set(zip(plan, plan[1:]))
    assert all((a, b) in pairs for a in forms for b in forms if a != b)
    for clip in (True, False):
        st.reset()
        st.set_clip(clip)
        refc, _ = oracle.decode_ogg(ogg_bytes["3test"], clip=clip)
        refu, _ = oracle.decode_ogg(ogg_bytes["3test"], clip=False)
        cuts = np.linspace(3, len(pk), len(plan) + 1).astype(int)
        got, sizes = [], []
        out = 0
        for k, form in enumerate(plan):
            for i in range(cuts[k], cuts[k + 1]):
                st.push_packet(pk[i], gr[i], fl[i])
            if k == len(plan) - 1:
                st.push_end()
            n = st.pending()[1]
            sizes.append(n)
            dt = np.int16 if form.endswith("s16") else np.float32
            exp = st.synth_begin(dtype=dt, planar=form.startswith("planar"), mix="mono" if form.startswith("mono") else None)
            assert exp == (n * ch if form == "il_f32" else n)
            out += 1
            if out == 2:
                got.append(st.synth_end().copy())
                out -= 1
        while out:
            got.append(st.synth_end().copy())
            out -= 1
        pos = 0
        for form, n, g in zip(plan, sizes, got):
            u, c = refu[pos * ch:(pos + n) * ch], refc[pos * ch:(pos + n) * ch]
            pos += n
            if form == "il_f32":
                want = c
            elif form == "planar_f32":
                want = np.ascontiguousarray(c.reshape(-1, ch).T)
            else:
                want, _ = mix_rule(u, ch, clip, np.int16 if form.endswith("s16") else np.float32)
            assert same_bits(g, want), (form, clip, pos)
        assert pos * ch == refu.size


@pytest.mark.gpu
def test_resident_batch_mono(oracle, gpu_ctx, ogg_bytes):
    """nvh_batch_synth_mix on a resident batch, launched twice: identical PCM, equal to the rule on the oracle's PCM; the guard
    behind the batch keeps its value; a short capacity and an unknown mix are refused."""
    torch = _torch()
    import nvorbis_amd as nv
    from nvorbis_amd import native
    data = ogg_bytes["3test"]
    pk, gr, fl = nv.demux_ogg(data)
    ref, info = oracle.decode_ogg(data, clip=False)
    ch = info["channels"]
    for clip in (True, False):
        st = _stream(nv, gpu_ctx, pk)
        st.set_clip(clip)
        for i in range(3, len(pk)):
            st.push_packet(pk[i], gr[i], fl[i])
        st.push_end()
        b = st.upload_batch()
        _OPEN.append(b)
        n = b.samples
        assert n * ch == ref.size
        for dt, tdt in ((np.float32, torch.float32), (np.int16, torch.int16)):
            want, _ = mix_rule(ref, ch, clip, dt)
            buf = torch.full((n + 64,), float(SENTINEL[np.dtype(dt)]), dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            first = None
            for rep in range(2):
                b.synth(buf.data_ptr(), n, dtype=dt, mix="mono")
                ks = b.kernels()
                assert any(k.endswith("_mono") for k in ks), ks
                gpu_ctx.synchronize()
                h = buf.cpu().numpy()
                assert same_bits(h[:n], want), (clip, dt, rep)
                _note(ks)
                assert (h[n:] == SENTINEL[np.dtype(dt)]).all()
                if first is None:
                    first = h.copy()
                assert np.array_equal(h, first)
            with pytest.raises(native.NvhError) as e:
                b.synth(buf.data_ptr(), n - 1, dtype=dt, mix="mono")
            assert e.value.code == native.ERR_ARGUMENT
            assert native.lib().nvh_batch_synth_mix(b._h, native.PCM_F32, 5, C.c_void_p(buf.data_ptr()), n) == native.ERR_ARGUMENT
        b.free()
        st.close()
    # the bench shape: 4096 stereo long blocks in one batch (frame groups; NVH_FPW=1: k_synth + k_synth_emit), and six channels
    # at 4096 (the wide emission), each through the oracle
    import bench
    from tests import synth_stream as ss
    headers, ll, _ = bench.ll_packets(nv, os.path.join(GOLDEN, "3test.ogg"))
    pk2 = list(headers) + [ll[0]] + [ll[(1 + i) % len(ll)] for i in range(4096)]
    pk6, gr6, fl6 = ss.filtered_stream(oracle, "six_ch_res2_4096", 150, 12, consistent_windows=True)
    for pk, gr, fl, fam in ((pk2, [-1] * len(pk2), [0] * len(pk2), "k_synth_group2"), (pk6, gr6, fl6, None)):
        ref, info = oracle.decode_packets(pk, gr, fl, clip=False)
        ch = info["channels"]
        for clip in (True, False):
            for dt in (np.float32, np.int16):
                want, _ = mix_rule(ref, ch, clip, dt)
                got, kern, _ = _decode_mono(nv, torch, gpu_ctx, pk, gr, fl, clip, 8192, dt)
                assert same_bits(got, want), (fam, clip, dt)
                _note(k for ks in kern for k in ks)
                if fam and not _toggled():
                    assert any(fam + ("_s16_mono" if dt == np.int16 else "_mono") in ks for ks in kern), kern


@pytest.mark.gpu
def test_throwing_packet_gpu_parse_mono(gpu_ctx):
    """GPU-parse mode with a throwing packet in the batch: the mixing call reports the same codes and samples_before as the
    unmixed call -- what this test is for.  Its PCM is compared with the rule applied to the unmixed call's unclipped PCM:
    a consistency check only (the oracle stops at the throwing packet; the parity of the mix is the other tests')."""
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
        for mix in (None, "mono"):
            st = _stream(nv, gpu_ctx, pk)
            st.set_gpu_parse(True)
            st.set_clip(False)
            for i in range(3, 40):
                st.push_packet(pk[i], gr[i], fl[i])
            pcm = st.synth_host(dtype=np.float32 if mix is None else dt, mix=mix).copy()
            res[mix] = (pcm, [(e.code, at) for e, at in st.parse_errors], st.channels)
            st.close()
        (a, ea, ch), (m, em, _) = res[None], res["mono"]
        assert ea and all(c == native.ERR_RUNTIME for c, _ in ea)
        assert em == [(c, at // ch) for c, at in ea]
        want, _ = mix_rule(a, ch, False, dt)
        assert same_bits(m, want)


# (setup, seed, packets of the prefix): prefixes of synthetic streams, found with the oracle, in which a channel alone leaves
# [-1, 1] while no mixed sample does; the whole stream of the same setup and seed is loud enough that the mix clips too
CLIP_CASES = [("res2_alias_stereo", 2, 27), ("stereo_8192", 1, 5), ("three_ch_res2_misaligned", 1, 5), ("ch4_res1", 4, 7),
              ("ch4_res1", 1, 14)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,k", CLIP_CASES)
def test_has_clipped_follows_the_mix(oracle, gpu_ctx, name, seed, k):
    """A stream whose float samples exceed +-1 in one channel only: with clipping ON, HasClipped stays False and the output is
    not clamped.  The same stream carried on until the sum exceeds +-1 too: HasClipped is True, the float output holds the clip
    value and the s16 output saturates.  (The replays of test_mono_twins_reached run this under the toggles that select the
    emitting kernels, each of which has its own clip.)"""
    torch = _torch()
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 40, seed)
    for npk, mix_clips in ((k, False), (len(pk), True)):
        p, g, f = pk[:npk], gr[:npk], fl[:npk]
        ref, info = oracle.decode_packets(p, g, f, clip=False)
        ch = info["channels"]
        alone = bool((np.abs(ref.reshape(-1, ch)) > CLIP).any())
        unclamped, clipped = mix_rule(ref, ch, False)
        assert alone and clipped == mix_clips, (name, seed, npk)  # (the premise, from the oracle)
        for dt in (np.float32, np.int16):
            want, _ = mix_rule(ref, ch, True, dt)
            for bf, first in ((1024, None), (13, None), (16, 3)):
                got, kern, hc = _decode_mono(nv, torch, gpu_ctx, p, g, f, True, bf, dt, first=first)
                assert same_bits(got, want), (name, seed, npk, dt, bf)
                _note(x for ks in kern for x in ks)
                assert hc == mix_clips, (name, seed, npk, dt, bf, kern)
                if not mix_clips and dt == np.float32:
                    assert same_bits(got, unclamped)  # nothing was clamped
                if mix_clips:
                    sat = np.abs(unclamped) > CLIP
                    if dt == np.float32:
                        assert (np.abs(got[sat]) == CLIP).all() and sat.any()
                    else:
                        assert np.array_equal(got[sat], np.where(unclamped[sat] > 0, 32767, -32768).astype(np.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_corpus_mono_views(oracle, gpu_parse):
    """decode_files_to_device(mix="mono") on the scale-0.1 corpus subset (writer files, a shipped one-channel file, one file with
    a damaged page: the redo path): views[i] has shape (T_i,), starts on a multiple of four samples of the arena, and equals the
    rule applied to the oracle's unclipped PCM of that file."""
    from nvorbis_amd import corpus
    from tests import c5_corpus, ogg_py
    ws = c5_corpus.writer_setup()
    files = [c5_corpus.corpus_file(ws, i, 0.1) for i in range(5)]
    files.append(open(os.path.join(GOLDEN, "1test.ogg"), "rb").read())  # one channel: the identity
    pages = ogg_py.read_pages(files[2])
    bad = bytearray(files[2])
    pg = pages[len(pages) // 2]
    bad[pg["offset"] + pg["length"] - 3] ^= 0x11
    files[2] = bytes(bad)
    t = {}
    arena, views = corpus.decode_files_to_device(files, device=0, workers=4, gpu_parse=gpu_parse, timings=t, mix="mono")
    assert t.get("files_reindexed") == [2]
    chans = set()
    for i, (v, data) in enumerate(zip(views, files)):
        ref, info = oracle.decode_ogg(data, clip=False)
        ch = info["channels"]
        chans.add(ch)
        want, _ = mix_rule(ref, ch, True)
        assert v.dim() == 1 and v.shape[0] == want.size, (i, tuple(v.shape), want.size)
        if i != 2:  # (the redone file has a tensor of its own)
            assert (v.data_ptr() - arena.data_ptr()) % 16 == 0, i
        assert same_bits(v.cpu().numpy(), want), i
    assert chans == {1, 2}
    del arena, views


@pytest.mark.gpu
def test_mono_twins_reached(tmp_path_factory):
    """(Last in this file: a replay child reports what its tests ran from here.)  Replays of this file's synthetic and resident
    tests in child processes under the kernel-variant toggles; then a bit-exact comparison must have named every one of the 14
    mono twins."""
    seen = set(_SEEN)
    if os.environ.get("NVH_TEST_CHILD"):
        out = os.environ.get("NVH_MONO_SEEN")
        if out:
            with open(out, "w") as fh:
                json.dump(sorted(seen), fh)
        pytest.skip("inside a replay: the parent checks the union")
    from tests.replay import run_children
    d = tmp_path_factory.mktemp("mono_seen")
    children, files = [], []
    for k, toggle in enumerate(["NVH_FPW=1", "NVH_FPW=4", "NVH_EMIT_ALWAYS", "NVH_NO_EMIT", "NVH_NO_COMPACT", "NVH_NO_SLAB", "NVH_GPU_PARSE"]):
        env = dict(os.environ)
        for t in toggle.split("+"):
            key, _, val = t.partition("=")
            env[key] = val or "1"
        env["NVH_TEST_CHILD"] = "1"
        env["NVH_MONO_SEEN"] = str(d / ("%d.json" % k))
        files.append(env["NVH_MONO_SEEN"])
        children.append((["test_pcm_mix.py"], env, ["-k", "synthetic_configs_mono or resident_batch_mono or throwing or has_clipped_follows or twins_reached"]))
    for k in range(0, len(children), 3):  # (three children at a time beside this process)
        run_children(children[k:k + 3], timeout=1500)
    for f in files:
        seen |= set(json.load(open(f)))
    missing = sorted(set(MONO_TWINS) - seen)
    assert not missing, (missing, sorted(seen))

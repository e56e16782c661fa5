"""Channel-map output (nvh_*_map / nvh_*_planar_map), picked inside the emitting kernels' _map twins.

The rule (include/nvorbis_hip.h): output slot j at time t is exactly the sample the un-mapped call of the same format emits for
channel map[j] at time t, clip and 16-bit conversion included.  A map has no arithmetic, so there is no tolerance anywhere: the
expected value is the un-mapped output of the same stream in the same format with its columns picked (and, for float, the
oracle's PCM with its columns picked); every comparison is bit for bit."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the Vorbis-to-WAVE permutations as the issue states them (output slot -> source channel)
WAVE = {1: (0,), 2: (0, 1), 3: (0, 2, 1), 4: (0, 1, 2, 3), 5: (0, 2, 1, 3, 4), 6: (0, 2, 1, 5, 3, 4), 7: (0, 2, 1, 6, 5, 3, 4),
        8: (0, 2, 1, 7, 5, 6, 3, 4)}
SUFFIXES = ["_map", "_s16_map", "_planar_map", "_s16_planar_map"]
# the 16 mapped kernels (as the launcher names them in the timing slots); every one must be reached by this file's runs
MAP_TWINS = [fam + s for fam in ("k_synth8+k_synth8_emit", "k_ola_compact", "k_ola_emit", "k_ola_emit_seq") for s in SUFFIXES]
_SEEN = set()  # twins a bit-exact comparison of this process named
SENTINEL = {np.dtype(np.float32): np.float32(-1234.5), np.dtype(np.int16): np.int16(-7777)}
CLIP = np.float32(0.99999994)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def suffix(dt, planar):
    return ("_s16" if np.dtype(dt) == np.int16 else "") + ("_planar" if planar else "") + "_map"


def maps_for(ch):
    """The maps every wide setup runs: WAVE order, the reversing permutation, and selections of 1, 2 and C - 1 channels that
    drop channel 0 (and are not in ascending order)."""
    out = [WAVE[ch], tuple(range(ch - 1, -1, -1))]
    for oc in (1, 2, ch - 1):
        m = tuple(range(ch - 1, ch - 1 - oc, -1))
        if m not in out:
            out.append(m)
    return [m for m in out if m != tuple(range(ch))]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

NAMES = ("nvh_channel_map_wave", "nvh_stream_synth_map", "nvh_stream_synth_begin_map", "nvh_batch_synth_map",
         "nvh_stream_synth_planar_map", "nvh_stream_synth_begin_planar_map", "nvh_batch_synth_planar_map")


def test_map_entry_points_are_exported_and_declared():
    from nvorbis_amd import native
    L = native.lib()
    hdr = open(os.path.join(ROOT, "include", "nvorbis_hip.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "NativeMethods.cs")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in native.SIGNATURES, name
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern (?:unsafe )?int %s\(" % name, cs), name
    dec = open(os.path.join(ROOT, "csharp", "GpuStreamDecoder.cs")).read()
    assert "channelMap" in dec


def test_wave_map_is_the_table():
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    for ch, want in WAVE.items():
        m = (C.c_int32 * 8)(*([-1] * 8))
        assert L.nvh_channel_map_wave(ch, m) == native.OK
        assert tuple(m[:ch]) == want and all(v == -1 for v in m[ch:]), ch
        assert nv.wave_channel_map(ch) == want
        assert sorted(want) == list(range(ch))
    m = (C.c_int32 * 16)()
    for bad in (0, 9, -1, 255):
        assert L.nvh_channel_map_wave(bad, m) == native.ERR_ARGUMENT
        with pytest.raises(ValueError):
            nv.wave_channel_map(bad)
    assert L.nvh_channel_map_wave(6, None) == native.ERR_ARGUMENT


def _host_stream(nv, oracle, name, packets=12):
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, packets, 3)
    st = nv.Stream(None, pk[0], pk[1], pk[2])  # host-only: the arguments are checked before anything needs a device
    for i in range(3, len(pk)):
        st.push_packet(pk[i], gr[i], fl[i])
    return st


def test_map_entry_points_refuse_bad_arguments(oracle):
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    wr = C.c_int64(0)
    buf = np.zeros(1 << 18, np.float32)
    F32, S16 = native.PCM_F32, native.PCM_S16
    A = native.ERR_ARGUMENT

    def arr(*v):
        return (C.c_int32 * max(len(v), 1))(*v)
    good = arr(0, 2, 1, 5, 3, 4)
    assert L.nvh_stream_synth_map(None, F32, good, 6, buf.ctypes.data, None, 16, C.byref(wr)) == A
    assert L.nvh_stream_synth_begin_map(None, F32, good, 6, buf.ctypes.data, 16, C.byref(wr)) == A
    assert L.nvh_stream_synth_planar_map(None, F32, good, 6, buf.ctypes.data, None, 16, C.byref(wr)) == A
    assert L.nvh_stream_synth_begin_planar_map(None, F32, good, 6, buf.ctypes.data, 16, C.byref(wr)) == A
    assert L.nvh_batch_synth_map(None, F32, good, 6, None, 16) == A
    assert L.nvh_batch_synth_planar_map(None, F32, good, 6, None, 16) == A
    st = _host_stream(nv, oracle, "six_ch_res2_4096")
    try:
        assert st.channels == 6
        _, n = st.pending()
        assert n > 0
        h, p = st._h, buf.ctypes.data

        def every(m, oc, fmt=F32, host=p, dev=None, cap=None, stride=None):
            cap = 6 * n if cap is None else cap
            stride = n if stride is None else stride
            r = [L.nvh_stream_synth_map(h, fmt, m, oc, host, dev, cap, C.byref(wr)),
                 L.nvh_stream_synth_planar_map(h, fmt, m, oc, host, dev, stride, C.byref(wr))]
            if dev is None and host is not None:
                r += [L.nvh_stream_synth_begin_map(h, fmt, m, oc, host, cap, C.byref(wr)),
                      L.nvh_stream_synth_begin_planar_map(h, fmt, m, oc, host, stride, C.byref(wr))]
            return r
        # a null map, count 0, negative, greater than C; a duplicate, a negative entry, an entry >= C
        for m, oc in ((None, 6), (good, 0), (good, -1), (arr(0, 1, 2, 3, 4, 5, 0), 7), (arr(0, 2, 2), 3), (arr(0, -1), 2),
                      (arr(0, 6), 2), (arr(6), 1), (arr(1, 1), 2)):
            assert every(m, oc) == [A] * 4, (m and list(m), oc)
        for fmt in (2, -1, 7):  # unknown formats: the twin's own refusal, for the identity too
            assert every(good, 6, fmt=fmt) == [A] * 4
            assert every(arr(0, 1, 2, 3, 4, 5), 6, fmt=fmt) == [A] * 4
        # both destinations, or neither with PCM to write
        assert every(good, 6, dev=C.c_void_p(4096)) == [A] * 2
        assert every(good, 6, host=None) == [A] * 2
        # too small a capacity (output samples: n * OC) or stride (samples per channel)
        for m, oc in ((good, 6), (arr(5, 4), 2), (arr(3), 1)):
            assert every(m, oc, cap=n * oc - 1, stride=n - 1) == [A] * 4
            for fmt in (F32, S16):  # enough room: past the argument checks the missing device is reported
                assert every(m, oc, fmt=fmt, cap=n * oc, stride=n) == [native.ERR_NO_GPU] * 4
        # a device base not aligned to its sample size; mapped 16-bit PCM need not be 16-byte aligned, un-mapped must be
        assert L.nvh_stream_synth_map(h, F32, good, 6, None, C.c_void_p(4096 + 2), 6 * n, C.byref(wr)) == A
        assert L.nvh_stream_synth_map(h, S16, good, 6, None, C.c_void_p(4096 + 1), 6 * n, C.byref(wr)) == A
        assert L.nvh_stream_synth_map(h, S16, good, 6, None, C.c_void_p(4096 + 2), 6 * n, C.byref(wr)) == native.ERR_NO_GPU
        assert L.nvh_stream_synth_map(h, S16, arr(0, 1, 2, 3, 4, 5), 6, None, C.c_void_p(4096 + 2), 6 * n, C.byref(wr)) == A
        # the Python surface: ValueError before any device work
        for bad in ("WAVE", "vorbis", "", (), (0, 0), (0, 6), (-1,), (0, 1, 2, 3, 4, 5, 0), (0.0, 1), (True, 2), 3, [[0, 1]]):
            with pytest.raises(ValueError):
                st.synth_host(channel_map=bad)
            with pytest.raises(ValueError):
                st.synth_begin(channel_map=bad)
            with pytest.raises(ValueError):
                st.synth_device(0, 0, channel_map=bad)
        with pytest.raises(ValueError):
            st.synth_host(channel_map="wave", mix="mono")
        with pytest.raises(ValueError):
            st.synth_host(channel_map=(1, 0), out=np.zeros(2 * n - 1, np.float32))
    finally:
        st.close()


def test_nine_channels_host(oracle):
    """More than eight channels: a map that is not the identity is NVH_ERR_UNSUPPORTED, the identity is the un-mapped call."""
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    wr = C.c_int64(0)
    buf = np.zeros(1 << 18, np.float32)
    st = _host_stream(nv, oracle, "ch9_res2")
    try:
        assert st.channels == 9
        _, n = st.pending()
        ident = (C.c_int32 * 9)(*range(9))
        swap = (C.c_int32 * 9)(1, 0, 2, 3, 4, 5, 6, 7, 8)
        assert L.nvh_stream_synth_map(st._h, 0, swap, 9, buf.ctypes.data, None, 9 * n, C.byref(wr)) == native.ERR_UNSUPPORTED
        assert L.nvh_stream_synth_planar_map(st._h, 0, swap, 2, buf.ctypes.data, None, n, C.byref(wr)) == native.ERR_UNSUPPORTED
        assert L.nvh_stream_synth_map(st._h, 0, swap, 10, buf.ctypes.data, None, 9 * n, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_map(st._h, 0, ident, 9, buf.ctypes.data, None, 9 * n, C.byref(wr)) == native.ERR_NO_GPU
        with pytest.raises(ValueError):
            st.synth_host(channel_map="wave")
    finally:
        st.close()


def test_reader_and_decoder_reject_bad_maps(ogg_bytes):
    import nvorbis_amd as nv
    data = ogg_bytes["3test"]
    pk, _, _ = nv.demux_ogg(data)
    for bad in ("Wave", "", (), (0, 0), (-1, 0), (0.5,), 1, (0, 1, 2), (2,)):
        with pytest.raises(ValueError):
            nv.VorbisReader(data, ctx=object(), channel_map=bad)  # before the context is used
        with pytest.raises(ValueError):
            nv.StreamDecoder(None, pk, channel_map=bad)
    with pytest.raises(ValueError):
        nv.VorbisReader(data, ctx=object(), channel_map="wave", mix="mono")
    with pytest.raises(ValueError):
        nv.StreamDecoder(None, pk, channel_map=(1, 0), mix="mono")


def test_wave_on_a_stereo_file_is_the_identity(ogg_bytes):
    import nvorbis_amd as nv
    from nvorbis_amd import native
    assert nv.wave_channel_map(2) == (0, 1)
    pk, _, _ = nv.demux_ogg(ogg_bytes["3test"])
    dec = nv.StreamDecoder(None, pk, channel_map="wave")  # host-only
    try:
        assert dec.Channels == 2 and dec.OutputChannels == 2 and dec._channel_map == (0, 1)
    finally:
        dec.close()
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for i in range(3, 9):
            st.push_packet(pk[i], -1, 0)
        _, n = st.pending()
        wr = C.c_int64(0)
        buf = np.zeros(2 * n, np.int16)
        ident = (C.c_int32 * 2)(0, 1)
        L = native.lib()
        # the identity is the un-mapped call, that call's 16-byte rule for 16-bit PCM included
        assert L.nvh_stream_synth_map(st._h, 1, ident, 2, None, C.c_void_p(4096 + 8), 2 * n, C.byref(wr)) == native.ERR_ARGUMENT
        assert L.nvh_stream_synth_map(st._h, 1, ident, 2, buf.ctypes.data, None, 2 * n, C.byref(wr)) == native.ERR_NO_GPU
    finally:
        st.close()


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
        if k.endswith("_map"):
            _SEEN.add(k)


def _toggled():
    return any(os.environ.get(t) for t in ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB", "NVH_FPW", "NVH_NO_EMIT",
                                           "NVH_NO_EMIT8", "NVH_EMIT_ALWAYS", "NVH_GPU_PARSE"))


def _synth_device(torch, st, dt, cmap, planar, off, odd_stride):
    """The pending batch of `st` into a guard-filled device buffer at a base `off` samples in, mapped by `cmap` (None: un-mapped):
    a (samples per channel, output channels) array; asserts that nothing outside what the call reports was written."""
    _, n = st.pending()
    oc = len(cmap) if cmap is not None else st.channels
    dt = np.dtype(dt)
    tdt = torch.float32 if dt == np.float32 else torch.int16
    stride = ((n + 3) & ~3) + (5 if odd_stride else 8)
    size = off + (oc * stride if planar else n * oc) + 64
    buf = torch.full((size,), float(SENTINEL[dt]), dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ptr = buf.data_ptr() + off * dt.itemsize
    if planar:
        got = st.synth_device(ptr, 0, dtype=dt, plane_stride=stride, channel_map=cmap)
    else:
        got = st.synth_device(ptr, n * oc, dtype=dt, channel_map=cmap)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    keep = np.ones(size, bool)
    if planar:
        assert got == n
        for j in range(oc):
            keep[off + j * stride:off + j * stride + got] = False
        out = np.stack([h[off + j * stride:off + j * stride + got] for j in range(oc)], axis=1)
    else:
        assert got == n * oc
        keep[off:off + got] = False
        out = h[off:off + got].reshape(-1, oc)
    assert (h[keep] == SENTINEL[dt]).all(), ("written outside the reported samples", planar, off, stride, n, got)
    return out.copy()


def _decode(nv, torch, ctx, stream, dt, cmap=None, planar=False, bf=1024, offs=(0,), first=None, odd_stride=False, gpu_parse=False,
            clip=True):
    """A stream over the packets, batch by batch (the first batch of `first` frames when given) into device memory at the base
    offsets `offs` in turn: ((samples, output channels) PCM, kernel names per batch, has_clipped)."""
    pk, gr, fl = stream
    st = _stream(nv, ctx, pk)
    if gpu_parse:
        st.set_gpu_parse(True)
    st.set_clip(clip)
    out, kern = [], []
    i, k = 3, 0
    while i < len(pk):
        step = first if (first and i == 3) else bf
        for j in range(i, min(i + step, len(pk))):
            st.push_packet(pk[j], gr[j], fl[j])
        i += step
        if i >= len(pk):
            st.push_end()
        if st.pending()[0] == 0:
            continue
        out.append(_synth_device(torch, st, dt, cmap, planar, offs[k % len(offs)], odd_stride))
        k += 1
        kern.append(st.kernels())
    hc = st.has_clipped()
    oc = len(cmap) if cmap is not None else st.channels
    st.close()
    return (np.concatenate(out) if out else np.zeros((0, oc), dt)), kern, hc


_REF = {}  # (setup, consistent, packets, seed) -> (stream, {dtype: un-mapped (T, C) PCM}); computed once, never modified


def _reference(nv, torch, oracle, ctx, name, consistent, packets=40, seed=11):
    """The stream of a synthetic setup and its un-mapped interleaved output per format (host parser, one aligned batch), the float
    one checked against the oracle."""
    key = (name, consistent, packets, seed)
    if key not in _REF:
        from tests import synth_stream as ss
        stream = ss.filtered_stream(oracle, name, packets, seed + int(consistent), consistent_windows=consistent)
        ref, info = oracle.decode_packets(*stream, clip=True)
        un = {}
        for dt in (np.float32, np.int16):
            un[np.dtype(dt)], _, _ = _decode(nv, torch, ctx, stream, dt)
            un[np.dtype(dt)].setflags(write=False)
        if not any(os.environ.get(t) for t in ("NVH_UNFUSED", "NVH_NO_FUSED_IMDCT", "NVH_NO_COMPACT", "NVH_NO_SLAB")) or "floor0" not in name:
            assert same_bits(un[np.dtype(np.float32)], ref.reshape(-1, info["channels"])), name
        _REF[key] = (stream, un)
    return _REF[key]


# the destinations a mapped decode runs with: (batch frames, base offsets in samples, first batch, odd plane stride) -- one aligned
# batch; batches of 13 frames at bases in turn aligned and one sample off (the later batch's position, out_pos odd in a contiguous
# destination: the fall-back to the per-frame overlap kernel) with a plane stride that is no multiple of four; a first batch of 3
DESTS = [(1024, (0,), None, False), (13, (0, 1), None, True), (16, (0,), 3, False)]
WIDE = ["three_ch_res2_misaligned", "ch4_res1", "ch5_res2", "six_ch_res2_4096", "ch7_res1", "ch8_res2"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", WIDE)
@pytest.mark.parametrize("consistent", [True, False])
def test_wide_setups_mapped(oracle, gpu_ctx, name, consistent):
    """Three to eight channels, consistent and inconsistent window flags: the WAVE map, the reversing permutation and selections
    of 1, 2 and C - 1 channels that drop channel 0, both formats, both layouts, both parsers, aligned and fall-back destinations:
    every output equals the un-mapped output of the same format with its columns picked (for float: the oracle's), nothing is
    written outside the reported samples, and every batch names a kernel of the call's _map form."""
    torch = _torch()
    import nvorbis_amd as nv
    stream, un = _reference(nv, torch, oracle, gpu_ctx, name, consistent)
    ch = un[np.dtype(np.float32)].shape[1]
    for cmap in maps_for(ch):
        for dt in (np.float32, np.int16):
            want = un[np.dtype(dt)][:, list(cmap)]
            for planar in (False, True):
                for gpu_parse in (False, True):
                    for bf, offs, first, odd in (DESTS if not gpu_parse else DESTS[:2]):
                        got, kern, _ = _decode(nv, torch, gpu_ctx, stream, dt, cmap, planar, bf, offs, first, odd, gpu_parse)
                        assert same_bits(got, want), (name, consistent, cmap, dt, planar, gpu_parse, bf)
                        sfx = suffix(dt, planar)
                        assert all(any(k.endswith(sfx) for k in ks) for ks in kern), (sfx, kern)
                        _note(k for ks in kern for k in ks)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stereo_res1_coupled", "stereo_8192"])
def test_stereo_mapped(oracle, gpu_ctx, name):
    """Stereo: the swap and either channel alone.  Blocks up to 2048 run without paired emission (k_synth + the mapped
    k_ola_compact), blocks of 8192 take the wide kernel."""
    torch = _torch()
    import nvorbis_amd as nv
    stream, un = _reference(nv, torch, oracle, gpu_ctx, name, True)
    for cmap in ((1, 0), (0,), (1,)):
        for dt in (np.float32, np.int16):
            want = un[np.dtype(dt)][:, list(cmap)]
            for planar in (False, True):
                for bf, offs, first, odd in DESTS:
                    got, kern, _ = _decode(nv, torch, gpu_ctx, stream, dt, cmap, planar, bf, offs, first, odd)
                    assert same_bits(got, want), (name, cmap, dt, planar, bf)
                    _note(k for ks in kern for k in ks)
                    sfx = suffix(dt, planar)
                    if _toggled():
                        continue
                    for ks in kern:
                        if name == "stereo_8192":
                            assert ks[1].startswith("k_synth8") and (ks[1].endswith(sfx) or ks[3].endswith(sfx)), ks
                        else:
                            assert ks[1] == "k_synth" and ks[3] == "k_ola_compact" + sfx, ks


@pytest.mark.gpu
def test_identity_map_is_the_unmapped_call(oracle, gpu_ctx):
    torch = _torch()
    import nvorbis_amd as nv
    for name in ("six_ch_res2_4096", "stereo_res1_coupled"):
        stream, un = _reference(nv, torch, oracle, gpu_ctx, name, True)
        ch = un[np.dtype(np.float32)].shape[1]
        for dt in (np.float32, np.int16):
            for planar in (False, True):
                a, ka, _ = _decode(nv, torch, gpu_ctx, stream, dt, None, planar)
                b, kb, _ = _decode(nv, torch, gpu_ctx, stream, dt, tuple(range(ch)), planar)
                assert same_bits(a, b) and same_bits(a, un[np.dtype(dt)])
                assert ka == kb and not any(k.endswith("_map") for ks in kb for k in ks), (ka, kb)


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_pipelined_flights_alternate(oracle, gpu_ctx, gpu_parse):
    """synth_begin / synth_end alternating mapped, un-mapped, planar-mapped and mono flights on one six-channel stream, so that
    the carried tail crosses every pair of forms: each flight equals its form of the un-mapped output of that batch."""
    torch = _torch()
    import nvorbis_amd as nv
    stream, un = _reference(nv, torch, oracle, gpu_ctx, "six_ch_res2_4096", True, packets=99)
    pk, gr, fl = stream
    forms = ["map_f32", "il_f32", "pmap_s16", "mono_f32", "map_s16"]
    plan = [f for a in forms for b in forms if a != b for f in (a, b)]
    cmaps = {"map_f32": WAVE[6], "pmap_s16": (5, 0, 2), "map_s16": (3, 1)}

    def run(mapped):
        st = _stream(nv, gpu_ctx, pk)
        if gpu_parse:
            st.set_gpu_parse(True)
        cuts = np.linspace(3, len(pk), len(plan) + 1).astype(int)
        got, out = [], 0
        for k, form in enumerate(plan):
            for i in range(cuts[k], cuts[k + 1]):
                st.push_packet(pk[i], gr[i], fl[i])
            if k == len(plan) - 1:
                st.push_end()
            n = st.pending()[1]
            dt = np.int16 if form.endswith("s16") else np.float32
            cm = cmaps.get(form) if mapped else None
            planar = form.startswith("pmap")
            exp = st.synth_begin(dtype=dt, planar=planar, mix="mono" if form.startswith("mono") else None, channel_map=cm)
            if not form.startswith("mono"):
                assert exp == (n if planar else n * (len(cm) if cm else 6))
            out += 1
            if out == 2:
                got.append(st.synth_end().copy())
                out -= 1
        while out:
            got.append(st.synth_end().copy())
            out -= 1
        st.close()
        return got
    mapped, plain = run(True), run(False)
    pos = 0
    for form, g, u in zip(plan, mapped, plain):
        cm = cmaps.get(form)
        if form.startswith("pmap"):
            assert same_bits(g, np.ascontiguousarray(u[list(cm), :])), form
            n = u.shape[1]
            assert same_bits(np.ascontiguousarray(u.T), un[np.dtype(np.int16)][pos:pos + n])
        elif cm:
            assert same_bits(g, np.ascontiguousarray(u.reshape(-1, 6)[:, list(cm)]).reshape(-1)), form
            n = u.size // 6
            assert same_bits(u.reshape(-1, 6), un[u.dtype][pos:pos + n])
        else:
            assert same_bits(g, u), form
            n = u.size // (1 if form.startswith("mono") else 6)
        pos += n
    assert pos == un[np.dtype(np.float32)].shape[0]


@pytest.mark.gpu
def test_resident_batch_two_maps(oracle, gpu_ctx):
    """A resident batch synthesised with two different maps, each twice, then un-mapped: each launch equals the un-mapped output
    with its columns picked; the guard behind the batch keeps its value; a short capacity is refused."""
    torch = _torch()
    import nvorbis_amd as nv
    from nvorbis_amd import native
    stream, un = _reference(nv, torch, oracle, gpu_ctx, "six_ch_res2_4096", True)
    pk, gr, fl = stream
    st = _stream(nv, gpu_ctx, pk)
    for i in range(3, len(pk)):
        st.push_packet(pk[i], gr[i], fl[i])
    st.push_end()
    b = st.upload_batch()
    _OPEN.append(b)
    n = b.samples
    for dt, tdt in ((np.float32, torch.float32), (np.int16, torch.int16)):
        u = un[np.dtype(dt)]
        assert u.shape[0] == n
        for cmap in (WAVE[6], (4, 1), WAVE[6], None, (5,)):
            oc = len(cmap) if cmap else 6
            for planar in (False, True):
                buf = torch.full((n * oc + 64,), float(SENTINEL[np.dtype(dt)]), dtype=tdt, device="cuda")
                torch.cuda.synchronize()
                for rep in range(2):
                    b.synth(buf.data_ptr(), n * oc, dtype=dt, plane_stride=n if planar else None, channel_map=cmap)
                    ks = b.kernels()
                    gpu_ctx.synchronize()
                    h = buf.cpu().numpy()
                    got = h[:n * oc].reshape(oc, n).T if planar else h[:n * oc].reshape(n, oc)
                    want = u[:, list(cmap)] if cmap else u
                    assert same_bits(np.ascontiguousarray(got), np.ascontiguousarray(want)), (dt, cmap, planar, rep)
                    assert (h[n * oc:] == SENTINEL[np.dtype(dt)]).all()
                    assert any(k.endswith("_map") for k in ks) == (cmap is not None), ks
                    _note(ks)
        with pytest.raises(native.NvhError) as e:
            b.synth(0, 2 * n - 1, dtype=dt, channel_map=(4, 1))
        assert e.value.code == native.ERR_ARGUMENT


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_reader_wave_on_a_six_channel_ogg(oracle, gpu_ctx, gpu_parse):
    """VorbisReader(channel_map="wave") on a six-channel Ogg file: read_all and partial reads, both formats and layouts,
    equal the un-mapped reader's output (float interleaved: the oracle's) in WAVE order."""
    torch = _torch()
    import nvorbis_amd as nv
    from tests import ogg_py
    stream, _ = _reference(nv, torch, oracle, gpu_ctx, "six_ch_res2_4096", True)
    data = ogg_py.write_ogg(*stream[:2])
    ref, info = oracle.decode_ogg(data, clip=True)
    assert info["channels"] == 6
    w = list(WAVE[6])
    opened = []

    def reader(**kw):
        r = nv.VorbisReader(data, ctx=gpu_ctx, gpu_parse=gpu_parse, batch_frames=7, **kw)
        opened.append(r)
        return r
    try:
        for fmt, dt in (("f32", np.float32), ("s16", np.int16)):
            plain = reader(sample_format=fmt).read_all().reshape(-1, 6)
            if dt == np.float32:
                assert same_bits(plain, ref.reshape(-1, 6))
            for cmap in ("wave", (5, 3)):
                cols = w if cmap == "wave" else list(cmap)
                want = np.ascontiguousarray(plain[:, cols])
                r = reader(sample_format=fmt, channel_map=cmap)
                assert r.Channels == 6 and r.OutputChannels == len(cols)
                assert same_bits(r.read_all().reshape(-1, len(cols)), want), (fmt, cmap)
                assert r.SamplePosition == info["position"]
                r = reader(sample_format=fmt, layout="planar", channel_map=cmap)
                got = r.read_all()
                assert got.shape[0] == len(cols) and same_bits(np.ascontiguousarray(got.T), want), (fmt, cmap)
                # partial reads of odd sizes at an odd offset of the buffer
                r = reader(sample_format=fmt, channel_map=cmap)
                parts, buf = [], np.zeros(4000, dt)
                rng = np.random.default_rng(4)
                while True:
                    k = int(rng.integers(1, 600)) * len(cols)
                    n = r.ReadSamples(buf, 3, k)
                    if n <= 0:
                        break
                    parts.append(buf[3:3 + n].copy())
                assert same_bits(np.concatenate(parts).reshape(-1, len(cols)), want), (fmt, cmap)
    finally:
        for r in opened:
            r.close()


# (setup, seed, packets of the prefix) from tests/test_pcm_mix.py's clip cases: streams where one channel alone leaves [-1, 1]
CLIP_CASES = [("three_ch_res2_misaligned", 1, 5), ("ch4_res1", 4, 7), ("ch4_res1", 1, 14)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,k", CLIP_CASES)
def test_has_clipped_follows_the_emitted_samples(oracle, gpu_ctx, name, seed, k):
    """A stream prefix in which some channels leave [-1, 1] and others do not (the premise, from the oracle): a map that keeps
    only channels that stay inside leaves HasClipped false, a map that keeps a channel that leaves sets it -- in both formats
    and layouts, aligned and fall-back destinations."""
    torch = _torch()
    import nvorbis_amd as nv
    from tests import synth_stream as ss
    pk, gr, fl = ss.filtered_stream(oracle, name, 40, seed)
    stream = (pk[:k], gr[:k], fl[:k])
    ref, info = oracle.decode_packets(*stream, clip=False)
    ch = info["channels"]
    loud = (np.abs(ref.reshape(-1, ch)) > CLIP).any(axis=0)
    assert loud.any() and not loud.all(), (name, seed, k, loud)  # (the premise)
    quiet = tuple(int(c) for c in np.nonzero(~loud)[0][::-1])
    clipped, _ = oracle.decode_packets(*stream, clip=True)
    clipped = clipped.reshape(-1, ch)
    for cmap, want_flag in ((quiet, False), (quiet + (int(np.nonzero(loud)[0][0]),), True), ((int(np.nonzero(loud)[0][-1]),), True)):
        for planar in (False, True):
            for bf, offs, first, odd in DESTS:
                got, kern, hc = _decode(nv, torch, gpu_ctx, stream, np.float32, cmap, planar, bf, offs, first, odd)
                assert same_bits(got, np.ascontiguousarray(clipped[:, list(cmap)])), (name, cmap, planar, bf)
                assert hc == want_flag, (name, seed, cmap, planar, bf, kern)
                _note(x for ks in kern for x in ks)
            got, kern, hc = _decode(nv, torch, gpu_ctx, stream, np.int16, cmap, planar)
            assert hc == want_flag, (name, seed, cmap, planar, kern)


@pytest.mark.gpu
def test_nine_channels_gpu(oracle, gpu_ctx):
    torch = _torch()
    import nvorbis_amd as nv
    from nvorbis_amd import native
    stream, un = _reference(nv, torch, oracle, gpu_ctx, "ch9_res2", True)
    got, kern, _ = _decode(nv, torch, gpu_ctx, stream, np.float32, tuple(range(9)))
    assert same_bits(got, un[np.dtype(np.float32)]) and not any(k.endswith("_map") for ks in kern for k in ks)
    pk, gr, fl = stream
    st = _stream(nv, gpu_ctx, pk)
    for i in range(3, 12):
        st.push_packet(pk[i], gr[i], fl[i])
    for cmap in ((1, 0, 2, 3, 4, 5, 6, 7, 8), (8,), (0, 1)):
        with pytest.raises(native.NvhError) as e:
            st.synth_host(channel_map=cmap)
        assert e.value.code == native.ERR_UNSUPPORTED
    n = st.pending()[1]
    assert st.synth_host(channel_map=tuple(range(9))).size == 9 * n  # the identity is accepted


@pytest.mark.gpu
def test_map_twins_reached(tmp_path_factory):
    """(Last in this file: a replay child reports what its tests ran from here.)  Replays of this file's synthetic tests in child
    processes under the kernel-variant toggles; then a bit-exact comparison must have named every one of the 16 mapped kernels."""
    seen = set(_SEEN)
    if os.environ.get("NVH_TEST_CHILD"):
        out = os.environ.get("NVH_MAP_SEEN")
        if out:
            with open(out, "w") as fh:
                json.dump(sorted(seen), fh)
        pytest.skip("inside a replay: the parent checks the union")
    from tests.replay import run_children
    d = tmp_path_factory.mktemp("map_seen")
    children, files = [], []
    for k, toggle in enumerate(["NVH_EMIT_ALWAYS", "NVH_NO_EMIT8", "NVH_NO_SLAB", "NVH_NO_COMPACT"]):
        env = dict(os.environ)
        env[toggle] = "1"
        env["NVH_TEST_CHILD"] = "1"
        env["NVH_MAP_SEEN"] = str(d / ("%d.json" % k))
        files.append(env["NVH_MAP_SEEN"])
        children.append((["test_pcm_map.py"], env, ["-k", "wide_setups_mapped or stereo_mapped or resident_batch or has_clipped_follows or twins_reached"]))
    for k in range(0, len(children), 2):  # (two children at a time beside this process)
        run_children(children[k:k + 2], timeout=1500)
    for f in files:
        seen |= set(json.load(open(f)))
    missing = sorted(set(MAP_TWINS) - seen)
    assert not missing, (missing, sorted(seen))

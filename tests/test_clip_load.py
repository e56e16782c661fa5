"""The clip calls' host stage: every clip is read, demuxed and probed once per call (clips._load_clips), and its errors surface
clip by clip in one order -- the clip's headers (NvhError under the public call's own name), a channel map that does not fit
it, a rate the resampler refuses -- before the next clip is looked at and before any device is touched."""
import builtins
import os

import numpy as np
import pytest

from tests import ogg_py

OGG_FILES = ("1test", "2test", "3test", "issue6test")


def two_packets(data):
    """An Ogg stream that ends behind the comment header of `data`: two packets, no setup."""
    import nvorbis_amd as nv
    pa = nv.demux_ogg_array(data, 0)
    pw = ogg_py.PageWriter(0x4E56)
    pw.add_packet(pa[0], 0, flush=True)
    pw.add_packet(pa[1], 0, flush=True)
    return pw.finish()


def the_calls(nv):
    return (("decode_clips", lambda clips, **kw: nv.decode_clips(clips)),
            ("decode_clip_rows", lambda clips, **kw: nv.decode_clip_rows(clips, 16, **kw)),
            ("decode_clip_features", lambda clips, **kw: nv.decode_clip_features(clips, 16, **kw)))


def counting(monkeypatch, fn):
    """clips.demux_ogg_array behind a wrapper that counts its calls."""
    from nvorbis_amd import clips
    calls = []

    def wrapper(*a, **kw):
        calls.append(1)
        return fn(*a, **kw)
    monkeypatch.setattr(clips, "demux_ogg_array", wrapper)
    return calls


def test_load_clips_records(ogg_bytes):
    import nvorbis_amd as nv
    from nvorbis_amd import clips
    files = [ogg_bytes[n] for n in OGG_FILES]
    for want_index in (False, True):
        recs = clips._load_clips(files, "decode_clip_rows", want_index=want_index)
        assert len(recs) == len(files)
        for data, r in zip(files, recs):
            pa = nv.demux_ogg_array(data, 0)
            st = nv.Stream(None, pa[0], pa[1], pa[2])
            try:
                assert (r.channels, r.rate) == (st.channels, st.sample_rate)
                assert len(r.packets) == len(pa) and r.key == (pa[0], pa[2])
                if want_index:
                    for got, want in zip(r.index, st.index_packets(pa, 3)):
                        assert np.array_equal(got, want)
                else:
                    assert r.index is None
            finally:
                st.close()


def test_header_errors_carry_the_calls_own_name(ogg_bytes):
    import nvorbis_amd as nv
    from nvorbis_amd import native
    good = ogg_bytes["3test"]
    for name, call in the_calls(nv):
        with pytest.raises(native.NvhError) as e:
            call([good, two_packets(good)])
        assert e.value.clip == 1
        assert str(e.value).startswith("%s: clip 1: headers" % name), str(e.value)


def test_a_clips_own_errors_come_before_the_next_clip(ogg_bytes):
    """Clip 0's refused rate (ValueError) hides clip 1's headers; the other way round the headers (NvhError, clip 0) come first."""
    import nvorbis_amd as nv
    from nvorbis_amd import clips, native
    refused = 44101
    for n in OGG_FILES:
        pa = nv.demux_ogg_array(ogg_bytes[n], 0)
        st = nv.Stream(None, pa[0], pa[1], pa[2])
        st.close()
        with pytest.raises(ValueError):
            clips.resample_plan(st.sample_rate, refused)
    good = ogg_bytes["3test"]
    for name, call in the_calls(nv)[1:]:
        with pytest.raises(ValueError):
            call([good, two_packets(good)], sample_rate=refused)
        with pytest.raises(native.NvhError) as e:
            call([two_packets(good), good], sample_rate=refused)
        assert e.value.clip == 0 and str(e.value).startswith("%s: clip 0: headers" % name)


def test_features_demux_every_clip_once_on_the_host(ogg_bytes, monkeypatch):
    import nvorbis_amd as nv
    calls = counting(monkeypatch, nv.demux_ogg_array)
    files = [ogg_bytes["3test"], ogg_bytes["issue6test"], ogg_bytes["3test"]]
    with pytest.raises(ValueError, match="center=False needs length >= n_fft"):  # behind the load, before a device
        nv.decode_clip_features(files, 256, center=False)
    assert len(calls) == len(files)


@pytest.mark.gpu
def test_features_read_every_clip_once(gpu_ctx, ogg_bytes, tmp_path, monkeypatch):
    """One read, one demux per clip and call; and the records keep the clips' order through the rows' gather: the same two
    clips given the other way round give the same features, bit for bit."""
    import nvorbis_amd as nv
    path = str(tmp_path / "1test.ogg")
    with open(path, "wb") as fh:
        fh.write(ogg_bytes["1test"])
    calls, opened = counting(monkeypatch, nv.demux_ogg_array), []
    real_open = builtins.open

    def spy(file, *a, **kw):
        if isinstance(file, (str, os.PathLike)) and os.fspath(file) == path:
            opened.append(1)
        return real_open(file, *a, **kw)
    monkeypatch.setattr(builtins, "open", spy)
    feats, valid, frames = nv.decode_clip_features([ogg_bytes["1test"], path], 4096, [0, 1024], ctx=gpu_ctx, normalize="mean")
    assert (len(calls), len(opened)) == (2, 1)
    monkeypatch.undo()
    back, valid2, frames2 = nv.decode_clip_features([path, ogg_bytes["1test"]], 4096, [1024, 0], ctx=gpu_ctx, normalize="mean")
    a, b = feats.cpu().numpy().view(np.uint32), back.cpu().numpy().view(np.uint32)[::-1]
    assert a.shape == (2, 1, 80, 4096 // 160 + 1) and not np.array_equal(a[0], a[1])
    assert np.array_equal(a, b) and np.array_equal(valid, valid2[::-1]) and np.array_equal(frames, frames2[::-1])

"""Damaged Ogg clips through the clip calls (nvorbis_amd/clips.py): decode_clips, decode_clip_rows, decode_clip_features.

A clip that lost a page reaches the decoder with a resync flag on the packet behind the gap (StreamDecoder.cs:481-484: the decoder
picks up a new position there, and the overlap with the frame before is gone).  In a clip batch that packet sits in the middle of
a segment of a shared batch, so the reset happens inside the frame-group kernels, on either frame of a two-frame group.  Every
comparison is uint32 equality with oracle.decode_ogg of the same damaged bytes (for features: the numpy rules of
tests/test_mel_plan.py over the oracle's rows); there is no tolerance anywhere."""
import numpy as np
import pytest

from tests.test_clip_batches import _torch, mix_rule, same_bits, to_s16
from tests.test_ogg_damage import _damage, _stream
from tests.test_segment_clipped import over

pytestmark = pytest.mark.gpu

PAGE = 30  # the damaged page of a clip (page 2 + j holds audio packet j: one packet a page), and PAGE + 1
KINDS = ("crc", "drop", "junk", "seq")
_SETUP = []


class _OnPage:
    """A generator for _damage whose first draw -- the page -- is given; the other draws are a seeded generator's."""

    def __init__(self, page, seed):
        self.page, self.rng = page, np.random.default_rng(seed)

    def integers(self, *args, **kw):
        if self.page is not None:
            page, self.page = self.page, None
            return page
        return self.rng.integers(*args, **kw)


def clip_setup(oracle, ogg_bytes):
    """The clips of every test here, built once and never modified: dict(names, files {name: bytes}, refs {name: (clipped PCM,
    info, unclipped PCM)}, resync {name: audio packet index of the first resync packet, or None}, counts {name: audio packets},
    swap: a clip both readers refuse).  All share the headers of 3test.ogg; 60 frames (61 for one healthy clip), one packet a
    page, so that one lost page is one lost packet."""
    import nvorbis_amd as nv
    if _SETUP:
        return _SETUP[0]
    base, pages = _stream(ogg_bytes, seed=61, frames=60, page_packets=1)
    assert len(pages) == 62
    files = {"healthy": base}
    for kind in KINDS:
        for page in (PAGE, PAGE + 1):
            files["%s@%d" % (kind, page)] = _damage(base, pages, kind, _OnPage(page, page))
    files["truncate@45"] = _damage(base, pages, "truncate", _OnPage(45, 45))
    files["healthy61"] = _stream(ogg_bytes, seed=62, frames=61, page_packets=1)[0]
    refs, resync, counts = {}, {}, {}
    for name, data in files.items():
        pcm, info = oracle.decode_ogg(data)
        raw, _ = oracle.decode_ogg(data, clip=False)
        assert info["channels"] == 2 and info["sample_rate"] == 44100 and pcm.size == raw.size > 0
        assert info["has_clipped"] == over(raw)
        pcm.setflags(write=False)
        raw.setflags(write=False)
        refs[name] = (pcm, info, raw)
        _, _, fl = nv.demux_ogg(data)
        at = [i - 3 for i in range(3, len(fl)) if fl[i] & 2]
        resync[name], counts[name] = (at[0] if at else None), len(fl) - 3
    for kind in KINDS:  # the resync packet of PAGE + 1 is the packet behind PAGE's; neither is a clip's first or last packet
        a, b = resync["%s@%d" % (kind, PAGE)], resync["%s@%d" % (kind, PAGE + 1)]
        assert a is not None and b == a + 1 and 20 < a < 40, (kind, a, b)
    assert resync["healthy"] is None and resync["truncate@45"] is None and refs["truncate@45"][0].size < refs["healthy"][0].size
    swap = _damage(base, pages, "swap", _OnPage(PAGE, 1))
    with pytest.raises(RuntimeError):
        oracle.decode_ogg(swap)
    _SETUP.append(dict(names=list(files), files=files, refs=refs, resync=resync, counts=counts, swap=swap))
    return _SETUP[0]


def batch_order(setup):
    """The clips of a decode_clips call: every clip, an odd number of frames, every clip again -- each resync packet then falls
    once on an even and once on an odd frame of its batch (batches are cut every batch_frames frames, an even number)."""
    names, counts = setup["names"], setup["counts"]
    spacer = "healthy61" if sum(counts[n] for n in names) % 2 == 0 else "healthy"
    order = names + [spacer] + names
    seen, at = {}, 0
    for n in order:
        if setup["resync"][n] is not None:
            seen.setdefault(n, set()).add((at + setup["resync"][n]) % 2)
        at += counts[n]
    assert seen and all(v == {0, 1} for v in seen.values()), seen
    return order


@pytest.mark.parametrize("batch_frames", [16, 4096])
def test_decode_clips(oracle, gpu_ctx, ogg_bytes, batch_frames):
    """Every clip is the oracle's decode of its bytes, with both packet parsers, as f32 and under the mono mix, and the per-clip
    clip flags are what the oracle's PCM says: HasClipped for f32, a mixed sample beyond the clip value for the mix."""
    _torch()
    import nvorbis_amd as nv
    s = clip_setup(oracle, ogg_bytes)
    order = batch_order(s)
    files = [s["files"][n] for n in order]
    for gpu_parse in (True, False):
        got, clipped = nv.decode_clips(files, ctx=gpu_ctx, batch_frames=batch_frames, gpu_parse=gpu_parse, return_clipped=True)
        bad = [(i, n) for i, (n, g) in enumerate(zip(order, got)) if not same_bits(g, s["refs"][n][0])]
        assert not bad, ("f32", batch_frames, gpu_parse, bad)
        assert np.array_equal(clipped, [over(s["refs"][n][2]) for n in order]), (batch_frames, gpu_parse, clipped)
    got, clipped = nv.decode_clips(files, ctx=gpu_ctx, batch_frames=batch_frames, mix="mono", return_clipped=True)
    want = [mix_rule(s["refs"][n][2], 2, True) for n in order]
    bad = [(i, n) for i, (n, g, w) in enumerate(zip(order, got, want)) if not same_bits(g, w)]
    assert not bad, ("mono", batch_frames, bad)
    beyond = [over(mix_rule(s["refs"][n][2], 2, False)) for n in order]
    assert np.array_equal(clipped, beyond), (batch_frames, clipped, beyond)


def test_decode_clips_s16(oracle, gpu_ctx, ogg_bytes):
    """The same clips as 16-bit PCM: ov_read's conversion of the oracle's decode."""
    _torch()
    import nvorbis_amd as nv
    s = clip_setup(oracle, ogg_bytes)
    order = batch_order(s)
    got = nv.decode_clips([s["files"][n] for n in order], ctx=gpu_ctx, batch_frames=16, sample_format="s16")
    bad = [(i, n) for i, (n, g) in enumerate(zip(order, got)) if not same_bits(g, to_s16(s["refs"][n][0]))]
    assert not bad, bad


def row_calls(setup, length):
    """[(name, start)]: per clip a window that ends before the resync packet's first sample, one across it (an odd start), one
    across the end of the (shortened) stream and one behind it; a clip without a resync packet: around its middle."""
    import nvorbis_amd as nv
    out = []
    for name in setup["names"]:
        pa = nv.demux_ogg_array(setup["files"][name], 0)
        st = nv.Stream(None, pa[0], pa[1], pa[2])
        try:
            _, em, _, total = st.index_packets(pa, 3)
        finally:
            st.close()
        assert 2 * total == setup["refs"][name][0].size
        r = setup["resync"][name]
        edge = int(em[(r if r is not None else len(em) // 2) - 1])  # samples emitted in front of that packet
        assert length + 600 < edge < total - length
        out += [(name, (edge - length - 500) & ~3), (name, edge - length // 2 + 1), (name, total - length // 3), (name, total + 5)]
    return out


@pytest.mark.parametrize("length,gpu_parse", [(4000, True), (4000, False), (1001, True)])
def test_decode_clip_rows(oracle, gpu_ctx, ogg_bytes, length, gpu_parse):
    """Rows in front of the resync, across it, across the end of the shortened stream and behind it: each is the oracle's PCM cut
    and zero-padded, and valid and the per-row clip flags agree (tests/test_resample_rows.py: want_row)."""
    _torch()
    import nvorbis_amd as nv
    from tests.test_resample_rows import want_row
    s = clip_setup(oracle, ogg_bytes)
    calls = row_calls(s, length)
    files = {"damaged/" + n: d for n, d in s["files"].items()}  # (want_row's caches are keyed by name)
    ref = [want_row(oracle, files, "damaged/" + n, 44100, 44100, "f32", start, length) for n, start in calls]
    (rows, valid), clipped = nv.decode_clip_rows([s["files"][n] for n, _ in calls], length, [start for _, start in calls], ctx=gpu_ctx,
                                                 batch_frames=16, gpu_parse=gpu_parse, return_clipped=True)
    want_valid = np.asarray([v for _, v, _, _ in ref], np.int64)
    assert np.array_equal(valid, want_valid) and valid.dtype == np.int64
    assert (valid == 0).any() and (valid == length).any() and ((valid > 0) & (valid < length)).any()
    assert rows.shape == (len(calls), length, 2)
    bad = [calls[i] for i in range(len(calls)) if not same_bits(rows[i], ref[i][0])]
    assert not bad, (length, gpu_parse, bad)
    assert np.array_equal(clipped, [d for _, _, d, _ in ref]), (length, gpu_parse, clipped)


def test_decode_clip_features(oracle, gpu_ctx, ogg_bytes):
    """One call with the default keywords over the same rows: features and valid_frames are the numpy rules applied to the oracle's
    rows (tests/test_mel_rows.py: want_features)."""
    _torch()
    import nvorbis_amd as nv
    from tests.test_mel_rows import LENGTH, want_features
    s = clip_setup(oracle, ogg_bytes)
    calls = row_calls(s, LENGTH)
    files = {"damaged/" + n: d for n, d in s["files"].items()}
    mel = dict(n_fft=512, win_length=400, hop=160, n_mels=80, mel_scale="htk", norm=None, scale="ln")  # the defaults, spelled out
    ref = [want_features(oracle, files, "damaged/" + n, 44100, 44100, "f32", start, True, mel) for n, start in calls]
    feats, valid, valid_frames = nv.decode_clip_features([s["files"][n] for n, _ in calls], LENGTH, [start for _, start in calls], ctx=gpu_ctx)
    want = np.stack([f for f, _, _, _ in ref]).transpose(0, 1, 3, 2)  # (N, channels, bands, frames): band_major
    F = want.shape[3]
    assert feats.is_cuda and tuple(feats.shape) == want.shape == (len(calls), 2, 80, LENGTH // 160 + 1)
    want_vf = np.asarray([v for _, _, v, _ in ref], np.int64)
    assert np.array_equal(valid, [v for _, v, _, _ in ref]) and np.array_equal(valid_frames, want_vf) and valid_frames.dtype == np.int64
    assert (want_vf == 0).any() and (want_vf == F).any() and ((want_vf > 0) & (want_vf < F)).any()
    host = feats.cpu().numpy()
    bad = [calls[i] for i in range(len(calls)) if not same_bits(np.ascontiguousarray(host[i]), np.ascontiguousarray(want[i]))]
    assert not bad, bad


def test_a_refused_clip_names_itself(oracle, gpu_ctx, ogg_bytes):
    """Two exchanged pages: the checked demultiplexer refuses the clip, every clip call raises NvhError with the clip's index, and
    the same call without it gives the oracle's PCM afterwards."""
    _torch()
    import nvorbis_amd as nv
    from nvorbis_amd import native
    s = clip_setup(oracle, ogg_bytes)
    names = ["healthy", "crc@%d" % PAGE, "healthy61"]
    good = [s["files"][n] for n in names]
    with_swap = good[:2] + [s["swap"]] + good[2:]
    for call in (lambda f: nv.decode_clips(f, ctx=gpu_ctx, batch_frames=16),
                 lambda f: nv.decode_clip_rows(f, 1000, ctx=gpu_ctx, batch_frames=16),
                 lambda f: nv.decode_clip_features(f, 1000, ctx=gpu_ctx, batch_frames=16)):
        with pytest.raises(native.NvhError) as e:
            call(with_swap)
        assert e.value.clip == 2 and e.value.code == native.ERR_INVALID_DATA and "clip 2" in str(e.value)
    got = nv.decode_clips(good, ctx=gpu_ctx, batch_frames=16)
    assert all(same_bits(g, s["refs"][n][0]) for n, g in zip(names, got))
    rows, valid = nv.decode_clip_rows(good, 1000, ctx=gpu_ctx, batch_frames=16)
    assert np.array_equal(valid, [1000] * 3)
    assert all(same_bits(rows[i].reshape(-1), s["refs"][n][0][:2000]) for i, n in enumerate(names))

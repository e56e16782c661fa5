"""Per-row normalisation of features on the GPU: k_fnorm_rows alone on synthetic features, and the normalisation keywords of
decode_clip_features against the CPU oracle (include/nvorbis_hip.h states the rule under nvh_fnorm_rows).

The reference is the rule in numpy (tests/test_fnorm_plan.py: rule_fnorm, written from the header's text).  No tolerance anywhere:
everything is compared as uint32."""
import numpy as np
import pytest

from tests.test_clip_batches import _torch, same_bits
from tests.test_fnorm_plan import AXES, F32, MODES, make_fdesc, normal_features, rule_fnorm
from tests.test_mel_rows import FEATURE_CALLS, LENGTH, feature_call, feature_rows, want_features

SENT = F32(-1234.5)
GAP = F32(1e30)  # what lies between the source's rows and channels: never read
# (F, B).  (F | 1) * B <= 19952 floats is normalised out of LDS, anything larger re-reads its source (nvh_fnorm_check's header text:
# NVH_FNORM_RESIDENT_FLOATS): (130, 256) and (250, 80) re-read -- more than one tile of 64 frames, the last one partial -- and every
# other shape is resident, (249, 80) being the largest F at 80 bands that is.
KERNEL_SHAPES = [(1, 1), (2, 8), (63, 80), (64, 80), (65, 80), (130, 256), (257, 40), (249, 80), (250, 80)]
PARAMS = dict(eps=1e-3, pad_value=-7.5, peak_range=3.0, peak_offset=4.0, peak_gain=0.3)


def takes_lds_path(F, B):
    from nvorbis_amd import native
    return (F | 1) * B <= native.FNORM_RESIDENT_FLOATS


def strides(F, B, band_major):
    """(frame stride, band stride) of one (row, channel) block of F * B floats."""
    return (1, F) if band_major else (B, 1)


def pack(X, band_major, fill, cgap=3, rgap=5, tail=64):
    """X (rows, C, F, B) as a flat buffer: a channel's block, `cgap` floats of `fill`, ... `rgap` more behind a row, `tail` behind all."""
    rows, C_, F, B = X.shape
    cs = F * B + cgap
    rs = C_ * cs + rgap
    buf = np.full(rows * rs + tail, fill, F32)
    for i in range(rows):
        for c in range(C_):
            block = X[i, c].T if band_major else X[i, c]
            buf[i * rs + c * cs:i * rs + c * cs + F * B] = block.reshape(-1)
    return buf, rs, cs


def unpack(buf, shape, band_major, fill, cgap=3, rgap=5):
    """The inverse of pack, with the gaps and the tail checked against `fill`."""
    rows, C_, F, B = shape
    cs = F * B + cgap
    rs = C_ * cs + rgap
    out = np.empty(shape, F32)
    keep = np.ones(buf.shape, bool)
    for i in range(rows):
        for c in range(C_):
            o = i * rs + c * cs
            block = buf[o:o + F * B]
            out[i, c] = block.reshape(B, F).T if band_major else block.reshape(F, B)
            keep[o:o + F * B] = False
    assert (buf[keep] == fill).all(), "written outside the blocks: between the channels, between the rows or behind the end"
    return out


def kernel_case(F, B):
    """Six rows of two channels and their references, once per shape: (X, vf, {(mode, axis): R}, R without valid_frames)."""
    X = normal_features(F * 1000 + B, (6, 2, F, B))
    X[1] = F32(-8.0)  # a constant
    vf = [F, F, 0, 1, F // 2 + 1, min(F, 65)]
    X[4, :, F // 2, B // 2] = F32(90.0)  # one large value, the peak of row 4: its last counted frame
    if F // 2 + 1 < F:
        X[4, 1, F - 1, 0] = F32(500.0)   # ... and a larger one behind the counted frames, which is nobody's peak
    R = {(m, a): rule_fnorm(X, vf, m, a, **PARAMS) for m in MODES for a in AXES if a == "band" or m in ("mean", "mean_var")}
    for m in (None, "peak"):
        R[(m, "all")] = R[(m, "band")]  # the axis is ignored
    assert not R[("mean", "band")][1].view(np.uint32).any() and (R[("peak", "all")][4, 0, :F // 2 + 1].max() == F32(F32(94.0) * F32(0.3)))
    assert (R[("mean_var", "all")][2] == F32(-7.5)).all()
    R_all = {(m, a): rule_fnorm(X[3:5], None, m, a, **PARAMS) for m, a in (("mean_var", "band"), ("peak", "band"), ("mean", "all"))}
    X.setflags(write=False)
    for r in list(R.values()) + list(R_all.values()):
        r.setflags(write=False)
    return X, vf, R, R_all


_KERNEL_CASES = {}


def fdesc(mode, axis, shape, src, dst):
    """src, dst: (row stride, channel stride, band_major)"""
    rows, C_, F, B = shape
    sf, sb = strides(F, B, src[2])
    df, db = strides(F, B, dst[2])
    return make_fdesc(mode, axis, rows=rows, channels=C_, frames=F, bands=B, eps=PARAMS["eps"], pad_value=PARAMS["pad_value"],
                      range=PARAMS["peak_range"], offset=PARAMS["peak_offset"], gain=PARAMS["peak_gain"], src_row_stride=src[0],
                      src_chan_stride=src[1], src_frame_stride=sf, src_band_stride=sb, dst_row_stride=dst[0], dst_chan_stride=dst[1],
                      dst_frame_stride=df, dst_band_stride=db)


def mismatch(got, want):
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    return (len(bad), bad[:4].tolist(), [(float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:4]]) if len(bad) else None


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_kernel_alone(gpu_ctx, shape):
    """nvh_fnorm_rows on six rows of two channels -- noise with every frame counted, a constant, vf = 0, 1, F // 2 + 1 (with a single
    large value as its peak, and a larger one behind the counted frames) and min(F, 65) -- in all four modes and both axes; source
    and destination band-major and frame-major in all four pairings, out of place and (same layout) in place; row and channel
    strides with gaps that keep their sentinel, behind the end as well; and valid_frames = NULL.  (130, 256) and (250, 80) take the
    re-reading path, every other shape the LDS-resident one; (249, 80) and (250, 80) lie on the two sides of that boundary."""
    F, B = shape
    assert takes_lds_path(F, B) == (shape not in ((130, 256), (250, 80)))
    if shape not in _KERNEL_CASES:
        _KERNEL_CASES[shape] = kernel_case(F, B)
    check_kernel_case(gpu_ctx, _KERNEL_CASES[shape])


def check_kernel_case(gpu_ctx, case, null_rows=(3, 5)):
    """The launches and assertions of test_kernel_alone over one kernel_case(F, B); R_all holds rows null_rows[0]:null_rows[1]."""
    torch = _torch()
    X, vf, R, R_all = case
    d_src = {}
    for bm in (True, False):
        buf, rs, cs = pack(X, bm, GAP)
        d_src[bm] = (torch.from_numpy(buf).cuda(), rs, cs)
    for mode in MODES:
        for axis in AXES:
            want = R[(mode, axis)]
            for src_bm in (True, False):
                for dst_bm in (True, False):
                    _, drs, dcs = pack(X, dst_bm, SENT, 4, 7)
                    d_dst = torch.full((X.shape[0] * drs + 64,), float(SENT), dtype=torch.float32, device="cuda")
                    torch.cuda.synchronize()
                    s, srs, scs = d_src[src_bm]
                    gpu_ctx.fnorm_rows(fdesc(mode, axis, X.shape, (srs, scs, src_bm), (drs, dcs, dst_bm)), s.data_ptr(), d_dst.data_ptr(), vf)
                    gpu_ctx.synchronize()
                    got = unpack(d_dst.cpu().numpy(), X.shape, dst_bm, SENT, 4, 7)
                    assert mismatch(got, want) is None, (mode, axis, src_bm, dst_bm, mismatch(got, want))
            for bm in (True, False):  # in place
                buf, rs, cs = pack(X, bm, SENT)
                d = torch.from_numpy(buf).cuda()
                torch.cuda.synchronize()
                gpu_ctx.fnorm_rows(fdesc(mode, axis, X.shape, (rs, cs, bm), (rs, cs, bm)), d.data_ptr(), d.data_ptr(), vf)
                gpu_ctx.synchronize()
                got = unpack(d.cpu().numpy(), X.shape, bm, SENT)
                assert mismatch(got, want) is None, (mode, axis, bm, "in place", mismatch(got, want))
    # the source is as it was
    for bm in (True, False):
        assert same_bits(d_src[bm][0].cpu().numpy(), pack(X, bm, GAP)[0])
    # valid_frames = NULL: every frame of rows 3 and 4 counts, nothing is filled
    sub = np.ascontiguousarray(X[null_rows[0]:null_rows[1]])
    for (mode, axis), want in R_all.items():
        for src_bm, dst_bm in ((True, False), (False, False), (True, True)):
            buf, rs, cs = pack(sub, src_bm, GAP)
            s = torch.from_numpy(buf).cuda()
            _, drs, dcs = pack(sub, dst_bm, SENT)
            d_dst = torch.full((2 * drs + 64,), float(SENT), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            gpu_ctx.fnorm_rows(fdesc(mode, axis, sub.shape, (rs, cs, src_bm), (drs, dcs, dst_bm)), s.data_ptr(), d_dst.data_ptr(), None)
            gpu_ctx.synchronize()
            got = unpack(d_dst.cpu().numpy(), sub.shape, dst_bm, SENT)
            assert mismatch(got, want) is None, (mode, axis, src_bm, dst_bm, "NULL", mismatch(got, want))


@pytest.mark.gpu
def test_more_items_than_workgroups_and_two_parameter_sets(gpu_ctx):
    """3000 rows of (F, B) = (9, 20) with random vf: more work items than a launch has workgroups, so a workgroup walks several.
    mean_var with both axes, as two parameter sets one behind the other on one context (the second call's frame counts go through
    the staging the first one used), frame-major and band-major."""
    torch = _torch()
    rows, F, B = 3000, 9, 20
    x = normal_features(11, (rows, 1, F, B))
    rng = np.random.default_rng(12)
    vfs = [rng.integers(0, F + 1, rows), rng.integers(0, F + 1, rows)]
    sets = [dict(axis="band", eps=1e-5, pad_value=0.0), dict(axis="all", eps=1e-2, pad_value=-1.0)]
    bufs = []
    for (kw, vf, bm) in zip(sets, vfs, (False, True)):
        src = np.ascontiguousarray(x.transpose(0, 1, 3, 2) if bm else x).reshape(-1)
        d_src = torch.from_numpy(src).cuda()
        d_dst = torch.full((rows * F * B + 64,), float(SENT), dtype=torch.float32, device="cuda")
        bufs.append((d_src, d_dst))
    torch.cuda.synchronize()
    for (kw, vf, bm), (d_src, d_dst) in zip(zip(sets, vfs, (False, True)), bufs):
        sf, sb = strides(F, B, bm)
        d = make_fdesc("mean_var", kw["axis"], rows=rows, channels=1, frames=F, bands=B, eps=kw["eps"], pad_value=kw["pad_value"],
                       src_row_stride=F * B, src_frame_stride=sf, src_band_stride=sb, dst_row_stride=F * B, dst_frame_stride=B, dst_band_stride=1)
        gpu_ctx.fnorm_rows(d, d_src.data_ptr(), d_dst.data_ptr(), vf)  # (no wait between the two)
    gpu_ctx.synchronize()
    for (kw, vf), (_, d_dst) in zip(zip(sets, vfs), bufs):
        got = d_dst.cpu().numpy()
        want = rule_fnorm(x, vf, "mean_var", kw["axis"], eps=kw["eps"], pad_value=kw["pad_value"])
        assert (got[rows * F * B:] == SENT).all()
        assert mismatch(got[:rows * F * B].reshape(x.shape), want) is None, (kw, mismatch(got[:rows * F * B].reshape(x.shape), want))


@pytest.mark.gpu
def test_row_stride_beyond_31_bits(gpu_ctx):
    """Two rows 2^31 + 8 floats apart, in place (the buffer is allocated, not filled): the second row's elements lie behind index
    2^31, where 32-bit element arithmetic would wrap.  Band-major and frame-major; the floats around the second row keep their
    sentinel."""
    torch = _torch()
    F, B, rs = 65, 80, (1 << 31) + 8
    x = normal_features(21, (2, 1, F, B))
    vf = [F // 2, F]
    want = rule_fnorm(x, vf, "mean_var", "band", eps=1e-5, pad_value=0.5)
    big = torch.empty((rs + F * B + 64,), dtype=torch.float32, device="cuda")
    for bm in (True, False):
        body = np.ascontiguousarray(x.transpose(0, 1, 3, 2) if bm else x).reshape(2, F * B)
        big[:F * B] = torch.from_numpy(body[0]).cuda()
        big[rs - 64:rs + F * B + 64] = float(SENT)
        big[rs:rs + F * B] = torch.from_numpy(body[1]).cuda()
        torch.cuda.synchronize()
        fs, bs = strides(F, B, bm)
        d = make_fdesc("mean_var", "band", rows=2, channels=1, frames=F, bands=B, eps=1e-5, pad_value=0.5, src_row_stride=rs, dst_row_stride=rs,
                       src_frame_stride=fs, src_band_stride=bs, dst_frame_stride=fs, dst_band_stride=bs)
        gpu_ctx.fnorm_rows(d, big.data_ptr(), big.data_ptr(), vf)
        gpu_ctx.synchronize()
        got = np.stack([big[:F * B].cpu().numpy(), big[rs:rs + F * B].cpu().numpy()])
        got = got.reshape(2, 1, B, F).transpose(0, 1, 3, 2) if bm else got.reshape(2, 1, F, B)
        assert mismatch(got, want) is None, (bm, mismatch(got, want))
        assert (big[rs - 64:rs].cpu().numpy() == SENT).all() and (big[rs + F * B:].cpu().numpy() == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------------
# through decode_clip_features
# ---------------------------------------------------------------------------------------------------------------------------

# (keywords of the call, arguments of rule_fnorm, counted frames are valid_frames)
NORM_CASES = {
    "mean_band": (dict(normalize="mean", normalize_axis="band", pad_value=-2.0), dict(mode="mean", axis="band", pad_value=-2.0), True),
    "mean_var_band": (dict(normalize="mean_var"), dict(mode="mean_var", axis="band"), True),
    "mean_var_all": (dict(normalize="mean_var", normalize_axis="all", norm_eps=1e-3), dict(mode="mean_var", axis="all", eps=1e-3), True),
    "peak_db": (dict(normalize="peak", peak_range=80.0, peak_offset=40.0, peak_gain=1 / 40), dict(mode="peak"), True),
    "peak_unmasked": (dict(normalize="peak", mask_padding=False), dict(mode="peak"), False),
    "fill_only": (dict(pad_value=0.0), dict(mode=None, pad_value=0.0), True),
}


def expected(oracle, ogg_bytes, form, call):
    """(rows, files, starts, want (N, och, F, B) before normalisation, valid, valid_frames, clip flags) of one FEATURE_CALLS entry."""
    from tests.test_resample_rows import FILES, clip_at
    target, rates, extra, mel = call
    names = FILES if form == "mono" else ("3test", "issue6test")
    rows = feature_rows(ogg_bytes, names, target, rates)
    files = [clip_at(ogg_bytes, n, r) for n, r, _ in rows]
    starts = [s for _, _, s in rows]
    ref = [want_features(oracle, ogg_bytes, n, r, target, form, s, True, mel) for n, r, s in rows]
    want = np.stack([f for f, _, _, _ in ref])
    F = want.shape[2]
    want_vf = np.asarray([v for _, _, v, _ in ref], np.int64)
    assert (want_vf == 0).any() and (want_vf == F).any() and ((want_vf > 0) & (want_vf < F)).any()
    return files, starts, want, [v for _, v, _, _ in ref], want_vf, [c for _, _, _, c in ref]


def shaped(want, mel, form):
    """(N, och, F, B) as the call returns it"""
    if mel["band_major"]:
        want = want.transpose(0, 1, 3, 2)
    return want[:, 0] if form == "mono" else want


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(NORM_CASES))
@pytest.mark.parametrize("form", ["mono", "f32"])
def test_decode_clip_features_normalized(oracle, gpu_ctx, ogg_bytes, form, case):
    """The two calls of tests/test_mel_rows.py (band-major at 16 kHz from mixed rates; frame-major at the clips' own 44100 Hz), mono
    and stereo, to the device and to the host, with each normalisation: the features equal rule_fnorm over the expected features of
    that file with the expected valid_frames (rows with 0, F and something between), and valid, valid_frames and the clip flags are
    what they are without the keywords."""
    _torch()
    import nvorbis_amd as nv
    kw, rule_kw, masked = NORM_CASES[case]
    for k, call in enumerate(FEATURE_CALLS):
        target, rates, extra, mel = call
        files, starts, want, want_valid, want_vf, want_clipped = expected(oracle, ogg_bytes, form, call)
        want = shaped(rule_fnorm(want, want_vf if masked else None, **rule_kw), mel, form)
        device_out = (k + sorted(NORM_CASES).index(case)) % 2 == 0
        (feats, valid, valid_frames), clipped = feature_call(nv, gpu_ctx, files, starts, dict(extra, **kw), mel, form, True, True, device_out)
        assert (feats.is_cuda if device_out else isinstance(feats, np.ndarray)) and tuple(feats.shape) == want.shape
        assert np.array_equal(valid, want_valid) and np.array_equal(valid_frames, want_vf) and np.array_equal(clipped, want_clipped)
        host = feats.cpu().numpy() if device_out else feats
        bad = [i for i in range(len(files)) if not same_bits(np.ascontiguousarray(host[i]), np.ascontiguousarray(want[i]))]
        assert not bad, (form, case, target, bad, int(want_vf[bad[0]]))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["mono", "f32"])
def test_defaults_change_nothing_and_the_call_is_mel_rows_then_fnorm_rows(gpu_ctx, ogg_bytes, form):
    """A call with every new keyword at its default (pad_value left away: given, it is the fill-only form) gives the bits of a call
    without them; and a normalised call equals decode_clip_rows, nvh_mel_rows and nvh_fnorm_rows called by hand."""
    torch = _torch()
    import nvorbis_amd as nv
    from nvorbis_amd import clips
    from tests.test_resample_rows import FILES, clip_at
    names = FILES if form == "mono" else ("3test", "issue6test")
    kwf = {"mono": {"mix": "mono"}, "f32": {}}[form]
    for target, rates, extra, mel in FEATURE_CALLS:
        rows = feature_rows(ogg_bytes, names, target, rates)
        files = [clip_at(ogg_bytes, n, r) for n, r, _ in rows]
        starts = [s for _, _, s in rows]
        (plain, v0, f0), c0 = feature_call(nv, gpu_ctx, files, starts, extra, mel, form, True, True)
        defaults = dict(normalize=None, normalize_axis="band", norm_eps=1e-5, peak_range=80.0, peak_offset=40.0, peak_gain=1 / 40, mask_padding=True)
        (same, v1, f1), c1 = feature_call(nv, gpu_ctx, files, starts, dict(extra, **defaults), mel, form, True, True)
        assert same_bits(plain.cpu().numpy(), same.cpu().numpy()) and np.array_equal(v0, v1) and np.array_equal(f0, f1) and np.array_equal(c0, c1)
        norm = dict(normalize="mean_var", normalize_axis="all", norm_eps=1e-4, pad_value=3.0)
        (got, v2, f2), c2 = feature_call(nv, gpu_ctx, files, starts, dict(extra, **norm), mel, form, True, True)
        assert np.array_equal(v0, v2) and np.array_equal(f0, f2) and np.array_equal(c0, c2)
        # by hand: the rows, the features out of place, the normalisation out of place into a third buffer
        pcm, valid = nv.decode_clip_rows(files, LENGTH, starts, ctx=gpu_ctx, batch_frames=16, sample_format="f32", device_out=True,
                                         layout="interleaved" if form == "mono" else "planar", **extra, **kwf)
        n, och = pcm.shape[0], 1 if form == "mono" else pcm.shape[1]
        N_, W, H, B = mel["n_fft"], mel["win_length"], mel["hop"], mel["n_mels"]
        F = LENGTH // H + 1
        md = clips.mel_desc(target, N_, W, H, B, mel.get("f_min", 0.0), mel.get("f_max"), mel["mel_scale"], mel["norm"], mel["scale"],
                            mel.get("floor", 1e-10))
        shape = (n, och, B, F) if mel["band_major"] else (n, och, F, B)
        feats, out = torch.empty(shape, dtype=torch.float32, device=pcm.device), torch.empty(shape, dtype=torch.float32, device=pcm.device)
        fs, bs = (feats.stride(3), feats.stride(2)) if mel["band_major"] else (feats.stride(2), feats.stride(3))
        md.rows, md.channels, md.frames, md.first, md.src_length = n, och, F, (N_ - W) // 2 - N_ // 2, LENGTH
        md.src_row_stride, md.src_time_stride, md.src_chan_stride = pcm.stride(0), pcm.stride(-1), 0 if form == "mono" else pcm.stride(1)
        md.dst_row_stride, md.dst_chan_stride, md.dst_frame_stride, md.dst_band_stride = feats.stride(0), feats.stride(1), fs, bs
        nd = clips.fnorm_desc("mean_var", "all", 1e-4, 3.0, frames=F, bands=B)
        nd.rows, nd.channels = n, och
        nd.src_row_stride = nd.dst_row_stride = feats.stride(0)
        nd.src_chan_stride = nd.dst_chan_stride = feats.stride(1)
        nd.src_frame_stride = nd.dst_frame_stride = fs
        nd.src_band_stride = nd.dst_band_stride = bs
        torch.cuda.synchronize()
        gpu_ctx.mel_rows(md, pcm.data_ptr(), feats.data_ptr(), valid)
        gpu_ctx.fnorm_rows(nd, feats.data_ptr(), out.data_ptr(), f0)
        gpu_ctx.synchronize()
        assert same_bits(feats.cpu().numpy().reshape(plain.shape), plain.cpu().numpy())
        assert same_bits(out.cpu().numpy().reshape(got.shape), got.cpu().numpy())
        assert not same_bits(got.cpu().numpy(), plain.cpu().numpy())


@pytest.mark.gpu
def test_normalized_features_repeat_and_disturb_nothing(gpu_ctx, ogg_bytes):
    """The same normalised call twice gives the same bits (to the host as well), and decode_clip_rows with the same arguments gives
    the same bits before and after on the same context."""
    _torch()
    import nvorbis_amd as nv
    from tests.test_resample_rows import clip_at
    target, rates, extra, mel = FEATURE_CALLS[0]
    rows = feature_rows(ogg_bytes, ("3test", "issue6test"), target, rates)
    files = [clip_at(ogg_bytes, n, r) for n, r, _ in rows]
    starts = [s for _, _, s in rows]
    norm = dict(extra, normalize="mean_var", normalize_axis="band")

    def plain():
        (r, v), c = nv.decode_clip_rows(files, LENGTH, starts, ctx=gpu_ctx, batch_frames=16, layout="planar", device_out=True,
                                        return_clipped=True, **extra)
        return r.cpu().numpy(), v, c
    before = plain()
    (a, va, fa), ca = feature_call(nv, gpu_ctx, files, starts, norm, mel, "f32", True, True)
    (b, vb, fb_), cb = feature_call(nv, gpu_ctx, files, starts, norm, mel, "f32", True, True)
    (h, vh, fh), ch = feature_call(nv, gpu_ctx, files, starts, norm, mel, "f32", True, True, device_out=False)
    after = plain()
    assert isinstance(h, np.ndarray) and h.dtype == F32
    assert same_bits(a.cpu().numpy(), b.cpu().numpy()) and same_bits(a.cpu().numpy(), h)
    assert np.array_equal(va, vb) and np.array_equal(fa, fb_) and np.array_equal(ca, cb) and np.array_equal(va, vh) and np.array_equal(fa, fh)
    assert same_bits(np.ascontiguousarray(before[0]), np.ascontiguousarray(after[0]))
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2]) and np.array_equal(before[1], va)

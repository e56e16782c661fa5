"""Cepstra and deltas of features on the GPU: k_cep_rows alone on synthetic features, and the cepstral keywords of
decode_clip_features against the CPU oracle (include/nvorbis_hip.h states the rule under nvh_cep_rows).

The reference is the rule in numpy with numpy's own tables (tests/test_cep_plan.py: rule_tables and rule_cep, written from the
header's text; that file holds nvh_cep_tables to them).  No tolerance anywhere: everything is compared as uint32."""
import numpy as np
import pytest

from tests.test_cep_plan import F32, make_cdesc, normal_features, rule_cep, rule_tables
from tests.test_clip_batches import _torch, same_bits
from tests.test_fnorm_rows import mismatch, pack, strides, unpack

SENT = F32(-1234.5)
GAP = F32(1e30)  # what lies between the source's rows and channels: never read
HUGE = F32(1e30)  # behind vf of row 5: finite, its statics are finite, and no counted frame's delta may see it
T = 24  # NVH_CEP_TILE (nvorbis_amd/csrc/cep_dev.h), the header's NVH_CEP_FRAMES
# (F, B, K or None, o, N, dct_norm, lifter).  F around the tile at Kaldi's 23 -> 13 with both delta orders; then the band and
# column limits -- (80, None) has no transform, (256, 85) and (256, 256) read their table through the caches, the others stage it
# --; the widest halo (N = 8: 16 frames on each side, 56 slots); and (128, 105) / (128, 106), the last K whose table lies in LDS
# beside a tile of 28 slots and the first one whose does not (tests/test_cep_routes.py walks that edge to the byte).
KERNEL_SHAPES = [(F, 23, 13, 2, 2, "ortho", 22.0) for F in (1, 2, 4, T - 1, T, T + 1, 2 * T + 1)] + [
    (30, 1, 1, 2, 2, "ortho", 0.0), (30, 80, None, 2, 2, "ortho", 0.0), (30, 256, 85, 2, 2, None, 0.0), (30, 256, 256, 0, 2, "ortho", 22.0),
    (30, 40, 40, 0, 2, None, 22.0), (40, 23, 13, 2, 8, "ortho", 22.0), (30, 128, 105, 1, 2, "ortho", 0.0), (30, 128, 106, 1, 2, "ortho", 0.0)]
STAGED = {(23, 13): 1, (1, 1): 1, (80, None): 0, (256, 85): 0, (256, 256): 0, (40, 40): 1, (128, 105): 1, (128, 106): 0}


def cdesc(shape, rows, C_, src, dst):
    """src, dst: (row stride, channel stride, band_major)"""
    F, B, K, o, N, norm, lifter = shape
    Q = (1 + o) * (B if K is None else K)
    sf, sb = strides(F, B, src[2])
    df, dq = strides(F, Q, dst[2])
    return make_cdesc(transform=0 if K is None else 1, dct_norm=0 if norm == "ortho" else 1, order=o, window=N, rows=rows, channels=C_,
                      frames=F, bands=B, ceps=B if K is None else K, lifter=lifter, src_row_stride=src[0], src_chan_stride=src[1],
                      src_frame_stride=sf, src_band_stride=sb, dst_row_stride=dst[0], dst_chan_stride=dst[1], dst_frame_stride=df,
                      dst_col_stride=dq)


def kernel_case(shape):
    """Seven rows of two channels and their references, once per shape: (X, vf, R with vf, R of rows 3 and 4 without)."""
    F, B, K, o, N, norm, lifter = shape
    X = normal_features(F * 1000 + B + N, (7, 2, F, B))
    X[1] = F32(-8.0)  # a constant
    vf = [F, F, 0, 1, min(N, F), F // 2 + 1, F]
    if vf[5] < F:
        X[5, 1, vf[5]:] = HUGE
    tables = rule_tables(B, K, norm, lifter, N)
    with np.errstate(over="ignore"):
        R = rule_cep(X, vf, tables, o, N)
        R_all = rule_cep(X[3:5], None, tables, o, N)
    assert np.isfinite(R).all() and np.isfinite(R_all).all()
    Kc = B if K is None else K
    if o:
        assert not R[2, :, :, Kc:].view(np.uint32).any() and not R[5, :, vf[5]:, Kc:].view(np.uint32).any()  # +0 behind vf
        assert np.abs(R[5, :, :vf[5], Kc:]).max() < 1e3 and (F == 1 or np.abs(R[0, :, :, Kc:]).max() > 0)
    X.setflags(write=False)
    R.setflags(write=False)
    R_all.setflags(write=False)
    return X, vf, R, R_all


_KERNEL_CASES = {}


def route_of(d):
    import ctypes as C
    from nvorbis_amd import native
    out = (C.c_int64 * 4)()
    assert native.lib().nvh_cep_route(C.byref(d), out) == native.OK
    return list(out)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_kernel_alone(gpu_ctx, shape):
    """nvh_cep_rows on seven rows of two channels -- noise with every frame counted, a constant, vf = 0, 1, N, F // 2 + 1 (with a huge
    finite value in every frame behind it, which reaches no counted frame's deltas) and F again --; source and destination
    band-major and frame-major in all four pairings; row and channel strides with gaps that keep their sentinel, behind the end as
    well; the source unchanged; and valid_frames = NULL."""
    torch = _torch()
    F, B, K, o, N, norm, lifter = shape
    if shape not in _KERNEL_CASES:
        _KERNEL_CASES[shape] = kernel_case(shape)
    X, vf, R, R_all = _KERNEL_CASES[shape]
    oshape = R.shape
    d_src = {}
    for bm in (True, False):
        buf, rs, cs = pack(X, bm, GAP)
        d_src[bm] = (torch.from_numpy(buf).cuda(), rs, cs)
    for src_bm in (True, False):
        for dst_bm in (True, False):
            _, drs, dcs = pack(R, dst_bm, SENT, 4, 7)
            d_dst = torch.full((oshape[0] * drs + 64,), float(SENT), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            s, srs, scs = d_src[src_bm]
            d = cdesc(shape, 7, 2, (srs, scs, src_bm), (drs, dcs, dst_bm))
            route = route_of(d)
            assert route[0] == STAGED[(B, K)] and route[1] <= 81920 and route[3] == -(-F // T), route
            gpu_ctx.cep_rows(d, s.data_ptr(), d_dst.data_ptr(), vf)
            gpu_ctx.synchronize()
            got = unpack(d_dst.cpu().numpy(), oshape, dst_bm, SENT, 4, 7)
            assert mismatch(got, R) is None, (src_bm, dst_bm, mismatch(got, R))
    for bm in (True, False):  # the source is as it was
        assert same_bits(d_src[bm][0].cpu().numpy(), pack(X, bm, GAP)[0])
    # valid_frames = NULL: every frame of rows 3 and 4 counts
    sub = np.ascontiguousarray(X[3:5])
    for src_bm, dst_bm in ((True, False), (False, True)):
        buf, rs, cs = pack(sub, src_bm, GAP)
        s = torch.from_numpy(buf).cuda()
        _, drs, dcs = pack(R_all, dst_bm, SENT)
        d_dst = torch.full((2 * drs + 64,), float(SENT), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.cep_rows(cdesc(shape, 2, 2, (rs, cs, src_bm), (drs, dcs, dst_bm)), s.data_ptr(), d_dst.data_ptr(), None)
        gpu_ctx.synchronize()
        got = unpack(d_dst.cpu().numpy(), R_all.shape, dst_bm, SENT)
        assert mismatch(got, R_all) is None, (src_bm, dst_bm, "NULL", mismatch(got, R_all))


# ---------------------------------------------------------------------------------------------------------------------------
# through decode_clip_features
# ---------------------------------------------------------------------------------------------------------------------------

LENGTH = 8200  # 49 frames of Kaldi's 25 ms / 10 ms at 16 kHz: three tiles, the last of one frame
RATE = 16000
_WANT = {}


def mfcc_rows(ogg_bytes, name):
    """Starts at 16 kHz of three rows of one 44100 Hz file: from its start, across its end, and beyond it (no counted frame)."""
    import nvorbis_amd as nv
    from tests.test_resample_plan import rule_plan
    pa = nv.demux_ogg_array(ogg_bytes[name], 0)
    st = nv.Stream(None, pa[0], pa[1], pa[2])
    try:
        total = st.index_packets(pa, 3)[3]
    finally:
        st.close()
    L, M = rule_plan(44100, RATE)[:2]
    total_out = (total * L + M - 1) // M
    return [0, total_out - 3000, total_out + 5]


def want_mfcc(oracle, ogg_bytes, name, form, start, kw):
    """((och, F, 23) log-mel features before the cepstral stage, valid, valid_frames) of one row: oracle PCM -> the resampler's rule
    -> rule_front -> the mel rule, all existing rules with the library's mel tables."""
    from tests.test_mel_front_plan import front_tables, rule_front
    from tests.test_mel_plan import rule_mel, rule_power, rule_scale
    from tests.test_resample_rows import want_row
    key = (name, form, start)
    if key not in _WANT:
        row, valid, _, _ = want_row(oracle, ogg_bytes, name, 44100, RATE, form, start, LENGTH)
        N, W, H, B = kw["n_fft"], kw["win_length"], kw["hop"], kw["n_mels"]
        F = (LENGTH - W) // H + 1
        tw, win, fb = front_tables(RATE, N, W, B, kw["window"], kw["mel_triangles"], f_min=kw["f_min"], f_max=kw["f_max"])
        u = np.concatenate([rule_front(row[:, ch], valid, 0, F, N, W, H, win, remove_dc=kw["remove_dc"], preemphasis=kw["preemphasis"],
                                       gain=kw["sample_gain"]) for ch in range(row.shape[1])])
        mel = rule_scale(rule_mel(rule_power(u, tw), fb), kw["scale"], kw["floor"]).reshape(row.shape[1], F, B)
        begins = np.arange(F) * H
        mel.setflags(write=False)
        _WANT[key] = (mel, valid, int((begins < np.minimum(begins + W, valid)).sum()))
    return _WANT[key]


@pytest.mark.gpu
@pytest.mark.parametrize("band_major", [True, False])
@pytest.mark.parametrize("form", ["mono", "f32"])
def test_decode_clip_features_mfcc_deltas_cmvn(oracle, gpu_ctx, ogg_bytes, form, band_major):
    """decode_clip_features(**kaldi_mfcc_keywords(16000), deltas=2, normalize="mean_var") on the committed 44100 Hz files resampled
    to 16 kHz, mono mix and stereo, both orders, to the device and to the host: the 39 columns equal oracle PCM -> the existing
    numpy rules -> rule_cep -> rule_fnorm as uint32; the rows count every frame, some frames and none.  The same call without the
    new keywords is the Kaldi fbank call of today: its 23 bands equal the rules without the cepstral stage."""
    _torch()
    import nvorbis_amd as nv
    from tests.test_fnorm_plan import rule_fnorm
    from tests.test_resample_rows import clip_at
    kw = nv.kaldi_mfcc_keywords(RATE)
    assert (kw["n_fft"], kw["win_length"], kw["hop"], kw["n_mels"], kw["cepstra"], kw["lifter"]) == (512, 400, 160, 23, 13, 22.0)
    names = ("1test", "3test") if form == "mono" else ("3test", "issue6test")
    files, starts, ref = [], [], []
    for name in names:
        for s in mfcc_rows(ogg_bytes, name):
            files.append(clip_at(ogg_bytes, name, 44100))
            starts.append(s)
            ref.append(want_mfcc(oracle, ogg_bytes, name, form, s, kw))
    mel = np.stack([m for m, _, _ in ref])  # (N, och, F, 23)
    F = mel.shape[2]
    want_valid = np.asarray([v for _, v, _ in ref], np.int64)
    want_vf = np.asarray([v for _, _, v in ref], np.int64)
    assert F == 49 and (want_vf == 0).any() and (want_vf == F).any() and ((want_vf > 0) & (want_vf < F)).any()
    tables = rule_tables(23, 13, "ortho", 22.0, 2)
    want = rule_fnorm(rule_cep(mel, want_vf, tables, 2, 2), want_vf, "mean_var", "band")
    assert want.shape == (len(files), mel.shape[1], F, 39)

    def shaped(a):
        a = a.transpose(0, 1, 3, 2) if band_major else a
        return a[:, 0] if form == "mono" else a
    common = dict(ctx=gpu_ctx, batch_frames=16, sample_rate=RATE, band_major=band_major, **({"mix": "mono"} if form == "mono" else {}))
    fbank = {k: v for k, v in kw.items() if k not in ("cepstra", "dct_norm", "lifter")}
    before, v0, f0 = nv.decode_clip_features(files, LENGTH, starts, **fbank, **common)
    for device_out in (True, False):
        feats, valid, vf = nv.decode_clip_features(files, LENGTH, starts, deltas=2, normalize="mean_var", device_out=device_out, **kw, **common)
        assert (feats.is_cuda if device_out else isinstance(feats, np.ndarray)) and tuple(feats.shape) == shaped(want).shape
        assert np.array_equal(valid, want_valid) and np.array_equal(vf, want_vf)
        host = feats.cpu().numpy() if device_out else feats
        bad = [i for i in range(len(files)) if not same_bits(np.ascontiguousarray(host[i]), np.ascontiguousarray(shaped(want)[i]))]
        assert not bad, (form, band_major, device_out, bad, [int(want_vf[i]) for i in bad])
    # nothing leaked: the call without the new keywords, before and after, is the mel rule's output
    after, v1, f1 = nv.decode_clip_features(files, LENGTH, starts, **fbank, **common)
    assert same_bits(before.cpu().numpy(), after.cpu().numpy()) and np.array_equal(v0, v1) and np.array_equal(f0, f1) and np.array_equal(f0, want_vf)
    assert same_bits(before.cpu().numpy(), np.ascontiguousarray(shaped(mel)))


@pytest.mark.gpu
def test_deltas_without_a_transform_and_unmasked(oracle, gpu_ctx, ogg_bytes):
    """deltas=1 alone (no DCT: 46 columns from 23 bands) with mask_padding=False: every frame counts, in the cepstral stage too,
    and nothing is filled; and cepstra alone (13 columns, torchaudio's norm=None) with no normalisation."""
    _torch()
    import nvorbis_amd as nv
    from tests.test_resample_rows import clip_at
    kw = nv.kaldi_fbank_keywords(RATE, num_mel_bins=23)
    starts = mfcc_rows(ogg_bytes, "3test")
    files = [clip_at(ogg_bytes, "3test", 44100)] * 3
    ref = [want_mfcc(oracle, ogg_bytes, "3test", "mono", s, dict(kw)) for s in starts]
    mel = np.stack([m for m, _, _ in ref])
    want_vf = np.asarray([v for _, _, v in ref], np.int64)
    common = dict(ctx=gpu_ctx, batch_frames=16, sample_rate=RATE, mix="mono", band_major=False)
    got, _, vf = nv.decode_clip_features(files, LENGTH, starts, deltas=1, delta_window=3, mask_padding=False, **kw, **common)
    want = rule_cep(mel, None, rule_tables(23, None, "ortho", 0.0, 3), 1, 3)[:, 0]
    assert np.array_equal(vf, want_vf) and tuple(got.shape) == want.shape == (3, 49, 46) and same_bits(got.cpu().numpy(), want)
    got, _, _ = nv.decode_clip_features(files, LENGTH, starts, cepstra=13, dct_norm=None, **kw, **common)
    want = rule_cep(mel, want_vf, rule_tables(23, 13, None, 0.0, 2), 0, 2)[:, 0]
    assert tuple(got.shape) == (3, 49, 13) and same_bits(got.cpu().numpy(), want)

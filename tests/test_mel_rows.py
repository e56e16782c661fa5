"""Log-mel features on the GPU: k_mel_rows alone on synthetic rows, and decode_clip_features against the CPU oracle (include/
nvorbis_hip.h states the rule under nvh_mel_rows).

The reference is the rule in numpy (tests/test_mel_plan.py: rule_features, written from the header's text) with the LIBRARY'S OWN
tables (that file holds them to the formulas).  No tolerance anywhere: everything is compared as uint32."""
import numpy as np
import pytest

from tests.test_clip_batches import _torch, same_bits
from tests.test_mel_plan import F32, lib_tables, make_desc, rule_frames, rule_mel, rule_power, rule_scale

SENT = F32(-1234.5)
SCALES = ("power", "ln", "db")
# (rate, n_fft, win_length, hop, n_mels): the smallest transform with one band and with eight; the usual speech front end; an odd
# window with the band count at its limit; a hop beyond the window at the largest transform (the LDS budget); and the two stage
# counts whose register passes group differently from those (7 stages: 2 + 2 + 2 + 1; 9 stages: 3 + 3 + 3)
KERNEL_CONFIGS = [(8000, 64, 64, 16, 1), (8000, 64, 64, 16, 8), (16000, 512, 400, 160, 80), (44100, 2048, 1103, 441, 256),
                  (48000, 4096, 4096, 5000, 128), (16000, 256, 200, 80, 40), (22050, 1024, 1024, 256, 64)]


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------

def kernel_case(cfg, frames):
    """Six rows of two channels and their reference, once per (configuration, frame count): (first, S, valid per row, the source
    block X[row, channel, S], the expected blocks {scale: R[row, channel, frame, band]})."""
    rate, N, W, H, B = cfg
    tables = lib_tables(rate, N, W, B)
    tw, win, fb = tables
    first = (N - W) // 2 - N // 2  # negative: the first frames read in front of the row
    S = 6 * H + first + W - 5      # ... and frame 6 behind it
    rng = np.random.default_rng(N + B + frames)
    t = np.arange(S, dtype=np.float64)
    X = np.zeros((6, 2, S), F32)
    X[0] = rng.uniform(-1, 1, (2, S))
    X[1, 0] = 0.8 * np.sin(2 * np.pi * 1000.0 * t / rate)
    X[1, 1] = 0.3 * np.cos(2 * np.pi * 1000.0 * t / rate)
    X[3] = rng.uniform(-1, 1, (2, S))  # never read: valid = 0
    X[4] = rng.uniform(-1, 1, (2, S))
    q = 2 * H + first + W // 2 + 3  # the unit impulse, inside frame 2
    X[5, :, q] = 1.0
    valid = [S, S, S, 0, 2 * H + first + W // 2, S]  # row 4 ends inside frame 2
    assert 0 < valid[4] < S and 0 <= q < S
    u = np.concatenate([rule_frames(X[r, ch], valid[r], first, frames, N, W, H, win) for r in range(6) for ch in range(2)])
    m = rule_mel(rule_power(u, tw), fb).reshape(6, 2, frames, B)
    R = {s: rule_scale(m, s, 1e-10) for s in SCALES}
    # all zeros and valid = 0: every value is the floor's
    for s in SCALES:
        assert R[s].dtype == F32
        z = R[s][2:4]
        assert same_bits(z, np.full_like(z, R[s][2, 0, 0, 0]))
    assert same_bits(R["power"][2], np.zeros_like(R["power"][2])) and R["ln"][2, 0, 0, 0] == rule_scale(F32([0]), "ln", 1e-10)[0] < -23
    # the impulse row's closed form: frame f sees the impulse under window sample i = q - (f H + first), and every bin's power is
    # win[i]^2, so m[b] = win[i]^2 * sum_k fb[b][k], up to the rule's roundings (the float64 bound of tests/test_mel_plan.py)
    for f in range(frames):
        i = q - (f * H + first)
        w2 = float(win[i]) ** 2 if 0 <= i < W else 0.0
        closed = w2 * fb.astype(np.float64).sum(axis=1)
        err = np.abs(R["power"][5, 0, f].astype(np.float64) - closed)
        assert (err <= 8 * 2.0 ** -24 * w2 * (N // 2 + 1)).all(), (f, float(err.max()))
    if frames > 2:
        assert R["power"][5, 0, 2].any() or not fb.any()
    X.setflags(write=False)
    for s in SCALES:
        R[s].setflags(write=False)
    return first, S, valid, X, R


_KERNEL_CASES = {}


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [1, 4, 7])
@pytest.mark.parametrize("cfg", KERNEL_CONFIGS)
def test_kernel_alone(gpu_ctx, cfg, frames):
    """nvh_mel_rows on synthetic rows -- noise, a 1 kHz tone, zeros, valid = 0, a row that ends inside frame 2, a unit impulse --
    with interleaved, planar and mono source strides, band-major and frame-major destinations whose row and channel strides leave
    gaps, and the three scales: every value equals the numpy rule, the gaps and the tail keep their sentinel."""
    key = (cfg, frames)
    if key not in _KERNEL_CASES:
        _KERNEL_CASES[key] = kernel_case(cfg, frames)
    check_kernel_case(gpu_ctx, cfg, frames, _KERNEL_CASES[key])


def check_kernel_case(gpu_ctx, cfg, frames, case):
    """The launches and assertions of test_kernel_alone over one kernel_case(cfg, frames)."""
    torch = _torch()
    rate, N, W, H, B = cfg
    first, S, valid, X, R = case
    rows = X.shape[0]
    for layout in ("interleaved", "planar", "mono"):
        C_ = 1 if layout == "mono" else 2
        if layout == "interleaved":
            src, sstr = np.ascontiguousarray(X.transpose(0, 2, 1)), (S * 2, 2, 1)
        elif layout == "planar":
            src, sstr = np.ascontiguousarray(X.transpose(1, 0, 2)), (S, 1, rows * S)
        else:
            src, sstr = np.ascontiguousarray(X[:, 0, :]), (S, 1, 0)
        d_src = torch.from_numpy(src).cuda()
        cs = frames * B + 3   # three floats between a row's channels,
        rs = C_ * cs + 5      # five behind every row
        for band_major in (True, False):
            fstr, bstr = (1, frames) if band_major else (B, 1)
            for scale in SCALES:
                d_dst = torch.full((rows * rs + 64,), float(SENT), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                desc = make_desc(rate, N, W, B, hop=H, scale=scale, rows=rows, channels=C_, frames=frames, first=first, src_length=S,
                                 src_row_stride=sstr[0], src_time_stride=sstr[1], src_chan_stride=sstr[2], dst_row_stride=rs,
                                 dst_chan_stride=cs, dst_frame_stride=fstr, dst_band_stride=bstr)
                gpu_ctx.mel_rows(desc, d_src.data_ptr(), d_dst.data_ptr(), valid)
                gpu_ctx.synchronize()
                got = d_dst.cpu().numpy()
                assert (got[rows * rs:] == SENT).all(), "written behind the destination"
                got = got[:rows * rs].reshape(rows, rs)
                assert (got[:, C_ * cs:] == SENT).all(), "written between the rows"
                got = got[:, :C_ * cs].reshape(rows, C_, cs)
                assert (got[:, :, frames * B:] == SENT).all(), "written between the channels"
                got = got[:, :, :frames * B]
                got = got.reshape(rows, C_, B, frames).transpose(0, 1, 3, 2) if band_major else got.reshape(rows, C_, frames, B)
                want = R[scale][:, :C_]
                bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != want.view(np.uint32))
                assert not len(bad), (layout, band_major, scale, len(bad), bad[:4].tolist(),
                                      [(float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:4]])
    # valid = NULL: every row counts src_length samples (rows 3 and 4 then read their noise)
    d_src = torch.from_numpy(np.ascontiguousarray(X[3:5, 0, :])).cuda()
    d_dst = torch.full((2 * frames * B + 64,), float(SENT), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    desc = make_desc(rate, N, W, B, hop=H, scale="power", rows=2, channels=1, frames=frames, first=first, src_length=S, src_row_stride=S,
                     src_time_stride=1, src_chan_stride=0, dst_row_stride=frames * B, dst_chan_stride=0, dst_frame_stride=B, dst_band_stride=1)
    gpu_ctx.mel_rows(desc, d_src.data_ptr(), d_dst.data_ptr(), None)
    gpu_ctx.synchronize()
    got = d_dst.cpu().numpy()
    tw, win, fb = lib_tables(rate, N, W, B)
    u = np.concatenate([rule_frames(X[r, 0], S, first, frames, N, W, H, win) for r in (3, 4)])
    assert same_bits(got[:2 * frames * B], rule_mel(rule_power(u, tw), fb).reshape(-1)) and (got[2 * frames * B:] == SENT).all()


@pytest.mark.gpu
def test_many_items_per_workgroup_and_other_tables(gpu_ctx):
    """More work items than workgroups (a workgroup walks several, staging its tables once), the Slaney scale and norm, a band
    limited to [300, 3400] Hz, a floor of its own, and a second parameter set on the same context (the table cache)."""
    torch = _torch()
    rate, N, W, H, B, frames, rows = 8000, 64, 48, 8, 20, 9, 6000  # 18000 work items: four per workgroup
    rng = np.random.default_rng(5)
    S = (frames - 1) * H + W
    x = rng.uniform(-1, 1, (rows, S)).astype(F32)
    valid = rng.integers(0, S + 1, rows)
    d_src = torch.from_numpy(x).cuda()
    for kw in ({"mel_scale": "slaney", "norm": "slaney", "f_min": 300.0, "f_max": 3400.0, "floor": 1e-5}, {"mel_scale": "htk"}):
        d_dst = torch.full((rows * frames * B + 64,), float(SENT), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        desc = make_desc(rate, N, W, B, hop=H, scale="db", rows=rows, channels=1, frames=frames, first=0, src_length=S, src_row_stride=S,
                         src_time_stride=1, src_chan_stride=0, dst_row_stride=frames * B, dst_chan_stride=0, dst_frame_stride=B,
                         dst_band_stride=1, **kw)
        gpu_ctx.mel_rows(desc, d_src.data_ptr(), d_dst.data_ptr(), valid)
        gpu_ctx.synchronize()
        got = d_dst.cpu().numpy()
        from nvorbis_amd import clips
        tw, win, fb = clips.mel_tables(rate, N, W, B, kw.get("f_min", 0.0), kw.get("f_max"), kw["mel_scale"], kw.get("norm"))
        u = np.concatenate([rule_frames(x[r], valid[r], 0, frames, N, W, H, win) for r in range(rows)])
        want = rule_scale(rule_mel(rule_power(u, tw), fb), "db", kw.get("floor", 1e-10))
        assert same_bits(got[:rows * frames * B], want.reshape(-1)) and (got[rows * frames * B:] == SENT).all(), kw


# ---------------------------------------------------------------------------------------------------------------------------
# through decode_clip_features
# ---------------------------------------------------------------------------------------------------------------------------

LENGTH = 4000
# two parameter sets: the defaults at 16 kHz (mixed source rates, every row resampled), and another of everything at the clips' own
# 44100 Hz (no sample_rate: the rows are decode_clip_rows' plain rows)
FEATURE_CALLS = [
    (16000, (44100, 48000, 8000), dict(sample_rate=16000), dict(n_fft=512, win_length=400, hop=160, n_mels=80, mel_scale="htk", norm=None,
                                                                scale="ln", band_major=True)),
    (44100, (44100,), dict(), dict(n_fft=2048, win_length=1103, hop=441, n_mels=128, mel_scale="slaney", norm="slaney", scale="db",
                                   f_min=20.0, f_max=20000.0, floor=1e-8, band_major=False)),
]
_WANT = {}


def feature_rows(ogg_bytes, names, target, rates):
    """[(name, rate, start)]: per file and rate two of the starts 0, mid-clip, across the clip's end and beyond it."""
    import nvorbis_amd as nv
    from tests.test_resample_plan import rule_plan
    out = []
    for k, name in enumerate(names):
        pa = nv.demux_ogg_array(ogg_bytes[name], 0)
        st = nv.Stream(None, pa[0], pa[1], pa[2])
        try:
            total = st.index_packets(pa, 3)[3]
        finally:
            st.close()
        for j, rate in enumerate(rates):
            L, M = rule_plan(rate, target)[:2]
            total_out = (total * L + M - 1) // M
            starts = [0, (total_out // 2) & ~3, total_out - 1500, total_out + 5]
            out += [(name, rate, s) for s in starts[(k + j) % 2::2]]
    return out


def want_features(oracle, ogg_bytes, name, rate, target, form, start, center, mel):
    """((och, F, B) float32 features, valid, valid_frames, clip flag) of one row: oracle PCM -> the resampler's rule -> the mel rule."""
    from tests.test_resample_rows import want_row
    key = (name, rate, target, form, start, center, tuple(sorted((k, str(v)) for k, v in mel.items())))
    if key not in _WANT:
        row, valid, dec, res = want_row(oracle, ogg_bytes, name, rate, target, form, start, LENGTH)
        N, W, H, B = mel["n_fft"], mel["win_length"], mel["hop"], mel["n_mels"]
        from nvorbis_amd import clips
        tw, win, fb = clips.mel_tables(target, N, W, B, mel.get("f_min", 0.0), mel.get("f_max"), mel["mel_scale"], mel["norm"])
        first, F = ((N - W) // 2 - N // 2, LENGTH // H + 1) if center else ((N - W) // 2, (LENGTH - N) // H + 1)
        u = np.concatenate([rule_frames(row[:, ch], valid, first, F, N, W, H, win) for ch in range(row.shape[1])])
        feats = rule_scale(rule_mel(rule_power(u, tw), fb), mel["scale"], mel.get("floor", 1e-10)).reshape(row.shape[1], F, B)
        begins = np.arange(F) * H + first
        vf = sum(1 for b in begins if any(0 <= t < valid for t in range(int(b), int(b) + W)))  # a sample of the frame inside [0, valid)
        feats.setflags(write=False)
        _WANT[key] = (feats, valid, vf, bool(dec or res))
    return _WANT[key]


def feature_call(nv, gpu_ctx, files, starts, extra, mel, form, center, gpu_parse, device_out=True):
    kw = {"mono": {"mix": "mono"}, "map": {"channel_map": (1,)}, "f32": {}}[form]
    return nv.decode_clip_features(files, LENGTH, starts, ctx=gpu_ctx, batch_frames=16, gpu_parse=gpu_parse, center=center,
                                   device_out=device_out, return_clipped=True, **extra, **mel, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("form", ["mono", "f32", "map"])
def test_decode_clip_features(oracle, gpu_ctx, ogg_bytes, form, center):
    """One call mixes 44100, 48000 and 8000 Hz clips with sample_rate=16000, one runs at the clips' own rate with another parameter
    set; starts at 0, mid-clip, across the end and beyond it, length 4000, both parsers: features, valid, valid_frames and the clip
    flags equal oracle PCM -> the resampler's numpy rule -> the mel numpy rule."""
    _torch()
    import nvorbis_amd as nv
    from tests.test_resample_rows import FILES, clip_at
    names = FILES if form == "mono" else ("3test", "issue6test")
    for target, rates, extra, mel in FEATURE_CALLS:
        rows = feature_rows(ogg_bytes, names, target, rates)
        files = [clip_at(ogg_bytes, n, r) for n, r, _ in rows]
        starts = [s for _, _, s in rows]
        ref = [want_features(oracle, ogg_bytes, n, r, target, form, s, center, mel) for n, r, s in rows]
        want = np.stack([f for f, _, _, _ in ref])  # (N, och, F, B)
        F = want.shape[2]
        if mel["band_major"]:
            want = want.transpose(0, 1, 3, 2)
        if form == "mono":
            want = want[:, 0]
        want_vf = np.asarray([v for _, _, v, _ in ref], np.int64)
        assert (want_vf == 0).any() and (want_vf == F).any() and ((want_vf > 0) & (want_vf < F)).any()
        for gpu_parse in (True, False):
            (feats, valid, valid_frames), clipped = feature_call(nv, gpu_ctx, files, starts, extra, mel, form, center, gpu_parse)
            assert feats.is_cuda and tuple(feats.shape) == want.shape, (tuple(feats.shape), want.shape)
            assert np.array_equal(valid, [v for _, v, _, _ in ref]) and valid.dtype == np.int64
            assert np.array_equal(valid_frames, want_vf) and valid_frames.dtype == np.int64
            assert np.array_equal(clipped, [c for _, _, _, c in ref])
            host = feats.cpu().numpy()
            bad = [i for i in range(len(rows)) if not same_bits(np.ascontiguousarray(host[i]), np.ascontiguousarray(want[i]))]
            assert not bad, (form, center, target, gpu_parse, [rows[i] for i in bad])


@pytest.mark.gpu
def test_features_repeat_and_disturb_nothing(gpu_ctx, ogg_bytes):
    """The same call twice gives the same bits (to the host as well), and decode_clip_rows with the same arguments gives the same
    bits before and after a features call on the same context."""
    _torch()
    import nvorbis_amd as nv
    from tests.test_resample_rows import clip_at
    target, rates, extra, mel = FEATURE_CALLS[0]
    rows = feature_rows(ogg_bytes, ("3test", "issue6test"), target, rates)
    files = [clip_at(ogg_bytes, n, r) for n, r, _ in rows]
    starts = [s for _, _, s in rows]

    def plain():
        (r, v), c = nv.decode_clip_rows(files, LENGTH, starts, ctx=gpu_ctx, batch_frames=16, layout="planar", device_out=True,
                                        return_clipped=True, **extra)
        return r.cpu().numpy(), v, c
    before = plain()
    (a, va, fa), ca = feature_call(nv, gpu_ctx, files, starts, extra, mel, "f32", True, True)
    (b, vb, fb_), cb = feature_call(nv, gpu_ctx, files, starts, extra, mel, "f32", True, True)
    (h, vh, fh), ch = feature_call(nv, gpu_ctx, files, starts, extra, mel, "f32", True, True, device_out=False)
    after = plain()
    assert isinstance(h, np.ndarray) and h.dtype == F32
    assert same_bits(a.cpu().numpy(), b.cpu().numpy()) and same_bits(a.cpu().numpy(), h)
    assert np.array_equal(va, vb) and np.array_equal(fa, fb_) and np.array_equal(ca, cb) and np.array_equal(va, vh) and np.array_equal(fa, fh)
    assert same_bits(np.ascontiguousarray(before[0]), np.ascontiguousarray(after[0]))
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2]) and np.array_equal(before[1], va)

"""The front of a log-mel frame on the GPU: the front instances of k_mel_rows alone on synthetic rows, and decode_clip_features with
Kaldi's keywords and with reflect padding against the CPU oracle (include/nvorbis_hip.h states the rule under nvh_mel_front).

The reference is rule_front (tests/test_mel_front_plan.py, written from the header's text) followed by the numpy rule of
tests/test_mel_plan.py, with the LIBRARY'S OWN tables (the plan file holds them to the formulas).  No tolerance anywhere: everything
is compared as uint32.  tests/test_mel_front_plan.py holds every configuration here to its staged or unstaged route."""
import numpy as np
import pytest

from tests.test_clip_batches import _torch, same_bits
from tests.test_mel_front_plan import GPU_CONFIGS, front_tables, make_front, rule_front
from tests.test_mel_plan import F32, make_desc, rule_mel, rule_power, rule_scale

SENT = F32(-1234.5)
CONFIGS = sorted(GPU_CONFIGS)
# name -> (window, triangles, rule_front's options): each option alone, all together, and today's front
ALL = dict(gain=32768.0, remove_dc=True, preemphasis=0.97)
OPTIONS = {
    "gain": ("hann", "hz", {"gain": 32768.0}), "dc": ("hann", "hz", {"remove_dc": True}), "preemphasis": ("hann", "hz", {"preemphasis": 0.97}),
    "povey": ("povey", "hz", {}), "hamming": ("hamming", "hz", {}), "mel": ("hann", "mel", {}), "all": ("povey", "mel", ALL),
    "default": ("hann", "hz", {}),
}
# per source layout: (band-major destination, scale)
LAUNCHES = {"interleaved": (True, "power"), "planar": (False, "ln"), "mono": (True, "db")}
_CASES = {}


def source_rows(cfg, frames, first, S):
    """test_mel_rows.kernel_case's six rows of two channels: noise, a 1 kHz tone, zeros, valid = 0, a row that ends inside frame 2,
    a unit impulse.  The noise rows carry an offset of 0.25, so that the DC removal has something to remove."""
    rate, N, W, H, B = cfg
    rng = np.random.default_rng(N + B + frames + W)
    t = np.arange(S, dtype=np.float64)
    X = np.zeros((6, 2, S), F32)
    X[0] = 0.25 + 0.75 * rng.uniform(-1, 1, (2, S))
    X[1, 0] = 0.8 * np.sin(2 * np.pi * 1000.0 * t / rate)
    X[1, 1] = 0.3 * np.cos(2 * np.pi * 1000.0 * t / rate)
    X[3] = rng.uniform(-1, 1, (2, S))  # never read: valid = 0
    X[4] = rng.uniform(-1, 1, (2, S))
    q = min(S - 1, max(0, 2 * H + first + W // 2 + 3))  # the unit impulse, inside frame 2
    X[5, :, q] = 1.0
    valid = [S, S, S, 0, min(S - 1, max(1, 2 * H + first + W // 2)), S]
    X.setflags(write=False)
    return X, valid


def reference(cfg, frames, first, X, valid, window, triangles, opt):
    """{scale: R[row, channel, frame, band]} by rule_front and the rule."""
    rate, N, W, H, B = cfg
    tw, win, fb = front_tables(rate, N, W, B, window, triangles)
    u = np.concatenate([rule_front(X[r, ch], valid[r], first, frames, N, W, H, win, **opt) for r in range(X.shape[0]) for ch in range(2)])
    m = rule_mel(rule_power(u, tw), fb).reshape(X.shape[0], 2, frames, B)
    R = {s: rule_scale(m, s, 1e-10) for s in set(v[1] for v in LAUNCHES.values())}
    for r in R.values():
        assert r.dtype == F32
        r.setflags(write=False)
    return R


def run_front(gpu_ctx, cfg, frames, first, X, valid, front, layout, band_major, scale):
    """One launch with the strides of tests/test_mel_rows.py (gaps between channels and rows, a tail): the values [row, channel,
    frame, band] after the sentinels have been checked."""
    torch = _torch()
    rate, N, W, H, B = cfg
    rows, S = X.shape[0], X.shape[2]
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
    fstr, bstr = (1, frames) if band_major else (B, 1)
    d_dst = torch.full((rows * rs + 64,), float(SENT), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    desc = make_desc(rate, N, W, B, hop=H, scale=scale, rows=rows, channels=C_, frames=frames, first=first, src_length=S,
                     src_row_stride=sstr[0], src_time_stride=sstr[1], src_chan_stride=sstr[2], dst_row_stride=rs, dst_chan_stride=cs,
                     dst_frame_stride=fstr, dst_band_stride=bstr)
    gpu_ctx.mel_rows(desc, d_src.data_ptr(), d_dst.data_ptr(), valid, front)
    gpu_ctx.synchronize()
    got = d_dst.cpu().numpy()
    assert (got[rows * rs:] == SENT).all(), "written behind the destination"
    got = got[:rows * rs].reshape(rows, rs)
    assert (got[:, C_ * cs:] == SENT).all(), "written between the rows"
    got = got[:, :C_ * cs].reshape(rows, C_, cs)
    assert (got[:, :, frames * B:] == SENT).all(), "written between the channels"
    got = got[:, :, :frames * B]
    return np.ascontiguousarray(got.reshape(rows, C_, B, frames).transpose(0, 1, 3, 2) if band_major else got.reshape(rows, C_, frames, B))


def check(got, want, tag):
    bad = np.argwhere(got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    assert not len(bad), (tag, len(bad), bad[:4].tolist(), [(float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:4]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(OPTIONS))
@pytest.mark.parametrize("frames", [1, 4, 7])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_front_kernel_alone(gpu_ctx, cfg, frames, name):
    """nvh_mel_rows_front on the rows of tests/test_mel_rows.py's kernel test, each option alone and all together (gain 32768, DC,
    p = 0.97, Povey, mel triangles), interleaved, planar and mono sources, both destination orders, the three scales between them:
    every value equals rule_front + the rule, the gaps and the tail keep their sentinel.  "default": a front at today's values --
    the rule's values and, bit for bit, nvh_mel_rows' own output."""
    rate, N, W, H, B = cfg
    window, triangles, opt = OPTIONS[name]
    first = (N - W) // 2 - N // 2  # negative: the first frames read in front of the row
    S = 6 * H + first + W - 5      # ... and frame 6 behind it
    key = (cfg, frames, name)
    if key not in _CASES:
        X, valid = source_rows(cfg, frames, first, S)
        _CASES[key] = (X, valid, reference(cfg, frames, first, X, valid, window, triangles, opt))
    X, valid, R = _CASES[key]
    front = make_front(window, triangles, **opt)
    for layout, (band_major, scale) in LAUNCHES.items():
        got = run_front(gpu_ctx, cfg, frames, first, X, valid, front, layout, band_major, scale)
        check(got, R[scale][:, :got.shape[1]], (cfg, frames, name, layout))
        if name == "default":
            check(run_front(gpu_ctx, cfg, frames, first, X, valid, None, layout, band_major, scale), got, (cfg, frames, "nvh_mel_rows", layout))
    if name == "all":  # zeros and valid = 0 stay the floor's value under every option: 0 * g - mean(0) - p 0 = 0
        z = R["ln"][2:4]
        assert same_bits(z, np.full_like(z, rule_scale(F32([0]), "ln", 1e-10)[0]))


REFLECT = {"reflect": ("hann", "hz", {"reflect": True}), "reflect, all": ("povey", "mel", dict(ALL, reflect=True))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFLECT))
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_front_reflection(gpu_ctx, cfg, cut, name):
    """NVH_PAD_REFLECT with first = -(W div 2) and seven frames, the last of which reaches four samples past L: reads in front of
    the row and behind it are mirrored.  cut=False: valid == L for every row.  cut=True: valid < L, so that the mirrored reads
    behind L - 1 land in the zeros (a row ending 7 samples early, valid = 0, a row ending inside frame 2)."""
    rate, N, W, H, B = cfg
    window, triangles, opt = REFLECT[name]
    frames, first = 7, -(W // 2)
    S = 6 * H + first + W - 4
    assert 6 * H + first + W - 1 == S + 3 <= 2 * (S - 1) and -first <= S - 1
    key = (cfg, cut, name)
    if key not in _CASES:
        X, valid = source_rows(cfg, 70 + cut, first, S)
        valid = [S, S - 7, S, 0, valid[4], S - 1] if cut else [S] * 6
        _CASES[key] = (X, valid, reference(cfg, frames, first, X, valid, window, triangles, opt))
    X, valid, R = _CASES[key]
    front = make_front(window, triangles, **opt)
    for layout, (band_major, scale) in LAUNCHES.items():
        got = run_front(gpu_ctx, cfg, frames, first, X, None if not cut and layout == "planar" else valid, front, layout, band_major, scale)
        check(got, R[scale][:, :got.shape[1]], (cfg, cut, name, layout))
    if name == "reflect":  # the mirror shows: the last frame differs from the zero-padded one on the noise row
        tw, win, fb = front_tables(rate, N, W, B)
        zero = rule_mel(rule_power(rule_front(X[0, 0], S, first, frames, N, W, H, win), tw), fb)
        assert not same_bits(np.ascontiguousarray(R["power"][0, 0, 6]), zero[6]) and not same_bits(np.ascontiguousarray(R["power"][0, 0, 0]), zero[0])


# ---------------------------------------------------------------------------------------------------------------------------
# through decode_clip_features
# ---------------------------------------------------------------------------------------------------------------------------

LENGTH = 4000


def clip_rows(ogg_bytes):
    """Two short clips of 3test.ogg at its own 44100 Hz: from the start, and across the clip's end (valid < LENGTH)."""
    import nvorbis_amd as nv
    pa = nv.demux_ogg_array(ogg_bytes["3test"], 0)
    st = nv.Stream(None, pa[0], pa[1], pa[2])
    try:
        total = st.index_packets(pa, 3)[3]
    finally:
        st.close()
    return [ogg_bytes["3test"]] * 2, [0, total - 1500]


def want_clip_features(oracle, ogg_bytes, starts, kw, first, F):
    """((rows, n_mels, F) features, valid, valid_frames): oracle PCM -> the mono mix -> rule_front -> the mel rule."""
    from tests.test_resample_rows import want_row
    N, W, H, B = kw.get("n_fft", 512), kw.get("win_length", 400), kw.get("hop", 160), kw.get("n_mels", 80)
    tw, win, fb = front_tables(44100, N, W, B, kw.get("window", "hann"), kw.get("mel_triangles", "hz"), f_min=kw.get("f_min", 0.0),
                               f_max=kw.get("f_max"))
    feats, valids, vfs = [], [], []
    for start in starts:
        row, valid, _, _ = want_row(oracle, ogg_bytes, "3test", 44100, 44100, "mono", start, LENGTH)
        u = rule_front(row[:, 0], valid, first, F, N, W, H, win, reflect=kw.get("pad_mode") == "reflect", remove_dc=kw.get("remove_dc", False),
                       preemphasis=kw.get("preemphasis", 0.0), gain=kw.get("sample_gain", 1.0))
        feats.append(rule_scale(rule_mel(rule_power(u, tw), fb), kw.get("scale", "ln"), kw.get("floor", 1e-10)).T)
        begins = np.arange(F) * H + first  # the unreflected positions
        valids.append(valid)
        vfs.append(int((np.maximum(begins, 0) < np.minimum(begins + W, valid)).sum()))
    return np.stack(feats), np.asarray(valids), np.asarray(vfs)


@pytest.mark.gpu
def test_decode_clip_features_with_a_front(oracle, gpu_ctx, ogg_bytes):
    """decode_clip_features(**kaldi_fbank_keywords(44100)) and a call with pad_mode="reflect", mono mix, on two short clips: the
    features equal oracle PCM through the numpy rules, as uint32; valid_frames follows its formula.  A call without any new keyword
    gives the same tensor before and after them."""
    _torch()
    import nvorbis_amd as nv
    files, starts = clip_rows(ogg_bytes)
    common = dict(ctx=gpu_ctx, batch_frames=16, mix="mono")
    before, valid0, vf0 = nv.decode_clip_features(files, LENGTH, starts, **common)

    kw = nv.kaldi_fbank_keywords(44100)
    assert (kw["n_fft"], kw["win_length"], kw["hop"]) == (2048, 1102, 441)
    F = (LENGTH - 1102) // 441 + 1
    want, want_valid, want_vf = want_clip_features(oracle, ogg_bytes, starts, kw, 0, F)
    feats, valid, vf = nv.decode_clip_features(files, LENGTH, starts, **kw, **common)
    assert feats.is_cuda and tuple(feats.shape) == want.shape == (2, 80, F)
    assert np.array_equal(valid, want_valid) and valid[0] == LENGTH and 0 < valid[1] < LENGTH
    assert np.array_equal(vf, want_vf) and vf[0] == F and 0 < vf[1] < F
    assert same_bits(feats.cpu().numpy(), want)

    kw = dict(pad_mode="reflect")
    F = LENGTH // 160 + 1
    want, want_valid, want_vf = want_clip_features(oracle, ogg_bytes, starts, kw, -200, F)
    feats, valid, vf = nv.decode_clip_features(files, LENGTH, starts, **kw, **common)
    assert tuple(feats.shape) == want.shape == (2, 80, F) and np.array_equal(valid, want_valid) and np.array_equal(vf, want_vf)
    assert same_bits(feats.cpu().numpy(), want)
    # ... which is not the zero-padded call: frame 0 of the first row sees the mirror, and so does its last frame
    host = before.cpu().numpy()
    assert not same_bits(np.ascontiguousarray(host[0, :, 0]), np.ascontiguousarray(want[0, :, 0]))
    assert not same_bits(np.ascontiguousarray(host[0, :, F - 1]), np.ascontiguousarray(want[0, :, F - 1]))
    assert same_bits(np.ascontiguousarray(host[0, :, 2:F - 2]), np.ascontiguousarray(want[0, :, 2:F - 2]))  # ... and the inner frames do not

    after, valid1, vf1 = nv.decode_clip_features(files, LENGTH, starts, **common)
    assert same_bits(after.cpu().numpy(), host) and np.array_equal(valid0, valid1) and np.array_equal(vf0, vf1)
    want, _, _ = want_clip_features(oracle, ogg_bytes, starts, {}, -200, F)
    assert same_bits(host, want)

"""The log-mel features' host side (nvh_mel_plan, nvh_mel_tables; include/nvorbis_hip.h states the rule under nvh_mel_rows): the
tables against the formulas in numpy double, the rule restated in numpy -- written from the header's text, fed the library's own
tables -- against float64, the rule's logarithm against float64 log, and every argument check.  No device anywhere.

tests/test_mel_rows.py holds the kernel to rule_features() below bit for bit."""
import ctypes as C

import numpy as np
import pytest

# (rate, n_fft, win_length, n_mels)
CONFIGS = [(16000, 512, 400, 80), (8000, 64, 64, 8), (48000, 4096, 4096, 128), (44100, 2048, 1103, 256)]
HOPS = {512: 160, 64: 16, 4096: 5000, 2048: 441}
F32 = np.float32


def make_desc(rate=16000, n_fft=512, win_length=400, n_mels=80, hop=160, mel_scale="htk", norm=None, scale="ln", floor=1e-10,
              f_min=0.0, f_max=None, **kw):
    from nvorbis_amd import native
    d = native.MelDesc(rate=rate, n_fft=n_fft, win_length=win_length, hop=hop, n_mels=n_mels,
                       mel_scale={"htk": native.MEL_HTK, "slaney": native.MEL_SLANEY}.get(mel_scale, mel_scale),
                       norm={None: native.MEL_NORM_NONE, "slaney": native.MEL_NORM_SLANEY}.get(norm, norm),
                       scale={"power": native.MEL_POWER, "ln": native.MEL_LN, "db": native.MEL_DB}.get(scale, scale),
                       floor=floor, f_min=f_min, f_max=rate / 2.0 if f_max is None else f_max)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


_TABLES = {}


def lib_tables(rate, n_fft, win_length, n_mels, mel_scale="htk", norm=None):
    """(twiddles (n_fft / 2 + 1, 2), window (win_length,), bank (n_mels, n_fft / 2 + 1)) from nvh_mel_tables, read-only, once."""
    from nvorbis_amd import native
    key = (rate, n_fft, win_length, n_mels, mel_scale, norm)
    if key not in _TABLES:
        d = make_desc(rate, n_fft, win_length, n_mels, mel_scale=mel_scale, norm=norm)
        bins = n_fft // 2 + 1
        counts = [C.c_int64(0) for _ in range(3)]
        assert native.lib().nvh_mel_plan(C.byref(d), *[C.byref(c) for c in counts]) == native.OK
        assert [c.value for c in counts] == [2 * bins, win_length, n_mels * bins]
        tw, win, fb = np.zeros(2 * bins, F32), np.zeros(win_length, F32), np.zeros(n_mels * bins, F32)
        rc = native.lib().nvh_mel_tables(C.byref(d), tw.ctypes.data, win.ctypes.data, fb.ctypes.data, tw.size, win.size, fb.size,
                                         *[C.byref(c) for c in counts])
        assert rc == native.OK and [c.value for c in counts] == [2 * bins, win_length, n_mels * bins]
        out = (tw.reshape(bins, 2), win, fb.reshape(n_mels, bins))
        for a in out:
            a.setflags(write=False)
        _TABLES[key] = out
    return _TABLES[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the formulas, in double
# ---------------------------------------------------------------------------------------------------------------------------

def hz_to_mel(f, mel_scale):
    f = np.asarray(f, np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m, mel_scale):
    m = np.asarray(m, np.float64)
    if mel_scale == "htk":
        return 700.0 * (np.power(10.0, m / 2595.0) - 1.0)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)))


def formula_tables(rate, n_fft, win_length, n_mels, mel_scale="htk", norm=None, f_min=0.0, f_max=None):
    """The three tables in double, not yet rounded."""
    f_max = rate / 2.0 if f_max is None else f_max
    k = np.arange(n_fft // 2 + 1, dtype=np.float64)
    a = 2.0 * np.pi * k / n_fft
    tw = np.stack([np.cos(a), np.sin(a)], axis=1)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)
    m_lo, m_hi = float(hz_to_mel(f_min, mel_scale)), float(hz_to_mel(f_max, mel_scale))
    pt = mel_to_hz(m_lo + (m_hi - m_lo) * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1), mel_scale)
    f = k * rate / n_fft
    l, c, r = pt[:-2, None], pt[1:-1, None], pt[2:, None]
    fb = np.maximum(0.0, np.minimum((f[None, :] - l) / (c - l), (r - f[None, :]) / (r - c)))
    if norm == "slaney":
        fb = fb * (2.0 / (r - l))
    return tw, win, fb


# ---------------------------------------------------------------------------------------------------------------------------
# the rule, in numpy float32 (every operation rounded on its own: numpy fuses nothing)
# ---------------------------------------------------------------------------------------------------------------------------

def rule_ln(v):
    v = np.asarray(v, F32)
    g, e = np.frexp(v)  # v = g 2^e, g in [0.5, 1)
    g, e = g.astype(F32), e.astype(np.int32)
    low = g < F32(0.70710678)
    g = np.where(low, g + g, g).astype(F32)
    e = np.where(low, e - 1, e)
    s = ((g - F32(1)) / (g + F32(1))).astype(F32)
    z = s * s
    p = np.full_like(s, F32(1.0 / 11.0))
    for c in (F32(1.0 / 9.0), F32(1.0 / 7.0), F32(1.0 / 5.0), F32(1.0 / 3.0), F32(1)):
        p = p * z + c
    return e.astype(F32) * F32(0.6931471805599453) + (s + s) * p


def rule_frames(x, valid, first, frames, n_fft, win_length, hop, win):
    """u of frames 0 .. frames - 1 of one (row, channel): (frames, n_fft) float32.  x: the row's samples; 0 outside [0, valid)."""
    x = np.asarray(x, F32)
    valid = min(int(valid), x.size)
    t = np.arange(frames, dtype=np.int64)[:, None] * hop + first + np.arange(win_length, dtype=np.int64)[None, :]
    ok = (t >= 0) & (t < valid)
    xs = np.where(ok, x[np.clip(t, 0, max(x.size - 1, 0))] if x.size else F32(0), F32(0)).astype(F32)
    u = np.zeros((frames, n_fft), F32)
    off = (n_fft - win_length) // 2
    u[:, off:off + win_length] = xs * win[None, :]
    return u


def rule_power(u, tw):
    """P of every frame: (frames, n_fft / 2 + 1) float32."""
    F, N = u.shape
    NP = N // 2
    bits = NP.bit_length() - 1
    rev = np.zeros(NP, np.int64)
    for b in range(bits):
        rev |= ((np.arange(NP) >> b) & 1) << (bits - 1 - b)
    zr, zi = np.zeros((F, NP), F32), np.zeros((F, NP), F32)
    zr[:, rev] = u[:, 0::2]
    zi[:, rev] = u[:, 1::2]
    half = 1
    while half < NP:
        j = np.arange(half)
        c, s = tw[j * (N // (2 * half)), 0], tw[j * (N // (2 * half)), 1]
        zr, zi = zr.reshape(F, -1, 2, half), zi.reshape(F, -1, 2, half)
        ar, ai, br, bi = zr[:, :, 0], zi[:, :, 0], zr[:, :, 1], zi[:, :, 1]
        tr = br * c + bi * s
        ti = bi * c - br * s
        zr = np.stack([ar + tr, ar - tr], axis=2).reshape(F, NP)
        zi = np.stack([ai + ti, ai - ti], axis=2).reshape(F, NP)
        half *= 2
    k = np.arange(NP + 1)
    ar, ai = zr[:, k % NP], zi[:, k % NP]
    br, bi = zr[:, (NP - k) % NP], -zi[:, (NP - k) % NP]
    er, ei, dr, di = ar + br, ai + bi, ar - br, ai - bi
    c, s = tw[k, 0], tw[k, 1]
    tr = c * di - s * dr
    ti = -(c * dr + s * di)
    xr, xi = er + tr, ei + ti
    P = F32(0.25) * (xr * xr + xi * xi)
    assert P.dtype == F32
    return P


def rule_mel(P, fb):
    m = np.zeros((P.shape[0], fb.shape[0]), F32)
    for b in range(fb.shape[0]):
        acc = np.zeros(P.shape[0], F32)
        for k in np.nonzero(fb[b])[0]:
            acc = acc + P[:, k] * fb[b, k]
        m[:, b] = acc
    return m


def rule_scale(m, scale, floor):
    if scale == "power":
        return m
    v = rule_ln(np.maximum(m, F32(floor)))
    return v if scale == "ln" else v * F32(10.0 / np.log(10.0))


def rule_features(x, valid, first, frames, tables, n_fft, win_length, hop, scale="ln", floor=1e-10):
    """(frames, n_mels) float32 of one (row, channel) by the rule, from the library's tables."""
    tw, win, fb = tables
    out = rule_scale(rule_mel(rule_power(rule_frames(x, valid, first, frames, n_fft, win_length, hop, win), tw), fb), scale, floor)
    assert out.dtype == F32
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the tables
# ---------------------------------------------------------------------------------------------------------------------------

# (config, mel_scale, norm, table, slot) of every slot where this libm's double and numpy's straddle an f32 rounding boundary: none
STRADDLES = []


@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("mel_scale", ["htk", "slaney"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_tables_are_the_formulas_rounded_once(cfg, mel_scale, norm):
    """uint32 equality with np.float32(formula in double); at most one slot per table one ulp off (listed in STRADDLES if so)."""
    got = lib_tables(*cfg, mel_scale=mel_scale, norm=norm)
    want = formula_tables(*cfg, mel_scale=mel_scale, norm=norm)
    for name, g, w in zip(("twiddles", "window", "bank"), got, want):
        w32 = w.astype(F32)
        assert g.shape == w32.shape, name
        off = np.argwhere(g.view(np.uint32) != w32.view(np.uint32))
        for slot in off:
            print("straddle:", cfg, mel_scale, norm, name, tuple(slot), g[tuple(slot)], w32[tuple(slot)])
        assert len(off) <= 1, (name, len(off))
        for slot in off:
            s = tuple(slot)
            assert abs(float(g[s]) - float(w32[s])) <= float(np.spacing(np.abs(w32[s]))), (name, s)
            assert (cfg, mel_scale, norm, name, s) in STRADDLES, (cfg, mel_scale, norm, name, s)
    assert got[1][0] == 0  # the periodic Hann window begins at 0 (W = 1: its only sample)


def test_bands_without_a_bin_are_zero_rows_and_w1_is_zero():
    tw, win, fb = lib_tables(8000, 64, 1, 256)  # 256 bands over 33 bins: most bands hold no bin
    assert win.shape == (1,) and win[0] == 0
    empty = ~fb.any(axis=1)
    assert empty.any() and not empty.all()
    # non-zero bins of a band are consecutive (what the kernel's sparse bank relies on)
    for cfg in CONFIGS:
        for row in lib_tables(*cfg, mel_scale="slaney", norm="slaney")[2]:
            nz = np.nonzero(row)[0]
            assert nz.size == 0 or nz[-1] - nz[0] + 1 == nz.size


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the rule against float64
# ---------------------------------------------------------------------------------------------------------------------------

def signals(rate, n):
    rng = np.random.default_rng(rate + n)
    t = np.arange(n, dtype=np.float64)
    return {"noise": rng.uniform(-1, 1, n).astype(F32), "tone": (0.8 * np.sin(2 * np.pi * 1000.0 * t / rate)).astype(F32)}


@pytest.mark.parametrize("cfg", CONFIGS)
def test_rule_against_float64(cfg):
    """|rule - f64| <= 8 * 2^-24 * sum_k P64[k] of the frame, for every frame and band, POWER scale, noise and a 1 kHz tone, both mel
    scales and both norms.  Measured maxima in that unit (printed): (16000, 512, 400, 80) 1.61, (8000, 64, 64, 8) 1.92,
    (48000, 4096, 4096, 128) 2.52, (44100, 2048, 1103, 256) 1.64."""
    rate, N, W, B = cfg
    H, F = HOPS[N], 7
    worst = 0.0
    for name, x in signals(rate, 6 * H + N).items():
        for mel_scale in ("htk", "slaney"):
            for norm in (None, "slaney"):
                tw, win, fb = lib_tables(*cfg, mel_scale=mel_scale, norm=norm)
                first = (N - W) // 2 - N // 2
                u = rule_frames(x, x.size, first, F, N, W, H, win)
                got = rule_mel(rule_power(u, tw), fb).astype(np.float64)
                t = np.arange(F)[:, None] * H + first + np.arange(W)[None, :]
                xs = np.where((t >= 0) & (t < x.size), x.astype(np.float64)[np.clip(t, 0, x.size - 1)], 0.0)
                u64 = np.zeros((F, N))
                u64[:, (N - W) // 2:(N - W) // 2 + W] = xs * win.astype(np.float64)[None, :]
                P64 = np.abs(np.fft.rfft(u64, axis=1)) ** 2
                want = P64 @ fb.astype(np.float64).T
                unit = 2.0 ** -24 * P64.sum(axis=1)[:, None]
                assert (unit > 0).all()
                worst = max(worst, float((np.abs(got - want) / unit).max()))
    print("rule against float64, %r: max |rule - f64| / (2^-24 sum P64) = %.3f" % (cfg, worst))
    assert worst <= 8.0, worst


def test_ln_r_against_float64_log():
    """ln_r within 4 ulp of float64 log on 1e6 log-uniform values in [1e-10, 1e8].  Measured (printed): 2.59 ulp, 2.14e-7 relative."""
    rng = np.random.default_rng(7)
    v = np.exp(rng.uniform(np.log(1e-10), np.log(1e8), 1000000)).astype(F32)
    v = np.concatenate([v, np.asarray([1e-10, 1e8, 1.0, 0.5, 0.70710678, 2.0 ** -126], F32)])
    got = rule_ln(v)
    assert got.dtype == F32
    want = np.log(v.astype(np.float64))
    ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(F32)).astype(np.float64)
    inside = v >= F32(1e-10)
    rel = np.abs(got.astype(np.float64) - want)[want != 0] / np.abs(want[want != 0])
    print("ln_r: max %.2f ulp, max relative %.2e" % (float(ulp[inside & (want != 0)].max()), float(rel.max())))
    assert float(ulp[inside & (want != 0)].max()) <= 4.0
    assert got[-4] == 0  # ln_r(1) = 0 exactly


# ---------------------------------------------------------------------------------------------------------------------------
# 3. argument errors, each before NVH_ERR_NO_GPU
# ---------------------------------------------------------------------------------------------------------------------------

BAD_PARAMETERS = [
    {"rate": 0}, {"rate": -16000}, {"n_fft": 32}, {"n_fft": 8192}, {"n_fft": 400}, {"n_fft": 0}, {"win_length": 0}, {"win_length": 513},
    {"hop": 0}, {"hop": 65537}, {"n_mels": 0}, {"n_mels": 257}, {"f_min": -1.0}, {"f_min": 8000.0}, {"f_min": 4000.0, "f_max": 4000.0},
    {"f_max": 8000.5}, {"f_min": float("nan")}, {"f_max": float("nan")}, {"mel_scale": 2}, {"mel_scale": -1}, {"norm": 2}, {"scale": 3},
    {"scale": -1}, {"floor": 0.0}, {"floor": -1.0}, {"floor": 1e-39}, {"floor": float("nan")}, {"floor": float("inf")}, {"frames": -1},
    {"frames": (1 << 40) + 1}, {"first": (1 << 60) + 1}, {"first": -(1 << 60) - 1},
]


def test_plan_and_tables_check_their_arguments():
    from nvorbis_amd import native
    L = native.lib()
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    ptrs = [C.byref(a), C.byref(b), C.byref(c)]
    buf = np.zeros(4096, F32)
    p = buf.ctypes.data
    good = make_desc()
    assert L.nvh_mel_plan(C.byref(good), *ptrs) == native.OK and (a.value, b.value, c.value) == (514, 400, 80 * 257)
    assert L.nvh_mel_plan(None, *ptrs) == native.ERR_ARGUMENT
    for k in range(3):
        args = list(ptrs)
        args[k] = None
        assert L.nvh_mel_plan(C.byref(good), *args) == native.ERR_ARGUMENT, k
        assert L.nvh_mel_tables(C.byref(good), None, None, None, 0, 0, 0, *args) == native.ERR_ARGUMENT, k
    for bad in BAD_PARAMETERS:
        assert L.nvh_mel_plan(C.byref(make_desc(**bad)), *ptrs) == native.ERR_ARGUMENT, bad
        assert L.nvh_mel_tables(C.byref(make_desc(**bad)), None, None, None, 0, 0, 0, *ptrs) == native.ERR_ARGUMENT, bad
    # the limits themselves are inside
    for ok in ({"n_fft": 64, "win_length": 1}, {"n_fft": 4096, "win_length": 4096}, {"hop": 65536}, {"n_mels": 256}, {"floor": 2.0 ** -126},
               {"f_min": 7999.0}, {"frames": 1 << 40, "first": -(1 << 60)}, {"rate": 1, "f_max": 0.5}):
        assert L.nvh_mel_plan(C.byref(make_desc(**ok)), *ptrs) == native.OK, ok
    # the tables: counts are set even when a cap is too small; a table left out with (NULL, 0) is fine
    assert L.nvh_mel_tables(None, None, None, None, 0, 0, 0, *ptrs) == native.ERR_ARGUMENT
    a.value = b.value = c.value = -1
    assert L.nvh_mel_tables(C.byref(good), p, None, None, 8, 0, 0, *ptrs) == native.ERR_ARGUMENT
    assert (a.value, b.value, c.value) == (514, 400, 80 * 257) and not buf.any()
    assert L.nvh_mel_tables(C.byref(good), None, p, None, 0, 399, 0, *ptrs) == native.ERR_ARGUMENT and not buf.any()
    assert L.nvh_mel_tables(C.byref(good), None, None, p, 0, 0, 4096, *ptrs) == native.ERR_ARGUMENT and not buf.any()
    assert L.nvh_mel_tables(C.byref(good), None, None, None, 8, 0, 0, *ptrs) == native.ERR_ARGUMENT  # a cap without a buffer
    assert L.nvh_mel_tables(C.byref(good), p, None, None, -1, 0, 0, *ptrs) == native.ERR_ARGUMENT
    assert L.nvh_mel_tables(C.byref(good), None, p, None, 0, 400, 0, *ptrs) == native.OK and buf[:400].any() and not buf[400:].any()
    assert L.nvh_mel_tables(C.byref(good), None, None, None, 0, 0, 0, *ptrs) == native.OK


def test_rows_entry_point_checks_its_arguments_before_a_device():
    """nvh_mel_rows without a context: every argument error comes first, then NVH_ERR_NO_GPU."""
    from nvorbis_amd import native
    L = native.lib()
    fake = C.c_void_p(4096)  # never dereferenced: there is no context
    shape = dict(rows=2, channels=1, frames=5, first=-200, src_length=1000, src_row_stride=1000, src_time_stride=1, src_chan_stride=0,
                 dst_row_stride=400, dst_chan_stride=400, dst_frame_stride=80, dst_band_stride=1)

    def call(d, valid=(1000, 0), src=fake, dst=fake):
        v = None if valid is None else (C.c_int64 * len(valid))(*valid)
        return L.nvh_mel_rows(None, None if d is None else C.byref(d), src, dst, v)
    assert call(None) == native.ERR_ARGUMENT
    for bad in BAD_PARAMETERS:
        assert call(make_desc(**dict(shape, **bad))) == native.ERR_ARGUMENT, bad
    for bad in ({"rows": -1}, {"src_length": -1}, {"channels": 0}, {"channels": 65536}):
        assert call(make_desc(**dict(shape, **bad))) == native.ERR_ARGUMENT, bad
    assert call(make_desc(**shape), src=None) == native.ERR_ARGUMENT and call(make_desc(**shape), dst=None) == native.ERR_ARGUMENT
    assert call(make_desc(**shape), valid=(1001, 0)) == native.ERR_ARGUMENT and call(make_desc(**shape), valid=(5, -1)) == native.ERR_ARGUMENT
    assert call(make_desc(**dict(shape, rows=1 << 30, channels=65535, frames=1 << 40)), valid=None) == native.ERR_ARGUMENT  # work items beyond 64 bits
    assert call(make_desc(**shape)) == native.ERR_NO_GPU and call(make_desc(**shape), valid=None) == native.ERR_NO_GPU
    assert call(make_desc(**dict(shape, rows=0)), valid=None, src=None, dst=None) == native.ERR_NO_GPU  # (nothing to do, but no context either)
    assert call(make_desc(**dict(shape, frames=0)), src=None, dst=None) == native.ERR_NO_GPU


def test_decode_clip_features_refuses_bad_keywords_before_a_device(ogg_bytes):
    """Every ValueError of decode_clip_features, on a machine that may have no device at all."""
    import nvorbis_amd as nv
    from tests.test_resample_rows import clip_at
    good = ogg_bytes["3test"]  # 44100 Hz
    bads = [{"n_fft": 400}, {"n_fft": 32}, {"n_fft": 8192}, {"n_fft": 512.0}, {"n_fft": True}, {"win_length": 0}, {"win_length": 513},
            {"win_length": "400"}, {"hop": 0}, {"hop": 65537}, {"hop": 1.5}, {"n_mels": 0}, {"n_mels": 257}, {"f_min": -1.0},
            {"f_min": 30000.0}, {"f_max": 22050.5}, {"f_min": 100.0, "f_max": 100.0}, {"f_min": "0"}, {"f_max": float("nan")},
            {"mel_scale": "mel"}, {"mel_scale": None}, {"mel_scale": 0}, {"norm": "none"}, {"norm": 1}, {"scale": "log"}, {"scale": None},
            {"floor": 0.0}, {"floor": -1e-10}, {"floor": 1e-39}, {"floor": float("inf")}, {"floor": "1e-10"}, {"center": 1},
            {"band_major": None}, {"device_out": 0}, {"return_clipped": 1}, {"sample_rate": 0}, {"sample_rate": 16000.0},
            {"sample_rate": 44101}, {"mix": "stereo"}, {"channel_map": (0, 0)}, {"channel_map": (0,), "mix": "mono"},
            {"batch_frames": 0}, {"sample_rate": 16000, "f_max": 8000.5}]
    for bad in bads:
        with pytest.raises(ValueError):
            nv.decode_clip_features([good], 4000, **bad)
    for length in (-1, 4000.0, True):
        with pytest.raises(ValueError):
            nv.decode_clip_features([good], length)
    with pytest.raises(ValueError):
        nv.decode_clip_features([good], 511, center=False)  # length < n_fft
    with pytest.raises(ValueError):
        nv.decode_clip_features([good], 4000, [-1])
    with pytest.raises(ValueError):
        nv.decode_clip_features([good, good], 4000, [0])
    with pytest.raises(ValueError):  # without sample_rate all clips share one rate
        nv.decode_clip_features([good, clip_at(ogg_bytes, "3test", 48000)], 4000)
    with pytest.raises(ValueError):  # ... and there is a rate to take
        nv.decode_clip_features([], 4000)
    with pytest.raises(ValueError):  # mono and stereo clips in one tensor
        nv.decode_clip_features([good, ogg_bytes["1test"]], 4000)
    with pytest.raises(TypeError):
        nv.decode_clip_features([good], 4000, None, 16000)  # the keywords are keyword-only


def test_mel_tables_in_python_are_the_librarys():
    from nvorbis_amd import clips
    got = clips.mel_tables(44100, 2048, 1103, 256, mel_scale="slaney", norm="slaney")
    for g, w in zip(got, lib_tables(44100, 2048, 1103, 256, "slaney", "slaney")):
        assert g.dtype == F32 and g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    with pytest.raises(ValueError):
        clips.mel_tables(16000, 500)

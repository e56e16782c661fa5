"""The front of a log-mel frame on the host (nvh_mel_front_check, nvh_mel_tables_front; include/nvorbis_hip.h states the rule under
nvh_mel_front): the windows and the mel-domain triangles against the formulas in numpy double, the front restated in numpy --
rule_front, written from the header's text -- against float64, every argument check, the distance to Kaldi's fbank, and the launch
route of every case of tests/test_mel_front.py.  No device anywhere.

tests/test_mel_front.py holds the kernel to rule_front() + the rule of tests/test_mel_plan.py bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests.test_fnorm_plan import rule_sum64 as sum64
from tests.test_mel_plan import F32, hz_to_mel, lib_tables, make_desc, mel_to_hz, rule_mel, rule_power, rule_scale
from tests.test_row_routes import defines, mel_route

WINDOWS = ("hann", "hann_symmetric", "hamming", "povey", "rectangular")
TRIANGLES = ("hz", "mel")
# (rate, n_fft, win_length, n_mels)
CONFIGS = [(16000, 512, 400, 80), (8000, 64, 64, 8), (16000, 64, 50, 23), (44100, 2048, 1103, 256)]
HOPS = {(512, 400): 160, (64, 64): 16, (64, 50): 16, (2048, 1103): 441}
# (rate, n_fft, win_length, hop, n_mels) of tests/test_mel_front.py -> staged
GPU_CONFIGS = {(8000, 64, 50, 16, 8): True, (8000, 64, 64, 16, 1): True, (16000, 512, 400, 160, 80): True, (48000, 4096, 4096, 5000, 128): False}


def make_front(window="hann", triangles="hz", reflect=False, remove_dc=False, preemphasis=0.0, gain=1.0, **kw):
    from nvorbis_amd import native
    f = native.MelFront(window=WINDOWS.index(window) if isinstance(window, str) else window,
                        triangles=TRIANGLES.index(triangles) if isinstance(triangles, str) else triangles,
                        pad_mode=int(reflect), remove_dc=int(remove_dc), preemphasis=preemphasis, gain=gain)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


_TABLES = {}


def front_tables(rate, n_fft, win_length, n_mels, window="hann", triangles="hz", mel_scale="htk", norm=None, f_min=0.0, f_max=None):
    """(twiddles, window, bank) from nvh_mel_tables_front, read-only, once."""
    from nvorbis_amd import native
    key = (rate, n_fft, win_length, n_mels, window, triangles, mel_scale, norm, f_min, f_max)
    if key not in _TABLES:
        d = make_desc(rate, n_fft, win_length, n_mels, mel_scale=mel_scale, norm=norm, f_min=f_min, f_max=f_max)
        f = make_front(window, triangles)
        bins = n_fft // 2 + 1
        counts = [C.c_int64(0) for _ in range(3)]
        tw, win, fb = np.zeros(2 * bins, F32), np.zeros(win_length, F32), np.zeros(n_mels * bins, F32)
        rc = native.lib().nvh_mel_tables_front(C.byref(d), C.byref(f), tw.ctypes.data, win.ctypes.data, fb.ctypes.data, tw.size, win.size,
                                               fb.size, *[C.byref(c) for c in counts])
        assert rc == native.OK and [c.value for c in counts] == [2 * bins, win_length, n_mels * bins]
        out = (tw.reshape(bins, 2), win, fb.reshape(n_mels, bins))
        for a in out:
            a.setflags(write=False)
        _TABLES[key] = out
    return _TABLES[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the formulas, in double
# ---------------------------------------------------------------------------------------------------------------------------

def formula_window(kind, W):
    n = np.arange(W, dtype=np.float64)
    if kind == "hann":
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / W)
    den = W - 1 if W > 1 else 1
    c = np.cos(2.0 * np.pi * n / den)
    return {"hann_symmetric": 0.5 - 0.5 * c, "hamming": 0.54 - 0.46 * c, "povey": np.power(0.5 - 0.5 * c, 0.85), "rectangular": np.ones(W)}[kind]


def formula_bank_mel(rate, n_fft, n_mels, mel_scale="htk", norm=None, f_min=0.0, f_max=None):
    """NVH_TRI_MEL in double: the B + 2 points stay on the mel scale, the bins go there."""
    f_max = rate / 2.0 if f_max is None else f_max
    m_lo, m_hi = float(hz_to_mel(f_min, mel_scale)), float(hz_to_mel(f_max, mel_scale))
    pm = m_lo + (m_hi - m_lo) * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1)
    m = hz_to_mel(np.arange(n_fft // 2 + 1, dtype=np.float64) * rate / n_fft, mel_scale)
    l, c, r = pm[:-2, None], pm[1:-1, None], pm[2:, None]
    fb = np.maximum(0.0, np.minimum((m[None, :] - l) / (c - l), (r - m[None, :]) / (r - c)))
    if norm == "slaney":
        hz = mel_to_hz(pm, mel_scale)
        fb = fb * (2.0 / (hz[2:, None] - hz[:-2, None]))
    return fb


# ---------------------------------------------------------------------------------------------------------------------------
# the front, in numpy float32 (every operation rounded on its own)
# ---------------------------------------------------------------------------------------------------------------------------

def front_times(L, first, frames, W, hop, reflect):
    t = np.arange(frames, dtype=np.int64)[:, None] * hop + first + np.arange(W, dtype=np.int64)[None, :]
    if reflect:
        t = np.where(t < 0, -t, np.where(t >= L, 2 * (L - 1) - t, t))
    return t


def rule_front(x, valid, first, frames, n_fft, win_length, hop, win, reflect=False, remove_dc=False, preemphasis=0.0, gain=1.0):
    """u of frames 0 .. frames - 1 of one (row, channel) under a front: (frames, n_fft) float32.  x: the row's src_length samples."""
    x = np.asarray(x, F32)
    L, W = x.size, win_length
    valid = min(int(valid), L)
    t = front_times(L, first, frames, W, hop, reflect)
    ok = (t >= 0) & (t < valid)  # after the reflection
    s = np.where(ok, x[np.clip(t, 0, max(L - 1, 0))] if L else F32(0), F32(0)).astype(F32)
    g, p = F32(gain), F32(preemphasis)
    if g != F32(1):
        s = s * g
    if remove_dc:
        mean = sum64(np.ascontiguousarray(s.T)) / F32(W)  # (frames,)
        s = s - mean[:, None]
    y = s
    if p > 0:
        prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)  # s[n-1]; s[0] under n = 0
        y = s - p * prev
    assert y.dtype == F32
    u = np.zeros((frames, n_fft), F32)
    off = (n_fft - W) // 2
    u[:, off:off + W] = y * win[None, :]
    return u


def front64(x, valid, first, frames, W, hop, reflect=False, remove_dc=False, preemphasis=0.0, gain=1.0, bound=False):
    """y of the same formulas in float64 from the same f32 inputs: (frames, W).  bound=True: the front applied to |x| with every
    subtraction turned into an addition -- what the size of a rounding error of y follows."""
    x = np.asarray(x, F32).astype(np.float64)
    x = np.abs(x) if bound else x
    sign = 1.0 if bound else -1.0
    L = x.size
    t = front_times(L, first, frames, W, hop, reflect)
    ok = (t >= 0) & (t < min(int(valid), L))
    s = np.where(ok, x[np.clip(t, 0, L - 1)], 0.0) * float(F32(gain))
    if remove_dc:
        s = s + sign * s.mean(axis=1, keepdims=True)
    if F32(preemphasis) > 0:
        s = s + sign * float(F32(preemphasis)) * np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the tables
# ---------------------------------------------------------------------------------------------------------------------------

# (config, window or (triangles, mel_scale, norm), slot) of every slot where this libm's double and numpy's straddle an f32 rounding
# boundary: none
STRADDLES = []


def close_tables(tag, got, want64):
    w32 = want64.astype(F32)
    assert got.shape == w32.shape and got.dtype == F32, tag
    off = np.argwhere(got.view(np.uint32) != w32.view(np.uint32))
    for slot in off:
        print("straddle:", tag, tuple(slot), got[tuple(slot)], w32[tuple(slot)])
    assert len(off) <= 1, (tag, len(off))
    for slot in off:
        s = tuple(slot)
        assert abs(float(got[s]) - float(w32[s])) <= float(np.spacing(np.abs(w32[s]))), (tag, s)
        assert tag + (s,) in STRADDLES, tag + (s,)


@pytest.mark.parametrize("cfg", CONFIGS + [(8000, 64, 1, 4)])
def test_windows_are_the_formulas_rounded_once(cfg):
    """uint32 equality with np.float32(formula in double), at most one slot per table one ulp off (listed in STRADDLES if so)."""
    for window in WINDOWS:
        tw, win, fb = front_tables(*cfg, window=window)
        close_tables((cfg, window), win, formula_window(window, cfg[2]))
        base = lib_tables(*cfg)
        assert np.array_equal(tw.view(np.uint32), base[0].view(np.uint32)) and np.array_equal(fb.view(np.uint32), base[2].view(np.uint32))
        if window not in ("hann", "rectangular") and cfg[2] > 2:  # symmetric: the same value from both ends, the ends themselves
            assert np.allclose(win, win[::-1], rtol=0, atol=1e-6)
            assert win[0] == (F32(0.54 - 0.46) if window == "hamming" else 0) and win.max() <= 1
    assert (front_tables(8000, 64, 1, 4, window="rectangular")[1] == 1).all()
    assert front_tables(8000, 64, 1, 4, window="hamming")[1][0] == F32(0.54 - 0.46)  # W = 1: the denominator is 1, n = 0


@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("mel_scale", ["htk", "slaney"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_mel_triangles_are_the_formula_rounded_once(cfg, mel_scale, norm):
    tw, win, fb = front_tables(*cfg, triangles="mel", mel_scale=mel_scale, norm=norm)
    close_tables((cfg, ("mel", mel_scale, norm)), fb, formula_bank_mel(cfg[0], cfg[1], cfg[3], mel_scale, norm))
    base = lib_tables(*cfg, mel_scale=mel_scale, norm=norm)
    assert np.array_equal(tw.view(np.uint32), base[0].view(np.uint32)) and np.array_equal(win.view(np.uint32), base[1].view(np.uint32))
    assert not np.array_equal(fb, base[2])  # ... and it is another bank than the Hz one
    for row in fb:  # the non-zero bins of a band are consecutive (what the kernel's sparse bank relies on)
        nz = np.nonzero(row)[0]
        assert nz.size == 0 or nz[-1] - nz[0] + 1 == nz.size


def test_mel_triangles_on_a_band_limit_and_many_bands():
    fb = front_tables(16000, 512, 400, 23, triangles="mel", f_min=20.0, f_max=7600.0)[2]
    close_tables(("band limit",), fb, formula_bank_mel(16000, 512, 23, "htk", None, 20.0, 7600.0))
    assert not fb[:, 0].any() and not fb[:, 250:].any()  # nothing below f_min or above f_max
    fb = front_tables(8000, 64, 64, 256, triangles="mel")[2]  # 256 bands over 33 bins: most bands hold no bin
    empty = ~fb.any(axis=1)
    assert empty.any() and not empty.all()
    for row in fb:
        nz = np.nonzero(row)[0]
        assert nz.size == 0 or nz[-1] - nz[0] + 1 == nz.size


@pytest.mark.parametrize("cfg", CONFIGS)
def test_a_front_at_todays_values_gives_todays_tables(cfg):
    from nvorbis_amd import clips, native
    for mel_scale, norm in (("htk", None), ("slaney", "slaney")):
        for g, w in zip(front_tables(*cfg, mel_scale=mel_scale, norm=norm), lib_tables(*cfg, mel_scale=mel_scale, norm=norm)):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    # front == NULL is nvh_mel_tables too; and Python's mel_tables takes the two keywords
    d = make_desc(*cfg)
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    win = np.zeros(cfg[2], F32)
    assert native.lib().nvh_mel_tables_front(C.byref(d), None, None, win.ctypes.data, None, 0, win.size, 0, C.byref(a), C.byref(b),
                                             C.byref(c)) == native.OK
    assert np.array_equal(win.view(np.uint32), lib_tables(*cfg)[1].view(np.uint32))
    got = clips.mel_tables(*cfg, window="povey", mel_triangles="mel")
    for g, w in zip(got, front_tables(*cfg, window="povey", triangles="mel")):
        assert g.dtype == F32 and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    for bad in ({"window": "hanning"}, {"window": 3}, {"mel_triangles": "linear"}, {"mel_triangles": None}):
        with pytest.raises(ValueError):
            clips.mel_tables(*cfg, **bad)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. rule_front against float64
# ---------------------------------------------------------------------------------------------------------------------------

ALL = dict(gain=32768.0, remove_dc=True, preemphasis=0.97)
# (window, triangles, the front's options): today's path, every window, the other triangles, each option alone, all together
FRONTS = ([("hann", "hz", {})] + [(w, "hz", {}) for w in WINDOWS[1:]] + [("hann", "mel", {})]
          + [("hann", "hz", o) for o in ({"gain": 32768.0}, {"remove_dc": True}, {"preemphasis": 0.97}, {"reflect": True})]
          + [("povey", "mel", ALL), ("povey", "mel", dict(ALL, reflect=True)), ("hamming", "hz", dict(ALL, gain=1.0))])


def signals(rate, n):
    rng = np.random.default_rng(rate + n)
    t = np.arange(n, dtype=np.float64)
    return {"noise": rng.uniform(-1, 1, n).astype(F32), "tone": (0.8 * np.sin(2 * np.pi * 1000.0 * t / rate)).astype(F32),
            "dc": (0.9 + 0.01 * rng.uniform(-1, 1, n)).astype(F32)}


@pytest.mark.parametrize("cfg", CONFIGS)
def test_rule_front_against_float64(cfg):
    """|rule - f64| <= 8 units for every frame and band, POWER scale, over FRONTS and three signals: noise, a 1 kHz tone, and 0.9 +
    0.01 noise.  The unit is NOT the frame's own sum of P: the DC removal cancels the signal and not the rounding error of the
    samples it was taken from (up to 34 such units on the DC signal).  The unit is 2^-24 * N * sum_n (e[n] win[n])^2, e the front
    applied to |x| with every subtraction turned into an addition (front64(bound=True)): the size the error of u follows, through
    Parseval (sum_k P[k] ~ N/2 sum u^2, and a band sums at most that).  Measured maxima in that unit, the library's tables
    (printed): (16000, 512, 400, 80) 0.81, (8000, 64, 64, 8) 0.93, (16000, 64, 50, 23) 1.00, (44100, 2048, 1103, 256) 0.89."""
    rate, N, W, B = cfg
    H, F = HOPS[(N, W)], 7
    worst, where = 0.0, None
    for name, x in signals(rate, 6 * H + N).items():
        for window, triangles, opt in FRONTS:
            tw, win, fb = front_tables(rate, N, W, B, window, triangles)
            first = (N - W) // 2 - N // 2
            u = rule_front(x, x.size, first, F, N, W, H, win, **opt)
            assert u.dtype == F32
            got = rule_mel(rule_power(u, tw), fb).astype(np.float64)
            w64 = win.astype(np.float64)[None, :]
            u64 = np.zeros((F, N))
            u64[:, (N - W) // 2:(N - W) // 2 + W] = front64(x, x.size, first, F, W, H, **opt) * w64
            want = (np.abs(np.fft.rfft(u64, axis=1)) ** 2) @ fb.astype(np.float64).T
            unit = 2.0 ** -24 * N * ((front64(x, x.size, first, F, W, H, bound=True, **opt) * w64) ** 2).sum(axis=1)[:, None]
            assert (unit > 0).all()
            err = float((np.abs(got - want) / unit).max())
            if err > worst:
                worst, where = err, (name, window, triangles, opt)
    print("rule_front against float64, %r: max |rule - f64| / unit = %.3f at %r" % (cfg, worst, where))
    assert worst <= 8.0, (worst, where)


def test_rule_front_at_todays_values_is_todays_rule():
    from tests.test_mel_plan import rule_frames
    rate, N, W, B = CONFIGS[2]
    x = signals(rate, 300)["noise"]
    win = lib_tables(rate, N, W, B)[1]
    for valid in (300, 120, 0):
        a = rule_front(x, valid, -25, 7, N, W, 16, win)
        assert np.array_equal(a.view(np.uint32), rule_frames(x, valid, -25, 7, N, W, 16, win).view(np.uint32))
    # the zeroing comes after the reflection: with valid < L the mirrored reads behind L - 1 land in the zeros, those in front of 0
    # read counted samples
    ones = np.ones(W, F32)
    u = rule_front(x, 280, -25, 18, N, W, 16, ones, reflect=True)
    off = (N - W) // 2
    assert np.array_equal(u[0, off:off + 25], x[25:0:-1]) and np.array_equal(u[0, off + 25:off + W], x[:W - 25])
    t_last = 17 * 16 - 25 + np.arange(W)  # 247 .. 296
    assert np.array_equal(u[17, off:off + W], np.where(t_last < 280, x[np.minimum(t_last, 299)], 0).astype(F32))
    full = rule_front(x, 300, -25, 19, N, W, 16, ones, reflect=True)  # frame 18: t = 263 .. 312, mirrored at 299
    t18 = 18 * 16 - 25 + np.arange(W)
    assert np.array_equal(full[18, off:off + W], x[np.where(t18 >= 300, 598 - t18, t18)])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. argument errors, each before NVH_ERR_NO_GPU
# ---------------------------------------------------------------------------------------------------------------------------

BAD_FRONTS = [{"window": -1}, {"window": 5}, {"triangles": -1}, {"triangles": 2}, {"pad_mode": -1}, {"pad_mode": 2}, {"remove_dc": -1},
              {"remove_dc": 2}, {"preemphasis": -0.1}, {"preemphasis": 1.5}, {"preemphasis": float("nan")}, {"gain": 0.0}, {"gain": -1.0},
              {"gain": float("inf")}, {"gain": float("nan")}, {"reserved": (1, 0)}, {"reserved": (0, 1)}]
SHAPE = dict(rows=2, channels=1, frames=5, first=-200, src_length=1000, src_row_stride=1000, src_time_stride=1, src_chan_stride=0,
             dst_row_stride=400, dst_chan_stride=400, dst_frame_stride=80, dst_band_stride=1)
# NVH_PAD_REFLECT: (desc fields at the limit, the one field one past it) for L >= 2, -first <= L - 1, (F-1) H + first + W - 1 <= 2 (L-1)
REFLECT_LIMITS = [
    (dict(n_fft=64, win_length=1, hop=1, frames=1, first=0, src_length=2), dict(src_length=1)),       # (with L = 1 the two others hold)
    (dict(n_fft=64, win_length=8, hop=1, frames=1, first=-9, src_length=10), dict(first=-10)),
    (dict(n_fft=64, win_length=19, hop=1, frames=1, first=0, src_length=10), dict(first=1)),
    (dict(n_fft=64, win_length=19, hop=1, frames=1, first=0, src_length=10), dict(win_length=20)),
    (dict(n_fft=512, win_length=400, hop=160, frames=7, first=-200, src_length=581), dict(frames=8)),  # 6 * 160 - 200 + 399 = 1159 <= 1160
    (dict(n_fft=512, win_length=400, hop=160, frames=7, first=-200, src_length=581), dict(src_length=580)),
]


def set_fields(front, kw):
    for k, v in kw.items():
        if k == "reserved":
            front.reserved[0], front.reserved[1] = v
        else:
            setattr(front, k, v)
    return front


def test_front_check_and_the_entry_points_refuse_bad_fronts_before_a_device():
    from nvorbis_amd import native
    from tests.test_mel_plan import BAD_PARAMETERS
    L = native.lib()
    fake = C.c_void_p(4096)  # never dereferenced: there is no context
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    ptrs = [C.byref(a), C.byref(b), C.byref(c)]
    valid = (C.c_int64 * 2)(1000, 0)

    def rows(d, f):
        return L.nvh_mel_rows_front(None, C.byref(d), None if f is None else C.byref(f), fake, fake, valid)
    good = make_desc(**SHAPE)
    assert L.nvh_mel_front_check(None, C.byref(make_front())) == native.ERR_ARGUMENT
    assert L.nvh_mel_front_check(C.byref(good), None) == native.OK and L.nvh_mel_front_check(C.byref(good), C.byref(make_front())) == native.OK
    assert rows(good, None) == native.ERR_NO_GPU and rows(good, make_front()) == native.ERR_NO_GPU
    assert L.nvh_mel_rows_front(None, None, C.byref(make_front()), fake, fake, valid) == native.ERR_ARGUMENT
    for bad in BAD_FRONTS:
        f = set_fields(make_front(), bad)
        assert L.nvh_mel_front_check(C.byref(good), C.byref(f)) == native.ERR_ARGUMENT, bad
        assert L.nvh_mel_tables_front(C.byref(good), C.byref(f), None, None, None, 0, 0, 0, *ptrs) == native.ERR_ARGUMENT, bad
        assert rows(good, f) == native.ERR_ARGUMENT, bad
    # the limits themselves are inside, and so is every constant
    for ok in ({"preemphasis": 0.0}, {"preemphasis": 1.0}, {"gain": 2.0 ** -126}, {"gain": 3.0e38}, {"remove_dc": 1}):
        f = set_fields(make_front(), ok)
        assert L.nvh_mel_front_check(C.byref(good), C.byref(f)) == native.OK and rows(good, f) == native.ERR_NO_GPU, ok
    for w in range(5):
        for t in range(2):
            assert rows(good, make_front(w, t)) == native.ERR_NO_GPU
    # the descriptor's own errors and those of the rows call come through the front calls too
    full = make_front("povey", "mel", False, True, 0.97, 32768.0)
    for bad in BAD_PARAMETERS:
        d = make_desc(**dict(SHAPE, **bad))
        assert L.nvh_mel_front_check(C.byref(d), C.byref(full)) == native.ERR_ARGUMENT and rows(d, full) == native.ERR_ARGUMENT, bad
    for bad in ({"rows": -1}, {"src_length": -1}, {"channels": 0}, {"channels": 65536}):
        assert rows(make_desc(**dict(SHAPE, **bad)), full) == native.ERR_ARGUMENT, bad
    assert L.nvh_mel_rows_front(None, C.byref(good), C.byref(full), None, fake, valid) == native.ERR_ARGUMENT
    assert L.nvh_mel_rows_front(None, C.byref(good), C.byref(full), fake, fake, (C.c_int64 * 2)(1001, 0)) == native.ERR_ARGUMENT
    # the three conditions of the reflection, each at its limit and one past it; NVH_PAD_ZERO does not look at them
    reflect = make_front(reflect=True)
    for at, past in REFLECT_LIMITS:
        shape = dict(SHAPE, rows=1, src_row_stride=0, **at)
        d_at, d_past = make_desc(**shape), make_desc(**dict(shape, **past))
        one = (C.c_int64 * 1)(0)
        for d, want, want_rows in ((d_at, native.OK, native.ERR_NO_GPU), (d_past, native.ERR_ARGUMENT, native.ERR_ARGUMENT)):
            assert L.nvh_mel_front_check(C.byref(d), C.byref(reflect)) == want, (at, past)
            assert L.nvh_mel_rows_front(None, C.byref(d), C.byref(reflect), fake, fake, one) == want_rows, (at, past)
        assert L.nvh_mel_front_check(C.byref(d_past), C.byref(make_front())) == native.OK
        assert L.nvh_mel_front_check(C.byref(make_desc(**dict(shape, **dict(past, frames=0)))), C.byref(reflect)) == native.OK  # no frame
    # the three existing calls behave as before under a descriptor a reflecting front would refuse
    assert L.nvh_mel_rows(None, C.byref(make_desc(**dict(SHAPE, src_length=1))), fake, fake, (C.c_int64 * 2)(1, 0)) == native.ERR_NO_GPU


def test_python_front_checks():
    from nvorbis_amd import clips, native
    assert clips.mel_front() is None and clips.mel_front("hann", "hz", "constant", False, 0.0, 1.0) is None
    f = clips.mel_front("povey", "mel", "reflect", True, 0.97, 32768.0)
    assert (f.window, f.triangles, f.pad_mode, f.remove_dc) == (native.WIN_POVEY, native.TRI_MEL, native.PAD_REFLECT, 1)
    assert F32(f.preemphasis) == F32(0.97) and f.gain == 32768.0 and tuple(f.reserved) == (0, 0)
    assert C.sizeof(native.MelFront) == 32
    d = native.MelFront()
    assert (d.window, d.triangles, d.pad_mode, d.remove_dc, d.preemphasis, d.gain) == (0, 0, 0, 0, 0.0, 1.0)


def test_decode_clip_features_refuses_bad_front_keywords_before_a_device(ogg_bytes):
    """Every new ValueError of decode_clip_features, on a machine that may have no device at all."""
    import nvorbis_amd as nv
    good = ogg_bytes["3test"]  # 44100 Hz
    bads = [{"window": "hanning"}, {"window": None}, {"window": 0}, {"remove_dc": 1}, {"remove_dc": None}, {"preemphasis": -0.1},
            {"preemphasis": 1.5}, {"preemphasis": float("nan")}, {"preemphasis": "0.97"}, {"preemphasis": True}, {"sample_gain": 0.0},
            {"sample_gain": -1.0}, {"sample_gain": float("inf")}, {"sample_gain": float("nan")}, {"sample_gain": 1e39}, {"sample_gain": None},
            {"pad_mode": "zeros"}, {"pad_mode": None}, {"pad_mode": 1}, {"mel_triangles": "linear"}, {"mel_triangles": None},
            {"frame_count": "win"}, {"frame_count": None}, {"frame_count": 400},
            {"frame_count": "window"},                          # needs center=False
            {"pad_mode": "reflect", "center": False}]           # needs center=True
    for bad in bads:
        with pytest.raises(ValueError):
            nv.decode_clip_features([good], 4000, **bad)
    with pytest.raises(ValueError):  # snip_edges: length < win_length
        nv.decode_clip_features([good], 399, center=False, frame_count="window")
    for length in (0, 1, 200):  # reflect: length < 2; -first = n_fft / 2 - (n_fft - win_length) / 2 = 200 > length - 1
        with pytest.raises(ValueError):
            nv.decode_clip_features([good], length, pad_mode="reflect")
    # (the third condition cannot fail here on its own: centred frames end at most win_length / 2 - 1 behind `length`, which the
    # second condition keeps within length - 2; the C call's test above reaches it)
    with pytest.raises(TypeError):
        nv.decode_clip_features([good], 4000, None, "povey")  # the keywords are keyword-only


def test_kaldi_fbank_keywords():
    import nvorbis_amd as nv
    kw = nv.kaldi_fbank_keywords(16000)
    assert (kw["win_length"], kw["hop"], kw["n_fft"], kw["n_mels"], kw["f_min"], kw["f_max"]) == (400, 160, 512, 80, 20.0, 8000.0)
    assert kw["mel_scale"] == "htk" and kw["mel_triangles"] == "mel" and kw["scale"] == "ln" and kw["floor"] == float(np.finfo(F32).eps)
    assert kw["center"] is False and kw["frame_count"] == "window" and kw["sample_gain"] == 32768.0
    assert kw["preemphasis"] == 0.97 and kw["remove_dc"] is True and kw["window"] == "povey"
    kw = nv.kaldi_fbank_keywords(8000, num_mel_bins=23, high_freq=-200.0, window="hamming", remove_dc=False, preemphasis=0.0)
    assert (kw["win_length"], kw["hop"], kw["n_fft"], kw["n_mels"], kw["f_max"], kw["window"]) == (200, 80, 256, 23, 3800.0, "hamming")
    assert nv.kaldi_fbank_keywords(44100)["n_fft"] == 2048 and nv.kaldi_fbank_keywords(44100)["win_length"] == 1102
    assert nv.kaldi_fbank_keywords(16000, high_freq=7600.0)["f_max"] == 7600.0
    assert nv.kaldi_fbank_keywords(16000, frame_length_ms=2.0, frame_shift_ms=1.0)["n_fft"] == 64  # (32 samples: the smallest transform)
    for bad in ({"frame_length_ms": 0.0}, {"frame_shift_ms": 0.0}, {"frame_length_ms": 500.0}, {"frame_length_ms": float("nan")}):
        with pytest.raises(ValueError):
            nv.kaldi_fbank_keywords(16000, **bad)
    with pytest.raises(ValueError):
        nv.kaldi_fbank_keywords(0)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. how close to Kaldi
# ---------------------------------------------------------------------------------------------------------------------------

def kaldi_fbank64(x, rate, frame_length_ms=25.0, frame_shift_ms=10.0, num_mel_bins=80, low_freq=20.0, high_freq=0.0, preemph=0.97):
    """Kaldi's compute-fbank-feats in float64, written from Kaldi's description of itself (feature-window.cc, mel-computations.cc;
    dither 0, snip_edges, remove_dc_offset, povey window, use_power, no energy): (F, num_mel_bins).  Independent of rule_front: the
    window at the buffer's start, the bank as Kaldi's loop over bins in the mel domain with its own 1127 ln(1 + f / 700), and no
    Nyquist bin."""
    W, H = int(rate * 0.001 * frame_length_ms), int(rate * 0.001 * frame_shift_ms)
    N = 1
    while N < W:
        N *= 2
    wave = np.asarray(x, np.float64) * 32768.0
    F = (wave.size - W) // H + 1
    povey = np.power(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / (W - 1)), 0.85)
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    nyquist = 0.5 * rate
    high = high_freq if high_freq > 0 else nyquist + high_freq
    mel_low, mel_high = mel(low_freq), mel(high)
    delta = (mel_high - mel_low) / (num_mel_bins + 1)
    bank = np.zeros((num_mel_bins, N // 2))
    for b in range(num_mel_bins):
        left, center, right = mel_low + b * delta, mel_low + (b + 1) * delta, mel_low + (b + 2) * delta
        for i in range(N // 2):
            m = mel(rate / N * i)
            if left < m < right:
                bank[b, i] = (m - left) / (center - left) if m <= center else (right - m) / (right - center)
    out = np.zeros((F, num_mel_bins))
    for f in range(F):
        w = wave[f * H:f * H + W].copy()
        w -= w.sum() / W
        for i in range(W - 1, 0, -1):
            w[i] -= preemph * w[i - 1]
        w[0] -= preemph * w[0]
        buf = np.zeros(N)
        buf[:W] = w * povey
        spec = np.fft.rfft(buf)
        power = (spec.real ** 2 + spec.imag ** 2)[:N // 2]
        out[f] = np.log(np.maximum(bank @ power, np.finfo(np.float32).eps))
    return out


def kaldi_signal(rate=16000):
    rng = np.random.default_rng(2024)
    t = np.arange(rate, dtype=np.float64)
    return (0.1 * rng.uniform(-1, 1, rate) + 0.3 * np.sin(2 * np.pi * 440.0 * t / rate)).astype(F32)  # 1 s of noise + tone


def rule_kaldi(x, rate):
    """decode_clip_features(**kaldi_fbank_keywords(rate)) on one row, by the numpy rules and the library's tables: (F, B), the floor."""
    import nvorbis_amd as nv
    kw = nv.kaldi_fbank_keywords(rate)
    N, W, H, B = kw["n_fft"], kw["win_length"], kw["hop"], kw["n_mels"]
    tw, win, fb = front_tables(rate, N, W, B, kw["window"], kw["mel_triangles"], f_min=kw["f_min"], f_max=kw["f_max"])
    F = (x.size - W) // H + 1
    u = rule_front(x, x.size, 0, F, N, W, H, win, remove_dc=kw["remove_dc"], preemphasis=kw["preemphasis"], gain=kw["sample_gain"])
    return rule_scale(rule_mel(rule_power(u, tw), fb), "ln", kw["floor"]), kw["floor"]


KALDI_MEASURED = 1.1e-4  # the measured maximum below (printed), in natural-log units


def test_the_kaldi_keywords_are_close_to_kaldi():
    """rule_front + the rule under kaldi_fbank_keywords(16000) against kaldi_fbank64 on 1 s of noise + a 440 Hz tone, 98 frames of 80
    bands, in the log domain on the bands whose energy is above 1e3 * floor (all of them on this signal).  Measured: max |ln rule -
    ln kaldi| = 1.10e-4 (the f32 arithmetic of the rule against float64 -- an error of a band follows the frame's whole power, and
    the bands far from the tone hold a thousandth of it; the two algorithms are the same function).  The bound is twice that."""
    x = kaldi_signal()
    got, floor = rule_kaldi(x, 16000)
    want = kaldi_fbank64(x, 16000)
    assert got.shape == want.shape == (98, 80)
    loud = want > np.log(1e3 * floor)
    assert loud.mean() > 0.9
    diff = float(np.abs(got.astype(np.float64) - want)[loud].max())
    print("kaldi closeness: max |ln rule - ln kaldi64| = %.3e over %d of %d values" % (diff, int(loud.sum()), loud.size))
    assert diff <= 2 * KALDI_MEASURED, diff


def test_the_kaldi_keywords_against_torchaudio():
    """The same comparison against torchaudio.compliance.kaldi.fbank(dither=0) where torchaudio is installed (f32 there too: the
    bound is that of the float64 comparison plus torchaudio's own f32 distance from Kaldi, taken as the same again)."""
    ta = pytest.importorskip("torchaudio")
    import torch
    x = kaldi_signal()
    got, floor = rule_kaldi(x, 16000)
    want = ta.compliance.kaldi.fbank(torch.from_numpy(x.copy())[None, :] * 32768.0, num_mel_bins=80, dither=0.0, sample_frequency=16000.0,
                                     window_type="povey", energy_floor=0.0).numpy().astype(np.float64)
    assert got.shape == want.shape
    loud = want > np.log(1e3 * floor)
    diff = float(np.abs(got.astype(np.float64) - want)[loud].max())
    print("kaldi closeness: max |ln rule - ln torchaudio| = %.3e" % diff)
    assert diff <= 4 * KALDI_MEASURED, diff


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the routes of tests/test_mel_front.py's cases
# ---------------------------------------------------------------------------------------------------------------------------

def front_route(cfg, triangles):
    """mel_route's `staged` with the sparse bank of the front's triangles: the front adds no LDS, so the sum is mel_route's."""
    D = defines("mel_dev.h")
    rate, N, W, H, B = cfg
    waves, points = D["NVH_MEL_WAVES"], N >> 1
    weights = 0
    for row in front_tables(rate, N, W, B, triangles=triangles)[2]:
        nz = np.nonzero(row)[0]
        weights += int(nz[-1] - nz[0] + 1) if nz.size else 0
    fixed = waves * 2 * (points + ((points >> 6) << 3)) + waves * D["NVH_MEL_OUT_STRIDE"]
    staged = fixed + 2 * (points + (points >> 4) + 1) + 3 * B + weights + W + (waves - 1) * H + W
    return staged * 4 <= D["NVH_MEL_LDS_BYTES"]


@pytest.mark.parametrize("cfg", sorted(GPU_CONFIGS))
def test_route_of_the_gpu_cases(cfg):
    """Every configuration of tests/test_mel_front.py takes the route it is there for, with either kind of triangles, and the front
    moves none of them (nor a case of tests/test_row_routes.py) from the route nvh_mel_rows gives it."""
    from tests.test_row_routes import MEL_ROUTES
    assert mel_route(cfg)[0] == GPU_CONFIGS[cfg]
    for triangles in TRIANGLES:
        assert front_route(cfg, triangles) == GPU_CONFIGS[cfg], triangles
    for other, (staged, _) in MEL_ROUTES.items():
        assert front_route(other, "hz") == staged and front_route(other, "mel") == staged, other

"""Per-row normalisation of features, without a GPU: the rule of include/nvorbis_hip.h (nvh_fnorm_rows) in numpy, how far it is from
float64, its closed forms, and every argument error of nvh_fnorm_check, nvh_fnorm_rows and the keywords of decode_clip_features.

rule_sum64 and rule_fnorm are written from the header's text; tests/test_fnorm_rows.py compares the kernel with them as uint32."""
import ctypes as C

import numpy as np
import pytest

F32 = np.float32
MODES = (None, "mean", "mean_var", "peak")
AXES = ("band", "all")


def make_fdesc(mode=None, axis="band", **kw):
    """A native.FnormDesc: the defaults of decode_clip_features, then whatever field `kw` names."""
    from nvorbis_amd import native
    d = native.FnormDesc(mode={None: 0, "mean": 1, "mean_var": 2, "peak": 3}.get(mode, mode), axis={"band": 0, "all": 1}.get(axis, axis),
                         rows=0, channels=1, frames=0, bands=1, eps=1e-5, pad_value=0.0, range=80.0, offset=40.0, gain=1 / 40)
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------

def rule_sum64(v):
    """sum64 over axis 0 of an f32 array (n, ...): 64 partials, element e into partial e mod 64 in rising order, six halvings."""
    v = np.asarray(v, F32)
    n = v.shape[0]
    k = -(-n // 64)
    padded = np.zeros((k * 64,) + v.shape[1:], F32)
    padded[:n] = v
    padded = padded.reshape((k, 64) + v.shape[1:])
    p = np.zeros((64,) + v.shape[1:], F32)
    for j in range(k):
        p = p + padded[j]
    for d in (32, 16, 8, 4, 2, 1):
        p = p[:d] + p[d:2 * d]
    assert p.dtype == F32
    return p[0]


def _group_sum(g, axis):
    """S1 of the rule over g (n, B): per band, or the bands' results in rising b into one accumulator."""
    s = rule_sum64(g)
    if axis == "band":
        return s
    acc = F32(0)
    for b in range(g.shape[1]):
        acc = F32(acc + s[b])
    return acc


def rule_fnorm(x, vf, mode, axis="band", eps=1e-5, pad_value=0.0, peak_range=80.0, peak_offset=40.0, peak_gain=1 / 40):
    """The rule over x (rows, channels, F, B) f32; vf None or one count per row.  Returns the same shape, f32."""
    x = np.asarray(x, F32)
    rows, chans, F, B = x.shape
    with np.errstate(over="ignore"):
        eps, pad_value, rng, off, gain = (F32(v) for v in (eps, pad_value, peak_range, peak_offset, peak_gain))
    out = np.empty_like(x)
    for i in range(rows):
        n = F if vf is None else int(vf[i])
        assert 0 <= n <= F
        for c in range(chans):
            g, y = x[i, c, :n], out[i, c]
            y[n:] = pad_value
            if n == 0:
                continue
            if mode is None:
                y[:n] = g
            elif mode == "peak":
                with np.errstate(invalid="ignore"):
                    t = F32(g.max() - rng)
                    y[:n] = (np.maximum(g, t) + off) * gain
            else:
                nn = F32(n if axis == "band" else n * B)
                mean = _group_sum(g, axis) / nn
                d = g - mean
                if mode == "mean":
                    y[:n] = d
                else:
                    var = _group_sum(d * d, axis) / nn
                    y[:n] = d / np.sqrt(var + eps)
    assert out.dtype == F32
    return out


def float64_fnorm(x, vf, mode, axis="band", eps=1e-5, pad_value=0.0, peak_range=80.0, peak_offset=40.0, peak_gain=1 / 40):
    """The same formulas in float64 (the parameters as the f32 values the rule uses)."""
    x = np.asarray(x, np.float64)
    eps, rng, off, gain = (float(F32(v)) for v in (eps, peak_range, peak_offset, peak_gain))
    out = np.full(x.shape, float(F32(pad_value)))
    for i in range(x.shape[0]):
        n = x.shape[2] if vf is None else int(vf[i])
        for c in range(x.shape[1]):
            g = x[i, c, :n]
            if n == 0:
                continue
            if mode is None:
                out[i, c, :n] = g
            elif mode == "peak":
                out[i, c, :n] = (np.maximum(g, g.max() - rng) + off) * gain
            else:
                ax = 0 if axis == "band" else None
                d = g - g.mean(axis=ax)
                out[i, c, :n] = d if mode == "mean" else d / np.sqrt((d * d).mean(axis=ax) + eps)
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def normal_features(seed, shape):
    """N(-8, 4): mean -8, variance 4, the spread of natural-log mel features of speech."""
    return np.random.default_rng(seed).normal(-8.0, 2.0, shape).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the summation's bound, and the rule against float64
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 1001])
def test_sum64_is_within_its_bound_of_the_float64_sum(n):
    """A partial is a chain of ceil(n / 64) additions and the halvings put six more on the path of every element, each addition
    within 2^-24 of its result (relatively), and every intermediate result is at most sum |v| (1 + small): the error is at most
    (ceil(n / 64) + 6) * 2^-24 * sum |v|, to first order.  Measured here on N(-8, 4) data, 16 columns per n: at most 0.21 of the
    bound (n = 1: exact)."""
    v = normal_features(n, (n, 16))
    got = rule_sum64(v).astype(np.float64)
    exact = v.astype(np.float64).sum(axis=0)
    bound = (-(-n // 64) + 6) * 2.0 ** -24 * np.abs(v.astype(np.float64)).sum(axis=0)
    print("sum64 n=%d: worst %.3f of the bound" % (n, float((np.abs(got - exact) / bound).max())))
    assert (np.abs(got - exact) <= bound).all()
    # the structure itself: partial l holds the elements l, l + 64, ..; pairs (l, l + 32) first
    if n == 130:
        col = v[:, 0]
        p = [F32(0)] * 64
        for e in range(n):
            p[e % 64] = F32(p[e % 64] + col[e])
        for d in (32, 16, 8, 4, 2, 1):
            for l in range(d):
                p[l] = F32(p[l] + p[l + d])
        assert bits(p[0]) == bits(rule_sum64(col))


# what test_rule_is_close_to_float64 measured (the maximum over its shapes): the assertion allows twice that, because the data is
# random but seeded
MEASURED = {("mean", "band"): 1.63e-06, ("mean", "all"): 1.33e-06, ("mean_var", "band"): 8.06e-07, ("mean_var", "all"): 1.02e-06,
            ("peak", "band"): 7.37e-08, (None, "band"): 0.0}


@pytest.mark.parametrize("mode,axis", sorted(MEASURED, key=str))
def test_rule_is_close_to_float64(mode, axis):
    """Every mode against the same formulas in float64 on N(-8, 4) data: rows of (F, B) = (1001, 8), (3000, 4) and (65, 80), two
    channels, vf = F, F // 2 + 1, 1 and 0.  Measured maximum absolute deviations (MEASURED above): mean 1.63e-6 per band and
    1.33e-6 over all (values of a few units, the mean itself within its sum's bound); mean_var 8.06e-7 and 1.02e-6 (values of unit
    variance; vf = 1 gives d = 0 exactly); peak 7.37e-8 (values around 0.8, three roundings); None: exact.  The assertion is twice the measured
    figure."""
    worst = 0.0
    for k, (F, B) in enumerate(((1001, 8), (3000, 4), (65, 80))):
        x = normal_features(100 + k, (4, 2, F, B))
        vf = [F, F // 2 + 1, 1, 0]
        got = rule_fnorm(x, vf, mode, axis, pad_value=-3.0).astype(np.float64)
        want = float64_fnorm(x, vf, mode, axis, pad_value=-3.0)
        worst = max(worst, float(np.abs(got - want).max()))
    print("fnorm %s/%s: max |rule - float64| = %.3g" % (mode, axis, worst))
    assert worst <= 2 * MEASURED[(mode, axis)]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. closed forms
# ---------------------------------------------------------------------------------------------------------------------------

def test_closed_forms():
    """A constant row (-8: every partial sum is a multiple of 8 below 2^24 * 8, so the sums are exact and the mean is the constant):
    `mean` gives +0 everywhere, `mean_var` 0 everywhere (d = +0, var = 0, sd = sqrt(eps)); `peak` with range 0 gives fl(fl(mx +
    offset) * gain) everywhere; vf = 0 gives pad_value everywhere; None copies the counted frames; frames behind vf are pad_value
    in every mode."""
    F, B = 130, 5
    const = np.full((1, 2, F, B), -8.0, F32)
    for axis in AXES:
        for vf in (None, [F], [77], [1]):
            n = F if vf is None else vf[0]
            assert not bits(rule_fnorm(const, vf, "mean", axis, pad_value=0.0)).any()  # +0, not -0
            got = rule_fnorm(const, vf, "mean_var", axis, pad_value=1.5)
            assert not bits(got[:, :, :n]).any() and (got[:, :, n:] == 1.5).all()
    x = normal_features(7, (3, 2, F, B))
    x[1, 0, 40, 2] = 55.0
    got = rule_fnorm(x, None, "peak", peak_range=0.0, peak_offset=4.0, peak_gain=0.25)
    for i in range(3):
        for c in range(2):
            want = F32(F32(x[i, c].max() + F32(4.0)) * F32(0.25))
            assert (bits(got[i, c]) == bits(want)).all()
    assert got[1, 0, 0, 0] == F32(59.0 * 0.25)
    inf = rule_fnorm(x, None, "peak", peak_range=float("inf"), peak_offset=4.0, peak_gain=0.25)  # no clamp at all
    assert (bits(inf) == bits((x + F32(4.0)) * F32(0.25))).all()
    for mode in MODES:
        for axis in AXES:
            got = rule_fnorm(x, [0, 0, 0], mode, axis, pad_value=-2.25)
            assert (bits(got) == bits(F32(-2.25))).all()
            got = rule_fnorm(x, [F, 31, 64], mode, axis, pad_value=-2.25)
            assert (got[1, :, 31:] == F32(-2.25)).all() and (got[2, :, 64:] == F32(-2.25)).all() and (got[0] != F32(-2.25)).all()
            if mode is None:
                assert (bits(got[1, :, :31]) == bits(x[1, :, :31])).all() and (bits(got[0]) == bits(x[0])).all()
    # a group's values depend on its counted frames only
    a = rule_fnorm(x, [50, 50, 50], "mean_var", "all")
    y = x.copy()
    y[:, :, 50:] = 1e6
    assert (bits(a) == bits(rule_fnorm(y, [50, 50, 50], "mean_var", "all"))).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. argument errors, each before NVH_ERR_NO_GPU
# ---------------------------------------------------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")
# every field just outside its limit (the descriptor otherwise make_fdesc's, with a shape)
BAD_FIELDS = [{"mode": -1}, {"mode": 4}, {"axis": -1}, {"axis": 2}, {"mode": 3, "axis": 2}, {"rows": -1}, {"channels": 0},
              {"channels": 65536}, {"frames": -1}, {"frames": (1 << 24) + 1}, {"bands": 0}, {"bands": 257}, {"pad_value": NAN},
              {"pad_value": INF}, {"pad_value": -INF}, {"mode": 2, "eps": 0.0}, {"mode": 2, "eps": 1e-39}, {"mode": 2, "eps": -1e-5},
              {"mode": 2, "eps": NAN}, {"mode": 2, "eps": INF}, {"mode": 3, "range": -1.0}, {"mode": 3, "range": NAN},
              {"mode": 3, "offset": INF}, {"mode": 3, "offset": NAN}, {"mode": 3, "gain": -INF}, {"mode": 3, "gain": NAN}]
SHAPE = dict(rows=2, channels=1, frames=5, bands=80, src_row_stride=400, src_chan_stride=400, src_frame_stride=80, src_band_stride=1,
             dst_row_stride=400, dst_chan_stride=400, dst_frame_stride=80, dst_band_stride=1)


def test_check_refuses_every_number_outside_the_rule():
    from nvorbis_amd import native
    L = native.lib()
    assert L.nvh_fnorm_check(None) == native.ERR_ARGUMENT
    for bad in BAD_FIELDS:
        assert L.nvh_fnorm_check(C.byref(make_fdesc(**dict(SHAPE, **bad)))) == native.ERR_ARGUMENT, bad
    for mode in (0, 1, 2, 3):
        for axis in (0, 1):
            assert L.nvh_fnorm_check(C.byref(make_fdesc(mode, axis, **SHAPE))) == native.OK
    # the limits themselves, and the numbers a mode does not use
    for good in ({"frames": 1 << 24}, {"frames": 0}, {"bands": 256}, {"channels": 65535}, {"rows": 0}, {"mode": 2, "eps": 2.0 ** -126},
                 {"mode": 3, "range": INF}, {"mode": 3, "range": 0.0}, {"mode": 1, "eps": 0.0}, {"mode": 0, "range": -1.0, "gain": NAN},
                 {"mode": 3, "eps": 0.0}):
        assert L.nvh_fnorm_check(C.byref(make_fdesc(**dict(SHAPE, **good)))) == native.OK, good


def test_rows_entry_point_checks_its_arguments_before_a_device():
    """nvh_fnorm_rows without a context: every argument error comes first, then NVH_ERR_NO_GPU."""
    from nvorbis_amd import native
    L = native.lib()
    fake = C.c_void_p(4096)  # never dereferenced: there is no context

    def call(d, vf=(5, 0), src=fake, dst=fake):
        v = None if vf is None else (C.c_int64 * len(vf))(*vf)
        return L.nvh_fnorm_rows(None, None if d is None else C.byref(d), src, dst, v)
    assert call(None) == native.ERR_ARGUMENT
    for bad in BAD_FIELDS:
        assert call(make_fdesc(**dict(SHAPE, **bad))) == native.ERR_ARGUMENT, bad
    good = make_fdesc("mean_var", "all", **SHAPE)
    assert call(good, src=None) == native.ERR_ARGUMENT and call(good, dst=None) == native.ERR_ARGUMENT
    assert call(good, vf=(6, 0)) == native.ERR_ARGUMENT and call(good, vf=(5, -1)) == native.ERR_ARGUMENT
    assert call(good) == native.ERR_NO_GPU and call(good, vf=None) == native.ERR_NO_GPU and call(good, dst=fake, src=fake, vf=(0, 5)) == native.ERR_NO_GPU
    assert call(make_fdesc(**dict(SHAPE, rows=0)), vf=None, src=None, dst=None) == native.ERR_NO_GPU  # (nothing to do, but no context either)
    assert call(make_fdesc(**dict(SHAPE, frames=0)), vf=(0, 0), src=None, dst=None) == native.ERR_NO_GPU
    assert call(make_fdesc(**dict(SHAPE, frames=0)), vf=(1, 0), src=None, dst=None) == native.ERR_ARGUMENT


def test_fnorm_desc_in_python():
    from nvorbis_amd import clips, native
    d = clips.fnorm_desc("mean_var", "all", 1e-3, -1.0, frames=7, bands=80)
    assert (d.mode, d.axis, d.frames, d.bands, d.rows, d.channels) == (native.FNORM_MEAN_VAR, native.FNORM_ALL, 7, 80, 0, 0)
    assert F32(d.eps) == F32(1e-3) and d.pad_value == -1.0
    d = clips.fnorm_desc("peak")
    assert (d.mode, d.axis) == (native.FNORM_PEAK, native.FNORM_PER_BAND) and (d.range, d.offset) == (80.0, 40.0) and F32(d.gain) == F32(1 / 40)
    assert clips.fnorm_desc().mode == native.FNORM_NONE and clips.fnorm_desc(peak_range=INF).range == INF
    for bad in BAD_KEYWORDS + [{"frames": -1}, {"frames": (1 << 24) + 1}, {"bands": 0}, {"bands": 257}, {"bands": 80.0}]:
        if "mask_padding" in bad:
            continue
        with pytest.raises(ValueError):
            clips.fnorm_desc(**bad)


BAD_KEYWORDS = [{"normalize": "cmvn"}, {"normalize": 1}, {"normalize": False}, {"normalize_axis": None}, {"normalize_axis": "frame"},
                {"normalize_axis": 0}, {"norm_eps": 0.0}, {"norm_eps": -1e-5}, {"norm_eps": 1e-39}, {"norm_eps": INF}, {"norm_eps": NAN},
                {"norm_eps": "1e-5"}, {"norm_eps": True}, {"pad_value": NAN}, {"pad_value": INF}, {"pad_value": 1e39}, {"pad_value": None},
                {"pad_value": "0"}, {"peak_range": -1.0}, {"peak_range": NAN}, {"peak_range": None}, {"peak_offset": INF},
                {"peak_offset": NAN}, {"peak_offset": "40"}, {"peak_gain": INF}, {"peak_gain": NAN}, {"peak_gain": 1e39},
                {"peak_gain": None}, {"mask_padding": 1}, {"mask_padding": None}, {"mask_padding": "yes"}]


def test_decode_clip_features_refuses_bad_normalisation_keywords_before_a_device(ogg_bytes):
    """Every ValueError of the normalisation keywords, whatever `normalize` is, on a machine that may have no device at all."""
    import nvorbis_amd as nv
    good = ogg_bytes["3test"]
    for bad in BAD_KEYWORDS:
        for base in ({}, {"normalize": "mean_var"}, {"normalize": "peak"}):
            with pytest.raises(ValueError):
                nv.decode_clip_features([good], 4000, **dict(base, **bad))
    with pytest.raises(TypeError):
        nv.decode_clip_features([good], 4000, None, normalize="mean", norm_epsilon=1e-5)

"""The row resampler's host side (nvh_resample_plan, nvh_resample_taps; include/nvorbis_hip.h states the rule): the plan's
numbers, the tap table against the formula evaluated in numpy double, the filter's response computed from the library's own taps,
and decode_clip_rows' sample_rate checks.  No device anywhere."""
import ctypes as C
import math

import numpy as np
import pytest

PAIRS = [(44100, 16000), (48000, 16000), (44100, 48000), (44100, 22050), (8000, 44100), (44100, 8000), (22050, 16000)]


def rule_plan(fi, fo):
    g = math.gcd(fi, fo)
    L, M = fo // g, fi // g
    half = 16 if L >= M else (16 * M + L - 1) // L
    return L, M, half, L * 2 * half


def lib_plan(fi, fo):
    from nvorbis_amd import native
    up, down, half, count = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    rc = native.lib().nvh_resample_plan(fi, fo, C.byref(up), C.byref(down), C.byref(half), C.byref(count))
    return rc, (up.value, down.value, half.value, count.value)


_TAPS = {}


def lib_taps(fi, fo):
    """The library's table as (L, 2 * half) float32, read-only, fetched once per pair."""
    from nvorbis_amd import native
    if (fi, fo) not in _TAPS:
        L, M, half, n = rule_plan(fi, fo)
        h = np.zeros(n, np.float32)
        count = C.c_int64(0)
        assert native.lib().nvh_resample_taps(fi, fo, h.ctypes.data, n, C.byref(count)) == native.OK and count.value == n
        h = h.reshape(L, 2 * half)
        h.setflags(write=False)
        _TAPS[(fi, fo)] = h
    return _TAPS[(fi, fo)]


def formula_taps(fi, fo):
    """The rule in numpy double (np.sinc, np.i0), not yet rounded."""
    L, M, half, _ = rule_plan(fi, fo)
    W = 16.0 * max(1.0, M / L)
    sc = 0.94 * min(1.0, L / M)
    k = np.arange(2 * half, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    t = (k - half + 1) - p / L
    u = t / W
    inside = np.abs(u) < 1
    win = np.i0(9.0 * np.sqrt(np.where(inside, 1 - u * u, 0.0))) / np.i0(9.0)
    return np.where(inside, sc * np.sinc(sc * t) * win, 0.0)


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_plan_is_the_rules(fi, fo):
    from nvorbis_amd import native
    rc, got = lib_plan(fi, fo)
    assert rc == native.OK and got == rule_plan(fi, fo), (got, rule_plan(fi, fo))


def test_plan_refuses_what_the_rule_refuses():
    from nvorbis_amd import native
    L = native.lib()
    assert lib_plan(1, 4096)[0] == native.OK and lib_plan(1, 4096)[1] == (4096, 1, 16, 4096 * 32)  # L = 4096: the last one taken
    assert lib_plan(1, 4097)[0] == native.ERR_UNSUPPORTED  # L > 4096
    assert lib_plan(44100, 44101)[0] == native.ERR_UNSUPPORTED
    # L * 2 * half: (8192, 1) has half = 131072, 262144 taps -- the last one taken; (8193, 1) one phase too long
    assert lib_plan(8192, 1) == (native.OK, (1, 8192, 131072, 262144))
    assert lib_plan(8193, 1)[0] == native.ERR_UNSUPPORTED
    assert lib_plan(8191, 4096) == (native.OK, (4096, 8191, 32, 262144))
    assert lib_plan(8193, 4096)[0] == native.ERR_UNSUPPORTED  # L = 4096, half = 33: 4096 * 66 taps
    for fi, fo in ((0, 16000), (16000, 0), (-1, 16000), (16000, -5)):
        assert lib_plan(fi, fo)[0] == native.ERR_ARGUMENT, (fi, fo)
    a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    ptrs = [C.byref(a), C.byref(b), C.byref(c), C.byref(d)]
    for k in range(4):
        args = list(ptrs)
        args[k] = None
        assert L.nvh_resample_plan(44100, 16000, *args) == native.ERR_ARGUMENT, k
    # the table: *count is set even when cap is too small
    count = C.c_int64(-1)
    assert L.nvh_resample_taps(44100, 16000, None, 0, C.byref(count)) == native.ERR_ARGUMENT and count.value == 160 * 90
    small = np.zeros(8, np.float32)
    count = C.c_int64(-1)
    assert L.nvh_resample_taps(44100, 16000, small.ctypes.data, 8, C.byref(count)) == native.ERR_ARGUMENT and count.value == 160 * 90
    assert not small.any()
    assert L.nvh_resample_taps(44100, 16000, small.ctypes.data, 8, None) == native.ERR_ARGUMENT
    assert L.nvh_resample_taps(0, 16000, small.ctypes.data, 8, C.byref(count)) == native.ERR_ARGUMENT
    assert L.nvh_resample_taps(1, 4097, small.ctypes.data, 8, C.byref(count)) == native.ERR_UNSUPPORTED


def test_rows_entry_point_checks_its_arguments_before_a_device():
    """nvh_resample_rows without a context: every argument error comes first, then the limits, then NVH_ERR_NO_GPU."""
    from nvorbis_amd import native
    L = native.lib()

    def desc(**kw):
        d = native.ResampleDesc(in_rate=44100, out_rate=16000, rows=1, channels=1, format=native.PCM_F32, length=8, src_length=64,
                                src_row_stride=64, src_time_stride=1, src_chan_stride=0, dst_row_stride=8, dst_time_stride=1,
                                dst_chan_stride=0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    one = lambda v: (C.c_int64 * 1)(v)
    row = (C.c_int32 * 1)(0)
    fake = C.c_void_p(4096)  # never dereferenced: there is no context

    def call(d, origin=0, start=0, valid=8, dst_row=0, src=fake, dst=fake):
        row[0] = dst_row
        return L.nvh_resample_rows(None, C.byref(d) if d is not None else None, src, dst, one(origin), one(start), one(valid), row, None)
    assert call(None) == native.ERR_ARGUMENT
    for bad in ({"in_rate": 0}, {"out_rate": -1}, {"rows": -1}, {"length": -1}, {"src_length": -1}, {"channels": 0}, {"format": 7}):
        assert call(desc(**bad)) == native.ERR_ARGUMENT, bad
    assert call(desc(), src=None) == native.ERR_ARGUMENT and call(desc(), dst=None) == native.ERR_ARGUMENT
    assert call(desc(), origin=-1) == native.ERR_ARGUMENT and call(desc(), start=-1) == native.ERR_ARGUMENT
    assert call(desc(), valid=9) == native.ERR_ARGUMENT and call(desc(), valid=-1) == native.ERR_ARGUMENT
    assert call(desc(), dst_row=-1) == native.ERR_ARGUMENT and call(desc(), start=1 << 48) == native.ERR_ARGUMENT
    assert L.nvh_resample_rows(None, C.byref(desc()), fake, fake, None, one(0), one(8), None, None) == native.ERR_ARGUMENT
    assert call(desc(out_rate=44101)) == native.ERR_UNSUPPORTED
    assert call(desc()) == native.ERR_NO_GPU and call(desc(), start=1 << 33, origin=(1 << 33) * 2) == native.ERR_NO_GPU
    assert call(desc(rows=0)) == native.ERR_NO_GPU  # (nothing to do, but no context either)


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_taps_are_the_formula_rounded_once(fi, fo):
    """Every tap within one f32 ulp of np.float32(formula in double): the double evaluations (the library's series and libm, numpy's
    np.i0 and np.sinc) agree to about 1e-14, so only the final rounding can land on the other side of a tie."""
    got = lib_taps(fi, fo)
    want = formula_taps(fi, fo).astype(np.float32)
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= np.spacing(np.abs(want)).astype(np.float64)).all(), float(err.max())
    assert (got[np.abs(formula_taps(fi, fo)) == 0] == 0).all()


def response_db(h, L, half, f):
    """Per phase, the magnitude of sum_k h[p][k] exp(-2 pi i f t) at frequency f in cycles per SOURCE sample, in double."""
    k = np.arange(2 * half, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    t = (k - half + 1) - p / L
    return np.abs((h.astype(np.float64) * np.exp(-2j * np.pi * f * t)).sum(axis=1))


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_filter_response_from_the_librarys_taps(fi, fo):
    L, M, half, _ = rule_plan(fi, fo)
    h = lib_taps(fi, fo)
    dc = h.astype(np.float64).sum(axis=1)
    assert (np.abs(dc - 1) <= 2e-5).all(), float(np.abs(dc - 1).max())
    nyq = 0.5 * min(1.0, L / M)  # the lower Nyquist, in cycles per source sample
    passband = 20 * np.log10(response_db(h, L, half, 0.8 * nyq))
    assert (passband >= -0.1).all() and (passband <= 0.1).all(), (float(passband.min()), float(passband.max()))
    if L < M:
        for mult in (1.12, 1.25, 1.5):
            stop = 20 * np.log10(np.maximum(response_db(h, L, half, mult * nyq), 1e-300))
            assert (stop <= -90.0).all(), (mult, float(stop.max()))


def test_decode_clip_rows_refuses_bad_sample_rates_before_a_device(ogg_bytes):
    import nvorbis_amd as nv
    good = ogg_bytes["3test"]  # 44100 Hz
    for bad in (0, -16000, 16000.0, True, "16000", 44101, 1, 4097 * 44100):
        with pytest.raises(ValueError):
            nv.decode_clip_rows([good], 16, sample_rate=bad)
    with pytest.raises(ValueError):
        nv.decode_clip_rows([good], 0, sample_rate=0)  # ... also where there is nothing to decode
    rows, valid = nv.decode_clip_rows([good, good], 0, sample_rate=16000)  # no samples asked for: no device needed
    assert rows.shape == (2, 0, 2) and np.array_equal(valid, [0, 0]) and valid.dtype == np.int64

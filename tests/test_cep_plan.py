"""Cepstra and deltas of features, without a GPU: the rule of include/nvorbis_hip.h (nvh_cep_rows) in numpy, its tables against
nvh_cep_tables bit for bit, its closed forms, how far it is from float64 (bounds that are derived, not measured), Kaldi's
algorithm restated in float64, and every argument error of nvh_cep_check, nvh_cep_rows, cep_desc and the keywords of
decode_clip_features.

rule_tables and rule_cep are written from the header's text; tests/test_cep_rows.py compares the kernel with them as uint32."""
import ctypes as C
import math

import numpy as np
import pytest

F32 = np.float32
NORMS = ("ortho", None)


def make_cdesc(**kw):
    """A native.CepDesc: 23 bands -> 13 cepstra, ortho, no lifter, order 2 over N = 2, one channel; then whatever field `kw` names."""
    from nvorbis_amd import native
    d = native.CepDesc(transform=1, dct_norm=0, order=2, window=2, rows=0, channels=1, frames=0, bands=23, ceps=13, lifter=0.0)
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------

def table64(B, K, norm, lifter):
    """D[k][b] in double, the header's order of operations."""
    Lf = float(F32(lifter))
    D = np.empty((K, B), np.float64)
    for k in range(K):
        w = 2.0 if norm is None else (math.sqrt(1.0 / B) if k == 0 else math.sqrt(2.0 / B))
        lift = 1.0 + (0.5 * Lf) * math.sin((math.pi * k) / Lf) if Lf > 0 else 1.0
        wl = w * lift
        for b in range(B):
            D[k, b] = wl * math.cos(((math.pi * (b + 0.5)) * k) / B)
    return D


def scales64(N):
    """(s_1[-N .. N], s_2[-2N .. 2N]) in double: one division of integers each."""
    d = 2 * sum(i * i for i in range(1, N + 1))
    s1 = np.asarray([j / d for j in range(-N, N + 1)], np.float64)
    s2 = np.asarray([sum(i * (j - i) for i in range(-N, N + 1) if abs(j - i) <= N) / (d * d) for j in range(-2 * N, 2 * N + 1)], np.float64)
    return s1, s2


def rule_tables(B, K, norm, lifter, N):
    """(D (K, B) or None for K None, s_1, s_2), every value rounded once to f32."""
    s1, s2 = scales64(N)
    return (None if K is None else table64(B, K, norm, lifter).astype(F32)), s1.astype(F32), s2.astype(F32)


def rule_cepstra(x, D):
    """c[.., f, k]: one accumulator from +0, b rising, product and sum rounded separately."""
    x = np.asarray(x, F32)
    if D is None:
        return x
    acc = np.zeros(x.shape[:-1] + (D.shape[0],), F32)
    for b in range(x.shape[-1]):
        acc = acc + x[..., b, None] * D[:, b]
    assert acc.dtype == F32
    return acc


def rule_deltas(c, n, s, reach):
    """Order m's columns of one (row, channel): c (F, K) f32, n counted frames, s = s_m[-reach .. reach]."""
    out = np.zeros(c.shape, F32)
    if n > 0:
        acc = np.zeros((n, c.shape[1]), F32)
        f = np.arange(n)
        for j in range(-reach, reach + 1):
            if s[j + reach] != 0:
                acc = acc + c[np.clip(f + j, 0, n - 1)] * s[j + reach]
        assert acc.dtype == F32
        out[:n] = acc
    return out


def rule_cep(x, vf, tables, order, N):
    """The rule over x (rows, channels, F, B) f32; vf None or one count per row; tables from rule_tables (or the library's).
    Returns (rows, channels, F, (1 + order) * K) f32."""
    D, s1, s2 = tables
    x = np.asarray(x, F32)
    c = rule_cepstra(x, D)
    parts = [c]
    for m, s in ((1, s1), (2, s2))[:order]:
        d = np.zeros(c.shape, F32)
        for i in range(x.shape[0]):
            n = x.shape[2] if vf is None else int(vf[i])
            assert 0 <= n <= x.shape[2]
            for ch in range(x.shape[1]):
                d[i, ch] = rule_deltas(c[i, ch], n, s, m * N)
        parts.append(d)
    out = np.concatenate(parts, axis=-1)
    assert out.dtype == F32
    return out


def lib_tables(B, K, norm, lifter, N):
    """The same three from nvh_cep_tables."""
    from nvorbis_amd import clips
    return clips.cep_tables(B, K, "ortho" if norm == "ortho" else None, lifter, N)


def normal_features(seed, shape):
    """N(-8, 4): the spread of natural-log mel features of speech."""
    return np.random.default_rng(seed).normal(-8.0, 2.0, shape).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the tables
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("lifter", [0.0, 22.0])
@pytest.mark.parametrize("N", [1, 2, 8])
def test_tables_equal_the_formulas_bit_for_bit(norm, lifter, N):
    for B, K in ((23, 13), (80, 80), (1, 1), (256, 85)):
        want = rule_tables(B, K, norm, lifter, N)
        got = lib_tables(B, K, norm, lifter, N)
        for w, g, name in zip(want, got, ("D", "s1", "s2")):
            assert g.dtype == F32 and g.shape == w.shape and (bits(g) == bits(w)).all(), (name, B, K)
    none = lib_tables(40, None, norm, lifter, N)
    assert none[0] is None and (bits(none[1]) == bits(rule_tables(40, None, norm, lifter, N)[1])).all()


def test_tables_are_what_they_claim():
    """The scales: s_1 = j / (2 sum i^2), s_2 the convolution of s_1 with itself (numpy's, to a few ulp of double), both
    antisymmetric / symmetric, N = 2 the familiar (-2, -1, 0, 1, 2) / 10.  The ortho table is orthonormal; the plain one is
    torchaudio's create_dct(norm=None) = 2 cos; lifter 22 is Kaldi's 1 + 11 sin(pi k / 22) on top."""
    for N in range(1, 9):
        s1, s2 = scales64(N)
        assert np.allclose(s2, np.convolve(s1, s1), rtol=1e-13, atol=1e-18) and s1[N] == 0 and (s1 == -s1[::-1]).all() and (s2 == s2[::-1]).all()
    assert (scales64(2)[0] == np.asarray([-2, -1, 0, 1, 2]) / 10).all()
    assert np.allclose(scales64(2)[1] * 100, [4, 4, 1, -4, -10, -4, 1, 4, 4], rtol=1e-15, atol=0)
    assert (rule_tables(5, None, None, 0, 1)[2] == F32([0.25, 0, -0.5, 0, 0.25])).all()  # zeros that the rule skips
    D = table64(40, 40, "ortho", 0.0)
    assert np.abs(D @ D.T - np.eye(40)).max() < 1e-14
    b = np.arange(40)
    assert np.allclose(table64(40, 13, None, 0.0), 2 * np.cos(np.pi * (b[None, :] + 0.5) * np.arange(13)[:, None] / 40), atol=1e-14)
    lift = 1 + 11 * np.sin(np.pi * np.arange(13) / 22)
    assert np.allclose(table64(40, 13, "ortho", 22.0), D[:13] * lift[:, None], rtol=1e-14, atol=1e-16)


def test_plan_and_caps():
    from nvorbis_amd import native
    L = native.lib()
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert L.nvh_cep_plan(C.byref(make_cdesc(window=3)), C.byref(a), C.byref(b)) == native.OK and (a.value, b.value) == (13 * 23, 20)
    assert L.nvh_cep_plan(C.byref(make_cdesc(transform=0, ceps=23)), C.byref(a), C.byref(b)) == native.OK and (a.value, b.value) == (0, 14)
    assert L.nvh_cep_plan(C.byref(make_cdesc()), None, C.byref(b)) == native.ERR_ARGUMENT
    assert L.nvh_cep_plan(None, C.byref(a), C.byref(b)) == native.ERR_ARGUMENT
    assert L.nvh_cep_plan(C.byref(make_cdesc(window=9)), C.byref(a), C.byref(b)) == native.ERR_ARGUMENT
    # a cap too small: the counts are set, the call fails, nothing is written
    d = make_cdesc()
    dct, sc = np.full(13 * 23, 7.0, F32), np.full(14, 7.0, F32)
    a.value = b.value = -1
    assert L.nvh_cep_tables(C.byref(d), dct.ctypes.data, sc.ctypes.data, 13 * 23 - 1, 14, C.byref(a), C.byref(b)) == native.ERR_ARGUMENT
    assert (a.value, b.value) == (13 * 23, 14) and (dct == 7.0).all() and (sc == 7.0).all()
    assert L.nvh_cep_tables(C.byref(d), dct.ctypes.data, sc.ctypes.data, 13 * 23, 13, C.byref(a), C.byref(b)) == native.ERR_ARGUMENT
    assert L.nvh_cep_tables(C.byref(d), None, sc.ctypes.data, 0, 14, C.byref(a), C.byref(b)) == native.OK and (dct == 7.0).all() and sc[0] == F32(-0.2)
    assert L.nvh_cep_tables(C.byref(d), None, None, 5, 0, C.byref(a), C.byref(b)) == native.ERR_ARGUMENT
    assert L.nvh_cep_tables(C.byref(d), dct.ctypes.data, None, -1, 0, C.byref(a), C.byref(b)) == native.ERR_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------------
# 2. closed forms
# ---------------------------------------------------------------------------------------------------------------------------

def cep_bound(x, D64):
    """|c - the float64 sum with the double table| <= (B + 3) 2^-24 sum_b |x[b]| |D64[k][b]|: the recursive-summation bound (B - 1
    additions on the path of the first product, fewer on the others) plus one rounding for the product and one for the table,
    to first order, with two to spare for the second-order terms."""
    return (x.shape[-1] + 3) * 2.0 ** -24 * (np.abs(x.astype(np.float64)) @ np.abs(D64).T)


def test_closed_forms():
    # a constant frame under ortho: c[0] is the chain of B equal products v * fl32(sqrt(1 / B)) -- sqrt(B) v -- and c[k > 0] is 0
    for B, K, v in ((23, 13, -8.0), (80, 80, 3.25), (256, 20, -11.5)):
        D, s1, s2 = rule_tables(B, K, "ortho", 0.0, 2)
        x = np.full((1, 1, 5, B), v, F32)
        y = rule_cep(x, None, (D, s1, s2), 2, 2)
        acc, p = F32(0), F32(F32(v) * D[0, 0])
        assert (D[0] == D[0, 0]).all()
        for _ in range(B):
            acc = F32(acc + p)
        assert (bits(y[..., 0]) == bits(acc)).all()
        bound = cep_bound(x[0, 0, :1], table64(B, K, "ortho", 0.0))[0]
        assert abs(float(acc) - math.sqrt(B) * v) <= bound[0] and (np.abs(y[0, 0, 0, 1:K].astype(np.float64)) <= bound[1:]).all()
        # ... and a constant row's deltas are within the delta bound of 0 (the scales of either order sum to 0)
        for m, s in ((1, s1), (2, s2)):
            lim = (2 * 2 * 2 + 3) * 2.0 ** -24 * np.abs(y[0, 0, 0, :K].astype(np.float64)) * np.abs(s.astype(np.float64)).sum()
            assert (np.abs(y[0, 0, :, m * K:(m + 1) * K].astype(np.float64)) <= lim).all()
    # a linear ramp over the frames, no transform: the first delta is the slope in the interior -- exactly for N = 1 (scales of
    # +-1/2, every product exact), within the delta bound for N = 2; the delta-delta of a ramp is within the bound of 0
    F, B = 40, 6
    slope = F32([0.5, -2.0, 0.25, 1.0, 4.0, -0.125])
    ramp = (np.arange(F, dtype=F32)[:, None] * slope[None, :] + F32(3.0))[None, None]
    for N in (1, 2):
        t = rule_tables(B, None, None, 0.0, N)
        y = rule_cep(ramp, None, t, 2, N)
        d1, d2 = y[0, 0, :, B:2 * B], y[0, 0, :, 2 * B:]
        s1, s2 = scales64(N)
        b1 = (2 * 1 * N + 3) * 2.0 ** -24 * np.abs(ramp[0, 0]).max(axis=0) * np.abs(s1).sum()
        b2 = (2 * 2 * N + 3) * 2.0 ** -24 * np.abs(ramp[0, 0]).max(axis=0) * np.abs(s2).sum()
        if N == 1:
            assert (bits(d1[N:F - N]) == bits(np.broadcast_to(slope, (F - 2 * N, B)))).all()
        assert (np.abs(d1[N:F - N].astype(np.float64) - slope) <= b1).all()
        assert (np.abs(d2[2 * N:F - 2 * N].astype(np.float64)) <= b2).all()
        assert (np.abs(d1[0] - slope) > b1).any()  # (the first frame's delta sees repeated frames: it is not the slope)
    # F = 1: every delta is the chain over the one frame clamped
    x = normal_features(3, (2, 2, 1, 23))
    for N in (1, 2, 8):
        t = rule_tables(23, 13, "ortho", 22.0, N)
        y = rule_cep(x, None, t, 2, N)
        c = y[..., :13]
        for m, s in ((1, t[1]), (2, t[2])):
            acc = np.zeros_like(c)
            for v in s:
                if v != 0:
                    acc = acc + c * v
            assert (bits(y[..., m * 13:(m + 1) * 13]) == bits(acc)).all()
    # vf: deltas behind it are +0, statics are written everywhere, and nothing behind vf reaches a counted frame
    x = normal_features(4, (3, 1, 30, 23))
    t = rule_tables(23, 13, "ortho", 22.0, 2)
    y = rule_cep(x, [30, 11, 0], t, 2, 2)
    assert not bits(y[1, :, 11:, 13:]).any() and not bits(y[2, :, :, 13:]).any() and (bits(y[..., :13]) == bits(rule_cepstra(x, t[0]))).all()
    x2 = x.copy()
    x2[1, :, 11:] = F32(3e38) / 23
    y2 = rule_cep(x2, [30, 11, 0], t, 2, 2)
    assert (bits(y2[1, :, :11]) == bits(y[1, :, :11])).all() and (bits(y2[1, :, 11:, 13:]) == 0).all()
    assert (bits(rule_cep(x[1:2, :, :11], None, t, 2, 2)) == bits(y[1:2, :, :11])).all()  # a row of vf frames is the same row


# ---------------------------------------------------------------------------------------------------------------------------
# 3. bounds against float64
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,K,norm,lifter", [(23, 13, "ortho", 22.0), (80, 80, None, 0.0), (256, 85, "ortho", 0.0), (1, 1, "ortho", 22.0)])
def test_cepstra_are_within_their_bound_of_float64(B, K, norm, lifter):
    x = normal_features(B * 7 + K, (1, 2, 50, B))
    D64 = table64(B, K, norm, lifter)
    got = rule_cepstra(x, D64.astype(F32)).astype(np.float64)
    want = x.astype(np.float64) @ D64.T
    bound = cep_bound(x, D64)
    print("cepstra (%d, %d): worst %.3f of the bound" % (B, K, float((np.abs(got - want) / bound).max())))
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("N", [1, 2, 8])
def test_deltas_are_within_their_bound_of_float64(N):
    """Every delta lies within (2 o N + 3) 2^-24 sum_j |c[.]| |s64[j]| of the same filter in float64 over the rule's own f32
    cepstra: at most 2 o N additions behind a product, one rounding for the product and one for the scale."""
    F, K = 45, 13
    t = rule_tables(23, K, "ortho", 22.0, N)
    x = normal_features(N, (3, 1, F, 23))
    vf = [F, 2 * N, 1]
    y = rule_cep(x, vf, t, 2, N)
    c = y[..., :K].astype(np.float64)
    worst = 0.0
    for m, s in ((1, scales64(N)[0]), (2, scales64(N)[1])):
        for i, n in enumerate(vf):
            f = np.arange(n)
            want, mag = np.zeros((n, K)), np.zeros((n, K))
            for j in range(-m * N, m * N + 1):
                cc = c[i, 0, np.clip(f + j, 0, n - 1)]
                want += cc * s[j + m * N]
                mag += np.abs(cc) * abs(s[j + m * N])
            bound = (2 * 2 * N + 3) * 2.0 ** -24 * mag
            err = np.abs(y[i, 0, :n, m * K:(m + 1) * K].astype(np.float64) - want)
            assert (err <= bound).all(), (m, i)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("deltas N=%d: worst %.3f of the bound" % (N, worst))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Kaldi's algorithm, restated in float64
# ---------------------------------------------------------------------------------------------------------------------------

def kaldi_mfcc_deltas64(logmel, num_ceps, cepstral_lifter, order, window):
    """compute-mfcc-feats' tail and add-deltas over logmel (F, B), in float64 and written from Kaldi's description: the DCT matrix
    of ComputeDctMatrix (row 0 sqrt(1 / B), row k sqrt(2 / B) cos(pi / B (n + 0.5) k)), truncated to num_ceps rows and applied;
    then the lifter coefficients 1 + 0.5 Q sin(pi i / Q) multiplied in; then DeltaFeatures: scales_[0] = (1), scales_[i] = the
    convolution of scales_[i - 1] with (j, j = -window .. window) divided by sum j^2, and every output block i the sum over the
    offsets of scales_[i][j] * input[clamp(frame + j)]."""
    F, B = logmel.shape
    M = np.empty((B, B))
    M[0] = math.sqrt(1.0 / B)
    for k in range(1, B):
        for n in range(B):
            M[k, n] = math.sqrt(2.0 / B) * math.cos(math.pi / B * (n + 0.5) * k)
    feat = logmel @ M[:num_ceps].T
    if cepstral_lifter != 0.0:
        feat = feat * np.asarray([1.0 + 0.5 * cepstral_lifter * math.sin(math.pi * i / cepstral_lifter) for i in range(num_ceps)])
    scales = [np.ones(1)]
    for i in range(1, order + 1):
        prev = scales[i - 1]
        cur = np.zeros(len(prev) + 2 * window)
        normalizer = 0.0
        for j in range(-window, window + 1):
            normalizer += j * j
            for k in range(len(prev)):
                cur[j + k + window] += j * prev[k]
        scales.append(cur * (1.0 / normalizer))
    out = np.zeros((F, (order + 1) * num_ceps))
    for frame in range(F):
        for i in range(order + 1):
            sc = scales[i]
            max_offset = (len(sc) - 1) // 2
            for j in range(-max_offset, max_offset + 1):
                offset_frame = min(max(frame + j, 0), F - 1)
                out[frame, i * num_ceps:(i + 1) * num_ceps] += sc[j + max_offset] * feat[offset_frame]
    return out


@pytest.mark.parametrize("window", [1, 2, 3])
def test_the_rule_in_float64_is_kaldis_algorithm(window):
    """The float64 form of the rule -- the lifter folded into the table, the composite filters s_1 and s_2 with clamped indices --
    agrees with the restatement to 1e-12 relative: the folding and the composite filter are Kaldi's mathematics."""
    F, B, K, Q = 37, 23, 13, 22.0
    x = normal_features(window, (F, B)).astype(np.float64)
    want = kaldi_mfcc_deltas64(x, K, Q, 2, window)
    c = x @ table64(B, K, "ortho", Q).T
    parts = [c]
    f = np.arange(F)
    for m, s in enumerate(scales64(window), 1):
        parts.append(sum(c[np.clip(f + j, 0, F - 1)] * s[j + m * window] for j in range(-m * window, m * window + 1)))
    got = np.concatenate(parts, axis=1)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # a short utterance as well: fewer frames than the filter is long
    assert np.abs(kaldi_mfcc_deltas64(x[:2], K, Q, 2, window)[:, :K] - c[:2]).max() <= 1e-12 * np.abs(c).max()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. argument errors, each before NVH_ERR_NO_GPU
# ---------------------------------------------------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")
# every field just outside its limit (the descriptor otherwise make_cdesc's, with a shape)
BAD_FIELDS = [{"transform": -1}, {"transform": 2}, {"dct_norm": -1}, {"dct_norm": 2}, {"transform": 0, "ceps": 23, "dct_norm": 2},
              {"order": -1}, {"order": 3}, {"window": 0}, {"window": 9}, {"order": 0, "window": 0}, {"order": 0, "window": 9},
              {"rows": -1}, {"channels": 0}, {"channels": 65536}, {"frames": -1}, {"frames": (1 << 24) + 1}, {"bands": 0},
              {"bands": 257}, {"ceps": 0}, {"ceps": 24}, {"ceps": -1}, {"transform": 0, "ceps": 13}, {"transform": 0, "ceps": 24},
              {"bands": 256, "ceps": 86}, {"bands": 256, "ceps": 129, "order": 1}, {"bands": 100, "ceps": 100, "transform": 0},
              {"lifter": -1.0}, {"lifter": NAN}, {"lifter": INF}, {"transform": 0, "ceps": 23, "lifter": NAN},
              {"reserved": (1, 0)}, {"reserved": (0, -1)}]
SHAPE = dict(rows=2, channels=1, frames=5, src_row_stride=115, src_chan_stride=115, src_frame_stride=23, src_band_stride=1,
             dst_row_stride=195, dst_chan_stride=195, dst_frame_stride=39, dst_col_stride=1)
GOOD_FIELDS = [{}, {"frames": 1 << 24}, {"frames": 0}, {"rows": 0}, {"channels": 65535}, {"bands": 256, "ceps": 85}, {"bands": 256, "ceps": 128, "order": 1},
               {"bands": 256, "ceps": 256, "order": 0}, {"bands": 256, "ceps": 256, "order": 0, "transform": 0}, {"bands": 1, "ceps": 1},
               {"window": 1}, {"window": 8}, {"lifter": 22.0}, {"lifter": 0.0}, {"lifter": 3e38}, {"dct_norm": 1}, {"transform": 0, "ceps": 23},
               {"bands": 85, "ceps": 85, "transform": 0}]


def bad_desc(bad):
    d = make_cdesc(**dict(SHAPE, **{k: v for k, v in bad.items() if k != "reserved"}))
    if "reserved" in bad:
        d.reserved[0], d.reserved[1] = bad["reserved"]
    return d


def test_check_refuses_every_number_outside_the_rule():
    from nvorbis_amd import native
    L = native.lib()
    assert L.nvh_cep_check(None) == native.ERR_ARGUMENT
    for bad in BAD_FIELDS:
        assert L.nvh_cep_check(C.byref(bad_desc(bad))) == native.ERR_ARGUMENT, bad
    for good in GOOD_FIELDS:
        assert L.nvh_cep_check(C.byref(bad_desc(good))) == native.OK, good


def test_rows_entry_point_checks_its_arguments_before_a_device():
    """nvh_cep_rows without a context: every argument error comes first, then NVH_ERR_NO_GPU."""
    from nvorbis_amd import native
    L = native.lib()
    fake = C.c_void_p(4096)  # never dereferenced: there is no context

    def call(d, vf=(5, 0), src=fake, dst=fake):
        v = None if vf is None else (C.c_int64 * len(vf))(*vf)
        return L.nvh_cep_rows(None, None if d is None else C.byref(d), src, dst, v)
    assert call(None) == native.ERR_ARGUMENT
    for bad in BAD_FIELDS:
        assert call(bad_desc(bad)) == native.ERR_ARGUMENT, bad
    good = bad_desc({})
    assert call(good, src=None) == native.ERR_ARGUMENT and call(good, dst=None) == native.ERR_ARGUMENT
    assert call(good, vf=(6, 0)) == native.ERR_ARGUMENT and call(good, vf=(5, -1)) == native.ERR_ARGUMENT
    assert call(good) == native.ERR_NO_GPU and call(good, vf=None) == native.ERR_NO_GPU and call(good, vf=(0, 5)) == native.ERR_NO_GPU
    assert call(bad_desc({"rows": 0}), vf=None, src=None, dst=None) == native.ERR_NO_GPU  # (nothing to do, but no context either)
    assert call(bad_desc({"frames": 0}), vf=(0, 0), src=None, dst=None) == native.ERR_NO_GPU
    assert call(bad_desc({"frames": 0}), vf=(1, 0), src=None, dst=None) == native.ERR_ARGUMENT
    # the route's export checks the descriptor alone
    out = (C.c_int64 * 4)()
    assert L.nvh_cep_route(C.byref(good), None) == native.ERR_ARGUMENT and L.nvh_cep_route(None, out) == native.ERR_ARGUMENT
    for bad in BAD_FIELDS:
        assert L.nvh_cep_route(C.byref(bad_desc(bad)), out) == native.ERR_ARGUMENT, bad
    assert L.nvh_cep_route(C.byref(good), out) == native.OK


def test_cep_desc_in_python():
    from nvorbis_amd import clips, native
    import nvorbis_amd as nv
    d = nv.cep_desc(13, "ortho", 22.0, 2, 3, frames=7, bands=23)
    assert (d.transform, d.dct_norm, d.order, d.window, d.frames, d.bands, d.ceps) == (native.CEP_DCT2, native.CEP_ORTHO, 2, 3, 7, 23, 13)
    assert d.lifter == 22.0 and (d.rows, d.channels) == (0, 0)
    d = clips.cep_desc(None, None, bands=80, deltas=1)
    assert (d.transform, d.dct_norm, d.ceps, d.order, d.window) == (native.CEP_NONE, native.CEP_PLAIN, 80, 1, 2)
    assert clips.cep_desc(bands=256).ceps == 256 and clips.cep_desc(85, bands=256, deltas=2).ceps == 85
    for bad in BAD_KEYWORDS + [{"frames": -1}, {"frames": (1 << 24) + 1}, {"bands": 0}, {"bands": 257}, {"bands": 80.0}]:
        with pytest.raises(ValueError):
            clips.cep_desc(**dict({"bands": 80}, **bad))


# (n_mels = 80 in the calls below)
BAD_KEYWORDS = [{"cepstra": 0}, {"cepstra": 81}, {"cepstra": -1}, {"cepstra": 13.0}, {"cepstra": True}, {"cepstra": "13"},
                {"dct_norm": "orthogonal"}, {"dct_norm": 0}, {"dct_norm": False}, {"lifter": -1.0}, {"lifter": NAN}, {"lifter": INF},
                {"lifter": 1e39}, {"lifter": None}, {"lifter": "22"}, {"lifter": True}, {"deltas": -1}, {"deltas": 3}, {"deltas": 1.0},
                {"deltas": True}, {"deltas": None}, {"delta_window": 0}, {"delta_window": 9}, {"delta_window": 2.0}, {"delta_window": None},
                {"delta_window": True}, {"deltas": 2, "cepstra": None, "bands": 86}, {"deltas": 1, "cepstra": 129, "bands": 256}]


def test_decode_clip_features_refuses_bad_cepstral_keywords_before_a_device(ogg_bytes):
    """Every ValueError of the new keywords, whatever the others are, on a machine that may have no device at all."""
    import nvorbis_amd as nv
    good = ogg_bytes["3test"]
    for bad in BAD_KEYWORDS:
        bad = dict(bad)
        n_mels = bad.pop("bands", 80)
        for base in ({}, {"cepstra": 13}, {"deltas": 2, "cepstra": 20}, {"normalize": "mean_var"}):
            with pytest.raises(ValueError):
                nv.decode_clip_features([good], 4000, n_mels=n_mels, **dict(base, **bad))
    with pytest.raises(ValueError):  # Q > 256
        nv.decode_clip_features([good], 4000, n_mels=128, deltas=2)
    with pytest.raises(TypeError):
        nv.decode_clip_features([good], 4000, None, cepstra=13, delta=2)


def test_kaldi_mfcc_keywords():
    import nvorbis_amd as nv
    kw = nv.kaldi_mfcc_keywords(16000)
    fb = nv.kaldi_fbank_keywords(16000, num_mel_bins=23)
    assert {k: v for k, v in kw.items() if k in fb} == fb
    assert {k: v for k, v in kw.items() if k not in fb} == dict(cepstra=13, dct_norm="ortho", lifter=22.0)
    kw = nv.kaldi_mfcc_keywords(8000, num_ceps=20, num_mel_bins=40, cepstral_lifter=0.0, high_freq=-200.0, window="hamming")
    assert (kw["cepstra"], kw["n_mels"], kw["lifter"], kw["f_max"], kw["window"]) == (20, 40, 0.0, 3800.0, "hamming")
    for bad in ({"num_ceps": 0}, {"num_ceps": 24}, {"num_ceps": 13.0}, {"num_mel_bins": 0}, {"num_mel_bins": 257}, {"cepstral_lifter": -1.0},
                {"cepstral_lifter": NAN}, {"cepstral_lifter": "22"}, {"frame_length_ms": 0.0}):
        with pytest.raises(ValueError):
            nv.kaldi_mfcc_keywords(16000, **bad)

"""Rows at one sample rate on the GPU: k_resample_rows alone on synthetic rows, and decode_clip_rows(sample_rate=...) against the
CPU oracle (include/nvorbis_hip.h states the rule under nvh_resample_rows).

The reference is the rule in numpy with the LIBRARY'S OWN tap table (tests/test_resample_plan.py holds that table to the formula):
a loop over the taps, float32 product, float32 sum, one accumulator.  No tolerance anywhere: floats are compared as uint32, 16-bit
samples as int16.  Output J of the rule depends on nothing but the source samples around (J * M) div L, so the reference computes
the outputs a row holds instead of resampling the whole clip and slicing -- the same numbers."""
import os
import struct

import numpy as np
import pytest

from tests.test_clip_batches import CLIP, _torch, mix_rule, same_bits, to_s16
from tests.test_resample_plan import lib_taps, rule_plan

KERNEL_PAIRS = [(44100, 16000), (44100, 48000), (48000, 16000), (8000, 44100)]
SENT = {np.dtype(np.float32): np.float32(-1234.5), np.dtype(np.int16): np.int16(-7777)}


def rule_outputs(x, origin, fi, fo, start, count):
    """Outputs [start, start + count) of the rule over source samples x (float32, x[e] = source sample origin + e; 0 outside):
    (float32 values after the second clip, whether it clamped)."""
    L, M, half, _ = rule_plan(fi, fo)
    h = lib_taps(fi, fo)
    n = (start + np.arange(count, dtype=np.int64)) * M
    c, p = n // L, n % L
    x = np.asarray(x, np.float32)
    acc = np.zeros(count, np.float32)
    for k in range(2 * half):
        s = c - half + 1 + k - origin
        ok = (s >= 0) & (s < x.size)
        xv = np.where(ok, x[np.clip(s, 0, max(x.size - 1, 0))] if x.size else np.float32(0), np.float32(0)).astype(np.float32)
        acc = (acc + (xv * h[p, k]).astype(np.float32)).astype(np.float32)
    hit = (acc > CLIP) | (acc < -CLIP)
    return np.where(acc > CLIP, CLIP, np.where(acc < -CLIP, -CLIP, acc)).astype(np.float32), bool(hit.any())


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------

def kernel_case(fi, fo, T):
    """Six rows of two channels and their reference, computed once per (pair, T): per row (origin, start, valid), the source
    block X[row, channel, S] and the expected float32 block R[row, channel, T] with the per-(row, channel) clip flags."""
    from nvorbis_amd import native
    L, M, half, _ = rule_plan(fi, fo)
    tile = native.RESAMPLE_TILE
    rng = np.random.default_rng(fi * 7 + fo + T)
    starts = [0, 1000, 77, 12345, 2 ** 33, 31]
    valids = [T, T, 0, min(T, tile + 100) if T > tile else T // 2, T, T]
    rows, need = [], 4
    for r, (st, v) in enumerate(zip(starts, valids)):
        c_first = st * M // L
        origin = max(0, c_first - half + 1)
        if r == 1:
            origin += 5  # the row's first reads fall in front of the row: zeros
        rows.append((origin, st, v))
        if v:
            need = max(need, (st + v - 1) * M // L + half + 1 - origin)
    S = need - 3  # ... and the longest row's last reads behind it
    X = rng.uniform(-1.2, 1.2, size=(len(rows), 2, S)).astype(np.float32)
    X[0, 0, : S // 2] = 1.15  # a held level above the clip: the filter's DC gain is 1, the second clip fires
    X[3, 1, :] = -1.15
    X[4, 0, :2 * half + 8] = 1.15  # (row 4 has its whole margin: its first output already clips)
    X[1] *= np.float32(0.05)  # a quiet row: no clip
    X[5] = 0
    q = min(S - 1, 31 * M // L + 3 - rows[5][0])
    X[5, :, q] = 1.0  # the unit impulse
    R = np.zeros((len(rows), 2, T), np.float32)
    hit = np.zeros((len(rows), 2), bool)
    for r, (origin, st, v) in enumerate(rows):
        for ch in range(2):
            R[r, ch, :v], hit[r, ch] = rule_outputs(X[r, ch], origin, fi, fo, st, v)
    # the impulse row reproduces the phases' taps: output J holds h[p][q + origin - c + half - 1] where that is a tap, else 0
    h = lib_taps(fi, fo)
    n = (31 + np.arange(valids[5], dtype=np.int64)) * M
    k = q + rows[5][0] - n // L + half - 1
    want = np.where((k >= 0) & (k < 2 * half), h[n % L, np.clip(k, 0, 2 * half - 1)], np.float32(0)).astype(np.float32)
    assert same_bits(R[5, 0, :valids[5]], want) and (want != 0).any()
    for a in (X, R, hit):
        a.setflags(write=False)
    return rows, X, R, hit


_KERNEL_CASES = {}


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 63, "3 tiles + 17"])
@pytest.mark.parametrize("fi,fo", KERNEL_PAIRS)
def test_kernel_alone(gpu_ctx, fi, fo, T):
    """nvh_resample_rows on synthetic rows, f32 and s16, interleaved / planar / mono strides, destination rows permuted: every
    row equals the numpy rule, the flag words equal the reference's, rows and tiles behind `valid` are zeros, the destination row
    nobody names and the tail behind the buffer keep their sentinel.  Row 4 starts at 2**33 (a 32-bit J * M goes wrong there),
    row 1 reads in front of its source row and the longest row behind it, row 5 is a unit impulse."""
    from nvorbis_amd import native
    T = 3 * native.RESAMPLE_TILE + 17 if isinstance(T, str) else T
    key = (fi, fo, T)
    if key not in _KERNEL_CASES:
        _KERNEL_CASES[key] = kernel_case(fi, fo, T)
    check_kernel_case(gpu_ctx, fi, fo, T, _KERNEL_CASES[key])


def check_kernel_case(gpu_ctx, fi, fo, T, case):
    """The launches and assertions of test_kernel_alone over one kernel_case(fi, fo, T)."""
    torch = _torch()
    from nvorbis_amd import native
    rows, X, R, hit = case
    N, S = len(rows), X.shape[2]
    assert hit.any(axis=1).any() and not hit.any(axis=1).all()
    dst_row = np.asarray([3, 0, 6, 1, 5, 2], np.int32)  # destination row 4 is nobody's
    ND = 7
    origin, start, valid = ([r[k] for r in rows] for k in range(3))
    for layout in ("interleaved", "planar", "mono"):
        C_ = 1 if layout == "mono" else 2
        if layout == "interleaved":
            src = np.ascontiguousarray(X.transpose(0, 2, 1))  # (N, S, 2)
            sstr, dstr, dshape = (S * 2, 2, 1), (T * 2, 2, 1), (ND, T, 2)
        elif layout == "planar":
            src = np.ascontiguousarray(X.transpose(1, 0, 2))  # (2, N, S)
            sstr, dstr, dshape = (S, 1, N * S), (T, 1, ND * T), (2, ND, T)
        else:
            src = np.ascontiguousarray(X[:, 0, :])  # (N, S)
            sstr, dstr, dshape = (S, 1, 0), (T, 1, 0), (ND, T)
        d_src = torch.from_numpy(src).cuda()
        for dt in (np.float32, np.int16):
            tdt = torch.float32 if dt == np.float32 else torch.int16
            count = int(np.prod(dshape))
            d_dst = torch.full((count + 64,), float(SENT[np.dtype(dt)]), dtype=tdt, device="cuda")
            d_flags = torch.zeros(ND, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            desc = native.ResampleDesc(in_rate=fi, out_rate=fo, rows=N, channels=C_, format=native.PCM_S16 if dt == np.int16 else native.PCM_F32,
                                       length=T, src_length=S, src_row_stride=sstr[0], src_time_stride=sstr[1], src_chan_stride=sstr[2],
                                       dst_row_stride=dstr[0], dst_time_stride=dstr[1], dst_chan_stride=dstr[2])
            gpu_ctx.resample_rows(desc, d_src.data_ptr(), d_dst.data_ptr(), origin, start, valid, dst_row, d_flags.data_ptr())
            gpu_ctx.synchronize()
            got = d_dst.cpu().numpy()
            flags = d_flags.cpu().numpy() != 0
            assert (got[count:] == SENT[np.dtype(dt)]).all(), "written behind the destination"
            got = got[:count].reshape(dshape)
            for r in range(N):
                d = int(dst_row[r])
                for ch in range(C_):
                    row = got[d, :, ch] if layout == "interleaved" else got[ch, d] if layout == "planar" else got[d]
                    want = R[r, ch] if dt == np.float32 else to_s16(R[r, ch])
                    assert same_bits(np.ascontiguousarray(row), want), (layout, dt, r, ch, rows[r])
                    assert not np.ascontiguousarray(row[valid[r]:]).view(np.uint8).any()
                assert flags[d] == hit[r, :C_].any(), (layout, dt, r, flags, hit)
            nobody = got[4] if layout != "planar" else got[:, 4]
            assert (nobody == SENT[np.dtype(dt)]).all() and not flags[4]


@pytest.mark.gpu
def test_a_table_and_a_span_beyond_lds(gpu_ctx):
    """(1024, 1): 32768 taps per output and a source span per tile far beyond the LDS budget, and (1, 4096): 4096 phases, a table
    of 131072 taps.  Both tables are read through L2, the first one's samples as well; both equal the rule."""
    torch = _torch()
    from nvorbis_amd import native
    for fi, fo, T, start in ((1024, 1, 5, 3), (1, 4096, 700, 4000)):
        L, M, half, _ = rule_plan(fi, fo)
        origin = max(0, start * M // L - half + 1)
        S = (start + T - 1) * M // L + half + 1 - origin
        x = np.random.default_rng(T).uniform(-1.2, 1.2, S).astype(np.float32)
        want, hit = rule_outputs(x, origin, fi, fo, start, T)
        d_src = torch.from_numpy(x).cuda()
        d_dst = torch.full((T + 16,), float(SENT[np.dtype(np.float32)]), dtype=torch.float32, device="cuda")
        d_flags = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        desc = native.ResampleDesc(in_rate=fi, out_rate=fo, rows=1, channels=1, format=native.PCM_F32, length=T, src_length=S,
                                   src_row_stride=S, src_time_stride=1, src_chan_stride=0, dst_row_stride=T, dst_time_stride=1,
                                   dst_chan_stride=0)
        gpu_ctx.resample_rows(desc, d_src.data_ptr(), d_dst.data_ptr(), [origin], [start], [T], None, d_flags.data_ptr())
        gpu_ctx.synchronize()
        got = d_dst.cpu().numpy()
        assert same_bits(got[:T], want) and (got[T:] == SENT[np.dtype(np.float32)]).all(), (fi, fo)
        assert bool(d_flags.cpu().numpy()[0]) == hit


# ---------------------------------------------------------------------------------------------------------------------------
# through decode_clip_rows
# ---------------------------------------------------------------------------------------------------------------------------

FILES = ("1test", "2test", "3test", "issue6test")  # mono, mono, stereo, stereo; all 44100 Hz
_CLIPS, _REFS, _ROWS = {}, {}, {}


def clip_at(ogg_bytes, name, rate):
    """The golden file, or a copy whose identification packet says `rate` (re-paged; every packet's granule is the serial
    decoder's position behind it, so every page carries a granule and the last one the clip's length).  The PCM is unchanged."""
    import nvorbis_amd as nv
    from tests import ogg_py
    if (name, rate) not in _CLIPS:
        data = ogg_bytes[name]
        if rate != 44100:
            pa = nv.demux_ogg_array(data, 0)
            st = nv.Stream(None, pa[0], pa[1], pa[2])
            try:
                assert st.sample_rate == 44100
                pos, _, _, total = st.index_packets(pa, 3)
            finally:
                st.close()
            pk = [bytes(pa[i]) for i in range(len(pa))]
            pk[0] = pk[0][:12] + struct.pack("<I", rate) + pk[0][16:]
            eos = bool(nv.demux_ogg(data)[2][-1] & 1)  # (issue6test.ogg ends without the flag: its tail is drained, not trimmed)
            data = ogg_py.write_ogg(pk, [0, 0, 0] + [int(v) for v in pos], eos=eos)
            pb = nv.demux_ogg_array(data, 0)
            sb = nv.Stream(None, pb[0], pb[1], pb[2])
            try:
                assert sb.sample_rate == rate and sb.index_packets(pb, 3)[3] == total
            finally:
                sb.close()
        _CLIPS[(name, rate)] = data
    return _CLIPS[(name, rate)]


def file_pcm(oracle, ogg_bytes, name, rate, clip):
    """The oracle's whole-file PCM [T, channels] of the (rewritten) file; the rewritten files decode to the golden file's bits."""
    key = (name, rate, clip)
    if key not in _REFS:
        pcm, info = oracle.decode_ogg(clip_at(ogg_bytes, name, rate), clip=clip)
        pcm = pcm.reshape(-1, info["channels"])
        if rate != 44100:
            assert same_bits(pcm, file_pcm(oracle, ogg_bytes, name, 44100, clip))
        pcm.setflags(write=False)
        _REFS[key] = pcm
    return _REFS[key]


def form_source(oracle, ogg_bytes, name, rate, form):
    """(x [T, och] float32: the clip in the requested output form, before the resampler; u: the same before ClipSamples' clip)."""
    if form == "mono":
        raw = file_pcm(oracle, ogg_bytes, name, rate, False)
        return mix_rule(raw, raw.shape[1], True).reshape(-1, 1), mix_rule(raw, raw.shape[1], False).reshape(-1, 1)
    x, u = file_pcm(oracle, ogg_bytes, name, rate, True), file_pcm(oracle, ogg_bytes, name, rate, False)
    if form == "map":
        return x[:, 1:2], u[:, 1:2]
    return x, u


def want_row(oracle, ogg_bytes, name, rate, target, form, start, length):
    """(row [length, och] float32, valid, decode flag of the source window, resampler's flag) of one row, cached."""
    key = (name, rate, target, "mono" if form == "mono" else "map" if form == "map" else "pcm", start, length)
    if key not in _ROWS:
        x, u = form_source(oracle, ogg_bytes, name, rate, form)
        total = x.shape[0]
        row = np.zeros((length, x.shape[1]), np.float32)
        if rate == target:
            cut = x[start:start + length]
            row[:cut.shape[0]] = cut
            w = u[start:start + length]
            _ROWS[key] = (row, cut.shape[0], bool(((w > CLIP) | (w < -CLIP)).any()), False)
        else:
            L, M, half, _ = rule_plan(rate, target)
            valid = min(length, max(0, (total * L + M - 1) // M - start))
            dec = res = False
            if valid:
                for ch in range(x.shape[1]):
                    row[:valid, ch], hit = rule_outputs(x[:, ch], 0, rate, target, start, valid)
                    res |= hit
                origin = max(0, start * M // L - half + 1) & ~3
                take = ((start + valid - 1) * M // L + half + 1 - origin + 3) & ~3
                w = u[origin:origin + take]
                dec = bool(((w > CLIP) | (w < -CLIP)).any())
            _ROWS[key] = (row, valid, dec, res)
        _ROWS[key][0].setflags(write=False)
    return _ROWS[key]


def name_sets(form):
    """Files whose channel counts differ share a tensor only under the mono mix; a map that selects channel 1 needs stereo."""
    return [FILES] if form == "mono" else [("3test", "issue6test"), ("1test", "2test")] if form in ("f32", "s16") else [("3test", "issue6test")]


def the_calls(ogg_bytes, names, target):
    """[(name, rate, start)] of one call: source rates 44100, 48000 and 8000 mixed, starts at 0, inside the first `half` outputs,
    in the middle, across the clip's end and beyond it, and on the stretch of 3test.ogg that clips."""
    import nvorbis_amd as nv
    out = []
    for k, name in enumerate(names):
        for j, rate in enumerate((44100, 48000, 8000)):
            pa = nv.demux_ogg_array(ogg_bytes[name], 0)
            st = nv.Stream(None, pa[0], pa[1], pa[2])
            try:
                total = st.index_packets(pa, 3)[3]
            finally:
                st.close()
            L, M = rule_plan(rate, target)[:2]  # (1, 1 for a clip at the target rate)
            total_out = (total * L + M - 1) // M
            starts = [0, 7, (total_out // 2) & ~3, total_out - 300, total_out + 5]
            starts = starts if (k + j) % 2 == 0 else starts[::-1][:3]
            if name == "3test":
                starts.append(7600 * L // M)  # 3test.ogg clips from source sample 7706 on: the rows' flags are not all clear
            out += [(name, rate, s) for s in starts]
    return out


def form_kwargs(form):
    return {"f32": {}, "s16": {"sample_format": "s16"}, "planar": {"layout": "planar"}, "mono": {"mix": "mono"},
            "map": {"channel_map": (1,)}}[form]


def assemble(rows, form):
    out = np.stack([to_s16(r) if form == "s16" else r for r in rows])  # (N, length, och)
    if form == "mono":
        return out[:, :, 0]
    return out.transpose(0, 2, 1) if form == "planar" else out


@pytest.mark.gpu
@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("form", ["f32", "s16", "planar", "mono", "map"])
def test_decode_clip_rows_at_one_rate(oracle, gpu_ctx, ogg_bytes, form, device_out):
    """One call mixes clips at 44100, 48000 and 8000 Hz with sample_rate=16000 (every row resampled) and a second one with
    sample_rate=44100 (the 44100 Hz clips' rows are today's, the others resampled), lengths 1000 and 1001, both parsers: rows,
    valid and the per-row clip flags equal oracle PCM -> numpy rule."""
    _torch()
    import nvorbis_amd as nv
    for target, names in [(t, n) for t in (16000, 44100) for n in name_sets(form)]:
        calls = the_calls(ogg_bytes, names, target)
        files = [clip_at(ogg_bytes, n, r) for n, r, _ in calls]
        starts = [s for _, _, s in calls]
        for length, gpu_parse in ((1000, True), (1001, False), (1000, False)):
            ref = [want_row(oracle, ogg_bytes, n, r, target, form, s, length) for n, r, s in calls]
            (rows, valid), clipped = nv.decode_clip_rows(files, length, starts, ctx=gpu_ctx, batch_frames=16, gpu_parse=gpu_parse,
                                                         device_out=device_out, return_clipped=True, sample_rate=target,
                                                         **form_kwargs(form))
            want_valid = np.asarray([v for _, v, _, _ in ref], np.int64)
            assert np.array_equal(valid, want_valid) and valid.dtype == np.int64
            assert (valid == 0).any() and (valid == length).any() and ((valid > 0) & (valid < length)).any()
            host = rows.cpu().numpy() if device_out else rows
            want = assemble([r for r, _, _, _ in ref], form)
            assert tuple(host.shape) == want.shape, (host.shape, want.shape)
            bad = [i for i in range(len(calls)) if not same_bits(np.ascontiguousarray(host[i]), np.ascontiguousarray(want[i]))]
            assert not bad, (form, device_out, target, length, gpu_parse, [calls[i] for i in bad])
            want_clipped = np.asarray([d or r for _, _, d, r in ref])
            assert np.array_equal(clipped, want_clipped), (form, target, length, clipped, want_clipped)
            plain, plain_valid = nv.decode_clip_rows(files, length, starts, ctx=gpu_ctx, batch_frames=16, gpu_parse=gpu_parse,
                                                     device_out=device_out, sample_rate=target, **form_kwargs(form))
            assert np.array_equal(plain_valid, valid)
            assert same_bits(np.ascontiguousarray(plain.cpu().numpy() if device_out else plain), np.ascontiguousarray(host))


def test_the_flags_fire_somewhere(oracle, ogg_bytes):
    """The references of the calls above are not all-quiet: some row's source window clipped in the decode stage, some row's
    outputs in the resampler, most rows in neither."""
    for form in ("f32", "mono", "map"):
        names = name_sets(form)[0]
        refs = [want_row(oracle, ogg_bytes, n, r, 16000, form, s, 1000) for n, r, s in the_calls(ogg_bytes, names, 16000)]
        assert any(d for _, _, d, _ in refs) and not all(d or r for _, _, d, r in refs), form
    refs = [want_row(oracle, ogg_bytes, n, r, t, "f32", s, 1000) for t in (16000, 44100) for n, r, s in the_calls(ogg_bytes, names, t)]
    assert any(r for _, _, _, r in refs)


@pytest.mark.gpu
@pytest.mark.parametrize("device_out", [False, True])
def test_every_clip_at_the_target_rate_is_todays_call(oracle, gpu_ctx, ogg_bytes, monkeypatch, device_out):
    """sample_rate equal to every clip's rate: the bits of the call without the keyword, and no batch names k_resample_rows."""
    _torch()
    import nvorbis_amd as nv
    from nvorbis_amd import clips as clips_mod
    named, seen = [], []
    flush = clips_mod._RowGroup.flush

    def spy(self):
        flush(self)
        named.append(",".join(self.stream.kernels()))
    monkeypatch.setattr(clips_mod._RowGroup, "flush", spy)
    files = [ogg_bytes["3test"], ogg_bytes["issue6test"]] * 3
    starts = [0, 4, 1001, 20000, 7, 50000]
    for kw in ({}, {"sample_format": "s16"}, {"layout": "planar"}, {"mix": "mono"}):
        a, va = nv.decode_clip_rows(files, 1000, starts, ctx=gpu_ctx, batch_frames=16, device_out=device_out, **kw)
        count = len(named)
        b, vb = nv.decode_clip_rows(files, 1000, starts, ctx=gpu_ctx, batch_frames=16, device_out=device_out, sample_rate=44100, **kw)
        assert len(named) == 2 * count and named[:count] == named[count:] and count > 0
        assert np.array_equal(va, vb)
        ha, hb = (a.cpu().numpy(), b.cpu().numpy()) if device_out else (a, b)
        assert same_bits(np.ascontiguousarray(ha), np.ascontiguousarray(hb))
        seen += named
        del named[:]
    assert seen and not any("k_resample_rows" in k for k in seen)

"""The launch routes of k_resample_rows, k_mel_rows and k_fnorm_rows that the kernels' own test files do not reach: taps in LDS with
the source through L2 (and both source routes inside one launch), a tile span on the two sides of its LDS budget, a workgroup that
walks several tiles; the unstaged transform below n_fft = 4096 with every grouping of its stages; more frames than a workgroup has
threads; the re-reading route walking its work items.

Every launcher chooses its route from budgets (csrc/resample_dev.h, mel_dev.h, fnorm_dev.h).  resample_route, mel_route and
fnorm_route below redo that choice on the CPU, the budgets read from the headers' #define lines, and the tests without a gpu mark
hold every case to the route it is here for: a case that a changed budget moves elsewhere fails there.  The gpu tests compare with
the numpy rules of the kernels' own test files, as uint32 or int16: no tolerance anywhere.

What the gpu tests see, measured once on an MI355X with a library built from a copy of csrc/ in which one value was changed (no
index, bound or barrier; nothing of it is kept).  Each row: the change; the tests here that then fail; the gpu tests of
test_resample_rows.py, test_mel_rows.py, test_fnorm_rows.py and test_clip_load.py (the other callers of the three kernels) all pass.
  resample_chains: prod negated under !SRC_LDS && TAPS_LDS   test_taps_in_lds_source_through_l2[* - 2 tiles + 17],
                                                             test_span_on_both_sides_of_the_lds_budget[264-35]
  k_resample_rows: acc negated where span is the budget
    or one more                                              test_span_on_both_sides_of_the_lds_budget[264-35], [181-24]
  k_resample_rows: acc negated where tile != blockIdx.y      test_a_workgroup_walks_several_tiles[*]
  mel_pass: tr negated under !TWL && R == 1                  test_mel_unstaged_..[n_fft 64 / 30000, 256 / 6000, 2048 / 1024: 1, 4, 7]
  mel_pass: tr negated under !TWL && R == 2 && points < 512  test_mel_unstaged_..[n_fft 64 / 30000, 128 / 20000, 256 / 6000: 1, 4, 7]
  k_fnorm_rows: the last pass's value doubled where the
    destination is band-major and F > 512                    test_fnorm_more_frames_than_threads[*],
                                                             test_decode_clip_features_of_1001_frames[8-True], [24-True]
  k_fnorm_rows: eps doubled and gain negated for an item
    behind a re-reading workgroup's first                    test_fnorm_reread_walks_items
Every case's CPU reference takes under 0.2 s and every gpu test under 0.4 s (the largest: (1001, 80) through the whole matrix).

Every route of a kernel gives the same bits, so the gpu tests cannot see a launcher that chooses another route than the functions
here.  The library says what it would launch (nvh_resample_route, nvh_mel_route, nvh_fnorm_route: the launchers' own checks and
route functions, no GPU), every CPU test here holds that to the restatement for its cases, and test_route_sweep_* walk both sides
of every threshold.  In a copy of csrc/ with `>= 4096` turned into `> 4096` in resample_dev.h, `>= 16384` into `>` or the budget's
`<=` into `<` in mel_dev.h, or `<=` into `<` in fnorm_dev.h, test_route_sweep_resample / _mel / _mel / _fnorm fail and no other CPU
test does.  test_row_block_* queue three calls of each operation with no wait between them (nvh_internal.h: RowBlock)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import test_fnorm_rows as fnr
from tests import test_mel_rows as mlr
from tests import test_resample_rows as rsr
from tests.test_clip_batches import _torch, same_bits, to_s16
from tests.test_fnorm_plan import AXES, F32, MODES, make_fdesc, normal_features, rule_fnorm
from tests.test_mel_plan import lib_tables
from tests.test_resample_plan import rule_plan

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nvorbis_amd", "csrc")
_DEFINES = {}


def defines(header):
    """{name: value} of the integer #define lines of a csrc header (a value may name earlier ones)."""
    if header not in _DEFINES:
        out = {}
        for m in re.finditer(r"^#define\s+(NVH_\w+)\s+(.+?)\s*(?://.*)?$", open(os.path.join(CSRC, header)).read(), re.M):
            expr = re.sub(r"NVH_\w+", lambda k: str(out[k.group(0)]), m.group(2))
            assert re.fullmatch(r"[\d\s()+\-*/]+", expr), (header, m.group(0))
            out[m.group(1)] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}))
        _DEFINES[header] = out
    return _DEFINES[header]


# ---------------------------------------------------------------------------------------------------------------------------
# the launchers' choices, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------

def resample_route(fi, fo, channels, T, rows):
    """nvh_resample_rows' launch of rows [(origin, start, valid)]: (taps_in_lds, gy, spans), spans[row][tile] the source span of
    the tile's counted outputs (k_resample_rows stages it in LDS up to NVH_RS_SRC_FLOATS) or None where the tile is all pad."""
    D = defines("resample_dev.h")
    L, M, half, _ = rule_plan(fi, fo)
    tile = D["NVH_RS_TILE"]
    taps_in_lds = L * ((2 * half) | 1) <= D["NVH_RS_TAP_FLOATS"]
    tiles = (T + tile - 1) // tile
    gy = min((tiles + 3) // 4 if len(rows) * channels * tiles >= 4096 else tiles, 65535)
    spans = []
    for _, start, valid in rows:
        per = []
        for t0 in range(0, T, tile):
            vend = min(t0 + tile, T, valid)
            per.append((start + vend - 1) * M // L + half - ((start + t0) * M // L - half + 1) + 1 if vend > t0 else None)
        spans.append(per)
    return taps_in_lds, gy, spans


def in_lds(span):
    return span <= defines("resample_dev.h")["NVH_RS_SRC_FLOATS"]


def mel_route(cfg):
    """nvh_mel_rows' launch of (rate, n_fft, win_length, hop, n_mels): (staged, the stages per register pass).  The geometry is
    mel_dev.h's (its functions restated, its numbers read); the sparse bank's size comes from the library's dense bank."""
    D = defines("mel_dev.h")
    rate, N, W, H, B = cfg
    waves, points = D["NVH_MEL_WAVES"], N >> 1
    weights = 0
    for row in lib_tables(rate, N, W, B)[2]:
        nz = np.nonzero(row)[0]
        weights += int(nz[-1] - nz[0] + 1) if nz.size else 0
    fixed = waves * 2 * (points + ((points >> 6) << 3)) + waves * D["NVH_MEL_OUT_STRIDE"]
    tw_slots = points + (points >> 4) + 1
    staged = fixed + 2 * tw_slots + 3 * B + weights + W + (waves - 1) * H + W
    passes, left = [], N.bit_length() - 2  # the radix-2 stages half = 1 .. N/4
    while points >= 512 and left >= 3:
        passes.append(3)
        left -= 3
    passes += [2] * (left // 2) + [1] * (left % 2)
    return staged * 4 <= D["NVH_MEL_LDS_BYTES"], passes


def fnorm_route(F, B, items):
    """nvh_fnorm_rows' launch: (resident, workgroups, Walk's inner count can exceed the workgroup's threads)."""
    D = defines("fnorm_dev.h")
    return (F | 1) * B <= D["NVH_FNORM_DATA_FLOATS"], min(items, D["NVH_FNORM_MAX_BLOCKS"]), F > D["NVH_FNORM_THREADS"]


# ---------------------------------------------------------------------------------------------------------------------------
# the launchers' own choices: nvh_resample_route, nvh_mel_route and nvh_fnorm_route run the launchers' argument checks and route
# functions on the host, so a launcher that drifts from the three functions above fails here, not only one whose budget moved.
# full_*: the functions above with the fields they lack, written from the launchers' text as it stood before the exports existed
# (nvh_resample.hip, nvh_mel.hip, nvh_fnorm.hip at c952e63..02176a0), in the exports' order.
# ---------------------------------------------------------------------------------------------------------------------------

def lib_route(name, count, *descs):
    from nvorbis_amd import native
    out = (C.c_int64 * count)()
    rc = getattr(native.lib(), name)(*[None if d is None else C.byref(d) for d in descs], out)
    assert rc == native.OK, (name, rc)
    return list(out)


def lib_resample(fi, fo, channels, T, nrows):
    """[taps_in_lds, tiles, gy, lds_bytes] of the library."""
    from nvorbis_amd import native
    return lib_route("nvh_resample_route", 4, native.ResampleDesc(in_rate=fi, out_rate=fo, rows=nrows, channels=channels, format=native.PCM_F32,
                                                                   length=T, src_length=0))


def full_resample(fi, fo, channels, T, nrows):
    D = defines("resample_dev.h")
    L, M, half, _ = rule_plan(fi, fo)
    taps, gy, _ = resample_route(fi, fo, channels, T, [(0, 0, 0)] * nrows)
    padded = L * ((2 * half) | 1)
    return [int(taps), (T + D["NVH_RS_TILE"] - 1) // D["NVH_RS_TILE"], gy, ((padded if taps else 0) + D["NVH_RS_SRC_FLOATS"]) * 4]


def sparse_weights(bank):
    """Floats of the sparse bank: per band its first non-zero bin up to its last."""
    total = 0
    for row in bank:
        nz = np.nonzero(row)[0]
        total += int(nz[-1] - nz[0] + 1) if nz.size else 0
    return total


def lib_mel(cfg, rows=1, channels=1, frames=1, front=None):
    """[staged, span, lds_bytes, blocks, front_in_kernel, weights] of the library."""
    from tests.test_mel_plan import make_desc
    rate, N, W, H, B = cfg
    return lib_route("nvh_mel_route", 6, make_desc(rate, N, W, B, hop=H, rows=rows, channels=channels, frames=frames, src_length=4 * W), front)


def full_mel(cfg, rows=1, channels=1, frames=1, front=None):
    """`staged` is mel_route's (today's bank; a front with mel-domain triangles has a bank of its own: bank_of below)."""
    D = defines("mel_dev.h")
    rate, N, W, H, B = cfg
    waves, points = D["NVH_MEL_WAVES"], N >> 1
    staged = mel_route(cfg)[0]
    weights = sparse_weights(lib_tables(rate, N, W, B)[2])
    fixed = waves * 2 * (points + ((points >> 6) << 3)) + waves * D["NVH_MEL_OUT_STRIDE"]
    span = (waves - 1) * H + W
    floats = fixed + 2 * (points + (points >> 4) + 1) + 3 * B + weights + W + span
    assert staged == (floats * 4 <= D["NVH_MEL_LDS_BYTES"])
    total = rows * channels * ((frames + waves - 1) // waves)
    blocks = min((total + 3) // 4 if total >= 16384 else total, 1 << 20)
    default = front is None or (front.window, front.triangles, front.pad_mode, front.remove_dc, front.preemphasis, front.gain) == (0, 0, 0, 0, 0.0, 1.0)
    in_kernel = not default and bool(front.pad_mode == 1 or front.remove_dc or front.preemphasis > 0.0 or front.gain != 1.0)
    return [int(staged), span if staged else 0, (floats if staged else fixed) * 4, blocks, int(in_kernel), weights]


def lib_fnorm(F, B, rows, channels=1):
    """[resident, lds_bytes, blocks] of the library."""
    return lib_route("nvh_fnorm_route", 3, make_fdesc("mean_var", "band", rows=rows, channels=channels, frames=F, bands=B))


def full_fnorm(F, B, rows, channels=1):
    D = defines("fnorm_dev.h")
    resident, blocks, _ = fnorm_route(F, B, rows * channels)
    data = (F | 1) * B if resident else max(B * (D["NVH_FNORM_TILE"] + 1), D["NVH_FNORM_TILE"] * (B | 1))
    return [int(resident), (D["NVH_FNORM_FIXED_FLOATS"] + data) * 4, blocks]


def test_the_headers_numbers_are_read():
    from nvorbis_amd import native
    rs, ml, fn = defines("resample_dev.h"), defines("mel_dev.h"), defines("fnorm_dev.h")
    assert rs["NVH_RS_TILE"] == native.RESAMPLE_TILE and ml["NVH_MEL_WAVES"] == native.MEL_FRAMES
    assert fn["NVH_FNORM_DATA_FLOATS"] == native.FNORM_RESIDENT_FLOATS and fn["NVH_FNORM_THREADS"] == 64 * fn["NVH_FNORM_WAVES"]
    assert ml["NVH_MEL_OUT_STRIDE"] == ml["NVH_MEL_MAX_BANDS"] + 1 and rs["NVH_RS_SRC_FLOATS"] > 0 and rs["NVH_RS_TAP_FLOATS"] > 0
    # the routes the kernels' own files name are what the predicates say of them
    assert resample_route(1024, 1, 1, 5, [(0, 3, 5)])[0] is False and resample_route(44100, 16000, 2, 63, [(0, 0, 63)])[0] is True
    assert mel_route((48000, 4096, 4096, 5000, 128)) == (False, [3, 3, 3, 2]) and mel_route((16000, 512, 400, 160, 80)) == (True, [2, 2, 2, 2])
    assert mel_route((22050, 1024, 1024, 256, 64)) == (True, [3, 3, 3])
    for F, B in fnr.KERNEL_SHAPES:
        assert fnorm_route(F, B, 12)[0] == fnr.takes_lds_path(F, B) and not fnorm_route(F, B, 12)[2]
        assert lib_fnorm(F, B, 12) == full_fnorm(F, B, 12)
    # ... and what the library launches for them
    assert lib_resample(1024, 1, 1, 5, 1) == full_resample(1024, 1, 1, 5, 1) and lib_resample(44100, 16000, 2, 63, 1) == full_resample(44100, 16000, 2, 63, 1)
    for cfg in ((48000, 4096, 4096, 5000, 128), (16000, 512, 400, 160, 80), (22050, 1024, 1024, 256, 64)):
        assert lib_mel(cfg) == full_mel(cfg), cfg


# ---------------------------------------------------------------------------------------------------------------------------
# k_resample_rows
# ---------------------------------------------------------------------------------------------------------------------------

L2_PAIRS = [(48000, 6000), (96000, 8000)]  # small tables, a full tile's span beyond NVH_RS_SRC_FLOATS
_RS_CASES = {}


def tile():
    return defines("resample_dev.h")["NVH_RS_TILE"]


def two_tiles_17():
    return 2 * tile() + 17


def rs_case(fi, fo, T):
    if (fi, fo, T) not in _RS_CASES:
        _RS_CASES[(fi, fo, T)] = rsr.kernel_case(fi, fo, T)
    return _RS_CASES[(fi, fo, T)]


@pytest.mark.parametrize("fi,fo", L2_PAIRS)
def test_route_taps_in_lds_source_through_l2(fi, fo):
    """kernel_case's rows at T = 2 tiles + 17: the table is staged, every full tile reads its source through L2, the last tile of 17
    outputs and the second tile of the row with valid = tile + 100 stage theirs -- both source routes inside one launch and inside
    one workgroup's walk.  T = 1: a span of 2 * half, staged."""
    T = two_tiles_17()
    rows = rs_case(fi, fo, T)[0]
    taps, gy, spans = resample_route(fi, fo, 2, T, rows)
    assert taps and gy == 3
    assert lib_resample(fi, fo, 2, T, len(rows)) == full_resample(fi, fo, 2, T, len(rows)) and lib_resample(fi, fo, 2, T, len(rows))[::2] == [1, 3]
    assert [v for _, _, v in rows] == [T, T, 0, tile() + 100, T, T]
    for (_, _, v), per in zip(rows, spans):
        if v == T:
            assert not in_lds(per[0]) and not in_lds(per[1]) and in_lds(per[2]), per
    assert spans[2] == [None] * 3
    assert not in_lds(spans[3][0]) and in_lds(spans[3][1]) and spans[3][2] is None, spans[3]
    taps, gy, spans = resample_route(fi, fo, 2, 1, rs_case(fi, fo, 1)[0])
    assert taps and gy == 1 and all(per[0] is None or per[0] == 2 * rule_plan(fi, fo)[2] for per in spans)
    assert lib_resample(fi, fo, 2, 1, len(spans)) == full_resample(fi, fo, 2, 1, len(spans)) and lib_resample(fi, fo, 2, 1, len(spans))[::2] == [1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, "2 tiles + 17"])
@pytest.mark.parametrize("fi,fo", L2_PAIRS)
def test_taps_in_lds_source_through_l2(gpu_ctx, fi, fo, T):
    """resample_chains<TAPS_LDS, !SRC_LDS>, and the switch between the source routes from tile to tile: test_resample_rows.py's
    kernel test (its rows, strides, formats and sentinels) at 8 : 1 and 12 : 1."""
    T = two_tiles_17() if isinstance(T, str) else T
    rsr.check_kernel_case(gpu_ctx, fi, fo, T, rs_case(fi, fo, T))


def rs_rows_case(fi, fo, T, specs, seed):
    """kernel_case's tuple for rows of one's own: specs [(start, valid, kind)], kind "noise" (quiet), "loud" (a held level above
    the clip), "front" (the origin five samples late: the first reads fall in front of the row) or "impulse".  Every row has its
    whole margin otherwise, and the longest row's last reads fall behind the source."""
    L, M, half, _ = rule_plan(fi, fo)
    rows, need = [], 4
    for start, valid, kind in specs:
        origin = max(0, start * M // L - half + 1) + (5 if kind == "front" else 0)
        rows.append((origin, start, valid))
        if valid:
            need = max(need, (start + valid - 1) * M // L + half + 1 - origin)
    S = need - 3
    X = np.random.default_rng(seed).uniform(-1.2, 1.2, size=(len(rows), 2, S)).astype(np.float32)
    for r, (_, _, kind) in enumerate(specs):
        if kind == "loud":
            X[r, 0, S // 3:] = 1.15
            X[r, 1, : S // 2] = -1.15
        elif kind == "impulse":
            X[r] = 0
            X[r, :, min(S - 1, half + 7)] = 1.0
        else:
            X[r] *= np.float32(0.05)
    R = np.zeros((len(rows), 2, T), np.float32)
    hit = np.zeros((len(rows), 2), bool)
    for r, (origin, start, valid) in enumerate(rows):
        for ch in range(2):
            R[r, ch, :valid], hit[r, ch] = rsr.rule_outputs(X[r, ch], origin, fi, fo, start, valid)
    for a in (X, R, hit):
        a.setflags(write=False)
    return rows, X, R, hit


def boundary_specs(fi, fo):
    """Six rows of three full tiles.  A full tile's span is 2 * half + ((s + 511) M div L - s M div L) at its first output s, one
    of two neighbouring numbers by s mod L: three rows begin on the smaller one, three on the larger, and one of each lies a
    multiple of L behind 2^33."""
    L, M, half, _ = rule_plan(fi, fo)
    span = lambda s: (s + tile() - 1) * M // L - s * M // L + 2 * half
    low = min(span(s) for s in range(L))
    small = [s for s in range(L) if span(s) == low][:3]
    large = [s for s in range(L) if span(s) == low + 1][:3]
    assert len(small) == 3 and len(large) == 3
    far = (2 ** 33 // L + 1) * L
    T = 3 * tile()
    return [(small[0], T, "noise"), (large[0], T, "loud"), (small[1] + far, T, "front"), (large[1] + far, T, "noise"),
            (small[2] + 7 * L, T, "impulse"), (large[2] + 11 * L, T, "noise")]


def boundary_case(fi, fo):
    if (fi, fo) not in _RS_CASES:
        _RS_CASES[(fi, fo)] = rs_rows_case(fi, fo, 3 * tile(), boundary_specs(fi, fo), fi + fo)
    return _RS_CASES[(fi, fo)]


def test_route_span_boundary():
    """(264, 35): full tiles of exactly NVH_RS_SRC_FLOATS samples (staged) and of one more (through L2) in one launch, the table
    staged.  (181, 24): NVH_RS_SRC_FLOATS - 1 and NVH_RS_SRC_FLOATS, every tile staged."""
    budget = defines("resample_dev.h")["NVH_RS_SRC_FLOATS"]
    for (fi, fo), want in (((264, 35), {budget, budget + 1}), ((181, 24), {budget - 1, budget})):
        rows = [(0, s, v) for s, v, _ in boundary_specs(fi, fo)]  # (the origin moves no route)
        taps, gy, spans = resample_route(fi, fo, 2, 3 * tile(), rows)
        assert taps and gy == 3
        assert lib_resample(fi, fo, 2, 3 * tile(), len(rows)) == full_resample(fi, fo, 2, 3 * tile(), len(rows))
        assert lib_resample(fi, fo, 2, 3 * tile(), len(rows))[::2] == [1, 3]
        seen = {s for per in spans for s in per}
        assert seen == want, (fi, fo, seen)
        assert {s for per in spans for s in per[:1]} == want  # ... both already among the rows' first tiles


@pytest.mark.gpu
@pytest.mark.parametrize("fi,fo", [(264, 35), (181, 24)])
def test_span_on_both_sides_of_the_lds_budget(gpu_ctx, fi, fo):
    """Full tiles whose span is the budget, one more and one less: the staged span's last float and the first tile beyond it."""
    case = boundary_case(fi, fo)
    assert case[3].any(axis=1).any() and not case[3].any(axis=1).all()
    rsr.check_kernel_case(gpu_ctx, fi, fo, 3 * tile(), case)


WALK_PAIRS = [(8000, 44100), (44100, 16000)]  # L >= M; down-sampling
WALK_ROWS = 256


def walk_length():
    return 8 * tile() + 17


def walk_specs():
    """Eight distinct rows: valid 0 (twice), inside the first tile, on a tile's end, inside a middle tile (twice) and T (twice)."""
    T = walk_length()
    return [(0, T, "loud"), (2 ** 33, 0, "noise"), (12345, 300, "loud"), (77, 3 * tile(), "front"), (1000, 4 * tile() + 77, "noise"),
            (31, T, "impulse"), (5, 0, "loud"), (2 ** 33 + 9, 6 * tile() + 1, "loud")]


def walk_case(fi, fo):
    if ("walk", fi, fo) not in _RS_CASES:
        _RS_CASES[("walk", fi, fo)] = rs_rows_case(fi, fo, walk_length(), walk_specs(), fi * 3 + fo)
    return _RS_CASES[("walk", fi, fo)]


def walk_rows():
    """Which distinct row every one of the WALK_ROWS rows repeats, and the rows' destination rows (one more than rows: one is nobody's)."""
    rng = np.random.default_rng(99)
    idx = np.concatenate([np.arange(8), rng.integers(0, 8, WALK_ROWS - 8)])
    perm = rng.permutation(WALK_ROWS + 1).astype(np.int32)
    return idx, perm[:WALK_ROWS], int(perm[WALK_ROWS])


@pytest.mark.parametrize("fi,fo", WALK_PAIRS)
def test_route_a_workgroup_walks_several_tiles(fi, fo):
    """256 rows x 2 channels x 9 tiles: gridDim.y = 3, so a workgroup walks tiles y, y + 3, y + 6 -- staged tiles behind staged
    ones, pad-only tiles behind staged ones, workgroups that never stage the table."""
    T = walk_length()
    L, M, half, _ = rule_plan(fi, fo)
    rows = [(0, s, v) for s, v, _ in walk_specs()]
    taps, gy, spans = resample_route(fi, fo, 2, T, [rows[i] for i in walk_rows()[0]])
    tiles = (T + tile() - 1) // tile()
    assert taps and tiles == 9 and gy == 3 and WALK_ROWS * 2 * tiles >= 4096
    assert lib_resample(fi, fo, 2, T, WALK_ROWS) == full_resample(fi, fo, 2, T, WALK_ROWS) and lib_resample(fi, fo, 2, T, WALK_ROWS)[:3] == [1, 9, 3]
    assert all(s is None or in_lds(s) for per in spans for s in per)
    staged = [[s is not None for s in per] for per in spans[:8]]
    assert staged[1] == staged[6] == [False] * 9 and staged[0] == staged[5] == [True] * 9
    assert staged[2] == [True] + [False] * 8 and staged[3] == [True] * 3 + [False] * 6
    assert staged[4] == [True] * 5 + [False] * 4 and staged[7] == [True] * 7 + [False] * 2
    assert (L >= M) == ((fi, fo) == WALK_PAIRS[0])


@pytest.mark.gpu
@pytest.mark.parametrize("fi,fo", WALK_PAIRS)
def test_a_workgroup_walks_several_tiles(gpu_ctx, fi, fo):
    """The tile loop with more than one iteration: every destination row equals the rule (f32 and s16, interleaved and planar, the
    destination rows permuted), zeros behind `valid`, the clip flag per destination row; nobody's row and the tail keep the sentinel."""
    torch = _torch()
    from nvorbis_amd import native
    T = walk_length()
    rows, X, R, hit = walk_case(fi, fo)
    idx, dst_row, nobody = walk_rows()
    N, ND, S = WALK_ROWS, WALK_ROWS + 1, X.shape[2]
    origin, start, valid = ([rows[i][k] for i in idx] for k in range(3))
    want_flags = np.zeros(ND, bool)
    want_flags[dst_row] = hit[idx].any(axis=1)
    assert want_flags.any() and not want_flags[dst_row].all()
    full = X[idx]  # (N, 2, S)
    for layout in ("interleaved", "planar"):
        if layout == "interleaved":
            src = np.ascontiguousarray(full.transpose(0, 2, 1))
            sstr, dstr, dshape = (S * 2, 2, 1), (T * 2, 2, 1), (ND, T, 2)
        else:
            src = np.ascontiguousarray(full.transpose(1, 0, 2))
            sstr, dstr, dshape = (S, 1, N * S), (T, 1, ND * T), (2, ND, T)
        d_src = torch.from_numpy(src).cuda()
        for dt in (np.float32, np.int16):
            sent = rsr.SENT[np.dtype(dt)]
            count = int(np.prod(dshape))
            d_dst = torch.full((count + 64,), float(sent), dtype=torch.float32 if dt == np.float32 else torch.int16, device="cuda")
            d_flags = torch.zeros(ND, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            desc = native.ResampleDesc(in_rate=fi, out_rate=fo, rows=N, channels=2, format=native.PCM_S16 if dt == np.int16 else native.PCM_F32,
                                       length=T, src_length=S, src_row_stride=sstr[0], src_time_stride=sstr[1], src_chan_stride=sstr[2],
                                       dst_row_stride=dstr[0], dst_time_stride=dstr[1], dst_chan_stride=dstr[2])
            gpu_ctx.resample_rows(desc, d_src.data_ptr(), d_dst.data_ptr(), origin, start, valid, dst_row, d_flags.data_ptr())
            gpu_ctx.synchronize()
            got = d_dst.cpu().numpy()
            assert (got[count:] == sent).all(), "written behind the destination"
            got = got[:count].reshape(dshape)
            got = got.transpose(0, 2, 1) if layout == "interleaved" else got.transpose(1, 0, 2)  # (ND, 2, T)
            want = np.full((ND, 2, T), sent, dt)
            want[dst_row] = (R if dt == np.float32 else to_s16(R))[idx]
            bad = sorted({int(d) for d in np.argwhere(np.ascontiguousarray(got).view(np.uint8).reshape(ND, -1)
                                                      != want.view(np.uint8).reshape(ND, -1))[:, 0]})
            assert not bad, (layout, dt, len(bad), [(d, rows[idx[list(dst_row).index(d)]] if d != nobody else "nobody") for d in bad[:4]])
            assert np.array_equal(d_flags.cpu().numpy() != 0, want_flags), (layout, dt)


# ---------------------------------------------------------------------------------------------------------------------------
# k_mel_rows
# ---------------------------------------------------------------------------------------------------------------------------

# (rate, n_fft, win_length, hop, n_mels) -> (staged, the stages per register pass)
MEL_ROUTES = {
    (22050, 2048, 2048, 1024, 128): (False, [3, 3, 3, 1]),  # the tables leave no room for the span: mel_pass<1> unstaged
    (16000, 256, 256, 6000, 40): (False, [2, 2, 2, 1]),     # a long hop: the grouping below 512 points, unstaged
    (8000, 64, 64, 30000, 8): (False, [2, 2, 1]),
    (8000, 128, 128, 32, 20): (True, [2, 2, 2]),            # six stages, no remainder pass, staged ...
    (8000, 128, 100, 20000, 20): (False, [2, 2, 2]),        # ... and unstaged, under a window shorter than the transform
}
_MEL_CASES = {}


@pytest.mark.parametrize("cfg", sorted(MEL_ROUTES))
def test_route_mel(cfg):
    assert mel_route(cfg) == MEL_ROUTES[cfg]
    for frames in (1, 4, 7):  # (the gpu test's)
        got = lib_mel(cfg, rows=6, channels=2, frames=frames)
        assert got == full_mel(cfg, rows=6, channels=2, frames=frames) and bool(got[0]) == MEL_ROUTES[cfg][0], (frames, got)


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [1, 4, 7])
@pytest.mark.parametrize("cfg", sorted(MEL_ROUTES))
def test_mel_unstaged_below_4096_and_six_stages(gpu_ctx, cfg, frames):
    """test_mel_rows.py's kernel test -- its six rows, source strides, destination orders, scales, sentinels and the valid = NULL
    call -- on the configurations of MEL_ROUTES."""
    if (cfg, frames) not in _MEL_CASES:
        _MEL_CASES[(cfg, frames)] = mlr.kernel_case(cfg, frames)
    mlr.check_kernel_case(gpu_ctx, cfg, frames, _MEL_CASES[(cfg, frames)])


# ---------------------------------------------------------------------------------------------------------------------------
# k_fnorm_rows
# ---------------------------------------------------------------------------------------------------------------------------

# (F, B) -> resident.  More frames than NVH_FNORM_THREADS: Walk(tid, F) has d_out = 0 and wraps at every step
LONG_SHAPES = {(513, 3): True, (600, 33): True, (1001, 8): True, (1001, 24): False, (1001, 80): False}
_FN_CASES = {}


def long_vf(F):
    return [F, F, 0, 1, 511, 512, min(F, 513)]


def long_case(F, B):
    """test_fnorm_rows.kernel_case with seven rows and the frame counts of long_vf: (X, vf, {(mode, axis): R}, R of rows 3 and 4
    without valid_frames).  Row 1 is a constant; row 4 (vf = 511) has one large value in its last counted frame and a larger one
    behind the counted frames."""
    X = normal_features(F * 1000 + B, (7, 2, F, B))
    X[1] = F32(-8.0)
    vf = long_vf(F)
    X[4, :, 510, B // 2] = F32(90.0)
    X[4, 1, F - 1, 0] = F32(500.0)
    R = {(m, a): rule_fnorm(X, vf, m, a, **fnr.PARAMS) for m in MODES for a in AXES if a == "band" or m in ("mean", "mean_var")}
    for m in (None, "peak"):
        R[(m, "all")] = R[(m, "band")]  # the axis is ignored
    assert not R[("mean", "band")][1].view(np.uint32).any() and R[("peak", "all")][4, 0, :511].max() == F32(F32(94.0) * F32(0.3))
    assert (R[("mean_var", "all")][2] == F32(-7.5)).all()
    R_all = {(m, a): rule_fnorm(X[3:5], None, m, a, **fnr.PARAMS) for m, a in (("mean_var", "band"), ("peak", "band"), ("mean", "all"))}
    X.setflags(write=False)
    for r in list(R.values()) + list(R_all.values()):
        r.setflags(write=False)
    return X, vf, R, R_all


@pytest.mark.parametrize("shape", sorted(LONG_SHAPES))
def test_route_fnorm_more_frames_than_threads(shape):
    F, B = shape
    resident, blocks, wraps = fnorm_route(F, B, 14)
    assert resident == LONG_SHAPES[shape] and blocks == 14 and wraps
    assert lib_fnorm(F, B, 7, 2) == full_fnorm(F, B, 7, 2) and lib_fnorm(F, B, 7, 2)[::2] == [int(resident), 14]
    assert {0, 1, 511, 512, 513, F} <= set(long_vf(F))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(LONG_SHAPES))
def test_fnorm_more_frames_than_threads(gpu_ctx, shape):
    """test_fnorm_rows.py's kernel test -- four modes, both axes, the four source/destination pairings, in place, the gaps' sentinels,
    valid_frames = NULL -- at more than 512 frames, frame counts on both sides of 512."""
    if shape not in _FN_CASES:
        _FN_CASES[shape] = long_case(*shape)
    fnr.check_kernel_case(gpu_ctx, _FN_CASES[shape])


ITEMS_SHAPE = (78, 256)
ITEMS_ROWS = 1025  # x 2 channels


def test_route_fnorm_reread_walks_items():
    F, B = ITEMS_SHAPE
    resident, blocks, _ = fnorm_route(F, B, ITEMS_ROWS * 2)
    assert not resident and blocks < ITEMS_ROWS * 2
    assert fnorm_route(F - 1, B, 1)[0]  # ... the smallest shape of 256 bands that re-reads
    assert lib_fnorm(F, B, ITEMS_ROWS, 2) == full_fnorm(F, B, ITEMS_ROWS, 2) and lib_fnorm(F, B, ITEMS_ROWS, 2)[::2] == [0, blocks]
    assert lib_fnorm(F - 1, B, 1) == full_fnorm(F - 1, B, 1) and lib_fnorm(F - 1, B, 1)[0] == 1


@pytest.mark.gpu
def test_fnorm_reread_walks_items(gpu_ctx):
    """More (row, channel)s than workgroups on the re-reading route: the barrier between a workgroup's items, the partials zeroed
    again, the tile buffer used again.  1025 rows repeat eight distinct ones (their data and their frame count, 0 among them) in
    random order; source and expectation are put together on the device and compared there, bit for bit."""
    torch = _torch()
    F, B = ITEMS_SHAPE
    K, rows = 8, ITEMS_ROWS
    X = normal_features(31, (K, 2, F, B))
    vfs = [F, 0, 1, 63, 64, 65, 40, F - 1]
    rng = np.random.default_rng(32)
    idx = np.concatenate([np.arange(K), rng.integers(0, K, rows - K)])
    d_idx = torch.from_numpy(idx).cuda()
    vf = [vfs[i] for i in idx]
    block, tail = 2 * F * B, 64
    modes = [("mean_var", "band"), ("mean_var", "all"), ("peak", "band")]
    want = {m: rule_fnorm(X, vfs, m[0], m[1], **fnr.PARAMS) for m in modes}
    d_src = {bm: torch.from_numpy(np.ascontiguousarray(X.transpose(0, 1, 3, 2) if bm else X).reshape(K, block)).cuda()[d_idx].reshape(-1)
             for bm in (True, False)}
    for src_bm, dst_bm in ((True, False), (False, False), (False, True)):
        sf, sb = fnr.strides(F, B, src_bm)
        df, db = fnr.strides(F, B, dst_bm)
        for m in modes:
            w = np.ascontiguousarray(want[m].transpose(0, 1, 3, 2) if dst_bm else want[m]).reshape(K, block)
            d_want = torch.from_numpy(w).cuda()[d_idx].reshape(-1)
            d_dst = torch.full((rows * block + tail,), float(fnr.SENT), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            d = make_fdesc(m[0], m[1], rows=rows, channels=2, frames=F, bands=B, eps=fnr.PARAMS["eps"], pad_value=fnr.PARAMS["pad_value"],
                           range=fnr.PARAMS["peak_range"], offset=fnr.PARAMS["peak_offset"], gain=fnr.PARAMS["peak_gain"],
                           src_row_stride=block, src_chan_stride=F * B, src_frame_stride=sf, src_band_stride=sb,
                           dst_row_stride=block, dst_chan_stride=F * B, dst_frame_stride=df, dst_band_stride=db)
            gpu_ctx.fnorm_rows(d, d_src[src_bm].data_ptr(), d_dst.data_ptr(), vf)
            gpu_ctx.synchronize()
            assert bool((d_dst[rows * block:] == float(fnr.SENT)).all()), "written behind the destination"
            same = (d_dst[:rows * block].view(torch.int32) == d_want.view(torch.int32)).reshape(rows, block).all(dim=1)
            bad = torch.nonzero(~same).reshape(-1).cpu().numpy()
            assert not len(bad), (src_bm, dst_bm, m, len(bad), [(int(r), vf[r]) for r in bad[:6]])


# ---------------------------------------------------------------------------------------------------------------------------
# through decode_clip_features
# ---------------------------------------------------------------------------------------------------------------------------

def long_call(n_mels, band_major):
    return (16000, (44100, 48000, 8000), dict(sample_rate=16000),
            dict(n_fft=64, win_length=64, hop=4, n_mels=n_mels, mel_scale="htk", norm=None, scale="ln", band_major=band_major))


def test_route_features_of_1001_frames():
    F = mlr.LENGTH // 4 + 1
    assert F == 1001 and fnorm_route(F, 8, 1) == (True, 1, True) and fnorm_route(F, 24, 1) == (False, 1, True)
    assert mel_route((16000, 64, 64, 4, 8))[0] and mel_route((16000, 64, 64, 4, 24))[0]
    for B in (8, 24):
        assert lib_fnorm(F, B, 3) == full_fnorm(F, B, 3) and lib_fnorm(F, B, 3)[0] == int(B == 8)
        assert lib_mel((16000, 64, 64, 4, B), rows=3, frames=F) == full_mel((16000, 64, 64, 4, B), rows=3, frames=F)


@pytest.mark.gpu
@pytest.mark.parametrize("band_major", [True, False])
@pytest.mark.parametrize("n_mels", [8, 24])
def test_decode_clip_features_of_1001_frames(oracle, gpu_ctx, ogg_bytes, n_mels, band_major):
    """hop = 4 over 4000 samples: 1001 frames per row, normalised in place (8 bands resident, 24 re-reading) with the rows' real
    valid_frames (0, 1001 and between): the features equal oracle PCM -> resampler's rule -> mel rule -> rule_fnorm."""
    _torch()
    import nvorbis_amd as nv
    call = long_call(n_mels, band_major)
    target, rates, extra, mel = call
    files, starts, want, want_valid, want_vf, want_clipped = fnr.expected(oracle, ogg_bytes, "f32", call)
    assert want.shape[2:] == (1001, n_mels)
    want = fnr.shaped(rule_fnorm(want, want_vf, mode="mean_var", axis="band"), mel, "f32")
    (feats, valid, valid_frames), clipped = mlr.feature_call(nv, gpu_ctx, files, starts, dict(extra, normalize="mean_var"), mel, "f32", True, True)
    assert feats.is_cuda and tuple(feats.shape) == want.shape
    assert np.array_equal(valid, want_valid) and np.array_equal(valid_frames, want_vf) and np.array_equal(clipped, want_clipped)
    host = feats.cpu().numpy()
    bad = [i for i in range(len(files)) if not same_bits(np.ascontiguousarray(host[i]), np.ascontiguousarray(want[i]))]
    assert not bad, (n_mels, band_major, bad, int(want_vf[bad[0]]))


# ---------------------------------------------------------------------------------------------------------------------------
# the edges of every threshold of the three route functions, through the exports
# ---------------------------------------------------------------------------------------------------------------------------

def test_route_sweep_resample():
    """rows * channels * tiles on both sides of 4096 (four tiles per workgroup from there on), gridDim.y at its cap, and the tap
    table on both sides of NVH_RS_TAP_FLOATS: L * ((2 * half) | 1) has an odd factor of at least 33, so it is never the budget
    itself (a power of two); 43 * 381 = budget - 1 (508 -> 43) and 1 * 16385 = budget + 1 (512 -> 1) are as close as rates get."""
    T4 = 4 * tile()
    # (in_rate, out_rate, channels, T, rows): the product 4095 keeps a workgroup per tile, 4096 and more gives it four
    edge = [(44100, 16000, 1, 3 * tile(), 1365), (44100, 16000, 1, T4, 1024), (44100, 16000, 3, 5 * tile(), 273), (44100, 16000, 2, 2 * tile(), 1024),
            (8000, 44100, 1, 4095 * tile(), 1), (8000, 44100, 1, 4095 * tile() + 1, 1), (8000, 44100, 1, T4 + 1, 819), (8000, 44100, 1, T4 + 1, 820),
            (8000, 44100, 5, 7 * tile(), 117), (8000, 44100, 5, 7 * tile(), 118)]
    want_gy = [3, 1, 5, 1, 4095, 1024, 5, 2, 7, 2]
    for case, gy in zip(edge, want_gy):
        want = full_resample(*case)
        assert lib_resample(*case) == want and want[2] == gy, (case, want)
    for tiles in (65535 * 4, 65535 * 4 + 1, 1 << 19):  # the cap: (tiles + 3) // 4 = 65535, 65536, 2^17
        case = (44100, 16000, 1, tiles * tile(), 1)
        want = full_resample(*case)
        assert lib_resample(*case) == want and want[1:3] == [tiles, 65535], (case, want)
    budget = defines("resample_dev.h")["NVH_RS_TAP_FLOATS"]
    below, above = (508, 43), (512, 1)
    for (fi, fo), padded in ((below, budget - 1), (above, budget + 1)):
        L, M, half, _ = rule_plan(fi, fo)
        assert L * ((2 * half) | 1) == padded and max(fi, fo) <= 192000
        want = full_resample(fi, fo, 2, 63, 3)
        assert lib_resample(fi, fo, 2, 63, 3) == want and want[0] == int(padded < budget), (fi, fo, want)
    assert full_resample(*below, 1, 1, 1)[3] - full_resample(*above, 1, 1, 1)[3] == 4 * (budget - 1)


def test_route_sweep_mel():
    """The work items on both sides of 16384 (four items per workgroup from there on) and at the cap of 2^20 workgroups; for two
    transforms the longest hop whose span is still staged, and the next; every field of a front on its own."""
    from tests.test_mel_front_plan import front_tables, make_front
    cfg = (16000, 512, 400, 160, 80)
    waves = defines("mel_dev.h")["NVH_MEL_WAVES"]
    for shape, blocks in (((16383, 1, waves), 16383), ((16384, 1, waves), 4096), ((16383, 1, waves + 1), 8192), ((1, 1, 16383 * waves), 16383),
                          ((1, 1, 16383 * waves + 1), 4096), ((5461, 3, 1), 16383), ((8192, 2, 2), 4096), ((16385, 1, 1), 4097),
                          (((4 << 20) - 3, 1, 1), 1 << 20), (((4 << 20) + 5, 1, 1), 1 << 20), (((4 << 20) - 4, 1, 1), (1 << 20) - 1)):
        want = full_mel(cfg, *shape)
        assert lib_mel(cfg, *shape) == want and want[3] == blocks, (shape, want)
    budget = defines("mel_dev.h")["NVH_MEL_LDS_BYTES"]
    for rate, N, B in ((16000, 512, 80), (22050, 2048, 128)):
        # a hop longer by one is a span longer by waves - 1 floats, a window longer by one is two floats more: one of three
        # neighbouring windows lets the longest staged hop meet the budget to the byte
        W = next(w for w in (N, N - 1, N - 2) if (budget - full_mel((rate, N, w, 1, B))[2]) % (4 * (waves - 1)) == 0)
        at_one = full_mel((rate, N, W, 1, B))
        assert at_one[0] == 1
        last = 1 + (budget - at_one[2]) // (4 * (waves - 1))
        assert 2 < last < 65536
        for H, staged in ((last - 1, 1), (last, 1), (last + 1, 0)):
            want = full_mel((rate, N, W, H, B), 6, 2, 7)
            assert lib_mel((rate, N, W, H, B), 6, 2, 7) == want and want[0] == staged and (want[1] > 0) == bool(staged), (N, H, want)
            assert want[2] == budget - 4 * (waves - 1) * (last - H) if staged else want[2] < at_one[2]
    # a front: the window and the triangles change tables alone, everything else is the kernel's
    assert lib_mel(cfg, front=make_front()) == full_mel(cfg, front=make_front()) == lib_mel(cfg) and lib_mel(cfg)[4] == 0
    for kw, in_kernel in ((dict(window="povey"), 0), (dict(window="rectangular"), 0), (dict(reflect=True), 1), (dict(remove_dc=True), 1),
                          (dict(preemphasis=0.97), 1), (dict(gain=32768.0), 1), (dict(gain=0.5), 1), (dict(window="hamming", remove_dc=True), 1)):
        want = full_mel(cfg, front=make_front(**kw))
        assert lib_mel(cfg, front=make_front(**kw)) == want and want[4] == in_kernel, (kw, want)
    got = lib_mel(cfg, front=make_front(triangles="mel"))  # (a bank of its own: its size is the front's tables')
    rate, N, W, H, B = cfg
    assert got[4] == 0 and got[5] == sparse_weights(front_tables(rate, N, W, B, triangles="mel")[2]) != lib_mel(cfg)[5]
    assert got[:2] == [1, (waves - 1) * H + W] and got[2] - lib_mel(cfg)[2] == 4 * (got[5] - lib_mel(cfg)[5]) and got[3] == 1


def test_route_sweep_fnorm():
    """(F | 1) * B on both sides of NVH_FNORM_DATA_FLOATS = 19952 = 1247 * 16, and the work items on both sides of the 2048
    workgroups of a launch."""
    budget = defines("fnorm_dev.h")["NVH_FNORM_DATA_FLOATS"]
    for (F, B), resident in (((1246, 16), 1), ((1247, 16), 1), ((1248, 16), 0), ((1245, 16), 1), ((77, 256), 1), ((78, 256), 0),
                             ((19951, 1), 1), ((19952, 1), 0), ((1, 256), 1), ((1 << 24, 1), 0)):
        assert ((F | 1) * B <= budget) == bool(resident)
        for rows, channels in ((1, 1), (2048, 1), (2049, 1), (1024, 2), (683, 3), (5, 65535)):
            want = full_fnorm(F, B, rows, channels)
            assert lib_fnorm(F, B, rows, channels) == want and want[0] == resident and want[2] == min(rows * channels, 2048), (F, B, rows, want)
    assert full_fnorm(1247, 16, 1)[1] == 4 * (528 + budget) == defines("fnorm_dev.h")["NVH_FNORM_LDS_BYTES"]


def test_routes_return_the_rows_calls_argument_errors():
    """The exports run the rows calls' own checks on the descriptor: a bad descriptor is the same error, without a context."""
    from nvorbis_amd import native
    from tests.test_mel_front_plan import make_front
    from tests.test_mel_plan import make_desc
    lib, out = native.lib(), (C.c_int64 * 6)()
    no_ctx = lambda rc: native.ERR_NO_GPU if rc == native.OK else rc  # (what the rows call answers without a context)
    rs = lambda **kw: native.ResampleDesc(**dict(dict(in_rate=44100, out_rate=16000, rows=2, channels=1, format=native.PCM_F32, length=9), **kw))
    for d, rc in ((rs(channels=0), native.ERR_ARGUMENT), (rs(format=7), native.ERR_ARGUMENT), (rs(length=(1 << 48) + 1), native.ERR_ARGUMENT),
                  (rs(in_rate=1, out_rate=4097), native.ERR_UNSUPPORTED), (rs(), native.OK), (rs(rows=0), native.OK)):
        z = [(C.c_int64 * 2)() for _ in range(3)]
        assert lib.nvh_resample_route(C.byref(d), out) == rc and lib.nvh_resample_rows(None, C.byref(d), 8, 8, z[0], z[1], z[2], None, None) == no_ctx(rc)
    assert lib.nvh_resample_route(None, out) == lib.nvh_resample_route(C.byref(rs()), None) == native.ERR_ARGUMENT
    for d, f, rc in ((make_desc(n_fft=100), None, native.ERR_ARGUMENT), (make_desc(rows=1, channels=0, frames=1), None, native.ERR_ARGUMENT),
                     (make_desc(rows=1, channels=1, frames=1), make_front(gain=0.0), native.ERR_ARGUMENT),
                     (make_desc(rows=1, channels=1, frames=1, src_length=1), make_front(reflect=True), native.ERR_ARGUMENT),
                     (make_desc(rows=1 << 30, channels=65535, frames=1 << 40), None, native.ERR_ARGUMENT),
                     (make_desc(rows=1, channels=1, frames=1), None, native.OK)):
        fp = None if f is None else C.byref(f)
        assert lib.nvh_mel_route(C.byref(d), fp, out) == rc and lib.nvh_mel_rows_front(None, C.byref(d), fp, 8, 8, None) == no_ctx(rc)
    assert lib.nvh_mel_route(None, None, out) == lib.nvh_mel_route(C.byref(make_desc()), None, None) == native.ERR_ARGUMENT
    for d, rc in ((make_fdesc("mean", bands=0), native.ERR_ARGUMENT), (make_fdesc(7), native.ERR_ARGUMENT),
                  (make_fdesc("mean_var", eps=0.0), native.ERR_ARGUMENT), (make_fdesc("peak", rows=3, frames=4, bands=2), native.OK)):
        assert lib.nvh_fnorm_route(C.byref(d), out) == rc and lib.nvh_fnorm_rows(None, C.byref(d), 8, 8, None) == no_ctx(rc)
    assert lib.nvh_fnorm_route(None, out) == lib.nvh_fnorm_route(C.byref(make_fdesc()), None) == native.ERR_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------------
# the per-row block (nvh_internal.h: RowBlock) of the three calls: three calls queued with no wait between them, of 3, 700 and 5
# rows.  700 rows outgrow the block's first size class, so the second call gives the image and the device copy back and takes
# larger ones while the first call's work may still be in flight, and the third writes its image behind the second's copy.  A
# context of its own: the block starts empty.  Every call has its own per-row arrays, source and destination; the 700 rows repeat
# eight distinct ones, so that the reference is eight rows of the kernels' numpy rules.
# ---------------------------------------------------------------------------------------------------------------------------

BLOCK_CALLS = (3, 700, 5)


def block_calls():
    """Per call, which of eight distinct rows every row repeats: [0, 1, 2], 700 at random (every one among them), [7, 3, 5, 4, 6]."""
    rng = np.random.default_rng(700)
    idx = [np.arange(3), np.concatenate([np.arange(8), rng.integers(0, 8, 692)]), np.array([7, 3, 5, 4, 6])]
    assert tuple(len(i) for i in idx) == BLOCK_CALLS
    return idx


def run_block_calls(launch, X, R, sent=fnr.SENT):
    """launch(ctx, rows, d_src, d_dst, idx) queues one call; X[k] the distinct rows' sources, R[k] their expected outputs (float32).
    The three calls back to back, one wait, every destination compared bit for bit and its tail for the sentinel."""
    torch = _torch()
    import nvorbis_amd as nv
    ctx = nv.Context(0)
    try:
        idx = block_calls()
        per = int(np.prod(R.shape[1:]))
        src = [torch.from_numpy(np.ascontiguousarray(X[i])).cuda() for i in idx]
        dst = [torch.full((len(i) * per + 64,), float(sent), dtype=torch.float32, device="cuda") for i in idx]
        torch.cuda.synchronize()
        for i, s, d in zip(idx, src, dst):
            launch(ctx, len(i), s.data_ptr(), d.data_ptr(), i)
        ctx.synchronize()
        for call, (i, d) in enumerate(zip(idx, dst)):
            got = d.cpu().numpy()
            assert (got[len(i) * per:] == sent).all(), (call, "written behind the destination")
            want = np.ascontiguousarray(R[i]).reshape(len(i), per)
            bad = np.argwhere((got[:len(i) * per].reshape(len(i), per).view(np.uint32) != want.view(np.uint32)).any(axis=1))[:, 0]
            assert not len(bad), (call, len(bad), [(int(r), int(i[r])) for r in bad[:6]])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_row_block_resample():
    from nvorbis_amd import native
    fi, fo, T, S = 3, 2, 40, 110
    L, M, half, _ = rule_plan(fi, fo)
    rows = []
    for start, valid in ((0, T), (1, T), (2 ** 33 + 1, 17), (5, 0), (77, 1), (2 ** 20, T - 1), (3, T), (40, 23)):
        origin = max(0, start * M // L - half + 1)
        assert not valid or (start + valid - 1) * M // L + half + 1 - origin <= S
        rows.append((origin, start, valid))
    X = (np.random.default_rng(40).uniform(-1.2, 1.2, size=(8, S)) * 0.05).astype(np.float32)
    R = np.zeros((8, T), np.float32)  # (zeros behind `valid`)
    for k, (origin, start, valid) in enumerate(rows):
        R[k, :valid] = rsr.rule_outputs(X[k], origin, fi, fo, start, valid)[0]

    def launch(ctx, n, d_src, d_dst, idx):
        desc = native.ResampleDesc(in_rate=fi, out_rate=fo, rows=n, channels=1, format=native.PCM_F32, length=T, src_length=S, src_row_stride=S,
                                   src_time_stride=1, src_chan_stride=0, dst_row_stride=T, dst_time_stride=1, dst_chan_stride=0)
        ctx.resample_rows(desc, d_src, d_dst, *([rows[k][j] for k in idx] for j in range(3)))

    run_block_calls(launch, X, R)


@pytest.mark.gpu
def test_row_block_mel():
    from tests.test_mel_plan import make_desc, rule_frames, rule_mel, rule_power, rule_scale
    rate, N, W, H, B, frames = 8000, 64, 64, 16, 8, 3
    S = (frames - 1) * H + W
    tw, win, fb = lib_tables(rate, N, W, B)
    valid = [S, 0, 50, S - 1, 1, 64, 33, S]
    X = np.random.default_rng(64).uniform(-1, 1, (8, S)).astype(np.float32)
    u = np.concatenate([rule_frames(X[k], valid[k], 0, frames, N, W, H, win) for k in range(8)])
    R = rule_scale(rule_mel(rule_power(u, tw), fb).reshape(8, frames, B), "ln", 1e-10)

    def launch(ctx, n, d_src, d_dst, idx):
        desc = make_desc(rate, N, W, B, hop=H, scale="ln", rows=n, channels=1, frames=frames, first=0, src_length=S, src_row_stride=S,
                         src_time_stride=1, src_chan_stride=0, dst_row_stride=frames * B, dst_chan_stride=0, dst_frame_stride=B, dst_band_stride=1)
        ctx.mel_rows(desc, d_src, d_dst, [valid[k] for k in idx])

    run_block_calls(launch, X, R)


@pytest.mark.gpu
def test_row_block_fnorm():
    F, B = 5, 3
    vf = [5, 0, 1, 4, 2, 5, 3, 1]
    X = normal_features(53, (8, 1, F, B))
    R = rule_fnorm(X, vf, "mean_var", "band", **fnr.PARAMS)

    def launch(ctx, n, d_src, d_dst, idx):
        P = fnr.PARAMS
        desc = make_fdesc("mean_var", "band", rows=n, channels=1, frames=F, bands=B, eps=P["eps"], pad_value=P["pad_value"], range=P["peak_range"],
                          offset=P["peak_offset"], gain=P["peak_gain"], src_row_stride=F * B, src_chan_stride=0, src_frame_stride=B, src_band_stride=1,
                          dst_row_stride=F * B, dst_chan_stride=0, dst_frame_stride=B, dst_band_stride=1)
        ctx.fnorm_rows(desc, d_src, d_dst, [vf[k] for k in idx])

    run_block_calls(launch, X, R)

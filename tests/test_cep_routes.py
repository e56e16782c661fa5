"""The launch routes of nvh_cep_rows: a Python restatement of the route from the stated geometry (include/nvorbis_hip.h,
nvorbis_amd/csrc/cep_dev.h: the numbers are read from the header, the functions restated) against nvh_cep_route on both sides of
every threshold -- the LDS budget to the byte, the grid cap, the tile count -- and, on the GPU, one case held to each route, a
workgroup that walks several items, and three calls queued back to back through the per-row block."""
import ctypes as C

import numpy as np
import pytest

from tests.test_cep_plan import F32, make_cdesc, normal_features, rule_cep, rule_tables
from tests.test_cep_rows import SENT
from tests.test_clip_batches import _torch
from tests.test_row_routes import defines, lib_route, run_block_calls


def cep_route(dct, B, K, o, N, items):
    """nvh_cep_rows' launch: (table staged in LDS, bytes of dynamic LDS, workgroups).  A work item stages tile + 2 o N frames of
    B | 1 floats and, with a transform, their K | 1 cepstra behind 64 floats of delta scales; the table is B rows of K rounded up to
    whole blocks, staged where it fits the budget beside them."""
    D = defines("cep_dev.h")
    slots = D["NVH_CEP_TILE"] + 2 * o * N
    block = D["NVH_CEP_KBLOCK"]
    tile = D["NVH_CEP_SCALE_FLOATS"] + slots * ((B | 1) + ((K | 1) if dct else 0))
    table = B * ((K + block - 1) // block * block) if dct else 0
    staged = dct and (tile + table) * 4 <= D["NVH_CEP_LDS_BYTES"]
    return int(bool(staged)), (tile + (table if staged else 0)) * 4, min(items, D["NVH_CEP_MAX_BLOCKS"])


def lib_cep(dct, B, K, o, N, rows=1, channels=1, frames=1):
    return lib_route("nvh_cep_route", 4, make_cdesc(transform=dct, bands=B, ceps=K, order=o, window=N, rows=rows, channels=channels, frames=frames))


def test_the_headers_numbers_are_read():
    D = defines("cep_dev.h")
    from nvorbis_amd import native
    assert D["NVH_CEP_TILE"] == native.CEP_FRAMES == 24 and D["NVH_CEP_THREADS"] == 256 and D["NVH_CEP_LDS_BYTES"] == 81920
    assert D["NVH_CEP_WINDOW_MAX"] == native.CEP_MAX_WINDOW == 8 and D["NVH_CEP_KBLOCK"] == 4 and D["NVH_CEP_SCALE_FLOATS"] == 64
    header = open(__file__.replace("tests/test_cep_routes.py", "include/nvorbis_hip.h")).read()
    assert "#define NVH_CEP_FRAMES 24\n" in header and "#define NVH_CEP_MAX_WINDOW 8\n" in header


def test_route_sweep():
    """Every (o, N), every fifth B and every K that is a limit, a block edge or one of a spread: the export equals the restatement,
    no launch is beyond the budget, and without a transform no table is staged."""
    budget = defines("cep_dev.h")["NVH_CEP_LDS_BYTES"]
    seen = set()
    for o in (0, 1, 2):
        for N in range(1, 9):
            for B in sorted(set(range(1, 257, 5)) | {255, 256}):
                kmax = min(B, 256 // (1 + o))
                for K in sorted(set([1, 2, 3, 4, 5, kmax - 1, kmax] + list(range(7, kmax, 11))) & set(range(1, kmax + 1))):
                    want = cep_route(1, B, K, o, N, 1)
                    assert lib_cep(1, B, K, o, N)[:3] == list(want), (B, K, o, N)
                    assert want[1] <= budget
                    seen.add(want[0])
                if (1 + o) * B <= 256:
                    want = cep_route(0, B, B, o, N, 1)
                    assert want[0] == 0 and lib_cep(0, B, B, o, N)[:3] == list(want), (B, o, N)
    assert seen == {0, 1}


def test_route_lds_budget_to_the_byte():
    """Over every valid (B, K, o, N): the parameter sets whose tile and table come closest to the budget from below and from above
    (and one that meets it exactly, if there is one) take the staged and the unstaged route; and along K at fixed (B, o, N) the
    route flips once, from staged to unstaged, where the restated bytes cross the budget."""
    D = defines("cep_dev.h")
    budget = D["NVH_CEP_LDS_BYTES"]
    B, K = np.meshgrid(np.arange(1, 257), np.arange(1, 257), indexing="ij")
    best = {}
    for o in (0, 1, 2):
        for N in range(1, 9):
            slots = D["NVH_CEP_TILE"] + 2 * o * N
            total = 4 * (D["NVH_CEP_SCALE_FLOATS"] + slots * ((B | 1) + (K | 1)) + B * ((K + 3) // 4 * 4))
            ok = (K <= B) & ((1 + o) * K <= 256)
            for side, pick in (("under", np.where(ok & (total <= budget), total, -1)), ("over", np.where(ok & (total > budget), -total, -10 ** 9))):
                i = np.unravel_index(np.argmax(pick), pick.shape)
                cand = (int(abs(pick[i])), int(B[i]), int(K[i]), o, N)
                if side not in best or abs(cand[0] - budget) < abs(best[side][0] - budget):
                    best[side] = cand
    for side, (total, b, k, o, N) in best.items():
        got = lib_cep(1, b, k, o, N)
        print("closest %s the budget: %d bytes at B=%d K=%d o=%d N=%d" % (side, total, b, k, o, N))
        assert got[0] == (side == "under") and got[:3] == list(cep_route(1, b, k, o, N, 1))
        assert got[1] == total if side == "under" else got[1] < total
    assert best["under"][0] <= budget < best["over"][0]
    for b, o, N in ((128, 1, 2), (80, 2, 2), (256, 0, 1), (200, 2, 8)):
        flips = [lib_cep(1, b, k, o, N)[0] for k in range(1, min(b, 256 // (1 + o)) + 1)]
        first_out = flips.index(0) + 1 if 0 in flips else None
        assert flips == sorted(flips, reverse=True)
        if first_out:
            assert cep_route(1, b, first_out - 1, o, N, 1)[0] == 1 and cep_route(1, b, first_out, o, N, 1)[0] == 0
    assert lib_cep(1, 128, 105, 1, 2)[0] == 1 and lib_cep(1, 128, 106, 1, 2)[0] == 0  # (tests/test_cep_rows.py runs both)


def test_route_grid_cap_and_work_items():
    """Work items are rows * channels * tiles, tiles = ceil(F / tile); a launch has min(items, cap) workgroups."""
    D = defines("cep_dev.h")
    cap, tile = D["NVH_CEP_MAX_BLOCKS"], D["NVH_CEP_TILE"]
    for rows, channels, frames in ((cap - 1, 1, 1), (cap, 1, tile), (cap + 1, 1, 1), (1, 1, tile * cap), (1, 1, tile * cap + 1), (1, 1, tile * cap - tile),
                                   (683, 3, 1), (683, 3, tile + 1), (1, 1, tile - 1), (1, 1, tile), (1, 1, tile + 1), (5, 2, 2 * tile + 1),
                                   (0, 1, 5), (5, 1, 0), (3, 65535, 1 << 24)):
        tiles = -(-frames // tile)
        items = rows * channels * tiles if rows and frames else 0
        got = lib_cep(1, 23, 13, 2, 2, rows, channels, frames)
        assert got[2] == min(items, cap) and got[3] == tiles, (rows, channels, frames, got)
    from nvorbis_amd import native
    out = (C.c_int64 * 4)()
    d = make_cdesc(rows=(1 << 31) - 1, channels=65535, frames=1 << 24)  # 2^31 * 2^16 * 2^19.5 items: beyond 64 bits
    assert native.lib().nvh_cep_route(C.byref(d), out) == native.ERR_ARGUMENT
    d = make_cdesc(rows=(1 << 31) - 1, channels=65535, frames=24 * 65536)  # 2^63 - a little
    assert native.lib().nvh_cep_route(C.byref(d), out) == native.OK and out[2] == cap


# ---------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------

def run_plain(ctx, x, vf, dct, K, o, N, norm, lifter, band_major_out):
    """One call over x (rows, 1, F, B) frame-major in a buffer of its own: the output (rows, 1, F, Q) and the route."""
    torch = _torch()
    rows, _, F, B = x.shape
    Q = (1 + o) * K
    d_src = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()
    d_dst = torch.full((rows * F * Q + 64,), float(SENT), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    d = make_cdesc(transform=dct, dct_norm=0 if norm == "ortho" else 1, bands=B, ceps=K, order=o, window=N, lifter=lifter, rows=rows, channels=1,
                   frames=F, src_row_stride=F * B, src_frame_stride=B, src_band_stride=1, dst_row_stride=F * Q,
                   dst_frame_stride=1 if band_major_out else Q, dst_col_stride=F if band_major_out else 1)
    route = lib_route("nvh_cep_route", 4, d)
    ctx.cep_rows(d, d_src.data_ptr(), d_dst.data_ptr(), vf)
    ctx.synchronize()
    got = d_dst.cpu().numpy()
    assert (got[rows * F * Q:] == SENT).all(), "written behind the destination"
    got = got[:rows * F * Q]
    return (got.reshape(rows, 1, Q, F).transpose(0, 1, 3, 2) if band_major_out else got.reshape(rows, 1, F, Q)), route


@pytest.mark.gpu
@pytest.mark.parametrize("name,dct,B,K,o,N", [("staged", 1, 64, 31, 2, 3), ("through the caches", 1, 250, 70, 2, 3), ("no table", 0, 64, 64, 2, 3)])
def test_each_route(gpu_ctx, name, dct, B, K, o, N):
    F = 53
    want_route = cep_route(dct, B, K, o, N, 3 * 3)
    assert want_route[0] == (name == "staged")
    x = normal_features(B + K, (3, 1, F, B))
    vf = [F, 29, 3]
    want = rule_cep(x, vf, rule_tables(B, K if dct else None, "ortho", 22.0, N), o, N)
    for bm in (False, True):
        got, route = run_plain(gpu_ctx, x, vf, dct, K, o, N, "ortho", 22.0, bm)
        assert route[:3] == list(want_route) and route[3] == 3
        assert (np.ascontiguousarray(got).view(np.uint32) == want.view(np.uint32)).all(), (name, bm)


@pytest.mark.gpu
def test_a_workgroup_walks_several_items(gpu_ctx):
    """1100 rows of 49 frames: 3300 work items on 2048 workgroups, so most workgroups take a second item -- another row's tile, with
    another vf -- after their first; the table and the scales are staged once."""
    rows, F, B, K, o, N = 1100, 49, 8, 5, 2, 2
    assert cep_route(1, B, K, o, N, rows * 3) == (1, cep_route(1, B, K, o, N, 1)[1], defines("cep_dev.h")["NVH_CEP_MAX_BLOCKS"])
    x = normal_features(49, (rows, 1, F, B))
    vf = np.random.default_rng(50).integers(0, F + 1, rows)
    want = rule_cep(x, vf, rule_tables(B, K, None, 0.0, N), o, N)
    got, route = run_plain(gpu_ctx, x, vf, 1, K, o, N, None, 0.0, False)
    assert route == [1, cep_route(1, B, K, o, N, 1)[1], 2048, 3]
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=(1, 2, 3)))[:, 0]
    assert not len(bad), (len(bad), bad[:6].tolist())


@pytest.mark.gpu
def test_row_block_cep():
    """Three calls of 3, 700 and 5 rows queued with no wait between them on a context of its own (tests/test_row_routes.py:
    run_block_calls): the per-row block of the cepstral stage grows under the second and is written again under the third."""
    F, B, K, o, N = 7, 6, 4, 2, 1
    vf = [7, 0, 1, 4, 2, 7, 3, 5]
    X = normal_features(76, (8, 1, F, B))
    R = rule_cep(X, vf, rule_tables(B, K, "ortho", 22.0, N), o, N)
    Q = (1 + o) * K

    def launch(ctx, n, d_src, d_dst, idx):
        d = make_cdesc(bands=B, ceps=K, order=o, window=N, lifter=22.0, rows=n, channels=1, frames=F, src_row_stride=F * B, src_frame_stride=B,
                       src_band_stride=1, dst_row_stride=F * Q, dst_frame_stride=Q, dst_col_stride=1)
        ctx.cep_rows(d, d_src, d_dst, [vf[k] for k in idx])

    run_block_calls(launch, X, R, SENT)

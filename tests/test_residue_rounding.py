"""Residue sums that round: the order of additions of every residue walk, pinned.

Every kernel that accumulates residue vectors -- residue_walk, residue_walk_two and the lean body of synth_group_steady, the stage
and partition tie-break of residue_walk_bins, residue_walk_general (kernels_synth.hip), the global-memory k_residue family
(kernels.hip), the wide k_synth8* forms -- promises the reference's additions in the reference's order: cascade stage by stage,
inside a stage the lower partition first (Residue0.cs:132-175).  On config()'s books that promise cannot fail: the values are dyadic
with a few mantissa bits, every partial sum is exact, and most classes have at most two stages.  The setups of
tests/synth_stream.py: rounding() have three stages in every class and value books with full 21-bit mantissas at scales up to 2^15
apart; their streams come from the structured full-depth encoder (tests/vorbis_encode.py), since random bits almost never reach
the third stage.

CPU: the Python slab walker of tests/test_host_slabs.py in the reference's order equals the oracle bit for bit; the oracle's
residue has no non-finite and no subnormal element (both are out of scope here); and the walker in a WRONG order -- stages
reversed, the partition tie reversed, chain-major -- differs from it in many elements.  The last are conditions on the streams,
met by the reference alone: a kernel that added in one of those orders could not pass the GPU tests below.  Quirk B-13
(sequence_p accumulated in double, then cast) is pinned through the oracle's codebook tables (orc_codebook_tables), which the
library's tables equal bit for bit and whose values are found, whole, in the lattice and VQ pools the kernels gather from.

GPU: uint32-exact against oracle.decode_packets, clip on and off, batch_frames 1024 and 5, the host parser and -- where it takes the
stream -- the GPU parser, with the kernels that ran asserted; replayed under the toggles that pick another walk."""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

from tests import synth_stream as ss, vorbis_encode as ve
from tests.test_host_slabs import REFERENCE_ORDER, _slab_residue_sums, slab_frames

KINDS = (1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1)
SEED = 9
# res2_alias_stereo's partitions share a bin in short blocks only, one element per two partitions: mostly short blocks
KINDS_OF = {"res2_alias_stereo": (1,) + (0,) * 40 + (1,)}

STAGES_REVERSED = lambda w: (w[0], -w[1], w[2])
TIE_REVERSED = lambda w: (w[0], w[1], -w[2])
CHAIN_MAJOR = lambda w: (w[0], w[2], w[1])

# partitions of one stage that add into the same element (quirk B-1, vector overrun): the partition tie-break matters
ALIASING = ("three_ch_res2_misaligned", "table_books_b1", "equal_blocks_overrun", "res2_alias_stereo")
# every setup of the GPU tests below that the host parser writes slabs for (up to eight channels); ch9_res2 and ch16_res1_4096
# have none, their streams rest on the same recipe
SLAB_SETUPS = ("stereo_res1_coupled", "mono_res1_2048", "grid_2ch_256_2048", "grid_2ch_256_1024", "three_ch_res2_misaligned",
               "table_books_b1", "res0_slab", "odd_dims_slab", "res2_alias_stereo", "two_pass_slab", "equal_blocks_overrun",
               "table_books_general", "table_books_pair", "ch5_res2", "six_ch_res2_4096", "res0_3ch", "mono_res0_small_blocks")
NO_SLABS = ("ch9_res2", "ch16_res1_4096")
MIN_STAGE_SHARE = 0.10  # of the non-zero elements, stage order reversed
MIN_TIE_CHANGES = 50    # elements, partition tie reversed and chain-major each (aliasing setups)


@functools.lru_cache(maxsize=None)
def headers(name):
    return tuple(ss.make_stream(ss.rounding(name), 0, 1)[0][:3])


@functools.lru_cache(maxsize=None)
def stream(name, kinds=None, seed=SEED):
    """(packets, granules, flags) of a rounding setup's structured full-depth stream."""
    hdr = list(headers(name))
    pk, gr = ve.encode_stream(ve.setup_of(hdr), hdr, list(kinds or KINDS_OF.get(name, KINDS)), seed)
    return tuple(pk), tuple(gr), (0,) * len(pk)


def _changed(a, b):
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


@functools.lru_cache(maxsize=None)
def measure(name):
    """The stream of `name` through the slab walker in the reference's order and in the wrong ones, against the oracle."""
    from tests import oracle_py
    oracle = oracle_py.load()
    pk = stream(name)[0]
    m = dict(frames=0, nonzero=0, mismatch=0, bad_values=0, stages=0, tie=0, chain=0, vectors=0, third=0)
    for i, words, h, want, lat, vq in slab_frames(oracle, pk, range(3, len(pk))):
        nch, half = want.shape
        got = _slab_residue_sums(words, h, lat, nch, half, vq, REFERENCE_ORDER)
        m["frames"] += 1
        m["vectors"] += h["nrec"]
        recs = words[h["off_rec"] * 4:][:2 * h["nrec"]].reshape(h["nrec"], 2)
        m["third"] += int(np.count_nonzero(((recs[:, 1] >> 28) & 7) == 2))
        m["mismatch"] += _changed(got, want)
        mag = np.abs(want[want != 0])
        m["bad_values"] += int(np.count_nonzero(~np.isfinite(want))) + int(np.count_nonzero(mag < np.finfo(np.float32).tiny))
        m["nonzero"] += int(np.count_nonzero(want))
        m["stages"] += _changed(_slab_residue_sums(words, h, lat, nch, half, vq, STAGES_REVERSED), want)
        if name in ALIASING:
            m["tie"] += _changed(_slab_residue_sums(words, h, lat, nch, half, vq, TIE_REVERSED), want)
            m["chain"] += _changed(_slab_residue_sums(words, h, lat, nch, half, vq, CHAIN_MAJOR), want)
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_rounding_setups_stay_out_of_the_config_list():
    """rounding() derives: three stages per class, the residue's own books in turn, full-width values on the residue's value
    books and nowhere else -- and adds no name to the lists other tests are parametrised over."""
    assert not any("round" in n for n in ss.CONFIG_NAMES + ss.GRID_NAMES)
    for name in SLAB_SETUPS + NO_SLABS:
        base, cfg = ss.config(name), ss.rounding(name)
        assert len(cfg["books"]) == len(base["books"])
        used = set()
        for r0, r1 in zip(base["residues"], cfg["residues"]):
            a0, a1 = ss._residue_args(r0), ss._residue_args(r1)
            assert a1[:5] == a0[:5] and a1[5] == [7] * len(a0[5]), name
            assert a1[6] == [a0[6][i % len(a0[6])] for i in range(3 * len(a0[5]))], name
            used.update(a1[6])
        for i, (b0, b1) in enumerate(zip(base["books"], cfg["books"])):
            assert (b1.bits, b1.dims, b1.lookup, b1.value_bits, b1.sequence_p, b1.mults) == \
                   (b0.bits, b0.dims, b0.lookup, b0.value_bits, b0.sequence_p, b0.mults), (name, i)
            if i in used and b0.lookup and i != ss.FLOOR0_LSP_BOOK:
                assert b1.min_me == (-(0x155555 ^ (i * 0x1357)), -21 - 5 * (i % 4)) and -b1.min_me[0] >= 1 << 20, (name, i)
                assert b1.delta_me == (0x1C71C7 ^ (i * 0x2461), -22 - 5 * (i % 4)) and b1.delta_me[0] >= 1 << 20, (name, i)
            else:
                assert (b1.min_me, b1.delta_me) == (b0.min_me, b0.delta_me), (name, i)


@pytest.mark.parametrize("name", SLAB_SETUPS)
def test_reference_order_equals_the_oracle(name):
    """The slabs of the rounding stream, walked in the reference's order: the oracle's IResidue.Decode bit for bit on every
    frame; every frame decodes, and a third of the vector writes are third stages."""
    m = measure(name)
    assert m["frames"] == len(KINDS_OF.get(name, KINDS)) and m["vectors"] > 100, m
    assert m["third"] * 3 == m["vectors"], m
    assert m["mismatch"] == 0, m


@pytest.mark.parametrize("name", SLAB_SETUPS)
def test_no_nonfinite_or_subnormal_residue(name):
    """Denormal and overflowing books are out of scope: no element of the oracle's residue is non-finite or subnormal."""
    m = measure(name)
    assert m["nonzero"] > 0 and m["bad_values"] == 0, m


@pytest.mark.parametrize("name", SLAB_SETUPS)
def test_the_stream_discriminates(name):
    """Conditions on the input, met by the reference alone: with the cascade stages added in reverse at least 10 % of the
    non-zero elements change bits; on the setups whose partitions share elements the reversed partition tie and the chain-major
    order change at least 50 elements each.  (If one fails the stream changes, never the threshold.)"""
    m = measure(name)
    print("ROUNDING %-26s frames %3d nonzero %6d stages reversed %6d (%.1f %%) tie reversed %4d chain-major %4d" % (
        name, m["frames"], m["nonzero"], m["stages"], 100.0 * m["stages"] / m["nonzero"], m["tie"], m["chain"]))
    assert m["stages"] >= MIN_STAGE_SHARE * m["nonzero"], m
    if name in ALIASING:
        assert m["tie"] >= MIN_TIE_CHANGES and m["chain"] >= MIN_TIE_CHANGES, m


def _find(hay, needle):
    if needle.size > hay.size:
        return []
    return np.flatnonzero((np.lib.stride_tricks.sliding_window_view(hay, needle.size) == needle).all(axis=1)).tolist()


@pytest.mark.parametrize("name", ["table_books_pair", "table_books_general", "table_books_b1"])
def test_value_pools_equal_the_oracles_tables(oracle, name):
    """Quirk B-13 and its neighbours on values with 21-bit mantissas: sequence_p accumulated in double and cast per component,
    type 2 tables, lattice values.  Every value book's table as the oracle built it (orc_codebook_tables) equals the library's
    (nvh_stream_codebook_tables) bit for bit and sits, whole and once, in the VQ pool the table gather reads; a lattice book's
    values (type 1 without sequence_p) sit in the lattice pool in order."""
    import nvorbis_amd as nv
    from tests.test_host_logic import _tables
    hdr = list(headers(name))
    O, vp = oracle.L, C.c_void_p
    O.orc_codebook_info.argtypes = [vp, C.c_int] + [C.POINTER(C.c_int)] * 7
    O.orc_codebook_tables.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    st = nv.Stream(None, hdr[0], hdr[1], hdr[2])
    d = oracle.open_headers(hdr)
    try:
        lat, vq = st.lattice_pool(), st.vq_pool().view(np.uint32)
        kinds = set()
        for b, bk in enumerate(ss.rounding(name)["books"]):
            if bk.lookup == 0:
                continue
            p = _tables(nv.lib().nvh_stream_codebook_info, nv.lib().nvh_stream_codebook_tables, st._h, b, 0)
            o = _tables(O.orc_codebook_info, O.orc_codebook_tables, d, b, 0)
            tab = o["lookup"].view(np.uint32)
            assert tab.size == bk.entries * bk.dims and np.isfinite(o["lookup"]).all()
            assert np.array_equal(p["lookup"].view(np.uint32), tab), (name, b)
            assert len(_find(vq, tab)) == 1, (name, b)
            if bk.lookup == 1 and not bk.sequence_p:
                lv = bk.lookup1_values()
                assert len(_find(lat, tab.reshape(bk.entries, bk.dims)[:lv, 0])) == 1, (name, b)
            if b != ss.FLOOR0_LSP_BOOK:
                kinds.add((bk.lookup, bk.sequence_p))
        assert kinds == {(1, 0), (1, 1), (2, 0), (2, 1)}
    finally:
        O.orc_close(d)
        st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

T7 = {}  # measured run time of each GPU test (printed and bounded by the last test)

# The synthesis-slot names a batch may carry on the default toggles (nvh_launch.hip), by the walk the setup is here for, and the
# setups that reach it.  A slab batch names one of them and, beside it, only k_ola_compact (and the GPU parser's own kernels).
SLAB_ROUTES = {
    # residue_walk / residue_walk_two / the steady body: per-channel Residue1, stereo Residue2, the table gather
    "pair": ({"k_synth", "k_synth_group2"}, ("stereo_res1_coupled", "mono_res1_2048", "table_books_pair", "grid_2ch_256_2048",
                                             "grid_2ch_256_1024")),
    # more than two channels: k_synth8's walk -- the quirk-B-1 bin walk (residue_walk_bins) for the first two
    "wide": ({"k_synth8", "k_synth8+k_synth8_emit"}, ("three_ch_res2_misaligned", "table_books_b1", "ch5_res2", "six_ch_res2_4096")),
    # residue_walk_general
    "general": ({"k_synth_g"}, ("res0_slab", "odd_dims_slab", "res2_alias_stereo", "two_pass_slab", "equal_blocks_overrun",
                                "table_books_general")),
    "wide_general": ({"k_synth8_g"}, ("res0_3ch",)),
}
# outside the slab contract: what the batch must name (no k_synth*)
DESCRIPTOR_ROUTES = {
    "ch9_res2": ("k_spectrum_gen8",),                   # nine channels: the LDS-resident descriptor kernel
    "ch16_res1_4096": ("k_residue", "k_couple_floor"),  # a sequential residue, 128 KiB of spectra: the global-memory pair
    "mono_res0_small_blocks": ("k_spectrum_gen", "k_imdct_window"),  # n < 256: the generic kernels
}
GPU_SETUPS = tuple(n for _, names in SLAB_ROUTES.values() for n in names) + tuple(DESCRIPTOR_ROUTES)
NO_GPU_PARSE = ("ch9_res2", "ch16_res1_4096")  # more than NVH_PARSE_MAX_CH channels: set_gpu_parse raises ERR_UNSUPPORTED
_PARSE_KERNELS = ("k_parse_slab", "k_parse_links", "k_parse", "k_parse_fetch")


def _toggled():
    from tests.test_steady_groups import _TOGGLED
    return _TOGGLED


def _timed(name, t0):
    T7[name] = T7.get(name, 0.0) + time.time() - t0


def _decode(nv, ctx, pk, gr, fl, clip, batch_frames, gpu_parse):
    """The Stream path in batches of `batch_frames` frames: (PCM, [the four slot names of every batch])."""
    st = nv.Stream(ctx, pk[0], pk[1], pk[2])
    out, names = [], []
    try:
        st.set_clip(clip)
        if gpu_parse:
            st.set_gpu_parse(True)
        nfr = len(pk) - 3
        for a in range(0, nfr, batch_frames):
            b = min(a + batch_frames, nfr)
            for j in range(a, b):
                st.push_packet(pk[3 + j], gr[3 + j], fl[3 + j])
            if b >= nfr:
                st.push_end()
            out.append(st.synth_host().copy())
            names.append([k for k in st.kernels() if k != "-"])
    finally:
        st.close()
    return np.concatenate(out), names


def _check_route(name, names, what):
    for batch in names:
        ran = [k for k in batch if k not in _PARSE_KERNELS]
        if name in DESCRIPTOR_ROUTES:
            assert not any(k.startswith("k_synth") for k in ran) and all(k in ran for k in DESCRIPTOR_ROUTES[name]), (what, batch)
        else:
            synth = next(s for s, setups in SLAB_ROUTES.values() if name in setups)
            assert len([k for k in ran if k in synth]) == 1 and all(k in synth or k == "k_ola_compact" for k in ran), (what, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SETUPS)
def test_rounding_stream_bit_exact(oracle, gpu_ctx, name):
    """The rounding stream of every setup, uint32-exact against the oracle: clip on and off, batches of 1024 and of 5 frames, the
    host parser and -- where it takes the stream -- the GPU parser; on the default toggles every batch names the kernel of the walk
    the setup is here for.  ch9_res2 and ch16_res1_4096 have no slabs for the CPU conditions above to be checked on: their streams
    rest on the same recipe (three stages per class, the same value rule, the same encoder and kinds)."""
    import nvorbis_amd as nv
    from nvorbis_amd import native
    t0 = time.time()
    pk, gr, fl = (list(x) for x in stream(name))
    parsers = [False]
    st = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    try:
        st.set_gpu_parse(True)
        parsers.append(True)
    except native.NvhError as e:
        assert e.code == native.ERR_UNSUPPORTED
    finally:
        st.close()
    assert (len(parsers) == 2) == (name not in NO_GPU_PARSE)
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        assert ref.size > 0 and np.isfinite(ref).all()
        for bf in (1024, 5):
            for gpu_parse in parsers:
                got, names = _decode(nv, gpu_ctx, pk, gr, fl, clip, bf, gpu_parse)
                what = (name, clip, bf, gpu_parse)
                assert got.size == ref.size, what
                bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
                assert bad.size == 0, (what, bad.size, int(bad[0]), float(got[bad[0]]), float(ref[bad[0]]))
                if clip and bf == 1024:
                    print("ROUTE %-26s gpu_parse %d %s" % (name, gpu_parse, names))
                if not _toggled():
                    _check_route(name, names, what)
    _timed("bit_exact[%s]" % name, t0)


def _steady_case(oracle, ctx, pk, gr, fl, bounds, want, what):
    """tests/test_steady_groups.py: _run over `bounds`, clip on and off, both parsers: PCM == oracle; with host-written slabs the
    steady groups the device counted == the host's count == `want` (none under a toggle that takes the lean body away), and the
    second batch ran as frame groups of two.  The GPU parser writes the entry form of the slabs: no steady group."""
    import nvorbis_amd as nv
    from tests.test_frame_groups import _assert_same
    from tests.test_steady_groups import _run, _want
    # (NVH_GPU_PARSE makes the GPU parser a stream's default: no host slabs to count on.  NVH_NO_SLAB / NVH_UNFUSED launch no slab
    # kernel: the host's count then describes slabs nobody takes)
    parsers = (True,) if os.environ.get("NVH_GPU_PARSE") else (False, True)
    no_slabs = bool(os.environ.get("NVH_NO_SLAB") or os.environ.get("NVH_UNFUSED"))
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        for gpu_parse in parsers:
            out, steady, pending, names, _ = _run(nv, ctx, pk, gr, fl, bounds, clip=clip, gpu_parse=gpu_parse)
            _assert_same(np.concatenate(out), ref, (what, clip, gpu_parse))
            if gpu_parse or no_slabs:
                assert steady == [0] * len(want), (what, steady)
            else:
                assert steady == pending == _want(want), (what, steady, pending)
                if not _toggled():
                    assert names[1] == "k_synth_group2", (what, names)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid_2ch_256_2048", "grid_2ch_256_1024"])
def test_steady_groups_three_stage_chains(oracle, gpu_ctx, name):
    """Ten long stereo Residue2 frames behind the stream's first, batches [0, 1) and [1, 10): three steady groups through the lean
    body (both instantiations, n = 2048 and 1024), the first group and the last frame through the general one -- the two-frame
    walk with its peeled first stage and the masked later ones, whole wavefronts of lanes on chains of three stages."""
    import nvorbis_amd as nv
    from tests.test_steady_groups import _chains
    t0 = time.time()
    pk, gr, fl = (list(x) for x in stream(name, (1,) * 10, SEED))
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for i in range(3, len(pk)):
            st.push_packet(pk[i], gr[i], fl[i])
        words, first = st.pending_slabs()
    finally:
        st.close()
    for f in range(1, 10):
        depth, lpc = _chains(words, first, f)
        lanes = np.repeat(depth, lpc)
        assert any(lanes[w0:w0 + 64].size == 64 and lanes[w0:w0 + 64].min() >= 3 for w0 in range(0, lanes.size, 64)), (f, lanes.size)
    _steady_case(oracle, gpu_ctx, pk, gr, fl, [0, 1, 10], [0, 3], name)
    _timed("steady[%s]" % name, t0)


@pytest.mark.gpu
def test_steady_and_general_groups_mixed(oracle, gpu_ctx):
    """L | L L | L S | S L | L L | L L | L at 2048 / 256 behind the stream's first frame, as tests/test_steady_groups.py:
    test_steady_and_general_groups_trade_quarters: steady groups of both launches beside general ones, on sums that round."""
    t0 = time.time()
    kinds = (1,) + (1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1)
    pk, gr, fl = (list(x) for x in stream("grid_2ch_256_2048", kinds, SEED + 1))
    _steady_case(oracle, gpu_ctx, pk, gr, fl, [0, 1, len(kinds)], [0, 3], "mixed")
    _timed("steady_mixed", t0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_ch_res2_misaligned", "six_ch_res2_4096"])
def test_wide_paired_emission(oracle, gpu_ctx, name):
    """Twenty long frames in one batch: the wide kernel's emitting twin (k_synth8 for the odd frames, k_synth8_emit for the even
    ones) walks the same three-stage chains -- the quirk-B-1 bin walk on three channels, the pair walk on six.  (The twelve-frame
    streams above switch block sizes too often for a batch to emit.)"""
    import nvorbis_amd as nv
    t0 = time.time()
    pk, gr, fl = (list(x) for x in stream(name, (1,) * 20, SEED + 2))
    for clip in (True, False):
        ref = oracle.decode_packets(pk, gr, fl, clip=clip)[0]
        for gpu_parse in (False, True):
            got, names = _decode(nv, gpu_ctx, pk, gr, fl, clip, 1024, gpu_parse)
            assert got.size == ref.size and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, clip, gpu_parse)
            if not _toggled():
                assert [k for k in names[0] if k not in _PARSE_KERNELS][0] == "k_synth8+k_synth8_emit", (name, gpu_parse, names)
    _timed("wide_emit[%s]" % name, t0)


@pytest.mark.gpu
@pytest.mark.parametrize("toggle", ["NVH_NO_STEADY", "NVH_NO_WALK_TWO", "NVH_FPW=1", "NVH_FPW=4", "NVH_NO_EMIT", "NVH_NO_SLAB",
                                    "NVH_UNFUSED", "NVH_GPU_PARSE"])
def test_replay_under_a_toggle(toggle):
    """The toggles are read once per process: this file's GPU tests again in a child process per value -- without the lean body,
    without the two-frame walk, one and four frames per workgroup, without paired emission, through the descriptor kernels
    (k_spectrum_* and, unfused, the global-memory k_residue for every setup), with the GPU parser as the default one."""
    if os.environ.get("NVH_TEST_CHILD"):
        pytest.skip("already inside a replay")
    from tests.replay import run_children
    t0 = time.time()
    env = dict(os.environ)
    key, _, val = toggle.partition("=")
    env[key] = val or "1"
    env["NVH_TEST_CHILD"] = "1"
    run_children([(["test_residue_rounding.py"], env, [])], timeout=300)
    _timed("replay[%s]" % toggle, t0)


@pytest.mark.gpu
def test_t7_run_times():
    """(Last.)  The measured run time of each GPU test of this file, against the budget of a few seconds each."""
    for k, v in sorted(T7.items()):
        print("T7 %-44s %6.2f s" % (k, v))
    assert all(v < 10.0 for v in T7.values()), T7

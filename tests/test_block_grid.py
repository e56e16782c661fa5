"""Every pair of block sizes Vorbis I allows (block0 <= block1 out of 64 ... 8192: 36 pairs), mono and stereo, against the oracle.

The router picks kernels by comparing the two block sizes with fixed thresholds (nvh_setup.hip: slab_setup_ok; nvh_launch.hip:
assign_emission, slab_wide, slab_lds_bytes, batch_launch), and the suite's other setups sit on nine of the 36 pairs.  The 72
setups here are one recipe (tests/synth_stream.py: _grid_config, GRID_NAMES) at every pair; the recipe is the one the issue
proposed, unchanged.

CPU: the oracle is pinned to the specification decoder on every cell the reference's transform allows (block0 >= 256; the
block1 == 8192 column for stereo only, the specification decoder needs 5 s for such a cell), and the host parser's geometry and
the host slab writer's floor and residue sections are checked against the oracle with the assertions of tests/test_host_logic.py
and tests/test_host_slabs.py.

GPU: per cell a structured full-depth stream and a random-bit stream with inconsistent window flags, both parsers, clip on and
off, batches of 1024, 5 and 2 frames: every PCM bit and HasClipped equal the oracle's, and the kernels the batches name are the
family ROUTES promises for the cell.  The forms of PCM (s16, planar, mono mix) run on the routes no other file reaches, and the
last test replays the file under the toggles that change routes and checks which kernels the comparisons reached."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import spec_pin, synth_stream as ss, vorbis_encode as ve
from tests.test_frame_groups import EMIT_NAME, _fpw, _names_checked
from tests.test_pcm_mix import mix_rule, same_bits
from tests.test_pcm_s16 import to_s16

CELLS = list(ss.GRID_NAMES)


def _cell(name):
    return ss.grid_cell(name)


# ---- which cells are pinned to the specification decoder, and why the others are not ------------------------------------------
_B10 = spec_pin.UNPINNED["mono_res0_small_blocks"]
_COST = "the stereo cell of the same pair is pinned; the specification decoder takes 4-7 s per block1 == 8192 cell"
UNPINNED = {n: (_B10 if _cell(n)[1] < 256 else _COST) for n in CELLS if _cell(n)[1] < 256 or (_cell(n)[2] == 8192 and _cell(n)[0] == 1)}
PINNED = [n for n in CELLS if n not in UNPINNED]

# ---- the routes: nvh_launch.hip / nvh_setup.hip as read for mono and stereo setups on the default toggles -----------------------
# family -> what a batch of the structured stream (one batch, host parser) must name in the slots (-, synthesis, transform, overlap)
#   descriptor : block0 < 256 -- nvh_setup.hip: slab_ok needs block0 >= 256, so no slab kernel; nvh_launch.hip: `compact` needs
#                block0 >= 256 too, so neither fused transform exists and the slot names k_imdct_window, the overlap
#                k_ola_emit or k_ola_emit_seq
#   narrow     : block0 >= 256, block1 <= 2048 -- assign_emission: `narrow`, frame groups of NVH_FPW frames emit through block
#                switches (k_synth_group2 by default; at NVH_FPW=4 a batch whose slabs leave no room for four frames' LDS goes
#                to k_synth + k_synth_emit, nvh_launch.hip: `if (!slab_size_ok(b) && b->fpw > 1)`)
#   wide4096   : block1 == 4096 -- slab_wide (block1 > 2048) and `wide_emit` (block1 <= 4096): k_synth8 + k_synth8_emit
#   wide8192   : block1 == 8192 -- slab_wide, no paired emission (`wide_emit` needs block1 <= 4096): k_synth8 and k_ola_compact
ROUTES = {
    "descriptor": dict(synth=None, transform="k_imdct_window", overlap=("k_ola_emit", "k_ola_emit_seq")),
    "narrow": dict(synth="group", transform="-", overlap=None),
    "wide4096": dict(synth="k_synth8+k_synth8_emit", transform="-", overlap=None),
    "wide8192": dict(synth="k_synth8", transform="-", overlap=("k_ola_compact",)),
}
# cells the GPU parser refuses at open (NVH_ERR_UNSUPPORTED): none -- the recipe's books, floors and channel counts are inside
# nvh_setup.hip: plan_parse_tables' limits at every block size.  (name -> reason; read by the CPU and the GPU tests)
GPU_PARSE_REFUSED = {}


def family(name):
    _, b0, b1 = _cell(name)
    if b0 < 256:
        return "descriptor"
    return "narrow" if b1 <= 2048 else ("wide4096" if b1 == 4096 else "wide8192")


# ---- streams --------------------------------------------------------------------------------------------------------------------
# 72 frames, two runs of short blocks between runs of long ones: all four transitions (long-long, long-short, short-short,
# short-long), opening and closing on long blocks, the switches at frames 13, 20, 40 and 48 -- inside and between groups of two
# and four frames, inside and between batches of 5 and of 2.  Frame groups emit through the switches (every frame but the
# first).  Where only equal neighbours in their steady state pair (k_synth8_emit, NVH_FPW=1) eight frames stand outside: the
# first, the last (it hands out its tail as well), and per run of short blocks the long block in front of it (it emits the
# flat part of its window too), its first block and the long block behind it -- 64 of 72 emit, above the router's 7/8 (a first
# draft of 48 frames had 41: its wide cells ran k_synth8 + k_ola_compact).
GRID_KINDS = np.array([1] * 13 + [0] * 7 + [1] * 20 + [0] * 8 + [1] * 24, dtype=bool)
_STREAMS = {}
_ORACLE = {}


def cell_stream(oracle, name, kind):
    """(packets, granules, flags) of a cell's stream; kind "structured": full-depth packets on GRID_KINDS with consistent window
    flags, no silent channel; "random": random side information, inconsistent window flags, silent channels, 60 frames."""
    key = (name, kind)
    if key not in _STREAMS:
        if kind == "structured":
            hdr = list(spec_pin.headers(name))
            pk, gr = ve.encode_stream(ve.setup_of(hdr), hdr, GRID_KINDS, 100 + CELLS.index(name))
            _STREAMS[key] = (list(pk), list(gr), [0] * len(pk))
        else:
            _STREAMS[key] = ss.filtered_stream(oracle, name, 60, 300 + CELLS.index(name), consistent_windows=False)
    return _STREAMS[key]


def oracle_pcm(oracle, name, kind, clip):
    key = (name, kind, clip)
    if key not in _ORACLE:
        pk, gr, fl = cell_stream(oracle, name, kind)
        pcm, info = oracle.decode_packets(pk, gr, fl, clip=clip)
        pcm.setflags(write=False)
        _ORACLE[key] = (pcm, info["has_clipped"])
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------

def test_grid_names_cover_every_pair_and_stay_out_of_the_config_list():
    assert len(CELLS) == len(set(CELLS)) == 72
    cells = {_cell(n) for n in CELLS}
    assert cells == {(ch, b0, b1) for ch in (1, 2) for b0 in ss.BLOCK_SIZES for b1 in ss.BLOCK_SIZES if b0 <= b1}
    assert not set(CELLS) & set(ss.CONFIG_NAMES)
    for bad in ("grid_3ch_256_2048", "grid_2ch_2048_256", "grid_2ch_96_2048"):
        with pytest.raises(KeyError):
            ss.config(bad)
    for n in CELLS:
        c = ss.config(n)
        assert (c["channels"], c["block0"], c["block1"]) == _cell(n) and c["modes"] == [(0, 0), (1, 1)]


def test_every_cell_is_pinned_or_says_why():
    assert set(PINNED) | set(UNPINNED) == set(CELLS) and not set(PINNED) & set(UNPINNED)
    assert len(PINNED) == 42 - 6 and all(UNPINNED[n] for n in UNPINNED)
    for n in CELLS:
        ch, b0, b1 = _cell(n)
        if b0 < 256:
            assert UNPINNED[n] == _B10
        elif n in UNPINNED:  # only the mono cells of the 8192 column, whose stereo cell is pinned
            assert (ch, b1) == (1, 8192) and ss.grid_name(2, b0, b1) in PINNED
    assert set(ROUTES) == {family(n) for n in CELLS}
    assert GRID_KINDS[0] and GRID_KINDS[-1]
    pairs = {(bool(a), bool(b)) for a, b in zip(GRID_KINDS[:-1], GRID_KINDS[1:])}
    assert pairs == {(True, True), (True, False), (False, False), (False, True)}


@pytest.mark.parametrize("name", PINNED)
def test_cell_pinned_to_the_spec_decoder(oracle, name):
    """The structured stream of tests/spec_pin.py (long x 4, short x 3, long x 5: all four transitions; a quarter of the channels
    silent) with an empty quirk set: the oracle, clip off, agrees with vorbis_spec.SpecDecoder within spec_pin.FLOOR1_BOUND x
    peak (1e-6), the sample counts are (last granule + block1 / 2) x channels, the peak is above 1e-3 and every sample finite.
    Measured on the 36 cells pinned here: the largest error 3.4e-7 of the peak (stereo 512/4096), the smallest peak 8.6e-3 (mono
    256/256)."""
    ch, b0, b1 = _cell(name)
    pk, gr = spec_pin.stream(name)
    ref, info = oracle.decode_packets(list(pk), list(gr), [0] * len(pk), clip=False)
    ref = ref.astype(np.float64)
    pcm = spec_pin.spec_pcm(name, ())
    assert info["channels"] == ch and (info["block0"], info["block1"]) == (b0, b1)
    assert ref.size == pcm.size == (gr[-1] + b1 // 2) * ch
    peak = float(np.abs(ref).max())
    assert peak > 1e-3 and np.isfinite(ref).all()
    err = float(np.abs(ref - pcm).max())
    print("%s: spec pin %.2e of the peak (peak %.3g)" % (name, err / peak, peak))
    assert err <= spec_pin.FLOOR1_BOUND * peak, (name, err / peak)


def _host_frames(nv, pk):
    """Per audio packet that yields a decoded frame on a host-only stream: (packet index, slab words or None, block size)."""
    s = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        for i in range(3, len(pk)):
            s.drop_pending()
            s.push_packet(pk[i], -1, 0)
            if s.pending()[0] != 1 or int(s.pending_geometry()[-1][0]) == 0:
                continue
            yield s, i, int(s.pending_geometry()[-1][0])
    finally:
        s.close()


@pytest.mark.parametrize("name", CELLS)
def test_cell_host_geometry_and_slabs(oracle, name):
    """A host-only stream of the cell: the parser's frame geometry and sample count equal the oracle's trace on both of the
    cell's streams (tests/test_host_logic.py: test_parser_geometry_synthetic_configs' assertions); the GPU parser's plan accepts
    the setup unless GPU_PARSE_REFUSED says otherwise; with block0 >= 256 the slab writer's floor sections reproduce the oracle's
    Floor1 curves bin for bin and its residue sections the oracle's residue vectors bit for bit (tests/test_host_slabs.py:
    check_frame_floors, _slab_residue_sums).  Below 256 no batch takes the slabs; that is the router's decision, made where a
    device is (nvh_setup.hip: slab_setup_ok), and a host-only stream has nothing that reports it: test_cell_bit_exact asserts it
    from the kernel names (ROUTES: descriptor)."""
    import nvorbis_amd as nv
    from tests import vorbis_spec as vs
    from tests.test_gpu_parity import _open_headers
    from tests.test_host_logic import _parse_all
    from tests.test_host_slabs import _slab_residue_sums, check_frame_floors, parse_slab
    ch, b0, b1 = _cell(name)
    for kind in ("structured", "random"):
        pk, gr, fl = cell_stream(oracle, name, kind)
        geo, smp, pos, err = _parse_all(nv, pk, gr, fl)
        pcm, info = oracle.decode_packets(pk, gr, fl, trace=True)
        assert err is None
        assert smp * info["channels"] == pcm.size
        ok = info["trace"][info["trace"][:, 3] == 1]
        dec = geo[geo[:, 0] != 0]
        assert dec.shape[0] == ok.shape[0]
        assert np.array_equal(dec[:, 0], ok[:, 4]) and np.array_equal(dec[:, 1], ok[:, 0]) and np.array_equal(dec[:, 3], ok[:, 2])
        if kind == "structured":
            assert set(dec[:, 0].tolist()) == {b0, b1}
    pk = cell_stream(oracle, name, "structured")[0]
    s = nv.Stream(None, pk[0], pk[1], pk[2])
    try:
        assert (s.channels, s.block0, s.block1) == (ch, b0, b1)
        assert bool(s.parse_book_info(0)["gpu_parse_ok"]) == (name not in GPU_PARSE_REFUSED)
    finally:
        s.close()
    if b0 < 256:
        return
    S = vs.Setup(pk[0], pk[2])
    db = np.array([oracle.L.orc_inverse_db(i) for i in range(256)], np.float32)
    frames = vectors = curves = 0
    sizes = set()
    for kind, count in (("structured", 16), ("random", 30)):
        # (the structured stream's first 16 frames hold both block sizes and three of the four transitions; every frame is full depth)
        pk = cell_stream(oracle, name, kind)[0][:3 + count]
        d = _open_headers(oracle, pk)
        scratch = np.zeros(ch * b1, np.float32)
        try:
            lat = vq = None
            for s, i, n in _host_frames(nv, pk):
                if lat is None:
                    lat, vq = s.lattice_pool(), s.vq_pool()
                a, b, c, e = C.c_int(), C.c_int(), C.c_int(), C.c_int()
                if oracle.L.orc_decode_packet_block(d, pk[i], len(pk[i]), scratch.ctypes.data, C.byref(a), C.byref(b), C.byref(c), C.byref(e)) != 1:
                    continue
                words, first = s.pending_slabs()
                h = parse_slab(words)
                assert h["n"] == n == e.value and h["vecs"] * 4 == words.size and int(first[1]) * 4 == words.size
                curves += check_frame_floors(oracle, d, S, s, pk[i], words, db, b1, (name, kind, i))
                posn, idx, anyx = np.zeros(16, np.int32), np.zeros(16, np.int32), C.c_int()
                ncall = oracle.L.orc_last_residue_calls(d, posn.ctypes.data, idx.ctypes.data, 16, C.byref(anyx))
                ref = np.zeros(ch * b1, np.float32)
                for k in range(ncall):
                    bits = C.c_int()
                    assert oracle.L.orc_residue_decode_at(d, int(idx[k]), pk[i], len(pk[i]), int(posn[k]), anyx.value, n, ref.ctypes.data,
                                                          C.byref(bits)) == 0
                got = _slab_residue_sums(words, h, lat, ch, n // 2, vq)
                want = ref.reshape(ch, b1)[:, :n // 2]
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, kind, i, float(np.abs(got - want).max()))
                frames += 1
                vectors += h["nrec"]
                sizes.add(n)
        finally:
            oracle.L.orc_close(d)
    assert frames >= 20 and vectors > 100 and curves >= 20 and sizes == {b0, b1}, (frames, vectors, curves, sizes)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------

_SEEN = set()  # what the bit-exact comparisons of this process reached: kernel names, "name|Nch", "name|n>=2048"


def _bits_equal(got, ref, what):
    assert got.size == ref.size, (what, got.size, ref.size)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (what, float(np.abs(got - ref).max()))


def _open(nv, ctx, pk, clip, gpu_parse):
    """A stream with the parser asked for, or None where the GPU parser refuses the setup (NVH_ERR_UNSUPPORTED at open)."""
    from nvorbis_amd import native
    st = nv.Stream(ctx, pk[0], pk[1], pk[2])
    st.set_clip(clip)
    if gpu_parse:
        try:
            st.set_gpu_parse(True)
        except nv.NvhError as e:
            st.close()
            assert e.code == native.ERR_UNSUPPORTED, e
            return None
    return st


def _batches(st, pk, gr, fl, bf, **form):
    """The stream batch by batch (bf frames each, push_end before the last): ([PCM of every batch], [(frames, largest block of
    the batch, the four slots' kernel names)])."""
    nfr = len(pk) - 3
    out, info = [], []
    for a in range(0, nfr, bf):
        b = min(a + bf, nfr)
        for j in range(a, b):
            st.push_packet(pk[3 + j], gr[3 + j], fl[3 + j])
        if b >= nfr:
            st.push_end()
        fr = st.pending()[0]
        if fr == 0:
            continue
        nmax = int(st.pending_geometry()[:, 0].max())
        out.append(st.synth_host(**form).copy())
        info.append((fr, nmax, st.kernels()))
    return out, info


def _note(info, ch):
    for fr, nmax, names in info:
        for k in names:
            if k != "-":
                _SEEN.add(k)
                _SEEN.add("%s|%dch" % (k, ch))
                if nmax >= 2048:
                    _SEEN.add(k + "|n>=2048")


def _check_route(name, info):
    """The one batch of the structured stream against ROUTES (default toggles, host parser)."""
    assert len(info) == 1 and info[0][0] == len(GRID_KINDS), info
    slots = info[0][2]
    r = ROUTES[family(name)]
    if r["synth"] is None:
        assert not any(k.startswith("k_synth") for k in slots), (name, slots)
    elif r["synth"] == "group":
        # (NVH_FPW=4: nvh_launch.hip sends a batch whose slabs leave no room for four frames' LDS to one frame per workgroup)
        assert slots[1] in ((EMIT_NAME[_fpw()], EMIT_NAME[1]) if _fpw() == 4 else (EMIT_NAME[_fpw()],)), (name, slots)
    else:
        assert slots[1] == r["synth"], (name, slots)
    assert slots[2] == r["transform"], (name, slots)
    if r["overlap"] is not None:
        assert slots[3] in r["overlap"], (name, slots)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CELLS)
def test_cell_bit_exact(oracle, gpu_ctx, name):
    """One cell: the structured and the random stream, clip on and off, the host and the GPU parser, batches of 1024, 5 and 2
    frames (a group and a batch boundary on every kind of switch): the PCM equals the oracle's in every bit, HasClipped agrees,
    and the structured stream's single batch names the kernels of the cell's family (ROUTES) -- which, for the slab families,
    says that at least 7/8 of its frames emit."""
    import nvorbis_amd as nv
    ch, b0, b1 = _cell(name)
    largest = 0
    for kind in ("structured", "random"):
        pk, gr, fl = cell_stream(oracle, name, kind)
        for clip in (True, False):
            ref, ref_clipped = oracle_pcm(oracle, name, kind, clip)
            for gpu_parse in (False, True):
                for bf in (1024, 5, 2):
                    st = _open(nv, gpu_ctx, pk, clip, gpu_parse)
                    assert (st is None) == (gpu_parse and name in GPU_PARSE_REFUSED), (name, gpu_parse)
                    if st is None:
                        break
                    try:
                        out, info = _batches(st, pk, gr, fl, bf)
                        what = (name, kind, clip, gpu_parse, bf)
                        _bits_equal(np.concatenate(out) if out else np.zeros(0, np.float32), ref, what)
                        assert st.has_clipped() == ref_clipped, what
                        assert not st.parse_errors, what
                    finally:
                        st.close()
                    _note(info, ch)
                    largest = max([largest] + [i[1] for i in info])
                    if kind == "structured" and bf == 1024 and not gpu_parse and _names_checked():
                        _check_route(name, info)
    assert largest == b1  # (what the replay test's "at n >= 2048" rests on)


# the routes no other file's PCM forms reach: mono and stereo through k_synth8 + k_synth8_emit (block1 == 4096, the short block
# small and as large as the long one), frame groups through a 1024 : 2048 switch, the descriptor kernels at n = 2048
FORM_CELLS = ["grid_1ch_256_4096", "grid_2ch_256_4096", "grid_1ch_4096_4096", "grid_2ch_4096_4096", "grid_2ch_1024_2048", "grid_2ch_64_2048"]
# form -> (synth_host arguments, the twins' suffix for a stereo and for a mono stream: nvh_launch.hip takes planar and mixed output of
# a one-channel stream as plain interleaved PCM, `if (ch == 1 && !out.mapped())`)
FORMS = {
    "s16": (dict(dtype=np.int16), "_s16", "_s16"),
    "planar": (dict(planar=True), "_planar", ""),
    "mono": (dict(mix="mono"), "_mono", ""),
    "mono_s16": (dict(mix="mono", dtype=np.int16), "_s16_mono", "_s16"),
}


def _writes_pcm(k):
    return "emit" in k or k.startswith("k_synth_group") or k.startswith("k_ola_")


def _form_reference(form, ref_clip, ref_raw, ch, clip):
    """(expected PCM, expected HasClipped) of a form from the oracle's PCM (ref_clip: with the run's clip setting, ref_raw: unclipped)."""
    if form == "s16":
        return to_s16(ref_clip[0]), ref_clip[1]
    if form == "planar":
        return np.ascontiguousarray(ref_clip[0].reshape(-1, ch).T), ref_clip[1]
    m, clipped = mix_rule(ref_raw[0], ch, clip, np.int16 if form == "mono_s16" else np.float32)
    return m, clipped and clip


@pytest.mark.gpu
@pytest.mark.parametrize("name", FORM_CELLS)
@pytest.mark.parametrize("form", list(FORMS))
def test_cell_pcm_forms(oracle, gpu_ctx, name, form):
    """Interleaved s16, planar f32 and the mono mix as f32 and s16 on the new routes, both streams, clip on and off, batches of
    1024 and 5 frames: to_s16 (tests/test_pcm_s16.py) / the transposition / mix_rule (tests/test_pcm_mix.py) of the oracle's
    PCM, bit for bit; every batch ran the float batch's kernels with the form's twins in the slots that write PCM."""
    import nvorbis_amd as nv
    ch, b0, b1 = _cell(name)
    kw, sfx2, sfx1 = FORMS[form]
    sfx = sfx2 if ch == 2 else sfx1
    for kind in ("structured", "random"):
        pk, gr, fl = cell_stream(oracle, name, kind)
        for clip in (True, False):
            want, want_clipped = _form_reference(form, oracle_pcm(oracle, name, kind, clip), oracle_pcm(oracle, name, kind, False), ch, clip)
            for bf in (1024, 5):
                sf, st = _open(nv, gpu_ctx, pk, clip, False), _open(nv, gpu_ctx, pk, clip, False)
                try:
                    _, finfo = _batches(sf, pk, gr, fl, bf)
                    out, info = _batches(st, pk, gr, fl, bf, **kw)
                    what = (name, form, kind, clip, bf)
                    got = np.concatenate(out, axis=1 if form == "planar" else 0)
                    assert same_bits(got, want), what
                    assert st.has_clipped() == want_clipped, what
                finally:
                    sf.close()
                    st.close()
                _note(info, ch)
                for (_, _, kf), (_, _, ks) in zip(finfo, info):
                    assert ks == [k + sfx if _writes_pcm(k) else k for k in kf], (what, kf, ks)
                if kind == "structured" and bf == 1024 and _names_checked():
                    slots = info[0][2]
                    fam = family(name)
                    if fam == "wide4096":
                        assert slots[1] == "k_synth8+k_synth8_emit" + sfx, (what, slots)
                    elif fam == "narrow":
                        assert slots[1] in ((EMIT_NAME[_fpw()] + sfx, EMIT_NAME[1] + sfx) if _fpw() == 4 else (EMIT_NAME[_fpw()] + sfx,)), (what, slots)
                    else:
                        assert slots[3] in ("k_ola_emit" + sfx, "k_ola_emit_seq" + sfx), (what, slots)


REPLAYS = ["NVH_FPW=1", "NVH_FPW=4", "NVH_EMIT_ALWAYS=1", "NVH_NO_EMIT=1", "NVH_NO_SLAB=1", "NVH_POISON_PLANES=1",
           "NVH_POISON_PLANES=1+NVH_GPU_PARSE=1"]
REACHED = ["k_synth_group2", "k_synth_group4", "k_synth+k_synth_emit", "k_synth8+k_synth8_emit|1ch", "k_synth8+k_synth8_emit|2ch",
           "k_imdct_window|n>=2048"]


@pytest.mark.gpu
def test_replays_reach_every_route(tmp_path_factory):
    """(Last in this file.)  The GPU tests above replayed in child processes (tests/replay.py) under NVH_FPW=1, NVH_FPW=4,
    NVH_EMIT_ALWAYS, NVH_NO_EMIT, NVH_NO_SLAB and NVH_POISON_PLANES with both parsers, at most six children at a time.  The union
    of the kernel names the bit-exact comparisons reached, this process's included, holds both frame-group kernels, k_synth +
    k_synth_emit, k_synth8 + k_synth8_emit with one and with two channels, k_imdct_window and k_ola_emit (or _seq) in batches
    with blocks of 2048 samples and more."""
    if os.environ.get("NVH_TEST_CHILD"):
        out = os.environ.get("NVH_GRID_SEEN")
        if out:
            with open(out, "w") as fh:
                json.dump(sorted(_SEEN), fh)
        return  # inside a replay: the parent checks the union
    from tests.replay import run_children
    d = tmp_path_factory.mktemp("grid_seen")
    children, files = [], []
    for k, toggles in enumerate(REPLAYS):
        env = dict(os.environ)
        for t in toggles.split("+"):
            key, _, val = t.partition("=")
            env[key] = val
        env["NVH_TEST_CHILD"] = "1"
        env["NVH_GRID_SEEN"] = str(d / ("%d.json" % k))
        files.append(env["NVH_GRID_SEEN"])
        children.append((["test_block_grid.py"], env, []))
    run_children(children[:4], timeout=1500)
    run_children(children[4:], timeout=1500)
    seen = set(_SEEN)
    for f in files:
        seen |= set(json.load(open(f)))
    missing = sorted(set(REACHED) - seen)
    assert not missing, "no bit-exact comparison reached %s (seen: %s)" % (missing, sorted(seen))
    assert {"k_ola_emit|n>=2048", "k_ola_emit_seq|n>=2048"} & seen, sorted(seen)

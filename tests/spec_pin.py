"""Structured streams of every synthetic configuration and their decode by the spec-derived decoder (test infrastructure for
tests/test_spec_pin.py and the GPU comparisons in tests/test_gpu_parity.py).

QUIRKS names, per configuration of tests/synth_stream.py, the reference departures (tests/vorbis_spec.py's
switches) that its structured stream exercises: with exactly that set the spec-derived decoder agrees with the oracle, and
without any one of them it does not.  The measured max |oracle - spec| / peak is in the comment behind each entry.
"""
import functools

import numpy as np

from tests import synth_stream as ss, vorbis_encode as ve, vorbis_spec as vs

# (B10 is not modelled: mono_res0_small_blocks, whose blocks of 64 / 128 samples take the reference's inverse MDCT below
# n = 256, which is not a transform, SURVEY.md Appendix A.3, is the one configuration left unpinned)
UNPINNED = {"mono_res0_small_blocks": "B10: the reference's inverse MDCT for n < 256 is not a transform"}

QUIRKS = {
    "stereo_res1_coupled": (),                  # 2.5e-7
    "three_ch_res2_misaligned": ("B1",),        # 2.2e-7
    "six_ch_res2_4096": ("B4",),                # 1.6e-7
    "floor0_stereo": ("B9",),                   # 6.8e-7 (Floor0 bound below)
    "floor0_slab": (),                          # 1.6e-5 (Floor0 bound below)
    "two_submaps": ("B2", "B3", "B4"),          # 7.9e-8
    "equal_blocks_overrun": (),                 # 2.3e-7
    "mono_8192": ("B6",),                       # 2.1e-7
    "stereo_8192": ("B6",),                     # 2.5e-7
    "ch4_res1": (),                             # 2.1e-7
    "ch5_res2": ("B1", "B4"),                   # 1.3e-7
    "ch7_res1": ("B2", "B4"),                   # 1.3e-7
    "ch8_res2": ("B4",),                        # 1.1e-7
    "mono_res1_2048": (),                       # 2.3e-7
    "res0_slab": (),                            # 2.2e-7
    "odd_dims_slab": (),                        # 1.8e-7
    "res2_alias_stereo": ("B1",),               # 1.8e-7
    "two_pass_slab": ("B2",),                   # 1.9e-7
    "res0_3ch": ("B2", "B4"),                   # 1.3e-7
    "table_books_pair": (),                     # 3.8e-7
    "table_books_general": (),                  # 2.8e-7
    "table_books_b1": ("B1",),                  # 2.2e-7
    "ch9_res2": ("B4",),                        # 1.5e-7
    "ch16_res1_4096": ("B2", "B4"),             # 1.1e-7
    "ch40_res1": ("B2", "B4"),                  # 1.5e-7
    "longcode_res1": (),                        # 1.6e-7
    "longcode_res2": (),                        # 2.0e-7
    "longcode_many_books": (),                  # 1.7e-7
}

FLOOR1_BOUND = 1e-6  # x peak
# Floor0: the oracle evaluates the curve in float32 with the reference's operation order (the Bark map, 2 cos(w) - 2 cos(c)
# products, sqrt, exp), the spec-derived decoder in double.  Measured on 24 structured streams (floor0_stereo and
# floor0_slab, both long modes, 60 Markov frames each -- both block sizes, 20 % silent channels): max 1.05e-4 x peak.
FLOOR0_BOUND = 4e-4  # x peak

# long x 4, short x 3, long x 5: the reference's first emitted samples line up with the specification's only when the
# stream opens with long blocks (tests/test_spec_pin.py: test_ogg_writer_round_trip), and its last block is a long one
KINDS = np.array([1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1], dtype=bool)
P_SILENT = 0.25


def bound(name):
    cfg_floors = vs.Setup(*headers(name)[0::2]).floors
    return FLOOR0_BOUND if any(f.type == 0 for f in cfg_floors) else FLOOR1_BOUND


@functools.lru_cache(maxsize=None)
def headers(name):
    return tuple(ss.make_stream(ss.config(name), 0, 1)[0][:3])


@functools.lru_cache(maxsize=None)
def stream(name, seed=7):
    """(packets, granules) of the configuration's structured stream: KINDS, full-depth side information, P_SILENT."""
    hdr = list(headers(name))
    pk, gr = ve.encode_stream(ve.setup_of(hdr), hdr, KINDS, seed, p_silent=P_SILENT)
    return tuple(pk), tuple(gr)


@functools.lru_cache(maxsize=None)
def spec_pcm(name, quirks):
    """Interleaved float64 PCM of the spec-derived decoder with `quirks` (a sorted tuple), followed by the windowed right half
    of the last block -- the tail the reference hands out after the last packet of a packet list."""
    pk, _ = stream(name)
    with np.errstate(all="ignore"):
        dec = vs.SpecDecoder(pk[0], pk[2], quirks)
        outs = [dec.packet(p) for p in pk[3:]]
    outs.append(dec.prev_tail)
    return np.concatenate(outs, axis=1).T.reshape(-1).copy()


# the long-code configurations (tests/synth_stream.py: LONGCODE_NAMES) also get a longer stream, 24 frames, so that every code
# length of every book is written and the slab test's frame / vector minimum is met: long x 4, short x 3, long x 5, short x 4, long x 8
KINDS24 = np.array([1] * 4 + [0] * 3 + [1] * 5 + [0] * 4 + [1] * 8, dtype=bool)


@functools.lru_cache(maxsize=None)
def stream24(name, seed=24):
    """(packets, granules, stats) of a configuration's 24-frame structured stream; stats["symbols"][(book, code length)] counts
    the symbols the encoder wrote (tests/vorbis_encode.py: BookEnc.put)."""
    hdr = list(headers(name))
    stats = {}
    pk, gr = ve.encode_stream(ve.setup_of(hdr), hdr, KINDS24, seed, p_silent=P_SILENT, stats=stats)
    return tuple(pk), tuple(gr), stats


@functools.lru_cache(maxsize=None)
def stream24_cut(name, seed=24):
    """stream24 with every second audio packet cut at a seeded random byte count somewhere in its second half: packets that end
    inside a long code (the reference then matches against the zero-padded word, Codebook.cs:299-318)."""
    pk, gr, _ = stream24(name, seed)
    rng = np.random.default_rng(seed + 1)
    out = list(pk)
    for i in range(3, len(out), 2):
        n = len(out[i])
        out[i] = out[i][:int(rng.integers(n // 2, n))]
    return tuple(out), gr

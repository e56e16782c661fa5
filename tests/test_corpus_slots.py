"""The slot plan of the corpus pass (nvorbis_amd/corpus.py: _Slot, _plan_slots) and the one function that decodes a file into a
slot (_decode_into).

Without a GPU: the plan of six files in the three output forms against numbers written out by hand below, against the expressions
decode_files_to_device held inline before there was a planner (restated in _inline_layout), and the views and synth_device
arguments a slot gives, on a CPU tensor.  On the GPU: a slot one sample per channel too short is refused before the batch that
would pass its end is synthesised, in every form, and the right slot gives the streaming reader's PCM bit for bit."""
import numpy as np
import pytest

from tests.test_ogg_damage import _stream

# (samples per channel, channels) per file
FILES = [(0, 1), (1, 2), (3, 1), (4, 6), (5, 2), (1023, 3)]
PER_CH = [p for p, _ in FILES]
CHANS = [c for _, c in FILES]
STRIDES = [0, 4, 4, 4, 8, 1024]
# form -> (planar, mono, offsets, reserved elements, counts the decode must reach, total elements)
WANT = {
    "interleaved": (False, False, [0, 0, 2, 5, 29, 39], [0, 2, 3, 24, 10, 3069], [0, 2, 3, 24, 10, 3069], 3108),
    "mono": (False, True, [0, 0, 4, 8, 12, 20], [0, 4, 4, 4, 8, 1024], [0, 1, 3, 4, 5, 1023], 1044),
    "planar": (True, False, [0, 0, 8, 12, 36, 52], [0, 8, 4, 24, 16, 3072], [0, 1, 3, 4, 5, 1023], 3124),
}
FORMS = sorted(WANT)


def _inline_layout(totals, chans, planar, mono):
    """(offs, ends, strides, total) as decode_files_to_device computed them inline, from the index pass's floats per file."""
    n = len(totals)
    per_ch = [int(totals[i]) // max(int(chans[i]), 1) for i in range(n)]
    if mono:
        totals = np.asarray(per_ch, np.int64)
    strides = [(t + 3) & ~3 for t in per_ch]
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([int(chans[i]) * strides[i] for i in range(n)] if planar else strides if mono else totals)
    ends = [int(offs[i]) + int(totals[i]) for i in range(n)]
    return [int(o) for o in offs[:n]], ends, strides, int(offs[-1])


@pytest.mark.parametrize("form", FORMS)
def test_plan_against_the_table(form):
    """Offsets, reserved sizes, counts and the total of the six files; interleaved slots abut, mono and planar slots start on
    multiples of four; the inline expressions of old give the same offsets, ends and strides; a slot cannot be changed."""
    from nvorbis_amd import corpus
    planar, mono, offs, reserved, counts, total = WANT[form]
    slots, got_total = corpus._plan_slots(PER_CH, CHANS, planar, mono)
    assert got_total == total and len(slots) == len(FILES)
    assert [s.off for s in slots] == offs
    assert [s.reserved for s in slots] == reserved
    assert [s.count for s in slots] == counts
    assert [(s.per_ch, s.ch, s.stride) for s in slots] == [(p, c, st) for (p, c), st in zip(FILES, STRIDES)]
    assert all(a.off + a.reserved == b.off for a, b in zip(slots, slots[1:])) and slots[-1].off + slots[-1].reserved == total
    if form == "interleaved":
        assert all(a.off + a.count == b.off for a, b in zip(slots, slots[1:]))
    else:
        assert all(s.off % 4 == 0 for s in slots)
    old_offs, old_ends, old_strides, old_total = _inline_layout([p * c for p, c in FILES], CHANS, planar, mono)
    assert (old_offs, old_strides, old_total) == (offs, STRIDES, total)
    if not planar:  # (the planar pass counted a file from 0 to its samples per channel; there was no end)
        assert [s.off + s.count for s in slots] == old_ends
    with pytest.raises(AttributeError):
        slots[1].off = 4


@pytest.mark.parametrize("form", FORMS)
def test_plan_of_no_files(form):
    from nvorbis_amd import corpus
    planar, mono = WANT[form][:2]
    assert corpus._plan_slots([], [], planar, mono) == ([], 0)


@pytest.mark.parametrize("form", FORMS)
def test_views_on_a_cpu_tensor(form):
    """Every slot's view of arange(total): shape, strides, storage offset and first element; a file without samples is an empty
    view, not an error."""
    import torch
    from nvorbis_amd import corpus
    planar, mono, offs, _, counts, total = WANT[form]
    slots, _ = corpus._plan_slots(PER_CH, CHANS, planar, mono)
    t = torch.arange(total, dtype=torch.float32)
    for s, (per, ch), off, count, stride in zip(slots, FILES, offs, counts, STRIDES):
        v = s.view(t)
        if planar:
            assert tuple(v.shape) == (ch, per)
            if per:  # (a view without elements has no stride to speak of: torch reports (1, 1) for the file of 0 samples)
                assert v.stride() == (stride, 1)
                assert [float(v[c, 0]) for c in range(ch)] == [off + c * stride for c in range(ch)]
                assert float(v[ch - 1, per - 1]) == off + (ch - 1) * stride + per - 1 < total
        else:
            assert tuple(v.shape) == (count,) and v.stride() == (1,)
            if count:
                assert float(v[0]) == off and float(v[-1]) == off + count - 1
        assert v.storage_offset() == off and (not v.numel() or v.data_ptr() == t.data_ptr() + 4 * off)
    if planar:
        v = slots[5].view(t)
        assert tuple(v.shape) == (3, 1023) and v.stride() == (1024, 1) and float(v[0, 0]) == 52
        assert tuple(slots[0].view(t).shape) == (1, 0)
    else:
        assert tuple(slots[0].view(t).shape) == (0,)


@pytest.mark.parametrize("form", FORMS)
def test_synth_arguments_on_a_cpu_tensor(form):
    """Behind k units of progress the next synth_device call writes at base + 4 * (off + k): with the capacity count - k
    (interleaved, mono), or with the slot's plane stride and no capacity (planar)."""
    import torch
    from nvorbis_amd import corpus
    planar, mono, offs, _, counts, total = WANT[form]
    slots, _ = corpus._plan_slots(PER_CH, CHANS, planar, mono)
    base = torch.zeros(total, dtype=torch.float32).data_ptr()
    for s, off, count, stride in zip(slots, offs, counts, STRIDES):
        for k in sorted({0, 1, count // 2, count}):
            if k > count:
                continue
            want = (base + 4 * (off + k), 0, stride) if planar else (base + 4 * (off + k), count - k, None)
            assert s.synth_args(base, k) == want, (form, off, k)


# ---------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------

POISON = 0x5A5A5A5A
_FILE = []


def _short_file(ogg_bytes):
    """One two-channel stream of 60 packets (the headers of 3test.ogg): (bytes, checked packet list, samples per channel)."""
    if not _FILE:
        import nvorbis_amd as nv
        from nvorbis_amd import reader
        data, _ = _stream(ogg_bytes, seed=5, frames=60, page_packets=4)
        pa = reader.demux_ogg_array(data)
        st = nv.Stream(None, pa[0], pa[1], pa[2])
        try:
            per, ch = int(st.index_total(pa, 3)), st.channels
        finally:
            st.close()
        assert ch == 2 and per > 2048 and len(pa) == 63
        _FILE.append((data, pa, per))
    return _FILE[0]


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_a_slot_too_short_is_refused_before_the_write(ogg_bytes, gpu_ctx, form, gpu_parse):
    """_decode_into with a slot planned one sample per channel short, in a tensor that holds the whole file and more: the batch
    that would pass the slot's end raises "produces more than" and the tensor keeps its poison from the slot's end on.  With
    the right slot the view is VorbisReader.read_all() of that form, bit for bit, and the poison stands behind the slot."""
    import torch
    import nvorbis_amd as nv
    from nvorbis_amd import corpus
    planar, mono = WANT[form][:2]
    data, pa, per = _short_file(ogg_bytes)
    (short,), _ = corpus._plan_slots([per - 1], [2], planar, mono)
    (right,), size = corpus._plan_slots([per], [2], planar, mono)
    assert short.count < right.count and short.reserved <= right.reserved == size

    def poisoned():
        t = torch.full((size + 64,), POISON, dtype=torch.int32, device="cuda:0").view(torch.float32)
        torch.cuda.synchronize()  # (filled on torch's stream, written by the context's)
        return t

    t = poisoned()
    with pytest.raises(RuntimeError, match=r"file 7 produces more than the %d %s its index says" % (
            short.count, "samples per channel" if planar else "floats")):
        corpus._decode_into(gpu_ctx, pa, short, t.data_ptr(), 7, batch_frames=16, gpu_parse=gpu_parse)
    gpu_ctx.synchronize()
    end = short.reserved if planar else short.count
    assert bool((t.view(torch.int32)[end:] == POISON).all())
    assert bool((t.view(torch.int32)[:end] != POISON).any())  # (the batches in front of the refused one were written)

    t = poisoned()
    corpus._decode_into(gpu_ctx, pa, right, t.data_ptr(), 7, batch_frames=16, gpu_parse=gpu_parse)
    gpu_ctx.synchronize()
    got = right.view(t).contiguous().cpu().numpy()
    rd = nv.VorbisReader(data, ctx=gpu_ctx, layout="planar" if planar else "interleaved", mix="mono" if mono else None)
    try:
        want = rd.read_all()
    finally:
        rd.close()
    assert want.shape == ((2, per) if planar else (per,) if mono else (2 * per,))
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert bool((t.view(torch.int32)[size:] == POISON).all())

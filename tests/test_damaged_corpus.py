"""Damaged Ogg files through the corpus pass (nvorbis_amd/corpus.py): the lacing-only index against the checked demultiplexer on
the host, then decode_files_to_device, transcode on its host and its device route and the gather's flat payload on the GPU.

A file takes one of four routes through decode_files_to_device: ARENA (index and checked list agree in packet count and payload:
decoded into its slot of the arena), RE-INDEXED (they differ: a tensor of its own), INDEX FALLBACK (the index refuses the file,
the checked list sizes its slot: arena) or REFUSED (the checked demultiplexer refuses it: the call raises).  Every PCM comparison
is uint32 equality with oracle.decode_ogg of the same damaged bytes; there is no tolerance anywhere."""
import threading

import numpy as np
import pytest

from tests import c5_corpus, ogg_py, vorbis_encode as ve
from tests.test_ogg_damage import _damage, _stream

CRC_VALID_KINDS = ("drop", "junk", "seq", "truncate")
# byte ranges of an Ogg page header's fields (RFC 3533 section 6); the lacing values follow at 27
FIELDS = {"capture": (0, 4), "version": (4, 5), "flags": (5, 6), "granule": (6, 14), "serial": (14, 18), "seq": (18, 22), "crc": (22, 26),
          "nseg": (26, 27)}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# what the two host readers make of a file
# ---------------------------------------------------------------------------------------------------------------------------

def _floats(pa):
    """Floats the serial decoder emits for a packet list (Stream.index_total x channels): what sizes a file's arena slot."""
    import nvorbis_amd as nv
    st = nv.Stream(None, pa[0], pa[1], pa[2])
    try:
        return int(st.index_total(pa, 3)) * st.channels
    finally:
        st.close()


def look(data):
    """(index, checked): per reader the error code it refuses the file with, or (PacketArray, payload bytes, floats)."""
    from nvorbis_amd import native, reader
    try:
        pa, payload = reader.index_ogg_array(data)
        idx = (pa, int(payload), _floats(pa))
    except native.NvhError as e:
        idx = e.code
    try:
        pb = reader.demux_ogg_array(data)
        chk = (pb, int(pb.offsets[-1]), _floats(pb))
    except native.NvhError as e:
        chk = e.code
    return idx, chk


def shape_of(seen):
    return (len(seen[0]), seen[1])


def route_of(idx, chk):
    """The route decode_files_to_device must send the file: "refused", "fallback", "arena" or "redo"."""
    if isinstance(chk, int):
        return "refused"
    if isinstance(idx, int):
        return "fallback"
    return "arena" if shape_of(idx) == shape_of(chk) else "redo"


def slot_floats(idx, chk):
    """The size of the file's arena slot: the index's count, the checked list's where the index refused."""
    return chk[2] if isinstance(idx, int) else idx[2]


def assert_lists_agree(idx, chk, what):
    """Index and checked list of one file: the same packets in count, payload, granule positions, flags and emitted samples, the
    headers whole and every audio packet's head (the index keeps up to 8 bytes of each)."""
    pa, pb = idx[0], chk[0]
    n = len(pa)
    assert n == len(pb) and idx[1] == chk[1] and idx[2] == chk[2], (what, n, len(pb), idx[1:], chk[1:])
    assert np.array_equal(pa.granules[:n], pb.granules[:n]) and np.array_equal(pa.flags[:n], pb.flags[:n]), what
    assert [pa[i] for i in range(3)] == [pb[i] for i in range(3)], what
    assert all(pa[i] == pb[i][:8] for i in range(3, n)), what


def flip(data, pages, k, byte, bit):
    buf = bytearray(data)
    buf[pages[k]["offset"] + byte] ^= bit
    return bytes(buf)


def header_flips(pages):
    """(page, byte, bit, field) for bits 0x01 and 0x80 of every header and lacing byte of every audio page."""
    for k in range(2, len(pages)):
        for byte in range(27 + len(pages[k]["segs"])):
            field = next((f for f, (a, b) in FIELDS.items() if a <= byte < b), "lacing")
            for bit in (0x01, 0x80):
                yield k, byte, bit, field


def lacing_dense_file(ogg_bytes):
    """The three headers of 3test.ogg and 1500 one-byte audio packets, 255 to a page: 7535 bytes hold 1503 packets, more than the
    index's first guess of a packet per 48 bytes (220)."""
    hdr = ve.shipped_headers(ogg_bytes["3test"])
    pk = list(hdr) + [bytes([0x00 if i % 7 else 0x0E]) for i in range(1500)]
    data = ogg_py.write_ogg(pk, [0, 0, 0] + [-1] * 1500, page_packets=255)
    assert len(data) == 7535 and len(data) // 48 + 64 == 220
    return data


# ---------------------------------------------------------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", CRC_VALID_KINDS + ("swap",))
def test_index_and_checked_list_agree_on_crc_valid_damage(ogg_bytes, kind):
    """A dropped page, junk between pages, a sequence jump and a cut file leave every remaining page's checksum valid: the
    lacing-only index sees the packets the checked demultiplexer sees (such a file keeps its arena slot).  Two exchanged pages
    make the granule position regress: both readers refuse the file with the same code."""
    from nvorbis_amd import native
    rng = np.random.default_rng(sum(kind.encode()))
    for trial in range(6):
        data, pages = _stream(ogg_bytes, seed=trial + 1, page_packets=int(rng.integers(1, 6)))
        idx, chk = look(_damage(data, pages, kind, rng))
        if kind == "swap":
            assert idx == chk == native.ERR_INVALID_DATA, (trial, idx, chk)
            continue
        assert not isinstance(idx, int) and not isinstance(chk, int), (kind, trial, idx, chk)
        assert_lists_agree(idx, chk, (kind, trial))


def test_a_failed_checksum_changes_the_shape(ogg_bytes):
    """A flipped body bit: the checked demultiplexer drops the page, the index does not look -- count and payload differ, which is
    what the corpus pass finds the file by."""
    rng = np.random.default_rng(11)
    for trial in range(6):
        data, pages = _stream(ogg_bytes, seed=trial + 1, page_packets=int(rng.integers(1, 6)))
        idx, chk = look(_damage(data, pages, "crc", rng))
        assert route_of(idx, chk) == "redo" and len(chk[0]) < len(idx[0]) and chk[1] < idx[1], (trial, shape_of(idx), shape_of(chk))


def test_header_flips_take_one_of_three_routes(ogg_bytes):
    """Bits 0x01 and 0x80 of every header and lacing byte of every audio page of one stream (40 frames, four packets a page):
    equal shapes imply equal sample counts (else the arena slot would be wrong and nothing would notice before the decode);
    where the index raises, the checked demultiplexer decides and the index pass sizes the file from it; and every route --
    agree, shapes differ, index refuses -- occurs."""
    from nvorbis_amd import corpus
    data, pages = _stream(ogg_bytes, seed=3, frames=40, page_packets=4)
    flips = list(header_flips(pages))
    assert 700 <= len(flips) <= 1000, len(flips)
    files = [flip(data, pages, k, byte, bit) for k, byte, bit, _ in flips]
    seen = [look(f) for f in files]
    routes = {}
    for (k, byte, bit, field), (idx, chk) in zip(flips, seen):
        r = route_of(idx, chk)
        routes.setdefault(r, set()).add(field)
        if r == "arena":
            assert idx[2] == chk[2], ("equal shapes, other sample counts", k, byte, bit, idx[2], chk[2])
            assert np.array_equal(idx[0].granules, chk[0].granules) and np.array_equal(idx[0].flags, chk[0].flags), (k, byte, bit)
    assert set(routes) >= {"arena", "redo", "fallback"}, {r: sorted(f) for r, f in routes.items()}
    assert "granule" in routes["fallback"] and {"flags", "seq", "crc", "nseg", "lacing", "version"} <= routes["redo"]
    # the product's own index pass over all of them: a file only the checked demultiplexer takes is sized from its list
    accepted = [i for i, (_, chk) in enumerate(seen) if not isinstance(chk, int)]
    shape, totals, chans, errors = corpus._index_pass([files[i] for i in accepted], 4)
    assert not errors, errors[:3]
    for j, i in enumerate(accepted):
        idx, chk = seen[i]
        assert shape[j] == shape_of(chk if isinstance(idx, int) else idx), (flips[i], shape[j])
        assert totals[j] == slot_floats(idx, chk) and chans[j] == 2, (flips[i], totals[j])
    refused = [files[i] for i, (_, chk) in enumerate(seen) if isinstance(chk, int)]
    if refused:
        assert len(corpus._index_pass(refused, 2)[3]) == len(refused)


def _on_a_fresh_thread(fn):
    """fn() on a thread of its own (index_ogg_array keeps its scratch arrays per thread): its result, or its exception raised."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001 -- handed to the caller's thread
            box["error"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_lacing_dense_file_takes_the_retry(ogg_bytes, oracle, monkeypatch):
    """1503 packets in 7535 bytes: the first call has room for 220 and reports what it needs, the second has it.  On a thread
    whose scratch is fresh two calls run, behind a file that grew the scratch one; both give the checked list.  If the second
    call reports too little room as well, index_ogg_array raises: no truncated PacketArray."""
    import nvorbis_amd as nv
    from nvorbis_amd import native, reader
    data = lacing_dense_file(ogg_bytes)
    chk = reader.demux_ogg_array(data)
    assert (len(chk), int(chk.offsets[-1]), _floats(chk)) == (1503, 5800, 2 * 383616)
    pcm, _ = oracle.decode_ogg(data)
    assert pcm.size == 767232 and not pcm.any()
    L = nv.lib()
    real = L.nvh_ogg_index_packets
    calls = []

    def counted(*args):
        calls.append(args[8])  # the packet capacity offered
        return real(*args)

    monkeypatch.setattr(L, "nvh_ogg_index_packets", counted)

    def both_agree():
        pa, payload = reader.index_ogg_array(data)
        assert_lists_agree((pa, int(payload), _floats(pa)), (chk, int(chk.offsets[-1]), _floats(chk)), "lacing-dense")
        return len(calls)

    assert _on_a_fresh_thread(both_agree) == 2 and calls[0] < 1503 <= calls[1], calls
    big, _ = _stream(ogg_bytes, seed=2, frames=90, page_packets=4)
    assert len(big) // 48 + 64 > 1503

    def behind_a_large_file():
        reader.index_ogg_array(big)
        del calls[:]
        return both_agree()

    assert _on_a_fresh_thread(behind_a_large_file) == 1 and calls[0] >= 1503, calls

    def short_of_room(*args):  # every call reports more packets than it was offered
        rc = real(*args)
        assert rc in (native.OK, native.ERR_ARGUMENT)
        args[9]._obj.value = args[8] + 1
        return native.ERR_ARGUMENT

    monkeypatch.setattr(L, "nvh_ogg_index_packets", short_of_room)
    with pytest.raises(native.NvhError) as e:
        _on_a_fresh_thread(lambda: reader.index_ogg_array(data))
    assert e.value.code == native.ERR_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------------
# on the GPU: one list of files through every route
# ---------------------------------------------------------------------------------------------------------------------------

# damage kind or header-flip class -> the route it must take (the header flips: on a middle page and on the last page)
WANT_ROUTE = {"healthy": "arena", "shipped": "arena", "dense": "arena", "crc": "redo", "drop": "arena", "junk": "arena", "seq": "arena",
              "truncate": "arena", "granule": "fallback", "lacing": "redo", "nseg": "redo", "flags": "redo", "swap": "refused"}
ORDER = ["crc", "healthy", "healthy", "drop", "healthy", "junk", "healthy", "granule:mid", "lacing:mid", "nseg:mid", "healthy", "seq",
         "healthy", "flags:mid", "healthy", "dense", "healthy", "truncate", "granule:last", "healthy", "lacing:last", "healthy",
         "nseg:last", "healthy", "swap", "shipped", "shipped", "shipped", "shipped", "healthy", "flags:last"]
_LIST = []


def header_flip_of(data, pages, field, k):
    """The first one-bit flip of `field` on page k that takes the class's route (a segment count that grows on the last page, say,
    makes both readers drop the page: that one agrees)."""
    a, b = FIELDS.get(field, (27, 27 + len(pages[k]["segs"])))
    for byte in range(a, b):
        for bit in (0x01, 0x80, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40):
            bad = flip(data, pages, k, byte, bit)
            if route_of(*look(bad)) == WANT_ROUTE[field]:
                return bad
    raise AssertionError("no %s flip on page %d takes the route %s" % (field, k, WANT_ROUTE[field]))


def corpus_list(oracle, ogg_bytes):
    """The files of ORDER without what the oracle refuses: dicts of the label, the bytes, what the host readers see of them, the
    route and the oracle's PCM.  Built once, shared, never modified."""
    if _LIST:
        return _LIST[0]
    ws = c5_corpus.writer_setup()
    rng = np.random.default_rng(29)
    healthy = iter(c5_corpus.corpus_file(ws, i, 0.02) for i in range(100, 100 + ORDER.count("healthy")))
    shipped = iter(ogg_bytes[n] for n in c5_corpus.SHIPPED)
    out, left_out = [], []
    for n, label in enumerate(ORDER):
        kind, _, where = label.partition(":")
        if kind == "healthy":
            data = next(healthy)
        elif kind == "shipped":
            data = next(shipped)
        elif kind == "dense":
            data = lacing_dense_file(ogg_bytes)
        else:
            per_page = 1 + n % 5  # (whole pages: the last page holds as many packets as a middle one)
            base, pages = _stream(ogg_bytes, seed=40 + n, frames=60 + per_page * (n % 4), page_packets=per_page)
            if where:
                data = header_flip_of(base, pages, kind, len(pages) // 2 if where == "mid" else len(pages) - 1)
            else:
                data = _damage(base, pages, kind, rng)
        idx, chk = look(data)
        try:
            pcm, info = oracle.decode_ogg(data)
        except RuntimeError:
            left_out.append(label)
            assert route_of(idx, chk) == "refused", label
            continue
        pcm.setflags(write=False)
        out.append(dict(label=label, data=data, idx=idx, chk=chk, route=route_of(idx, chk), pcm=pcm))
        assert out[-1]["route"] == WANT_ROUTE[kind], (label, out[-1]["route"])
        assert pcm.size == chk[2], (label, pcm.size, chk[2])  # the checked list's sample count is the oracle's
    assert left_out == ["swap"], left_out  # the oracle takes every other file: nothing else is left out of the list
    assert len(out) == len(ORDER) - 1 == 30
    redo = [i for i, f in enumerate(out) if f["route"] == "redo"]
    assert redo[0] == 0 and redo[-1] == len(out) - 1 and any(b == a + 1 for a, b in zip(redo, redo[1:])), redo
    assert any(f["route"] == "fallback" for f in out)
    _LIST.append(out)
    return out


def _assert_all_pcm(got, lst, what):
    """Every array or tensor of `got` is the oracle's PCM of its file; the failure names every file that is not."""
    assert len(got) == len(lst), (what, len(got), len(lst))
    bad = []
    for i, (g, f) in enumerate(zip(got, lst)):
        g = (g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)).reshape(-1)
        want = f["pcm"]
        if g.size != want.size:
            bad.append("file %d (%s): %d floats, the oracle has %d" % (i, f["label"], g.size, want.size))
        elif not same_bits(g, want):
            differ = np.nonzero(g.view(np.uint32) != want.view(np.uint32))[0]
            bad.append("file %d (%s): %d of %d floats differ, the first at %d" % (i, f["label"], differ.size, want.size, differ[0]))
    assert not bad, "%s: %d of %d files are not the oracle's PCM:\n%s" % (what, len(bad), len(lst), "\n".join(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_device_arena(oracle, ogg_bytes, gpu_parse):
    """decode_files_to_device over the list: exactly the files whose index shape differs from the checked one are decoded again,
    every view is the oracle's PCM, and the others are where the index pass put them: slices of the arena, slot behind slot."""
    from nvorbis_amd import corpus
    lst = corpus_list(oracle, ogg_bytes)
    t = {}
    arena, views = corpus.decode_files_to_device([f["data"] for f in lst], device=0, workers=4, gpu_parse=gpu_parse, timings=t)
    redo = [i for i, f in enumerate(lst) if f["route"] == "redo"]
    assert t.get("files_reindexed") == redo
    _assert_all_pcm(views, lst, "decode_files_to_device, gpu_parse=%s" % gpu_parse)
    slots = [slot_floats(f["idx"], f["chk"]) for f in lst]
    offs = np.concatenate([[0], np.cumsum(slots)])
    assert int(arena.numel()) == int(offs[-1])
    lo, hi = arena.data_ptr(), arena.data_ptr() + 4 * int(arena.numel())
    for i, (f, v) in enumerate(zip(lst, views)):
        if i in redo:
            assert not lo <= v.data_ptr() < hi, (i, f["label"])
        else:
            assert v.data_ptr() == lo + 4 * int(offs[i]) and v.numel() == slots[i], (i, f["label"])
    assert views[0].numel() != slots[0]  # (a tensor of its own with another length than its slot: what a running offset trips over)


@pytest.mark.gpu
def test_transcode_host_route(oracle, ogg_bytes):
    """transcode with its defaults (the host exchange, one rank): every returned array is the oracle's PCM -- behind a re-indexed
    file too, whose own PCM is not in the arena and whose arena slot has another length.

    Before corpus._views_to_host the read-back was cut at a running offset of the views' lengths: file 0 (a failed checksum) came
    back as the first floats of its stale arena slot, and every file behind it was cut from a shifted place."""
    from nvorbis_amd import corpus
    lst = corpus_list(oracle, ogg_bytes)
    out = corpus.transcode([f["data"] for f in lst])
    assert len(out) == len(lst) and all(isinstance(o, np.ndarray) and o.dtype == np.float32 for o in out)
    _assert_all_pcm(out, lst, "transcode, host route")


@pytest.mark.gpu
def test_transcode_device_route(oracle, ogg_bytes):
    """transcode(device="cuda:0", to_host=False): every tensor is the oracle's PCM, on the device."""
    from nvorbis_amd import corpus
    lst = corpus_list(oracle, ogg_bytes)
    out = corpus.transcode([f["data"] for f in lst], device="cuda:0", to_host=False)
    assert len(out) == len(lst) and all(o.is_cuda for o in out)
    _assert_all_pcm(out, lst, "transcode, device route")


@pytest.mark.gpu
def test_flat_payload(oracle, ogg_bytes):
    """The gather's payload of a rank (corpus._flat_payload): with re-indexed files among the views it is the files' PCM back to
    back, copied; without one it is the arena itself, no copy."""
    import torch
    from nvorbis_amd import corpus
    lst = corpus_list(oracle, ogg_bytes)
    dev = torch.device("cuda:0")
    arena, views = corpus.decode_files_to_device([f["data"] for f in lst], device=0, workers=4)
    flat = corpus._flat_payload([v.reshape(-1) for v in views], torch, dev)
    want = np.concatenate([f["pcm"] for f in lst])
    assert flat.is_contiguous() and same_bits(flat.cpu().numpy(), want)
    assert any(f["route"] == "redo" for f in lst[1:-1])
    rest = [f for f in lst if f["route"] != "redo"]
    t = {}
    arena, views = corpus.decode_files_to_device([f["data"] for f in rest], device=0, workers=4, timings=t)
    assert "files_reindexed" not in t
    flat = corpus._flat_payload([v.reshape(-1) for v in views], torch, dev)
    assert flat.data_ptr() == arena.data_ptr() and flat.numel() == arena.numel()
    assert same_bits(flat.cpu().numpy(), np.concatenate([f["pcm"] for f in rest]))


@pytest.mark.gpu
def test_a_refused_file_fails_the_call_and_nothing_else(oracle, ogg_bytes):
    """Two exchanged pages between healthy files: decode_files_to_device raises RuntimeError naming the file's index; the next call
    of the process, on the healthy files alone, gives the oracle's PCM, and the kept worker contexts close."""
    from nvorbis_amd import corpus
    lst = corpus_list(oracle, ogg_bytes)
    healthy = [f for f in lst if f["label"] == "healthy"][:4]
    base, pages = _stream(ogg_bytes, seed=7, frames=40, page_packets=3)
    swap = _damage(base, pages, "swap", np.random.default_rng(7))
    with pytest.raises(RuntimeError):
        oracle.decode_ogg(swap)
    files = [f["data"] for f in healthy]
    with pytest.raises(RuntimeError, match=r"index failed for files \[2\]"):
        corpus.decode_files_to_device(files[:2] + [swap] + files[2:], device=0, workers=4, keep_contexts=True)
    try:
        arena, views = corpus.decode_files_to_device(files, device=0, workers=4, keep_contexts=True)
        _assert_all_pcm(views, healthy, "behind a refused file")
        assert all(views[i].data_ptr() + 4 * views[i].numel() == views[i + 1].data_ptr() for i in range(len(views) - 1))
    finally:
        corpus.close_worker_contexts()
    assert not corpus._WORKER_CONTEXTS

"""The PCM output descriptor (nvh_pcm_out) behind every synthesis entry point.

nvh_stream_synth_out / nvh_stream_synth_begin_out / nvh_batch_synth_out take one descriptor; the 18 named synthesis calls are
shorthands that fill one.  Two things are pinned here:

  * CPU: the result codes of the named calls on host-only streams -- which argument error wins, and whether *written /
    *expected was cleared -- are those of tests/golden/synth_arg_codes.json, a table recorded from the commit it names with
    tools/gen_synth_arg_codes.py BEFORE the descriptor existed; the descriptor call with the equivalent descriptor gives the same.
  * GPU: every named call, invoked directly, returns the code, the count and the bytes of the descriptor call (the Python
    surface only uses the descriptor calls, so nothing else would notice a named call that drifts).

Nothing numeric changes between the two forms: every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TABLE = os.path.join(GOLDEN, "synth_arg_codes.json")

SYNC = ("nvh_stream_synth", "nvh_stream_synth_pcm", "nvh_stream_synth_planar", "nvh_stream_synth_mix", "nvh_stream_synth_map",
        "nvh_stream_synth_planar_map")
BEGIN = ("nvh_stream_synth_begin", "nvh_stream_synth_begin_pcm", "nvh_stream_synth_begin_planar", "nvh_stream_synth_begin_mix",
         "nvh_stream_synth_begin_map", "nvh_stream_synth_begin_planar_map")
BATCH = ("nvh_batch_synth", "nvh_batch_synth_pcm", "nvh_batch_synth_planar", "nvh_batch_synth_mix", "nvh_batch_synth_map",
         "nvh_batch_synth_planar_map")
NAMED = SYNC + BEGIN + BATCH
OUT = ("nvh_stream_synth_out", "nvh_stream_synth_begin_out", "nvh_batch_synth_out")
UNSET = -12345  # what *written / *expected holds before each call of the sweep

# the streams of the sweep: (source, audio packets pushed).  All host-only; every existing CPU test builds them the same way.
STREAMS = {
    "stereo": ("3test", 9),           # pending frames with PCM to write
    "stereo_empty": ("3test", 0),     # nothing pending
    "stereo_first": ("3test", 1),     # the first audio packet alone: one pending frame that emits nothing
    "mono": ("mono_res1_2048", 12),
    "six": ("six_ch_res2_4096", 12),
    "nine": ("ch9_res2", 12),
}


def form(name):
    """(planar, mix, map) of a named call: which of its arguments exist."""
    return "planar" in name, name.endswith("_mix"), name.endswith("_map")


def open_host_stream(nv, oracle, ogg_bytes, key):
    source, packets = STREAMS[key]
    if source == "3test":
        pk, gr, fl = nv.demux_ogg(ogg_bytes["3test"])
        pk, gr, fl = pk[:3 + packets], [-1] * (3 + packets), [0] * (3 + packets)
    else:
        from tests import synth_stream as ss
        pk, gr, fl = ss.filtered_stream(oracle, source, packets, 3)
    st = nv.Stream(None, pk[0], pk[1], pk[2])
    for i in range(3, len(pk)):
        st.push_packet(pk[i], int(gr[i]), int(fl[i]))
    return st


def _dest(dest, buf):
    """(pcm_host, d_pcm) of a cell's destination: the pair itself, or "host", "dev+K" (the made-up device address 4096 + K: a host-only stream never
    touches it), "both", "neither"."""
    if isinstance(dest, tuple):  # (the GPU test: real addresses)
        return dest
    host = buf.ctypes.data if dest in ("host", "both") else None
    dev = C.c_void_p(4096 + int(dest[4:])) if dest.startswith("dev+") else C.c_void_p(4096) if dest == "both" else None
    return host, dev


def call_named(L, handle, cell, buf):
    """One cell through its named call: (code, *written or *expected afterwards, UNSET where the call left it alone)."""
    name, fmt, mix, cmap, oc, dest, extent = cell
    planar, has_mix, has_map = form(name)
    host, dev = _dest(dest, buf)
    wr = C.c_int64(UNSET)
    args = [handle]
    if not name.endswith(("nvh_stream_synth", "nvh_stream_synth_begin", "nvh_batch_synth")):
        args.append(fmt)
    if has_mix:
        args.append(mix)
    if has_map:
        args += [(C.c_int32 * max(len(cmap), 1))(*cmap) if cmap is not None else None, oc]
    if name in SYNC:
        args += [host, dev, extent, C.byref(wr)]
    elif name in BEGIN:
        args += [host, extent, C.byref(wr)]
    else:
        args += [dev, extent]
    return getattr(L, name)(*args), wr.value


def descriptor(native, cell):
    """(the named call whose recorded result the descriptor call must reproduce, the descriptor made of the cell's arguments).
    That call is the cell's own, except where a named call asks for more than a descriptor can say -- there it is the twin
    whose descriptor it fills: a *_mix call with NVH_MIX_NONE checks its capacity before the device like every mix call, where
    the same descriptor coming from the *_pcm call checks it after (the parent's difference, kept); a *_map call always asks
    for a map, where a descriptor with out_channels == 0 asks for none (the *_pcm / *_planar call)."""
    name, fmt, mix, cmap, oc, dest, extent = cell
    planar, has_mix, has_map = form(name)
    if has_mix and mix == native.MIX_NONE:
        name = name[:-len("_mix")] + "_pcm"
    elif has_map and oc == 0:
        name, cmap = (name[:-len("_map")] if planar else name[:-len("_map")] + "_pcm"), None
    arr = (C.c_int32 * max(len(cmap), 1))(*cmap) if has_map and cmap is not None else None
    return name, native.PcmOut(format=fmt, mix=mix if has_mix else native.MIX_NONE, planar=int(planar),
                               out_channels=oc if has_map else 0, map=arr, extent=extent)


def call_out(L, handle, name, d, dest, buf):
    """A descriptor through the descriptor call of the kind of `name`."""
    host, dev = _dest(dest, buf)
    wr = C.c_int64(UNSET)
    if name in SYNC:
        rc = L.nvh_stream_synth_out(handle, C.byref(d), host, dev, C.byref(wr))
    elif name in BEGIN:
        rc = L.nvh_stream_synth_begin_out(handle, C.byref(d), host, C.byref(wr))
    else:
        rc = L.nvh_batch_synth_out(handle, C.byref(d), dev)
    return rc, wr.value


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------

def test_descriptor_calls_are_exported_and_declared():
    import re
    from nvorbis_amd import native
    L = native.lib()
    hdr = open(os.path.join(ROOT, "include", "nvorbis_hip.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "NativeMethods.cs")).read()
    for name in NAMED + OUT:
        assert hasattr(L, name), name
        assert name in native.SIGNATURES, name
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
    for name in OUT:
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern (?:unsafe )?int %s\(" % name, cs), name
    assert "nvh_stream_synth_out(" in open(os.path.join(ROOT, "csharp", "GpuStreamDecoder.cs")).read()
    # the struct as the header lays it out: four int32, a pointer, an int64
    assert [f[0] for f in native.PcmOut._fields_] == ["format", "mix", "planar", "out_channels", "map", "extent"]
    assert C.sizeof(native.PcmOut) == 32 and native.PcmOut.map.offset == 16 and native.PcmOut.extent.offset == 24


def test_result_codes_are_the_recorded_ones(oracle, ogg_bytes):
    """Every cell of the recorded table: the named call returns the recorded code and leaves *written / *expected as recorded,
    and the descriptor call with the equivalent descriptor does the same."""
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    table = json.load(open(TABLE))
    assert table["recorded_from"] and 200 <= len(table["cells"]) <= 1000
    buf = np.zeros(1 << 18, np.float32)
    recorded = {json.dumps(row[:8]): (row[8], row[9]) for row in table["cells"]}
    seen_calls, own, twin = set(), 0, 0
    for key in ["null"] + list(STREAMS):
        st = open_host_stream(nv, oracle, ogg_bytes, key) if key != "null" else None
        try:
            if st is not None:
                assert [st.channels, st.pending()[1]] == table["streams"][key], key  # the cells' extents were sized for these
            handle = st._h if st is not None else None
            for row in table["cells"]:
                if row[0] != key:
                    continue
                cell, want = row[1:8], (row[8], row[9])
                assert call_named(L, handle, cell, buf) == want, row
                seen_calls.add(cell[0])
                name, d = descriptor(native, cell)
                if name != cell[0]:  # the descriptor is the twin's: the twin's recorded result, where the table has that cell
                    want = recorded.get(json.dumps([key, name, cell[1], 0, None, 0, cell[5], cell[6]]))
                    twin += want is not None
                else:
                    own += 1
                if want is not None:
                    assert call_out(L, handle, name, d, cell[5], buf) == want, (row, name)
        finally:
            if st is not None:
                st.close()
    assert seen_calls == set(NAMED)
    assert own >= 500 and twin >= 40, (own, twin)


def test_descriptors_no_named_call_can_express_are_refused(oracle, ogg_bytes):
    """A null descriptor, a mix together with the planar layout or with a map, a layout flag that is neither 0 nor 1:
    NVH_ERR_ARGUMENT from all three calls, before anything needs a device, with *written / *expected left alone."""
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    buf = np.zeros(1 << 18, np.float32)
    st = open_host_stream(nv, oracle, ogg_bytes, "six")
    try:
        n = st.pending()[1]
        wave = (C.c_int32 * 6)(0, 2, 1, 5, 3, 4)
        bad = [None,
               native.PcmOut(mix=native.MIX_MONO, planar=1, extent=n),
               native.PcmOut(mix=native.MIX_MONO, out_channels=6, map=wave, extent=6 * n),
               native.PcmOut(planar=2, extent=n), native.PcmOut(planar=-1, extent=n)]
        for d in bad:
            ref = C.byref(d) if d is not None else None
            for handle in (st._h, None):
                wr = C.c_int64(UNSET)
                assert L.nvh_stream_synth_out(handle, ref, buf.ctypes.data, None, C.byref(wr)) == native.ERR_ARGUMENT
                assert L.nvh_stream_synth_begin_out(handle, ref, buf.ctypes.data, C.byref(wr)) == native.ERR_ARGUMENT
                assert wr.value == UNSET
            assert L.nvh_batch_synth_out(None, ref, None) == native.ERR_ARGUMENT
        # the same descriptors without the offending field pass the argument checks
        for d in (native.PcmOut(mix=native.MIX_MONO, extent=n), native.PcmOut(planar=1, extent=n),
                  native.PcmOut(out_channels=6, map=wave, extent=6 * n)):
            wr = C.c_int64(UNSET)
            assert L.nvh_stream_synth_out(st._h, C.byref(d), buf.ctypes.data, None, C.byref(wr)) == native.ERR_NO_GPU
            assert wr.value == 0
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------

FIRST, SECOND = 12, 5  # audio packets of the two consecutive batches (the first holds a short / long block transition)
GUARD = 0xA5           # every destination is filled with this byte before a call: the comparison covers what was NOT written too


def _cells(kind, fmt, ch, cmap, n, stride):
    """The named calls of one kind (SYNC / BEGIN / BATCH) in format `fmt` for a batch of n samples per channel, as cells without
    a destination: ([name, format, mix, map, out_channels, None, extent], samples the destination must hold)."""
    out = []
    for name in kind:
        planar, has_mix, has_map = form(name)
        if name in ("nvh_stream_synth", "nvh_stream_synth_begin", "nvh_batch_synth") and fmt != 0:
            continue  # (float only)
        oc = len(cmap) if has_map else 0
        extent = stride if planar else n * oc if has_map else n if has_mix else n * ch
        room = stride * (oc or ch) if planar else extent
        out.append(([name, fmt, 1 if has_mix else 0, list(cmap) if has_map else None, oc, None, extent], max(room, 1)))
    return out


def _both(L, native, ha, hb, cell, dest_a, dest_b):
    """The cell's named call on handle ha into dest_a, the descriptor call on hb into dest_b: the (code, count) both returned."""
    a = call_named(L, ha, cell[:5] + [dest_a] + cell[6:], None)
    name, d = descriptor(native, cell)
    assert name == cell[0]
    b = call_out(L, hb, name, d, dest_b, None)
    assert a == b, (cell, a, b)
    return a


class _Pinned:
    """Page-locked host memory as a byte array."""

    def __init__(self, L, nbytes):
        self.L, self.p = L, C.c_void_p()
        assert L.nvh_pinned_alloc(nbytes, C.byref(self.p)) == 0
        self.bytes = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def free(self):
        self.bytes = None
        self.L.nvh_pinned_free(self.p)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "s16"])
@pytest.mark.parametrize("key", ["stereo", "six"])
def test_named_calls_are_their_descriptor_calls(gpu_ctx, oracle, ogg_bytes, key, fmt):
    """Each of the 18 named calls, invoked directly, against the descriptor call with the descriptor it stands for: the same code,
    the same *written / *expected, byte-identical destinations (guard bytes included).  Host and pipelined paths over two
    consecutive, unequal batches on two streams fed the same packets (the carried tail and its buffer flip are in play); the
    resident batch uploaded once, both calls on it; and the batch that emits nothing -- the stream's first audio packet alone,
    where a plane stride of 0 and a capacity of 0 are legal -- through every form."""
    import torch
    import nvorbis_amd as nv
    from nvorbis_amd import native
    L = native.lib()
    if key == "stereo":
        pk, gr, fl = nv.demux_ogg(ogg_bytes["3test"])
        cmap = (1, 0)
    else:
        from tests import synth_stream as ss
        pk, gr, fl = ss.filtered_stream(oracle, STREAMS[key][0], FIRST + SECOND, 3)
        cmap = (0, 2, 1, 5, 3, 4)
    sb = 2 if fmt else 4
    A, B = nv.Stream(gpu_ctx, pk[0], pk[1], pk[2]), nv.Stream(gpu_ctx, pk[0], pk[1], pk[2])
    ch = A.channels
    pins = []
    try:
        def push(lo, hi):
            for st in (A, B):
                for i in range(lo, hi):
                    st.push_packet(pk[i], int(gr[i]), int(fl[i]))
            frames, n = A.pending()
            assert (frames, n) == B.pending() and frames == hi - lo
            return n
        batches = ((3, 3 + FIRST), (3 + FIRST, 3 + FIRST + SECOND))

        # ---- the synchronous calls into pageable host memory, two batches ----
        for k in range(len(_cells(SYNC, fmt, ch, cmap, 0, 0))):
            A.reset(), B.reset()
            for lo, hi in batches:
                n = push(lo, hi)
                if lo == 3:
                    assert len({int(g[0]) for g in A.pending_geometry()}) == 2  # short and long blocks
                cell, room = _cells(SYNC, fmt, ch, cmap, n, n + 5)[k]
                da, db = np.full(room * sb, GUARD, np.uint8), np.full(room * sb, GUARD, np.uint8)
                rc, wr = _both(L, native, A._h, B._h, cell, (da.ctypes.data, None), (db.ctypes.data, None))
                planar, has_mix, _ = form(cell[0])
                assert rc == native.OK and wr == (n if planar or has_mix else cell[6]) and wr > 0, (cell, rc, wr)
                assert np.array_equal(da, db) and (da != GUARD).any(), cell

        # ---- the pipelined calls into page-locked memory, both batches outstanding ----
        big = (A.block1 * FIRST + 5) * ch  # (a packet emits less than a long block per channel)
        pins = [_Pinned(L, big * sb) for _ in range(4)]  # (two flights for each of the two streams)
        for k in range(len(_cells(BEGIN, fmt, ch, cmap, 0, 0))):
            A.reset(), B.reset()
            want = []
            for j, (lo, hi) in enumerate(batches):
                n = push(lo, hi)
                cell, room = _cells(BEGIN, fmt, ch, cmap, n, n + 5)[k]
                assert room <= big
                pins[j].bytes[:] = GUARD
                pins[2 + j].bytes[:] = GUARD
                rc, exp = _both(L, native, A._h, B._h, cell, (pins[j].p, None), (pins[2 + j].p, None))
                assert rc == native.OK and exp > 0, (cell, rc, exp)
                want.append(exp)
            for j in range(2):
                wa, wb = C.c_int64(UNSET), C.c_int64(UNSET)
                assert L.nvh_stream_synth_end(A._h, C.byref(wa)) == native.OK and L.nvh_stream_synth_end(B._h, C.byref(wb)) == native.OK
                assert wa.value == wb.value == want[j]
                assert np.array_equal(pins[j].bytes, pins[2 + j].bytes) and (pins[j].bytes != GUARD).any()

        # ---- the resident batch: uploaded once, both calls on it ----
        A.reset()
        for i in range(3, 3 + FIRST):
            A.push_packet(pk[i], int(gr[i]), int(fl[i]))
        b = A.upload_batch()
        try:
            n = b.samples
            assert n > 0
            for cell, room in _cells(BATCH, fmt, ch, cmap, n, n + 8):
                da = torch.full((room * sb,), GUARD, dtype=torch.uint8, device="cuda")
                db = torch.full((room * sb,), GUARD, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                rc, _ = _both(L, native, b._h, b._h, cell, (None, C.c_void_p(da.data_ptr())), (None, C.c_void_p(db.data_ptr())))
                assert rc == native.OK, cell
                gpu_ctx.synchronize()
                assert torch.equal(da, db) and bool((da != GUARD).any()), cell
        finally:
            b.free()

        # ---- the batch that emits nothing: the first audio packet alone, every form, stride 0 / capacity 0 ----
        one = np.full(sb, GUARD, np.uint8)
        dev = torch.full((16,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for kind in (SYNC, BEGIN, BATCH):
            for cell, _ in _cells(kind, fmt, ch, cmap, 0, 0):
                assert cell[6] == 0
                A.reset(), B.reset()
                assert push(3, 4) == 0
                if kind is BATCH:
                    b = A.upload_batch()
                    try:
                        assert b.frames == 1 and b.samples == 0
                        rc, _ = _both(L, native, b._h, b._h, cell, (None, C.c_void_p(dev.data_ptr())), (None, C.c_void_p(dev.data_ptr())))
                        assert rc == native.OK, cell
                        gpu_ctx.synchronize()
                    finally:
                        b.free()
                    B.drop_pending()
                    continue
                dest = (one.ctypes.data, None) if kind is SYNC else (pins[0].p, None)
                dest_b = (one.ctypes.data, None) if kind is SYNC else (pins[2].p, None)
                pins[0].bytes[:sb] = GUARD
                pins[2].bytes[:sb] = GUARD
                assert _both(L, native, A._h, B._h, cell, dest, dest_b) == (native.OK, 0), cell
                if kind is BEGIN:
                    for st in (A, B):
                        wr = C.c_int64(UNSET)
                        assert L.nvh_stream_synth_end(st._h, C.byref(wr)) == native.OK and wr.value == 0
                assert (one == GUARD).all() and (pins[0].bytes[:sb] == GUARD).all() and (pins[2].bytes[:sb] == GUARD).all()
        assert bool((dev == GUARD).all())
    finally:
        A.close(), B.close()
        for p in pins:
            p.free()

#!/usr/bin/env python
"""tests/golden/synth_arg_codes.json: the result codes of the 18 named synthesis calls on host-only streams (no GPU involved).

Run on the commit whose behaviour is to be pinned -- it only uses the named calls -- and commit the file; tests/test_pcm_out.py
replays it against the named calls and the descriptor calls of later commits.  One factor at a time around a valid call (float32,
a host destination, exactly enough room), per stream and call: formats, mixes, maps, destinations, device alignments, extents;
plus the pairs that show which check wins (a bad map against a bad format, a short extent against a bad destination).

    python tools/gen_synth_arg_codes.py [--check]      (--check: compare with the committed file instead of writing it)
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS_BAD = (2, -1, 7)
MIXES_BAD = (2, -1, 9)
# every factor: the un-mapped calls on the stereo file, the mapped calls on six channels; elsewhere the factors the shape changes


def maps_for(ch):
    """(map, count) variants for a stream of `ch` channels, the first three valid: identity, a permutation, a subset."""
    ident = list(range(ch))
    perm = ident[::-1] if ch > 1 else ident
    sub = [ch - 1] if ch > 1 else ident
    return [(ident, ch), (perm, ch), (sub, len(sub)),
            (None, ch), (ident, 0), (None, 0), (ident, -1), (ident + [0], ch + 1),          # null, count 0, -1, C + 1
            ([0, 0], 2), ([0, -1], 2), ([0, ch], 2)]                                         # duplicate, negative, >= C


def exact(name, ch, n, mix, oc):
    """Exactly enough room for the call: samples per channel for the planar forms, output samples otherwise."""
    from tests.test_pcm_out import form
    planar, has_mix, has_map = form(name)
    if planar:
        return n
    if has_map:
        return n * max(min(oc, ch), 1)
    if has_mix and mix == 1:
        return n
    return n * ch


def cells_for(key, ch, n):
    from tests import test_pcm_out as T
    out = []

    def add(name, fmt=0, mix=1, cmap=None, oc=0, dest="host", extent=None, short=0):
        planar, has_mix, has_map = T.form(name)
        mix = mix if has_mix else 0
        if not has_map:
            cmap, oc = None, 0
        if name in T.BEGIN and dest not in ("host", "neither"):
            return
        if name in T.BATCH:
            return  # (a batch needs a device: only the null-handle cells below)
        if name in ("nvh_stream_synth", "nvh_stream_synth_begin") and fmt != 0:
            return
        if extent is None:
            extent = exact(name, ch, n, mix, oc if has_map else 0) - short
        cell = [key, name, fmt, mix, cmap, oc, dest, extent]
        if cell not in out:
            out.append(cell)

    for name in T.SYNC + T.BEGIN:
        planar, has_mix, has_map = T.form(name)
        full = key == ("six" if has_map else "stereo")
        maps = maps_for(ch) if has_map else [(None, 0)]
        valid_maps = maps[:3] if has_map else maps
        base = dict(cmap=valid_maps[-2][0], oc=valid_maps[-2][1]) if has_map else {}  # (the permutation)
        # extents, for every valid map / mix of the call: exactly enough, one short, 0, -1
        for cmap, oc in (valid_maps if full else valid_maps[:2]):
            for mix in ((0, 1) if has_mix else (1,)):
                add(name, mix=mix, cmap=cmap, oc=oc)
                add(name, mix=mix, cmap=cmap, oc=oc, short=1)
                if full or key in ("stereo_empty", "stereo_first"):
                    add(name, mix=mix, cmap=cmap, oc=oc, extent=0)
                    add(name, mix=mix, cmap=cmap, oc=oc, extent=-1)
        # maps that are not maps of the stream
        for cmap, oc in (maps[3:] if full or key == "nine" else maps[3:6]):
            add(name, cmap=cmap, oc=oc)
        # destinations; with one sample too few as well (which check wins)
        for dest in (("dev+0", "both", "neither") if full else ("neither",)):
            add(name, dest=dest, **base)
            if full:
                add(name, dest=dest, short=1, **base)
                if has_mix:
                    add(name, mix=0, dest=dest)
        if not full:
            add(name, fmt=1, dest="dev+8", **base)
            add(name, fmt=1, dest="dev+8", cmap=valid_maps[0][0], oc=valid_maps[0][1])
            if key == "nine" and has_map:
                add(name, fmt=7, **base)  # a bad format behind a map this stream cannot take
            continue
        # formats and mixes
        add(name, fmt=1, **base)
        for fmt in FORMATS_BAD:
            add(name, fmt=fmt, **base)
        if has_map:
            add(name, fmt=7, cmap=[0, 0], oc=2)
            add(name, fmt=7, cmap=valid_maps[0][0], oc=valid_maps[0][1])
        if has_mix:
            for mix in MIXES_BAD:
                add(name, mix=mix)
                add(name, fmt=1, mix=mix)
            add(name, fmt=7, mix=9)
        # device addresses, both formats (and the identity map, which takes its un-mapped twin's rule)
        if name in T.SYNC:
            for off in (0, 1, 2, 8):
                for fmt in (0, 1):
                    add(name, fmt=fmt, dest="dev+%d" % off, **base)
                    if has_map:
                        add(name, fmt=fmt, dest="dev+%d" % off, cmap=valid_maps[0][0], oc=valid_maps[0][1])
                    if has_mix:
                        add(name, fmt=fmt, mix=0, dest="dev+%d" % off)
    return out


def null_cells():
    from tests import test_pcm_out as T
    out = []
    for name in T.NAMED:
        planar, has_mix, has_map = T.form(name)
        dest = "dev+0" if name in T.BATCH else "host"
        out.append(["null", name, 0, 1 if has_mix else 0, [0, 1] if has_map else None, 2 if has_map else 0, dest, 16])
        if has_map:  # a bad map and no handle
            out.append(["null", name, 0, 0, None, 2, dest, 16])
    return out


def main():
    import nvorbis_amd as nv
    from nvorbis_amd import native
    from tests import oracle_py, test_pcm_out as T
    oracle = oracle_py.load()
    ogg = {"3test": open(os.path.join(T.GOLDEN, "3test.ogg"), "rb").read()}
    L = native.lib()
    buf = np.zeros(1 << 18, np.float32)
    head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip()
    dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "nvorbis_amd/csrc", "include"]).decode().strip()
    assert not dirty, "the library sources differ from HEAD:\n" + dirty
    table = {"recorded_from": "commit %s (library %s): the named calls on host-only streams, tools/gen_synth_arg_codes.py" % (head, native.build_id()),
             "columns": ["stream", "call", "format", "mix", "map", "out_channels", "destination", "extent", "code",
                         "written (%d: left alone)" % T.UNSET],
             "streams": {}, "cells": []}
    for row in null_cells():
        table["cells"].append(row + list(T.call_named(L, None, row[1:], buf)))
    for key in T.STREAMS:
        st = T.open_host_stream(nv, oracle, ogg, key)
        ch, n = st.channels, st.pending()[1]
        table["streams"][key] = [ch, n]
        for row in cells_for(key, ch, n):
            table["cells"].append(row + list(T.call_named(L, st._h, row[1:], buf)))
        st.close()
    text = "{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(table[k])) for k in ("recorded_from", "columns", "streams")) + \
        ',\n "cells": [\n' + ",\n".join("  " + json.dumps(r) for r in table["cells"]) + "\n ]\n}\n"
    if "--check" in sys.argv:
        old = json.load(open(T.TABLE))
        diff = [(a, b) for a, b in zip(old["cells"], table["cells"]) if a != b]
        print("%d cells, %d differ from %s" % (len(table["cells"]), len(diff) + abs(len(old["cells"]) - len(table["cells"])), T.TABLE))
        for a, b in diff[:20]:
            print(" ", a, "->", b[8:])
        sys.exit(1 if diff or len(old["cells"]) != len(table["cells"]) else 0)
    open(T.TABLE, "w").write(text)
    codes = {}
    for r in table["cells"]:
        codes[r[8]] = codes.get(r[8], 0) + 1
    print("wrote %s: %d cells, codes %s" % (T.TABLE, len(table["cells"]), codes))


if __name__ == "__main__":
    main()

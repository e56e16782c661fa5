"""pcm_map_rates.py -- channel-map output (the _map twins) against interleaved PCM, this build against its parent commit, on one
box in one session:

  * C4 (six channels, n = 4096, full-depth packets, 2048 frames per resident batch, Batch.synth into HBM) on one stream and on
    three:
      (a) the parent's interleaved f32 pass,
      (b) this build's un-mapped interleaved f32 pass (the same machine code: profiles/pcm_twins_isa.txt),
      (c) WAVE order, interleaved, f32 and s16,
      (d) WAVE order, planar, f32,
      (e) interleaved f32 followed by a torch index_select to WAVE order (what a consumer runs without the twins),
      (f) the selecting map {0, 2}, interleaved f32;
  * C2 (bench.py's shape: stereo n = 2048 frames of 3test.ogg's long packets, 4096 frames per batch) on one stream:
      (g) the swap {1, 0}, which runs without paired emission (k_synth + the mapped k_ola_compact: the narrow emitting kernels
          have no mapped forms), against the parent's and this build's interleaved pass.

The parent commit's library (built from a checkout of the parent: python -m nvorbis_amd.build there) is given with --parent-lib;
it has no map entry points, so it runs the interleaved rows only.  The driver starts one child process per (library, round),
parent and this build alternated, each child under a time limit of its own; a child that fails ends the run.  One JSON object
per line, every line tagged with the build it came from.

    python tools/pcm_map_rates.py --parent-lib PATH [--passes 200] [--repeats 2]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTYPES = {"f32": (np.float32, "float32"), "s16": (np.int16, "int16")}
WAVE6 = (0, 2, 1, 5, 3, 4)
# (row, format, channel map, planar, index_select afterwards)
C4_ROWS = (("b interleaved", "f32", None, False, False), ("c wave", "f32", WAVE6, False, False), ("c wave", "s16", WAVE6, False, False),
           ("d wave planar", "f32", WAVE6, True, False), ("e interleaved+index_select", "f32", None, False, True),
           ("f select {0,2}", "f32", (0, 2), False, False))
C2_ROWS = (("b interleaved", "f32", None, False, False), ("g swap {1,0}", "f32", (1, 0), False, False))
PARENT_C4 = (("a interleaved", "f32", None, False, False),)
PARENT_C2 = (("a interleaved", "f32", None, False, False),)


def _passes(torch, tstreams, items, ch, row, passes, warm):
    """Microseconds per pass: every stream's batches launched in turn, `passes` times, between two synchronisations."""
    _, fmt, cmap, planar, select = row
    dt, tname = DTYPES[fmt]
    oc = len(cmap) if cmap else ch
    bufs = []
    for st, bl in items:
        per = []
        for b in bl:
            pcm = torch.empty(b.samples * oc, dtype=getattr(torch, tname), device="cuda")
            sel = torch.empty(b.samples, ch, dtype=getattr(torch, tname), device="cuda") if select else None
            per.append((pcm, sel))
        bufs.append(per)
    idx = torch.tensor(WAVE6, device="cuda") if select else None
    torch.cuda.synchronize()

    def run(n):
        for i in range(n):
            for ts, (st, bl), per in zip(tstreams, items, bufs):
                b, (pcm, sel) = bl[i % len(bl)], per[i % len(bl)]
                with torch.cuda.stream(ts):  # (the context launches on this stream: set_hip_stream)
                    if cmap is None:
                        b.synth(pcm.data_ptr(), pcm.numel(), dtype=dt)
                    else:
                        b.synth(pcm.data_ptr(), pcm.numel(), dtype=dt, plane_stride=b.samples if planar else None, channel_map=cmap)
                    if select:
                        torch.index_select(pcm.view(b.samples, ch), 1, idx, out=sel)
    run(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(passes)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / passes
    return sec, [k for k in items[0][1][0].kernels() if k != "-"]


def c4_items(nv, torch, bench, ctxs):
    from tests import vorbis_encode as ve
    hdr3 = ve.shipped_headers(open(os.path.join(ROOT, "tests", "golden", "3test.ogg"), "rb").read())
    h4 = ve.c4_headers(hdr3, psize=48)
    s4 = ve.setup_of(h4)
    pool4 = ve.packet_pool(s4, 148, per_kind=128, class_weights=[0] + [1] * 9)
    p, _ = ve.stream_from_pool(s4, h4, pool4, np.ones(2100, dtype=bool), np.random.default_rng(7))
    items = []
    for k, ctx in enumerate(ctxs):
        st, bl = bench.make_batches(nv, torch, ctx, p[:3], p[3:], 6, 2048, 2, seed_off=k)
        items.append((st, [b for b, _ in bl]))
    return items


def c2_items(nv, torch, bench, ctxs, headers, ll):
    items = []
    for k, ctx in enumerate(ctxs):
        st, bl = bench.make_batches(nv, torch, ctx, headers, ll, 2, 4096, 1, seed_off=k)
        items.append((st, [b for b, _ in bl]))
    return items


def worker(a):
    """One library, every row it can run (NVH_LIB chose it; --parent: the library of the parent commit, interleaved rows only)."""
    from nvorbis_amd import native
    if a.parent:  # the parent's library has no map entry points: bind what it has
        for name in [n for n in native.SIGNATURES if n.endswith("_map") or n == "nvh_channel_map_wave"]:
            del native.SIGNATURES[name]
    import torch

    import bench
    import nvorbis_amd as nv
    tag = "parent" if a.parent else "this"

    def out(row):
        row["build"] = tag
        print(json.dumps(row), flush=True)
    headers, ll, ch = bench.ll_packets(nv, os.path.join(ROOT, "tests", "golden", "3test.ogg"))
    assert ch == 2
    ctxs = [nv.Context(0) for _ in range(3)]
    tstreams = [torch.cuda.Stream() for _ in range(3)]
    for c, ts in zip(ctxs, tstreams):
        c.set_hip_stream(ts.cuda_stream)  # the library's launches and the index_selects in one order per stream
    out({"library": native.build_id()})
    for n in (1, 3):
        items = c4_items(nv, torch, bench, ctxs[:n])
        for _ in range(2):  # twice each, the rows alternated: the second round is the one to read
            for row in (PARENT_C4 if a.parent else C4_ROWS):
                sec, kern = _passes(torch, tstreams[:n], items, 6, row, a.passes // 2, 6)
                out({"what": "C4", "streams": n, "row": row[0], "format": row[1], "us_per_pass": sec * 1e6,
                     "frames_per_s": 2048 * n / sec, "kernels": kern})
        for st, bl in items:
            for b in bl:
                b.free()
            st.close()
    items = c2_items(nv, torch, bench, ctxs[:1], headers, ll)
    for _ in range(2):
        for row in (PARENT_C2 if a.parent else C2_ROWS):
            sec, kern = _passes(torch, tstreams[:1], items, 2, row, a.passes, 3)
            out({"what": "C2", "streams": 1, "row": row[0], "format": row[1], "us_per_pass": sec * 1e6, "frames_per_s": 4096 / sec,
                 "kernels": kern})
    for st, bl in items:
        for b in bl:
            b.free()
        st.close()
    for c in ctxs:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libnvorbis_hip.so built from the parent commit")
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=2, help="child processes per library, parent and this build alternated")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's library is needed for the comparison")
    base = [sys.executable, os.path.abspath(__file__), "--worker", "--passes", str(a.passes)]
    for _ in range(a.repeats):
        for parent in (True, False):
            env = dict(os.environ)
            env.pop("NVH_LIB", None)
            if parent:
                env["NVH_LIB"] = os.path.abspath(a.parent_lib)
                env["NVH_ALLOW_STALE"] = "1"  # (built from other sources: that is the point)
            # a fresh child per step, under its own time limit; a step that fails or runs over ends the run
            rc = subprocess.run(base + (["--parent"] if parent else []), env=env, cwd=ROOT, timeout=a.step_timeout).returncode
            if rc != 0:
                sys.exit("the %s build's step failed (exit %d): nothing further is started" % ("parent" if parent else "this", rc))


if __name__ == "__main__":
    main()

"""pcm_mix_rates.py -- the mono down-mix (the _mono twins) against interleaved PCM, this build against its parent commit, on one box
in one session:

  * the resident pass on bench.py's shape (stereo n = 2048 frames of 3test.ogg's long packets, 4096 frames per batch, Batch.synth
    into HBM) on one stream and on three: interleaved f32, mono f32, mono s16, and interleaved f32 followed by a torch mean over
    the channels (what a consumer of mono input runs without the twins);
  * C4 (six channels, n = 4096, full-depth packets, 2048 frames per batch) on one stream, the same rows;
  * end to end with the GPU parser and the pipelined pinned read-back at 32 768 packets per batch: interleaved f32 and s16,
    mono f32 and mono s16.

The parent commit's library (built from a checkout of the parent: python -m nvorbis_amd.build there) is given with --parent-lib;
it has no mixing entry points, so it runs the interleaved rows only.  The driver starts one child process per (library, round),
parent and this build alternated, each child under a time limit of its own; a child that fails ends the run.  One JSON object
per line, every line tagged with the build it came from.

    python tools/pcm_mix_rates.py --parent-lib PATH [--passes 200] [--rounds 16] [--repeats 2]
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

FRAMES = 4096
DTYPES = {"f32": (np.float32, "float32"), "s16": (np.int16, "int16")}
# (format, what is launched): "mean" = interleaved + torch mean over the channels
ROWS = (("f32", "interleaved"), ("f32", "mono"), ("s16", "mono"), ("f32", "interleaved+mean"))
PARENT_ROWS = (("f32", "interleaved"),)


def _launch(torch, b, pcm, mono, dt, form, ch):
    if form == "mono":
        b.synth(mono.data_ptr(), b.samples, dtype=dt, mix="mono")
        return
    b.synth(pcm.data_ptr(), pcm.numel(), dtype=dt)
    if form == "interleaved+mean":  # on the stream the context launches on (set_hip_stream below)
        torch.mean(pcm.view(b.samples, ch), dim=1, out=mono)


def resident(nv, torch, ctxs, tstreams, headers, ll, passes, fmt, form):
    """Microseconds per 4096-frame pass with len(ctxs) streams (one batch each, launches interleaved), by wall clock over `passes`
    queued launches per stream between two synchronisations."""
    dt, tname = DTYPES[fmt]
    items = []
    for k, ctx in enumerate(ctxs):
        st = nv.Stream(ctx, *headers)
        st.push_packet(ll[k % len(ll)], -1, 0)
        st.synth_host()
        for i in range(FRAMES):
            st.push_packet(ll[(k + 1 + i) % len(ll)], -1, 0)
        b = st.upload_batch()
        pcm = torch.empty(b.samples * st.channels, dtype=getattr(torch, tname), device="cuda")
        mono = torch.empty(b.samples, dtype=getattr(torch, tname), device="cuda")
        items.append((st, b, pcm, mono))
    torch.cuda.synchronize()

    def run(n):
        for _ in range(n):
            for ts, (st, b, pcm, mono) in zip(tstreams, items):
                with torch.cuda.stream(ts):
                    _launch(torch, b, pcm, mono, dt, form, st.channels)
    run(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(passes)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / passes
    kern = [k for k in items[0][1].kernels() if k != "-"]
    for st, b, pcm, mono in items:
        b.free()
        st.close()
    return {"what": "resident", "streams": len(ctxs), "format": fmt, "form": form, "us_per_pass": sec * 1e6,
            "frames_per_s": FRAMES * len(ctxs) / sec, "kernels": kern}


def c4(nv, torch, bench, ctx, tstream, passes, fmt, form):
    """C4 on one stream: two resident batches of 2048 six-channel n = 4096 full-depth frames, alternated."""
    from tests import vorbis_encode as ve
    dt, tname = DTYPES[fmt]
    hdr3 = ve.shipped_headers(open(os.path.join(ROOT, "tests", "golden", "3test.ogg"), "rb").read())
    h4 = ve.c4_headers(hdr3, psize=48)
    s4 = ve.setup_of(h4)
    pool4 = ve.packet_pool(s4, 148, per_kind=128, class_weights=[0] + [1] * 9)
    p, _ = ve.stream_from_pool(s4, h4, pool4, np.ones(2100, dtype=bool), np.random.default_rng(7))
    st, bl = bench.make_batches(nv, torch, ctx, p[:3], p[3:], 6, 2048, 2)
    bufs = [(torch.empty(b.samples * 6, dtype=getattr(torch, tname), device="cuda"),
             torch.empty(b.samples, dtype=getattr(torch, tname), device="cuda")) for b, _ in bl]

    def run(n):
        with torch.cuda.stream(tstream):
            for i in range(n):
                _launch(torch, bl[i % 2][0], bufs[i % 2][0], bufs[i % 2][1], dt, form, 6)
    run(6)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(passes)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / passes
    kern = [k for k in bl[0][0].kernels() if k != "-"]
    for b, _ in bl:
        b.free()
    st.close()
    return {"what": "C4", "streams": 1, "format": fmt, "form": form, "us_per_pass": sec * 1e6, "frames_per_s": 2048 / sec,
            "kernels": kern}


def end_to_end(nv, ctx, headers, ll, fmt, mono, frames=32768, rounds=16):
    """bench.end_to_end's GPU-parser leg: packets in host memory -> GPU parse -> kernels -> pipelined read-back into page-locked
    host memory, two batches outstanding, one host thread; what is read back as the one difference."""
    dt, _ = DTYPES[fmt]
    kw = {"mix": "mono"} if mono else {}
    pk = [ll[(i + 1) % len(ll)] for i in range(frames)]
    offs = np.zeros(frames + 1, np.int64)
    offs[1:] = np.cumsum([len(p) for p in pk])
    pa = nv.PacketArray(np.frombuffer(b"".join(pk), np.uint8), offs, np.full(frames, -1, np.int64), np.zeros(frames, np.uint8))
    st = nv.Stream(ctx, *headers)
    st.set_gpu_parse(True)
    st.push_packet(ll[0], -1, 0)
    st.synth_host(dtype=dt)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        outstanding = 0
        for _r in range(rounds):
            assert st.push_packets(pa, 0, frames) == frames
            st.synth_begin(dtype=dt, **kw)
            outstanding += 1
            if outstanding == 2:
                st.synth_end()
                outstanding -= 1
        while outstanding:
            st.synth_end()
            outstanding -= 1
        sec = (time.perf_counter() - t0) / rounds
        best = sec if best is None or sec < best else best
    st.close()
    return {"what": "end_to_end", "format": fmt, "form": "mono" if mono else "interleaved", "packets_per_batch": frames,
            "frames_per_s": frames / best, "ms_per_batch": best * 1e3}


def worker(a):
    """One library, every row it can run (NVH_LIB chose it; --parent: the library of the parent commit, interleaved rows only)."""
    from nvorbis_amd import native
    if a.parent:  # the parent's library has no mixing entry points: bind what it has
        for name in [n for n in native.SIGNATURES if n.endswith("_mix")]:
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
        c.set_hip_stream(ts.cuda_stream)  # the library's launches and the means in one order per stream
    out({"library": native.build_id(), "shape": "stereo n = 2048 (3test.ogg long packets), %d frames per resident batch" % FRAMES})
    rows = PARENT_ROWS if a.parent else ROWS
    for n in (1, 3):
        for _ in range(2):  # twice each, the forms alternated: the second round is the one to read
            for fmt, form in rows:
                out(resident(nv, torch, ctxs[:n], tstreams[:n], headers, ll, a.passes, fmt, form))
    for _ in range(2):
        for fmt, form in rows:
            out(c4(nv, torch, bench, ctxs[0], tstreams[0], a.passes // 2, fmt, form))
    for _ in range(2):
        for fmt in ("f32", "s16"):
            out(end_to_end(nv, ctxs[0], headers, ll, fmt, not a.parent, rounds=a.rounds))
    for c in ctxs:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libnvorbis_hip.so built from the parent commit")
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=2, help="child processes per library, parent and this build alternated")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's library is needed for the comparison")
    base = [sys.executable, os.path.abspath(__file__), "--worker", "--passes", str(a.passes), "--rounds", str(a.rounds)]
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

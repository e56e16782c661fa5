"""pcm_layout_rates.py -- interleaved and channel-planar PCM side by side, in one process, the layouts alternated:

  * the resident pass on bench.py's shape (stereo n = 2048 frames of 3test.ogg's long packets, 4096 frames per batch, Batch.synth
    into HBM) on one stream and on three, for interleaved, planar (the _planar twins), and interleaved followed by a torch
    transpose into [C, T] (what a consumer of [channels, frames] runs without the planar twins), in float32 and int16;
  * C4 (six channels, n = 4096, full-depth packets, 2048 frames per batch) on one stream, interleaved against planar;
  * end to end with the GPU parser and the pipelined pinned read-back at 32 768 packets per batch, interleaved against planar.

One JSON object per line.

    python tools/pcm_layout_rates.py [--passes 200] [--rounds 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import nvorbis_amd as nv  # noqa: E402

FRAMES = 4096
DTYPES = {"f32": (np.float32, "float32"), "s16": (np.int16, "int16")}
LAYOUTS = ("interleaved", "planar", "interleaved+transpose")


def _launch(torch, b, pcm, planes, dt, layout, ch):
    if layout == "planar":
        b.synth(pcm.data_ptr(), 0, dtype=dt, plane_stride=b.samples)
        return
    b.synth(pcm.data_ptr(), pcm.numel(), dtype=dt)
    if layout == "interleaved+transpose":  # on the stream the context launches on (set_hip_stream below)
        planes.copy_(pcm.view(b.samples, ch).t())


def resident(torch, ctxs, tstreams, headers, ll, passes, fmt, layout):
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
        planes = torch.empty((st.channels, b.samples), dtype=getattr(torch, tname), device="cuda")
        items.append((st, b, pcm, planes))
    torch.cuda.synchronize()

    def run(n):
        for _ in range(n):
            for ts, (st, b, pcm, planes) in zip(tstreams, items):
                with torch.cuda.stream(ts):
                    _launch(torch, b, pcm, planes, dt, layout, st.channels)
    run(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(passes)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / passes
    kern = [k for k in items[0][1].kernels() if k != "-"]
    for st, b, pcm, planes in items:
        b.free()
        st.close()
    return {"what": "resident", "streams": len(ctxs), "format": fmt, "layout": layout, "us_per_pass": sec * 1e6,
            "frames_per_s": FRAMES * len(ctxs) / sec, "kernels": kern}


def c4(torch, ctx, tstream, passes, layout):
    """C4 on one stream: two resident batches of 2048 six-channel n = 4096 full-depth frames, alternated."""
    from tests import vorbis_encode as ve
    hdr3 = ve.shipped_headers(open(os.path.join(bench.ROOT, "tests", "golden", "3test.ogg"), "rb").read())
    h4 = ve.c4_headers(hdr3, psize=48)
    s4 = ve.setup_of(h4)
    pool4 = ve.packet_pool(s4, 148, per_kind=128, class_weights=[0] + [1] * 9)
    p, _ = ve.stream_from_pool(s4, h4, pool4, np.ones(2100, dtype=bool), np.random.default_rng(7))
    st, bl = bench.make_batches(nv, torch, ctx, p[:3], p[3:], 6, 2048, 2)
    planes = [torch.empty((6, b.samples), dtype=torch.float32, device="cuda") for b, _ in bl]

    def run(n):
        with torch.cuda.stream(tstream):
            for i in range(n):
                b, pcm = bl[i % 2]
                _launch(torch, b, pcm, planes[i % 2], np.float32, layout, 6)
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
    return {"what": "C4", "streams": 1, "format": "f32", "layout": layout, "us_per_pass": sec * 1e6, "frames_per_s": 2048 / sec,
            "kernels": kern}


def end_to_end(ctx, headers, ll, fmt, planar, frames=32768, rounds=16):
    """bench.end_to_end's GPU-parser leg: packets in host memory -> GPU parse -> kernels -> pipelined read-back into page-locked
    host memory, two batches outstanding, one host thread; the layout of the read-back as the one difference."""
    dt, _ = DTYPES[fmt]
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
            st.synth_begin(dtype=dt, planar=planar)
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
    return {"what": "end_to_end", "format": fmt, "layout": "planar" if planar else "interleaved", "packets_per_batch": frames,
            "frames_per_s": frames / best, "ms_per_batch": best * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=16)
    a = ap.parse_args()
    import torch
    headers, ll, ch = bench.ll_packets(nv, os.path.join(bench.ROOT, "tests", "golden", "3test.ogg"))
    assert ch == 2
    ctxs = [nv.Context(0) for _ in range(3)]
    tstreams = [torch.cuda.Stream() for _ in range(3)]
    for c, ts in zip(ctxs, tstreams):
        c.set_hip_stream(ts.cuda_stream)  # the library's launches and the transposes in one order per stream
    print(json.dumps({"library": nv.native.build_id(), "shape": "stereo n = 2048 (3test.ogg long packets), %d frames per resident batch" % FRAMES}))
    for n in (1, 3):
        for fmt in ("f32", "s16"):
            for _ in range(2):  # twice each, the layouts alternated: the second round is the one to read
                for layout in LAYOUTS:
                    print(json.dumps(resident(torch, ctxs[:n], tstreams[:n], headers, ll, a.passes, fmt, layout)), flush=True)
    for _ in range(2):
        for layout in ("interleaved", "planar"):
            print(json.dumps(c4(torch, ctxs[0], tstreams[0], a.passes // 2, layout)), flush=True)
    for _ in range(2):
        for planar in (False, True):
            print(json.dumps(end_to_end(ctxs[0], headers, ll, "f32", planar, rounds=a.rounds)), flush=True)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()

"""pcm_format_rates.py -- float32 and 16-bit PCM side by side, in one process, on bench.py's shape (stereo n = 2048 frames of
3test.ogg's long packets, bench.ll_packets): the resident pass (4096 frames per batch, Batch.synth into HBM) on one stream and on
three, and the end-to-end rate with the GPU parser and the pipelined read-back at 32 768 packets per batch (bench.end_to_end's
shape, with the output format as the one difference).  One JSON object per line.

    python tools/pcm_format_rates.py [--passes 200] [--rounds 16]
    python tools/pcm_format_rates.py --only-resident s16|f32 --passes 50   (one format's resident pass alone: a --pmc run)
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


def resident(torch, ctxs, headers, ll, passes, fmt):
    """Seconds per 4096-frame pass with len(ctxs) streams (one batch each, launches interleaved), by wall clock over `passes`
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
        items.append((st, b, pcm))
    torch.cuda.synchronize()
    for _ in range(3):
        for ctx, (st, b, pcm) in zip(ctxs, items):
            b.synth(pcm.data_ptr(), pcm.numel(), dtype=dt)
    for ctx in ctxs:
        ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        for ctx, (st, b, pcm) in zip(ctxs, items):
            b.synth(pcm.data_ptr(), pcm.numel(), dtype=dt)
    for ctx in ctxs:
        ctx.synchronize()
    sec = (time.perf_counter() - t0) / passes
    kern = [k for k in items[0][1].kernels() if k != "-"]
    out_bytes = items[0][2].numel() * items[0][2].element_size()
    for st, b, pcm in items:
        b.free()
        st.close()
    return {"streams": len(ctxs), "format": fmt, "us_per_pass": sec * 1e6, "frames_per_s": FRAMES * len(ctxs) / sec,
            "pcm_bytes_per_pass_per_stream": out_bytes, "kernels": kern}


def end_to_end(ctx, headers, ll, fmt, frames=32768, rounds=16):
    """bench.end_to_end's GPU-parser leg, in `fmt`: packets in host memory -> GPU parse -> kernels -> pipelined read-back into
    page-locked host memory, two batches outstanding, one host thread."""
    dt, _ = DTYPES[fmt]
    pk = [ll[(i + 1) % len(ll)] for i in range(frames)]
    offs = np.zeros(frames + 1, np.int64)
    offs[1:] = np.cumsum([len(p) for p in pk])
    pa = nv.PacketArray(np.frombuffer(b"".join(pk), np.uint8), offs, np.full(frames, -1, np.int64), np.zeros(frames, np.uint8))
    st = nv.Stream(ctx, *headers)
    st.set_gpu_parse(True)
    st.push_packet(ll[0], -1, 0)
    st.synth_host(dtype=dt)
    best, push_s = None, None
    for _ in range(3):
        t0 = time.perf_counter()
        outstanding, tp = 0, 0.0
        for _r in range(rounds):
            a = time.perf_counter()
            assert st.push_packets(pa, 0, frames) == frames
            tp += time.perf_counter() - a
            st.synth_begin(dtype=dt)
            outstanding += 1
            if outstanding == 2:
                st.synth_end()
                outstanding -= 1
        while outstanding:
            st.synth_end()
            outstanding -= 1
        sec = (time.perf_counter() - t0) / rounds
        if best is None or sec < best:
            best, push_s = sec, tp / rounds
    # the host push alone, and one batch's blocking synthesis (upload + GPU parse + kernels + read-back) alone
    st.push_packets(pa, 0, frames)
    t0 = time.perf_counter()
    st.synth_host(pinned=True, dtype=dt)
    blocking = time.perf_counter() - t0
    st.close()
    return {"format": fmt, "packets_per_batch": frames, "frames_per_s": frames / best, "ms_per_batch": best * 1e3,
            "host_push_ms_per_batch": push_s * 1e3, "blocking_synth_ms_per_batch": blocking * 1e3,
            "pcm_GBps_over_pcie": frames * 1024 * 2 * np.dtype(dt).itemsize / best / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--only-resident", choices=sorted(DTYPES))
    a = ap.parse_args()
    import torch
    headers, ll, ch = bench.ll_packets(nv, os.path.join(bench.ROOT, "tests", "golden", "3test.ogg"))
    assert ch == 2
    ctxs = [nv.Context(0) for _ in range(3)]
    print(json.dumps({"library": nv.native.build_id(), "shape": "stereo n = 2048 (3test.ogg long packets), %d frames per resident batch" % FRAMES}))
    if a.only_resident:
        print(json.dumps(resident(torch, ctxs[:1], headers, ll, a.passes, a.only_resident)))
        return
    for n in (1, 3):
        for fmt in ("f32", "s16", "f32", "s16"):  # twice each, alternating: the second pair is the one to read
            print(json.dumps(resident(torch, ctxs[:n], headers, ll, a.passes, fmt)), flush=True)
    for fmt in ("f32", "s16", "f32", "s16"):
        print(json.dumps(end_to_end(ctxs[0], headers, ll, fmt, rounds=a.rounds)), flush=True)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What rows at one sample rate cost: nv.decode_clip_rows(..., sample_rate=16000) against the same call without the keyword.

    python tools/time_resample_rows.py [--rows 1024] [--runs 3] [--out profiles/resample_rows_rates.txt]

Workload: `--rows` rows of one second each from 2test.ogg, 3test.ogg and issue6test.ogg (all 44100 Hz; seeded random starts, whole
rows inside the clips), to the device.  Resampled: length 16000 at sample_rate=16000 -- every row decodes 44100 + 2 * 45 source
samples and k_resample_rows writes 16000.  Plain: length 44100 without the keyword -- one-second rows at the source rate.  Two
cases: the mono mix of the three files, and the stereo files as interleaved stereo f32.  The two calls alternate in one process,
`--runs` runs each; reported are rows/s as min - max, and k_resample_rows' own time by events around nvh_resample_rows (the context
runs on a torch stream, so that torch's events bracket it: the per-row block's copy and the kernel) with its share of the call.  No rate is promised anywhere: these are the
numbers as measured."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def workload(names, rows, rate_out):
    import numpy as np
    import nvorbis_amd as nv
    data = {n: open(os.path.join(GOLDEN, n), "rb").read() for n in names}
    totals = {}
    for n in names:
        pa = nv.demux_ogg_array(data[n], 0)
        st = nv.Stream(None, pa[0], pa[1], pa[2])
        totals[n] = st.index_total(pa)
        st.close()
    rng = np.random.default_rng(11)
    files, src_starts = [], []
    for k in range(rows):
        n = names[k % len(names)]
        files.append(data[n])
        src_starts.append(int(rng.integers(0, (totals[n] - 44100 - 64) // 4)) * 4)
    # the same second of every clip in both calls: the resampled call's starts count target-rate samples
    return files, src_starts, [s * rate_out // 44100 for s in src_starts]


def measure(rows, runs):
    import torch
    import nvorbis_amd as nv
    # a stream of torch's that the context runs on too (torch's default stream is the null handle, which a context answers with a
    # stream of its own): events recorded on it bracket what nvh_resample_rows queues
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    ctx = nv.Context(0, hip_stream=side.cuda_stream)
    spans = []
    inner = nv.Context.resample_rows

    def timed(self, *a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        inner(self, *a, **kw)
        e1.record(side)
        spans.append((e0, e1))
    nv.Context.resample_rows = timed
    out = []
    try:
        for label, names, kw in (("three files, mono mix", ("2test.ogg", "3test.ogg", "issue6test.ogg"), {"mix": "mono"}),
                                 ("stereo files, stereo f32", ("3test.ogg", "issue6test.ogg"), {})):
            files, src_starts, out_starts = workload(names, rows, 16000)

            def resampled(n=rows):
                r, _ = nv.decode_clip_rows(files[:n], 16000, out_starts[:n], ctx=ctx, device_out=True, sample_rate=16000, **kw)
                torch.cuda.synchronize()
                return r

            def plain(n=rows):
                r, _ = nv.decode_clip_rows(files[:n], 44100, src_starts[:n], ctx=ctx, device_out=True, **kw)
                torch.cuda.synchronize()
                return r
            resampled(32)  # warm-up: library, setup cache, tap table, allocations
            plain(32)
            tr, tp, kernel_ms = [], [], []
            for _ in range(runs):  # alternating
                del spans[:]
                t0 = time.perf_counter()
                resampled()
                tr.append(time.perf_counter() - t0)
                kernel_ms.append(sum(a.elapsed_time(b) for a, b in spans))
                t0 = time.perf_counter()
                plain()
                tp.append(time.perf_counter() - t0)
            r = {"case": label, "rows": rows, "resampled_rows_per_s": [rows / t for t in tr], "plain_rows_per_s": [rows / t for t in tp],
                 "kernel_ms": kernel_ms, "kernel_share": [k * 1e-3 / t for k, t in zip(kernel_ms, tr)]}
            print("RESAMPLE_ROWS " + json.dumps(r), flush=True)
            out.append(r)
    finally:
        nv.Context.resample_rows = inner
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_rows_rates.txt"))
    a = ap.parse_args()
    res = measure(a.rows, a.runs)
    lines = ["# tools/time_resample_rows.py: %d rows of one second each to the device, %d runs each, the two calls alternating in one process."
             % (a.rows, a.runs),
             "# resampled: decode_clip_rows(length=16000, sample_rate=16000) on 44100 Hz clips; plain: length=44100 without the keyword.",
             "# rows/s as min - max; kernel: k_resample_rows by events around nvh_resample_rows, ms per call and its share of the call.",
             "%-28s %-23s %-23s %-19s %s" % ("case", "resampled rows/s", "plain rows/s", "kernel ms", "kernel share")]
    for r in res:
        lines.append("%-28s %9.0f - %-11.0f %9.0f - %-11.0f %7.3f - %-9.3f %.4f - %.4f" % (
            r["case"], min(r["resampled_rows_per_s"]), max(r["resampled_rows_per_s"]), min(r["plain_rows_per_s"]),
            max(r["plain_rows_per_s"]), min(r["kernel_ms"]), max(r["kernel_ms"]), min(r["kernel_share"]), max(r["kernel_share"])))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()

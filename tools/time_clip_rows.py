#!/usr/bin/env python3
"""What fixed-length rows cost: nv.decode_clip_rows against decode_clips + slice + pad with torch.

    python tools/time_clip_rows.py [--windows 2048] [--length 44100] [--runs 3] [--out profiles/clip_rows_rates.txt]

Workload: `--windows` windows of `--length` samples from the golden files, the starts seeded random multiples of 4 and the same
starts plus 1.  Four cases: every file with the mono mix to the device (four setups), the stereo files as stereo f32 to the host
(two setups: 3test.ogg and issue6test.ogg), and both forms for 3test.ogg alone -- one setup: the kernels write the returned buffer.  The baseline is the
route without windows, in the same process, alternating with the windowed one: decode_clips on the whole files, then every
window sliced and zero-padded into the same [N, T(, C)] tensor with torch.  Reported: rows/s as min - max over the runs, what
Stream.kernels() named per batch, and an estimate of the share of decoded frames inside the geometric conditions of paired
emission (as tools/clip_rates.py estimates it).

--chunks: k_zero_rows' chunk size.  The same mono-to-device workload and the pad test's shape (rows of 262144 samples from
1test.ogg, 17318 samples long: every row is mostly pad) in child processes under NVH_ZERO_CHUNK_KIB = 4, 16 and 64."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ("1test.ogg", "2test.ogg", "3test.ogg", "issue6test.ogg")


def workload(names, windows, shift):
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
    files, starts = [], []
    for k in range(windows):
        n = names[k % len(names)]
        files.append(data[n])
        starts.append(int(rng.integers(0, totals[n] // 4)) * 4 + shift)
    return files, starts


def baseline(nv, torch, files, starts, length, ctx, mono, device_out):
    """decode_clips on the whole files, then slice and pad with torch into the tensor decode_clip_rows returns."""
    pcm = nv.decode_clips(files, ctx=ctx, mix="mono" if mono else None, device_out=device_out)
    ch = 1 if mono else 2
    if device_out:
        out = torch.zeros((len(files), length) if mono else (len(files), length, ch), dtype=torch.float32, device=pcm[0].device)
        for i, (p, s) in enumerate(zip(pcm, starts)):
            x = p[s * ch:(s + length) * ch]
            out[i].view(-1)[:x.numel()] = x
        torch.cuda.synchronize()
        return out
    out = torch.zeros((len(files), length) if mono else (len(files), length, ch), dtype=torch.float32)
    for i, (p, s) in enumerate(zip(pcm, starts)):
        x = torch.from_numpy(p[s * ch:(s + length) * ch])
        out[i].view(-1)[:x.numel()] = x
    return out


def windowed(nv, torch, files, starts, length, ctx, mono, device_out):
    rows, _ = nv.decode_clip_rows(files, length, starts, ctx=ctx, mix="mono" if mono else None, device_out=device_out)
    if device_out:
        torch.cuda.synchronize()
    return rows


def watch(nv):
    """Record what every batch of decode_clip_rows names and its frames' emission geometry."""
    import numpy as np
    from nvorbis_amd import clips
    seen = {"kernels": {}, "decoded": 0, "eligible": 0}
    flush = clips._RowGroup.flush

    def spy(self):
        st = self.stream
        if st.pending()[0]:
            geo = st.pending_geometry()
            for g in range(geo.shape[0]):
                n, start, valid, _, es, ec, ov, _ = (int(v) for v in geo[g])
                seen["decoded"] += n != 0
                if g and n >= 256 and geo[g - 1, 0] >= 256 and ov == g - 1 and es == start and ec == valid - start and valid % 64 == 0:
                    seen["eligible"] += 1
        had = st.pending()[1]
        flush(self)
        if had:
            k = ",".join(st.kernels())
            seen["kernels"][k] = seen["kernels"].get(k, 0) + 1
    clips._RowGroup.flush = spy
    return seen, lambda: setattr(clips._RowGroup, "flush", flush)


def measure(windows, length, runs, cases=None):
    import torch
    import nvorbis_amd as nv
    ctx = nv.Context(0)
    out = []
    all_cases = [("four files, mono mix, device", FILES, True, True), ("stereo files, stereo f32, host", FILES[2:], False, False),
                 ("3test.ogg alone, mono mix, device", FILES[2:3], True, True), ("3test.ogg alone, stereo f32, host", FILES[2:3], False, False)]
    for label, names, mono, dev in all_cases[:cases]:
        for shift in (0, 1):
            files, starts = workload(names, windows, shift)
            windowed(nv, torch, files[:32], starts[:32], length, ctx, mono, dev)  # warm-up: library, setup cache, allocations
            baseline(nv, torch, files[:32], starts[:32], length, ctx, mono, dev)
            seen, undo = watch(nv)
            windowed(nv, torch, files, starts, length, ctx, mono, dev)
            undo()
            tw, tb = [], []
            for _ in range(runs):  # alternating
                t0 = time.perf_counter()
                windowed(nv, torch, files, starts, length, ctx, mono, dev)
                tw.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                baseline(nv, torch, files, starts, length, ctx, mono, dev)
                tb.append(time.perf_counter() - t0)
            r = {"case": label, "starts": "multiples of 4" if shift == 0 else "multiples of 4, plus 1", "windows": windows,
                 "rows_per_s": [windows / t for t in tw], "baseline_rows_per_s": [windows / t for t in tb],
                 "kernels": seen["kernels"], "paired_share": seen["eligible"] / max(seen["decoded"], 1), "frames": seen["decoded"]}
            print("CLIP_ROWS " + json.dumps(r), flush=True)
            out.append(r)
    ctx.close()
    return out


def chunk_child(windows, length, runs):
    """One chunk size (the environment's): the mono-to-device workload and the pad shape, seconds per call as min - max."""
    import torch
    import nvorbis_amd as nv
    ctx = nv.Context(0)
    files, starts = workload(FILES, windows, 0)
    pad_files = [open(os.path.join(GOLDEN, "1test.ogg"), "rb").read()] * 64
    res = {}
    for label, call in (("workload", lambda: windowed(nv, torch, files, starts, length, ctx, True, True)),
                        ("pad shape", lambda: windowed(nv, torch, pad_files, [0] * 64, 262144, ctx, False, True))):
        call()
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        res[label] = ts
    ctx.close()
    print("CLIP_ROWS_CHUNK " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=2048)
    ap.add_argument("--length", type=int, default=44100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", type=int, default=None)
    ap.add_argument("--chunks", action="store_true")
    ap.add_argument("--chunk-child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_rows_rates.txt"))
    a = ap.parse_args()
    if a.chunk_child:
        return chunk_child(a.windows, a.length, a.runs)
    lines = ["# tools/time_clip_rows.py: %d windows of %d samples, %d runs each, decode_clip_rows and the baseline alternating in one process;"
             % (a.windows, a.length, a.runs),
             "# baseline: decode_clips on the whole files, then slice + zero-pad into the same tensor with torch.  rows/s, min - max."]
    rows = measure(a.windows, a.length, a.runs, a.cases)
    lines.append("%-36s %-24s %-23s %-23s" % ("case", "starts", "decode_clip_rows", "decode_clips + torch"))
    for r in rows:
        lines.append("%-36s %-24s %9.0f - %-11.0f %9.0f - %-11.0f" % (r["case"], r["starts"], min(r["rows_per_s"]), max(r["rows_per_s"]),
                                                                    min(r["baseline_rows_per_s"]), max(r["baseline_rows_per_s"])))
    for r in rows:
        lines.append("# %s, %s: Stream.kernels() per batch %s; estimated share of the %d decoded frames inside the geometric conditions of "
                     "paired emission %.3f" % (r["case"], r["starts"], json.dumps(r["kernels"]), r["frames"], r["paired_share"]))
    if a.chunks:
        lines.append("# k_zero_rows' chunk (NVH_ZERO_CHUNK_KIB; KiB of a 4-byte plane), seconds per call, min - max of %d: the four-file mono "
                     "workload above, and 64 rows of 262144 samples from 1test.ogg (mono, 17318 samples: the rest of every row is pad)" % a.runs)
        for kib in (4, 16, 64):
            env = dict(os.environ, NVH_ZERO_CHUNK_KIB=str(kib))
            cmd = [sys.executable, os.path.abspath(__file__), "--chunk-child", "--windows", str(a.windows), "--length", str(a.length),
                   "--runs", str(a.runs)]
            p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            got = [l for l in p.stdout.splitlines() if l.startswith("CLIP_ROWS_CHUNK ")]
            if p.returncode != 0 or not got:
                raise SystemExit("chunk child %d KiB failed (exit %d):\n%s" % (kib, p.returncode, p.stdout[-2000:]))
            res = json.loads(got[-1][len("CLIP_ROWS_CHUNK "):])
            lines.append("chunk %2d KiB: workload %.4f - %.4f s, pad shape %.4f - %.4f s" %
                         (kib, min(res["workload"]), max(res["workload"]), min(res["pad shape"]), max(res["pad shape"])))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()

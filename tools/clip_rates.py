#!/usr/bin/env python3
"""What a short-clip workload costs: one VorbisReader per clip (the parent commit's way) against nv.decode_clips.

    python tools/clip_rates.py --parent-tree DIR [--clips 2048] [--runs 3] [--out profiles/clip_batch_rates.txt]

Workload: `--clips` clips of 40 packets and as many of 8 packets, cut from tests/golden/3test.ogg and rewritten as Ogg files of
their own (tests/ogg_py.write_ogg; the last packet carries the end-of-stream flag and the clip's exact length, as an encoder
writes it).  One context, the GPU packet parser, f32 interleaved, PCM into page-locked host memory and from there into one array
per clip.  DIR is a checkout of the parent commit with its library built: the baseline runs there -- one VorbisReader per clip,
sequentially and on 16 threads with a context each -- in a process of its own; decode_clips runs in this tree.  Parent and
branch alternate, `--runs` runs each; the table reports clips/s and frames/s as min - max.

    python tools/clip_rates.py --flags --parent-tree DIR [--clips 2048] [--runs 3] [--out profiles/segment_clipped_rates.txt]

--flags: what per-segment HasClipped costs.  The same workload through nv.decode_clips in the parent tree (clips_plain), in this
tree without the keyword (clips_plain) and with return_clipped=True (clips_flags), and the headline of `python bench.py` in both
trees; parent and branch alternate.

Every measurement is a child process (this script with --child): a fresh HIP runtime each time, nothing shared between runs."""
import argparse
import json
import os
import pickle
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_workload(nclips, path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import nvorbis_amd as nv
    from tests import ogg_py
    pk, _, _ = nv.demux_ogg(open(os.path.join(ROOT, "tests", "golden", "3test.ogg"), "rb").read())
    probe = nv.Stream(None, pk[0], pk[1], pk[2])
    rng = np.random.default_rng(7)
    sets = {}
    for length in (40, 8):
        files = []
        for _ in range(nclips):
            first = int(rng.integers(3, len(pk) - length))
            run = list(pk[first:first + length])
            _, em, _, _ = probe.index_packets(nv.PacketArray.from_list(pk[:3] + run))
            files.append(ogg_py.write_ogg(pk[:3] + run, [0, 0, 0] + [int(v) for v in em], serial=0x2000 + len(files)))
        sets[length] = files
    probe.close()
    with open(path, "wb") as fh:
        pickle.dump(sets, fh)


def paired_share(nv, files, batch_frames, align):
    """The segments decode_clips makes of `files`, batch by batch on one stream: what Stream.kernels() names for each batch (the
    fact), and an ESTIMATE of the share of decoded frames inside the geometric conditions of paired emission, recomputed here from
    the pending geometry (the library's own count is assign_emission's in nvh_launch.hip and is not exported; 3test.ogg's
    channels always execute) -- a batch below 7/8 runs without paired emission altogether, which the kernel names show."""
    import numpy as np
    ctx = nv.Context(0)
    pa0 = nv.demux_ogg_array(files[0], 0)
    st = nv.Stream(ctx, pa0[0], pa0[1], pa0[2])
    st.set_gpu_parse(True)
    named, eligible, decoded = {}, 0, 0

    def flush():
        nonlocal eligible, decoded
        if not st.pending()[0]:
            return
        geo, table = st.pending_geometry(), st.pending_segments()
        pos = np.zeros(geo.shape[0], np.int64)  # out_pos of every frame: emit counts run on, a segment's first frame is aligned
        at = 0
        for g in range(geo.shape[0]):
            if geo[g, 0] and geo[g, 6] == -1:
                at = (at + align - 1) // align * align
            pos[g] = at
            at += int(geo[g, 5])
        assert at <= table[-1, 2]
        for g in range(geo.shape[0]):
            n, start, valid, _, es, ec, ov, ol = (int(v) for v in geo[g])
            decoded += n != 0
            if g and n >= 256 and geo[g - 1, 0] >= 256 and ov == g - 1 and es == start and ec == valid - start and \
                    valid % 64 == 0 and (pos[g] * st.channels) % 4 == 0:
                eligible += 1
        st.synth_host(pinned=True)
        k = ",".join(st.kernels())
        named[k] = named.get(k, 0) + 1

    for data in files:
        pa, nxt = nv.demux_ogg_array(data, 0), 3
        while nxt < len(pa):
            room = batch_frames - st.pending()[0]
            if room <= 0:
                flush()
                continue
            took = st.push_packets(pa, nxt, room)
            nxt += took
            if took < room:
                break
        st.next_segment(align)
    flush()
    st.close()
    ctx.close()
    return named, eligible / max(decoded, 1)


def child(mode, workload, length, batch_frames):
    """Runs in the tree PYTHONPATH names (the parent's for the reader modes): one JSON line."""
    import nvorbis_amd as nv
    with open(workload, "rb") as fh:
        files = pickle.load(fh)[length]
    frames = sum(len(nv.demux_ogg_array(f, 0)) - 3 for f in files[:8]) // 8 * len(files)
    out = {"mode": mode, "packets_per_clip": length, "clips": len(files), "frames": frames}

    def read_all(ctx, part):
        n = 0
        for f in part:
            r = nv.VorbisReader(f, ctx=ctx, gpu_parse=True)
            n += r.read_all().size
            r.close()
        return n

    if mode == "reader_seq":
        ctx = nv.Context(0)
        read_all(ctx, files[:32])  # warm-up: library, setup cache, allocations
        t0 = time.perf_counter()
        out["samples"] = read_all(ctx, files)
        dt = time.perf_counter() - t0
        ctx.close()
    elif mode == "reader_t16":
        from concurrent.futures import ThreadPoolExecutor
        ctxs = [nv.Context(0) for _ in range(16)]
        parts = [files[k::16] for k in range(16)]
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda a: read_all(a[0], a[1][:4]), zip(ctxs, parts)))
            t0 = time.perf_counter()
            out["samples"] = sum(ex.map(lambda a: read_all(*a), zip(ctxs, parts)))
            dt = time.perf_counter() - t0
        for c in ctxs:
            c.close()
    elif mode in ("clips_plain", "clips_flags"):
        kw = {"return_clipped": True} if mode == "clips_flags" else {}
        ctx = nv.Context(0)
        nv.decode_clips(files[:32], ctx=ctx, batch_frames=batch_frames, **kw)
        t0 = time.perf_counter()
        res = nv.decode_clips(files, ctx=ctx, batch_frames=batch_frames, gpu_parse=True, align=4, **kw)
        dt = time.perf_counter() - t0
        if kw:
            res, clipped = res
            out["clipped_clips"] = int(clipped.sum())
        out["samples"] = sum(r.size for r in res)
        ctx.close()
    else:
        ctx = nv.Context(0)
        nv.decode_clips(files[:32], ctx=ctx, batch_frames=batch_frames)
        t0 = time.perf_counter()
        res = nv.decode_clips(files, ctx=ctx, batch_frames=batch_frames, gpu_parse=True, align=4)
        dt = time.perf_counter() - t0
        out["samples"] = sum(r.size for r in res)
        ctx.close()
        named, share = paired_share(nv, files, batch_frames, 4)
        out["kernels"], out["paired_share"] = named, share
    out["seconds"] = dt
    out["clips_per_s"], out["frames_per_s"] = len(files) / dt, frames / dt
    print("CLIP_RATES " + json.dumps(out))


def run_child(tree, mode, workload, length, batch_frames):
    env = dict(os.environ, PYTHONPATH=tree)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--workload", workload, "--length", str(length),
           "--batch-frames", str(batch_frames)]
    p = subprocess.run(cmd, cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("CLIP_RATES ")]
    if p.returncode != 0 or not lines:
        raise SystemExit("%s in %s failed (exit %d):\n%s" % (mode, tree, p.returncode, p.stdout[-2000:]))
    return json.loads(lines[-1][len("CLIP_RATES "):])


def bench_headline(tree):
    """`python bench.py --gpus 1 --steps 20 --warmup 5` in `tree`: the headline (frames/s) of its one JSON line."""
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree,
                       env=dict(os.environ, PYTHONPATH=tree), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("bench.py in %s failed (exit %d):\n%s" % (tree, p.returncode, p.stdout[-2000:]))
    return float(json.loads(lines[-1])["value"])


def flags_main(a, parent):
    """--flags: profiles/segment_clipped_rates.txt"""
    workdir = tempfile.mkdtemp(prefix="clip_rates_")
    workload = os.path.join(workdir, "workload.pkl")
    make_workload(a.clips, workload)
    bench, rows = {"parent": [], "branch": []}, {}
    for _ in range(a.runs):  # parent and branch alternate
        for who, tree in (("parent", parent), ("branch", ROOT)):
            bench[who].append(bench_headline(tree))
            print("bench %s %.1f M frames/s" % (who, bench[who][-1] / 1e6), flush=True)
    for length in (40, 8):
        for _ in range(a.runs):
            for who, tree, mode in (("parent", parent, "clips_plain"), ("branch", ROOT, "clips_plain"), ("branch", ROOT, "clips_flags")):
                r = run_child(tree, mode, workload, length, a.batch_frames)
                rows.setdefault((length, who, mode), []).append(r)
                print(who, json.dumps(r), flush=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/clip_rates.py --flags: parent commit against this tree, alternating, %d runs each; min - max over the runs.\n" % a.runs)
        fh.write("# python bench.py --gpus 1 --steps 20 --warmup 5, the headline (frames/s, kernel only):\n")
        for who in ("parent", "branch"):
            fh.write("%-8s %12.0f - %-12.0f  (%s)\n" % (who, min(bench[who]), max(bench[who]),
                                                       ", ".join("%.1f M" % (v / 1e6) for v in bench[who])))
        fh.write("# nv.decode_clips: %d clips per length cut from 3test.ogg, one context, GPU packet parser, f32 interleaved to the host,\n"
                 "# batch_frames %d, align 4.  clips_plain: without the keyword; clips_flags: return_clipped=True.\n" % (a.clips, a.batch_frames))
        fh.write("%-8s %-8s %-12s %-25s %-27s\n" % ("packets", "tree", "mode", "clips/s", "frames/s"))
        for (length, who, mode), rs in rows.items():
            c, f = [r["clips_per_s"] for r in rs], [r["frames_per_s"] for r in rs]
            fh.write("%-8d %-8s %-12s %10.0f - %-12.0f %11.0f - %-13.0f\n" % (length, who, mode, min(c), max(c), min(f), max(f)))
        for (length, who, mode), rs in rows.items():
            if mode == "clips_flags":
                fh.write("# %d packets per clip: %d of %d clips flagged\n" % (length, rs[-1]["clipped_clips"], rs[-1]["clips"]))
    print(open(a.out).read())
    shutil.rmtree(workdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--flags", action="store_true")
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch-frames", type=int, default=4096)
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--workload")
    ap.add_argument("--length", type=int, default=40)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.workload, a.length, a.batch_frames)
    if not a.parent_tree:
        raise SystemExit("--parent-tree: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent_tree)
    a.out = a.out or os.path.join(ROOT, "profiles", "segment_clipped_rates.txt" if a.flags else "clip_batch_rates.txt")
    if a.flags:
        return flags_main(a, parent)
    workdir = tempfile.mkdtemp(prefix="clip_rates_")
    workload = os.path.join(workdir, "workload.pkl")  # (the clips, for the child processes)
    make_workload(a.clips, workload)
    rows = {}
    for length in (40, 8):
        for _ in range(a.runs):  # parent and branch alternate
            for tree, mode in ((parent, "reader_seq"), (ROOT, "decode_clips"), (parent, "reader_t16")):
                r = run_child(tree, mode, workload, length, a.batch_frames)
                rows.setdefault((length, mode), []).append(r)
                print(json.dumps(r), flush=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/clip_rates.py: %d clips per length cut from 3test.ogg, %d runs each, parent and branch alternating;\n"
                 "# one context (16 for the threaded baseline), GPU packet parser, f32 interleaved, batch_frames %d, align 4.\n"
                 "# reader_seq / reader_t16: the parent commit, one VorbisReader per clip, sequentially / on 16 threads;\n"
                 "# decode_clips: this tree.  min - max over the runs.\n" % (a.clips, a.runs, a.batch_frames))
        fh.write("%-8s %-13s %-25s %-27s\n" % ("packets", "mode", "clips/s", "frames/s"))
        for (length, mode), rs in rows.items():
            c, f = [r["clips_per_s"] for r in rs], [r["frames_per_s"] for r in rs]
            fh.write("%-8d %-13s %10.0f - %-12.0f %11.0f - %-13.0f\n" % (length, mode, min(c), max(c), min(f), max(f)))
        for (length, mode), rs in rows.items():
            if mode == "decode_clips":
                fh.write("# %d packets per clip: Stream.kernels() per batch %s; estimated share of frames inside the conditions of paired emission: "
                         "%.3f of the decoded frames (a batch under 7/8 runs without paired emission)\n"
                         % (length, json.dumps(rs[-1]["kernels"]), rs[-1]["paired_share"]))
    print(open(a.out).read())
    shutil.rmtree(workdir, ignore_errors=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the per-row normalisation of features costs: nvh_fnorm_rows alone against the torch expression of the same thing on the same
device tensor.

    python tools/time_fnorm_rows.py [--rows 1024] [--frames 1001] [--bands 80] [--runs 5] [--out profiles/fnorm_rows_rates.txt]

Workload: `--rows` mono rows of `--frames` frames x `--bands` bands (seeded N(-8, 4) values, already on the device), band-major
(rows, B, F) and frame-major (rows, F, B), valid_frames spread evenly over [0, F]; mean and variance per band (NVH_FNORM_MEAN_VAR,
NVH_FNORM_PER_BAND), eps 1e-5, pad_value 0, out of place.  Fused: one nvh_fnorm_rows call (its per-row block's copy and
k_fnorm_rows).  Torch: the mask from valid_frames, the masked mean, the masked variance, subtract, divide, masked_fill.  Both run on
one stream of torch's that the context runs on too, bracketed by events; the two alternate in one process after a warm-up of each,
`--runs` runs each.  Reported: ms per call as min - max, the path the shape took (LDS-resident or re-reading:
NVH_FNORM_RESIDENT_FLOATS), and the largest difference between the two results (they are not the same arithmetic: torch's
reductions round in another order).  No rate is promised anywhere: these are the numbers as measured."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(rows, frames, bands, runs, band_major):
    import numpy as np
    import torch
    import nvorbis_amd as nv
    from nvorbis_amd import clips
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    ctx = nv.Context(0, hip_stream=side.cuda_stream)
    try:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        shape = (rows, bands, frames) if band_major else (rows, frames, bands)
        x = torch.randn(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 8
        vf = np.round(np.linspace(0, frames, rows)).astype(np.int64)
        t_vf = torch.from_numpy(vf).cuda()
        out = torch.empty_like(x)
        desc = clips.fnorm_desc("mean_var", "band", 1e-5, 0.0, frames=frames, bands=bands)
        desc.rows, desc.channels = rows, 1
        fs, bs = (1, frames) if band_major else (bands, 1)
        desc.src_row_stride = desc.dst_row_stride = frames * bands
        desc.src_frame_stride = desc.dst_frame_stride = fs
        desc.src_band_stride = desc.dst_band_stride = bs
        f_axis = 2 if band_major else 1

        def fused():
            ctx.fnorm_rows(desc, x.data_ptr(), out.data_ptr(), vf)
            return out

        def eager():
            mask = torch.arange(frames, device=x.device)[None, :] < t_vf[:, None]
            mask = mask[:, None, :] if band_major else mask[:, :, None]
            n = t_vf.clamp(min=1).to(torch.float32)[:, None, None]
            mean = (x * mask).sum(dim=f_axis, keepdim=True) / n
            d = x - mean
            var = (d * d * mask).sum(dim=f_axis, keepdim=True) / n
            return (d / torch.sqrt(var + 1e-5)).masked_fill(~mask, 0.0)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            r = fn()
            e1.record(side)
            e1.synchronize()
            return e0.elapsed_time(e1), r
        _, a = timed(fused)  # warm-up: allocations, the LDS opt-in
        _, b = timed(eager)
        diff = float((a - b).abs().max())
        del b
        tf, te = [], []
        for _ in range(runs):  # alternating
            tf.append(timed(fused)[0])
            te.append(timed(eager)[0])
        from nvorbis_amd import native
        r = {"layout": "band-major" if band_major else "frame-major", "rows": rows, "frames": frames, "bands": bands,
             "path": "LDS-resident" if (frames | 1) * bands <= native.FNORM_RESIDENT_FLOATS else "re-reading",
             "fused_ms": tf, "torch_ms": te, "max_abs_difference": diff}
        print("FNORM_ROWS " + json.dumps(r), flush=True)
        return r
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--bands", type=int, default=80)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fnorm_rows_rates.txt"))
    a = ap.parse_args()
    lines = ["# tools/time_fnorm_rows.py: %d mono rows of %d frames x %d bands on the device, valid_frames spread over [0, F], mean and"
             % (a.rows, a.frames, a.bands),
             "# variance per band, out of place; one warm-up and %d runs each, the two alternating in one process, timed by events on one" % a.runs,
             "# stream.  fused: nvh_fnorm_rows alone (k_fnorm_rows and its per-row copy); torch: mask, masked mean and variance, subtract,",
             "# divide, masked_fill.",
             "%-12s %-13s %-8s %-21s" % ("layout", "path", "", "ms per call")]
    for band_major in (True, False):
        r = measure(a.rows, a.frames, a.bands, a.runs, band_major)
        lo_f, hi_f, lo_t, hi_t = min(r["fused_ms"]), max(r["fused_ms"]), min(r["torch_ms"]), max(r["torch_ms"])
        lines += ["%-12s %-13s %-8s %8.3f - %-10.3f" % (r["layout"], r["path"], "fused", lo_f, hi_f),
                  "%-12s %-13s %-8s %8.3f - %-10.3f" % (r["layout"], r["path"], "torch", lo_t, hi_t),
                  "# %s: the fused kernel is %s, %.2f - %.2f times torch's time; largest |fused - torch| %.3g (different arithmetic, not an"
                  " error bound)" % (r["layout"], "ahead" if hi_f < lo_t else "NOT ahead" if lo_f > hi_t else "level with torch within the spread",
                                     lo_f / hi_t, hi_f / lo_t, r["max_abs_difference"])]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()

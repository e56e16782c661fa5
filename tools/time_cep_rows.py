#!/usr/bin/env python3
"""What cepstra and deltas of features cost: nvh_cep_rows alone against the torch expression of the same thing on the same device
tensor.

    python tools/time_cep_rows.py [--rows 1024] [--frames 1001] [--bands 80] [--ceps 13] [--lifter 22] [--order 2] [--window 2]
                                  [--runs 5] [--out profiles/cep_rows_rates.txt]

Workload: `--rows` mono rows of `--frames` frames x `--bands` bands (seeded N(-8, 4) values, already on the device), band-major
(rows, B, F) -> (rows, Q, F) and frame-major (rows, F, B) -> (rows, F, Q); `--ceps` DCT-II coefficients (ortho, the lifter folded in),
deltas of `--order` orders over `--window` frames; every frame counted (valid_frames NULL: torch's padding knows no per-row
count).  Fused: one nvh_cep_rows call.  Torch: a matmul with the same f32 table (nvh_cep_tables'), then per order a replicate pad
and a conv1d with the same f32 scales, and the concatenation.  Both run on one stream of torch's that the context runs on too,
bracketed by events; the two alternate in one process after a warm-up of each, `--runs` runs each.  Reported: ms per call as min -
max, the route the shape took, and the largest difference between the two results (they are not the same arithmetic: torch's
matmul rounds in another order, and its second order sees repeated cepstra only through s_2's padding).  No rate is promised
anywhere: these are the numbers as measured."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(a, band_major):
    import torch
    import torch.nn.functional as Fn
    import nvorbis_amd as nv
    from nvorbis_amd import clips, native
    rows, frames, bands, K, o, N = a.rows, a.frames, a.bands, a.ceps, a.order, a.window
    Q = (1 + o) * K
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    ctx = nv.Context(0, hip_stream=side.cuda_stream)
    try:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        x = torch.randn((rows, bands, frames) if band_major else (rows, frames, bands), generator=gen, device="cuda", dtype=torch.float32) * 2 - 8
        out = torch.empty((rows, Q, frames) if band_major else (rows, frames, Q), device="cuda", dtype=torch.float32)
        desc = clips.cep_desc(K, "ortho", a.lifter, o, N, frames, bands)
        desc.rows, desc.channels = rows, 1
        desc.src_row_stride, desc.dst_row_stride = frames * bands, frames * Q
        desc.src_frame_stride, desc.src_band_stride = (1, frames) if band_major else (bands, 1)
        desc.dst_frame_stride, desc.dst_col_stride = (1, frames) if band_major else (Q, 1)
        route = (C.c_int64 * 4)()
        native.check(native.lib().nvh_cep_route(C.byref(desc), route), "nvh_cep_route")
        D, s1, s2 = clips.cep_tables(bands, K, "ortho", a.lifter, N)
        t_D = torch.from_numpy(D).cuda()
        t_s = [torch.from_numpy(s.copy()).cuda()[None, None, :].repeat(K, 1, 1) for s in (s1, s2)][:o]  # (K, 1, taps): one filter per cepstrum

        def fused():
            ctx.cep_rows(desc, x.data_ptr(), out.data_ptr(), None)
            return out

        def eager():
            c = torch.matmul(t_D, x) if band_major else torch.matmul(x, t_D.t()).transpose(1, 2)  # (rows, K, F)
            parts = [c]
            for m, w in enumerate(t_s, 1):
                parts.append(Fn.conv1d(Fn.pad(c, (m * N, m * N), mode="replicate"), w, groups=K))
            y = torch.cat(parts, dim=1)
            return y if band_major else y.transpose(1, 2).contiguous()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            r = fn()
            e1.record(side)
            e1.synchronize()
            return e0.elapsed_time(e1), r
        _, p = timed(fused)  # warm-up: allocations, the table, the LDS opt-in
        _, q = timed(eager)
        diff = float((p - q).abs().max())
        del q
        tf, te = [], []
        for _ in range(a.runs):  # alternating
            tf.append(timed(fused)[0])
            te.append(timed(eager)[0])
        r = {"layout": "band-major" if band_major else "frame-major", "rows": rows, "frames": frames, "bands": bands, "ceps": K, "order": o,
             "window": N, "route": "table in LDS" if route[0] else "table through the caches", "lds_bytes": int(route[1]),
             "workgroups": int(route[2]), "fused_ms": tf, "torch_ms": te, "max_abs_difference": diff}
        print("CEP_ROWS " + json.dumps(r), flush=True)
        return r
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--bands", type=int, default=80)
    ap.add_argument("--ceps", type=int, default=13)
    ap.add_argument("--lifter", type=float, default=22.0)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--window", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cep_rows_rates.txt"))
    a = ap.parse_args()
    lines = ["# tools/time_cep_rows.py: %d mono rows of %d frames x %d bands on the device -> %d cepstra (ortho, lifter %g), deltas of order %d"
             % (a.rows, a.frames, a.bands, a.ceps, a.lifter, a.order),
             "# over N = %d, every frame counted, out of place; one warm-up and %d runs each, the two alternating in one process, timed by" % (a.window, a.runs),
             "# events on one stream.  fused: nvh_cep_rows alone (k_cep_rows); torch: matmul with the same f32 table, then per order a",
             "# replicate pad and a grouped conv1d with the same f32 scales, and the concatenation.",
             "%-12s %-26s %-8s %-21s" % ("layout", "route", "", "ms per call")]
    for band_major in (True, False):
        r = measure(a, band_major)
        lo_f, hi_f, lo_t, hi_t = min(r["fused_ms"]), max(r["fused_ms"]), min(r["torch_ms"]), max(r["torch_ms"])
        lines += ["%-12s %-26s %-8s %8.3f - %-10.3f" % (r["layout"], r["route"], "fused", lo_f, hi_f),
                  "%-12s %-26s %-8s %8.3f - %-10.3f" % (r["layout"], r["route"], "torch", lo_t, hi_t),
                  "# %s (%d bytes of LDS, %d workgroups): the fused kernel is %s, %.2f - %.2f times torch's time; largest |fused - torch| %.3g"
                  " (different arithmetic, not an error bound)"
                  % (r["layout"], r["lds_bytes"], r["workgroups"],
                     "ahead" if hi_f < lo_t else "NOT ahead" if lo_f > hi_t else "level with torch within the spread", lo_f / hi_t, hi_f / lo_t,
                     r["max_abs_difference"])]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What log-mel features of rows cost: nvh_mel_rows alone against torch.stft + a filter-bank matmul + log on the same device rows.

    python tools/time_mel_rows.py [--rows 1024] [--seconds 10] [--runs 5] [--out profiles/mel_rows_rates.txt]

Workload: `--rows` mono rows of `--seconds` seconds at 16 kHz (seeded noise, already on the device), n_fft 512, win_length 400, hop
160, 80 HTK bands, natural logarithm with floor 1e-10, centred frames: (rows, 80, F) band-major, F = length // 160 + 1.  Fused:
one nvh_mel_rows call (its per-row block's copy and k_mel_rows).  Torch: torch.stft(center=True, pad_mode="constant") with the
library's window, |.|^2, torch.matmul with the library's bank, clamp, log.  Both run on one stream of torch's that the context
runs on too, bracketed by events; the two alternate in one process after a warm-up of each, `--runs` runs each.  Reported: ms per
call as min - max, rows/s from them, and the largest difference between the two results (they are not the same arithmetic: torch's
transform and matmul round differently from the rule, and differ between torch builds).  No rate is promised anywhere: these are
the numbers as measured."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(rows, seconds, runs):
    import numpy as np
    import torch
    import nvorbis_amd as nv
    from nvorbis_amd import clips
    rate, n_fft, win_length, hop, n_mels = 16000, 512, 400, 160, 80
    length = rate * seconds
    frames = length // hop + 1
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    ctx = nv.Context(0, hip_stream=side.cuda_stream)
    try:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        x = torch.rand((rows, length), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1
        _, win, fb = clips.mel_tables(rate, n_fft, win_length, n_mels)
        t_win, t_fb = torch.from_numpy(win.copy()).cuda(), torch.from_numpy(fb.copy()).cuda()
        desc = clips.mel_desc(rate, n_fft, win_length, hop, n_mels)
        out = torch.empty((rows, n_mels, frames), dtype=torch.float32, device="cuda")
        desc.rows, desc.channels, desc.frames, desc.first, desc.src_length = rows, 1, frames, (n_fft - win_length) // 2 - n_fft // 2, length
        desc.src_row_stride, desc.src_time_stride, desc.src_chan_stride = length, 1, 0
        desc.dst_row_stride, desc.dst_chan_stride, desc.dst_band_stride, desc.dst_frame_stride = n_mels * frames, 0, frames, 1

        def fused():
            ctx.mel_rows(desc, x.data_ptr(), out.data_ptr(), None)
            return out

        def eager():
            spec = torch.stft(x, n_fft, hop_length=hop, win_length=win_length, window=t_win, center=True, pad_mode="constant",
                              return_complex=True)
            power = spec.real * spec.real + spec.imag * spec.imag
            return torch.log(torch.clamp(torch.matmul(t_fb, power), min=1e-10))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            r = fn()
            e1.record(side)
            e1.synchronize()
            return e0.elapsed_time(e1), r
        _, a = timed(fused)  # warm-up: tables, plans, allocations
        _, b = timed(eager)
        diff = float((a - b).abs().max())
        del b
        tf, te = [], []
        for _ in range(runs):  # alternating
            tf.append(timed(fused)[0])
            te.append(timed(eager)[0])
        r = {"rows": rows, "seconds": seconds, "frames": frames, "fused_ms": tf, "torch_ms": te, "max_abs_difference": diff}
        print("MEL_ROWS " + json.dumps(r), flush=True)
        return r
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_rows_rates.txt"))
    a = ap.parse_args()
    r = measure(a.rows, a.seconds, a.runs)
    lo_f, hi_f, lo_t, hi_t = min(r["fused_ms"]), max(r["fused_ms"]), min(r["torch_ms"]), max(r["torch_ms"])
    lines = ["# tools/time_mel_rows.py: %d mono rows of %d s at 16 kHz on the device, n_fft 512, win_length 400, hop 160, 80 HTK bands, ln,"
             % (a.rows, a.seconds),
             "# %d frames per row; one warm-up and %d runs each, the two alternating in one process, timed by events on one stream."
             % (r["frames"], a.runs),
             "# fused: nvh_mel_rows alone (k_mel_rows and its per-row copy); torch: torch.stft + |.|^2 + matmul + clamp + log.",
             "%-8s %-21s %-21s" % ("", "ms per call", "rows/s"),
             "%-8s %8.2f - %-10.2f %8.0f - %-10.0f" % ("fused", lo_f, hi_f, a.rows / hi_f * 1e3, a.rows / lo_f * 1e3),
             "%-8s %8.2f - %-10.2f %8.0f - %-10.0f" % ("torch", lo_t, hi_t, a.rows / hi_t * 1e3, a.rows / lo_t * 1e3),
             "# the fused kernel is %s: %.2f - %.2f times torch's time" % ("ahead" if hi_f < lo_t else "NOT ahead" if lo_f > hi_t else
                                                                          "level with torch within the spread", lo_f / hi_t, hi_f / lo_t),
             "# largest |fused - torch| over all values: %.3g (natural-log units; different arithmetic, not an error bound)" % r["max_abs_difference"]]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the front of a frame costs: nvh_mel_rows_front with Kaldi's front against the default call, and the default call against
another build's.

    python tools/time_mel_front.py [--rows 1024] [--seconds 10] [--runs 5] [--calls 20] [--other-lib PATH/libnvorbis_hip.so]
                                   [--out profiles/mel_front_rates.txt]

Workload: that of tools/time_mel_rows.py -- `--rows` mono rows of `--seconds` seconds at 16 kHz (seeded noise, already on the
device), n_fft 512, win_length 400, hop 160, 80 HTK bands, natural logarithm, band-major output.
  default   nvh_mel_rows: centred frames, periodic Hann, zero padding, floor 1e-10 (F = length // 160 + 1).
  kaldi     nvh_mel_rows_front with kaldi_fbank_keywords(16000): gain 32768, DC removal, pre-emphasis 0.97, Povey window, triangles
            linear in mel over [20, 8000] Hz, floor 2^-23, frames by the window (F = (length - 400) // 160 + 1, three fewer).
  reflect   nvh_mel_rows_front with NVH_PAD_REFLECT alone, the default call's frames.
  other     nvh_mel_rows of the library given with --other-lib (the parent commit's build, say), loaded beside this one into the
            same process, on a context of its own on the same stream; its output is compared with `default` bit for bit.
The variants alternate in one process after a warm-up of each (every run begins with another one); a run is `--calls` calls
between two events on one stream, `--runs` runs each.  Reported: ms per call as min - max over the runs, and rows/s from them.  No
rate is promised anywhere: these are the numbers as measured."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(rows, seconds, runs, calls, other_lib):
    import torch
    import nvorbis_amd as nv
    from nvorbis_amd import clips, native
    rate = 16000
    length = rate * seconds
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    ctx = nv.Context(0, hip_stream=side.cuda_stream)
    other = other_ctx = None
    try:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        x = torch.rand((rows, length), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1

        def shaped(desc, frames, first):
            desc.rows, desc.channels, desc.frames, desc.first, desc.src_length = rows, 1, frames, first, length
            desc.src_row_stride, desc.src_time_stride, desc.src_chan_stride = length, 1, 0
            desc.dst_row_stride, desc.dst_chan_stride, desc.dst_band_stride, desc.dst_frame_stride = desc.n_mels * frames, 0, frames, 1
            return desc, torch.empty((rows, desc.n_mels, frames), dtype=torch.float32, device="cuda")
        d_def, out_def = shaped(clips.mel_desc(rate, 512, 400, 160, 80), length // 160 + 1, (512 - 400) // 2 - 256)
        kw = nv.kaldi_fbank_keywords(rate)
        d_kal, out_kal = shaped(clips.mel_desc(rate, kw["n_fft"], kw["win_length"], kw["hop"], kw["n_mels"], kw["f_min"], kw["f_max"],
                                               kw["mel_scale"], None, kw["scale"], kw["floor"]), (length - kw["win_length"]) // kw["hop"] + 1, 0)
        f_kal = clips.mel_front(kw["window"], kw["mel_triangles"], "constant", kw["remove_dc"], kw["preemphasis"], kw["sample_gain"])
        d_ref, out_ref = shaped(clips.mel_desc(rate, 512, 400, 160, 80), length // 160 + 1, (512 - 400) // 2 - 256)
        f_ref = clips.mel_front(pad_mode="reflect")
        variants = {"default": lambda: ctx.mel_rows(d_def, x.data_ptr(), out_def.data_ptr(), None),
                    "kaldi": lambda: ctx.mel_rows(d_kal, x.data_ptr(), out_kal.data_ptr(), None, f_kal),
                    "reflect": lambda: ctx.mel_rows(d_ref, x.data_ptr(), out_ref.data_ptr(), None, f_ref)}
        if other_lib:
            other = C.CDLL(os.path.abspath(other_lib))
            other.nvh_version.restype = C.c_char_p
            other_ctx = C.c_void_p()
            native.check(other.nvh_ctx_create(0, C.byref(other_ctx)), "nvh_ctx_create (other)")
            native.check(other.nvh_ctx_set_hip_stream(other_ctx, C.c_void_p(side.cuda_stream)), "nvh_ctx_set_hip_stream (other)")
            d_oth, out_oth = shaped(clips.mel_desc(rate, 512, 400, 160, 80), length // 160 + 1, (512 - 400) // 2 - 256)
            variants["other"] = lambda: native.check(other.nvh_mel_rows(other_ctx, C.byref(d_oth), C.c_void_p(x.data_ptr()),
                                                                        C.c_void_p(out_oth.data_ptr()), None), "nvh_mel_rows (other)")

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(calls):
                fn()
            e1.record(side)
            e1.synchronize()
            return e0.elapsed_time(e1) / calls
        for fn in variants.values():  # warm-up: tables, code objects
            timed(fn)
        ms = {name: [] for name in variants}
        names = list(variants)
        for i in range(runs):  # alternating, every run beginning with another variant
            for name in names[i % len(names):] + names[:i % len(names)]:
                ms[name].append(timed(variants[name]))
        r = {"rows": rows, "seconds": seconds, "calls": calls, "frames": {"default": d_def.frames, "kaldi": d_kal.frames}, "ms": ms}
        if other_lib:
            r["other_version"] = other.nvh_version().decode()
            r["other_same_bits"] = bool((out_oth.view(torch.int32) == out_def.view(torch.int32)).all())
        print("MEL_FRONT " + json.dumps(r), flush=True)
        return r
    finally:
        if other_ctx:
            other.nvh_ctx_destroy.argtypes = [C.c_void_p]
            other.nvh_ctx_destroy(other_ctx)
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--note", action="append", default=[], help="a line to append to the file (the compiler's resource figures, say)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_front_rates.txt"))
    a = ap.parse_args()
    r = measure(a.rows, a.seconds, a.runs, a.calls, a.other_lib)
    lines = ["# tools/time_mel_front.py: %d mono rows of %d s at 16 kHz on the device, n_fft 512, win_length 400, hop 160, 80 bands, ln;"
             % (a.rows, a.seconds),
             "# %d frames per row (kaldi: %d); one warm-up and %d runs of %d calls each, the variants alternating in one process, timed"
             % (r["frames"]["default"], r["frames"]["kaldi"], a.runs, a.calls),
             "# by events on one stream.  default: nvh_mel_rows; kaldi: nvh_mel_rows_front with gain 32768, DC removal, pre-emphasis 0.97,",
             "# Povey window, mel-domain triangles; reflect: nvh_mel_rows_front with NVH_PAD_REFLECT alone; other: nvh_mel_rows of",
             "# another build in the same process.",
             "%-8s %-21s %-21s" % ("", "ms per call", "rows/s")]
    for name, v in r["ms"].items():
        lines.append("%-8s %8.3f - %-10.3f %8.0f - %-10.0f" % (name, min(v), max(v), a.rows / max(v) * 1e3, a.rows / min(v) * 1e3))
    d = r["ms"]["default"]
    for name in ("kaldi", "reflect"):
        v = r["ms"][name]
        lines.append("# %s takes %.3f - %.3f times the default call's time" % (name, min(v) / max(d), max(v) / min(d)))
    if "other" in r["ms"]:
        o = r["ms"]["other"]
        where = ("inside" if min(o) <= min(d) and max(d) <= max(o) else "below (faster than)" if max(d) < min(o) else
                 "above (SLOWER than)" if min(d) > max(o) else "across an end of")
        lines.append("# other: %s; its output and the default call's are %s;" % (r["other_version"], "the same bits" if r["other_same_bits"]
                                                                                 else "NOT the same bits"))
        lines.append("# the default call takes %.4f - %.4f times the other build's time and lies %s the other build's own spread"
                     % (min(d) / max(o), max(d) / min(o), where))
    lines += ["# " + n for n in a.note]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()

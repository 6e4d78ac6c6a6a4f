"""colordetect timing: mi355_colordetect_frame (one host frame) and mi355_colordetect_frames_device (a batch of device frames)
at 1080p and 4K, the five formats, quality 1 and 10, max-colors 2 and 255, on smooth (synth.smooth_frame), noise and solid red
content. Every call ends in a stream synchronisation, so a host clock around it times the work; the median of --reps calls
after one warm-up call is reported.

Algorithmic bytes = data_len per frame: with quality * ch <= 40 every 128-byte line of the plane is touched, so the whole plane
is read. A host frame also crosses PCIe (data_len up, the palette down): its time is a transfer time, not a kernel time.

  python tools/bench_colordetect.py [--reps N] [--batch 8] [--sizes 1080p,4k]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))

import mi355fx  # noqa: E402
from mi355fx import synth  # noqa: E402

SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
FORMATS = {"RGB": 3, "RGBA": 4, "ARGB": 4, "BGR": 3, "BGRA": 4}
RED = {"RGB": (255, 0, 0), "RGBA": (255, 0, 0, 255), "ARGB": (255, 255, 0, 0), "BGR": (0, 0, 255), "BGRA": (0, 0, 255, 255)}


def content(kind, fmt, w, h):
    ch = FORMATS[fmt]
    if kind == "smooth":
        rgba = synth.smooth_frame(w, h).reshape(-1, 4)
        return np.ascontiguousarray(rgba[:, :ch]).reshape(-1) if ch == 3 else rgba.reshape(-1)
    if kind == "noise":
        return synth.noise_frame(w, h, channels=ch).reshape(-1)
    return np.tile(np.array(RED[fmt], np.uint8), w * h)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sizes", default="1080p,4k")
    a = ap.parse_args()
    print("%-6s %-5s %-7s %2s %4s | %12s %9s | %12s %9s %8s" % ("size", "fmt", "content", "q", "maxc", "host us/frm", "GB/s", "dev us/batch", "TB/s", "colours"))
    with mi355fx.Context(0) as ctx:
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for fmt, ch in FORMATS.items():
                data_len = w * h * ch
                d = ctx.alloc(data_len * a.batch)
                try:
                    for kind in ("smooth", "noise", "red"):
                        frame = content(kind, fmt, w, h)
                        assert frame.nbytes == data_len
                        for f in range(a.batch):
                            ctx.h2d(d + f * data_len, frame)
                        for q in (1, 10):
                            for mc in (2, 255):
                                t_host = timed(lambda: ctx.colordetect_frame(frame, fmt, q, mc), a.reps)
                                t_dev = timed(lambda: ctx.colordetect_frames_device(d, data_len, data_len, a.batch, fmt, q, mc), a.reps)
                                pal_host = ctx.colordetect_frame(frame, fmt, q, mc)
                                pal_dev = ctx.colordetect_frames_device(d, data_len, data_len, a.batch, fmt, q, mc)
                                assert all(p == pal_host for p in pal_dev), (size, fmt, kind, q, mc)
                                print("%-6s %-5s %-7s %2d %4d | %12.1f %9.1f | %12.1f %9.2f %8d" % (
                                    size, fmt, kind, q, mc, t_host * 1e6, data_len / t_host / 1e9, t_dev * 1e6,
                                    data_len * a.batch / t_dev / 1e12, len(pal_host)), flush=True)
                finally:
                    ctx.free(d)


if __name__ == "__main__":
    main()

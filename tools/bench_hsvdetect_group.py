"""hsvdetector of many independent instances: 32 instances, one RGBx -> RGBA device frame each per interval, at 1080p
and at 4K, in two modes:

  lone   32 contexts driven from 32 threads: every instance calls mi355_hsvdetect_frames_device on its own HIP stream and
         synchronises it (one launch, one synchronisation per frame) - what 32 elements do without the switch;
  group  the same 32 threads submit to the video group's hsvdetector queue with a rendezvous of 32 and wait for their frame
         (one launch per interval for packed frames).

An interval starts when every thread has passed a barrier and ends when every thread's frame is complete (a second barrier), so the
host clock around it times work that ended in a device synchronisation. Both modes pay the same two barriers. Per size the modes
alternate (lone, group, lone, group); each run is --warmup untimed intervals, then --intervals timed ones; the median interval of
each run is printed, and the median over both runs of a mode with the frames/s it amounts to. Both modes must have written
identical bytes.

With --no-threads one thread drives all instances: an interval is N lone calls and then N synchronisations, or N submits and
then N waits (the N-th submit fills the rendezvous and the set goes out). No barrier, lock hand-over or condition variable is in
that figure: it is the one to compare two builds of the library by.

  python tools/bench_hsvdetect_group.py [--instances N] [--intervals K] [--warmup W] [--no-threads] [--out FILE]
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))

import mi355fx  # noqa: E402
from mi355fx import synth  # noqa: E402

SETTINGS = (120.0, 40.0, 0.8, 0.5, 0.7, 0.6)   # a hue on the dial: both alpha values occur on the smooth frame


def run(n, call, warm, reps):
    """`call(s)` on thread s once per interval; the median and the spread of the timed intervals, by thread 0's clock."""
    bar = threading.Barrier(n)
    ts, errors = [], []

    def instance(s):
        try:
            for k in range(warm + reps):
                bar.wait()
                t0 = time.perf_counter()
                call(s)
                bar.wait()
                if s == 0 and k >= warm:
                    ts.append(time.perf_counter() - t0)
        except Exception as e:   # a failed call must not leave the others at the barrier
            errors.append(e)
            bar.abort()

    threads = [threading.Thread(target=instance, args=(s,)) for s in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def run_one_thread(interval, warm, reps):
    """`interval()` on this thread, once per interval; the median and the spread of the timed ones."""
    ts = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        interval()
        if k >= warm:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-threads", action="store_true", help="one thread drives all instances (N submits, then N waits; N lone calls, then N synchronisations)")
    ap.add_argument("--instances", type=int, default=32)
    ap.add_argument("--intervals", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    n = a.instances
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("hsvdetector, %d instances, one RGBx -> RGBA device frame each per interval; %d warm-up + %d timed intervals per run" % (n, a.warmup, a.intervals))
    say("%-10s | %-38s | %-38s | %s" % ("size", "lone: %d contexts on %d threads" % (n, 1 if a.no_threads else n), "group: rendezvous of %d" % n, "group / lone"))
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    g = mi355fx.Group(0)
    g.set_hsvdetect_rendezvous(n, 2_000_000)
    try:
        for w, h in ((1920, 1080), (3840, 2160)):
            n_bytes = w * h * 4
            src = [c.alloc(n_bytes) for c in ctxs]
            dst_lone = [c.alloc(n_bytes) for c in ctxs]
            dst_group = [c.alloc(n_bytes) for c in ctxs]
            try:
                made = {}
                for s, c in enumerate(ctxs):   # four different frames, dealt out in turn
                    host = made.get(s % 4)
                    if host is None:
                        host = made[s % 4] = synth.smooth_frame(w, h, seed=7 + s % 4).reshape(-1)
                    c.h2d(src[s], host)
                    c.synchronize()

                def lone(s):
                    ctxs[s].hsvdetect_frames_device(src[s], 0, w * 4, "RGBx", dst_lone[s], 0, w * 4, "RGBA", 1, w, h, SETTINGS)
                    ctxs[s].synchronize()

                def grouped(s):
                    g.wait_hsvdetect(g.submit_hsvdetect(ctxs[s], src[s], w * 4, "RGBx", dst_group[s], w * 4, "RGBA", w, h, SETTINGS))

                before = g.hsvdetect_stats()
                res = {"lone": [], "group": []}
                def lone_interval():
                    for s in range(n):
                        ctxs[s].hsvdetect_frames_device(src[s], 0, w * 4, "RGBx", dst_lone[s], 0, w * 4, "RGBA", 1, w, h, SETTINGS)
                    for s in range(n):
                        ctxs[s].synchronize()

                def group_interval():
                    tk = [g.submit_hsvdetect(ctxs[s], src[s], w * 4, "RGBx", dst_group[s], w * 4, "RGBA", w, h, SETTINGS) for s in range(n)]
                    for t in tk:
                        g.wait_hsvdetect(t)

                for _ in range(2):
                    if a.no_threads:
                        res["lone"].append(run_one_thread(lone_interval, a.warmup, a.intervals))
                        res["group"].append(run_one_thread(group_interval, a.warmup, a.intervals))
                    else:
                        res["lone"].append(run(n, lone, a.warmup, a.intervals))
                        res["group"].append(run(n, grouped, a.warmup, a.intervals))
                after = g.hsvdetect_stats()
                alphas = set()
                for s, c in enumerate(ctxs):
                    x, y = np.zeros(n_bytes, np.uint8), np.zeros(n_bytes, np.uint8)
                    c.d2h(x, dst_lone[s])
                    c.d2h(y, dst_group[s])
                    assert (x == y).all(), "instance %d: the group's bytes differ from the lone ones" % s
                    alphas |= set(np.unique(y[3::4]).tolist())
                assert alphas == {0, 255}, alphas
                cols, meds = [], []
                for mode in ("lone", "group"):
                    med = float(np.median([r[0] for r in res[mode]]))
                    meds.append(med)
                    cols.append("%8.0f frames/s  %7.3f ms (%s)" % (n / med, med * 1e3, ", ".join("%.3f" % (r[0] * 1e3) for r in res[mode])))
                say("%-10s | %-38s | %-38s | %.2fx the frames/s" % ("%dx%d" % (w, h), cols[0], cols[1], meds[0] / meds[1]))
                sets, done = after[1] - before[1], after[0] - before[0]
                say("%-10s | %-38s | frames per launch set %.1f, launches per set %.2f; identical bytes in both modes" %
                    ("", "", done / max(sets, 1), (after[3] - before[3]) / max(sets, 1)))
            finally:
                for c, bufs in zip(ctxs, zip(src, dst_lone, dst_group)):
                    for d in bufs:
                        c.free(d)
    finally:
        g.close()
        for c in ctxs:
            c.close()
    say("ms: median interval of a mode over its two runs (each run's median in brackets); frames/s = instances / that median")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

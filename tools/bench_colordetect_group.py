"""colordetect of many independent instances: 32 instances, one 4K RGBA device frame each per interval, max-colors 2,
quality 10 and 1, on smooth, solid and noise content, in two modes:

  lone   32 contexts driven from 32 threads: every instance calls mi355_colordetect_frames_device on its own HIP stream
         (two launches, one copy, one synchronisation per frame) - what 32 elements do without the switch;
  group  the same 32 threads submit to the video group's colordetect queue with a rendezvous of 32 and wait for their palette
         (one histogram launch, one MMCQ launch, one copy per interval).

An interval starts when every thread has passed a barrier and ends when every thread has its palette (a second barrier), so the
host clock around it times work that ended in a device synchronisation. Both modes pay the same two barriers. Per case the modes
alternate (lone, group, lone, group); each run is --warmup untimed intervals, then --intervals timed ones; the median interval of
each run is printed, and the median over both runs of a mode with the frames/s it amounts to.

With --no-threads one thread drives all instances: an interval is N lone calls, or N submits followed by N waits (the N-th
submit fills the rendezvous, the set goes out, the first wait takes its time). No barrier, lock hand-over or condition variable
is in that figure: it is the one to compare two builds of the library by.

  python tools/bench_colordetect_group.py [--instances N] [--intervals K] [--warmup W] [--no-threads] [--out FILE]
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

W, H = 3840, 2160


def content(kind, s):
    if kind == "smooth":
        return synth.smooth_frame(W, H, seed=7 + s % 4).reshape(-1)
    if kind == "noise":
        return synth.noise_frame(W, H, seed=11 + s % 4).reshape(-1)
    px = np.array([(37 * s) % 251, (91 * s + 40) % 251, (13 * s + 200) % 251, 255], np.uint8)   # solid: one colour per instance
    return np.tile(px, W * H)


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
    ap.add_argument("--no-threads", action="store_true", help="one thread drives all instances (N submits, then N waits)")
    ap.add_argument("--instances", type=int, default=32)
    ap.add_argument("--intervals", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    n, n_bytes = a.instances, W * H * 4
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("colordetect, %d instances, one %dx%d RGBA device frame each per interval, max-colors 2; %d warm-up + %d timed intervals per run" %
        (n, W, H, a.warmup, a.intervals))
    say("%-8s %-8s | %-38s | %-38s" % ("content", "quality", "lone: %d contexts on %d threads" % (n, 1 if a.no_threads else n), "group: rendezvous of %d" % n))
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    frames = [c.alloc(n_bytes) for c in ctxs]
    g = mi355fx.Group(0)
    g.set_colordetect_rendezvous(n, 2_000_000)
    try:
        for kind in ("smooth", "solid", "noise"):
            made = {}
            for s, c in enumerate(ctxs):
                if kind == "solid":
                    host = content(kind, s)
                else:   # four different frames, dealt out in turn
                    host = made.get(s % 4)
                    if host is None:
                        host = made[s % 4] = content(kind, s)
                c.h2d(frames[s], host)
                c.synchronize()
            for q in (10, 1):
                got = [[None, None] for _ in range(n)]

                def lone(s):
                    got[s][0] = ctxs[s].colordetect_frames_device(frames[s], n_bytes, n_bytes, 1, "RGBA", q, 2)[0]

                def grouped(s):
                    got[s][1] = g.wait_colordetect(g.submit_colordetect(ctxs[s], frames[s], n_bytes, "RGBA", q, 2))

                before = g.colordetect_stats()
                res = {"lone": [], "group": []}
                def lone_interval():
                    for s in range(n):
                        lone(s)

                def group_interval():
                    tk = [g.submit_colordetect(ctxs[s], frames[s], n_bytes, "RGBA", q, 2) for s in range(n)]
                    for s in range(n):
                        got[s][1] = g.wait_colordetect(tk[s])

                for _ in range(2):
                    if a.no_threads:
                        res["lone"].append(run_one_thread(lone_interval, a.warmup, a.intervals))
                        res["group"].append(run_one_thread(group_interval, a.warmup, a.intervals))
                    else:
                        res["lone"].append(run(n, lone, a.warmup, a.intervals))
                        res["group"].append(run(n, grouped, a.warmup, a.intervals))
                after = g.colordetect_stats()
                assert all(x == y and len(x) >= 1 for x, y in got), "group palettes differ from the lone ones"
                cols = []
                for mode in ("lone", "group"):
                    med = float(np.median([r[0] for r in res[mode]]))
                    cols.append("%8.0f frames/s  %7.3f ms (%s)" % (n / med, med * 1e3, ", ".join("%.3f" % (r[0] * 1e3) for r in res[mode])))
                say("%-8s %-8d | %-38s | %-38s" % (kind, q, cols[0], cols[1]))
                sets, done = after[1] - before[1], after[0] - before[0]
                say("%-8s %-8s | %-38s | frames per launch set %.1f, launches per set %.2f" %
                    ("", "", "", done / max(sets, 1), (after[3] - before[3]) / max(sets, 1)))
    finally:
        g.close()
        for c, d in zip(ctxs, frames):
            c.free(d)
            c.close()
    say("ms: median interval of a mode over its two runs (each run's median in brackets); frames/s = instances / that median")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

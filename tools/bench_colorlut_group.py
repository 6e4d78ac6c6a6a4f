"""colorlut frames in the colorlut queue of the video group against lone contexts: 32 independent `colorlut`
instances, each with its own context, its own LUT and its own device frames, grading one frame per interval. One thread, no thread
noise. Five legs:

  (i)   32 x 640x640 RGBA, 32 different seeded 33^3 LUTs
  (ii)  32 x 1920x1080 RGBA, 32 LUTs
  (iii) 32 x 3840x2160 RGBA, 32 LUTs
  (iv)  32 x 1920x1080 RGBA64_LE, 32 LUTs
  (v)   32 x 1920x1080 RGBA, ONE LUT loaded in all 32 contexts

  lone  : 32 mi355_colorlut_frames_device calls with n_frames = 1 on the 32 contexts at their default flags (whatever route the
          lone dispatch and its auto-pick settle on), then a synchronisation of each.
  group : 32 mi355_group_submit_colorlut then 32 mi355_group_wait_colorlut - one set: one launch of colorlut_jobs_kernel (RGBA) or
          of colorlut_rows_jobs_kernel (RGBA64).

Both ways run in the same process, INTERLEAVED: after --warmup intervals of both (the lone way's auto-pick measures and settles in
them; the kernel each context ended on is reported), --rounds rounds, each --block lone intervals then --block group intervals
(default 20 x 50 = 1000 timed intervals per way), a host clock around every interval. Per way: the median, the 5th and 95th
percentile and the spread (half of p95 - p5). Before the timing each leg grades the same sources into two destinations, lone and
through the group, and compares them byte for byte. No ratio is fixed in advance; a leg that is slower through the group is reported
as it is.

  python tools/bench_colorlut_group.py [--rounds R] [--block B] [--warmup W] [--legs i,ii,iii,iv,v] [--out profiles/colorlut_group.txt] [--child]

--child is what a profiler watches (`rocprofv3 --kernel-trace --stats -- python tools/bench_colorlut_group.py --child`): leg (ii)'s
32 members, alternately one set of 32 through the queue (colorlut_jobs_kernel) and 32 lone launches of whatever the lone route picks;
100 warm-up pairs, then 100 timed ones. `--kernel-stats DIR` prints the kernels' durations over the timed pairs from the trace's
database under DIR.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))

import mi355fx  # noqa: E402
from mi355fx import synth  # noqa: E402
from mi355fx.cube import parse_cube  # noqa: E402

MEMBERS = 32
LEGS = {
    "i": ("32 x 640x640 RGBA, 32 LUTs (33^3)", 640, 640, "RGBA", False),
    "ii": ("32 x 1920x1080 RGBA, 32 LUTs (33^3)", 1920, 1080, "RGBA", False),
    "iii": ("32 x 3840x2160 RGBA, 32 LUTs (33^3)", 3840, 2160, "RGBA", False),
    "iv": ("32 x 1920x1080 RGBA64_LE, 32 LUTs (33^3)", 1920, 1080, "RGBA64_LE", False),
    "v": ("32 x 1920x1080 RGBA, ONE LUT (33^3)", 1920, 1080, "RGBA", True),
}


def seeded_lut(k):
    """A 33^3 LUT of its own per camera: the synthetic grade with another amplitude, so that no two tables are alike."""
    return parse_cube(synth.cube_text_3d(33, amp=0.02 + 0.002 * k))


def picture(base, fmt, seed):
    """Camera `seed`'s frame: the synthetic picture `base` ([h, w, 4] bytes) shifted sideways, widened to 16 bits for RGBA64."""
    rgba = np.roll(base, 97 * seed, axis=1)
    if fmt == "RGBA":
        return np.ascontiguousarray(rgba).reshape(-1)
    return np.ascontiguousarray(rgba.astype("<u2") * 257).view(np.uint8).reshape(-1)


class Member:
    """One instance: its context with its LUT, its source and the destination the timed intervals write."""

    def __init__(self, w, h, fmt, lut, host):
        self.ctx = mi355fx.Context(0)
        self.L = self.ctx.L
        self.ctx.colorlut_load(lut.is3d, lut.size, lut.table, lut.domain_scale, lut.domain_offset)
        self.w, self.h, self.fmt, self.stride = w, h, mi355fx.FMT[fmt], w * (4 if fmt == "RGBA" else 8)
        self.nbytes = host.nbytes
        self.src, self.dst = self.ctx.alloc(self.nbytes), self.ctx.alloc(self.nbytes)
        self.ctx.h2d(self.src, host)
        self.t = C.c_uint64(0)

    def lone(self, dst=None):
        rc = self.L.mi355_colorlut_frames_device(self.ctx.h, self.src, 0, self.stride, dst or self.dst, 0, self.stride, 1, self.w, self.h, self.fmt)
        assert rc == 0, rc

    def submit(self, g, dst=None):
        rc = self.L.mi355_group_submit_colorlut(g.h, self.ctx.h, self.src, self.stride, dst or self.dst, self.stride, self.w, self.h, self.fmt, C.byref(self.t))
        assert rc == 0, rc

    def wait(self, g):
        rc = self.L.mi355_group_wait_colorlut(g.h, self.t.value)
        assert rc == 0, rc

    def close(self):
        self.ctx.free(self.src)
        self.ctx.free(self.dst)
        self.ctx.close()


def identical_bytes(g, members):
    """Every source graded twice, lone into the member's destination and through the group into a second one: equal byte for byte?"""
    same = True
    seconds = [m.ctx.alloc(m.nbytes) for m in members]
    for m, b in zip(members, seconds):
        m.lone()
        m.submit(g, b)
    for m, b in zip(members, seconds):
        m.wait(g)
        m.ctx.synchronize()
        got_a, got_b = np.empty(m.nbytes, np.uint8), np.empty(m.nbytes, np.uint8)
        m.ctx.d2h(got_a, m.dst)
        m.ctx.d2h(got_b, b)
        same = same and bool((got_a == got_b).all())
        m.ctx.free(b)
    return same


def stats_row(times_s):
    us = np.array(times_s) * 1e6
    p5, p95 = np.percentile(us, 5), np.percentile(us, 95)
    med = float(np.median(us))
    return dict(us_per_interval_median=med, us_per_interval_p5=float(p5), us_per_interval_p95=float(p95), us_spread=float(p95 - p5) / 2,
                frames_per_s=MEMBERS * 1e6 / med)


def intervals(g, members):
    def lone_interval():
        for m in members:
            m.lone()
        for m in members:
            m.ctx.synchronize()

    def group_interval():
        for m in members:
            m.submit(g)
        for m in members:
            m.wait(g)

    return lone_interval, group_interval


def make_members(leg):
    label, w, h, fmt, one_lut = LEGS[leg]
    luts = [seeded_lut(0 if one_lut else k) for k in range(MEMBERS)]
    base = synth.smooth_frame(w, h).reshape(h, w, 4)
    return label, [Member(w, h, fmt, luts[k], picture(base, fmt, k)) for k in range(MEMBERS)]


def measure(leg, warmup, rounds, block):
    label, members = make_members(leg)
    g = mi355fx.Group(0)
    same = identical_bytes(g, members)
    lone_interval, group_interval = intervals(g, members)
    for _ in range(warmup):
        lone_interval()
    for _ in range(warmup):
        group_interval()
    lone_kernels = sorted({m.ctx.colorlut_kernel_name() for m in members})
    before = g.colorlut_stats()
    times = {"lone": [], "group": []}
    for _ in range(rounds):
        for name, fn in (("lone", lone_interval), ("group", group_interval)):
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
    frames, sets, _, launches = (a - b for a, b in zip(g.colorlut_stats(), before))
    rows = {name: stats_row(v) for name, v in times.items()}
    rows["lone"].update(kernels_after_warmup=lone_kernels, kernels_at_the_end=sorted({m.ctx.colorlut_kernel_name() for m in members}))
    rows["group"].update(frames_launched=frames, launch_sets=sets, largest_set=g.colorlut_stats()[2], kernel_launches=launches)
    g.close()
    for m in members:
        m.close()
    return label, rows, same


def child(calls=100):
    """`calls` warm-up pairs, then `calls` timed ones, a set of 32 and 32 lone launches ALTERNATING (the clocks and the caches are the
    same for both): the figures are those of the last launches of each kernel in the trace."""
    _, members = make_members("ii")
    g = mi355fx.Group(0)
    lone_interval, group_interval = intervals(g, members)
    for _ in range(2 * calls):
        group_interval()
        lone_interval()
    print("child: %d + %d alternating pairs of a set of %d frames and %d lone launches; group stats %s; lone kernels %s"
          % (calls, calls, MEMBERS, MEMBERS, g.colorlut_stats(), sorted({m.ctx.colorlut_kernel_name() for m in members})))
    g.close()
    for m in members:
        m.close()


def kernel_stats(trace_dir, calls=100):
    """Per interval of the timed pairs: the one colorlut_jobs_kernel launch against the SUM of the 32 lone launches, from the rocpd
    database rocprofv3 left under trace_dir."""
    import glob
    import sqlite3
    db = sorted(glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True))[0]
    rows = sqlite3.connect(db).execute("select name, duration from kernels where name like '%colorlut%' order by start").fetchall()
    jobs = np.array([d for n, d in rows if "colorlut_jobs_kernel" in n][-calls:]) / 1e3
    lone = [(n, d) for n, d in rows if "jobs_kernel" not in n][-calls * MEMBERS:]
    names = sorted({n.split("(")[0] for n, _ in lone})
    sums = np.array([d for _, d in lone]).reshape(-1, MEMBERS).sum(axis=1) / 1e3

    def row(name, us):
        p5, p95 = np.percentile(us, 5), np.percentile(us, 95)
        return dict(kernel=name, intervals=len(us), us_median=float(np.median(us)), us_p5=float(p5), us_p95=float(p95), us_spread=float(p95 - p5) / 2)

    a, b = row("colorlut_jobs_kernel (one launch, 32 jobs)", jobs), row("sum of 32 lone launches: " + ", ".join(names), sums)
    return [a, b, dict(yardstick="device time of one colorlut_jobs_kernel launch over 32 x 1080p RGBA against the 32 lone launches of the same frames",
                       jobs_over_lone=a["us_median"] / b["us_median"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", default="i,ii,iii,iv,v")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorlut_group.txt"))
    ap.add_argument("--child", action="store_true", help="only sets of 32 frames and lone launches of the same frames (for a profiler run)")
    ap.add_argument("--kernel-stats", metavar="DIR", help="print the yardstick from the trace of a --child run under DIR (no device needed)")
    a = ap.parse_args()
    if a.child:
        child()
        return
    if a.kernel_stats:
        sys.stdout.write("".join(json.dumps(r) + "\n" for r in kernel_stats(a.kernel_stats)))
        return
    rows = []
    for leg in a.legs.split(","):
        label, r, same = measure(leg, a.warmup, a.rounds, a.block)
        for name in ("lone", "group"):
            rows.append(dict(leg=leg, frames=label, path=name, intervals=a.rounds * a.block, **r[name]))
        lone, grp = r["lone"], r["group"]
        rows.append(dict(leg=leg, frames=label, identical_bytes_in_both_modes=same,
                         lone_over_group_time=lone["us_per_interval_median"] / grp["us_per_interval_median"],
                         us_saved_per_interval=lone["us_per_interval_median"] - grp["us_per_interval_median"], us_spreads_together=lone["us_spread"] + grp["us_spread"],
                         separated=bool(abs(lone["us_per_interval_median"] - grp["us_per_interval_median"]) > lone["us_spread"] + grp["us_spread"])))
        sys.stdout.write("".join(json.dumps(x) + "\n" for x in rows[-3:]))
        sys.stdout.flush()
    rows.append(dict(note="an interval is one frame per member, one thread: lone = 32 asynchronous calls on 32 contexts and their 32 synchronisations; group = 32 submits "
                          "and 32 waits, one set of one launch. Rounds alternate the two ways; spread = (p95 - p5) / 2 over all intervals of a way. One machine, one run."))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

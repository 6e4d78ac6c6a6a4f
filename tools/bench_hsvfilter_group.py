"""hsvfilter frames in the filter queue of the video group against lone contexts: 32 independent `hsvfilter` instances,
each with its own context, its own device frame and its own settings snapshot, filtering one frame per interval in place. One
thread, no thread noise. Four legs:

  (i)   32 x 1920x1080 BGRx, 32 different settings (a hue shift per camera: what mi355_group_submit_chain cannot batch)
  (ii)  the same frames, one setting
  (iii) 32 x 640x640 RGB (the yoloxinference feed)
  (iv)  32 x 3840x2160 RGBA

  lone  : 32 mi355_hsvfilter_frames_device calls with n_frames = 1 on the 32 contexts, then a synchronisation of each.
  group : 32 mi355_group_submit_hsvfilter then 32 mi355_group_wait_hsvfilter - one set, one launch of hsvfilter_jobs_kernel.

Both ways run in the same process, INTERLEAVED: after --warmup intervals of both, --rounds rounds, each --block lone intervals then
--block group intervals (default 20 x 50 = 1000 timed intervals per way), a host clock around every interval. Per way: the median,
the 5th and 95th percentile and the spread (half of p95 - p5). Before the timing each leg filters two copies of the same frames
once, lone and through the group, and compares them byte for byte. No ratio is fixed in advance; a leg that is slower through the
group is reported as it is.

  python tools/bench_hsvfilter_group.py [--rounds R] [--block B] [--warmup W] [--legs i,ii,iii,iv] [--out profiles/hsvfilter_group.txt] [--child]

--child is what a profiler watches (`rocprofv3 --kernel-trace --stats -- python tools/bench_hsvfilter_group.py --child`): leg (ii)'s
32 frames laid out contiguously, filtered alternately by a set of 32 through the queue (hsvfilter_jobs_kernel) and by ONE lone
mi355_hsvfilter_frames_device call over all 32 (hsvfilter_flat_kernel), the same bytes; 300 warm-up pairs, then 300 timed ones.
`--kernel-stats DIR` prints the two kernels' durations over the timed pairs from the trace's database under DIR.
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

MEMBERS = 32
ONE = (90.0, 1.0, 0.0, 1.0, 0.0)
PER_CAMERA = [(-170.0 + 11.0 * k, 1.0 + 0.01 * (k % 5), 0.0, 1.0, 0.005 * (k % 3)) for k in range(MEMBERS)]   # zero, positive and negative shifts, identity s / v or not
LEGS = {
    "i": ("32 x 1920x1080 BGRx, 32 settings", 1920, 1080, "BGRx", PER_CAMERA),
    "ii": ("32 x 1920x1080 BGRx, one setting", 1920, 1080, "BGRx", [ONE] * MEMBERS),
    "iii": ("32 x 640x640 RGB, one setting", 640, 640, "RGB", [ONE] * MEMBERS),
    "iv": ("32 x 3840x2160 RGBA, one setting", 3840, 2160, "RGBA", [ONE] * MEMBERS),
}


def picture(w, h, fmt, seed):
    ps = mi355fx.FMT_LAYOUT[fmt][0]
    rgba = np.roll(synth.smooth_frame(w, h).reshape(h, w, 4), 97 * seed, axis=1)
    return np.ascontiguousarray(rgba[:, :, :ps]).reshape(-1)


class Member:
    """One instance: its context, its frame (`d`, timed) and the two copies the byte comparison filters once."""

    def __init__(self, w, h, fmt, st, host, d=None):
        self.ctx = mi355fx.Context(0)
        self.L = self.ctx.L
        self.w, self.h, self.fmt, self.stride = w, h, mi355fx.FMT[fmt], w * mi355fx.FMT_LAYOUT[fmt][0]
        self.s = mi355fx.HsvSettings(*[float(v) for v in st])
        self.nbytes = host.nbytes
        self.own = d is None
        self.d = self.ctx.alloc(self.nbytes) if self.own else d
        self.ctx.h2d(self.d, host)
        self.t = C.c_uint64(0)

    def lone(self, d=None):
        rc = self.L.mi355_hsvfilter_frames_device(self.ctx.h, d or self.d, 1, 0, self.w, self.h, self.stride, self.fmt, C.byref(self.s))
        assert rc == 0, rc

    def submit(self, g, d=None):
        rc = self.L.mi355_group_submit_hsvfilter(g.h, self.ctx.h, d or self.d, self.w, self.h, self.stride, self.fmt, C.byref(self.s), C.byref(self.t))
        assert rc == 0, rc

    def wait(self, g):
        rc = self.L.mi355_group_wait_hsvfilter(g.h, self.t.value)
        assert rc == 0, rc

    def close(self):
        if self.own:
            self.ctx.free(self.d)
        self.ctx.close()


def identical_bytes(g, members, hosts):
    """Two fresh copies of every frame, one filtered lone, one through the group: equal byte for byte?"""
    same = True
    copies = []
    for m, host in zip(members, hosts):
        a, b = m.ctx.alloc(m.nbytes), m.ctx.alloc(m.nbytes)
        m.ctx.h2d(a, host)
        m.ctx.h2d(b, host)
        copies.append((a, b))
    for m, (a, b) in zip(members, copies):
        m.lone(a)
        m.submit(g, b)
    for m, (a, b) in zip(members, copies):
        m.wait(g)
        m.ctx.synchronize()
        got_a, got_b = np.empty(m.nbytes, np.uint8), np.empty(m.nbytes, np.uint8)
        m.ctx.d2h(got_a, a)
        m.ctx.d2h(got_b, b)
        same = same and bool((got_a == got_b).all())
        m.ctx.free(a)
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


def measure(leg, warmup, rounds, block):
    label, w, h, fmt, settings = LEGS[leg]
    hosts = [picture(w, h, fmt, k) for k in range(MEMBERS)]
    members = [Member(w, h, fmt, settings[k], hosts[k]) for k in range(MEMBERS)]
    g = mi355fx.Group(0)
    same = identical_bytes(g, members, hosts)
    lone_interval, group_interval = intervals(g, members)
    for _ in range(warmup):
        lone_interval()
    for _ in range(warmup):
        group_interval()
    before = g.hsvfilter_stats()
    times = {"lone": [], "group": []}
    for _ in range(rounds):
        for name, fn in (("lone", lone_interval), ("group", group_interval)):
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
    frames, sets, _, launches = (a - b for a, b in zip(g.hsvfilter_stats(), before))
    rows = {name: stats_row(v) for name, v in times.items()}
    rows["group"].update(frames_launched=frames, launch_sets=sets, largest_set=g.hsvfilter_stats()[2], kernel_launches=launches)
    g.close()
    for m in members:
        m.close()
    return label, rows, same


def child(calls=300):
    """The two kernels on the SAME device bytes: member k's frame is frame k of the lone call's batch. `calls` warm-up pairs, then
    `calls` timed ones, a set and a lone launch ALTERNATING (the clocks and the caches are the same for both): the figures are
    those of the last `calls` launches of each kernel in the trace."""
    _, w, h, fmt, settings = LEGS["ii"]
    with mi355fx.Context(0) as ctx:
        host = np.concatenate([picture(w, h, fmt, k) for k in range(MEMBERS)])
        pitch = host.nbytes // MEMBERS
        d = ctx.alloc(host.nbytes)
        members = [Member(w, h, fmt, settings[k], host[k * pitch: (k + 1) * pitch], d + k * pitch) for k in range(MEMBERS)]
        g = mi355fx.Group(0)
        _, group_interval = intervals(g, members)
        for _ in range(2 * calls):
            group_interval()
            ctx.hsvfilter_frames_device(d, MEMBERS, pitch, w, h, w * 4, fmt, settings[0])
            ctx.synchronize()
        print("child: %d + %d alternating pairs of a set of %d frames and a lone launch over the same %d frames; group stats %s"
              % (calls, calls, MEMBERS, MEMBERS, g.hsvfilter_stats()))
        g.close()
        for m in members:
            m.close()
        ctx.free(d)


def kernel_stats(trace_dir, calls=300):
    """The durations of the two kernels over the timed pairs, from the rocpd database rocprofv3 left under trace_dir."""
    import glob
    import sqlite3
    db = sorted(glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True))[0]
    rows = sqlite3.connect(db).execute("select name, duration from kernels where name like '%hsvfilter%' order by start").fetchall()
    out = {}
    for name in ("hsvfilter_jobs_kernel", "hsvfilter_flat_kernel"):
        us = np.array([d for n, d in rows if name in n][-calls:]) / 1e3
        p5, p95 = np.percentile(us, 5), np.percentile(us, 95)
        out[name] = dict(kernel=name, launches=len(us), us_median=float(np.median(us)), us_p5=float(p5), us_p95=float(p95), us_spread=float(p95 - p5) / 2)
    jobs, lone = out["hsvfilter_jobs_kernel"], out["hsvfilter_flat_kernel"]
    return [jobs, lone, dict(yardstick="hsvfilter_jobs_kernel over 32 x 1080p BGRx against ONE lone launch over the same 32 contiguous frames",
                             jobs_over_lone=jobs["us_median"] / lone["us_median"], lone_spread_share=lone["us_spread"] / lone["us_median"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", default="i,ii,iii,iv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hsvfilter_group.txt"))
    ap.add_argument("--child", action="store_true", help="only sets of 32 frames and lone launches of 32 frames (for a profiler run)")
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
    rows.append(dict(note="an interval is one frame per member, one thread: lone = 32 asynchronous calls on 32 contexts and their 32 synchronisations; group = 32 submits "
                          "and 32 waits, one set of one launch. Rounds alternate the two ways; spread = (p95 - p5) / 2 over all intervals of a way. One machine, one run."))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

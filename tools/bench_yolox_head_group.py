"""yoloxinference's head maps in the decoder queue of the video group against lone contexts: 32 independent
`yoloxinference ! yoloxtensordec` instances, each with its own context and its own device maps of tools/bench_yolox_head.py's shape -
levels 80 x 80, 40 x 40, 20 x 20, 80 classes, 8400 candidates, about 1 % above both thresholds - decoding one tensor per interval. Two
mixes: 32 heads; 16 heads + 16 decoded X tensors (the tensors the head maps decode to). One thread, no thread noise.

  lone  : 32 mi355_yolox_head_dets_device (or, for a tensor member, mi355_yolodec_tensors_device) calls with n_tensors = 1 on the 32
          contexts - each a settings upload, two launches, one download and one synchronisation.
  group : 32 mi355_group_submit_yolox_head / _submit_yolodec then 32 mi355_group_wait_yolodec - per set one upload of the level
          tables, two launches for the heads (and two for the X tensors) and one download.

Both ways run in the same process on the same maps, INTERLEAVED: after the warm-up of both, --rounds rounds, each --block lone
intervals then --block group intervals, a host clock around every interval (both intervals end in a device synchronisation: the lone
call's own, the wait's event). Per way: the median over all intervals, the 5th and 95th percentile, the spread (half of p95 - p5),
and the medians of the rounds. The group's results are compared with the lone calls' byte for byte. No ratio is fixed in advance;
`separated` says whether the group's median lies below the lone median by more than the two spreads together.

  python tools/bench_yolox_head_group.py [--rounds R] [--block B] [--warmup W] [--out profiles/yolox_head_group_bench.txt] [--child]

--child is what a profiler watches (`rocprofv3 --kernel-trace --stats -- python tools/bench_yolox_head_group.py --child`): sets of 32
heads through the queue (yolox_head_score_jobs_kernel) and lone calls of 32 tensors (yolox_head_score_kernel), the same maps.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mi355fx  # noqa: E402
import bench_yolox_head as B  # noqa: E402  (the maps and settings of the lone benchmark)

MEMBERS = 32
MIXES = (("32 x head", ["head"] * 32), ("16 x head + 16 x X tensor", ["head", "tensor"] * 16))
X = mi355fx.YOLO_LAYOUT["X"]


class Member:
    """One instance: its context, its head maps in the engine's fused [5 + C, h, w] form per level and, for a tensor member, the
    tensor they decode to."""

    def __init__(self, kind, seed, levels=None):
        """levels: maps that are on the device already (the profiler run: the lone batch's own), else a device copy of its own"""
        self.ctx = mi355fx.Context(0)
        self.L = self.ctx.L
        self.is_head = kind == "head"
        self.maps = []
        for (reg, obj, cls, s) in ([] if levels else B.head(100 + seed % 8)):     # eight distinct heads; every member has its own device copy
            h, w = reg.shape[1:]
            d = self.ctx.alloc(B.F * h * w * 4)
            self.ctx.h2d(d, np.concatenate([a.reshape(-1) for a in (reg, obj, cls)]))
            self.maps.append(d)
            levels = (levels or []) + [(d, d + 16 * h * w, d + 20 * h * w, B.F * h * w * 4, B.F * h * w * 4, B.F * h * w * 4, h, w, s)]
        self.lv, self.n_lv = mi355fx._yolox_levels(levels), len(levels)
        self.pitch = B.A * B.F * 4
        self.d_tensor = None
        if not self.is_head:
            self.d_tensor = self.ctx.alloc(self.pitch)
            self.ctx._ck(self.L.mi355_yolox_head_decode_device(self.ctx.h, self.lv, self.n_lv, 1, B.CLASSES, self.d_tensor, self.pitch))
            self.ctx.synchronize()
        self.p = mi355fx.YoloParams(*B.PARAMS)
        self.dets = np.zeros(B.MAX_DETS, mi355fx.YOLO_DET)
        self.n, self.t = C.c_uint32(0), C.c_uint64(0)
        self.ref = None

    def lone(self):
        if self.is_head:
            rc = self.L.mi355_yolox_head_dets_device(self.ctx.h, self.lv, self.n_lv, 1, B.CLASSES, C.byref(self.p), self.dets.ctypes.data, B.MAX_DETS, C.byref(self.n))
        else:
            rc = self.L.mi355_yolodec_tensors_device(self.ctx.h, self.d_tensor, self.pitch, 1, X, B.F, B.A, C.byref(self.p), self.dets.ctypes.data, B.MAX_DETS,
                                                     C.byref(self.n))
        assert rc == 0, rc

    def submit(self, g):
        if self.is_head:
            rc = self.L.mi355_group_submit_yolox_head(g.h, self.ctx.h, self.lv, self.n_lv, B.CLASSES, C.byref(self.p), B.MAX_DETS, C.byref(self.t))
        else:
            rc = self.L.mi355_group_submit_yolodec(g.h, self.ctx.h, self.d_tensor, X, B.F, B.A, C.byref(self.p), B.MAX_DETS, C.byref(self.t))
        assert rc == 0, rc

    def wait(self, g):
        rc = self.L.mi355_group_wait_yolodec(g.h, self.t.value, self.dets.ctypes.data, C.byref(self.n))
        assert rc == 0, rc

    def result(self):
        n = self.n.value
        return n, self.dets[:min(n, B.MAX_DETS)].tobytes()

    def close(self):
        for d in self.maps + ([self.d_tensor] if self.d_tensor is not None else []):
            self.ctx.free(d)
        self.ctx.close()


def stats_row(times_s, block):
    us = np.array(times_s) * 1e6
    p5, p95 = np.percentile(us, 5), np.percentile(us, 95)
    rounds = [float(np.median(us[k:k + block])) for k in range(0, len(us), block)]
    return dict(us_per_interval_median=float(np.median(us)), us_per_interval_mean=float(us.mean()), us_per_interval_p5=float(p5), us_per_interval_p95=float(p95),
                us_spread=float(p95 - p5) / 2, us_round_medians_min=min(rounds), us_round_medians_max=max(rounds), us_per_member_median=float(np.median(us)) / MEMBERS)


def intervals(g, members):
    def lone_interval():
        for m in members:
            m.lone()

    def group_interval():
        for m in members:
            m.submit(g)
        for m in members:
            m.wait(g)

    return lone_interval, group_interval


def measure(members, warmup, rounds, block):
    g = mi355fx.Group(0)
    lone_interval, group_interval = intervals(g, members)
    for _ in range(warmup):
        lone_interval()
    for m in members:
        m.ref = m.result()
    for _ in range(warmup):
        group_interval()
    assert all(m.result() == m.ref for m in members), "group != lone"
    before, heads_before = g.yolodec_stats(), g.yolox_head_stats()
    times = {"lone": [], "group": []}
    for _ in range(rounds):
        for name, fn in (("lone", lone_interval), ("group", group_interval)):
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        assert all(m.result() == m.ref for m in members), "group != lone"
    t, s, _, k = (a - b for a, b in zip(g.yolodec_stats(), before))
    hd, hs, up, hk = (a - b for a, b in zip(g.yolox_head_stats(), heads_before))
    rows = {name: stats_row(v, block) for name, v in times.items()}
    rows["group"].update(members_launched=t, launch_sets=s, kernel_launches=k, launches_per_set=k / max(s, 1), heads=hd, sets_with_a_head=hs, table_uploads=up,
                         head_kernel_launches=hk)
    g.close()
    return rows, float(np.mean([m.ref[0] for m in members]))


def child(calls=23):
    """The two score kernels on the SAME device maps: member k's levels are tensor k of the lone batch."""
    with mi355fx.Context(0) as ctx:
        b = B.Batch(ctx, MEMBERS)
        members = [Member("head", k, [(r + k * pr, o + k * po, c + k * pc, pr, po, pc, h, w, s) for r, o, c, pr, po, pc, h, w, s in b.levels]) for k in range(MEMBERS)]
        g = mi355fx.Group(0)
        _, group_interval = intervals(g, members)
        for _ in range(calls):
            group_interval()
        for _ in range(calls):
            b.fused()
        ref = b.result()
        group_interval()
        assert [m.n.value for m in members] == ref[0] and b"".join(m.result()[1] for m in members) == ref[1], "group != lone"
        g.close()
        for m in members:
            m.close()
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_head_group_bench.txt"))
    ap.add_argument("--child", action="store_true", help="only sets of 32 heads and lone calls of 32 tensors (for a profiler run)")
    a = ap.parse_args()
    if a.child:
        child()
        return
    rows = []
    for label, kinds in MIXES:
        members = [Member(kind, k) for k, kind in enumerate(kinds)]
        r, mean_dets = measure(members, a.warmup, a.rounds, a.block)
        for name in ("lone", "group"):
            rows.append(dict(members=label, path=name, intervals=a.rounds * a.block, rounds=a.rounds, **r[name]))
        lone, grp = r["lone"], r["group"]
        rows.append(dict(members=label, levels=B.SHAPES, classes=B.CLASSES, candidates=B.A, max_dets=B.MAX_DETS, detections_mean=mean_dets,
                         lone_over_group_speed=lone["us_per_interval_median"] / grp["us_per_interval_median"],
                         us_saved_per_interval=lone["us_per_interval_median"] - grp["us_per_interval_median"], us_spreads_together=lone["us_spread"] + grp["us_spread"],
                         separated=bool(lone["us_per_interval_median"] - grp["us_per_interval_median"] > lone["us_spread"] + grp["us_spread"])))
        for m in members:
            m.close()
    rows.append(dict(note="an interval is one tensor per member, one thread: lone = 32 calls of a settings upload, two launches, one download and one synchronisation "
                          "each; group = 32 submits and 32 waits, one set of one table upload, two launches per kind of member present and one download. Rounds "
                          "alternate the two ways; spread = (p95 - p5) / 2 over all intervals of a way. One machine, one run."))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""The decoder queue of the video group against lone contexts: 32 independent yolov8tensordec2 / yoloxtensordec
instances, each with its own context and its own device tensor of the real shape - V8 84 x 8400 or X 8400 x 85, about 1 % of the
candidates above threshold (tests/yolodec_cases.realistic) - decoding one tensor per interval. Three member sets: 32 x V8, 32 x X,
16 + 16. Both ways run in the same process, on the same tensors, one after the other, and their results are compared.

  (a) one thread   : 32 lone mi355_yolodec_tensors_device calls (n_tensors = 1) on the 32 contexts, against 32
                     mi355_group_submit_yolodec then 32 mi355_group_wait_yolodec. No thread noise.
  (b) 32 threads   : each thread owns a context and decodes its tensor once per interval (a barrier starts the interval), lone
                     against submit + wait at once with a rendezvous of 32.

Per way: microseconds per interval (mean, median, best) and per tensor, and for the group the launch sets, kernel launches and
tensors per set over the measured intervals. No figure is fixed in advance; what comes out is written down.

  python tools/bench_yolodec_group.py [--intervals K] [--warmup W] [--out profiles/yolodec_group.txt] [--no-threads]
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mi355fx  # noqa: E402
import yolodec_cases as Y  # noqa: E402

MEMBERS = 32
MAX_DETS = 128
LINGER_US = 2000
SETS = (("32 x V8", ["V8"] * 32), ("32 x X", ["X"] * 32), ("16 x V8 + 16 x X", ["V8", "X"] * 16))


class Member:
    def __init__(self, layout, seed):
        self.ctx = mi355fx.Context(0)
        case = Y.realistic(layout, seed=seed % 8)          # eight distinct tensors per layout; every member has its own device copy
        self.layout, self.F, self.N = mi355fx.YOLO_LAYOUT[layout], case.F, case.N
        self.d = self.ctx.alloc(case.data.nbytes)
        self.ctx.h2d(self.d, case.data)
        self.p = mi355fx.YoloParams(*case.params)
        self.dets = np.zeros(MAX_DETS, mi355fx.YOLO_DET)
        self.ref = np.zeros(MAX_DETS, mi355fx.YOLO_DET)
        self.n, self.t = C.c_uint32(0), C.c_uint64(0)
        self.L = self.ctx.L

    def lone(self):
        rc = self.L.mi355_yolodec_tensors_device(self.ctx.h, self.d, self.F * self.N * 4, 1, self.layout, self.F, self.N, C.byref(self.p), self.dets.ctypes.data,
                                                 MAX_DETS, C.byref(self.n))
        assert rc == 0, rc

    def submit(self, g):
        rc = self.L.mi355_group_submit_yolodec(g.h, self.ctx.h, self.d, self.layout, self.F, self.N, C.byref(self.p), MAX_DETS, C.byref(self.t))
        assert rc == 0, rc

    def wait(self, g):
        rc = self.L.mi355_group_wait_yolodec(g.h, self.t.value, self.dets.ctypes.data, C.byref(self.n))
        assert rc == 0, rc

    def close(self):
        self.ctx.free(self.d)
        self.ctx.close()


def stats_row(times_s):
    us = np.array(times_s) * 1e6
    return dict(us_per_interval_mean=float(us.mean()), us_per_interval_median=float(np.median(us)), us_per_interval_best=float(us.min()),
                us_per_tensor_mean=float(us.mean()) / MEMBERS)


def queue_row(g, before):
    t, s, largest, k = (a - b for a, b in zip(g.yolodec_stats(), before))
    return dict(tensors=t, launch_sets=s, kernel_launches=k, tensors_per_set=t / max(s, 1), launches_per_set=k / max(s, 1))


def one_thread(members, warmup, intervals):
    def lone_interval():
        for m in members:
            m.lone()

    g = mi355fx.Group(0)

    def group_interval():
        for m in members:
            m.submit(g)
        for m in members:
            m.wait(g)

    rows = {}
    for name, fn in (("lone", lone_interval), ("group", group_interval)):
        for _ in range(warmup):
            fn()
        before = g.yolodec_stats()
        times = []
        for _ in range(intervals):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        rows[name] = stats_row(times)
        if name == "lone":
            for m in members:
                m.ref[:] = m.dets
                m.ref_n = m.n.value
        else:
            rows[name].update(queue_row(g, before))
            assert all(m.n.value == m.ref_n and m.dets[:min(m.ref_n, MAX_DETS)].tobytes() == m.ref[:min(m.ref_n, MAX_DETS)].tobytes() for m in members), "group != lone"
    g.close()
    return rows


def threads(members, warmup, intervals):
    rows = {}
    for name in ("lone", "group"):
        g = mi355fx.Group(0)
        g.set_yolodec_rendezvous(MEMBERS, LINGER_US)
        bar = threading.Barrier(MEMBERS + 1)
        errors = []

        def element(m):
            try:
                for _ in range(warmup + intervals):
                    bar.wait()
                    if name == "lone":
                        m.lone()
                    else:
                        m.submit(g)
                        m.wait(g)
                    bar.wait()
            except Exception as e:      # noqa: BLE001 - told to the main thread
                errors.append(e)
                bar.abort()

        ts = [threading.Thread(target=element, args=(m,)) for m in members]
        for t in ts:
            t.start()
        times, before = [], None
        try:
            for k in range(warmup + intervals):
                if k == warmup:
                    before = g.yolodec_stats()
                t0 = time.perf_counter()
                bar.wait()
                bar.wait()
                if k >= warmup:
                    times.append(time.perf_counter() - t0)
        except threading.BrokenBarrierError:
            pass
        for t in ts:
            t.join()
        assert not errors, errors
        rows[name] = stats_row(times)
        if name == "group":
            rows[name].update(queue_row(g, before))
        assert all(m.n.value == m.ref_n for m in members), "%s != lone, one thread" % name
        g.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--intervals", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolodec_group.txt"))
    ap.add_argument("--no-threads", action="store_true")
    a = ap.parse_args()
    rows = []
    for label, layouts in SETS:
        members = [Member(l, k) for k, l in enumerate(layouts)]
        ways = [("one thread", one_thread)] + ([] if a.no_threads else [("32 threads", threads)])
        for way, fn in ways:
            r = fn(members, a.warmup, a.intervals)
            for name in ("lone", "group"):
                rows.append(dict(members=label, way=way, path=name, intervals=a.intervals, max_dets=MAX_DETS, **r[name]))
            rows.append(dict(members=label, way=way, group_over_lone_time=r["group"]["us_per_interval_mean"] / r["lone"]["us_per_interval_mean"],
                             lone_over_group_speed=r["lone"]["us_per_interval_mean"] / r["group"]["us_per_interval_mean"]))
        for m in members:
            m.close()
    rows.append(dict(note="an interval is one tensor per member: lone = 32 calls of two launches, one synchronisation and one download each; group = at most three "
                          "launches and one download per set. (b) includes two barrier crossings of 33 Python threads per interval in both paths; rendezvous 32, "
                          "linger %d us" % LINGER_US))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

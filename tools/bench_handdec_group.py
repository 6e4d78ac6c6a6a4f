"""The hand-decoder queue of the video group against lone contexts: 32 independent handdetectiontensordec /
handlandmarktensordec instances, each with its own context and its own device tensor of tools/bench_handdec.py's shapes - palm
[2016, 8] at 42 % valid rows and a threshold of 0.7, landmarks [2, 63] with scores - decoding one tensor per interval. Three mixes:
32 palm, 32 landmarks, 16 + 16. One thread, no thread noise.

  lone  : 32 mi355_handdec_palm_tensors_device / mi355_handdec_landmarks_tensors_device calls (n_tensors = 1) on the 32 contexts -
          each a params upload, one launch, one download and one synchronisation.
  group : 32 mi355_group_submit_handdec_* then 32 mi355_group_wait_handdec - per set one or two launches and one download.

Both ways run in the same process on the same tensors, INTERLEAVED: after the warm-up of both, --rounds rounds, each --block lone
intervals then --block group intervals, a host clock around every interval (both intervals end in a device synchronisation: the
lone call's own, the wait's event). Per way: the median over all intervals, the 5th and 95th percentile, the spread (half of p95 -
p5), and the medians of the rounds (how far the same code moves between rounds of one run). The group's results are compared with
the lone calls' byte for byte. No ratio is fixed in advance; `separated` says whether the group's median lies below the lone median
by more than the two spreads together.

  python tools/bench_handdec_group.py [--rounds R] [--block B] [--warmup W] [--out profiles/handdec_group.txt]
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
import bench_handdec as B  # noqa: E402  (the tensors and settings of the lone benchmark)

MEMBERS = 32
PALM_ROWS, HANDS = 2016, 2
MIXES = (("32 x palm", ["palm"] * 32), ("32 x landmarks", ["landmarks"] * 32), ("16 x palm + 16 x landmarks", ["palm", "landmarks"] * 16))


class Member:
    def __init__(self, kind, seed):
        self.ctx = mi355fx.Context(0)
        self.L = self.ctx.L
        self.palm = kind == "palm"
        if self.palm:                                       # eight distinct tensors per kind; every member has its own device copy
            data, scores = B.palm_tensor(PALM_ROWS, 100 + seed % 8), None
            self.p = mi355fx.HandParams(*B.PALM_PARAMS)
        else:
            data, scores = B.landmark_tensor(HANDS, 100 + seed % 8)
            self.p = mi355fx.HandParams(*B.LANDMARK_PARAMS)
        self.rows, self.bytes = data.shape[0], data.nbytes
        self.d = self.ctx.alloc(data.nbytes)
        self.ctx.h2d(self.d, data)
        self.ds, self.ns = None, 0
        if scores is not None:
            self.ds, self.ns = self.ctx.alloc(scores.nbytes), scores.size
            self.ctx.h2d(self.ds, scores)
        self.dets, self.kps = np.zeros(mi355fx.HAND_MAX, mi355fx.HAND_DET), np.zeros(mi355fx.HAND_MAX, mi355fx.HAND_KP)
        self.n, self.t = C.c_uint32(0), C.c_uint64(0)
        self.ref = None

    def lone(self):
        if self.palm:
            rc = self.L.mi355_handdec_palm_tensors_device(self.ctx.h, self.d, self.bytes, 1, self.rows, C.byref(self.p), self.dets.ctypes.data, C.byref(self.n))
        else:
            rc = self.L.mi355_handdec_landmarks_tensors_device(self.ctx.h, self.d, self.bytes, 1, self.rows, B.D, self.ds, self.ns * 4, self.ns, C.byref(self.p),
                                                               self.dets.ctypes.data, self.kps.ctypes.data, C.byref(self.n))
        assert rc == 0, rc

    def submit(self, g):
        if self.palm:
            rc = self.L.mi355_group_submit_handdec_palm(g.h, self.ctx.h, self.d, self.rows, C.byref(self.p), C.byref(self.t))
        else:
            rc = self.L.mi355_group_submit_handdec_landmarks(g.h, self.ctx.h, self.d, self.rows, B.D, self.ds, self.ns, C.byref(self.p), C.byref(self.t))
        assert rc == 0, rc

    def wait(self, g):
        rc = self.L.mi355_group_wait_handdec(g.h, self.t.value, self.dets.ctypes.data, self.kps.ctypes.data, C.byref(self.n))
        assert rc == 0, rc

    def result(self):
        n = self.n.value
        return n, self.dets[:n].tobytes(), b"" if self.palm else self.kps[:n].tobytes()

    def close(self):
        self.ctx.free(self.d)
        if self.ds is not None:
            self.ctx.free(self.ds)
        self.ctx.close()


def stats_row(times_s, block):
    us = np.array(times_s) * 1e6
    p5, p95 = np.percentile(us, 5), np.percentile(us, 95)
    rounds = [float(np.median(us[k:k + block])) for k in range(0, len(us), block)]
    return dict(us_per_interval_median=float(np.median(us)), us_per_interval_mean=float(us.mean()), us_per_interval_p5=float(p5), us_per_interval_p95=float(p95),
                us_spread=float(p95 - p5) / 2, us_round_medians_min=min(rounds), us_round_medians_max=max(rounds), us_per_tensor_median=float(np.median(us)) / MEMBERS)


def measure(members, warmup, rounds, block):
    g = mi355fx.Group(0)

    def lone_interval():
        for m in members:
            m.lone()

    def group_interval():
        for m in members:
            m.submit(g)
        for m in members:
            m.wait(g)

    for _ in range(warmup):
        lone_interval()
    for m in members:
        m.ref = m.result()
    for _ in range(warmup):
        group_interval()
    assert all(m.result() == m.ref for m in members), "group != lone"
    before = g.handdec_stats()
    times = {"lone": [], "group": []}
    for _ in range(rounds):
        for name, fn in (("lone", lone_interval), ("group", group_interval)):
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        assert all(m.result() == m.ref for m in members), "group != lone"
    t, s, _, k = (a - b for a, b in zip(g.handdec_stats(), before))
    rows = {name: stats_row(v, block) for name, v in times.items()}
    rows["group"].update(tensors=t, launch_sets=s, kernel_launches=k, tensors_per_set=t / max(s, 1), launches_per_set=k / max(s, 1))
    g.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handdec_group.txt"))
    a = ap.parse_args()
    rows = []
    for label, kinds in MIXES:
        members = [Member(kind, k) for k, kind in enumerate(kinds)]
        r = measure(members, a.warmup, a.rounds, a.block)
        for name in ("lone", "group"):
            rows.append(dict(members=label, path=name, intervals=a.rounds * a.block, rounds=a.rounds, **r[name]))
        lone, grp = r["lone"], r["group"]
        rows.append(dict(members=label, lone_over_group_speed=lone["us_per_interval_median"] / grp["us_per_interval_median"],
                         us_saved_per_interval=lone["us_per_interval_median"] - grp["us_per_interval_median"], us_spreads_together=lone["us_spread"] + grp["us_spread"],
                         separated=bool(lone["us_per_interval_median"] - grp["us_per_interval_median"] > lone["us_spread"] + grp["us_spread"])))
        for m in members:
            m.close()
    rows.append(dict(note="an interval is one tensor per member, one thread: lone = 32 calls of a params upload, one launch, one download and one synchronisation each; "
                          "group = 32 submits and 32 waits, one set of one or two launches and one download. Rounds alternate the two ways; spread = (p95 - p5) / 2 "
                          "over all intervals of a way. One machine, one run."))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

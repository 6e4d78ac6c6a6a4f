"""yoloxinference frames in the decoder queue of the video group against lone calls: 32 independent
`yoloxinference ! yoloxtensordec` instances that share ONE finalized net - YOLOX-nano, -tiny or -s, 80 classes, seeded random
parameters (tools/bench_yolox_net.py's) - each handing over one 640 x 640 RGB frame per interval. Every member has a context of its
own; the 32 frames lie in one device allocation, so the three legs read the same bytes. One thread, no thread noise.

  (i)   lone  : 32 mi355_yolox_infer_dets_device calls of ONE frame each on the net's context - each a conversion, a forward of one
                frame (88 - 118 launches), the head's two launches, a settings upload, a download and a synchronisation.
  (ii)  group : 32 mi355_group_submit_yolox_infer then 32 mi355_group_wait_yolodec - one set: one upload, the conversion launch, ONE
                forward of 32 frames in the queue's lane, the head score and NMS job launches, one download.
  (iii) batch : ONE mi355_yolox_infer_dets_device call over the same 32 frames - the yardstick: what the set would cost if nothing of
                the queue (job tables and their lookup, the upload, 64 entries under the group's lock) cost anything.

The legs run in the same process INTERLEAVED: after the warm-up of all three, --rounds rounds, each --block intervals of every leg in
turn, a host clock around every interval (every interval ends in a device synchronisation: the lone call's own, the wait's event).
Per leg: the median over all intervals, the 5th and 95th percentile and the spread (half of p95 - p5). For leg (ii) the interval is
split on the host: the time until the 32nd submit has returned (it launches the set: the host side of the upload and of every
launch, under the group's lock) and the time in the 32 waits. The three legs' results are compared byte for byte once before timing
and after every round. No ratio is fixed in advance; the two ratios lone / group and group / batch are reported.

The thresholds are taken from the data: the objectness threshold is the 99th percentile of frame 0's objectness (about 1 % of the
candidates stay, as in tools/bench_yolox_head.py), the class threshold 0 - random parameters say nothing else.

  python tools/bench_yolox_net_group.py [--rounds R] [--block B] [--warmup W] [--variants nano,tiny,s] [--out profiles/yolox_net_group_bench.txt]
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
import bench_yolox_net as B  # noqa: E402  (the size, the classes and the seeded parameters of the lone benchmark)

MEMBERS = 32
H, W = B.H, B.W
A = sum((H >> (3 + l)) * (W >> (3 + l)) for l in range(3))
MAX_DETS = B.MAX_DETS
LEGS = ("lone", "group", "batch")


class Bench:
    def __init__(self, owner, net):
        self.owner, self.net, self.L = owner, net, owner.L
        self.ctxs = [mi355fx.Context(0) for _ in range(MEMBERS)]
        frames = np.random.default_rng(5).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
        self.pitch, self.stride = H * W * 3, 3 * W
        self.d_frames = owner.alloc(self.pitch * MEMBERS)
        for k in range(MEMBERS):
            owner.h2d(self.d_frames + k * self.pitch, frames[k % len(frames)])
        # the thresholds: about 1 % of frame 0's candidates stay
        F = 5 + B.CLASSES
        tensor = np.zeros((A, F), np.float32)
        d_t = owner.alloc(tensor.nbytes)
        net.infer_frames_device(self.d_frames, self.pitch, self.stride, 1, W, H, d_t, tensor.nbytes)
        owner.synchronize()
        owner.d2h(tensor, d_t)
        owner.free(d_t)
        self.params = (float(np.percentile(tensor[:, 4], 99.0)), 0.0, 0.45)
        self.p1 = mi355fx.YoloParams(*self.params)
        self.p32 = mi355fx._yolo_params([self.params] * MEMBERS)[0]
        self.dets = {leg: np.zeros((MEMBERS, MAX_DETS), mi355fx.YOLO_DET) for leg in LEGS}
        self.n = {leg: (C.c_uint32 * MEMBERS)() for leg in LEGS}
        self.tickets = (C.c_uint64 * MEMBERS)()
        # member k's count and ticket, as the pointers the entry points take
        self.n_at = {leg: [C.cast(C.addressof(self.n[leg]) + 4 * k, C.POINTER(C.c_uint32)) for k in range(MEMBERS)] for leg in LEGS}
        self.ticket_at = [C.cast(C.addressof(self.tickets) + 8 * k, C.POINTER(C.c_uint64)) for k in range(MEMBERS)]
        self.g = mi355fx.Group(0)
        self.submit_s, self.wait_s = [], []

    def frame(self, k):
        return self.d_frames + k * self.pitch

    def lone(self):
        dets, n = self.dets["lone"], self.n_at["lone"]
        for k in range(MEMBERS):
            rc = self.L.mi355_yolox_infer_dets_device(self.net.h, self.frame(k), 0, self.stride, 1, W, H, C.byref(self.p1), dets[k].ctypes.data, MAX_DETS,
                                                      n[k])
            assert rc == 0, rc

    def group(self):
        dets, n, g = self.dets["group"], self.n_at["group"], self.g
        t0 = time.perf_counter()
        for k in range(MEMBERS):
            rc = self.L.mi355_group_submit_yolox_infer(g.h, self.ctxs[k].h, self.net.h, self.frame(k), self.stride, W, H, C.byref(self.p1), MAX_DETS,
                                                       self.ticket_at[k])
            assert rc == 0, rc
        t1 = time.perf_counter()
        for k in range(MEMBERS):
            rc = self.L.mi355_group_wait_yolodec(g.h, self.tickets[k], dets[k].ctypes.data, n[k])
            assert rc == 0, rc
        self.submit_s.append(t1 - t0)
        self.wait_s.append(time.perf_counter() - t1)

    def batch(self):
        rc = self.L.mi355_yolox_infer_dets_device(self.net.h, self.d_frames, self.pitch, self.stride, MEMBERS, W, H, self.p32, self.dets["batch"].ctypes.data, MAX_DETS,
                                                  self.n["batch"])
        assert rc == 0, rc

    def result(self, leg):
        n = list(self.n[leg])
        return n, b"".join(self.dets[leg][k, :min(n[k], MAX_DETS)].tobytes() for k in range(MEMBERS))

    def same(self):
        ref = self.result("lone")
        return all(self.result(leg) == ref for leg in LEGS)

    def close(self):
        self.g.close()
        self.owner.free(self.d_frames)
        for c in self.ctxs:
            c.close()


def stats_row(times_s):
    ms = np.array(times_s) * 1e3
    p5, p95 = np.percentile(ms, 5), np.percentile(ms, 95)
    return dict(ms_per_interval_median=float(np.median(ms)), ms_per_interval_p5=float(p5), ms_per_interval_p95=float(p95), ms_spread=float(p95 - p5) / 2,
                ms_per_frame_median=float(np.median(ms)) / MEMBERS)


def measure(owner, net, warmup, rounds, block):
    b = Bench(owner, net)
    for leg in LEGS:
        for _ in range(warmup):
            getattr(b, leg)()
    assert b.same(), "the three legs differ"
    before, infer_before = b.g.yolodec_stats(), b.g.yolox_infer_stats()
    b.submit_s, b.wait_s = [], []
    times = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg in LEGS:
            fn = getattr(b, leg)
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                times[leg].append(time.perf_counter() - t0)
        assert b.same(), "the three legs differ"
    rows = {leg: stats_row(v) for leg, v in times.items()}
    t, s, _, k = (x - y for x, y in zip(b.g.yolodec_stats(), before))
    st = b.g.yolox_infer_stats()
    rows["group"].update(members_launched=t, launch_sets=s, launches_per_set=k / max(s, 1), forwards=st[1] - infer_before[1], frames_in_the_largest_forward=st[2],
                         lanes=st[4], lane_allocations=st[5], ms_in_the_32_submits_median=float(np.median(b.submit_s)) * 1e3,
                         ms_in_the_32_waits_median=float(np.median(b.wait_s)) * 1e3)
    mean_dets = float(np.mean(b.result("lone")[0]))
    params = b.params
    b.close()
    return rows, mean_dets, params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variants", default="nano,tiny,s")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_net_group_bench.txt"))
    a = ap.parse_args()
    rows = []
    with mi355fx.Context(0) as owner:
        for variant in a.variants.split(","):
            cfg = mi355fx.yolox_net_config(*mi355fx.YOLOX_VARIANTS[variant], B.CLASSES)
            with mi355fx.YoloxNet(owner, cfg) as net:
                for k, arr in enumerate(B.seeded_params(net.params(), 11)):
                    net.set_param(k, arr)
                net.finalize()
                r, mean_dets, params = measure(owner, net, a.warmup, a.rounds, a.block)
                for leg in LEGS:
                    rows.append(dict(case="gpu", variant=variant, leg=leg, intervals=a.rounds * a.block, rounds=a.rounds, **r[leg]))
                lone, grp, bat = (r[leg]["ms_per_interval_median"] for leg in LEGS)
                rows.append(dict(case="gpu", variant=variant, members=MEMBERS, size=(H, W), classes=B.CLASSES, launches_per_forward=net.launches(), max_dets=MAX_DETS,
                                 thresholds=params, detections_mean=mean_dets, lone_over_group=lone / grp, group_over_batch=grp / bat, ms_group_minus_batch=grp - bat,
                                 ms_spreads_group_and_batch=r["group"]["ms_spread"] + r["batch"]["ms_spread"]))
    rows.append(dict(note="an interval is one frame per member, one thread: lone = 32 calls of one frame, each ending in a synchronisation; group = 32 submits and 32 "
                          "waits, one set with one forward of 32 frames; batch = one lone call over the same 32 frames. Rounds alternate the three legs; spread = "
                          "(p95 - p5) / 2 over all intervals of a leg. Random parameters: the detections say nothing. One MI355X, one run."))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""yoloxinference's network timing: YOLOX-nano, -tiny and -s with 80 classes at 640 x 640, seeded random parameters, as
1, 8 and 32 frames per call on one MI355X. Two legs, every call ending in a stream synchronisation:

  (i)  forward    : mi355_yolox_net_forward_device alone on an input tensor converted beforehand.
  (ii) infer_dets : mi355_yolox_infer_dets_device - RGB frames on the device in, detections out (conversion, forward, head decode, NMS,
                    download of the records).

The legs run in the same process INTERLEAVED: after the warm-up of both, --rounds rounds, each --block calls of every leg in turn, a
host clock around every call. Per leg: the median over all calls, the 5th and 95th percentile and the spread (half of p95 - p5). The
forward's FLOPs are 2 x the multiply-adds of the plan (mi355_selftest_yolox_net_plan); `fraction_of_f32_peak` is FLOPs / median time
over the 157.3 TFLOPS of the vector f32 FMA peak. Reported, not asserted.

  python tools/bench_yolox_net.py [--rounds R] [--block B] [--warmup W] [--variants nano,tiny,s] [--frames 1,8,32] [--out profiles/yolox_net_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))

import mi355fx  # noqa: E402

H = W = 640
CLASSES = 80
F32_PEAK_TFLOPS = 157.3
PARAMS = (0.5, 0.5, 0.45)
MAX_DETS = 128
LEGS = ("forward", "infer_dets")


def seeded_params(table, seed):
    """weights ~ N(0, 1 / fan_in), BatchNorm near the identity, prediction biases at the reference's prior (head.rs:18, :140)"""
    rng = np.random.default_rng(seed)
    out = []
    for name, dims in table:
        if name.endswith(".bn.weight"):
            a = rng.uniform(0.9, 1.1, dims)
        elif name.endswith(".bn.bias") or name.endswith(".bn.running_mean"):
            a = rng.uniform(-0.1, 0.1, dims)
        elif name.endswith(".bn.running_var"):
            a = rng.uniform(0.8, 1.2, dims)
        elif name.endswith(".bias"):
            a = np.full(dims, -np.log((1 - 1e-2) / 1e-2))
        else:
            a = rng.normal(0.0, 1.0 / np.sqrt(dims[1] * dims[2] * dims[3]), dims)
        out.append(a.astype(np.float32))
    return out


class Batch:
    def __init__(self, ctx, net, n):
        self.ctx, self.net, self.n = ctx, net, n
        frames = np.random.default_rng(5).integers(0, 256, (min(n, 4), H, W, 3), dtype=np.uint8)
        self.pitch = H * W * 3
        self.d_frames = ctx.alloc(self.pitch * n)
        for k in range(n):
            ctx.h2d(self.d_frames + k * self.pitch, frames[k % len(frames)])
        self.in_pitch = 3 * H * W * 4
        self.d_in = ctx.alloc(self.in_pitch * n)
        ctx.yolox_input_frames_device(self.d_frames, self.pitch, 3 * W, n, W, H, self.d_in, self.in_pitch)
        ctx.synchronize()
        self.dets = None

    def forward(self):
        self.net.forward_device(self.d_in, self.in_pitch, self.n, H, W)
        self.ctx.synchronize()

    def infer_dets(self):
        self.dets = self.net.infer_dets_device(self.d_frames, self.pitch, 3 * W, self.n, W, H, [PARAMS] * self.n, MAX_DETS, return_counts=True)

    def close(self):
        self.ctx.free(self.d_frames)
        self.ctx.free(self.d_in)


def stats_row(times_s):
    ms = np.array(times_s) * 1e3
    p5, p95 = np.percentile(ms, 5), np.percentile(ms, 95)
    return dict(ms_per_call_median=float(np.median(ms)), ms_per_call_p5=float(p5), ms_per_call_p95=float(p95), ms_spread=float(p95 - p5) / 2)


def measure(ctx, net, n, warmup, rounds, block):
    b = Batch(ctx, net, n)
    for name in LEGS:
        for _ in range(warmup):
            getattr(b, name)()
    times = {name: [] for name in LEGS}
    for _ in range(rounds):
        for name in LEGS:
            fn = getattr(b, name)
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
    counts = b.dets[1]
    b.close()
    return {name: stats_row(v) for name, v in times.items()}, float(np.mean(counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variants", default="nano,tiny,s")
    ap.add_argument("--frames", default="1,8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_net_bench.txt"))
    a = ap.parse_args()
    rows = []
    with mi355fx.Context(0) as ctx:
        for variant in a.variants.split(","):
            cfg = mi355fx.yolox_net_config(*mi355fx.YOLOX_VARIANTS[variant], CLASSES)
            with mi355fx.YoloxNet(ctx, cfg) as net:
                for k, arr in enumerate(seeded_params(net.params(), 11)):
                    net.set_param(k, arr)
                net.finalize()
                for n in [int(v) for v in a.frames.split(",")]:
                    rc, plan = mi355fx.selftest_yolox_net_plan(cfg, n, H, W)
                    assert rc == 0
                    r, mean_dets = measure(ctx, net, n, a.warmup, a.rounds, a.block)
                    flops = 2.0 * plan.macs
                    fwd = r["forward"]["ms_per_call_median"] * 1e-3
                    for name in LEGS:
                        rows.append(dict(case="gpu", variant=variant, n_frames=n, leg=name, calls=a.rounds * a.block, **r[name],
                                         ms_per_frame_median=r[name]["ms_per_call_median"] / n))
                    rows.append(dict(case="gpu", variant=variant, n_frames=n, size=(H, W), classes=CLASSES, launches=plan.launches, arena_mib=plan.arena_bytes / 2 ** 20,
                                     forward_gflop=flops / 1e9, forward_tflops=flops / fwd / 1e12, fraction_of_f32_peak=flops / fwd / 1e12 / F32_PEAK_TFLOPS,
                                     detections_mean=mean_dets))
    rows.append(dict(note="a call ends in a stream synchronisation; infer_dets also downloads n_frames x max_dets records. Rounds alternate the two legs; spread = "
                          "(p95 - p5) / 2 over all calls of a leg. Random parameters: the detections say nothing. One MI355X, one run."))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

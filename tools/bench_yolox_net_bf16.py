"""yoloxinference's network under its two precisions: YOLOX-nano, -tiny and -s with 80 classes at 640 x 640, the SAME
seeded random parameters as an F32 net and as a BF16 net (mi355_yolox_net_set_precision) on one context, as 1, 8 and 32 frames per call
on one MI355X. Per precision two legs, every call ending in a stream synchronisation:

  forward    : mi355_yolox_net_forward_device alone on an input tensor converted beforehand.
  infer_dets : mi355_yolox_infer_dets_device - RGB frames on the device in, detections out.

The four (precision, leg) pairs run in the same process INTERLEAVED: after the warm-up of all, --rounds rounds, each --block calls of
every pair in turn, a host clock around every call (5 x 10 = 50 calls per pair). Per pair: the median over all calls, the 5th and 95th
percentile and the spread (half of p95 - p5). The f32 legs run the code the library always ran and are the yardstick; a `speedup` row
gives f32 median / bf16 median and `beyond_spread`: whether the difference of the medians exceeds the SUM of the two spreads.
Reported, not asserted.

  python tools/bench_yolox_net_bf16.py [--rounds R] [--block B] [--warmup W] [--variants nano,tiny,s] [--frames 1,8,32] [--out profiles/yolox_net_bf16_bench.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mi355fx  # noqa: E402
import bench_yolox_net as F  # noqa: E402

PRECISIONS = ("f32", "bf16")
BF16_PEAK_TFLOPS = 2516.6


def measure(ctx, nets, n, warmup, rounds, block):
    batches = {p: F.Batch(ctx, nets[p], n) for p in PRECISIONS}
    pairs = [(p, leg) for leg in F.LEGS for p in PRECISIONS]
    for p, leg in pairs:
        for _ in range(warmup):
            getattr(batches[p], leg)()
    times = {pair: [] for pair in pairs}
    for _ in range(rounds):
        for pair in pairs:
            fn = getattr(batches[pair[0]], pair[1])
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                times[pair].append(time.perf_counter() - t0)
    for b in batches.values():
        b.close()
    return {pair: F.stats_row(v) for pair, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variants", default="nano,tiny,s")
    ap.add_argument("--frames", default="1,8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_net_bf16_bench.txt"))
    a = ap.parse_args()
    rows = []
    with mi355fx.Context(0) as ctx:
        for variant in a.variants.split(","):
            cfg = mi355fx.yolox_net_config(*mi355fx.YOLOX_VARIANTS[variant], F.CLASSES)
            nets = {}
            try:
                for p in PRECISIONS:
                    nets[p] = net = mi355fx.YoloxNet(ctx, cfg)
                    net.set_precision(p)
                    for k, arr in enumerate(F.seeded_params(net.params(), 11)):
                        net.set_param(k, arr)
                    net.finalize()
                for n in [int(v) for v in a.frames.split(",")]:
                    rc, plan = mi355fx.selftest_yolox_net_plan(cfg, n, F.H, F.W)
                    assert rc == 0
                    r = measure(ctx, nets, n, a.warmup, a.rounds, a.block)
                    flops = 2.0 * plan.macs
                    for (p, leg), row in r.items():
                        extra = dict(forward_tflops=flops / (row["ms_per_call_median"] * 1e-3) / 1e12) if leg == "forward" else {}
                        rows.append(dict(case="gpu", variant=variant, n_frames=n, precision=p, leg=leg, calls=a.rounds * a.block, **row,
                                         ms_per_frame_median=row["ms_per_call_median"] / n, **extra))
                    for leg in F.LEGS:
                        f, b = r[("f32", leg)], r[("bf16", leg)]
                        gain = f["ms_per_call_median"] - b["ms_per_call_median"]
                        rows.append(dict(case="gpu", variant=variant, n_frames=n, leg=leg, speedup=f["ms_per_call_median"] / b["ms_per_call_median"],
                                         gain_ms=gain, sum_of_spreads_ms=f["ms_spread"] + b["ms_spread"], beyond_spread=bool(gain > f["ms_spread"] + b["ms_spread"])))
            finally:
                for net in nets.values():
                    net.close()
    rows.append(dict(note="a call ends in a stream synchronisation; infer_dets also downloads n_frames x max_dets records. Rounds alternate the four (precision, leg) "
                          "pairs; spread = (p95 - p5) / 2 over all calls of a pair. forward_tflops counts the plan's multiply-adds twice (bf16 matrix peak %.0f, f32 vector "
                          "peak %.1f TFLOPS). Random parameters: the detections say nothing. One MI355X, one run." % (BF16_PEAK_TFLOPS, F.F32_PEAK_TFLOPS)))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

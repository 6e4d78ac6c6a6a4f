"""agingradio timing: a lone instance on 10 ms of stereo at 48 kHz (host and device buffers, defaults and with the
lowpass off), a 10 s device buffer (the serial lowpass phase's ns per frame), and 32 / 256 stereo members of an agingradio audio
group per 10 ms interval (device and host buffers). Every timed call ends in a stream synchronisation (a group interval in its
launch set's), so a host clock around it times the work; the median of --reps calls after warm-up calls is reported.

The group is driven from one thread: the member that completes the set runs the launch set inline, so an interval here costs its
submits (host copies into the pinned slots) and the launch set, without thread hand-offs.

  python tools/bench_agingradio.py [--reps N] [--cpu tools/agingradio_cpu]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))

import mi355fx  # noqa: E402

DEFAULTS = dict(white_noise_ampl=0.011, clicks_prob=1.0 / 100000.0, bits_to_quantize=4.0, cubic_curve_distortion=1.0, cubic_curve_passes=3)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def lone(ctx, frames, lowpass, device, reps):
    x = np.sin(np.arange(frames * 2) * 1e-3).astype(np.float32)
    ctx.agingradio_setup(2, 48000, lowpass, 1)
    if device:
        d = ctx.alloc(x.nbytes)
        ctx.h2d(d, x)

        def run():
            ctx.agingradio_process_device(d, frames, False, DEFAULTS)
            ctx.synchronize()
        t = timed(run, reps)
        ctx.free(d)
        return t
    return timed(lambda: ctx.agingradio_process(x, 2, DEFAULTS), reps)


def group(n, device, lowpass, reps):
    g = mi355fx.AudioGroup("agingradio", n)
    g.set_linger(0)
    ctx = mi355fx.Context(0)
    xs = [np.sin(np.arange(960) * 1e-3 + m).astype(np.float32) for m in range(n)]
    ds = []
    for m in range(n):
        g.agingradio_setup(m, 2, 48000, lowpass, 100 + m)
        if device:
            ds.append(ctx.alloc(xs[m].nbytes))
            ctx.h2d(ds[m], xs[m])

    def interval():
        tickets = [g.submit_agingradio(m, ds[m], DEFAULTS, frames=480, is_f64=False) if device else g.submit_agingradio(m, xs[m], DEFAULTS, channels=2)
                   for m in range(n)]
        for t in tickets:
            g.wait(t)
    t = timed(interval, reps)
    st = g.stats()
    for d in ds:
        ctx.free(d)
    g.close()
    ctx.close()
    return t, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=51)
    ap.add_argument("--cpu", default=os.path.join(ROOT, "tools", "agingradio_cpu"))
    ap.add_argument("--no-long", action="store_true", help="skip the 10 s buffer")
    a = ap.parse_args()
    rows = []
    with mi355fx.Context(0) as ctx:
        for lowpass in (2000, 0):
            for device in (False, True):
                t = lone(ctx, 480, lowpass, device, a.reps)
                rows.append(dict(case="lone 10 ms stereo", buffers="device" if device else "host", lowpass=lowpass, ms=t * 1e3))
        if not a.no_long:
            for lowpass in (2000, 0):
                t = lone(ctx, 480000, lowpass, True, max(5, a.reps // 10))
                rows.append(dict(case="lone 10 s stereo", buffers="device", lowpass=lowpass, ms=t * 1e3, ns_per_frame=t * 1e9 / 480000))
    for n in (32, 256):
        for device in (True, False):
            t, st = group(n, device, 2000, a.reps)
            rows.append(dict(case="group %d stereo members, 10 ms interval" % n, buffers="device" if device else "host", lowpass=2000, ms=t * 1e3,
                             launch_sets=int(st[1]), buffers_total=int(st[0])))
    if os.path.exists(a.cpu):
        for lowpass in (2000, 0):
            out = subprocess.run([a.cpu, "2", "480", "10", str(lowpass)], capture_output=True, text=True, timeout=120).stdout.strip()
            r = json.loads(out)
            rows.append(dict(case="one CPU core, 10 ms stereo", buffers="host", lowpass=lowpass, ms=r["ms_per_buffer"], ns_per_sample=r["ns_per_sample"],
                             per_32_members_ms=32 * r["ms_per_buffer"], per_256_members_ms=256 * r["ms_per_buffer"]))
            out = subprocess.run([a.cpu, "2", "480000", "10", str(lowpass)], capture_output=True, text=True, timeout=120).stdout.strip()
            r = json.loads(out)
            rows.append(dict(case="one CPU core, 10 s stereo", buffers="host", lowpass=lowpass, ms=r["ms_per_buffer"], ns_per_frame=2 * r["ns_per_sample"]))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()

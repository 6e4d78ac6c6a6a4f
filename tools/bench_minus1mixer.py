"""minus1mixer timing: one 10 ms interval (480 frames at 48 kHz, S16 in and out) of a conference bridge with
N = 8, 64 and 256 participants, as a lone mixer on a context and as a group of 32 such rooms, and the same loop on one CPU core.

  lone, stream events : K intervals of mi355_mixer_process_device enqueued back to back on the context's stream between two stream
                        events (hipEventElapsedTime / K): the stream's time per interval, table copy included. It is the larger of
                        the device's time and the host's enqueue time per call (small rooms: the host's; the call builds and
                        enqueues a job table, and waits only for the table copy two calls back).
  lone, host clock    : one mi355_mixer_process_device + synchronise, and one mi355_mixer_process on host buffers (upload, launch,
                        download), median of --reps calls: what a streaming thread waits for.
  group of 32         : one interval = 32 submits and 32 waits from one thread (the submit that completes the set runs its launch
                        set inline, and the set ends in a stream synchronisation), device and host buffers, host clock, median. The
                        group's stream is its own, so no event brackets it from outside.
  one CPU core        : a C restatement of aggregate_one_buffer + split_output_buf (the interleaved f32 buffer N channels wide with
                        the branchy add per output channel, then the slicing pass), compiled here with -O3 -ffp-contract=off.

  python tools/bench_minus1mixer.py [--reps N] [--intervals K] [--cpu none]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))

import mi355fx  # noqa: E402

FRAMES = 480
SIZES = (8, 64, 256)
ROOMS = 32

CPU_SOURCE = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
/* one interval: every input's segment into the wide buffer, then one slicing pass per output */
static void interval(int n, int frames, const int16_t *in, const unsigned char *contrib, float *wide, int16_t *out) {
  memset(wide, 0, sizeof(float) * (size_t)n * frames);
  for (int i = 0; i < n; i++) {
    const unsigned char *c = contrib + (size_t)i * n;
    for (int f = 0; f < frames; f++) {
      const float s = (float)in[(size_t)i * frames + f] / 32768.0f;
      float *frame = wide + (size_t)f * n;
      for (int o = 0; o < n; o++)
        if (c[o]) frame[o] += s;
    }
  }
  for (int o = 0; o < n; o++)
    for (int f = 0; f < frames; f++) {
      const float v = wide[(size_t)f * n + o] * 32768.0f;
      out[(size_t)o * frames + f] = v != v ? 0 : v >= 32767.0f ? 32767 : v <= -32768.0f ? -32768 : (int16_t)v;
    }
}
int main(int argc, char **argv) {
  const int n = atoi(argv[1]), frames = atoi(argv[2]), reps = atoi(argv[3]);
  int16_t *in = malloc(sizeof(int16_t) * (size_t)n * frames), *out = malloc(sizeof(int16_t) * (size_t)n * frames);
  unsigned char *contrib = malloc((size_t)n * n);
  float *wide = malloc(sizeof(float) * (size_t)n * frames);
  uint32_t x = 12345;
  for (size_t k = 0; k < (size_t)n * frames; k++) { x = x * 1664525u + 1013904223u; in[k] = (int16_t)((x >> 16) % 201) - 100; }
  for (int i = 0; i < n; i++) for (int o = 0; o < n; o++) contrib[(size_t)i * n + o] = i != o;
  double best = 1e30, sum = 0;
  long check = 0;
  for (int r = 0; r < reps + 3; r++) {
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    interval(n, frames, in, contrib, wide, out);
    clock_gettime(CLOCK_MONOTONIC, &b);
    const double ms = (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) * 1e-6;
    check += out[(size_t)r % ((size_t)n * frames)];
    if (r < 3) continue;
    sum += ms;
    if (ms < best) best = ms;
  }
  printf("{\"ms_mean\": %.6f, \"ms_best\": %.6f, \"check\": %ld}\n", sum / reps, best, check);
  return 0;
}
"""


class Hip:
    """the three event calls of the HIP runtime the library is linked against"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so")
        for name, args in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                           ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
                           ("hipEventDestroy", [C.c_void_p])):
            getattr(self.L, name).argtypes = args
            getattr(self.L, name).restype = C.c_int

    def ck(self, rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    def event(self):
        e = C.c_void_p()
        self.ck(self.L.hipEventCreate(C.byref(e)))
        return e


def median_of(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def room(rng, n):
    """(host input arrays, host output arrays) of one room: n S16 participants, 480 frames"""
    return [rng.integers(-100, 101, FRAMES).astype(np.int16) for _ in range(n)], [np.zeros(FRAMES, np.int16) for _ in range(n)]


def on_device(ctx, ins, outs):
    d_in, d_out = ctx.alloc(FRAMES * 2 * len(ins)), ctx.alloc(FRAMES * 2 * len(outs))
    for i, x in enumerate(ins):
        ctx.h2d(d_in + i * FRAMES * 2, x)
    ctx.synchronize()
    segs = [(i, (d_in + i * FRAMES * 2, 1, FRAMES), 0) for i in range(len(ins))]
    douts = [((d_out + o * FRAMES * 2, 1), o, 1) for o in range(len(outs))]
    return (d_in, d_out), segs, douts


def lone(hip, n, reps, intervals):
    rng = np.random.default_rng(n)
    ins, outs = room(rng, n)
    with mi355fx.Context(0) as ctx:
        ctx.mixer_setup_minus1(n)
        held, segs, douts = on_device(ctx, ins, outs)
        sa, oa = mi355fx.mixer_tables(segs, douts)   # built once: the timed loop is the library call alone

        def enqueue():
            ctx._ck(ctx.L.mi355_mixer_process_device(ctx.h, sa, n, oa, n, FRAMES))

        def sync_call():
            enqueue()
            ctx.synchronize()
        for _ in range(5):
            sync_call()
        stream = ctx.L.mi355_ctx_stream(ctx.h)
        e0, e1 = hip.event(), hip.event()
        per = []
        for _ in range(max(3, reps // 10)):
            hip.ck(hip.L.hipEventRecord(e0, stream))
            for _ in range(intervals):
                enqueue()
            hip.ck(hip.L.hipEventRecord(e1, stream))
            hip.ck(hip.L.hipEventSynchronize(e1))
            ms = C.c_float(0)
            hip.ck(hip.L.hipEventElapsedTime(C.byref(ms), e0, e1))
            per.append(ms.value / intervals)
        hip.L.hipEventDestroy(e0)
        hip.L.hipEventDestroy(e1)
        t_dev = median_of(sync_call, reps)
        hs, ho = mi355fx.mixer_tables([(i, x, 0) for i, x in enumerate(ins)], [(y, o, 1) for o, y in enumerate(outs)])
        t_host = median_of(lambda: ctx._ck(ctx.L.mi355_mixer_process(ctx.h, hs, n, ho, n, FRAMES)), reps)
        for p in held:
            ctx.free(p)
    return dict(case="lone mixer", participants=n, frames=FRAMES, stream_ms_per_interval_events=float(np.median(per)), intervals_per_event_pair=intervals,
                host_clock_ms_device_buffers=t_dev * 1e3, host_clock_ms_host_buffers=t_host * 1e3)


def group(n, device, reps):
    rng = np.random.default_rng(1000 + n)
    g = mi355fx.AudioGroup("mixer", ROOMS)
    g.set_linger(0)
    ctx = mi355fx.Context(0)
    calls, held = [], []
    for m in range(ROOMS):
        g.mixer_setup_minus1(m, n)
        ins, outs = room(rng, n)
        if device:
            h, segs, douts = on_device(ctx, ins, outs)
            held += list(h)
            calls.append(mi355fx.mixer_tables(segs, douts) + (ins, outs))
        else:
            calls.append(mi355fx.mixer_tables([(i, x, 0) for i, x in enumerate(ins)], [(y, o, 1) for o, y in enumerate(outs)]) + (ins, outs))
    tickets = [C.c_uint64(0) for _ in range(ROOMS)]

    def interval():
        for m, (sa, oa, _, _) in enumerate(calls):
            g._ck(g.L.mi355_agroup_submit_mixer(g.h, m, sa, n, oa, n, FRAMES, int(device), C.byref(tickets[m])))
        for t in tickets:
            g._ck(g.L.mi355_agroup_wait(g.h, t.value, None))
    t = median_of(interval, reps)
    st, launches = g.stats(), g.mixer_launches()
    for p in held:
        ctx.free(p)
    g.close()
    ctx.close()
    return dict(case="group of %d rooms" % ROOMS, participants=n, frames=FRAMES, buffers="device" if device else "host", host_clock_ms_per_interval=t * 1e3,
                launch_sets=int(st[1]), kernel_launches=int(launches))


def cpu_rows(reps):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        return [dict(case="one CPU core", error="no C compiler here: not measured")]
    rows = []
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "mix_cpu.c"), os.path.join(d, "mix_cpu")
        open(src, "w").write(CPU_SOURCE)
        subprocess.check_call([cc, "-O3", "-std=c11", "-D_POSIX_C_SOURCE=199309L", "-ffp-contract=off", src, "-o", exe])
        for n in SIZES:
            r = json.loads(subprocess.run([exe, str(n), str(FRAMES), str(reps)], capture_output=True, text=True, timeout=300, check=True).stdout)
            rows.append(dict(case="one CPU core", participants=n, frames=FRAMES, ms_per_interval_mean=r["ms_mean"], ms_per_interval_best=r["ms_best"],
                             ms_for_32_rooms_mean=ROOMS * r["ms_mean"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=101)
    ap.add_argument("--intervals", type=int, default=200, help="intervals between the two events of a device-time sample")
    ap.add_argument("--cpu", default="cc", help="'none' skips the CPU leg")
    a = ap.parse_args()
    rows = []
    hip = Hip()
    for n in SIZES:
        rows.append(lone(hip, n, a.reps, a.intervals))
    for n in SIZES:
        for device in (True, False):
            rows.append(group(n, device, a.reps))
    if a.cpu != "none":
        rows += cpu_rows(a.reps)
    rows.append(dict(note="group rows are a host clock around 32 submits + 32 waits (the launch set ends in a stream synchronisation): the group's "
                          "stream is its own, so no event brackets it from outside; the lone rows' event figure is stream time per interval = "
                          "max(device time, host enqueue time per call)"))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()

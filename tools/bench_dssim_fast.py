"""Dssim on (reference, frame) pairs: the exact form against the fast form (MI355_FLAG_DSSIM_FAST).

  pairs  --pairs 4K RGBA device frames per call through mi355_dssim_compare_pairs_device on one context; the flag alternates
         0, 1, 0, 1, ... between repeats in one process. A repeat is --calls calls; every call ends in the library's own
         synchronisation, so the host clock around a repeat times finished device work.
  group  (--members N, 0 to leave it out) N contexts, N native threads, one pair each per interval through the video group's
         compare queue with a rendezvous of N; the members' flag alternates between repeats in the same way.

Per form: median, minimum and maximum over the repeats, in ms per pair and pairs/s, the ratio of the medians, and the values the two
forms give for the first pairs (they differ by f32 rounding noise; identical frames give 0.0 in both). No profiler, no counters: a
--pmc or kernel-trace pass is a run of its own.

  python tools/bench_dssim_fast.py [--pairs 8] [--calls 6] [--repeats 5] [--members 32] [--width 3840 --height 2160] [--out FILE]
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))

import mi355fx  # noqa: E402


def frames(rng, w, h, n):
    """n (reference, frame) pairs: smooth blocks, the frame a noisy copy (amplitude 2 + 5 k); pair 0 identical."""
    out = []
    for k in range(n):
        base = np.kron(rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 4), dtype=np.uint8), np.ones((8, 8, 1), np.uint8))[:h, :w].copy()
        base[..., 3] = 255
        mod = base.copy()
        if k:
            mod[..., :3] = np.clip(base[..., :3].astype(np.int16) + rng.integers(-2 - 5 * k, 3 + 5 * k, (h, w, 3)), 0, 255).astype(np.uint8)
        out.append((base.reshape(-1), mod.reshape(-1)))
    return out


def stats(ts, pairs):
    ms = np.array(ts) * 1e3 / pairs
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def line(name, s):
    return "%-28s median %.4f ms/pair (%.0f pairs/s)   min %.4f   max %.4f" % (name, s[0], 1e3 / s[0], s[1], s[2])


def bench_pairs(a, emit):
    rng = np.random.default_rng(7)
    w, h = a.width, a.height
    with mi355fx.Context(0) as c:
        dev = []
        for ref, mod in frames(rng, w, h, a.pairs):
            dr, dm = c.alloc(ref.nbytes), c.alloc(mod.nbytes)
            c.h2d(dr, ref); c.h2d(dm, mod)
            dev.append((dr, dm))
        refs, mods = [p[0] for p in dev], [p[1] for p in dev]
        values, ts = {}, {0: [], 1: []}
        for flag in (0, 1):                                  # warm-up: code objects, scratch, image pools
            c.set_flag(mi355fx.FLAG_DSSIM_FAST, flag)
            for _ in range(2):
                values[flag] = c.dssim_compare_pairs_device(refs, mods, w * 4, w, h)
        for rep in range(2 * a.repeats):
            flag = rep % 2
            c.set_flag(mi355fx.FLAG_DSSIM_FAST, flag)
            t0 = time.perf_counter()
            for _ in range(a.calls):
                got = c.dssim_compare_pairs_device(refs, mods, w * 4, w, h)
            ts[flag].append((time.perf_counter() - t0) / a.calls)
            assert got == values[flag], "a form's values changed between calls"
        for dr, dm in dev:
            c.free(dr); c.free(dm)
    s0, s1 = stats(ts[0], a.pairs), stats(ts[1], a.pairs)
    emit("pairs: %d pairs of %dx%d RGBA per call, %d calls per repeat, %d repeats per form, forms alternating" % (a.pairs, w, h, a.calls, a.repeats))
    emit(line("  exact (flag 0)", s0))
    emit(line("  fast  (flag 1)", s1))
    emit("  exact / fast = %.2f (medians); spread exact %.1f %%, fast %.1f %% ((max - min) / median)" %
         (s0[0] / s1[0], 100 * (s0[2] - s0[1]) / s0[0], 100 * (s1[2] - s1[1]) / s1[0]))
    emit("  values exact: " + " ".join("%.9f" % v for v in values[0][:4]))
    emit("  values fast:  " + " ".join("%.9f" % v for v in values[1][:4]))
    emit("  max |fast - exact| over the pairs: %.3e" % max(abs(x - y) for x, y in zip(values[0], values[1])))
    assert values[0][0] == 0.0 and values[1][0] == 0.0


def bench_group(a, emit):
    n, w, h = a.members, a.width, a.height
    rng = np.random.default_rng(11)
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    g = mi355fx.Group(0)
    try:
        g.set_rendezvous(n, 20000)   # all members of an interval in one launch sequence (linger 20 ms)
        dev = []
        base = frames(rng, w, h, 4)
        for s, c in enumerate(ctxs):
            ref, mod = base[s % 4]
            dr, dm = c.alloc(ref.nbytes), c.alloc(mod.nbytes)
            c.h2d(dr, ref); c.h2d(dm, mod)
            dev.append((dr, dm))
        ts = {0: [], 1: []}
        bar = threading.Barrier(n)
        errors = []

        def member(s, flag, reps, sink):
            try:
                for k in range(reps):
                    bar.wait()
                    t0 = time.perf_counter()
                    g.wait_compare(g.submit_compare(ctxs[s], dev[s][0], dev[s][1], w * 4, w, h, "RGBA", 5))
                    bar.wait()
                    if s == 0 and k >= 1:
                        sink.append(time.perf_counter() - t0)
            except Exception as e:
                errors.append(e)
                bar.abort()

        for rep in range(2 * a.repeats + 2):
            flag = rep % 2
            for c in ctxs:
                c.set_flag(mi355fx.FLAG_DSSIM_FAST, flag)
            sink = []
            th = [threading.Thread(target=member, args=(s, flag, a.calls + 1, sink)) for s in range(n)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            if errors:
                raise errors[0]
            if rep >= 2:                                     # the first run of each form is warm-up
                ts[flag].append(float(np.mean(sink)))
        st = g.compare_stats()
        for c, (dr, dm) in zip(ctxs, dev):
            c.free(dr); c.free(dm)
    finally:
        g.close()
        for c in ctxs:
            c.close()
    s0, s1 = stats(ts[0], n), stats(ts[1], n)
    emit("group: %d members on %d threads, one %dx%d RGBA pair each per interval, %d intervals per repeat, %d repeats per form" % (n, n, w, h, a.calls, a.repeats))
    emit("  (%d pairs in %d launch sequences, largest %d)" % st)
    emit(line("  exact members", s0))
    emit(line("  fast members", s1))
    emit("  exact / fast = %.2f (medians)" % (s0[0] / s1[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("at least 5 repeats per form")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("tools/bench_dssim_fast.py --pairs %d --calls %d --repeats %d --members %d --width %d --height %d" % (a.pairs, a.calls, a.repeats, a.members, a.width, a.height))
    bench_pairs(a, emit)
    if a.members > 0:
        bench_group(a, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

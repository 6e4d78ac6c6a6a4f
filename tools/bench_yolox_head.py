"""YOLOX head decode timing: seeded synthetic head maps of the real shape - levels 80 x 80, 40 x 40, 20 x 20 with
strides 8 / 16 / 32, 80 classes, 8400 candidates, about 1 % of them above both thresholds - as 1, 8, 32 and 256 tensors per call on
one MI355X. Three legs, every call ending in its own stream synchronisation and download:

  (i)   fused       : mi355_yolox_head_dets_device - head maps to detections, two launches, no decoded tensor.
  (ii)  materialise : mi355_yolox_head_decode_device, then mi355_yolodec_tensors_device (X) on the tensor it wrote.
  (iii) x_decoder   : mi355_yolodec_tensors_device (X) alone on a tensor decoded beforehand - the tensor decoder's code path as it
                      was, paying nothing for the decode.

The legs run in the same process on the same heads, INTERLEAVED: after the warm-up of all three, --rounds rounds, each --block calls
of every leg in turn, a host clock around every call. Per leg: the median over all calls, the 5th and 95th percentile, the spread
(half of p95 - p5) and the medians of the rounds. The three legs' records are compared byte for byte. `fused_no_slower` says whether
the fused median is at most the X decoder's plus the two spreads together. One CPU core: tools/yolox_head_cpu.cpp (decode, then the
X decoder's restatement) on the same heads, compiled here; "cpu: not measured" when no compiler is found.

  python tools/bench_yolox_head.py [--rounds R] [--block B] [--warmup W] [--out profiles/yolox_head_bench.txt] [--child N_TENSORS]
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

SHAPES, STRIDES, CLASSES = ((80, 80), (40, 40), (20, 20)), (8, 16, 32), 80
A = sum(h * w for h, w in SHAPES)
F = 5 + CLASSES
BATCHES = (1, 8, 32, 256)
PARAMS = (0.36, 0.45, 0.45)
MAX_DETS = 128
LEGS = ("fused", "materialise", "x_decoder")


def head(seed):
    """Low objectness and class logits everywhere; 1.25 % of the candidates with a confident objectness and one confident class out of
    five; offsets of a few cells around twelve centres per level so that NMS has work. -> (reg, obj, cls, stride) per level."""
    rng = np.random.default_rng(seed)
    levels = []
    for (h, w), s in zip(SHAPES, STRIDES):
        hw = h * w
        reg = np.concatenate([rng.normal(0.0, 1.5, (2, hw)), rng.normal(1.2, 0.3, (2, hw))]).astype(np.float32)
        obj = rng.normal(-5.0, 1.0, (1, hw)).astype(np.float32)
        cls = rng.normal(-4.0, 1.0, (CLASSES, hw)).astype(np.float32)
        hot = np.nonzero(rng.random(hw) < 0.0125)[0]
        obj[0, hot] = rng.uniform(0.0, 4.0, len(hot)).astype(np.float32)
        cls[rng.integers(0, 5, len(hot)), hot] = rng.uniform(0.5, 4.0, len(hot)).astype(np.float32)
        levels.append((reg.reshape(4, h, w), obj.reshape(1, h, w), cls.reshape(CLASSES, h, w), s))
    return levels


def heads(T):
    base = [head(100 + k) for k in range(min(T, 8))]   # eight distinct heads, repeated: the device reads T distinct buffers
    return [base[k % len(base)] for k in range(T)]


class Batch:
    """T heads uploaded in the engine's fused [5 + C, h, w] form per level, the decoded tensors beside them, and the arrays of a call"""

    def __init__(self, ctx, T):
        self.ctx, self.T = ctx, T
        hs = heads(T)
        self.maps, self.levels = [], []
        for l, ((h, w), s) in enumerate(zip(SHAPES, STRIDES)):
            hw, pitch = h * w, F * h * w * 4
            d = ctx.alloc(pitch * T)
            for k, hd in enumerate(hs):
                ctx.h2d(d + k * pitch, np.concatenate([a.reshape(-1) for a in hd[l][:3]]))
            self.maps.append(d)
            self.levels.append((d, d + 16 * hw, d + 20 * hw, pitch, pitch, pitch, h, w, s))
        self.lv = mi355fx._yolox_levels(self.levels)
        self.pitch = A * F * 4
        self.d_pre, self.d_tmp = ctx.alloc(self.pitch * T), ctx.alloc(self.pitch * T)
        self.p = (mi355fx.YoloParams * T)(*[mi355fx.YoloParams(*PARAMS) for _ in range(T)])
        self.dets = np.zeros(T * MAX_DETS, mi355fx.YOLO_DET)
        self.n = (C.c_uint32 * T)()
        ctx._ck(ctx.L.mi355_yolox_head_decode_device(ctx.h, self.lv, len(SHAPES), T, CLASSES, self.d_pre, self.pitch))
        ctx.synchronize()

    def fused(self):
        c = self.ctx
        c._ck(c.L.mi355_yolox_head_dets_device(c.h, self.lv, len(SHAPES), self.T, CLASSES, self.p, self.dets.ctypes.data, MAX_DETS, self.n))

    def x_on(self, d):
        c = self.ctx
        c._ck(c.L.mi355_yolodec_tensors_device(c.h, d, self.pitch, self.T, mi355fx.YOLO_LAYOUT["X"], F, A, self.p, self.dets.ctypes.data, MAX_DETS, self.n))

    def materialise(self):
        c = self.ctx
        c._ck(c.L.mi355_yolox_head_decode_device(c.h, self.lv, len(SHAPES), self.T, CLASSES, self.d_tmp, self.pitch))
        self.x_on(self.d_tmp)

    def x_decoder(self):
        self.x_on(self.d_pre)

    def result(self):
        n = list(self.n)
        return n, b"".join(self.dets[t * MAX_DETS: t * MAX_DETS + min(n[t], MAX_DETS)].tobytes() for t in range(self.T))

    def close(self):
        for d in self.maps + [self.d_pre, self.d_tmp]:
            self.ctx.free(d)


def stats_row(times_s, block, T):
    us = np.array(times_s) * 1e6
    p5, p95 = np.percentile(us, 5), np.percentile(us, 95)
    rounds = [float(np.median(us[k:k + block])) for k in range(0, len(us), block)]
    return dict(us_per_call_median=float(np.median(us)), us_per_call_mean=float(us.mean()), us_per_call_p5=float(p5), us_per_call_p95=float(p95),
                us_spread=float(p95 - p5) / 2, us_round_medians_min=min(rounds), us_round_medians_max=max(rounds), us_per_tensor_median=float(np.median(us)) / T)


def measure(ctx, T, warmup, rounds, block):
    b = Batch(ctx, T)
    ref = None
    for name in LEGS:
        for _ in range(warmup):
            getattr(b, name)()
        ref = ref or b.result()
        assert b.result() == ref, "the legs disagree: %s" % name
    times = {name: [] for name in LEGS}
    for _ in range(rounds):
        for name in LEGS:
            fn = getattr(b, name)
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
            assert b.result() == ref, "the legs disagree: %s" % name
    rows = {name: stats_row(v, block, T) for name, v in times.items()}
    n = ref[0]
    b.close()
    return rows, float(np.mean(n)), int(n[0])


def cpu_rows(reps=5):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        return [dict(case="one CPU core", note="cpu: not measured")]
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libyolox_head_cpu.so")
        subprocess.check_call([cxx, "-O3", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tools", "yolox_head_cpu.cpp"), "-o", so])
        L = C.CDLL(so)
        L.yolox_head_dets_cpu.restype = C.c_int
        L.yolox_head_dets_cpu.argtypes = [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_uint32)] * 3 + [C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                                                                                         C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        hs = heads(8)
        n_lv = len(SHAPES)
        args = []
        for hd in hs:
            ptrs = [(C.c_void_p * n_lv)(*[lv[k].ctypes.data for lv in hd]) for k in range(3)]
            dims = [(C.c_uint32 * n_lv)(*v) for v in ([h for h, _ in SHAPES], [w for _, w in SHAPES], STRIDES)]
            args.append(ptrs + dims + [n_lv])
        scratch, dets, n = np.zeros(A * F, np.float32), np.zeros(MAX_DETS, mi355fx.YOLO_DET), C.c_uint32(0)
        times = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            for a in args:
                assert L.yolox_head_dets_cpu(*a, CLASSES, *PARAMS, scratch.ctypes.data, dets.ctypes.data, MAX_DETS, C.byref(n)) == 0
            times.append((time.perf_counter() - t0) / len(args))
        times = times[1:]
    return [dict(case="one CPU core", levels=SHAPES, classes=CLASSES, candidates=A, ms_per_tensor_mean=float(np.mean(times)) * 1e3,
                 ms_per_tensor_best=float(min(times)) * 1e3, ms_for_256_tensors_mean=float(np.mean(times)) * 1e3 * 256)]


def child(T, calls=23):
    """what a profiler watches (`rocprofv3 --kernel-trace --stats -- python tools/bench_yolox_head.py --child 256`): the three legs"""
    with mi355fx.Context(0) as ctx:
        b = Batch(ctx, T)
        for name in LEGS:
            for _ in range(calls):
                getattr(b, name)()
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_head_bench.txt"))
    ap.add_argument("--child", type=int, metavar="N_TENSORS", help="only the calls of one batch size (for a profiler run)")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return
    rows = []
    with mi355fx.Context(0) as ctx:
        for T in BATCHES:
            r, mean_dets, first = measure(ctx, T, a.warmup, a.rounds, a.block)
            for name in LEGS:
                rows.append(dict(case="gpu", n_tensors=T, leg=name, calls=a.rounds * a.block, rounds=a.rounds, **r[name]))
            fu, x = r["fused"], r["x_decoder"]
            together = fu["us_spread"] + x["us_spread"]
            rows.append(dict(case="gpu", n_tensors=T, levels=SHAPES, classes=CLASSES, candidates=A, detections_mean=mean_dets, detections_first_tensor=first,
                             max_dets=MAX_DETS, x_decoder_over_fused_speed=x["us_per_call_median"] / fu["us_per_call_median"],
                             materialise_over_fused_speed=r["materialise"]["us_per_call_median"] / fu["us_per_call_median"], us_spreads_together=together,
                             fused_no_slower=bool(fu["us_per_call_median"] <= x["us_per_call_median"] + together)))
    rows += cpu_rows()
    rows.append(dict(note="a call ends in its own stream synchronisation and downloads n_tensors x max_dets records. Rounds alternate the three legs; spread = "
                          "(p95 - p5) / 2 over all calls of a leg. The x_decoder leg reads a tensor decoded beforehand and pays nothing for the decode. One "
                          "machine, one run."))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""yolov8tensordec2 / yoloxtensordec timing: seeded synthetic tensors of the real shapes - V8 84 x 8400 and
X 8400 x 85, about 1 % of the candidates above threshold, clustered so that NMS has work - decoded by
mi355_yolodec_tensors_device as n_tensors = 1, 8, 32 and 256 neighbouring tensors in device memory, each call two launches, one
synchronisation and one download.

  per call     : warm-up, then two stream events around --calls calls (every call ends in its own stream synchronisation, so
                 this is what the streaming thread waits for: launches, kernels, download), and a host clock around the same loop.
  per launch   : a child run of this script under `rocprofv3 --kernel-trace --stats` (a run of its own); the score kernel reads
                 T * F * N * 4 bytes, reported over its mean kernel time as a share of the 8 TB/s peak.
  one CPU core : tools/yolodec_cpu.cpp (the C++ restatement) on the same tensors, compiled here, timed in the same run; "cpu: not
                 measured" when no compiler is found.

  python tools/bench_yolodec.py [--calls K] [--out profiles/yolodec_bench.txt] [--no-profile] [--child-one LAYOUT N_TENSORS]
"""
import argparse
import csv
import ctypes as C
import glob
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

N = 8400
SHAPES = (("V8", 84), ("X", 85))
BATCHES = (1, 8, 32, 256)
PARAMS = (0.36, 0.45, 0.45)
MAX_DETS = 128
PEAK_BYTES_PER_S = 8e12
CHILD_WARM, CHILD_CALLS = 3, 20


def tensor(layout, F, seed):
    """Low class scores, ~1 % of the candidates with one confident class out of five, boxes in twelve clusters."""
    rng = np.random.default_rng(seed)
    n_cls = F - (4 if layout == "V8" else 5)
    scores = rng.random((N, n_cls), dtype=np.float32) * np.float32(0.3)
    hot = rng.random(N) < (0.01 if layout == "V8" else 0.0125)
    cls = rng.integers(0, 5, N)
    scores[hot, cls[hot]] = np.float32(0.5) + rng.random(int(hot.sum()), dtype=np.float32) * np.float32(0.5)
    centres = rng.random((12, 2), dtype=np.float32) * np.float32(600) + np.float32(20)
    xy = centres[rng.integers(0, 12, N)] + (rng.standard_normal((N, 2)) * 6.0).astype(np.float32)
    wh = np.float32(30) + rng.random((N, 2), dtype=np.float32) * np.float32(30)
    cols = [xy, wh]
    if layout == "X":
        cols.append(np.float32(0.2) + rng.random((N, 1), dtype=np.float32) * np.float32(0.8))
    a = np.concatenate(cols + [scores], axis=1).astype(np.float32)
    return np.ascontiguousarray(a.T) if layout == "V8" else np.ascontiguousarray(a)


def tensors(layout, F, T):
    base = [tensor(layout, F, 100 + k) for k in range(min(T, 8))]   # eight distinct tensors, repeated: the device reads T distinct buffers
    return [base[k % len(base)] for k in range(T)]


class Hip:
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


class Batch:
    """T tensors of one shape uploaded side by side, and the arrays of one call"""

    def __init__(self, ctx, layout, F, T):
        self.ctx, self.layout, self.F, self.T = ctx, layout, F, T
        self.host = tensors(layout, F, T)
        self.pitch = F * N * 4
        self.d = ctx.alloc(self.pitch * T)
        for k, t in enumerate(self.host):
            ctx.h2d(self.d + k * self.pitch, t)
        ctx.synchronize()
        self.p = (mi355fx.YoloParams * T)(*[mi355fx.YoloParams(*PARAMS) for _ in range(T)])
        self.dets = np.zeros(T * MAX_DETS, mi355fx.YOLO_DET)
        self.n = (C.c_uint32 * T)()

    def call(self):
        c = self.ctx
        c._ck(c.L.mi355_yolodec_tensors_device(c.h, self.d, self.pitch, self.T, mi355fx.YOLO_LAYOUT[self.layout], self.F, N, self.p, self.dets.ctypes.data,
                                               MAX_DETS, self.n))

    def close(self):
        self.ctx.free(self.d)


def gpu_rows(calls):
    hip = Hip()
    rows = []
    with mi355fx.Context(0) as ctx:
        stream = ctx.L.mi355_ctx_stream(ctx.h)
        for layout, F in SHAPES:
            for T in BATCHES:
                b = Batch(ctx, layout, F, T)
                for _ in range(10):
                    b.call()
                e0, e1 = hip.event(), hip.event()
                t0 = time.perf_counter()
                hip.ck(hip.L.hipEventRecord(e0, stream))
                for _ in range(calls):
                    b.call()
                hip.ck(hip.L.hipEventRecord(e1, stream))
                hip.ck(hip.L.hipEventSynchronize(e1))
                t1 = time.perf_counter()
                ms = C.c_float(0)
                hip.ck(hip.L.hipEventElapsedTime(C.byref(ms), e0, e1))
                hip.L.hipEventDestroy(e0)
                hip.L.hipEventDestroy(e1)
                rows.append(dict(case="gpu", layout=layout, fields=F, candidates=N, n_tensors=T, calls=calls, ms_per_call_events=ms.value / calls,
                                 ms_per_call_host_clock=(t1 - t0) * 1e3 / calls, ms_per_tensor_events=ms.value / calls / T,
                                 detections_first_tensor=int(b.n[0]), detections_mean=float(np.mean(list(b.n))), max_dets=MAX_DETS))
                b.close()
    return rows


def child():
    """what the profiler watches: per shape and batch size CHILD_WARM + CHILD_CALLS calls, in the order of SHAPES x BATCHES"""
    with mi355fx.Context(0) as ctx:
        for layout, F in SHAPES:
            for T in BATCHES:
                b = Batch(ctx, layout, F, T)
                for _ in range(CHILD_WARM + CHILD_CALLS):
                    b.call()
                b.close()


def child_one(layout, T, calls=CHILD_WARM + CHILD_CALLS):
    """one shape and batch size alone: what a counter run (`rocprofv3 --pmc ... -- python tools/bench_yolodec.py --child-one X 256`) watches"""
    with mi355fx.Context(0) as ctx:
        b = Batch(ctx, layout, dict(SHAPES)[layout], T)
        for _ in range(calls):
            b.call()
        b.close()


def profile_rows():
    prof = shutil.which("rocprofv3")
    if not prof:
        return [dict(case="per launch", error="rocprofv3 not found: not measured")]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "y", "--", sys.executable, os.path.abspath(__file__), "--child"],
                           capture_output=True, text=True, timeout=600)
        paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not paths:
            return [dict(case="per launch", error="the profiled child run failed (rc %d): not measured" % r.returncode, stderr=r.stderr[-400:])]
        trace = {"score": [], "nms": []}
        for row in csv.DictReader(open(paths[0])):
            name = row["Kernel_Name"]
            kind = "score" if "yolodec_score_kernel" in name else "nms" if "yolodec_nms_kernel" in name else None
            if kind:
                trace[kind].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    per = CHILD_WARM + CHILD_CALLS
    want = per * len(SHAPES) * len(BATCHES)
    if len(trace["score"]) != want or len(trace["nms"]) != want:
        return [dict(case="per launch", error="expected %d launches of each kernel in the trace, found %d and %d: not measured"
                     % (want, len(trace["score"]), len(trace["nms"])))]
    for k in trace:
        trace[k].sort()
    rows, at = [], 0
    for layout, F in SHAPES:
        for T in BATCHES:
            us = {k: [(e - s) * 1e-3 for s, e in trace[k][at + CHILD_WARM:at + per]] for k in trace}
            at += per
            score_us, nms_us = float(np.mean(us["score"])), float(np.mean(us["nms"]))
            nbytes = T * F * N * 4
            rows.append(dict(case="per launch", layout=layout, n_tensors=T, launches_averaged=CHILD_CALLS, score_kernel_us=score_us, score_kernel_us_min=float(min(us["score"])),
                             nms_kernel_us=nms_us, nms_kernel_us_min=float(min(us["nms"])), score_bytes=nbytes,
                             score_share_of_8TBps_peak=nbytes / (score_us * 1e-6) / PEAK_BYTES_PER_S))
    return rows


def cpu_rows(reps=20):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        return [dict(case="one CPU core", note="cpu: not measured")]
    rows = []
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libyolodec_cpu.so")
        subprocess.check_call([cxx, "-O3", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tools", "yolodec_cpu.cpp"), "-o", so])
        L = C.CDLL(so)
        L.yolodec_cpu.restype = C.c_int
        L.yolodec_cpu.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        for layout, F in SHAPES:
            ts = tensors(layout, F, 8)
            dets = np.zeros(MAX_DETS, mi355fx.YOLO_DET)
            n = C.c_uint32(0)
            times = []
            for r in range(reps + 2):
                t0 = time.perf_counter()
                for t in ts:
                    L.yolodec_cpu(t.ctypes.data, mi355fx.YOLO_LAYOUT[layout], F, N, *PARAMS, dets.ctypes.data, MAX_DETS, C.byref(n))
                times.append((time.perf_counter() - t0) / len(ts))
            times = times[2:]
            rows.append(dict(case="one CPU core", layout=layout, fields=F, candidates=N, ms_per_tensor_mean=float(np.mean(times)) * 1e3,
                             ms_per_tensor_best=float(min(times)) * 1e3, ms_for_256_tensors_mean=float(np.mean(times)) * 1e3 * 256))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls between the two events (at least 200)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolodec_bench.txt"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-one", nargs=2, metavar=("LAYOUT", "N_TENSORS"), help="only the calls of one shape and batch size (for a counter run)")
    a = ap.parse_args()
    if a.child:
        child()
        return
    if a.child_one:
        child_one(a.child_one[0], int(a.child_one[1]))
        return
    rows = gpu_rows(max(a.calls, 200))
    rows += cpu_rows()
    if not a.no_profile:
        rows += profile_rows()
    rows.append(dict(note="a call ends in its own stream synchronisation and downloads n_tensors x max_dets records: ms_per_call is what the streaming "
                          "thread waits for; the lone tensor's figure is launch, synchronisation and copy latency, not kernel time (see the per-launch rows)"))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

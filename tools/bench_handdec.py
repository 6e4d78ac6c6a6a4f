"""handdetectiontensordec / handlandmarktensordec timing: seeded synthetic tensors - palm [2016, 8] and [2944, 8]
(the row counts of the 192 x 192 and 256 x 256 palm models), about 42 % of the rows valid and a confidence threshold of 0.7; landmarks
[2, 63] and [8, 63] with scores - decoded by mi355_handdec_palm_tensors_device / mi355_handdec_landmarks_tensors_device as
n_tensors = 1, 8, 32 and 256 neighbouring tensors in device memory, each call ONE launch, one synchronisation and one download.

  per call     : warm-up, then two stream events around --calls calls (every call ends in its own stream synchronisation, so
                 this is what the streaming thread waits for: launch, kernel, download), and a host clock around the same loop.
  per launch   : a child run of this script under `rocprofv3 --kernel-trace --stats` (a run of its own): kernel times, and THE CHECK
                 that a call is one launch whatever n_tensors is (launches counted in the trace against calls made).
  one CPU core : tools/handdec_cpu.cpp (the C++ restatement) on the same tensors, compiled here, timed in the same run; "cpu: not
                 measured" when no compiler is found.

  python tools/bench_handdec.py [--calls K] [--out profiles/handdec_bench.txt] [--no-profile]
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

SHAPES = (("palm", 2016), ("palm", 2944), ("landmarks", 2), ("landmarks", 8))
BATCHES = (1, 8, 32, 256)
D = 3
PALM_PARAMS = (0.7, 0.08, 2, 192, 192)
LANDMARK_PARAMS = (0.5, 0.2, 2, 640, 360)
CHILD_WARM, CHILD_CALLS = 3, 20


def palm_tensor(N, seed):
    """the synthetic rows of tests/handdec_cases.py: about 42 % valid, uniform scores"""
    rng = np.random.default_rng(seed)
    kp0 = rng.uniform(0.1, 0.9, (N, 2))
    size = rng.uniform(0.03, 0.5, N)
    a = rng.uniform(0, 2 * np.pi, N)
    span = size * rng.uniform(0.1, 1.8, N)
    kp2 = kp0 + span[:, None] * np.stack([np.cos(a), np.sin(a)], axis=1)
    centre = rng.uniform(-0.1, 1.1, (N, 2))
    score = rng.uniform(0, 1, N)
    return np.concatenate([score[:, None], centre, size[:, None], kp0, kp2], axis=1).astype(np.float32)


def landmark_tensor(H, seed):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0, 1, (H, 1, 2)) * np.array((640.0, 360.0))
    pts = np.zeros((H, 21, D))
    pts[:, :, :2] = centre + rng.uniform(20, 120, (H, 1, 1)) * rng.uniform(-0.5, 0.5, (H, 21, 2))
    pts[:, :, 2] = rng.uniform(0, 1, (H, 21))
    return pts.reshape(H, 21 * D).astype(np.float32), rng.uniform(0.4, 1, H).astype(np.float32)


def tensors(kind, rows, T):
    base = [palm_tensor(rows, 100 + k) if kind == "palm" else landmark_tensor(rows, 100 + k) for k in range(min(T, 8))]   # eight distinct, repeated
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

    def __init__(self, ctx, kind, rows, T):
        self.ctx, self.kind, self.rows, self.T = ctx, kind, rows, T
        host = tensors(kind, rows, T)
        self.pitch = (rows * 8 if kind == "palm" else rows * 21 * D) * 4
        self.d = ctx.alloc(self.pitch * T)
        self.ds, self.spitch = None, rows * 4
        if kind == "landmarks":
            self.ds = ctx.alloc(self.spitch * T)
        for k, t in enumerate(host):
            if kind == "palm":
                ctx.h2d(self.d + k * self.pitch, t)
            else:
                ctx.h2d(self.d + k * self.pitch, t[0])
                ctx.h2d(self.ds + k * self.spitch, t[1])
        ctx.synchronize()
        q = PALM_PARAMS if kind == "palm" else LANDMARK_PARAMS
        self.p = (mi355fx.HandParams * T)(*[mi355fx.HandParams(*q) for _ in range(T)])
        self.dets = np.zeros(T * mi355fx.HAND_MAX, mi355fx.HAND_DET)
        self.kps = np.zeros(T * mi355fx.HAND_MAX, mi355fx.HAND_KP)
        self.n = (C.c_uint32 * T)()

    def call(self):
        c = self.ctx
        if self.kind == "palm":
            c._ck(c.L.mi355_handdec_palm_tensors_device(c.h, self.d, self.pitch, self.T, self.rows, self.p, self.dets.ctypes.data, self.n))
        else:
            c._ck(c.L.mi355_handdec_landmarks_tensors_device(c.h, self.d, self.pitch, self.T, self.rows, D, self.ds, self.spitch, self.rows, self.p,
                                                             self.dets.ctypes.data, self.kps.ctypes.data, self.n))

    def close(self):
        self.ctx.free(self.d)
        if self.ds is not None:
            self.ctx.free(self.ds)


def gpu_rows(calls):
    hip = Hip()
    rows = []
    with mi355fx.Context(0) as ctx:
        stream = ctx.L.mi355_ctx_stream(ctx.h)
        for kind, n_rows in SHAPES:
            for T in BATCHES:
                b = Batch(ctx, kind, n_rows, T)
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
                rows.append(dict(case="gpu", decoder=kind, rows=n_rows, n_tensors=T, calls=calls, ms_per_call_events=ms.value / calls,
                                 ms_per_call_host_clock=(t1 - t0) * 1e3 / calls, us_per_tensor_events=ms.value * 1e3 / calls / T,
                                 hands_first_tensor=int(b.n[0]), hands_mean=float(np.mean(list(b.n)))))
                b.close()
    return rows


def child():
    """what the profiler watches: per shape and batch size CHILD_WARM + CHILD_CALLS calls, in the order of SHAPES x BATCHES"""
    with mi355fx.Context(0) as ctx:
        for kind, n_rows in SHAPES:
            for T in BATCHES:
                b = Batch(ctx, kind, n_rows, T)
                for _ in range(CHILD_WARM + CHILD_CALLS):
                    b.call()
                b.close()


def profile_rows():
    prof = shutil.which("rocprofv3")
    if not prof:
        return [dict(case="per launch", error="rocprofv3 not found: not measured")]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "h", "--", sys.executable, os.path.abspath(__file__), "--child"],
                           capture_output=True, text=True, timeout=600)
        paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not paths:
            return [dict(case="per launch", error="the profiled child run failed (rc %d): not measured" % r.returncode, stderr=r.stderr[-400:])]
        trace, others = {"palm": [], "landmarks": []}, {}
        for row in csv.DictReader(open(paths[0])):
            name = row["Kernel_Name"]
            kind = "palm" if "handdec_palm_kernel" in name else "landmarks" if "handdec_landmark_kernel" in name else None
            if kind:
                trace[kind].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
            else:
                others[name[:60]] = others.get(name[:60], 0) + 1   # not the decoders': whatever the runtime itself launches (copies, fills)
    per = CHILD_WARM + CHILD_CALLS
    calls = {k: per * len(BATCHES) * sum(1 for kind, _ in SHAPES if kind == k) for k in trace}
    one = all(len(trace[k]) == calls[k] for k in trace)
    rows = [dict(case="launches per call", calls_palm=calls["palm"], launches_palm=len(trace["palm"]), calls_landmarks=calls["landmarks"],
                 launches_landmarks=len(trace["landmarks"]), other_kernels_in_the_trace=others, one_launch_per_call_whatever_n_tensors=one)]
    if not one:
        return rows
    for k in trace:
        trace[k].sort()
    at = {"palm": 0, "landmarks": 0}
    for kind, n_rows in SHAPES:
        for T in BATCHES:
            us = [(e - s) * 1e-3 for s, e in trace[kind][at[kind] + CHILD_WARM:at[kind] + per]]
            at[kind] += per
            rows.append(dict(case="per launch", decoder=kind, rows=n_rows, n_tensors=T, launches_averaged=CHILD_CALLS, kernel_us=float(np.mean(us)),
                             kernel_us_min=float(min(us))))
    return rows


def cpu_rows(reps=20):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        return [dict(case="one CPU core", note="cpu: not measured")]
    rows = []
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libhanddec_cpu.so")
        subprocess.check_call([cxx, "-O3", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tools", "handdec_cpu.cpp"), "-o", so])
        L = C.CDLL(so)
        L.handdec_palm_cpu.restype = C.c_int
        L.handdec_palm_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.handdec_landmarks_cpu.restype = C.c_int
        L.handdec_landmarks_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        dets, kps = np.zeros(mi355fx.HAND_MAX, mi355fx.HAND_DET), np.zeros(mi355fx.HAND_MAX, mi355fx.HAND_KP)
        n = C.c_uint32(0)
        for kind, n_rows in SHAPES:
            ts = tensors(kind, n_rows, 8)
            times = []
            for r in range(reps + 2):
                t0 = time.perf_counter()
                for t in ts:
                    if kind == "palm":
                        L.handdec_palm_cpu(t.ctypes.data, n_rows, *PALM_PARAMS, dets.ctypes.data, C.byref(n))
                    else:
                        L.handdec_landmarks_cpu(t[0].ctypes.data, n_rows, D, t[1].ctypes.data, n_rows, *LANDMARK_PARAMS, dets.ctypes.data, kps.ctypes.data, C.byref(n))
                times.append((time.perf_counter() - t0) / len(ts))
            times = times[2:]
            rows.append(dict(case="one CPU core", decoder=kind, rows=n_rows, us_per_tensor_mean=float(np.mean(times)) * 1e6, us_per_tensor_best=float(min(times)) * 1e6,
                             ms_for_256_tensors_mean=float(np.mean(times)) * 1e3 * 256))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls between the two events (at least 200)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handdec_bench.txt"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child()
        return
    rows = gpu_rows(max(a.calls, 200))
    rows += cpu_rows()
    if not a.no_profile:
        rows += profile_rows()
    rows.append(dict(note="a call ends in its own stream synchronisation and downloads n_tensors x 10 records: ms_per_call is what the streaming thread waits "
                          "for; the lone tensor's figure is launch, synchronisation and copy latency, not kernel time (see the per-launch rows). The CPU figure "
                          "includes the ctypes call (about a microsecond)"))
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

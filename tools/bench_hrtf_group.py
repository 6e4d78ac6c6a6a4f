"""hrtfrender, one instance per listener: 2, 8 and 32 renderers x 8 sources (256-tap sphere at 48 kHz, block 512 x 8 = 85.3 ms) on native
threads, own context per instance against the hrtf audio group, host and device buffers, the legs alternated inside one process and
repeated (tools/agroup_bench <n> hrtf <repeats>: medians with min / max). Beside them one CPU core running the oracle's restatement
of the crate's algorithm on one renderer - a port, as bench.py's cpu_baseline is, not the reference's binary.
Run on the GPU box: python tools/bench_hrtf_group.py [--members 2 8 32] [--repeats 5] [--out profiles/hrtf_group_bench.txt]
Kernel trace (a run of its own, one thread: 32 members x 100 intervals through the group, then through own contexts):
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o hrtf_group -- python3 tools/bench_hrtf_group.py --trace-leg
  python tools/bench_hrtf_group.py --kernel-stats <dir>   -> profiles/hrtf_group_kernel_stats.csv, launches per interval, the launch set's duration"""
import argparse, csv, glob, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))
sys.path.insert(0, ROOT)
MESH = os.path.join(ROOT, "tests", "golden", "test.hrir")


def cpu_port(seconds=6.0):
    from mi355fx import synth
    from oracle import oracle as O
    rate, steps, bl, sources = 48000, 8, 512, 8
    data = synth.hrir_sphere_bytes(open(MESH, "rb").read(), 256, rate=rate)
    r = O.HrtfRender(O.HrirSphere(data, rate), sources, steps, bl)
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (steps * bl, sources)).astype(np.float32)
    pos = rng.standard_normal((sources, 3)).astype(np.float32)
    gains = np.full(sources, 0.5, np.float32)
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        pos[n % sources, 0] += 0.01
        r.process_block(x, pos, gains)
        n += 1
    dt = (time.perf_counter() - t0) / n
    return {"cpu_port_ms_per_block_one_renderer": dt * 1e3, "cpu_port_realtime_one_core": (steps * bl / rate) / dt,
            "cpu_note": "oracle C restatement of the crate's FFT overlap-save (a port, generic mixed-radix f32 FFT), 1 thread, one renderer of 8 sources"}


def trace_leg(n=32, intervals=100):
    """what the kernel trace is taken of: n group members fed from ONE thread (every member submits, then every member waits: on the
    device exactly the launch sets n element threads produce), then the same blocks through one lone context per member"""
    import mi355fx
    from mi355fx import synth
    rate, steps, bl, sources = 48000, 8, 512, 8
    data = synth.hrir_sphere_bytes(open(MESH, "rb").read(), 256, rate=rate)
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (steps * bl, sources)).astype(np.float32)
    pos = rng.standard_normal((sources, 3)).astype(np.float32)
    gains = np.full(sources, 0.5, np.float32)
    g = mi355fx.AudioGroup("hrtf", n)
    ctxs = []
    for m in range(n):
        g.hrtf_load_sphere(m, data, rate)
        g.hrtf_setup(m, sources, bl, steps)
        c = mi355fx.Context(0)
        c.hrtf_load_sphere(data, rate)
        c.hrtf_setup(sources, bl, steps)
        ctxs.append(c)
    for i in range(intervals):
        pos[i % sources, 0] += 0.01
        for t in [g.submit_hrtf(m, x, pos, gains) for m in range(n)]:
            g.wait(t)
    sets, launches = g.stats()[1], g.hrtf_launches()
    assert launches == 3 * sets == 3 * intervals, (launches, sets)
    for i in range(intervals):
        pos[i % sources, 0] += 0.01
        for c in ctxs:
            c.hrtf_process_block(x, pos, gains)
    print(json.dumps({"trace_leg": "%d members x %d intervals through the group (host buffers, one thread), then through own contexts" % (n, intervals),
                      "agroup_launch_sets": sets, "agroup_kernel_launches": launches, "own_context_kernel_launches": 3 * n * intervals}))
    for c in ctxs:
        c.close()
    g.close()


def kernel_stats(d, out, n=32, intervals=100):
    """the rocprofv3 kernel summary, verbatim; from the trace: launches per interval of either form and the launch set's own duration"""
    stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    trace = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert stats and trace, "no rocprofv3 --kernel-trace --stats output under " + d
    with open(stats[-1]) as f:
        text = f.read()
    with open(out, "w") as f:
        f.write(text)
    names, jobs = {}, []
    with open(trace[-1]) as f:
        for row in csv.DictReader(f):
            k = row.get("Kernel_Name", "").split("(")[0]
            if "hrtf" not in k:
                continue
            names[k] = names.get(k, 0) + 1
            if "_jobs_kernel" in k:
                jobs.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), k))
    jobs.sort()
    group = sum(v for k, v in names.items() if "_jobs_kernel" in k)
    lone = sum(v for k, v in names.items() if "_jobs_kernel" not in k)
    assert group == 3 * intervals and lone == 3 * n * intervals, names   # three launches per interval instead of three per member
    spans = sorted(jobs[i + 2][1] - jobs[i][0] for i in range(0, len(jobs), 3))
    busy = sorted(sum(e - s for s, e, _ in jobs[i:i + 3]) for i in range(0, len(jobs), 3))
    print(json.dumps({"hrtf_kernel_launches_in_trace": names, "agroup_launches_per_interval": group / intervals, "own_context_launches_per_interval": lone / intervals,
                      "launch_set_first_start_to_last_end_us": {"median": spans[len(spans) // 2] / 1e3, "min": spans[0] / 1e3, "max": spans[-1] / 1e3},
                      "launch_set_kernel_time_us_median": busy[len(busy) // 2] / 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="*", default=[2, 8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hrtf_group_bench.txt"))
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "hrtf_group_kernel_stats.csv"))
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --stats run of tools/agroup_bench <n> hrtf")
    ap.add_argument("--trace-leg", action="store_true", help="the single-threaded leg a rocprofv3 --kernel-trace --stats run is taken of")
    a = ap.parse_args()
    if a.trace_leg:
        trace_leg()
        return
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.stats_out)
        return
    tool = os.path.join(ROOT, "tools", "agroup_bench")
    lines = ["# python tools/bench_hrtf_group.py --members %s --repeats %d" % (" ".join(map(str, a.members)), a.repeats)]
    for n in a.members:
        r = subprocess.run([tool, str(n), "hrtf", str(a.repeats), MESH], capture_output=True, text=True, timeout=240)
        if r.returncode != 0:   # a leg that failed ends the run: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode if r.returncode > 0 else 1)
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                d = json.loads(l)
                assert d["agroup_kernel_launches"] == 3 * d["agroup_launch_sets"]   # uniform members: three launches per launch set
                lines.append(l)
                print(l, flush=True)
    if not a.no_cpu:
        l = json.dumps(cpu_port())
        lines.append(l)
        print(l, flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Guard for the host dispatch of csrc/colorlut_kernels.hip: the kernel that serves every case of tests/colorlut_route_cases.py and the
CRC-32 of what it leaves in the destination buffer, written at the commit BEFORE the dispatch was restated as a list of routes;
tests/test_gpu_colorlut_routes.py asserts that the tree under test still takes the same routes to the same bytes.
The cases are recorded twice (--recordings N: more often), each time in a fresh process. A case whose name or CRC differs between
recordings does not go into the file and is listed under "dropped"; that is refused for a case with a pinned variant
(LUT_VARIANT != 0), for the group case and for every launch of an auto sequence but its fourth measured one. (The names of
colorlut_route_cases.MEASURED_CASES are not compared, here or in the test: see there.)
Run on the GPU box: python tools/record_colorlut_routes.py --commit <hash of the commit the library was built from> [--out FILE]"""
import argparse, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import colorlut_route_cases as RC


def may_drop(name):
    head = name.split("/", 1)[0]
    if head in RC.LUTS:
        return "/v0/" in name
    return head == "auto" and name.endswith("/auto4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit")
    ap.add_argument("--out", default=RC.GOLDEN)
    ap.add_argument("--recordings", type=int, default=2)
    ap.add_argument("--raw", help="one recording, unmerged, into this file (what the child processes run)")
    a = ap.parse_args()
    if a.raw:
        import mi355fx
        with open(a.raw, "w") as f:
            json.dump(RC.run_all(mi355fx), f)
        return
    if not a.commit:
        ap.error("--commit is required")
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(max(a.recordings, 2)):
            path = os.path.join(tmp, "rec%d.json" % i)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--raw", path])
            with open(path) as f:
                recs.append(json.load(f))
    assert all(r.keys() == recs[0].keys() for r in recs)
    dropped = sorted(n for n in recs[0] if any(r[n] != recs[0][n] for r in recs))
    for n in dropped:
        print("differs:", n, [r[n] for r in recs], flush=True)
    refused = [n for n in dropped if not may_drop(n)]
    if refused:
        sys.exit("the recordings differ in %d cases that may not be dropped: %s" % (len(refused), refused[:10]))
    kept = {n: v for n, v in recs[0].items() if n not in dropped}
    missing = [k for k in RC.KERNEL_NAMES if k not in RC.NOT_COVERED and k not in {v[0] for v in kept.values()}]
    if missing:
        sys.exit("kernel names no case reaches: %s" % missing)
    doc = {"commit": a.commit, "what": "per case [index into kernels, index into crcs]: Context.colorlut_kernel_name() after the launch, zlib.crc32 of the whole destination buffer",
           "dropped": dropped, "recordings": len(recs)}
    doc.update(RC.pack(kept))
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(doc.items())) + "\n}\n")
    print("%d recordings: %d cases, %d dropped, %d kernel names" % (len(recs), len(kept), len(dropped), len(doc["kernels"])))


if __name__ == "__main__":
    main()

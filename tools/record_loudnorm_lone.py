"""Guard for the bits of a single audioloudnorm context: SHA-256 of the input and of the concatenated loudnorm_push / loudnorm_drain
output of every stream of tests/loudnorm_streams.py. Written once, at the commit BEFORE the single context became a batch of one (it
ran a host-driven implementation of the limiter of its own until then); tests/test_gpu_loudnorm.py asserts the hashes still hold.
Run on the GPU box: python tools/record_loudnorm_lone.py --commit <hash of the commit the library was built from> [--out FILE]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mi355fx
import loudnorm_cases as LC
import loudnorm_streams as LS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=LS.GOLDEN)
    a = ap.parse_args()
    doc = {"commit": a.commit, "what": "hashlib.sha256 of the f64 input bytes / of the concatenated f64 output bytes of a single context", "streams": {}}
    for s in LS.streams():
        x = s.make()
        with mi355fx.Context(0) as ctx:
            got = LS.run_lone(ctx, s, x)
        assert got.size == x.size, (s.name, got.size, x.size)
        doc["streams"][s.name] = {"chunk": s.chunk, "input_sha256": LS.sha(x), "output_sha256": LS.sha(got)}
        print(s.name, doc["streams"][s.name]["output_sha256"][:16], flush=True)
        if s.name.startswith("case/"):
            LC.get(s.name[5:]).release()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

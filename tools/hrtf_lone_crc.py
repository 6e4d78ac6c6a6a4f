"""Guard for the bits of hrtfrender's lone-context path: CRC-32 of three seeded output blocks (and of the last mesh lookup) for every
member shape of tests/hrtf_group_cases.py, through entry points a lone Context has always had. Written once, at the commit BEFORE the
kernels' bodies were shared with the group form; tests/test_gpu_agroup_hrtf.py asserts the lone path still produces them.
--extend adds the file's "extra" section and leaves the rest as it is: a reset after the first block and the device entry point
(hrtf_group_cases.lone_extra_crcs over extra_members()). Written once as well, at the commit before the two elements' shared helpers (the transform in LDS, the
status helpers) moved to csrc/audio_fft.hpp.
Run on the GPU box: python tools/hrtf_lone_crc.py --commit <hash of the commit the library was built from> [--extend] [--out FILE]
(MI355FX_LIB selects the library build)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mi355fx
from mi355fx import synth
import hrtf_group_cases as H


def extend(a):
    with open(a.out) as f:
        doc = json.load(f)
    doc["extra"] = {"commit": a.commit, "blocks": H.GUARD_BLOCKS, "what": "as above over hrtf_group_cases.lone_extra_crcs", "shapes": {}}
    for m in H.extra_members():
        doc["extra"]["shapes"][m["key"]] = H.lone_extra_crcs(mi355fx, synth, m)
        assert doc["extra"]["shapes"][m["key"]]["transform"] == m["transform"], m
        print(m["key"], doc["extra"]["shapes"][m["key"]])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=H.CRC_FIXTURE)
    ap.add_argument("--extend", action="store_true", help="keep the file's entries and write its \"extra\" section only")
    a = ap.parse_args()
    if a.extend:
        return extend(a)
    doc = {"commit": a.commit, "blocks": H.GUARD_BLOCKS, "what": "zlib.crc32 of the f32 output blocks / i32 faces / f32 weights of a lone context",
           "shapes": {}}
    for m in H.members():
        doc["shapes"][m["key"]] = H.lone_crcs(mi355fx, synth, m)
        assert doc["shapes"][m["key"]]["transform"] == m["transform"], m
        print(m["key"], doc["shapes"][m["key"]])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

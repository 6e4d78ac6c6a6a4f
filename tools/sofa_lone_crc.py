"""Guard for the bits of sofalizer's lone-context path: CRC-32 of every seeded output block (one filter replaced half way) for every
member shape of tests/sofa_group_cases.py and every shape of audio_state_cases.SOFA_NEW_SHAPES, through entry points a lone Context
has always had. Written once, at the commit BEFORE the kernels' bodies were shared with the job-table form;
tests/test_gpu_agroup_sofa.py asserts the lone path still produces them.
--extend adds the file's "extra" section and leaves the rest as it is: a reset with a filter set behind it, two set_filter calls on
one channel before the first block, and the device entry point (sofa_group_cases.lone_reset_outputs / lone_device_outputs). Written once as well, at the commit before the two elements' shared helpers (the transform in LDS, the
status helpers) moved to csrc/audio_fft.hpp.
Run on the GPU box: python tools/sofa_lone_crc.py --commit <hash of the commit the library was built from> [--extend] [--out FILE]
(MI355FX_LIB selects the library build)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mi355fx
import sofa_group_cases as S


def extend(a):
    with open(a.out) as f:
        doc = json.load(f)
    doc["extra"] = {"commit": a.commit, "what": "as above over sofa_group_cases.lone_reset_outputs / lone_device_outputs", "shapes": {}}
    for shape in S.EXTRA_SHAPES:
        doc["extra"]["shapes"][S.key(shape)] = S.lone_extra_crcs(mi355fx, shape)
        print(S.key(shape), doc["extra"]["shapes"][S.key(shape)])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=S.CRC_FIXTURE)
    ap.add_argument("--extend", action="store_true", help="keep the file's entries and write its \"extra\" section only")
    a = ap.parse_args()
    if a.extend:
        return extend(a)
    doc = {"commit": a.commit, "what": "zlib.crc32 of the f32 [B][2] output blocks of a lone context over sofa_group_cases.schedule(shape)",
           "shapes": {}}
    for shape in S.guard_shapes():
        doc["shapes"][S.key(shape)] = S.lone_crcs(mi355fx, shape)
        print(S.key(shape), doc["shapes"][S.key(shape)])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

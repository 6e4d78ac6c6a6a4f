"""Guard for the bits of sofalizer's lone-context path: CRC-32 of every seeded output block (one filter replaced half way) for every
member shape of tests/sofa_group_cases.py and every shape of audio_state_cases.SOFA_NEW_SHAPES, through entry points a lone Context
has always had. Written once, at the commit BEFORE the kernels' bodies were shared with the job-table form;
tests/test_gpu_agroup_sofa.py asserts the lone path still produces them.
Run on the GPU box: python tools/sofa_lone_crc.py --commit <hash of the commit the library was built from> [--out FILE]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gst-plugins-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mi355fx
import sofa_group_cases as S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=S.CRC_FIXTURE)
    a = ap.parse_args()
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

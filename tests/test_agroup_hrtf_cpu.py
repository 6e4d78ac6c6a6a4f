"""CPU companion of tests/test_gpu_agroup_hrtf.py: the member shapes against the rule that picks the convolution form, the
lone-path guard fixture, and the surfaces (header, shim, bindings) the hrtf group kind adds."""
import json
import os
import re

import audio_state_cases as A
import hrtf_group_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_agroup_create_hrtf", "mi355_agroup_shared_hrtf", "mi355_agroup_hrtf_load_sphere", "mi355_agroup_hrtf_setup", "mi355_agroup_hrtf_reset",
             "mi355_agroup_submit_hrtf", "mi355_agroup_hrtf_info", "mi355_agroup_hrtf_last_lookup"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_shapes_table_matches_the_form_rule():
    table = [(256, 8, 8, 512, 0, 0), (512, 4, 2, 1500, 0, 2048), (400, 2, 8, 512, 0, 1024), (1, 1, 8, 512, 0, 0), (2049, 2, 2, 2048, 0, 4096),
             (2050, 2, 2, 2048, 0, 0), (128, 64, 8, 512, 1, 1024), (100, 3, 4, 77, 2, 0)]
    assert H.SHAPES == table
    for (length, channels, steps, block, method, n) in H.SHAPES:
        assert 1 <= channels <= 64 and 1 <= steps <= 64
        assert A.hrtf_expected_transform(length, block, method) == n, (length, block, method)
    assert 2050 - 1 + 2048 == 4097   # one point above the ceiling of the transform
    r = H.RESAMPLED
    assert r["len"] == int(r["file_len"] * r["rate"] / r["file_rate"] + 0.5) == 218
    assert A.hrtf_expected_transform(r["len"], r["block"], r["method"]) == r["transform"]
    ms = H.members()
    assert len(ms) == 9 and len({m["key"] for m in ms}) == 9
    # both forms and three transform sizes in one set
    assert sorted({m["transform"] for m in ms}) == [0, 1024, 2048, 4096]


def test_streams_are_seeded_and_move():
    m = H.members()[0]
    a, b = H.stream(m, 3), H.stream(m, 3)
    for (x0, p0, g0), (x1, p1, g1) in zip(a, b):
        assert (x0 == x1).all() and (p0 == p1).all() and (g0 == g1).all()
        assert x0.shape == (m["steps"] * m["block"], m["channels"]) and p0.shape == (m["channels"], 3)
    assert not (a[0][1] == a[1][1]).all()            # moving sources
    assert not (H.stream(m, 1, seed=1)[0][0] == a[0][0]).all()


def test_guard_fixture_names_a_commit_and_covers_every_shape():
    with open(H.CRC_FIXTURE) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{40}", doc["commit"])
    assert doc["blocks"] == H.GUARD_BLOCKS == 3
    assert set(doc["shapes"]) == {m["key"] for m in H.members()}
    for m in H.members():
        e = doc["shapes"][m["key"]]
        assert e["transform"] == m["transform"]
        assert len(e["out"]) == 3 and len(set(e["out"])) == 3
        for c in e["out"] + [e["faces"], e["uvw"]]:
            assert re.fullmatch(r"[0-9a-f]{8}", c)
    # the "extra" section: a reset after the first block and the device entry point, recorded at a later commit than the rest
    extra = doc["extra"]
    assert re.fullmatch(r"[0-9a-f]{40}", extra["commit"]) and extra["commit"] != doc["commit"] and extra["blocks"] == H.GUARD_BLOCKS
    ms = H.extra_members()
    assert [m["key"] for m in ms] == ["L1_C1_S8_B512_m1", "L1_C1_S8_B512_m2", "L400_C2_S8_B512_m0", "L100_C3_S4_B77_m2"]
    assert set(extra["shapes"]) == {m["key"] for m in ms}
    smallest = min(H.members(), key=lambda m: (m["len"], m["channels"]))
    for m in ms[:2]:                                                     # the smallest member, once per form
        assert {k: m[k] for k in m if k not in ("key", "method", "transform")} == {k: smallest[k] for k in smallest if k not in ("key", "method", "transform")}
    assert [(m["method"], m["transform"]) for m in ms[:2]] == [(1, 512), (2, 0)]
    for m in ms:
        e = extra["shapes"][m["key"]]
        assert e["transform"] == m["transform"] == A.hrtf_expected_transform(m["len"], m["block"], m["method"])
        for run in (e["reset"], e["device"]):
            assert len(run) == H.GUARD_BLOCKS and len(set(run)) == len(run)
        for c in e["reset"] + e["device"] + [e["faces"], e["uvw"]]:
            assert re.fullmatch(r"[0-9a-f]{8}", c)
        assert e["reset"][0] == e["device"][0] and e["reset"][2] == e["device"][2]   # a reset clears tails: heard in the block behind it alone
        assert (e["reset"][1] != e["device"][1]) == (m["len"] > 1)                 # ... when the HRIR has a tail at all
        if m["key"] in doc["shapes"]:
            base = doc["shapes"][m["key"]]
            assert e["device"] == base["out"] and (e["faces"], e["uvw"]) == (base["faces"], base["uvw"])


def test_header_declares_the_new_names():
    h = _read("include", "mi355fx.h")
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, h), name
    assert "audio/hrtf/src/hrtf/imp.rs" in h[h.index("hrtfrender through an audio group"):h.index("mi355_agroup_create_hrtf(")]


def test_shim_takes_a_member_of_the_shared_group():
    c = _read("gst", "gsthrtfrender.c")
    for call in ("mi355_agroup_shared_hrtf(", "mi355_agroup_hrtf_load_sphere(", "mi355_agroup_hrtf_setup(", "mi355_agroup_submit_hrtf(", "mi355_agroup_wait(",
                 "mi355_agroup_hrtf_reset(", "mi355_agroup_release("):
        assert call in c, call
    assert 'g_getenv("MI355_GROUP_MEMBERS")' in c
    # without the variable nothing changes: the lone calls stay
    for call in ("mi355_hrtf_load_sphere(", "mi355_hrtf_setup(", "mi355_hrtf_process_block(", "mi355_hrtf_reset(", "mi355_hrtf_teardown("):
        assert call in c, call


def test_bindings_and_documents_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    doc = _read("INTEGRATION.md")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        assert name in doc, name
    for method in ("hrtf_load_sphere", "hrtf_setup", "hrtf_reset", "submit_hrtf", "hrtf_info", "hrtf_last_lookup"):
        assert re.search(r"    def %s\(self, member" % method, py), method
    assert "KIND_HRTF" in _read("gst-plugins-rs_amd", "csrc", "agroup.hip")
    assert "hrtf" in _read("tools", "agroup_bench.cpp")

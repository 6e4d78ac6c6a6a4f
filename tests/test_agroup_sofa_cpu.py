"""CPU companion of tests/test_gpu_agroup_sofa.py: the member shapes, the lone-path guard fixture, and the surfaces (library exports,
header, bindings, documents) the sofa group kind adds."""
import ctypes
import json
import os
import re

import audio_state_cases as A
import sofa_group_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_agroup_create_sofa", "mi355_agroup_shared_sofa", "mi355_agroup_sofa_setup", "mi355_agroup_sofa_set_filter", "mi355_agroup_sofa_set_drop",
             "mi355_agroup_sofa_reset", "mi355_agroup_submit_sofa", "mi355_agroup_sofa_info", "mi355_agroup_sofa_launches"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_shapes_table_is_the_one_the_group_test_names():
    table = [(2, 20, 8, 8), (1, 33, 16, 64), (3, 64, 64, 64), (2, 17, 16, 48), (6, 128, 64, 256), (64, 40, 16, 32), (2, 200, 64, 256), (1, 3000, 2048, 2048)]
    assert S.SHAPES == table
    assert S.DROPS == {(6, 128, 64, 256): (3,)}
    for (C, L, P, B) in S.SHAPES:
        assert 1 <= C <= 64 and B % P == 0 and P & (P - 1) == 0 and 8 <= P <= 2048
    assert sorted({s[2] for s in S.SHAPES}) == [8, 16, 64, 2048]        # four convolution launches per set
    assert [S.partitions(s) for s in S.SHAPES] == [3, 3, 1, 2, 2, 3, 4, 2]
    assert (3 * 4096 + 2048) * 8 == 112 * 1024                           # the LDS of a P = 2048 workgroup
    for s in S.guard_shapes():
        assert S.n_blocks(s) * (s[3] // s[2]) >= 2 * S.partitions(s) + 1, s
    assert S.expected_launches(S.SHAPES, range(8)) == 9 and S.expected_launches(S.SHAPES, []) == 5
    assert S.expected_launches([(2, 128, 64, 256)] * 4, []) == 2 and S.expected_launches([(2, 128, 64, 256)] * 4, [1]) == 3


def test_schedules_are_seeded_and_replace_one_filter_half_way():
    shape = (6, 128, 64, 256)
    a, b = S.schedule(shape), S.schedule(shape)
    assert a["drops"] == (3,) and [f[0] for f in a["filters"]] == [0, 1, 2, 4, 5]
    for (x0, g0, c0), (x1, g1, c1) in zip(a["blocks"], b["blocks"]):
        assert (x0 == x1).all() and (g0 == g1).all() and len(c0) == len(c1)
        assert x0.shape == (256, 6) and (x0[:, 3] == 100.0).all()
    assert [len(c) for (_, _, c) in a["blocks"]] == [0, 0, 1, 0]
    assert a["blocks"][2][2][0][0] == 5                                  # the last channel that is not dropped
    assert not (a["blocks"][0][1] == a["blocks"][1][1]).all()            # gains move with every block
    assert not (S.schedule(shape, seed=1)["blocks"][0][0] == a["blocks"][0][0]).all()


def test_guard_fixture_names_a_commit_and_covers_every_shape():
    with open(S.CRC_FIXTURE) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{40}", doc["commit"])
    shapes = S.guard_shapes()
    assert len(shapes) == 17 and set(S.SHAPES) <= set(shapes) and set(A.SOFA_NEW_SHAPES) <= set(shapes)
    assert set(doc["shapes"]) == {S.key(s) for s in shapes}
    for s in shapes:
        e = doc["shapes"][S.key(s)]
        assert len(e) == S.n_blocks(s) and len(set(e)) == len(e), s
        for c in e:
            assert re.fullmatch(r"[0-9a-f]{8}", c)
    # the "extra" section: the reset / double set_filter run and the device entry point, recorded at a later commit than the rest
    extra = doc["extra"]
    assert re.fullmatch(r"[0-9a-f]{40}", extra["commit"]) and extra["commit"] != doc["commit"]
    assert S.EXTRA_SHAPES == [(2, 20, 8, 8), (2, 17, 16, 48), (6, 128, 64, 256)] and set(S.EXTRA_SHAPES) <= set(shapes)
    assert set(extra["shapes"]) == {S.key(s) for s in S.EXTRA_SHAPES}
    for s in S.EXTRA_SHAPES:
        e, base = extra["shapes"][S.key(s)], doc["shapes"][S.key(s)]
        assert sorted(e) == ["device", "reset"], s
        for run in e.values():
            assert len(run) == S.n_blocks(s) >= 4 and len(set(run)) == len(run), s
            assert all(re.fullmatch(r"[0-9a-f]{8}", c) for c in run)
        assert e["device"] == base, s                                  # the device entry point computes what the host one does
        assert e["reset"][:2] == base[:2], s                           # of two filters set before the first block only the last counts
        assert not set(e["reset"][2:]) & set(base), s                  # ... and the reset and the filter behind it are heard


def test_library_exports_the_new_names():
    lib = ctypes.CDLL(os.path.join(ROOT, "gst-plugins-rs_amd", "libmi355fx.so"))
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
    lib.mi355_abi_version.restype = ctypes.c_int
    assert lib.mi355_abi_version() == 1


def test_header_declares_the_new_names():
    h = _read("include", "mi355fx.h")
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, h), name
    block = h[h.index("sofalizer through an audio group"):h.index("mi355_agroup_create_sofa(int")]
    assert "audio/hrtf/src/sofa/imp.rs" in block
    for name in NEW_NAMES:
        assert name.replace("mi355_agroup_shared_sofa", "_shared_sofa") in block, name
    assert re.search(r"#define MI355FX_ABI_VERSION\s+1\b", h)


def test_bindings_and_documents_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    doc = _read("INTEGRATION.md")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        assert name in doc, name
    for method in ("sofa_setup", "sofa_set_filter", "sofa_set_drop", "sofa_reset", "submit_sofa", "sofa_output", "sofa_info"):
        assert re.search(r"    def %s\(self, member" % method, py), method
    assert re.search(r"    def sofa_launches\(self\)", py)
    assert 'kind == "sofa"' in py
    assert "KIND_SOFA" in _read("gst-plugins-rs_amd", "csrc", "agroup.hip")
    assert "SofaGroup" in _read("gst-plugins-rs_amd", "csrc", "internal.hpp")
    assert "mi355_agroup_submit_sofa(" in _read("tools", "agroup_bench.cpp")

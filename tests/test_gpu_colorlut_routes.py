"""The host dispatch of csrc/colorlut_kernels.hip against the route table recorded at the commit before it was restated
(tests/golden/colorlut_routes_parent.json, tools/record_colorlut_routes.py): every case of tests/colorlut_route_cases.py is served by
the kernel of the same name and leaves the same bytes in the whole destination buffer (CRC-32; the buffer is prefilled, so padding
and unwritten bytes count). A case the parent recordings disagreed on is not in the file and is not compared; of the six launches
of colorlut_route_cases.MEASURED_CASES only the bytes are compared (their name is a measured choice in any build)."""
import json

import pytest

import colorlut_route_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(RC.GOLDEN) as f:
        doc = json.load(f)
    return doc, RC.unpack(doc)


def _compare(got, golden):
    doc, exp = golden
    got = RC.normalise(got)
    bad = [(n, v, exp[n]) for n, v in got.items() if n in exp and v != exp[n]]
    unknown = [n for n in got if n not in exp and n not in doc["dropped"]]
    assert not unknown, "cases the golden does not know: %s" % unknown[:5]
    assert not bad, "%d of %d cases differ from the parent's route table (name, got, parent): %s" % (len(bad), len(got), bad[:8])


@pytest.mark.parametrize("lut", RC.LUTS)
def test_product_routes(mi355lib, golden, lut):
    """Entry and format x LUT_VARIANT 0-9 x BRICK_SETS x the seven geometries, then FUSED_VARIANT 1 and FORCE_GENERIC 1 over the same
    at BRICK_SETS 0: 1960 launches of a few KB on one context."""
    import mi355fx
    got = RC.run_product(mi355fx, lut)
    assert len(got) == len(RC.product_cases())
    _compare(got, golden)


def test_auto_sequences(mi355lib, golden):
    """The measured choice from a fresh context, launch by launch: colorlut and the fused entry on a 33^3 and a 1D LUT, hsvfilter
    under MI355_FLAG_HSV_TABLE 1 and 2; at the floor of 16384 pixel groups and just below it."""
    import mi355fx
    _compare(RC.run_auto(mi355fx), golden)


def test_group_route(mi355lib, golden):
    import mi355fx
    _compare(RC.run_group(mi355fx), golden)


def test_golden_covers_every_kernel_name(golden):
    """Every name the dispatch can report occurs in the golden, but for the two kernels that need launches of megapixels."""
    doc, exp = golden
    seen = {v[0] for v in exp.values()}
    assert sorted(set(RC.KERNEL_NAMES) - seen) == sorted(RC.NOT_COVERED)
    assert all(n.split("/", 1)[0] in RC.LUTS and "/v0/" in n or n.endswith("/auto4") for n in doc["dropped"]), doc["dropped"]

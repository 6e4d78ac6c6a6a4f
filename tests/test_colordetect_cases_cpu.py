"""The claims of tests/colordetect_cases.py, proved without a GPU: every case reaches the labels it names (the traced restatement,
the model of cut_box's work split, the model of the histogram kernel's waves), the claims cover the label table but for the labels
proved unreachable, the models tile what they must, and one-token mutants of the restatement are caught by the cases that claim
the mutated decision."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest

import colordetect_cases as K
import colordetect_restate as R


# ------------------------------------------------------------------------------------------------ palette cases

@pytest.mark.parametrize("case", K.PALETTE_CASES + K.LARGE_CASES, ids=lambda c: c.name)
def test_palette_case_reaches_what_it_claims(case):
    pal, trace, boxes = case.traced()
    assert pal == case.expected() == R.palette_from_histogram(case.bins(), case.box, case.max_colors)   # the trace changes nothing
    reached = case.reached()
    assert set(case.claims) <= reached, sorted(set(case.claims) - reached)
    assert set(case.claims) <= set(K.ALL_LABELS) and not reached & set(K.EXEMPT)
    assert set(trace) <= set(R.LABELS) | set(K.AXIS_LABELS)
    assert len(pal) <= case.max_colors and (case.samples == 0) == (pal == [])


def test_claims_cover_the_label_table():
    claimed = set(itertools.chain.from_iterable(c.claims for c in K.PALETTE_CASES))
    assert claimed | set(K.EXEMPT) == set(K.ALL_LABELS), sorted(set(K.ALL_LABELS) - claimed - set(K.EXEMPT))
    assert not claimed & set(K.EXEMPT) and set(K.EXEMPT) <= set(R.LABELS)
    # cases built for a cut or queue label stay small; only the filled boxes and the n = 255 pair are more than a few samples
    for c in K.PALETTE_CASES:
        assert c.samples <= K.FRAME_SAMPLES_MAX or c.name.startswith("dense_"), c.name
    assert {c.name for c in K.PALETTE_CASES} - {c.name for c in K.FRAME_CASES} == {c.name for c in K.PALETTE_CASES if c.name.startswith("dense_")}


def test_moving_a_claim_to_another_case_fails():
    """The stall label belongs to the cases built for it: no other small case reaches it."""
    label = "B.count1_top_cuttable_below"
    owners = [c.name for c in K.PALETTE_CASES if label in c.claims]
    reachers = [c.name for c in K.PALETTE_CASES if label in c.reached()]
    assert owners and set(owners) <= set(reachers)
    other = next(c for c in K.PALETTE_CASES if c.name == "one_bin_twice")
    assert label not in other.reached()


def test_axis_labels_are_the_reachable_ones():
    """Every width triple 1..32 gives one of the derived labels, and each label occurs."""
    seen = set()
    for w in itertools.product(range(1, 33), repeat=3):
        axis = K.cut_axis(w)
        assert w[axis] == max(w) and all(w[a] < w[axis] for a in range(axis))      # the first of the widest
        seen.add("cut.axis.%s/%s" % ("rgb"[axis], "".join(c for c, x in zip("rgb", w) if x == max(w))))
    assert sorted(seen) == K.AXIS_LABELS and len(K.AXIS_LABELS) == 7


def test_exempt_labels_never_occur_in_an_exhaustive_sweep():
    """Every histogram of at most 3 samples on a 3 x 3 x 3 sub-lattice of bins, max_colors 2..6. A round either cuts (at most
    max_colors - 1 of them in all) or pops a box of count 1 and pushes it back, which leaves the queue as it was: every later round
    of that phase repeats it. So a copy of the restatement with 20 rounds instead of 1000 takes the same decisions, and the sweep
    runs on that copy; every 40th histogram is run at 1000 rounds as well and must give the same labels and the same palette."""
    short = _mutant("MAX_ITERATIONS = 1000\n", "MAX_ITERATIONS = 20\n")
    lattice = list(itertools.product((0, 13, 31), repeat=3))
    hists = set()
    for n in (1, 2, 3):
        for combo in itertools.combinations_with_replacement(range(27), n):
            hists.add(tuple(sorted((k, combo.count(k)) for k in set(combo))))
    assert len(hists) == 27 + 378 + 3654
    seen = set()
    for k, h in enumerate(sorted(hists)):
        case = K.PaletteCase("sweep", {lattice[b]: c for b, c in h}, 2, [])
        bins = case.bins()
        for mc in range(2, 7):
            t = K.Trace()
            pal = short.palette_from_histogram(bins, case.box, mc, t)
            seen |= set(t)
            if k % 40 == 0:
                full = K.Trace()
                assert R.palette_from_histogram(bins, case.box, mc, full) == pal and set(full) == set(t)
    assert not seen & set(K.EXEMPT), sorted(seen & set(K.EXEMPT))
    assert seen <= set(K.ALL_LABELS)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_as_frame_round_trip(fmt):
    for case in K.FRAME_CASES:
        for q in (1, 2, 10):
            hist, box = R.histogram(case.as_frame(fmt, q), fmt, q)
            assert np.array_equal(hist, case.bins()) and box == case.box, (case.name, q)
            assert R.get_palette(case.as_frame(fmt, q), fmt, q, case.max_colors) == case.expected()


def test_large_counts_are_what_the_issue_names():
    sums = sorted({c.samples for c in K.LARGE_CASES})
    assert sums == [2 ** 32 - 2, 2 ** 32 - 1] and {c.max_colors for c in K.LARGE_CASES} == {2, 8} and len(K.LARGE_CASES) == 6
    for c in K.LARGE_CASES:
        assert max(c.hist.values()) >= 2 ** 31 - 1 and int(c.bins().astype(np.uint64).sum()) == c.samples


# ------------------------------------------------------------------------------------------------ the split model

def test_split_tiles_every_box_of_every_case():
    for case in K.PALETTE_CASES + K.LARGE_CASES:
        for lo, hi in case.traced()[2]:
            want = sorted((r << 10) | (g << 5) | b for r in range(lo[0], hi[0] + 1) for g in range(lo[1], hi[1] + 1) for b in range(lo[2], hi[2] + 1))
            assert sorted(K.split_bins(lo, hi)) == want, (case.name, lo, hi)


def test_split_tiles_all_width_triples():
    """Items cover (slice, part) once each in wave order; a slice's parts tile its rows; lane trips tile a part's bins."""
    for w3 in itertools.product(range(1, 33), repeat=3):
        sp = K.split(w3)
        axis, parts = sp["axis"], sp["parts"]
        w, n1, n2 = w3[axis], w3[sp["a1"]], w3[sp["a2"]]
        assert parts == {1: 8, 2: 4, 3: 2, 4: 2}.get(w, 1)
        assert sorted(s * parts + p for _, _, s, p, *_ in sp["items"]) == list(range(w * parts))
        rows = {}
        for wave, trip, s, part, r_beg, r_end, c, lane_trips in sp["items"]:
            assert (s * parts + part) == wave + 8 * trip and c == n2 and 0 <= r_beg <= r_end <= n1
            assert 64 * (lane_trips - 1) < (r_end - r_beg) * n2 <= 64 * lane_trips or (r_end == r_beg and lane_trips == 0)
            rows.setdefault(s, []).append((r_beg, r_end))
        for s, rr in rows.items():
            rr.sort()
            assert rr[0][0] == 0 and rr[-1][1] == n1 and all(a[1] == b[0] for a, b in zip(rr, rr[1:])), (w3, s)
    labels = set().union(*(K.split(w3)["labels"] for w3 in ((1, 1, 1), (2, 1, 1), (3, 3, 3), (3, 32, 32), (7, 5, 1), (8, 8, 8), (9, 1, 1), (32, 32, 32))))
    assert labels == set(K.SPLIT_LABELS)
    assert "split.part_over_64_bins" not in K.split((8, 8, 8))["labels"] and "split.wave_second_trip" not in K.split((8, 8, 8))["labels"]


# ------------------------------------------------------------------------------------------------ mutants of the restatement

MUTANTS = {
    # name: (old text, new text, labels whose claimants must notice)
    "axis_tie": ("axis = 0 if widths[0] >= widths[1] and widths[0] >= widths[2] else (1 if widths[1] >= widths[2] else 2)",
                 "axis = 0 if widths[0] > widths[1] and widths[0] > widths[2] else (1 if widths[1] > widths[2] else 2)",
                 ["cut.axis.r/rg", "cut.axis.r/rb", "cut.axis.r/rgb", "cut.axis.g/gb"]),
    "left_lt_right": ("if left <= right else max(", "if left < right else max(", ["cut.median.left_le_right"]),
    "right_half_up": ("i + right // 2) if", "i + (right + 1) // 2) if", ["cut.median.min_unclipped"]),
    "sort_reversed_stable": ("    q.sort(key=key) ", "    q.reverse(); q.sort(key=key) ", ["A.equal_keys_on_top", "B.equal_keys_on_top"]),
    "three_quarters": ("0.75 * max_colors", "0.76 * max_colors", ["A.target_met_after_cut"]),
    "half_inclusive": ("if 2 * partial[s] > total)", "if 2 * partial[s] >= total)", ["cut.median.exact_half"]),
    "retreat_through_empty": ("while c2 == 0 and d - 1 >= lo and partial[d - 1] != 0:", "while c2 == 0 and d - 1 >= lo:",
                              ["cut.retreat.stopped_by_empty_prefix"]),
}


def _mutant(old, new):
    src = open(R.__file__).read()
    assert src.count(old) == 1, old
    m = types.ModuleType("colordetect_restate_mutant")
    m.__file__ = R.__file__
    exec(compile(src.replace(old, new), R.__file__, "exec"), m.__dict__)
    return m


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_caught_by_a_claimant_of_its_label(name):
    old, new, labels = MUTANTS[name]
    M = _mutant(old, new)
    for label in labels:
        claimants = [c for c in K.PALETTE_CASES if label in c.claims]
        assert claimants, label
        caught = [c.name for c in claimants if M.palette_from_histogram(c.bins(), c.box, c.max_colors) != c.expected()]
        assert caught, (name, label, [c.name for c in claimants])


def test_unmutated_copy_agrees():
    M = _mutant("MAX_ITERATIONS = 1000\n", "MAX_ITERATIONS = 1000\n\n")
    for c in K.PALETTE_CASES:
        assert M.palette_from_histogram(c.bins(), c.box, c.max_colors) == c.expected()


# ------------------------------------------------------------------------------------------------ histogram cases

@pytest.mark.parametrize("n_cu", [256, 3])
def test_hist_case_reaches_what_it_claims(n_cu):
    claimed = set()
    for c in K.HIST_CASES:
        f = c.frame(n_cu)
        assert f.size == c.data_len and K.samples_of(c.data_len, c.ch, c.quality) == c.n and c.pixels <= K.MAX_FRAME_PIXELS, c.name
        blocks, per = K.lone_geometry(c.n, n_cu)
        hist, labels = K.wave_walk(c.sample_bins(n_cu), blocks, per)
        want, _box = R.histogram(f, c.fmt, c.quality)
        assert np.array_equal(hist, want.astype(np.int64)), c.name            # counted wave by wave == counted plainly
        reached = c.reached(n_cu)
        assert set(c.claims) <= reached, (c.name, sorted(set(c.claims) - reached))
        claimed |= set(c.claims)
    assert claimed == set(K.HIST_LABELS)
    assert {c.n for c in K.HIST_CASES} == set(K.HIST_COUNTS)
    for n in K.HIST_COUNTS:
        assert {c.kind for c in K.HIST_CASES if c.n == n} == set(K.HIST_KINDS), n
    assert {c.misalign for c in K.HIST_CASES if c.fmt == "RGBA"} == {0, 1, 2, 3}
    assert {(c.fmt, c.tail) for c in K.HIST_CASES if c.tail} == {(f, t) for f in K.FORMATS for t in range(1, R.LAYOUT[f][0])}


def test_launch_geometry_model():
    assert K.lone_geometry(16384, 256) == (1, 16384) and K.lone_geometry(16385, 256) == (2, 8193)
    assert K.lone_geometry(32769, 256) == (3, 10923) and K.lone_geometry(32769, 2) == (2, 16385)
    assert K.lone_geometry(32769, 256, n_frames=257) == (1, 32769) and K.lone_geometry(32769, 8, n_frames=3) == (3, 10923)
    for n_cu in (256, 3, 1):
        for n in K.HIST_COUNTS:
            blocks, per = K.lone_geometry(n, n_cu)
            rng = K.block_ranges(n, blocks, per)
            assert rng[0][0] == 0 and rng[-1][1] == n and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(rng, rng[1:] + [(n, n + 1)]))
    # from 3 compute units up the geometry of every count here is one and the same, and 320 frames get one block each
    for n in K.HIST_COUNTS:
        assert {K.lone_geometry(n, n_cu) for n_cu in range(3, 513)} == {K.lone_geometry(n, 256)}
        assert all(K.lone_geometry(n, n_cu, n_frames=320) == (1, n) for n_cu in range(1, 321))
    # the boundary of the two blocks of 16385 samples falls inside a wave
    assert K.lone_geometry(16385, 256)[1] % 64 == 1


@pytest.mark.parametrize("n_cu", [256, 40, 3, 1])
def test_job_plan_model_is_the_librarys(mi355lib, n_cu):
    lib = mi355lib
    sets = [[c.n for c in K.HIST_CASES[k:k + 32]] for k in range(0, len(K.HIST_CASES), 32)]
    sets += [[n] for n in K.HIST_COUNTS] + [[0, 5, 0, 32769], list(K.HIST_COUNTS), [2 ** 32 - 1, 1], [c.samples for c in K.FRAME_CASES[:32]]]
    for ns in sets:
        n = len(ns)
        first, blocks, per, total = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint64 * n)(), C.c_uint32(0)
        lib.mi355_selftest_colordetect_plan.restype = C.c_int
        lib.mi355_selftest_colordetect_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        assert lib.mi355_selftest_colordetect_plan(n_cu, n, (C.c_uint64 * n)(*ns), first, blocks, per, C.byref(total)) == 0
        assert (list(first), list(blocks), list(per), total.value) == K.job_plan(n_cu, ns), ns
    # a lone job's plan is the lone launch's geometry
    for n in K.HIST_COUNTS:
        _f, b, p, _t = K.job_plan(n_cu, [n])
        assert (b[0], p[0]) == K.lone_geometry(n, n_cu)


def test_selftest_entry_is_declared_and_bound(mi355lib):
    import mi355fx
    hdr = open(mi355fx.HEADER_PATH).read()
    assert "mi355_selftest_colordetect_mmcq(" in hdr and hasattr(mi355lib, "mi355_selftest_colordetect_mmcq")
    assert len(mi355lib.mi355_selftest_colordetect_mmcq.argtypes) == 6
    assert mi355lib.mi355_selftest_colordetect_mmcq(None, None, 2, None, None, None) == mi355fx.ERR_INVALID_ARG

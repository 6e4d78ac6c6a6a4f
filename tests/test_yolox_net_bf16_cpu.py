"""CPU checks of the BF16 precision of yoloxinference's network: the rounding helper against known answers and
against torch's bfloat16 casts, the bf16-operand restatement, the three new entry points in header, library and bindings, and the
cap on the cases the guard of tests/yolox_net_bf16.py may drop."""
import re

import numpy as np

import yolox_net_bf16 as B
import yolox_net_cases as K
import yolox_net_restate as R

NEW = {"mi355_yolox_net_set_precision": 2, "mi355_yolox_net_precision": 1, "mi355_selftest_yolox_net_op_bf16_device": 2}


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_bf16_round_known_answers():
    cases = [(0x3F808000, 0x3F80),   # a tie under an even upper half: down
             (0x3F818000, 0x3F82),   # a tie under an odd upper half: up
             (0x3F807FFF, 0x3F80),   # one below a tie
             (0x3F808001, 0x3F81),   # one above a tie
             (0x3F817FFF, 0x3F81), (0x3F818001, 0x3F82),
             (0x3F800000, 0x3F80), (0x40490000, 0x4049), (0x00000000, 0x0000),       # exact values
             (0xBF808000, 0xBF80), (0xBF818000, 0xBF82), (0xBF808001, 0xBF81), (0xC0490FDB, 0xC049),   # negative: the magnitude rounds
             (0x3FFFFFFF, 0x4000), (0x3F7FFFFF, 0x3F80)]                             # a carry into the exponent
    got = B.bf16_bits(_f([c[0] for c in cases]))
    assert [int(v) for v in got] == [c[1] for c in cases]
    back = B.bf16_round(_f([c[0] for c in cases])).view(np.uint32)
    assert [int(v) for v in back] == [c[1] << 16 for c in cases]
    pixels = np.arange(256, dtype=np.float32)
    assert (B.bf16_round(pixels).view(np.uint32) == pixels.view(np.uint32)).all()   # the stem's inputs are exact in bf16


def test_bf16_round_is_torch_bfloat16():
    import torch
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.normal(0.0, 1.0, 4096), rng.normal(0.0, 1e-6, 512), rng.normal(0.0, 1e6, 512)]).astype(np.float32)
    ties = (rng.integers(0x3000, 0x4F00, 1024).astype(np.uint32) << np.uint32(16)) | np.uint32(0x8000)
    a = np.concatenate([a, ties.view(np.float32), -ties.view(np.float32)])
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    assert (B.bf16_round(a).view(np.uint32) == want.view(np.uint32)).all()


def test_the_emulation_is_a_convolution_of_torch_bfloat16_operands():
    import torch
    rng = np.random.default_rng(2)
    for cin, cout, k, stride, h, w in ((5, 7, 3, 1, 6, 9), (33, 4, 1, 1, 5, 7), (12, 24, 3, 2, 8, 8)):
        x = rng.normal(0.0, 1.0, (2, cin, h, w)).astype(np.float32)
        wt = rng.normal(0.0, 0.3, (cout, cin, k, k)).astype(np.float32)
        with B.bf16_operands(np.float64):
            assert R.conv2d is not conv2d_original
            got = R.conv2d(x.astype(np.float64), wt.astype(np.float64), stride, (k - 1) // 2)
        xt = torch.from_numpy(x).to(torch.bfloat16).to(torch.float64)
        wtt = torch.from_numpy(wt).to(torch.bfloat16).to(torch.float64)
        want = torch.nn.functional.conv2d(xt, wtt, stride=stride, padding=(k - 1) // 2).numpy()
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert R.conv2d is conv2d_original                                             # the restatement is itself again


conv2d_original = R.conv2d


def test_depthwise_convolutions_pass_through_unrounded():
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, (1, 4, 5, 5)).astype(np.float32)
    w = rng.normal(0.0, 1.0, (4, 1, 3, 3)).astype(np.float32)
    plain = R.conv2d(x, w, 1, 1, 4)
    with B.bf16_operands(np.float32):
        assert (R.conv2d(x, w, 1, 1, 4) == plain).all()
        assert not (R.conv2d(x, np.repeat(w, 4, axis=1), 1, 1, 1) == conv2d_original(x, np.repeat(w, 4, axis=1), 1, 1, 1)).all()


def test_new_entry_points_in_header_library_and_bindings(mi355lib):
    import mi355fx
    text = re.sub(r"/\*.*?\*/", "", open(mi355fx.HEADER_PATH).read(), flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
        assert m, "the header does not declare %s" % name
        assert m.group(1).count(",") + 1 == n_args
        fn = getattr(mi355lib, name)                                               # exported
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, name
    assert re.search(r"#define\s+MI355_YOLOX_PRECISION_F32\s+0\b", text) and re.search(r"#define\s+MI355_YOLOX_PRECISION_BF16\s+1\b", text)
    assert mi355fx.YOLOX_PRECISION == {"f32": 0, "bf16": 1}
    assert mi355lib.mi355_yolox_net_set_precision(None, 1) == mi355fx.ERR_INVALID_ARG    # a null net, without a device
    assert mi355lib.mi355_yolox_net_precision(None) == mi355fx.ERR_INVALID_ARG
    for m in ("set_precision", "precision"):
        assert callable(getattr(mi355fx.YoloxNet, m))
    assert callable(mi355fx.Context.selftest_yolox_net_op_bf16)


def test_the_guard_drops_at_most_four_cases():
    kept, dropped = B._guarded()
    ratios = [r for _, r in kept + dropped]
    print("rms(emu32 - ref64) / rms(emu64 - ref64) over %d cases: %.3f .. %.3f; dropped: %s" % (len(ratios), min(ratios), max(ratios), [c.name for c, _ in dropped]))
    assert len(kept) + len(dropped) == len(K.all_cases()) == 40 and len(dropped) <= B.MAX_DROPPED
    assert len(B.bf16_cases()) == len(kept) >= 36
    rel = []
    for c, _ in kept:                                                              # the price of the mode, as the docs state it
        ref64, emu64, _ = B.references(c)
        rel += [float(np.sqrt(((e - r) ** 2).mean()) / np.sqrt((r ** 2).mean())) for e, r in zip(emu64, ref64)]
    print("bf16 operands: a level's raw maps differ from f64 by %.2f %% .. %.2f %% of their RMS" % (100 * min(rel), 100 * max(rel)))
    assert max(rel) < 0.1

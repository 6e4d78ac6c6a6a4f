"""colordetect on the GPU: histograms and palettes of mi355_colordetect_* against the independent restatement
(tests/colordetect_restate.py, DESIGN §4.8: parity unpinned), and the element mirror's message behaviour
(video/videofx/src/colordetect/imp.rs, video/videofx/tests/colordetect.rs)."""
import numpy as np
import pytest

import colordetect_restate as R

pytestmark = pytest.mark.gpu

FORMATS = ("RGB", "RGBA", "ARGB", "BGR", "BGRA")


def _dev_hist(ctx, data, fmt, quality):
    a = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    d = ctx.alloc(max(a.nbytes, 16))
    try:
        if a.nbytes:
            ctx.h2d(d, a)
        return ctx.colordetect_histogram_device(d, a.nbytes, fmt, quality)
    finally:
        ctx.free(d)


def _check_hist(ctx, data, fmt, quality):
    hist, box = _dev_hist(ctx, data, fmt, quality)
    want_hist, want_box = R.histogram(data, fmt, quality)
    assert np.array_equal(hist, want_hist), (fmt, quality)
    assert box == want_box, (fmt, quality, box, want_box)


def _solid(w, h, rgb, fmt="RGBA"):
    ch, ri, gi, bi, ai = R.LAYOUT[fmt]
    px = np.zeros(ch, np.uint8)
    px[ri], px[gi], px[bi] = rgb
    if ai is not None:
        px[ai] = 255
    return np.tile(px, w * h)


def _bars(w, h):
    cols = np.array([[192, 192, 192], [192, 192, 0], [0, 192, 192], [0, 192, 0], [192, 0, 192], [192, 0, 0], [0, 0, 192]], np.uint8)
    out = np.empty((h, w, 4), np.uint8)
    out[:, :, :3] = cols[(np.arange(w) * 7) // w][None, :, :]
    out[:, :, 3] = 255
    return out.reshape(-1)


def _two_colour(w, h):
    f = _solid(w, h, (10, 200, 30)).reshape(h, w * 4)
    f[: h // 3] = _solid(w, h // 3, (240, 20, 90)).reshape(h // 3, w * 4)
    return f.reshape(-1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_histogram_matches_restatement_all_qualities(ctx, synth, fmt):
    ch = R.LAYOUT[fmt][0]
    frame = synth.noise_frame(97, 61, channels=ch).reshape(-1)
    for q in range(1, 11):
        _check_hist(ctx, frame, fmt, q)


def test_histogram_ragged_sizes_and_tiny_frames(ctx, synth):
    noise = synth.noise_frame(257, 33).reshape(-1)
    for fmt in FORMATS:
        ch = R.LAYOUT[fmt][0]
        for n in (ch * 1000 + 1, ch * 1000 + ch - 1, 12345, 4 * 3 * 101 + 2):   # data_len not a multiple of ch
            for q in (1, 3, 10):
                _check_hist(ctx, noise[:n], fmt, q)
        for px in (1, 3):                                                          # 1- and 3-pixel frames, q > pixel_count
            for q in (1, 2, 10):
                _check_hist(ctx, noise[: px * ch], fmt, q)
        _check_hist(ctx, noise[: ch - 1], fmt, 1)                                  # less than one pixel: nothing kept


def test_histogram_rgb_padded_rows(ctx, synth):
    """width 641 RGB: rows of 1923 bytes padded to 1924; plane_data(0) is sampled straight across the padding."""
    w, h, stride = 641, 37, 1924
    plane = synth.noise_frame(stride // 4 + 1, h).reshape(-1)[: stride * h]
    for q in (1, 7, 10):
        _check_hist(ctx, plane, "RGB", q)
        _check_hist(ctx, plane, "BGR", q)


def test_histogram_alpha_and_white_boundaries(ctx):
    px = []
    for a in (124, 125, 255):
        for v in (250, 251):
            px += [(v, v, v, a), (251, 251, 250, a), (255, 255, 251, a), (0, 251, 251, a)]
    frame = np.array(px * 3, np.uint8).reshape(-1)
    for fmt in ("RGBA", "ARGB", "BGRA"):
        _check_hist(ctx, frame, fmt, 1)
    hist, box = _dev_hist(ctx, frame, "RGBA", 1)
    kept = sum(1 for r, g, b, a in px if a >= 125 and not (r > 250 and g > 250 and b > 250)) * 3
    assert int(hist.sum()) == kept


def test_histogram_all_colours_quality_1(ctx, synth):
    frame = synth.allcolors(0xA5).reshape(-1)
    hist, box = _dev_hist(ctx, frame, "RGBA", 1)
    want = np.full(32768, 512, np.uint32)
    want[32767] -= 125  # r, g, b > 250 all (5 x 5 x 5 colours) are dropped
    assert np.array_equal(hist, want) and box == (0, 31, 0, 31, 0, 31)
    assert np.array_equal(hist, R.histogram(frame, "RGBA", 1)[0])


def _frames(synth):
    return {
        "smooth": synth.smooth_frame(160, 90).reshape(-1),
        "noise": synth.noise_frame(128, 72).reshape(-1),
        "allcolours": synth.allcolors(0xFF).reshape(-1, 4)[::61].reshape(-1).copy(),
        "bars": _bars(140, 40),
        "red": _solid(64, 48, (255, 0, 0)),
        "two": _two_colour(90, 60),
    }


@pytest.mark.parametrize("max_colors", [2, 3, 5, 8, 16, 64, 255])
def test_palette_matches_restatement(ctx, synth, max_colors):
    """Whole pictures. Which branches of the MMCQ they reach is accidental: the directed coverage, case by case and branch by
    branch, lives in tests/test_gpu_colordetect_cases.py."""
    for name, frame in _frames(synth).items():
        for q in (1, 10):
            got = ctx.colordetect_frame(frame, "RGBA", q, max_colors)
            want = R.get_palette(frame, "RGBA", q, max_colors)
            assert got == want, (name, q, max_colors)
            assert 1 <= len(got) <= max_colors


def test_palette_known_values(ctx):
    red = _solid(64, 48, (255, 0, 0))
    pal = ctx.colordetect_frame(red, "RGBA", 10, 2)
    assert pal == [(252, 4, 4), (0, 4, 4)] and R.css_similar(*pal[0]) == "red"
    one = np.zeros(400, np.uint8)
    one[:4] = (90, 10, 200, 255)   # the only kept sample: one colour once the 1000 rounds are spent
    assert ctx.colordetect_frame(one, "RGBA", 1, 8) == R.get_palette(one, "RGBA", 1, 8) and len(ctx.colordetect_frame(one, "RGBA", 1, 8)) == 1
    for fmt in FORMATS:
        assert ctx.colordetect_frame(_solid(50, 20, (10, 130, 250), fmt), fmt, 3, 5) == R.get_palette(_solid(50, 20, (10, 130, 250), fmt), fmt, 3, 5)


def test_invalid_arguments_and_empty_palettes(ctx):
    import mi355fx
    frame = _solid(8, 8, (1, 2, 3))
    for q, mc in ((0, 2), (11, 2), (10, 1), (10, 256)):
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.colordetect_frame(frame, "RGBA", q, mc)
        assert e.value.status == mi355fx.ERR_INVALID_ARG
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx.colordetect_frame(frame, "RGBx", 10, 2)
    assert e.value.status == mi355fx.ERR_UNSUPPORTED
    assert ctx.colordetect_frame(np.full(4 * 300, 255, np.uint8), "RGBA", 1, 5) == []
    transparent = _solid(20, 15, (10, 20, 30))
    transparent[3::4] = 124
    assert ctx.colordetect_frame(transparent, "RGBA", 1, 5) == []


def test_device_batch_equals_host_calls(ctx, synth):
    """8 different frames at frame_pitch > data_len: one call == 8 host calls; the frames are not written."""
    w, h = 200, 120
    data_len = w * h * 3 - 5          # not a multiple of 3
    pitch = data_len + 4099
    frames = [synth.noise_frame(w, h, seed=s, channels=3).reshape(-1)[:data_len] for s in range(3)]
    frames += [synth.smooth_frame(w, h, seed=s).reshape(-1)[:data_len] for s in range(3)]
    frames += [_bars(w, h)[:data_len], _solid(w, h, (255, 0, 0))[:data_len]]
    buf = np.zeros(pitch * 8, np.uint8)
    for f, fr in enumerate(frames):
        buf[f * pitch: f * pitch + data_len] = fr
    d = ctx.alloc(buf.nbytes)
    try:
        ctx.h2d(d, buf)
        for mc in (2, 16, 255):
            for q in (1, 10):
                got = ctx.colordetect_frames_device(d, pitch, data_len, 8, "RGB", q, mc)
                assert got == [ctx.colordetect_frame(fr, "RGB", q, mc) for fr in frames], (q, mc)
                assert got == [R.get_palette(fr, "RGB", q, mc) for fr in frames], (q, mc)
        back = np.zeros_like(buf)
        ctx.d2h(back, d)
        assert np.array_equal(back, buf)
    finally:
        ctx.free(d)
    host = frames[0].copy()
    ctx.colordetect_frame(host, "RGB", 1, 8)
    assert np.array_equal(host, frames[0])


def test_element_messages():
    from mi355fx.elements import Element, FLOW_OK, FLOW_ERROR, FLOW_NOT_NEGOTIATED
    e = Element("colordetect")
    assert e.type_name == "GstColorDetect" and e.klass == "Filter/Video"
    assert e.formats(False) == list(FORMATS) and e.formats(True) == list(FORMATS)
    props = e.properties()
    assert props["quality"]["default"] == 10 and props["quality"]["min"] == 0 and props["quality"]["max"] == 10
    assert props["max-colors"]["default"] == 2 and props["max-colors"]["min"] == 2 and props["max-colors"]["max"] == 255
    assert props["quality"]["mutable"] == "playing" and props["max-colors"]["mutable"] == "playing"
    red, blue = _solid(64, 48, (255, 0, 0)), _solid(64, 48, (0, 0, 255))
    assert e.colordetect_transform(red) == FLOW_NOT_NEGOTIATED          # no state before set_info
    assert e.colordetect_pop_message() is None
    assert e.start() and e.colordetect_set_info("RGBA")
    assert e.colordetect_transform(red) == FLOW_OK and e.colordetect_transform(red) == FLOW_OK
    m = e.colordetect_pop_message()
    assert m == {"dominant-color": "red", "palette": [(252 << 16) | (4 << 8) | 4, (0 << 16) | (4 << 8) | 4]}
    assert e.colordetect_pop_message() is None                          # two red frames: exactly one message
    assert e.colordetect_transform(blue) == FLOW_OK
    m = e.colordetect_pop_message()
    assert m["dominant-color"] == "blue" and m["palette"] == R.pack(R.get_palette(blue, "RGBA", 10, 2))
    assert e.colordetect_set_info("RGBA") and e.colordetect_transform(blue) == FLOW_OK
    assert e.colordetect_pop_message() is None                          # set_info keeps the colour
    assert not e.colordetect_set_info("RGBx")
    assert e.stop() and e.start() and e.colordetect_set_info("RGBA")
    assert e.colordetect_transform(blue) == FLOW_OK
    assert e.colordetect_pop_message()["dominant-color"] == "blue"      # stop drops the state: posts again
    assert e.set_property("quality", 0) and e.get_property("quality") == 0
    assert e.colordetect_transform(red) == FLOW_ERROR and e.colordetect_pop_message() is None
    for name, bad in (("quality", 11), ("max-colors", 1), ("max-colors", 256), ("quality", 2.5)):
        assert not e.set_property(name, bad)
    assert e.set_property("quality", 1) and e.set_property("max-colors", 255)
    assert e.get_property("quality") == 1 and e.get_property("max-colors") == 255
    white = np.full(64 * 4, 255, np.uint8)
    assert e.colordetect_transform(white) == FLOW_ERROR                  # no colour: error, nothing posted
    assert e.colordetect_pop_message() is None
    e.close()


def test_element_device_path(ctx):
    from mi355fx.elements import Element, FLOW_OK
    e = Element("colordetect")
    assert e.start() and e.colordetect_set_info("BGR")
    fr = _solid(33, 17, (0, 128, 0), "BGR")
    d = ctx.alloc(fr.nbytes)
    try:
        ctx.h2d(d, fr)
        assert e.colordetect_transform_device(d, fr.nbytes) == FLOW_OK
    finally:
        ctx.free(d)
    m = e.colordetect_pop_message()
    assert m["dominant-color"] == R.css_similar(*R.get_palette(fr, "BGR", 10, 2)[0])
    assert m["palette"] == R.pack(R.get_palette(fr, "BGR", 10, 2))
    e.close()

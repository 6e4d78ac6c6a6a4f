"""colordetect without a GPU: the restatement of the palette contract reproduces its pinned checks, the host
library's css lookup agrees with the 148 named colours, and the GStreamer shim carries the reference's surface
(tests/golden/colordetect_surface.json, from docs/plugins/gst_plugins_cache.json)."""
import json
import os
import re
import subprocess

import numpy as np

import colordetect_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GST = os.path.join(ROOT, "gst")
SURFACE = json.load(open(os.path.join(ROOT, "tests", "golden", "colordetect_surface.json")))["colordetect"]


def _rgba(pixels):
    return np.array(pixels, np.uint8).reshape(-1)


def test_solid_red_palette_and_name():
    red = np.tile(np.array([255, 0, 0, 255], np.uint8), 320 * 240)
    pal = R.get_palette(red, "RGBA", 10, 2)
    assert pal == [(252, 4, 4), (0, 4, 4)]   # second entry: the inverted empty box past bin 31 (4 * (32 + 31 + 1) mod 256 = 0)
    assert R.css_similar(*pal[0]) == "red"


def test_one_kept_sample_gives_one_colour_and_white_gives_none():
    one = np.zeros(4 * 50, np.uint8)
    one[:4] = (17, 99, 200, 255)
    assert R.get_palette(one, "RGBA", 1, 8) == [((17 >> 3) * 8 + 4, (99 >> 3) * 8 + 4, (200 >> 3) * 8 + 4)]
    assert R.get_palette(np.full(4 * 100, 255, np.uint8), "RGBA", 1, 2) == []


def test_alpha_and_white_thresholds():
    frame = _rgba([(10, 10, 10, 124), (20, 20, 20, 125), (251, 251, 251, 255), (250, 251, 251, 255), (251, 250, 251, 255), (251, 251, 250, 255)])
    hist, box = R.histogram(frame, "RGBA", 1)
    assert int(hist.sum()) == 4   # alpha 124 dropped; only all three > 250 is white
    assert hist[(2 << 10) | (2 << 5) | 2] == 1 and hist[(31 << 10) | (31 << 5) | 31] == 3
    assert box == (2, 31, 2, 31, 2, 31)


def test_byte_orders_and_flat_sampling():
    px = {"RGB": (1, 2, 3), "RGBA": (1, 2, 3, 255), "ARGB": (255, 1, 2, 3), "BGR": (3, 2, 1), "BGRA": (3, 2, 1, 255)}
    for fmt, p in px.items():
        hist, box = R.histogram(np.array(p * 3 + (9,), np.uint8), fmt, 1)   # a trailing partial pixel is not sampled
        assert box == (0, 0, 0, 0, 0, 0) and int(hist.sum()) == 3, fmt
    # quality q samples pixel indices 0, q, 2q, ... of the flat run
    frame = np.zeros((10, 4), np.uint8)
    frame[:, 3] = 255
    frame[:, 0] = np.arange(10) * 8
    hist, box = R.histogram(frame.reshape(-1), "RGBA", 3)
    assert box[:2] == (0, 9) and int(hist.sum()) == 4


def test_hand_worked_two_colour_cut():
    # 3 samples at r bin 2 and 1 at r bin 20, g = b = 0: r is the widest axis (19 > 1); partial: [3 at 2 .. 3 up to 19, 4 at 20]
    # i = 2 (2 * 3 > 4), left 0 <= right 18: d = min(19, 2 + 9) = 11; partial[11] = 3 != 0; c2 = 1: boxes r 2..11 and 12..20
    frame = _rgba([(16, 0, 0, 255)] * 3 + [(160, 0, 0, 255)])
    hist, box = R.histogram(frame, "RGBA", 1)
    assert box == (2, 20, 0, 0, 0, 0)
    hist3 = np.asarray(hist, np.uint64).reshape(32, 32, 32)
    v1, v2 = R._cut(R.Box((2, 0, 0), (20, 0, 0), hist3), hist3)
    assert (v1.lo, v1.hi, v1.count, v1.avg) == ([2, 0, 0], [11, 0, 0], 3, (20, 4, 4))
    assert (v2.lo, v2.hi, v2.count, v2.avg) == ([12, 0, 0], [20, 0, 0], 1, (164, 4, 4))
    assert R.get_palette(frame, "RGBA", 1, 2) == [(20, 4, 4), (164, 4, 4)]


def test_inverted_box_past_bin_31():
    hist3 = np.zeros((32, 32, 32), np.uint64)
    v = R.Box((32, 5, 0), (31, 7, 31), hist3)
    assert v.count == 0 and v.volume == 0 and v.avg == (0, 4 * 13, 4 * 32 % 256)


def test_css_similar_maps_every_named_colour_to_itself_or_first_alias():
    from mi355fx.elements import _lib
    L = _lib()
    colours = R.css_colors()
    assert len(colours) == 148 and [c[0] for c in colours] == sorted(c[0] for c in colours)
    first = {}
    for name, r, g, b in colours:
        first.setdefault((r, g, b), name)
    for name, r, g, b in colours:
        got = L.mi355host_css_color_similar(r, g, b).decode()
        assert got == first[(r, g, b)] == R.css_similar(r, g, b), name
    assert L.mi355host_css_color_similar(0, 255, 255) == b"aqua" and L.mi355host_css_color_similar(128, 128, 128) == b"gray"
    rng = np.random.default_rng(5)
    for r, g, b in rng.integers(0, 256, size=(300, 3)):
        assert L.mi355host_css_color_similar(int(r), int(g), int(b)).decode() == R.css_similar(int(r), int(g), int(b))


def test_shim_carries_the_pinned_surface():
    src = open(os.path.join(GST, "gstcolordetect.c")).read()
    assert re.search(r'gst_element_register\(plugin, "colordetect", GST_RANK_NONE, GST_TYPE_COLOR_DETECT\)', src)
    assert "G_DEFINE_TYPE(%s, gst_color_detect, GST_TYPE_VIDEO_FILTER)" % SURFACE["type_name"] in src
    assert 'gst_element_class_set_static_metadata(element, "%s", "%s", "%s",' % (SURFACE["long_name"], SURFACE["klass"], SURFACE["description"]) in src
    assert '"%s"' % SURFACE["author"] in src
    assert 'GST_DEBUG_CATEGORY_INIT(gst_color_detect_debug, "colordetect", 0,' in src
    q, m = SURFACE["properties"]["quality"], SURFACE["properties"]["max-colors"]
    assert re.search(r'g_param_spec_uint\("quality", "[^"]*", "%s", %s, %s, %s, f\)' % (q["blurb"], q["min"], q["max"], q["default"]), src)
    assert re.search(r'g_param_spec_uint\("max-colors", "[^"]*", "%s", %s, %s, %s, f\)' % (m["blurb"], m["min"], m["max"], m["default"]), src)
    assert "GST_PARAM_MUTABLE_PLAYING" in src and q["mutable"] == m["mutable"] == "playing"
    assert '"{ %s }"' % ", ".join(SURFACE["sink_formats"]) in src and SURFACE["sink_formats"] == SURFACE["src_formats"]
    assert "trans->passthrough_on_same_caps = TRUE;" in src and "trans->transform_ip_on_passthrough = TRUE;" in src
    assert "vfilter->transform_frame_ip =" in src and "vfilter->transform_frame =" not in src
    assert "trans->transform_ip =" in src and "gst_mi355_buffer_peek_device(" in src and "vfilter->set_info =" in src
    assert '"%s"' % SURFACE["message"]["name"] in src
    for field in SURFACE["message"]["fields"]:
        assert '"%s"' % field in src
    assert "GST_TYPE_LIST" in src and "G_TYPE_UINT" in src and "gst_message_new_element(" in src
    assert "mi355_colordetect_frame(" in src and "mi355_colordetect_frames_device(" in src and "mi355host_css_color_similar(" in src
    plugin = open(os.path.join(GST, "plugin_rsvideofx.c")).read()
    order = [plugin.index("gst_%s_register(plugin)" % n) for n in ("rounded_corners", "color_detect", "video_compare")]
    assert order == sorted(order)
    mk = open(os.path.join(GST, "Makefile")).read()
    recipe = re.search(r"^libgstrsvideofx\.so:.*\n\t.*$", mk, flags=re.M).group(0)
    assert "gstcolordetect.c" in recipe.splitlines()[0] and "gstcolordetect.c" in recipe.splitlines()[1]


def test_shim_syntax_covers_the_new_file():
    r = subprocess.run(["make", "-C", GST, "syntax"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len([f for f in os.listdir(GST) if f.endswith(".c")])
    assert os.path.exists(os.path.join(GST, "gstcolordetect.c")) and "syntax ok: %d files" % n in r.stdout


def test_library_exports_the_entry_points(mi355lib):
    import mi355fx
    hdr = open(mi355fx.HEADER_PATH).read()
    for name in ("mi355_colordetect_frame", "mi355_colordetect_frames_device", "mi355_colordetect_histogram_device"):
        assert name + "(" in hdr and hasattr(mi355lib, name) and getattr(mi355lib, name).argtypes is not None

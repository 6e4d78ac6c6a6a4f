/* gst/plugin_rsaudiofx.c — plugin "rsaudiofx" = libgstrsaudiofx.so (audio/audiofx/src/lib.rs:23-46, Cargo.toml lib name
 * gstrsaudiofx). plugin_init registers the elements in the reference's order. Only audiornnoise (lib.rs:30) is missing: it runs
 * nnnoiseless 0.5.2's trained model, whose weights are not part of the reference tree. This library has the reference's file
 * and plugin name, so installing it removes audiornnoise from the system. */
#include <gst/gst.h>
#ifndef PACKAGE
#define PACKAGE "gst-plugin-audiofx"
#endif
gboolean gst_rs_aging_radio_register(GstPlugin *plugin);
gboolean gst_rs_audio_echo_register(GstPlugin *plugin);
gboolean gst_audio_loud_norm_register(GstPlugin *plugin);
gboolean gst_ebur128_level_register(GstPlugin *plugin);

static gboolean plugin_init(GstPlugin *plugin) {
  return gst_rs_aging_radio_register(plugin) && gst_rs_audio_echo_register(plugin) && gst_audio_loud_norm_register(plugin) && gst_ebur128_level_register(plugin);
}

GST_PLUGIN_DEFINE(GST_VERSION_MAJOR, GST_VERSION_MINOR, rsaudiofx, "GStreamer Rust Audio Effects Plugin (MI355X kernels)", plugin_init,
                  "0.16.0-alpha.1-mi355fx", "MPL", "gst-plugin-audiofx", "https://gitlab.freedesktop.org/gstreamer/gst-plugins-rs")

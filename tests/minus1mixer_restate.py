"""Restatement of the reference's mixing loop and splitter (checker only; the product never imports it).

MultiMixerElement::aggregate_one_buffer (audio/audiomultimixer/src/audiomultimixerelement.rs:606-753) adds one mono segment into
the f32 accumulators of every output channel it contributes to; Splitter's split_output_buf (audio/audiomultimixer/src/splitter.rs:433-467)
converts each output's channels with T::from_f32(acc * conv_scale). All arithmetic is np.float32; the segments are walked in a
literal loop in array order, because f32 addition is not associative (frames and channels are independent of each other, so those two
axes are array operations)."""
import numpy as np

F32, S16 = 0, 1
SCALE = {F32: np.float32(1.0), S16: np.float32(32768.0)}
DTYPE = {F32: np.float32, S16: np.int16}


def minus1(n):
    """update_output_config's matrix (minus1mixer.rs:500-537): contrib[i][o] = (i != o), one channel per output"""
    return ~np.eye(n, dtype=bool)


def fmt_of(a):
    return {np.dtype(np.float32): F32, np.dtype(np.int16): S16}[a.dtype]


def accumulate(contrib, segments, frames):
    """-> f32 accumulators [frames, n_out_channels]. segments: (input, data, out_offset), data a 1-D float32 / int16 array."""
    contrib = np.asarray(contrib, dtype=bool)
    acc = np.zeros((frames, contrib.shape[1]), np.float32)   # the aggregator's zero-filled buffer: +0.0
    with np.errstate(all="ignore"):
        for inp, data, off in segments:
            x = data.astype(np.float32) / SCALE[fmt_of(data)]   # f32::from(x) / conv_scale (:707)
            cols = np.flatnonzero(contrib[inp])
            if len(x) and len(cols):
                acc[off:off + len(x), cols] = acc[off:off + len(x), cols] + x[:, None]   # if contrib { *sample += in_sample } (:711-715)
    return acc


def convert(acc, fmt):
    """T::from_f32(acc * conv_scale) (splitter.rs:460): f32 as is; i16 as Rust's `as`: toward zero, NaN 0, saturating"""
    with np.errstate(all="ignore"):
        v = acc * SCALE[fmt]
        if fmt == F32:
            return v.astype(np.float32)
        t = np.clip(np.trunc(v), -32768.0, 32767.0)
        return np.where(np.isnan(v), np.float32(0.0), t).astype(np.int16)


def mix(contrib, segments, outputs, frames):
    """outputs: (format, channel_offset, n_channels) -> one interleaved array [frames * n_channels] per output"""
    acc = accumulate(contrib, segments, frames)
    return [np.ascontiguousarray(convert(acc[:, off:off + nch], fmt)).reshape(-1) for fmt, off, nch in outputs]

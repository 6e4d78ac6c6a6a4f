// mixer.hip — gfx950 kernel, planner and C ABI for minus1mixer / audiomultimixer.
//
// Reference loops replaced: MultiMixerElement::aggregate_one_buffer (audio/audiomultimixer/src/audiomultimixerelement.rs:606-753),
// which adds one mono input segment into every output channel it contributes to - in_sample = f32::from(x) / conv_scale (:707),
// `if contrib { *sample += in_sample }` (:711-715) - in an interleaved f32 buffer n_out_channels wide, and the splitter's
// split_output_buf (splitter.rs:433-467), which slices that buffer into the per-output buffers with T::from_f32(acc * conv_scale)
// (:460). minus1mixer builds contrib[i][o] = (i != o), one channel per output (minus1mixer.rs:500-537). One interval is a pure
// function of its segments and the contribution matrix; f32 addition is not associative, so the ORDER in which segments reach an
// output sample is part of the result: the kernel adds them in array order.
//
// Limits (beyond any of them MI355_ERR_UNSUPPORTED): n_inputs <= 256, n_out_channels <= 256, at most 1024 segments per interval,
// frames <= 2^20; and at most 1024 outputs (every block walks its mixer's output list).
//
// One kernel, one launch for every mixer of a launch set:
//   block = (mixer, tile of kMixTile = 64 frames, group of kMixGroup = 16 output channels); 256 threads = 4 waves; a lane owns one
//   frame of the tile and the 4 consecutive channels of its wave, as 4 f32 accumulators that start at +0.0.
//   The mixer's segments are walked in array order, 64 candidates at a time: lane l tests candidate l against the tile, the ballot
//   (the same 64-bit word in every wave) names the segments that touch it, in order. Those become rows of an LDS image
//   [<= 64 rows][64 frames] f32: wave w converts rows w, w + 4, ... - one coalesced load per row, the sample converted ONCE for all
//   16 channels, frames the segment does not cover staged as +0.0 - and writes the row's 16 contribution bits beside it. After the
//   barrier every lane walks the rows in order: acc[k] = bit ? acc[k] + row[lane] : acc[k] (a select: inf and NaN survive; the bit
//   is uniform per wave; lanes along frames read consecutive banks). An accumulator that starts at +0.0 never becomes -0.0, so the
//   +0.0 of an uncovered frame leaves it bit for bit as skipping would.
//   Then the outputs that own one of the wave's channels are found the same way (ballot over the mixer's outputs) and the lane
//   stores its samples straight into their buffers, F32 as is, S16 as Rust's saturating `as i16` of acc * 32768.
//   LDS: 64 * 64 * 4 + 64 * 4 = 16.25 KiB per block whatever the mixer's size (more rows = more chunks), so the 160 KiB of a CU hold
//   8 blocks = 32 waves. No wide intermediate in HBM, no atomics, nothing depends on the order blocks run in.
#include "internal.hpp"

#include <cstring>
#include <vector>

namespace mi355 {

constexpr unsigned kMixTile = MI355_MIXER_FRAME_TILE;   // frames per block: one wave wide
constexpr unsigned kMixGroup = 16;                      // output channels per block: 4 waves x 4 accumulators
constexpr unsigned kMixRows = 64;                       // rows staged per chunk = candidates per ballot
constexpr unsigned kMixMaxInputs = 256, kMixMaxChannels = 256, kMixMaxSegments = 1024, kMixMaxOutputs = 1024;
constexpr size_t kMixMaxFrames = (size_t)1 << 20;
static_assert(kMixTile == 64, "a lane per frame: the tile is one wave wide");

struct MixSeg { const void *data; uint32_t input, format, out_offset, num_frames; };
struct MixOut { void *data; uint32_t format, channel_offset, n_channels, pad; };
struct MixJob { uint32_t n_groups, n_segs, n_outs, frames, seg_off, out_off, bits_off, pad; };
struct MixTables {
  const uint32_t *first_block;   // [n_jobs + 1], running sum of the jobs' blocks
  const MixJob *jobs;
  const MixSeg *segs;
  const MixOut *outs;
  const uint16_t *bits;          // per job [n_inputs][n_groups]: bit k = contrib[input][16 * group + k]
  uint32_t n_jobs;
};

// block b of a launch -> its job (first_block[n_jobs] > b), then its frame tile and channel group: the blocks of one tile are
// neighbours (they read the same input samples). The planner's self-test walks these very functions.
__host__ __device__ inline uint32_t mixer_locate(const uint32_t *first_block, uint32_t n_jobs, uint32_t b) {
  uint32_t lo = 0, hi = n_jobs;   // first_block[lo] <= b < first_block[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first_block[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}
__host__ __device__ inline void mixer_split(uint32_t local, uint32_t n_groups, uint32_t *tile, uint32_t *group) {
  *tile = local / n_groups;
  *group = local % n_groups;
}

// T::from_f32 of the splitter for i16 = Rust's `as i16`: NaN -> 0, saturating, truncating toward zero
__device__ __forceinline__ int16_t mix_to_s16(float acc) {
  const float v = acc * 32768.0f;
  if (v != v) return 0;
  if (v >= 32767.0f) return 32767;
  if (v <= -32768.0f) return -32768;
  return (int16_t)(int)v;
}

__global__ __launch_bounds__(256) void mixer_kernel(MixTables T) {
  __shared__ float rows[kMixRows][kMixTile];
  __shared__ uint32_t rowbits[kMixRows];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t j = mixer_locate(T.first_block, T.n_jobs, blockIdx.x);
  const MixJob J = T.jobs[j];
  uint32_t tile, group;
  mixer_split(blockIdx.x - T.first_block[j], J.n_groups, &tile, &group);
  const uint32_t f0 = tile * kMixTile, f = f0 + lane;
  const uint32_t f1 = f0 + kMixTile < J.frames ? f0 + kMixTile : J.frames;
  const MixSeg *segs = T.segs + J.seg_off;
  const uint16_t *bits = T.bits + J.bits_off;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};

  for (uint32_t base = 0; base < J.n_segs; base += 64) {
    // which of these 64 segments touch the tile: the same word in every wave
    bool hit = false;
    if (base + lane < J.n_segs) {
      const MixSeg S = segs[base + lane];
      hit = S.num_frames != 0 && S.out_offset < f1 && S.out_offset + S.num_frames > f0;
    }
    const unsigned long long mask = __ballot(hit);
    if (mask == 0) continue;
    const unsigned cnt = (unsigned)__popcll(mask);
    unsigned long long m = mask;
    for (unsigned r = 0; m; r++) {
      const unsigned b = (unsigned)__ffsll(m) - 1u;
      m &= m - 1;
      if ((r & 3u) != wave) continue;
      const MixSeg S = segs[base + b];
      float v = 0.0f;   // +0.0 where the segment does not cover the frame
      if (f >= S.out_offset && f - S.out_offset < S.num_frames) {
        const uint32_t i = f - S.out_offset;
        v = S.format ? (float)((const int16_t *)S.data)[i] / 32768.0f : ((const float *)S.data)[i];
      }
      rows[r][lane] = v;
      if (lane == 0) rowbits[r] = bits[(size_t)S.input * J.n_groups + group];
    }
    __syncthreads();
    for (unsigned r = 0; r < cnt; r++) {
      const uint32_t w = rowbits[r] >> (4u * wave);
      const float v = rows[r][lane];
#pragma unroll
      for (unsigned k = 0; k < 4; k++) acc[k] = ((w >> k) & 1u) ? acc[k] + v : acc[k];
    }
    __syncthreads();   // the next chunk overwrites the rows
  }

  // the outputs that own one of this wave's channels [cw, cw + 4)
  const uint32_t cw = group * kMixGroup + 4u * wave;
  const MixOut *outs = T.outs + J.out_off;
  for (uint32_t base = 0; base < J.n_outs; base += 64) {
    bool hit = false;
    if (base + lane < J.n_outs) {
      const MixOut O = outs[base + lane];
      hit = O.channel_offset < cw + 4u && O.channel_offset + O.n_channels > cw;
    }
    unsigned long long m = __ballot(hit);
    while (m) {
      const unsigned b = (unsigned)__ffsll(m) - 1u;
      m &= m - 1;
      const MixOut O = outs[base + b];
      if (f >= J.frames) continue;
#pragma unroll
      for (unsigned k = 0; k < 4; k++) {
        const uint32_t c = cw + k;
        if (c < O.channel_offset || c - O.channel_offset >= O.n_channels) continue;
        const size_t idx = (size_t)f * O.n_channels + (c - O.channel_offset);
        if (O.format) ((int16_t *)O.data)[idx] = mix_to_s16(acc[k]);
        else ((float *)O.data)[idx] = acc[k];
      }
    }
  }
}

// ---------------------------------------------------------------- host side

static inline uint32_t mix_groups(uint32_t n_out) { return (n_out + kMixGroup - 1) / kMixGroup; }
static inline uint32_t mix_tiles(uint64_t frames) { return (uint32_t)((frames + kMixTile - 1) / kMixTile); }

// The job table of one launch (mi355_selftest_mixer_plan): member j gets ceil(frames / 64) * ceil(n_out_channels / 16) blocks -
// none when it has no frame - and its slices of the segment, output and contribution-bit tables. Every array is [n_members + 1]
// with the total in the last entry.
int mixer_plan(int n_members, const uint32_t *n_inputs, const uint32_t *n_out_channels, const uint32_t *n_segments, const uint32_t *n_outputs,
               const uint64_t *frames, uint32_t *first_block, uint32_t *seg_off, uint32_t *out_off, uint32_t *bits_off) {
  if (n_members < 0 || n_members > 4096 || !first_block || !seg_off || !out_off || !bits_off) return MI355_ERR_INVALID_ARG;
  if (n_members > 0 && (!n_inputs || !n_out_channels || !n_segments || !n_outputs || !frames)) return MI355_ERR_INVALID_ARG;
  uint64_t fb = 0, so = 0, oo = 0, bo = 0;
  for (int j = 0; j < n_members; j++) {
    if (n_inputs[j] == 0 || n_out_channels[j] == 0) return MI355_ERR_INVALID_ARG;
    if (n_inputs[j] > kMixMaxInputs || n_out_channels[j] > kMixMaxChannels || n_segments[j] > kMixMaxSegments || n_outputs[j] > kMixMaxOutputs || frames[j] > kMixMaxFrames)
      return MI355_ERR_UNSUPPORTED;
    first_block[j] = (uint32_t)fb; seg_off[j] = (uint32_t)so; out_off[j] = (uint32_t)oo; bits_off[j] = (uint32_t)bo;
    fb += (uint64_t)mix_tiles(frames[j]) * mix_groups(n_out_channels[j]);
    so += n_segments[j];
    oo += n_outputs[j];
    bo += (uint64_t)n_inputs[j] * mix_groups(n_out_channels[j]);
    if (fb > 0x7fffffffull || oo > 0x7fffffffull) return MI355_ERR_UNSUPPORTED;
  }
  first_block[n_members] = (uint32_t)fb; seg_off[n_members] = (uint32_t)so; out_off[n_members] = (uint32_t)oo; bits_off[n_members] = (uint32_t)bo;
  return MI355_OK;
}

// contrib (row-major n_inputs x n_out_channels; nullptr: minus1mixer's i != o) -> [n_inputs][groups] words of 16 bits
void mixer_pack_contrib(unsigned n_inputs, unsigned n_out, const uint8_t *contrib, std::vector<uint16_t> *bits) {
  const unsigned G = mix_groups(n_out);
  bits->assign((size_t)n_inputs * G, 0);
  for (unsigned i = 0; i < n_inputs; i++)
    for (unsigned c = 0; c < n_out; c++)
      if (contrib ? contrib[(size_t)i * n_out + c] != 0 : i != c) (*bits)[(size_t)i * G + c / kMixGroup] |= (uint16_t)(1u << (c % kMixGroup));
}

int mixer_check_setup(unsigned n_inputs, unsigned n_out, const char **why) {
  if (n_inputs == 0 || n_out == 0) { *why = "mixer: no input or no output channel"; return MI355_ERR_INVALID_ARG; }
  if (n_inputs > kMixMaxInputs || n_out > kMixMaxChannels) { *why = "mixer: at most 256 inputs and 256 output channels"; return MI355_ERR_UNSUPPORTED; }
  return MI355_OK;
}

// the checks of mi355_mixer_process for one interval, before anything is copied, launched or written
int mixer_check(unsigned n_inputs, unsigned n_out, const mi355_mixer_segment *segs, unsigned n_segs, const mi355_mixer_output *outs, unsigned n_outs,
                size_t frames, bool device, const char **why) {
  if (n_outs > kMixMaxOutputs) { *why = "mixer: at most 1024 outputs"; return MI355_ERR_UNSUPPORTED; }
  if (n_segs > kMixMaxSegments) { *why = "mixer: at most 1024 segments per interval"; return MI355_ERR_UNSUPPORTED; }
  if (frames > kMixMaxFrames) { *why = "mixer: at most 2^20 frames per interval"; return MI355_ERR_UNSUPPORTED; }
  if ((n_segs && !segs) || (n_outs && !outs)) { *why = "mixer: null segment or output array"; return MI355_ERR_INVALID_ARG; }
  for (unsigned s = 0; s < n_segs; s++) {
    const mi355_mixer_segment &S = segs[s];
    if (S.input >= n_inputs) { *why = "mixer: a segment names an input the mixer does not have"; return MI355_ERR_INVALID_ARG; }
    if (S.format > 1) { *why = "mixer: unknown segment format"; return MI355_ERR_INVALID_ARG; }
    if ((uint64_t)S.out_offset + S.num_frames > frames) { *why = "mixer: a segment ends after the interval"; return MI355_ERR_INVALID_ARG; }
    if (S.num_frames && !S.data) { *why = "mixer: null segment data"; return MI355_ERR_INVALID_ARG; }
    // the kernel loads samples as f32 / i16 (the host form packs every buffer at a multiple of 4 bytes itself)
    if (device && ((uintptr_t)S.data & (S.format ? 1u : 3u))) { *why = "mixer: device segment data not aligned to its sample type"; return MI355_ERR_INVALID_ARG; }
  }
  for (unsigned o = 0; o < n_outs; o++) {
    const mi355_mixer_output &O = outs[o];
    if (O.format > 1) { *why = "mixer: unknown output format"; return MI355_ERR_INVALID_ARG; }
    if (O.n_channels == 0) { *why = "mixer: an output without channels"; return MI355_ERR_INVALID_ARG; }
    if ((uint64_t)O.channel_offset + O.n_channels > n_out) { *why = "mixer: an output names channels the mixer does not have"; return MI355_ERR_INVALID_ARG; }
    if (frames && !O.data) { *why = "mixer: null output data"; return MI355_ERR_INVALID_ARG; }
    if (device && ((uintptr_t)O.data & (O.format ? 1u : 3u))) { *why = "mixer: device output data not aligned to its sample type"; return MI355_ERR_INVALID_ARG; }
  }
  return MI355_OK;
}

// where the host form packs a call's buffers in its staging slots: every buffer at a multiple of 4 bytes
void mixer_layout(const mi355_mixer_segment *segs, unsigned n_segs, const mi355_mixer_output *outs, unsigned n_outs, size_t frames, MixerLayout *L) {
  L->seg_off.resize(n_segs); L->seg_bytes.resize(n_segs);
  L->out_off.resize(n_outs); L->out_bytes.resize(n_outs);
  size_t at = 0;
  for (unsigned s = 0; s < n_segs; s++) {
    L->seg_off[s] = at;
    L->seg_bytes[s] = (size_t)segs[s].num_frames * (segs[s].format ? 2 : 4);
    at += (L->seg_bytes[s] + 3) & ~(size_t)3;
  }
  L->in_bytes = at;
  at = 0;
  for (unsigned o = 0; o < n_outs; o++) {
    L->out_off[o] = at;
    L->out_bytes[o] = frames * outs[o].n_channels * (outs[o].format ? 2 : 4);
    at += (L->out_bytes[o] + 3) & ~(size_t)3;
  }
  L->out_bytes_total = at;
}

struct MixerTablesBuf {
  char *h = nullptr, *d = nullptr;   // two pinned images of `cap` bytes, used in turn, and the device image of a launch's tables
  size_t cap = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};   // ev[k]: the last launch that used pinned image k has copied it out
  int use = 0;                             // the pinned image the next launch fills: an enqueue never waits for the copy before it
};

MixerTablesBuf *mixer_tables_new(std::string *err, int *status) {
  auto *B = new MixerTablesBuf();
  hipError_t e = hipEventCreateWithFlags(&B->ev[0], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&B->ev[1], hipEventDisableTiming);
  if (e != hipSuccess) {
    if (B->ev[0]) (void)hipEventDestroy(B->ev[0]);
    if (err) *err = std::string("hipEventCreate(mixer tables): ") + hipGetErrorString(e);
    if (status) *status = MI355_ERR_HIP;
    delete B;
    return nullptr;
  }
  return B;
}

void mixer_tables_free(MixerTablesBuf *B) {
  if (!B) return;
  if (B->h) (void)hipHostFree(B->h);
  if (B->d) (void)hipFree(B->d);
  for (hipEvent_t ev : B->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete B;
}

static int mix_hip(hipError_t e, const char *what, std::string *err) {
  if (e == hipSuccess) return MI355_OK;
  (void)hipGetLastError();
  if (err) *err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? MI355_ERR_OUT_OF_MEMORY : MI355_ERR_HIP;
}

// n checked calls (data pointers on the device) on `stream`: one table copy and ONE kernel launch - none when no call has a frame.
int mixer_launch(MixerTablesBuf *B, hipStream_t stream, const MixerCall *calls, int n, int *kernel_launches, std::string *err) {
  if (kernel_launches) *kernel_launches = 0;
  if (n <= 0) return MI355_OK;
  std::vector<uint32_t> ni((size_t)n), nc((size_t)n), ns((size_t)n), no((size_t)n), fb((size_t)n + 1), so((size_t)n + 1), oo((size_t)n + 1), bo((size_t)n + 1);
  std::vector<uint64_t> fr((size_t)n);
  for (int j = 0; j < n; j++) {
    ni[j] = calls[j].n_inputs; nc[j] = calls[j].n_out_channels; ns[j] = calls[j].n_segs; no[j] = calls[j].n_outs; fr[j] = calls[j].frames;
  }
  int rc = mixer_plan(n, ni.data(), nc.data(), ns.data(), no.data(), fr.data(), fb.data(), so.data(), oo.data(), bo.data());
  if (rc) { if (err) *err = "mixer: the launch set does not fit one job table"; return rc; }
  const uint32_t total = fb[(size_t)n];
  if (total == 0) return MI355_OK;
  // [first_block | jobs | segs | outs | bits], each part at a multiple of 16 bytes
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t o_fb = 0, o_jobs = up(o_fb + ((size_t)n + 1) * 4), o_segs = up(o_jobs + (size_t)n * sizeof(MixJob)),
               o_outs = up(o_segs + (size_t)so[(size_t)n] * sizeof(MixSeg)), o_bits = up(o_outs + (size_t)oo[(size_t)n] * sizeof(MixOut)),
               bytes = up(o_bits + (size_t)bo[(size_t)n] * 2);
  const int k = B->use;
  if ((rc = mix_hip(hipEventSynchronize(B->ev[k]), "hipEventSynchronize(mixer tables)", err))) return rc;
  if (bytes > B->cap) {
    (void)hipStreamSynchronize(stream);   // the launch that reads the old device image is over, and so are the copies out of the pinned ones
    if (B->h) (void)hipHostFree(B->h);
    if (B->d) (void)hipFree(B->d);
    B->h = B->d = nullptr; B->cap = 0;
    size_t cap = 16384;
    while (cap < bytes) cap *= 2;
    if ((rc = mix_hip(hipHostMalloc((void **)&B->h, 2 * cap, hipHostMallocDefault), "hipHostMalloc(mixer tables)", err))) return rc;
    if ((rc = mix_hip(hipMalloc((void **)&B->d, cap), "hipMalloc(mixer tables)", err))) return rc;
    B->cap = cap;
  }
  char *h = B->h + (size_t)k * B->cap;
  std::memcpy(h + o_fb, fb.data(), ((size_t)n + 1) * 4);
  MixJob *jobs = (MixJob *)(h + o_jobs);
  MixSeg *segs = (MixSeg *)(h + o_segs);
  MixOut *outs = (MixOut *)(h + o_outs);
  uint16_t *bits = (uint16_t *)(h + o_bits);
  for (int j = 0; j < n; j++) {
    const MixerCall &c = calls[j];
    MixJob &J = jobs[j];
    J.n_groups = mix_groups(c.n_out_channels); J.n_segs = c.n_segs; J.n_outs = c.n_outs; J.frames = (uint32_t)c.frames;
    J.seg_off = so[j]; J.out_off = oo[j]; J.bits_off = bo[j]; J.pad = 0;
    for (unsigned s = 0; s < c.n_segs; s++) segs[so[j] + s] = MixSeg{c.segs[s].data, c.segs[s].input, c.segs[s].format, c.segs[s].out_offset, c.segs[s].num_frames};
    for (unsigned o = 0; o < c.n_outs; o++) outs[oo[j] + o] = MixOut{c.outs[o].data, c.outs[o].format, c.outs[o].channel_offset, c.outs[o].n_channels, 0};
    std::memcpy(bits + bo[j], c.bits, (size_t)c.n_inputs * J.n_groups * 2);
  }
  if ((rc = mix_hip(hipMemcpyAsync(B->d, h, bytes, hipMemcpyHostToDevice, stream), "mixer: job tables", err))) return rc;
  if ((rc = mix_hip(hipEventRecord(B->ev[k], stream), "hipEventRecord(mixer tables)", err))) return rc;
  B->use = k ^ 1;
  MixTables T;
  T.first_block = (const uint32_t *)(B->d + o_fb);
  T.jobs = (const MixJob *)(B->d + o_jobs);
  T.segs = (const MixSeg *)(B->d + o_segs);
  T.outs = (const MixOut *)(B->d + o_outs);
  T.bits = (const uint16_t *)(B->d + o_bits);
  T.n_jobs = (uint32_t)n;
  hipLaunchKernelGGL(mixer_kernel, dim3(total), dim3(256), 0, stream, T);
  if ((rc = mix_hip(hipGetLastError(), "mixer kernel launch", err))) return rc;
  if (kernel_launches) *kernel_launches = 1;
  return MI355_OK;
}

// ---------------------------------------------------------------- one mixer on a context

struct MixerState {
  unsigned n_inputs = 0, n_out = 0;
  std::vector<uint16_t> bits;
  MixerTablesBuf *tables = nullptr;
  // the host form's slots: pinned + device, input and output side
  char *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr;
  size_t in_cap = 0, out_cap = 0;
};

void mixer_release(mi355_ctx *ctx) {
  auto *s = static_cast<MixerState *>(ctx->mixer);
  if (!s) return;
  mixer_tables_free(s->tables);
  if (s->h_in) (void)hipHostFree(s->h_in);
  if (s->d_in) (void)hipFree(s->d_in);
  if (s->h_out) (void)hipHostFree(s->h_out);
  if (s->d_out) (void)hipFree(s->d_out);
  delete s;
  ctx->mixer = nullptr;
}

static int mixer_ctx_setup(mi355_ctx *ctx, unsigned n_inputs, unsigned n_out, const uint8_t *contrib) {
  const char *why = "";
  int rc = mixer_check_setup(n_inputs, n_out, &why);
  if (rc) return set_error(ctx, rc, why);
  if ((rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
  auto *s = static_cast<MixerState *>(ctx->mixer);
  if (!s) {
    s = new MixerState();
    std::string err;
    s->tables = mixer_tables_new(&err, &rc);
    if (!s->tables) { delete s; return set_error(ctx, rc, err); }
    ctx->mixer = s;
  }
  // (the matrix travels with every launch's tables: an interval already enqueued keeps the one it was given)
  s->n_inputs = n_inputs;
  s->n_out = n_out;
  mixer_pack_contrib(n_inputs, n_out, contrib, &s->bits);
  return MI355_OK;
}

static int mixer_ctx_check(mi355_ctx *ctx, const mi355_mixer_segment *segs, unsigned n_segs, const mi355_mixer_output *outs, unsigned n_outs, size_t frames,
                           bool device, MixerState **out) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  auto *s = static_cast<MixerState *>(ctx->mixer);
  if (!s) return set_error(ctx, MI355_ERR_NOT_CONFIGURED, "mixer: not configured (setup not called)");
  const char *why = "";
  const int rc = mixer_check(s->n_inputs, s->n_out, segs, n_segs, outs, n_outs, frames, device, &why);
  if (rc) return set_error(ctx, rc, why);
  *out = s;
  return check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
}

static int mixer_ctx_enqueue(mi355_ctx *ctx, MixerState *s, const mi355_mixer_segment *segs, unsigned n_segs, const mi355_mixer_output *outs, unsigned n_outs,
                             size_t frames) {
  MixerCall c{s->n_inputs, s->n_out, s->bits.data(), segs, n_segs, outs, n_outs, frames};
  std::string err;
  const int rc = mixer_launch(s->tables, ctx->stream, &c, 1, nullptr, &err);
  return rc ? set_error(ctx, rc, err) : MI355_OK;
}

static int mixer_grow(mi355_ctx *ctx, char **h, char **d, size_t *cap, size_t need, const char *what) {
  if (need <= *cap) return MI355_OK;
  (void)hipStreamSynchronize(ctx->stream);
  if (*h) (void)hipHostFree(*h);
  if (*d) (void)hipFree(*d);
  *h = *d = nullptr; *cap = 0;
  size_t c = 4096;
  while (c < need) c *= 2;
  int rc = check_hip(ctx, hipHostMalloc((void **)h, c, hipHostMallocDefault), what);
  if (!rc) rc = check_hip(ctx, hipMalloc((void **)d, c), what);
  if (rc) return rc;
  *cap = c;
  return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_mixer_setup(mi355_ctx *ctx, unsigned n_inputs, unsigned n_out_channels, const uint8_t *contrib) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  if (!contrib) return set_error(ctx, MI355_ERR_INVALID_ARG, "mixer: null contribution matrix");
  return mixer_ctx_setup(ctx, n_inputs, n_out_channels, contrib);
}

int mi355_mixer_setup_minus1(mi355_ctx *ctx, unsigned n_streams) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  return mixer_ctx_setup(ctx, n_streams, n_streams, nullptr);
}

int mi355_mixer_reset(mi355_ctx *ctx) {
  if (!ctx) return MI355_ERR_INVALID_ARG;
  const int rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  if (rc) return rc;
  (void)hipStreamSynchronize(ctx->stream);
  mixer_release(ctx);
  return MI355_OK;
}

int mi355_mixer_process_device(mi355_ctx *ctx, const mi355_mixer_segment *segments, unsigned n_segments, const mi355_mixer_output *outputs,
                               unsigned n_outputs, size_t frames) {
  MixerState *s = nullptr;
  const int rc = mixer_ctx_check(ctx, segments, n_segments, outputs, n_outputs, frames, true, &s);
  if (rc) return rc;
  return mixer_ctx_enqueue(ctx, s, segments, n_segments, outputs, n_outputs, frames);
}

int mi355_mixer_process(mi355_ctx *ctx, const mi355_mixer_segment *segments, unsigned n_segments, const mi355_mixer_output *outputs, unsigned n_outputs,
                        size_t frames) {
  MixerState *s = nullptr;
  int rc = mixer_ctx_check(ctx, segments, n_segments, outputs, n_outputs, frames, false, &s);
  if (rc) return rc;
  if (frames == 0 || n_outputs == 0) return MI355_OK;
  MixerLayout L;
  mixer_layout(segments, n_segments, outputs, n_outputs, frames, &L);
  if ((rc = mixer_grow(ctx, &s->h_in, &s->d_in, &s->in_cap, L.in_bytes, "mixer: input staging"))) return rc;
  if ((rc = mixer_grow(ctx, &s->h_out, &s->d_out, &s->out_cap, L.out_bytes_total, "mixer: output staging"))) return rc;
  std::vector<mi355_mixer_segment> segs(segments, segments + n_segments);
  std::vector<mi355_mixer_output> outs(outputs, outputs + n_outputs);
  for (unsigned i = 0; i < n_segments; i++) {
    if (L.seg_bytes[i]) std::memcpy(s->h_in + L.seg_off[i], segments[i].data, L.seg_bytes[i]);
    segs[i].data = s->d_in + L.seg_off[i];
  }
  for (unsigned o = 0; o < n_outputs; o++) outs[o].data = s->d_out + L.out_off[o];
  if (L.in_bytes) {
    if ((rc = check_hip(ctx, hipMemcpyAsync(s->d_in, s->h_in, L.in_bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(H2D audio)"))) return rc;
    ctx->n_h2d++;
  }
  if ((rc = mixer_ctx_enqueue(ctx, s, segs.data(), n_segments, outs.data(), n_outputs, frames))) return rc;
  if ((rc = check_hip(ctx, hipMemcpyAsync(s->h_out, s->d_out, L.out_bytes_total, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(D2H audio)"))) return rc;
  ctx->n_d2h++;
  if ((rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "mixer: stream synchronize"))) return rc;
  for (unsigned o = 0; o < n_outputs; o++) std::memcpy(outputs[o].data, s->h_out + L.out_off[o], L.out_bytes[o]);
  return MI355_OK;
}

int mi355_selftest_mixer_plan(int n_members, const uint32_t *n_inputs, const uint32_t *n_out_channels, const uint32_t *n_segments,
                              const uint32_t *n_outputs, const uint64_t *frames, uint32_t *first_block, uint32_t *seg_offset, uint32_t *out_offset,
                              uint32_t *bits_offset, uint32_t block_capacity, uint32_t *block_member, uint32_t *block_tile, uint32_t *block_group) {
  const int rc = mixer_plan(n_members, n_inputs, n_out_channels, n_segments, n_outputs, frames, first_block, seg_offset, out_offset, bits_offset);
  if (rc) return rc;
  if (!block_member && !block_tile && !block_group) return MI355_OK;
  if (!block_member || !block_tile || !block_group || first_block[n_members] > block_capacity) return MI355_ERR_INVALID_ARG;
  std::vector<uint32_t> groups((size_t)n_members);
  for (int j = 0; j < n_members; j++) groups[(size_t)j] = mix_groups(n_out_channels[j]);
  for (uint32_t b = 0; b < first_block[n_members]; b++) {
    const uint32_t j = mixer_locate(first_block, (uint32_t)n_members, b);
    block_member[b] = j;
    mixer_split(b - first_block[j], groups[j], &block_tile[b], &block_group[b]);
  }
  return MI355_OK;
}

}  // extern "C"

// agroup.hip — independent AUDIO element instances that share launches: the dispatcher behind mi355_agroup_*.
//
// The reference runs one element instance per stream and hands it ONE buffer per call: rsaudioecho's transform_ip
// (audio/audiofx/src/audioecho/imp.rs:205-227), ebur128level's (audio/audiofx/src/ebur128level/imp.rs:682-745), audioloudnorm's
// sink_chain -> drain_full_frames -> State::process per 100 ms frame (audio/audiofx/src/audioloudnorm/imp.rs:1545-1586, :226-268).
// One such buffer is a few thousand samples: on a GPU a single instance is launch- and round-trip-bound (one context per
// instance: echo 0.22 ms per 32-instance interval where one CPU core needs 0.17; audioloudnorm 57x real time against 86x), while
// the `_batch` kernels of this library advance hundreds of streams per launch (echo 0.014 ms, loudnorm 1,658x aggregate). Those
// entry points need one caller that owns all streams; a process full of independent elements has none. An agroup is that caller:
//   * members = element instances of ONE kind and configuration on one device (a transcoding farm's N identical pipelines);
//   * each member submits its buffer of the interval from its own streaming thread and waits for its ticket;
//   * the batch runs when every attached member has submitted (whoever completes the set runs it), ONE launch set for all;
//   * members are independent: rsaudioecho - own ring, position, buffer size and parameters per submit (a job table); agingradio -
//     own setup (channels, rate, lowpass, seed), filter states and pair counter, buffer size, sample type and settings per submit
//     (agingradio.hip's job table); hrtfrender - own sphere (shared by content), channel count, block-length, interpolation-steps and
//     convolution form per member, own tails and previous directions (hrtf_kernels.hip's job tables: HrtfRender::process,
//     audio/hrtf/src/hrtf/imp.rs:164-278, for every member that has a block in ONE launch set); sofalizer - own channel count, filter
//     length, partition-length and block-length per member, own filter spectra, delay lines and drop flags, filters queued at
//     set_filter and transformed with the member's next launch set (sofa_kernels.hip's job tables: the block loop of
//     Sofalizer::process, audio/hrtf/src/sofa/imp.rs:235-322, for every member that has blocks in ONE launch set); minus1mixer /
//     audiomultimixer - a member is one mixer (one room of a bridge server) with its own contribution matrix, segment list, output
//     formats and frames per submit (mixer.hip's job tables: aggregate_one_buffer, audio/audiomultimixer/src/audiomultimixerelement.rs:606-753,
//     and split_output_buf, audio/audiomultimixer/src/splitter.rs:433-467, for every member that has submitted in ONE kernel launch);
//     ebur128level - own buffer size, 100 ms phase and `reset` (per-stream rounds in ebur128_kernels.hip); audioloudnorm - own frame
//     type and ring positions (loudnorm.hip: a launch sequence per CLASS of members that stand at the same frame type and size:
//     streams that started together are one class). A waiter that has lingered `linger_us` launches whoever is there: a member that
//     is late, paused or gone costs the others one linger, never a hang, and is never fed silence;
//   * per-member results are those of a single-instance context fed the same buffers, bit for bit (tests/test_gpu_agroup.py).
// No persistent kernel, nothing on the device waits for the host.
#include "internal.hpp"

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

using namespace mi355;

namespace mi355 {

// ---------------------------------------------------------------- rsaudioecho through a job table
// The arithmetic is echo_kernels.hip's (AudioEcho::process, audioecho/imp.rs:69-85 with RingBufferIter, ring_buffer.rs:37-82:
// e = ring[read]; out = inp + intensity * e; ring[write] = inp + feedback * e, f64, unfused), per job instead of per batch slot:
// every job carries its own buffer, ring, position, length and parameters.
struct EchoJob {
  void *data;
  double *w, *ring;
  unsigned long long n, size, pos, D;
  double intensity, feedback;
  int is_f64, pad;
};

template <typename T>
__device__ __forceinline__ void echo_job_widen(const EchoJob &J) {
  const T *data = (const T *)J.data;
  const size_t gs = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < J.n; i += gs) J.w[i] = (double)data[i];
}

__global__ __launch_bounds__(256) void echo_jobs_widen_kernel(const EchoJob *__restrict__ jobs) {
  const EchoJob J = jobs[blockIdx.y];
  if (J.feedback != 0.0) return;  // the chain form widens as it goes
  if (J.is_f64) echo_job_widen<double>(J); else echo_job_widen<float>(J);
}

template <typename T>
__device__ __forceinline__ void echo_job_main(const EchoJob &J) {
  T *data = (T *)J.data;
  const size_t n = J.n, size = J.size, pos = J.pos, D = J.D;
  const size_t gs = (size_t)gridDim.x * blockDim.x;
  if (J.feedback == 0.0) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {
      const double e = (i < D) ? J.ring[(pos + i + size - D) % size] : J.w[i - D];
      const double out = J.w[i] + J.intensity * e;
      data[i] = (T)out;
    }
  } else {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < D && t < n; t += gs) {
      double e = J.ring[(pos + t + size - D) % size];
      for (size_t i = t; i < n; i += D) {
        const double inp = (double)data[i];
        const double out = inp + J.intensity * e;
        const double wv = inp + J.feedback * e;
        data[i] = (T)out;
        J.w[i] = wv;
        e = wv;
      }
    }
  }
}

__global__ __launch_bounds__(256) void echo_jobs_main_kernel(const EchoJob *__restrict__ jobs) {
  const EchoJob J = jobs[blockIdx.y];
  if (J.is_f64) echo_job_main<double>(J); else echo_job_main<float>(J);
}

__global__ __launch_bounds__(256) void echo_jobs_commit_kernel(const EchoJob *__restrict__ jobs) {
  const EchoJob J = jobs[blockIdx.y];
  const size_t first = J.n > J.size ? J.n - J.size : 0;
  const size_t gs = (size_t)gridDim.x * blockDim.x;
  for (size_t i = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < J.n; i += gs) J.ring[(J.pos + i) % J.size] = J.w[i];
}

}  // namespace mi355

namespace {

enum { KIND_ECHO = 1, KIND_EBUR128 = 2, KIND_LOUDNORM = 3, KIND_AGING = 4, KIND_HRTF = 5, KIND_SOFA = 6, KIND_MIXER = 7 };

// a member's life cycle: at most ONE buffer is outstanding, its ticket is collected once, and nothing else of the member moves in between
//   IDLE -> FILLING (submit accepted; the buffer is on its way into the staging slot, possibly outside the lock) -> SUBMITTED (it
//   counts for the launch set being collected) -> RAN (the set has run; the result waits for wait(ticket)) -> COLLECTING (wait is
//   copying it out, possibly outside the lock) -> IDLE.
// Every submit_* and every setup / reset / load call of a member is refused unless the member is IDLE (check_member); wait takes
// only the ticket of the SUBMITTED or RAN buffer. detach drops a buffer that has not run; a result that has is still collected once.
enum { M_IDLE = 0, M_FILLING, M_SUBMITTED, M_RAN, M_COLLECTING };

struct Sub {   // one member's submission: the buffer it has outstanding
  int state = M_IDLE;
  bool have() const { return state == M_SUBMITTED; }   // part of the launch set being collected
  bool device = false;
  void *data = nullptr;      // caller's buffer (echo: in place; ebur128: input; loudnorm: input)
  void *out = nullptr;       // loudnorm / hrtfrender / sofalizer: caller's output buffer
  size_t n = 0;              // echo: interleaved samples; ebur128 / loudnorm / agingradio / hrtfrender / sofalizer / mixer: frames
  size_t bytes = 0;          // echo / agingradio: the buffer in bytes (they work in place: what goes up comes down)
  size_t out_cap = 0;        // loudnorm: capacity of `out` in frames
  int fmt = 0;               // echo / agingradio: is_f64; ebur128: sample format
  int final_frame = 0;       // loudnorm
  int n_blocks = 0;          // sofalizer: whole blocks in this buffer
  size_t delay = 0;
  double intensity = 0, feedback = 0;
  mi355_agingradio_settings ar{};   // agingradio: the settings transform_ip snapshotted for this buffer
  uint64_t interval = 0;     // the interval this submission belongs to
};

struct AgingMember {         // one agingradio instance's state (AudioFilterImpl::setup, agingradio/imp.rs:326-345)
  bool configured = false;
  unsigned channels = 0;
  double alpha = 0;
  double *d_state = nullptr; // lowpass output per channel; nullptr: lowpass-freq 0 at setup
  unsigned long long k = 0, seed = 0;   // frame pairs processed since setup; Philox key
};

struct MixerMember {         // one mixer: its matrix (mixer_setup) and what its outstanding submit carries
  bool configured = false;
  unsigned n_inputs = 0, n_out = 0;
  std::vector<uint16_t> bits;                // mixer_pack_contrib's words
  std::vector<mi355_mixer_segment> segs;     // copied at submit; a host member's `data` is resolved against its slot when the set runs
  std::vector<mi355_mixer_output> outs;      // copied at submit; `data` stays the caller's buffer (a host member's is filled by wait)
  MixerLayout layout;                        // host members: where the buffers sit in the member's input and output slot
};

struct Slab {                // one side of the staging: a slot of `cap` bytes per member, pinned host + device
  char *h = nullptr, *d = nullptr;
  size_t cap = 0;
};

struct JobTable {            // echo / agingradio: the job table of a launch set
  void *h = nullptr, *d = nullptr;   // the pinned block the host fills, the device block the kernels read
  hipEvent_t ready = nullptr;        // the job table of the previous launch set has left the pinned block
};

// What a kind is to the dispatcher. A new kind = one row of kKinds, its run_* and its create / submit entry points.
struct Kind {
  const char *name;                  // in the texts of HIP failures: "agroup <name>: <step>"
  int (*run)(mi355_agroup *);        // one launch set for the members that have submitted; g->mu held
  bool out_row_is_slot;              // a member's row of the output slab is the slot itself (else: the slot rounded down to whole frames)
  bool result_in_slab;               // a host member's result stays in a slab until wait collects it
  // wait: the member's result from its row to its buffer(s); nullptr: nothing to copy
  int (*copy_out)(mi355_agroup *, std::unique_lock<std::mutex> &, int member, size_t frames);
};
const Kind &kind_of(const mi355_agroup *g);

}  // namespace

struct mi355_agroup {
  int device = 0, kind = 0, n_members = 0;
  mi355_ctx *ctx = nullptr;   // the batch context: its stream carries every launch of the group
  std::mutex mu;
  std::condition_variable cv;
  std::string last_error;
  std::vector<char> attached;
  std::vector<Sub> sub;
  uint64_t interval = 1;      // the interval being collected; intervals < this one are complete
  unsigned linger_us = 0;     // echo: how long a waiter lingers for the missing members before it launches without them
  unsigned timeout_ms = 0;    // (accepted and ignored since every kind's members are independent: nobody waits for a member that does not come)
  // results of each member's last completed interval
  std::vector<int> res_status;
  std::vector<size_t> res_frames;
  std::vector<uint64_t> res_interval;
  uint64_t n_batches = 0, n_buffers = 0, n_largest = 0;
  int copying = 0;            // members that are copying between their buffer and their staging slot right now (outside the lock)
  std::vector<char> res_pending;   // [member]: a host member's result of a launch set that ran sits in the slabs and has not been collected
  Slab in, out;               // staging: input and (loudnorm, hrtfrender, sofalizer, mixer) output
  JobTable jobs;              // echo / agingradio
  // ---- echo
  size_t ring_len = 0;
  double *d_rings = nullptr, *d_w = nullptr;
  size_t w_cap = 0;                 // doubles per member in d_w
  std::vector<size_t> pos;          // per-member ring position
  // ---- agingradio
  std::vector<AgingMember> aging;
  // ---- hrtfrender
  HrtfGroup *hrtf = nullptr;        // the members' spheres, processors and job tables (hrtf_kernels.hip)
  std::vector<float> hrtf_pg;       // [member][4 * 64]: positions [C][3] then gains [C], copied at submit
  // ---- sofalizer
  SofaGroup *sofa = nullptr;        // the members' convolvers, filter queue and job tables (sofa_kernels.hip)
  std::vector<float> sofa_g;        // [member][64]: gains [C], copied at submit
  // ---- minus1mixer / audiomultimixer
  std::vector<MixerMember> mixer;
  MixerTablesBuf *mix_tables = nullptr;   // the job tables of a launch set (mixer.hip)
  uint64_t mix_launches = 0;
  // ---- ebur128
  unsigned channels = 0;
  int set_fmt = -1;                 // ebur128: the sample format of the launch set being collected, fixed by the first member accepted into it
  uint64_t query_interval[5] = {0, 0, 0, 0, 0};   // ebur128: the interval the cached answers below belong to
  std::vector<double> query_cache[5];
  uint64_t peak_interval[2] = {0, 0};
  std::vector<double> peak_cache[2];
  // ---- loudnorm
  std::vector<std::vector<double>> adapter;   // mi355_agroup_loudnorm_push: what a member has pushed and not yet handed over as a whole frame
  // ---- process-wide registry (mi355_agroup_shared_*): what the group was made from, members handed out, members released
  std::string shared_key;
  int handed_out = 0, released = 0;
};

namespace {

const size_t kEburSampleBytes[4] = {2, 4, 4, 8};   // ebur128's sample formats: s16, s32, f32, f64
const size_t kCopyUnderLock = 65536;               // (a 10 ms audio buffer is a few KB: cheaper than giving the lock away and taking it again)

int afail(mi355_agroup *g, int status, const std::string &msg) {
  g->last_error = msg;
  return status;
}

int ahip(mi355_agroup *g, hipError_t e, const char *what) {
  if (e == hipSuccess) return MI355_OK;
  (void)hipGetLastError();
  g->last_error = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? MI355_ERR_OUT_OF_MEMORY : MI355_ERR_HIP;
}

// a step of a launch set: its failure reads "agroup <kind>: <step>: <HIP's text>"
int astep(mi355_agroup *g, hipError_t e, const char *step) {
  if (e == hipSuccess) return MI355_OK;
  return ahip(g, e, (std::string("agroup ") + kind_of(g).name + ": " + step).c_str());
}

// the tail of a call into a sub-engine: one that reports through an error string, one that reports through the batch context
int asub(mi355_agroup *g, int rc, const std::string &err) { return rc ? afail(g, rc, err) : MI355_OK; }
int actx(mi355_agroup *g, int rc) {
  if (rc) g->last_error = g->ctx->last_error;
  return rc;
}

// ---------------------------------------------------------------- staging
// What moves along when a slab is replaced: the rows of the members `live` names, row(cap) bytes apart in a slab of `cap` bytes per member.
struct Keep {
  bool (*live)(const mi355_agroup *, int member);
  size_t (*row)(const mi355_agroup *, size_t cap);
};

// The row widths, here and nowhere else. An input row is the slot. An output row: hrtfrender's and sofalizer's output is stereo f32
// whatever the member's input channels are, and its row is the slot itself; so is a mixer's, which packs its outputs' buffers into
// it; loudnorm's (and whoever else has channels) is the slot rounded down to whole frames of `channels` doubles.
size_t in_row(const mi355_agroup *, size_t cap) { return cap; }
size_t out_row(const mi355_agroup *g, size_t cap) {
  const size_t fb = (size_t)g->channels * 8;
  return kind_of(g).out_row_is_slot || !fb ? cap : cap / fb * fb;
}

// input rows: submissions already copied in move along, and so do results that their members have not collected yet (rsaudioecho and
// agingradio work in place: the result of a member sits in its input slot). Output rows: the results not collected yet.
bool in_live(const mi355_agroup *g, int m) { return (g->sub[m].have() && !g->sub[m].device) || g->res_pending[(size_t)m]; }
bool out_live(const mi355_agroup *g, int m) { return g->res_pending[(size_t)m] != 0; }
const Keep kKeepIn = {in_live, in_row}, kKeepOut = {out_live, out_row};

// Slots of at least `need` bytes per member. A slab is replaced only while no copy runs on it (copying == 0: wait() and the submits
// copy outside the lock, copy_unlocked) and no launch is in flight (the stream drained); what it holds of members' business moves
// along, each row at the row width of the old slab to its place at the row width of the new one (round 6's stress run caught a
// result read from a slab another member's larger buffer had just replaced).
int slab_grow(mi355_agroup *g, std::unique_lock<std::mutex> &lk, Slab &s, size_t need, const char *what, const Keep &keep) {
  if (need <= s.cap) return MI355_OK;
  g->cv.wait(lk, [g] { return g->copying == 0; });   // nobody is writing into the old slots or reading from them
  if (need <= s.cap) return MI355_OK;                // (the lock was away: somebody else has grown it)
  (void)hipStreamSynchronize(g->ctx->stream);
  Slab n;
  n.cap = 4096;
  while (n.cap < need && n.cap < ((size_t)1 << 20)) n.cap *= 2;
  if (n.cap < need) n.cap = (need + 4095) & ~(size_t)4095;   // (large slots - a 3 s first frame - are sized exactly: they are pinned memory)
  int rc = ahip(g, hipHostMalloc((void **)&n.h, n.cap * (size_t)g->n_members, hipHostMallocDefault), (std::string("hipHostMalloc(") + what + ")").c_str());
  if (rc) return rc;
  if ((rc = ahip(g, hipMalloc((void **)&n.d, n.cap * (size_t)g->n_members), (std::string("hipMalloc(") + what + ")").c_str()))) { (void)hipHostFree(n.h); return rc; }
  if (s.h) {
    const size_t old_row = keep.row(g, s.cap), new_row = keep.row(g, n.cap);
    for (int m = 0; m < g->n_members; m++)
      if (keep.live(g, m)) std::memcpy(n.h + (size_t)m * new_row, s.h + (size_t)m * old_row, old_row);
  }
  if (s.h) (void)hipHostFree(s.h);
  if (s.d) (void)hipFree(s.d);
  s = n;
  return MI355_OK;
}

int ensure_staging(mi355_agroup *g, std::unique_lock<std::mutex> &lk, size_t need, size_t out_need) {
  if (int rc = slab_grow(g, lk, g->in, need, "agroup staging", kKeepIn)) return rc;
  return slab_grow(g, lk, g->out, out_need, "agroup output staging", kKeepOut);
}

char *in_slot(const mi355_agroup *g, int member) { return g->in.h + (size_t)member * g->in.cap; }

// Runs `copy` - the memcpy(s) between a member's buffer and its staging row - under the lock when it moves at most `threshold` bytes,
// else outside it (32 members copying 9 MB first frames one after the other would be the longest thing in the interval). The count
// pins the slabs in place while the lock is away: slab_grow replaces none before it is back at 0. The caller has marked the member
// busy (FILLING / COLLECTING), so its row and its buffers are nobody else's. `lk` owns g->mu on entry and on return.
template <typename Copy>
void copy_unlocked(mi355_agroup *g, std::unique_lock<std::mutex> &lk, size_t bytes, size_t threshold, Copy copy) {
  if (bytes <= threshold) { copy(); return; }
  g->copying++;
  lk.unlock();
  copy();
  lk.lock();
  g->copying--;
  g->cv.notify_all();
}

// ---------------------------------------------------------------- launch sets
typedef std::vector<std::pair<int, int>> Runs;   // [first, last] member of each run

// The runs of consecutive HOST members for which pred(member) holds: their rows go up and come down in ONE strided copy per run -
// normally one for all of them. A run - and so a copy - never spans the slot of a member that is not part of the launch set: that
// member may be filling its slot for the next set at this very moment, or its row may hold a result it has not collected yet, from
// an older slab than the device one (slab_grow).
template <typename Pred>
Runs host_runs(const mi355_agroup *g, Pred pred) {
  Runs runs;
  for (int m = 0; m < g->n_members; m++) {
    if (!pred(m) || g->sub[m].device) continue;
    if (!runs.empty() && runs.back().second == m - 1) runs.back().second = m;
    else runs.push_back({m, m});
  }
  return runs;
}

Runs set_runs(const mi355_agroup *g) {   // the host members of the launch set being run
  return host_runs(g, [g](int m) { return g->sub[m].have(); });
}

std::vector<int> set_members(const mi355_agroup *g) {
  std::vector<int> who;
  for (int m = 0; m < g->n_members; m++)
    if (g->sub[m].have()) who.push_back(m);
  return who;
}

// one strided copy per run between the pinned and the device side of `s`, rows `row` bytes apart, `width` bytes of each; none at width 0
int copy_runs(mi355_agroup *g, const Slab &s, size_t row, const Runs &runs, size_t width, hipMemcpyKind dir) {
  if (width == 0) return MI355_OK;
  const bool up = dir == hipMemcpyHostToDevice;
  for (const auto &r : runs) {
    char *h = s.h + (size_t)r.first * row, *d = s.d + (size_t)r.first * row;
    if (int rc = astep(g, hipMemcpy2DAsync(up ? d : h, row, up ? h : d, row, width, (size_t)(r.second - r.first + 1), dir, g->ctx->stream), up ? "upload" : "download")) return rc;
  }
  return MI355_OK;
}

int jobs_create(mi355_agroup *g, size_t bytes) {
  const std::string what = std::string("(agroup ") + kind_of(g).name + " jobs)";
  int rc = ahip(g, hipMalloc(&g->jobs.d, bytes), ("hipMalloc" + what).c_str());
  if (!rc) rc = ahip(g, hipHostMalloc(&g->jobs.h, bytes, hipHostMallocDefault), ("hipHostMalloc" + what).c_str());
  if (!rc) rc = ahip(g, hipEventCreateWithFlags(&g->jobs.ready, hipEventDisableTiming), "hipEventCreate(agroup)");
  return rc;
}

// the pinned block is the host's to fill once the previous set's table has left it; then the table goes up and the event is set anew
int jobs_begin(mi355_agroup *g) { return ahip(g, hipEventSynchronize(g->jobs.ready), "hipEventSynchronize(agroup jobs)"); }
int jobs_upload(mi355_agroup *g, size_t bytes) {
  if (int rc = astep(g, hipMemcpyAsync(g->jobs.d, g->jobs.h, bytes, hipMemcpyHostToDevice, g->ctx->stream), "job table")) return rc;
  return ahip(g, hipEventRecord(g->jobs.ready, g->ctx->stream), "hipEventRecord(agroup jobs)");
}

unsigned blocks_for(size_t n, int n_cu, int share) {
  size_t b = (n + 255) / 256;
  size_t cap = (size_t)n_cu * 8 / (size_t)(share > 0 ? share : 1);
  if (cap < 1) cap = 1;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

size_t widest_host_buffer(const mi355_agroup *g, const std::vector<int> &who) {   // echo / agingradio
  size_t w = 0;
  for (int m : who)
    if (!g->sub[m].device && g->sub[m].bytes > w) w = g->sub[m].bytes;
  return w;
}

// ---- rsaudioecho: one job per member that has submitted. Host members: their samples are in the pinned slots already (submit
// copied them) and work in place there.
int run_echo(mi355_agroup *g) {
  const std::vector<int> who = set_members(g);
  if (who.empty()) return MI355_OK;
  const size_t max_host = widest_host_buffer(g, who);
  size_t max_n = 0;
  for (int m : who)
    if (g->sub[m].n > max_n) max_n = g->sub[m].n;
  hipStream_t st = g->ctx->stream;
  int rc = MI355_OK;
  if (max_n > g->w_cap) {   // the scratch W[member][n]
    (void)hipStreamSynchronize(st);
    if (g->d_w) (void)hipFree(g->d_w);
    g->d_w = nullptr; g->w_cap = 0;
    size_t cap = 1024;
    while (cap < max_n) cap *= 2;
    if ((rc = ahip(g, hipMalloc((void **)&g->d_w, cap * 8 * (size_t)g->n_members), "hipMalloc(agroup echo scratch)"))) return rc;
    g->w_cap = cap;
  }
  const Runs runs = set_runs(g);
  if ((rc = copy_runs(g, g->in, g->in.cap, runs, max_host, hipMemcpyHostToDevice))) return rc;
  if ((rc = jobs_begin(g))) return rc;
  EchoJob *jobs = (EchoJob *)g->jobs.h;
  size_t widest = 1, widest_chain = 1;
  bool any_nofb = false;
  for (size_t j = 0; j < who.size(); j++) {
    const int m = who[j];
    const Sub &s = g->sub[m];
    EchoJob &J = jobs[j];
    J.data = s.device ? s.data : (void *)(g->in.d + (size_t)m * g->in.cap);
    J.w = g->d_w + (size_t)m * g->w_cap;
    J.ring = g->d_rings + (size_t)m * g->ring_len;
    J.n = s.n; J.size = g->ring_len; J.pos = g->pos[m];
    J.D = s.delay == 0 ? g->ring_len : s.delay;   // read == write index: the slot written `size` samples ago (ring_buffer.rs:44-45)
    J.intensity = s.intensity; J.feedback = s.feedback; J.is_f64 = s.fmt; J.pad = 0;
    if (s.feedback == 0.0) { any_nofb = true; if (s.n > widest_chain) widest_chain = s.n; }
    else { const size_t chains = J.D < s.n ? (size_t)J.D : s.n; if (chains > widest_chain) widest_chain = chains; }
    if (s.n > widest) widest = s.n;
  }
  const unsigned J = (unsigned)who.size();
  if ((rc = jobs_upload(g, J * sizeof(EchoJob)))) return rc;
  const EchoJob *d_jobs = (const EchoJob *)g->jobs.d;
  const unsigned gb = blocks_for(widest, g->ctx->n_cu, (int)J), mb = blocks_for(widest_chain, g->ctx->n_cu, (int)J);
  if (any_nofb) hipLaunchKernelGGL(echo_jobs_widen_kernel, dim3(gb, J), dim3(256), 0, st, d_jobs);
  hipLaunchKernelGGL(echo_jobs_main_kernel, dim3(mb, J), dim3(256), 0, st, d_jobs);
  hipLaunchKernelGGL(echo_jobs_commit_kernel, dim3(gb, J), dim3(256), 0, st, d_jobs);
  if ((rc = astep(g, hipGetLastError(), "kernel launch"))) return rc;
  if ((rc = copy_runs(g, g->in, g->in.cap, runs, max_host, hipMemcpyDeviceToHost))) return rc;
  if ((rc = astep(g, hipStreamSynchronize(st), "sync"))) return rc;
  for (int m : who) g->pos[m] = (g->pos[m] + g->sub[m].n) % g->ring_len;   // RingBufferIter::drop (ring_buffer.rs:78-82)
  return MI355_OK;
}

// ---- agingradio: one job per member that has submitted (agingradio.hip), each with its own buffer, sample type, settings, filter
// states and pair counter. Host members go through their staging slots as echo members do.
int run_aging(mi355_agroup *g) {
  const std::vector<int> who = set_members(g);
  if (who.empty()) return MI355_OK;
  const size_t max_host = widest_host_buffer(g, who);
  hipStream_t st = g->ctx->stream;
  int rc = MI355_OK;
  const Runs runs = set_runs(g);
  if ((rc = copy_runs(g, g->in, g->in.cap, runs, max_host, hipMemcpyHostToDevice))) return rc;
  if ((rc = jobs_begin(g))) return rc;
  AgingJob *jobs = (AgingJob *)g->jobs.h;
  for (size_t j = 0; j < who.size(); j++) {
    const int m = who[j];
    const Sub &s = g->sub[m];
    const AgingMember &A = g->aging[(size_t)m];
    AgingJob &J = jobs[j];
    J = AgingJob{};
    agingradio_settings_to_job(s.ar, &J);
    J.data = s.device ? s.data : (void *)(g->in.d + (size_t)m * g->in.cap);
    J.state = A.d_state;
    J.frames = s.n; J.k0 = A.k; J.seed = A.seed; J.alpha = A.alpha; J.channels = A.channels; J.is_f64 = s.fmt;
  }
  const unsigned J = (unsigned)who.size();
  if ((rc = jobs_upload(g, J * sizeof(AgingJob)))) return rc;
  std::string err;
  if ((rc = asub(g, launch_agingradio_jobs(st, g->ctx->n_cu, jobs, (AgingJob *)g->jobs.d, J, &err), err))) return rc;
  if ((rc = copy_runs(g, g->in, g->in.cap, runs, max_host, hipMemcpyDeviceToHost))) return rc;
  if ((rc = astep(g, hipStreamSynchronize(st), "sync"))) return rc;
  for (int m : who) g->aging[(size_t)m].k += g->sub[m].n / 2;   // chunks_exact_mut: an odd last frame is not a pair
  return MI355_OK;
}

// ---- ebur128level: the members that have submitted advance, each by its own buffer size and with its own 100 ms phase (the engine
// walks per-stream rounds, ebur128_kernels.hip); the others - late, detached, paused - do not move. One sample format per launch
// set: the set's (fixed when its first member was accepted, mi355_agroup_submit_ebur128), never "the last member's": it is every
// member's element size, the slot stride and the kernel template. Device members: one D2D copy each. Nothing comes down.
int run_ebur128(mi355_agroup *g) {
  const std::vector<int> who = set_members(g);
  if (who.empty()) return MI355_OK;
  const int fmt = g->set_fmt;
  const size_t frame_bytes = g->channels * kEburSampleBytes[fmt];
  std::vector<size_t> frames_per((size_t)g->n_members, 0);
  size_t max_host = 0;
  for (int m : who) {
    frames_per[(size_t)m] = g->sub[m].n;
    if (!g->sub[m].device && g->sub[m].n * frame_bytes > max_host) max_host = g->sub[m].n * frame_bytes;
  }
  int rc;
  if ((rc = copy_runs(g, g->in, g->in.cap, set_runs(g), max_host, hipMemcpyHostToDevice))) return rc;
  for (int m : who)
    if (g->sub[m].device)
      if ((rc = astep(g, hipMemcpyAsync(g->in.d + (size_t)m * g->in.cap, g->sub[m].data, g->sub[m].n * frame_bytes, hipMemcpyDeviceToDevice, g->ctx->stream), "gather"))) return rc;
  return actx(g, ebur128_add_frames_streams(g->ctx, g->in.d, g->in.cap / kEburSampleBytes[fmt], frames_per.data(), fmt, 1));
}

// ---- audioloudnorm: the members that have submitted advance, class by class - a class = the members that stand at the same frame
// type and hand over the same number of frames (streams that started together; a late starter is a class of its own until it has
// caught up with the 100 ms frames of the others). One launch sequence per class (loudnorm.hip: loudnorm_process_members), the
// other members do not move. A class goes up at the class's frame size, one copy per run of its host members; a device member by
// one D2D copy in and one out. res_frames of a member = what its class's frame produced.
int run_loudnorm(mi355_agroup *g) {
  const size_t ch = g->channels, N = (size_t)g->n_members;
  hipStream_t st = g->ctx->stream;
  std::vector<char> todo(N, 0);
  bool any = false;
  for (size_t m = 0; m < N; m++) if (g->sub[m].have()) { todo[m] = 1; any = true; }
  if (!any) return MI355_OK;
  const size_t in_stride = g->in.cap / 8, row = out_row(g, g->out.cap), cap_frames = row / (ch * 8);
  int rc;
  for (size_t m0 = 0; m0 < N; m0++) {
    if (!todo[m0]) continue;
    // the class of member m0
    const size_t frames = g->sub[m0].n;
    const int final_frame = g->sub[m0].final_frame, ft = loudnorm_member_frame_type(g->ctx, (unsigned)m0);
    const size_t fs = loudnorm_member_frame_size(g->ctx, (unsigned)m0);
    std::vector<unsigned char> cls(N, 0);
    for (size_t m = m0; m < N; m++)
      if (todo[m] && g->sub[m].n == frames && g->sub[m].final_frame == final_frame && loudnorm_member_frame_type(g->ctx, (unsigned)m) == ft &&
          loudnorm_member_frame_size(g->ctx, (unsigned)m) == fs) { cls[m] = 1; todo[m] = 0; }
    const size_t bytes = frames * ch * 8;
    if ((rc = copy_runs(g, g->in, g->in.cap, host_runs(g, [&cls](int m) { return cls[(size_t)m] != 0; }), bytes, hipMemcpyHostToDevice))) return rc;
    if (bytes)
      for (size_t m = 0; m < N; m++)
        if (cls[m] && g->sub[m].device)
          if ((rc = astep(g, hipMemcpyAsync(g->in.d + m * g->in.cap, g->sub[m].data, bytes, hipMemcpyDeviceToDevice, st), "gather"))) return rc;
    size_t out_frames = 0;
    if ((rc = actx(g, loudnorm_process_members(g->ctx, cls.data(), (const double *)g->in.d, in_stride, frames, (double *)g->out.d, cap_frames * ch, cap_frames, &out_frames, 1,
                                               final_frame)))) return rc;
    for (size_t m = 0; m < N; m++) if (cls[m]) g->res_frames[m] = out_frames;
    if (out_frames)
      for (size_t m = 0; m < N; m++)
        if (cls[m] && g->sub[m].device && g->sub[m].out)
          if ((rc = astep(g, hipMemcpyAsync(g->sub[m].out, g->out.d + m * row, out_frames * ch * 8, hipMemcpyDeviceToDevice, st), "scatter"))) return rc;
  }
  // output: packed [member][cap frames] in the device slab -> the pinned slab, one copy per run of the set's host members, as wide as
  // the run's longest output
  for (const auto &r : set_runs(g)) {
    size_t run_out = 0;
    for (int m = r.first; m <= r.second; m++)
      if (g->res_frames[(size_t)m] > run_out) run_out = g->res_frames[(size_t)m];
    if ((rc = copy_runs(g, g->out, row, Runs{r}, run_out * ch * 8, hipMemcpyDeviceToHost))) return rc;
  }
  return astep(g, hipStreamSynchronize(st), "sync");
}

// hrtfrender / sofalizer / mixer: the host members' input rows up, `launch`, their output rows down, the stream drained
template <typename Launch>
int run_through_slabs(mi355_agroup *g, size_t max_in, size_t max_out, Launch launch) {
  const Runs runs = set_runs(g);
  int rc;
  if ((rc = copy_runs(g, g->in, g->in.cap, runs, max_in, hipMemcpyHostToDevice))) return rc;
  if ((rc = launch())) return rc;
  if ((rc = copy_runs(g, g->out, g->out.cap, runs, max_out, hipMemcpyDeviceToHost))) return rc;
  return astep(g, hipStreamSynchronize(g->ctx->stream), "sync");
}

// ---- hrtfrender: the members that have submitted render their block in ONE launch set (hrtf_kernels.hip: prepare, at most one
// convolution launch per transform size present plus one for the FIR rows, mix). Device members pass their pointers straight through.
int run_hrtf(mi355_agroup *g) {
  std::vector<HrtfSubmit> subs;
  size_t max_in = 0, max_out = 0;
  for (int m : set_members(g)) {
    const Sub &s = g->sub[m];
    const float *pg = g->hrtf_pg.data() + (size_t)m * 256;
    const size_t C = (size_t)hrtf_group_channels(g->hrtf, m);
    HrtfSubmit h;
    h.member = m;
    h.d_in = s.device ? (const float *)s.data : (const float *)(g->in.d + (size_t)m * g->in.cap);
    h.d_out = s.device ? (float *)s.out : (float *)(g->out.d + (size_t)m * g->out.cap);
    h.positions = pg; h.gains = pg + 3 * C;
    subs.push_back(h);
    if (!s.device) {
      if (s.n * C * 4 > max_in) max_in = s.n * C * 4;
      if (s.n * 8 > max_out) max_out = s.n * 8;
    }
  }
  if (subs.empty()) return MI355_OK;
  return run_through_slabs(g, max_in, max_out, [&] {
    std::string err;
    return asub(g, hrtf_group_run(g->hrtf, g->ctx->stream, subs.data(), (int)subs.size(), &err), err);
  });
}

// ---- sofalizer: the members that have submitted render their blocks in ONE launch set (sofa_kernels.hip: the pending filters of
// those members transformed - one launch per partition length among them - then one convolution launch per partition length among
// the members, then the mix). Device members pass their pointers straight through.
int run_sofa(mi355_agroup *g) {
  std::vector<SofaSubmit> subs;
  size_t max_in = 0, max_out = 0;
  for (int m : set_members(g)) {
    const Sub &s = g->sub[m];
    SofaSubmit h;
    h.member = m;
    h.d_in = s.device ? (const float *)s.data : (const float *)(g->in.d + (size_t)m * g->in.cap);
    h.d_out = s.device ? (float *)s.out : (float *)(g->out.d + (size_t)m * g->out.cap);
    h.gains = g->sofa_g.data() + (size_t)m * 64;
    h.n_blocks = s.n_blocks;
    subs.push_back(h);
    if (!s.device) {
      const size_t in_bytes = s.n * (size_t)sofa_group_channels(g->sofa, m) * 4;
      if (in_bytes > max_in) max_in = in_bytes;
      if (s.n * 8 > max_out) max_out = s.n * 8;
    }
  }
  if (subs.empty()) return MI355_OK;
  return run_through_slabs(g, max_in, max_out, [&] {
    std::string err;
    return asub(g, sofa_group_run(g->sofa, g->ctx->stream, subs.data(), (int)subs.size(), &err), err);
  });
}

// ---- minus1mixer / audiomultimixer: the members that have submitted mix their interval in ONE kernel launch (mixer.hip: one job
// per member, blocks per (member, frame tile, channel group)). Host members: their segments were packed into their input slots at
// submit and their outputs are packed into their output slots. Device members pass their pointers straight through.
int run_mixer(mi355_agroup *g) {
  const std::vector<int> who = set_members(g);
  if (who.empty()) return MI355_OK;
  size_t max_in = 0, max_out = 0;
  for (int m : who)
    if (!g->sub[m].device) {
      const MixerLayout &L = g->mixer[(size_t)m].layout;
      if (L.in_bytes > max_in) max_in = L.in_bytes;
      if (L.out_bytes_total > max_out) max_out = L.out_bytes_total;
    }
  return run_through_slabs(g, max_in, max_out, [&]() -> int {
    std::vector<std::vector<mi355_mixer_segment>> segs(who.size());
    std::vector<std::vector<mi355_mixer_output>> outs(who.size());
    std::vector<MixerCall> calls(who.size());
    for (size_t j = 0; j < who.size(); j++) {
      const int m = who[j];
      const MixerMember &M = g->mixer[(size_t)m];
      segs[j] = M.segs;
      outs[j] = M.outs;
      if (!g->sub[m].device) {
        for (size_t i = 0; i < segs[j].size(); i++) segs[j][i].data = g->in.d + (size_t)m * g->in.cap + M.layout.seg_off[i];
        for (size_t o = 0; o < outs[j].size(); o++) outs[j][o].data = g->out.d + (size_t)m * g->out.cap + M.layout.out_off[o];
      }
      calls[j] = MixerCall{M.n_inputs, M.n_out, M.bits.data(), segs[j].data(), (unsigned)segs[j].size(), outs[j].data(), (unsigned)outs[j].size(), g->sub[m].n};
    }
    std::string err;
    int launches = 0;
    if (int rc = asub(g, mixer_launch(g->mix_tables, g->ctx->stream, calls.data(), (int)calls.size(), &launches, &err), err)) return rc;
    g->mix_launches += (uint64_t)launches;
    return MI355_OK;
  });
}

// ---- wait's copy-out, per kind. The member is COLLECTING: its row is not written again before it submits again, its buffers and
// (mixer) its output list and layout stay, and copy_unlocked keeps the slab where it is.
int copy_out_in_place(mi355_agroup *g, std::unique_lock<std::mutex> &lk, int member, size_t) {   // echo / agingradio
  const Sub &s = g->sub[member];
  if (s.device || !s.n) return MI355_OK;
  const char *src = in_slot(g, member);
  void *dst = s.data;
  const size_t bytes = s.bytes;
  copy_unlocked(g, lk, bytes, kCopyUnderLock, [=] { std::memcpy(dst, src, bytes); });
  return MI355_OK;
}

int copy_out_stereo(mi355_agroup *g, std::unique_lock<std::mutex> &lk, int member, size_t frames) {   // hrtfrender / sofalizer (a block is tens of KB)
  const Sub &s = g->sub[member];
  if (s.device || !frames || !s.out) return MI355_OK;
  const char *src = g->out.h + (size_t)member * g->out.cap;
  void *dst = s.out;
  copy_unlocked(g, lk, frames * 8, 0, [=] { std::memcpy(dst, src, frames * 8); });
  return MI355_OK;
}

int copy_out_mixer(mi355_agroup *g, std::unique_lock<std::mutex> &lk, int member, size_t frames) {
  const MixerMember &M = g->mixer[(size_t)member];
  if (g->sub[member].device || !frames || M.outs.empty()) return MI355_OK;
  const char *src = g->out.h + (size_t)member * g->out.cap;
  copy_unlocked(g, lk, M.layout.out_bytes_total, 0, [&M, src] {
    for (size_t o = 0; o < M.outs.size(); o++) std::memcpy(M.outs[o].data, src + M.layout.out_off[o], M.layout.out_bytes[o]);
  });
  return MI355_OK;
}

int copy_out_loudnorm(mi355_agroup *g, std::unique_lock<std::mutex> &lk, int member, size_t frames) {
  const Sub &s = g->sub[member];
  if (frames > s.out_cap) return afail(g, MI355_ERR_INVALID_ARG, "audioloudnorm: output buffer too small");
  if (s.device || !frames || !s.out) return MI355_OK;
  const char *src = g->out.h + (size_t)member * out_row(g, g->out.cap);
  void *dst = s.out;
  const size_t bytes = frames * g->channels * 8;
  copy_unlocked(g, lk, bytes, 0, [=] { std::memcpy(dst, src, bytes); });
  return MI355_OK;
}

//                   name          run           out row = slot  result in a slab  copy-out
const Kind kKinds[] = {
    {"",           nullptr,      false,          false,            nullptr},
    {"echo",       run_echo,     false,          true,             copy_out_in_place},
    {"ebur128",    run_ebur128,  false,          false,            nullptr},            // a meter: nothing comes down, nothing to collect
    {"loudnorm",   run_loudnorm, false,          true,             copy_out_loudnorm},
    {"agingradio", run_aging,    false,          true,             copy_out_in_place},
    {"hrtf",       run_hrtf,     true,           true,             copy_out_stereo},
    {"sofa",       run_sofa,     true,           true,             copy_out_stereo},
    {"mixer",      run_mixer,    true,           true,             copy_out_mixer},
};
const Kind &kind_of(const mi355_agroup *g) { return kKinds[g->kind]; }

// runs the collected interval. g->mu held (the members are blocked on it or on the condition variable anyway).
void run_interval(mi355_agroup *g) {
  (void)hipSetDevice(g->device);
  for (int m = 0; m < g->n_members; m++)
    if (g->sub[m].have()) g->res_frames[m] = g->sub[m].n;   // (loudnorm's run puts what the frame produced in its place)
  const int rc = kind_of(g).run(g);
  uint64_t carried = 0;
  for (int m = 0; m < g->n_members; m++) {
    Sub &s = g->sub[m];
    if (!s.have()) continue;
    carried++;
    g->res_status[m] = rc;
    g->res_interval[m] = s.interval;
    g->res_pending[(size_t)m] = !s.device && rc == MI355_OK && kind_of(g).result_in_slab;
    s.state = M_RAN;   // (data / out / n / fmt stay: wait(ticket of s.interval) copies the member's result out, once)
  }
  g->n_batches++;
  g->n_buffers += carried;
  if (carried > g->n_largest) g->n_largest = carried;
  g->interval++;
  g->cv.notify_all();
}

bool everybody_here(const mi355_agroup *g) {
  bool any = false;
  for (int m = 0; m < g->n_members; m++) {
    if (!g->attached[m]) continue;
    if (!g->sub[m].have()) return false;
    any = true;
  }
  return any;
}

mi355_agroup *agroup_new(int device, int kind, int n_members, int *status) {
  if (n_members < 1 || n_members > 4096) { if (status) *status = MI355_ERR_INVALID_ARG; return nullptr; }
  int st = MI355_OK;
  mi355_ctx *ctx = mi355_ctx_create(device, &st);
  if (!ctx) { if (status) *status = st ? st : MI355_ERR_NO_DEVICE; return nullptr; }
  mi355_agroup *g = new mi355_agroup();
  g->device = device; g->kind = kind; g->n_members = n_members; g->ctx = ctx;
  g->attached.assign((size_t)n_members, 1);
  g->sub.assign((size_t)n_members, Sub{});
  g->res_status.assign((size_t)n_members, MI355_OK);
  g->res_frames.assign((size_t)n_members, 0);
  g->res_interval.assign((size_t)n_members, 0);
  g->res_pending.assign((size_t)n_members, 0);
  return g;
}

// the end of every create_*: the status out, and a group that could not be set up is gone
mi355_agroup *created(mi355_agroup *g, int rc, int *status) {
  if (status) *status = rc;
  if (rc) { mi355_agroup_destroy(g); return nullptr; }
  return g;
}

uint64_t ticket_of(const mi355_agroup *g, uint64_t interval, int member) { return interval * (uint64_t)g->n_members + (uint64_t)member + 1; }

// common tail of every submit: the member's host buffer goes into its staging slot (copy_unlocked), then the slot counts; run the
// interval if it is complete. `lk` owns g->mu on entry and on return.
void submitted(mi355_agroup *g, std::unique_lock<std::mutex> &lk, int member, uint64_t *ticket, void *dst, const void *src, size_t bytes) {
  g->sub[member].state = M_FILLING;   // not idle any more, and (ebur128) part of the set whose format it shares, while the lock is away
  if (dst && bytes) copy_unlocked(g, lk, bytes, kCopyUnderLock, [=] { std::memcpy(dst, src, bytes); });
  g->sub[member].interval = g->interval;
  if (ticket) *ticket = ticket_of(g, g->interval, member);
  // (detached during the copy: the buffer is dropped as detach drops a submitted one; wait(ticket) answers "detached")
  g->sub[member].state = g->attached[member] ? M_SUBMITTED : M_IDLE;
  if (everybody_here(g)) run_interval(g);
}

// echo / agingradio / hrtfrender / sofalizer: a host member's buffer needs slots of its size and goes into its own; a device member's stays where it is
int stage_and_submit(mi355_agroup *g, std::unique_lock<std::mutex> &lk, int member, uint64_t *ticket, const void *src, size_t bytes, size_t out_bytes) {
  const bool host = !g->sub[member].device && bytes;
  if (host)
    if (int rc = ensure_staging(g, lk, bytes, out_bytes)) return rc;
  submitted(g, lk, member, ticket, host ? in_slot(g, member) : nullptr, src, bytes);
  return MI355_OK;
}

int check_member(mi355_agroup *g, int kind, int member) {
  if (g->kind != kind) return afail(g, MI355_ERR_INVALID_ARG, "agroup: this group batches another element kind");
  if (member < 0 || member >= g->n_members) return afail(g, MI355_ERR_INVALID_ARG, "agroup: no such member");
  if (!g->attached[member]) return afail(g, MI355_ERR_INVALID_ARG, "agroup: this member has been detached");
  // submitted, run and not collected, or on its way in or out: the slot, data / out and the member's configuration belong to that buffer
  if (g->sub[member].state != M_IDLE) return afail(g, MI355_ERR_INVALID_ARG, "agroup: this member's previous buffer has not been waited for");
  return MI355_OK;
}

// The opening of every call that needs an idle member: null, then the lock, then check_member's kind, member range, attached and
// idle, in this order; the group's device made current. The call goes on with its own argument checks when rc == 0, holding lk.
struct MemberCall {
  std::unique_lock<std::mutex> lk;
  int rc = MI355_ERR_INVALID_ARG;
  MemberCall(mi355_agroup *g, int kind, int member) {
    if (!g) return;
    lk = std::unique_lock<std::mutex>(g->mu);
    if ((rc = check_member(g, kind, member)) == MI355_OK) (void)hipSetDevice(g->device);
  }
};

// a query that takes any member of the kind, busy or detached ones too
int check_index(mi355_agroup *g, int kind, int member) {
  if (g->kind != kind || member < 0 || member >= g->n_members) return afail(g, MI355_ERR_INVALID_ARG, "agroup: bad member");
  return MI355_OK;
}

}  // namespace

extern "C" {

mi355_agroup *mi355_agroup_create_echo(int device, int n_members, size_t ring_len, int *status) {
  mi355_agroup *g = agroup_new(device, KIND_ECHO, n_members, status);
  if (!g) return nullptr;
  g->ring_len = ring_len;
  const size_t cells = (size_t)n_members * (ring_len ? ring_len : 1);
  int rc = ahip(g, hipMalloc((void **)&g->d_rings, cells * 8), "hipMalloc(agroup echo rings)");
  if (!rc) rc = ahip(g, hipMemset(g->d_rings, 0, cells * 8), "hipMemset(agroup echo rings)");
  if (!rc) rc = jobs_create(g, (size_t)n_members * sizeof(EchoJob));
  g->pos.assign((size_t)n_members, 0);
  return created(g, rc, status);
}

mi355_agroup *mi355_agroup_create_ebur128(int device, int n_members, unsigned channels, unsigned rate, unsigned mode, const int *channel_class, int *status) {
  mi355_agroup *g = agroup_new(device, KIND_EBUR128, n_members, status);
  if (!g) return nullptr;
  g->channels = channels;
  return created(g, ebur128_setup_batch(g->ctx, (unsigned)n_members, channels, rate, mode, channel_class), status);
}

mi355_agroup *mi355_agroup_create_loudnorm(int device, int n_members, unsigned channels, double loudness_target, double loudness_range_target,
                                           double max_true_peak, double offset, int *status) {
  mi355_agroup *g = agroup_new(device, KIND_LOUDNORM, n_members, status);
  if (!g) return nullptr;
  g->channels = channels;
  int rc = loudnorm_setup_batch(g->ctx, (unsigned)n_members, channels, loudness_target, loudness_range_target, max_true_peak, offset);
  if (!rc) {
    // the slots for the largest frames State::process sees (the 3 s first frame in, 3 s out at drain) now, not inside the first interval
    std::unique_lock<std::mutex> lk(g->mu);
    if ((size_t)n_members * 576000 * channels * 8 <= ((size_t)2 << 30))   // (thousands of members: sized when the frames come)
      rc = ensure_staging(g, lk, (size_t)576000 * channels * 8, (size_t)30 * 19200 * channels * 8);
  }
  return created(g, rc, status);
}

void mi355_agroup_destroy(mi355_agroup *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  {
    // members still blocked in wait are woken with a failure (destroying a group others still use is a caller bug; nothing hangs)
    std::lock_guard<std::mutex> lk(g->mu);
    for (int m = 0; m < g->n_members; m++) g->attached[m] = 0;
    g->cv.notify_all();
  }
  if (g->ctx) (void)hipStreamSynchronize(g->ctx->stream);
  for (Slab *s : {&g->in, &g->out}) {
    if (s->h) (void)hipHostFree(s->h);
    if (s->d) (void)hipFree(s->d);
  }
  if (g->d_rings) (void)hipFree(g->d_rings);
  if (g->d_w) (void)hipFree(g->d_w);
  if (g->jobs.d) (void)hipFree(g->jobs.d);
  if (g->jobs.h) (void)hipHostFree(g->jobs.h);
  if (g->jobs.ready) (void)hipEventDestroy(g->jobs.ready);
  for (AgingMember &A : g->aging)
    if (A.d_state) (void)hipFree(A.d_state);
  hrtf_group_free(g->hrtf);
  sofa_group_free(g->sofa);
  mixer_tables_free(g->mix_tables);
  if (g->ctx) mi355_ctx_destroy(g->ctx);   // releases the ebur128 / loudnorm batch engines with it
  delete g;
}

const char *mi355_agroup_last_error(mi355_agroup *g) { return g ? g->last_error.c_str() : "null agroup"; }

int mi355_agroup_set_linger(mi355_agroup *g, unsigned linger_us, unsigned timeout_ms) {
  if (!g) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  g->linger_us = linger_us;
  g->timeout_ms = timeout_ms;
  return MI355_OK;
}

int mi355_agroup_detach(mi355_agroup *g, int member) {
  if (!g) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (member < 0 || member >= g->n_members) return afail(g, MI355_ERR_INVALID_ARG, "agroup: no such member");
  g->attached[member] = 0;
  // a buffer that has not run is dropped (one on its way into its slot when its copy is done, submitted()); a result that has run
  // stays collectable, once
  if (g->sub[member].state == M_SUBMITTED) g->sub[member].state = M_IDLE;
  // the others may have been waiting for this one
  if (everybody_here(g)) run_interval(g);
  g->cv.notify_all();
  return MI355_OK;
}

int mi355_agroup_submit_echo(mi355_agroup *g, int member, void *data, size_t n, int is_f64, size_t delay_samples, double intensity, double feedback,
                             int device_data, uint64_t *ticket) {
  MemberCall c(g, KIND_ECHO, member);
  if (c.rc) return c.rc;
  // RingBufferIter::new: assert!(size >= delay); assert_ne!(size, 0) (ring_buffer.rs:41-42)
  if (g->ring_len == 0) return afail(g, MI355_ERR_INVALID_ARG, "rsaudioecho: ring buffer size is 0");
  if (delay_samples > g->ring_len) return afail(g, MI355_ERR_INVALID_ARG, "rsaudioecho: delay exceeds ring buffer size");
  if (n && !data) return afail(g, MI355_ERR_INVALID_ARG, "agroup: null buffer");
  Sub &s = g->sub[member];
  s.device = device_data != 0; s.data = data; s.n = n; s.fmt = is_f64 ? 1 : 0; s.delay = delay_samples; s.intensity = intensity; s.feedback = feedback;
  s.bytes = n * (is_f64 ? 8 : 4);
  return stage_and_submit(g, c.lk, member, ticket, data, s.bytes, 0);
}

int mi355_agroup_submit_ebur128(mi355_agroup *g, int member, const void *data, size_t frames, int sample_format, int device_data, uint64_t *ticket) {
  MemberCall c(g, KIND_EBUR128, member);
  if (c.rc) return c.rc;
  if (sample_format < 0 || sample_format > 3) return afail(g, MI355_ERR_INVALID_ARG, "ebur128: bad sample format");
  if (frames == 0 || !data) return afail(g, MI355_ERR_INVALID_ARG, "agroup: empty buffer");
  const size_t bytes = frames * g->channels * kEburSampleBytes[sample_format];
  if (int rc = ensure_staging(g, c.lk, bytes, 0)) return rc;
  // one sample format per launch set: the first member accepted fixes it, here, under the lock that submitted() may give away for
  // the copy. The set = the members that have submitted AND those whose buffer is still on its way into its slot (FILLING); checked
  // after ensure_staging, which may have given the lock away too.
  bool first = true;
  for (int m = 0; m < g->n_members; m++)
    if (m != member && (g->sub[m].state == M_SUBMITTED || g->sub[m].state == M_FILLING)) first = false;
  if (first) g->set_fmt = sample_format;
  else if (g->set_fmt != sample_format) return afail(g, MI355_ERR_INVALID_ARG, "agroup: the members of an ebur128level group submit one sample format");
  Sub &s = g->sub[member];
  s.device = device_data != 0; s.data = (void *)data; s.n = frames; s.fmt = sample_format;
  submitted(g, c.lk, member, ticket, s.device ? nullptr : in_slot(g, member), data, bytes);
  return MI355_OK;
}

// the `reset` action of one ebur128level instance (imp.rs:124-139, :320-333): this member's meter back to the state of a new one -
// history, histograms, peaks and its 100 ms phase; the other members are not touched. Not while this member has a buffer pending.
int mi355_agroup_ebur128_reset(mi355_agroup *g, int member) {
  MemberCall c(g, KIND_EBUR128, member);
  if (c.rc) return c.rc;
  if (int rc = actx(g, ebur128_reset_stream(g->ctx, (unsigned)member))) return rc;
  for (int k = 0; k < 5; k++) g->query_interval[k] = ~(uint64_t)0;   // cached answers are stale
  g->peak_interval[0] = g->peak_interval[1] = ~(uint64_t)0;
  return MI355_OK;
}

int mi355_agroup_submit_loudnorm(mi355_agroup *g, int member, const double *data, size_t frames, double *out, size_t out_capacity_frames, int final_frame,
                                 int device_data, uint64_t *ticket) {
  MemberCall c(g, KIND_LOUDNORM, member);
  if (c.rc) return c.rc;
  if (frames && !data) return afail(g, MI355_ERR_INVALID_ARG, "agroup: null buffer");
  const size_t ch = g->channels, bytes = frames * ch * 8;
  {
    // the output capacity is checked BEFORE anything changes (as mi355_loudnorm_process_batch does): a first or inner frame answers
    // 100 ms, the final frame what is still inside (imp.rs:270-310), a stream that ends inside its first 3 s its own length
    const size_t cur = loudnorm_member_frame_size(g->ctx, (unsigned)member);
    const size_t need = final_frame ? (cur == 19200 ? (size_t)30 * 19200 - (19200 - (frames < 19200 ? frames : 19200)) : frames) : (size_t)19200;
    if (!final_frame && frames != cur) return afail(g, MI355_ERR_INVALID_ARG, "audioloudnorm: a member hands over whole frames (mi355_agroup_loudnorm_frame_size)");
    if (final_frame && frames >= cur && frames != 0) return afail(g, MI355_ERR_INVALID_ARG, "audioloudnorm: the final frame is shorter than a full one");
    if (need > out_capacity_frames || (need && !out)) return afail(g, MI355_ERR_INVALID_ARG, "audioloudnorm: output buffer too small");
  }
  // what State::process can hand back for this frame: the first frame answers 100 ms, the final one up to 3 s (imp.rs:226-310)
  const size_t worst = final_frame ? (size_t)30 * 19200 : (frames > 19200 ? frames : (size_t)19200);
  if (int rc = ensure_staging(g, c.lk, bytes ? bytes : 8, worst * ch * 8)) return rc;
  Sub &s = g->sub[member];
  s.device = device_data != 0; s.data = (void *)data; s.out = out; s.n = frames; s.out_cap = out_capacity_frames; s.final_frame = final_frame ? 1 : 0;
  submitted(g, c.lk, member, ticket, s.device ? nullptr : in_slot(g, member), data, bytes);
  return MI355_OK;
}

// the frame member `member` hands over next: its first 3 s (576,000 frames at 192 kHz), then 100 ms (19,200)
size_t mi355_agroup_loudnorm_frame_size(mi355_agroup *g, int member) {
  if (!g || g->kind != KIND_LOUDNORM || member < 0 || member >= g->n_members) return 0;
  std::lock_guard<std::mutex> lk(g->mu);
  return loudnorm_member_frame_size(g->ctx, (unsigned)member);
}

// Waits until the member's interval has run; copies a host member's result back to its buffer. *out_frames (optional): frames
// produced (audioloudnorm), samples processed (rsaudioecho) or frames metered (ebur128level).
int mi355_agroup_wait(mi355_agroup *g, uint64_t ticket, size_t *out_frames) {
  if (!g) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (ticket == 0) return afail(g, MI355_ERR_INVALID_ARG, "agroup: unknown ticket");
  const uint64_t interval = (ticket - 1) / (uint64_t)g->n_members;
  const int member = (int)((ticket - 1) % (uint64_t)g->n_members);
  if (interval == 0 || interval > g->interval) return afail(g, MI355_ERR_INVALID_ARG, "agroup: unknown ticket");
  Sub &s = g->sub[member];
  // only the member's outstanding ticket is taken: the buffer that waits for its launch set, or the result that waits to be collected.
  // Anything else is refused HERE, before this call can run a launch set or touch a buffer.
  if (!(s.state == M_RAN && s.interval == interval)) {
    if (!g->attached[member]) return afail(g, MI355_ERR_INVALID_ARG, "agroup: destroyed or detached while waiting");
    if (!(s.state == M_SUBMITTED && s.interval == interval))
      return afail(g, MI355_ERR_INVALID_ARG, interval < g->interval ? "agroup: this ticket has been waited for already" : "agroup: unknown ticket");
  }
  const auto t0 = std::chrono::steady_clock::now();
  while (g->interval <= interval) {
    if (!g->attached[member]) return afail(g, MI355_ERR_INVALID_ARG, "agroup: destroyed or detached while waiting");
    if (everybody_here(g)) { run_interval(g); continue; }
    // independent members: linger for the others, then launch whoever is there
    if (g->linger_us == 0 || g->cv.wait_until(lk, t0 + std::chrono::microseconds(g->linger_us)) == std::cv_status::timeout) {
      if (g->interval <= interval) run_interval(g);
    }
  }
  // (another thread may have collected this very ticket while this one waited for the set)
  if (!(s.state == M_RAN && s.interval == interval) || g->res_interval[member] != interval)
    return afail(g, MI355_ERR_INVALID_ARG, "agroup: this ticket has been waited for already");
  s.state = M_COLLECTING;   // the ticket is spent: a second wait is refused, and the member stays busy until its result is out
  // the member is idle again once its result has been copied out (ebur128level, device members, failed sets: once it has been reported)
  auto collected = [&](int status) { g->res_pending[(size_t)member] = 0; s.state = M_IDLE; return status; };
  const int rc = g->res_status[member];
  if (rc) return collected(rc);   // last_error is the batch's
  const size_t frames = g->res_frames[member];
  if (out_frames) *out_frames = frames;
  // the lock is needed for the copy-out's pointer arithmetic only (copy_unlocked)
  const Kind &K = kind_of(g);
  return collected(K.copy_out ? K.copy_out(g, lk, member, frames) : MI355_OK);
}

// ebur128level's queries for one member (ebur128level/imp.rs:378-452). The engine answers for every member at once; the answers
// of an interval are computed once and served to the members that ask (what: 0 momentary, 1 short-term, 2 global, 3 relative
// threshold, 4 loudness range).
int mi355_agroup_ebur128_loudness(mi355_agroup *g, int member, int what, double *out) {
  if (!g || !out) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (g->kind != KIND_EBUR128) return afail(g, MI355_ERR_INVALID_ARG, "agroup: not an ebur128level group");
  if (member < 0 || member >= g->n_members || what < 0 || what > 4) return afail(g, MI355_ERR_INVALID_ARG, "agroup: bad member / query");
  if (g->query_interval[what] != g->interval) {
    (void)hipSetDevice(g->device);
    g->query_cache[what].assign((size_t)g->n_members, 0.0);
    if (int rc = actx(g, ebur128_query_batch(g->ctx, what, g->query_cache[what].data()))) return rc;
    g->query_interval[what] = g->interval;
  }
  *out = g->query_cache[what][(size_t)member];
  return MI355_OK;
}

int mi355_agroup_ebur128_peak(mi355_agroup *g, int member, int true_peak, unsigned channel, double *out) {
  if (!g || !out) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (g->kind != KIND_EBUR128) return afail(g, MI355_ERR_INVALID_ARG, "agroup: not an ebur128level group");
  if (member < 0 || member >= g->n_members || channel >= g->channels) return afail(g, MI355_ERR_INVALID_ARG, "agroup: bad member / channel");
  const int k = true_peak ? 1 : 0;
  if (g->peak_interval[k] != g->interval) {
    g->peak_cache[k].assign((size_t)g->n_members * g->channels, 0.0);
    if (int rc = actx(g, ebur128_peak_batch(g->ctx, k, g->peak_cache[k].data()))) return rc;
    g->peak_interval[k] = g->interval;
  }
  *out = g->peak_cache[k][(size_t)member * g->channels + channel];
  return MI355_OK;
}

int mi355_agroup_echo_get_state(mi355_agroup *g, int member, double *ring_out, size_t ring_len, size_t *pos_out) {
  if (!g) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (int rc = check_index(g, KIND_ECHO, member)) return rc;
  if (ring_out && ring_len != g->ring_len) return afail(g, MI355_ERR_INVALID_ARG, "agroup: ring length mismatch");
  (void)hipSetDevice(g->device);
  if (ring_out && g->ring_len)
    if (int rc = ahip(g, hipMemcpy(ring_out, g->d_rings + (size_t)member * g->ring_len, g->ring_len * 8, hipMemcpyDeviceToHost), "agroup echo: ring D2H")) return rc;
  if (pos_out) *pos_out = g->pos[(size_t)member];
  return MI355_OK;
}

mi355_agroup *mi355_agroup_create_agingradio(int device, int n_members, int *status) {
  mi355_agroup *g = agroup_new(device, KIND_AGING, n_members, status);
  if (!g) return nullptr;
  g->aging.assign((size_t)n_members, AgingMember{});
  return created(g, jobs_create(g, (size_t)n_members * sizeof(AgingJob)), status);
}

// AudioFilterImpl::setup of one member (agingradio/imp.rs:326-345): its filters restart at 0, its pair counter at 0, a new seed.
// Not while the member has a buffer pending.
int mi355_agroup_agingradio_setup(mi355_agroup *g, int member, unsigned channels, unsigned rate, unsigned lowpass_freq, uint64_t seed) {
  MemberCall c(g, KIND_AGING, member);
  if (c.rc) return c.rc;
  if (channels == 0 || rate == 0) return afail(g, MI355_ERR_INVALID_ARG, "agingradio: 0 channels or rate 0");
  if (lowpass_freq > 0 && channels > 2048) return afail(g, MI355_ERR_UNSUPPORTED, "agingradio: the lowpass runs on at most 2048 channels");
  AgingMember &A = g->aging[(size_t)member];
  if (A.d_state) (void)hipFree(A.d_state);   // (hipFree waits for the launch sets still using it)
  A = AgingMember{};
  if (lowpass_freq > 0) {
    agingradio_setup_filter(rate, lowpass_freq, &A.alpha);
    if (int rc = ahip(g, hipMalloc((void **)&A.d_state, (size_t)channels * 8), "hipMalloc(agroup agingradio filters)")) return rc;
    if (int rc = ahip(g, hipMemset(A.d_state, 0, (size_t)channels * 8), "hipMemset(agroup agingradio filters)")) return rc;
  }
  A.channels = channels;
  A.seed = seed;
  A.configured = true;
  return MI355_OK;
}

int mi355_agroup_submit_agingradio(mi355_agroup *g, int member, void *data, size_t frames, int is_f64, const mi355_agingradio_settings *settings,
                                   int device_data, uint64_t *ticket) {
  MemberCall c(g, KIND_AGING, member);
  if (c.rc) return c.rc;
  if (!g->aging[(size_t)member].configured) return afail(g, MI355_ERR_NOT_CONFIGURED, "agingradio: not negotiated (setup not called)");
  if (!settings) return afail(g, MI355_ERR_INVALID_ARG, "agingradio: null settings");
  if (frames && !data) return afail(g, MI355_ERR_INVALID_ARG, "agroup: null buffer");
  Sub &s = g->sub[member];
  s.device = device_data != 0; s.data = data; s.n = frames; s.fmt = is_f64 ? 1 : 0; s.ar = *settings;
  s.bytes = frames * (size_t)g->aging[(size_t)member].channels * (is_f64 ? 8 : 4);
  return stage_and_submit(g, c.lk, member, ticket, data, s.bytes, 0);
}

int mi355_agroup_agingradio_get_state(mi355_agroup *g, int member, double *filter_state, unsigned channels, uint64_t *pairs_done) {
  if (!g) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (int rc = check_index(g, KIND_AGING, member)) return rc;
  const AgingMember &A = g->aging[(size_t)member];
  if (!A.configured) return afail(g, MI355_ERR_NOT_CONFIGURED, "agingradio: not negotiated (setup not called)");
  (void)hipSetDevice(g->device);
  if (pairs_done) *pairs_done = A.k;
  if (filter_state && channels) {
    const unsigned n = channels < A.channels ? channels : A.channels;
    if (!A.d_state) std::memset(filter_state, 0, (size_t)n * 8);
    else if (int rc = ahip(g, hipMemcpy(filter_state, A.d_state, (size_t)n * 8, hipMemcpyDeviceToHost), "agroup agingradio: filters D2H")) return rc;
  }
  return MI355_OK;
}

// ---- hrtfrender members (HrtfRender, audio/hrtf/src/hrtf/imp.rs)
mi355_agroup *mi355_agroup_create_hrtf(int device, int n_members, int *status) {
  mi355_agroup *g = agroup_new(device, KIND_HRTF, n_members, status);
  if (!g) return nullptr;
  int rc = MI355_OK;
  g->hrtf = hrtf_group_new(n_members, &g->last_error, &rc);
  g->hrtf_pg.assign((size_t)n_members * 256, 0.0f);
  return created(g, rc, status);
}

// Settings::sphere -> HrirSphere::new(bytes, rate) of one member (imp.rs:84-94). Its processors go (set_caps builds them anew).
int mi355_agroup_hrtf_load_sphere(mi355_agroup *g, int member, const void *bytes, size_t len, uint32_t device_rate) {
  MemberCall c(g, KIND_HRTF, member);
  if (c.rc) return c.rc;
  if (!bytes) return afail(g, MI355_ERR_INVALID_ARG, "hrtfrender: null argument");
  std::string err;
  return asub(g, hrtf_group_load_sphere(g->hrtf, member, (const unsigned char *)bytes, len, device_rate, &err), err);
}

// set_caps of one member (imp.rs:648-707): one HrtfProcessor per channel; method = what MI355_FLAG_HRTF_METHOD is for a lone context
int mi355_agroup_hrtf_setup(mi355_agroup *g, int member, int channels, int block_length, int interpolation_steps, int method) {
  MemberCall c(g, KIND_HRTF, member);
  if (c.rc) return c.rc;
  std::string err;
  return asub(g, hrtf_group_setup(g->hrtf, member, channels, block_length, interpolation_steps, method, &err), err);
}

// State::reset_processors of one member (imp.rs:124-129): tails cleared, previous vectors and gains kept; on the group's stream, so
// after the member's last launch set and before its next. Not while the member has a block pending.
int mi355_agroup_hrtf_reset(mi355_agroup *g, int member) {
  MemberCall c(g, KIND_HRTF, member);
  if (c.rc) return c.rc;
  std::string err;
  return asub(g, hrtf_group_reset(g->hrtf, member, g->ctx->stream, &err), err);
}

// One block of one member (HrtfRender::process, imp.rs:164-278): in [S*B][C], out [S*B][2], positions [C][3] and gains [C] (host,
// copied here). wait() answers the frames rendered.
int mi355_agroup_submit_hrtf(mi355_agroup *g, int member, const float *in, float *out, const float *positions_xyz, const float *distance_gains,
                             int device_data, uint64_t *ticket) {
  MemberCall c(g, KIND_HRTF, member);
  if (c.rc) return c.rc;
  if (!in || !out || !positions_xyz || !distance_gains) return afail(g, MI355_ERR_INVALID_ARG, "hrtfrender: null argument");
  if (!hrtf_group_configured(g->hrtf, member)) return afail(g, MI355_ERR_NOT_CONFIGURED, "hrtfrender: not negotiated (setup not called)");
  const size_t C = (size_t)hrtf_group_channels(g->hrtf, member), frames = hrtf_group_frames(g->hrtf, member);
  float *pg = g->hrtf_pg.data() + (size_t)member * 256;
  std::memcpy(pg, positions_xyz, C * 12);
  std::memcpy(pg + 3 * C, distance_gains, C * 4);
  Sub &s = g->sub[member];
  s.device = device_data != 0; s.data = (void *)in; s.out = out; s.n = frames;
  return stage_and_submit(g, c.lk, member, ticket, in, frames * C * 4, frames * 8);
}

int mi355_agroup_hrtf_info(mi355_agroup *g, int member, uint32_t *hrir_len, int *fft_n, int *spheres_held) {
  if (!g) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (int rc = check_index(g, KIND_HRTF, member)) return rc;
  std::string err;
  return asub(g, hrtf_group_info(g->hrtf, member, hrir_len, fft_n, spheres_held, &err), err);
}

// diagnostics: faces [C][S] / weights [C][S][3] of the member's last block (what mi355_hrtf_last_lookup is for a lone context)
int mi355_agroup_hrtf_last_lookup(mi355_agroup *g, int member, int *faces, float *uvw) {
  if (!g) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (int rc = check_index(g, KIND_HRTF, member)) return rc;
  (void)hipSetDevice(g->device);
  std::string err;
  return asub(g, hrtf_group_last_lookup(g->hrtf, member, g->ctx->stream, faces, uvw, &err), err);
}

// kernel launches the group's hrtfrender launch sets have made so far (3 per set of uniform members; measurement plumbing)
uint64_t mi355_agroup_hrtf_launches(mi355_agroup *g) {
  if (!g || g->kind != KIND_HRTF) return 0;
  std::lock_guard<std::mutex> lk(g->mu);
  return hrtf_group_launches(g->hrtf);
}

// ---- sofalizer members (Sofalizer, audio/hrtf/src/sofa/imp.rs)
mi355_agroup *mi355_agroup_create_sofa(int device, int n_members, int *status) {
  mi355_agroup *g = agroup_new(device, KIND_SOFA, n_members, status);
  if (!g) return nullptr;
  int rc = MI355_OK;
  g->sofa = sofa_group_new(n_members, &g->last_error, &rc);
  g->sofa_g.assign((size_t)n_members * 64, 0.0f);
  return created(g, rc, status);
}

// set_caps of one member (sofa/imp.rs:747-838): the Renderer per channel that is not an LFE (:794-798), built for partition-length
// (:779-784). Everything the member needs on the device is allocated here, after the group's stream has drained.
int mi355_agroup_sofa_setup(mi355_agroup *g, int member, int channels, int filter_len, int partition_length, int block_length) {
  MemberCall c(g, KIND_SOFA, member);
  if (c.rc) return c.rc;
  std::string err;
  return asub(g, sofa_group_setup(g->sofa, member, g->ctx->stream, channels, filter_len, partition_length, block_length, &err), err);
}

// Renderer::set_filter of one channel (State::update_filters, sofa/imp.rs:129-160), queued: copied now, transformed with the member's
// next launch set; launches nothing and waits for nothing. Not while the member has a buffer pending.
int mi355_agroup_sofa_set_filter(mi355_agroup *g, int member, int channel, const float *left, const float *right, int delay_left, int delay_right) {
  MemberCall c(g, KIND_SOFA, member);
  if (c.rc) return c.rc;
  std::string err;
  return asub(g, sofa_group_set_filter(g->sofa, member, g->ctx->stream, channel, left, right, delay_left, delay_right, &err), err);
}

// ChannelProcessor::Drop of one channel (LFE1 / LFE2, sofa/imp.rs:812-818): fixed once the member's first block has run
int mi355_agroup_sofa_set_drop(mi355_agroup *g, int member, int channel, int drop) {
  MemberCall c(g, KIND_SOFA, member);
  if (c.rc) return c.rc;
  std::string err;
  return asub(g, sofa_group_set_drop(g->sofa, member, g->ctx->stream, channel, drop, &err), err);
}

// State::reset_processors of one member (sofa/imp.rs:123-127, flush-stop :846-853): history cleared, filters kept; on the group's
// stream, so after the member's last launch set and before its next. Not while the member has a buffer pending.
int mi355_agroup_sofa_reset(mi355_agroup *g, int member) {
  MemberCall c(g, KIND_SOFA, member);
  if (c.rc) return c.rc;
  std::string err;
  return asub(g, sofa_group_reset(g->sofa, member, g->ctx->stream, &err), err);
}

// n_blocks whole blocks of one member (the `while state.adapter.available() >= inblksz` loop of Sofalizer::process, sofa/imp.rs:235-322):
// in [n_blocks * B][C], out [n_blocks * B][2], gains [C] (host, copied here). wait() answers the frames rendered.
int mi355_agroup_submit_sofa(mi355_agroup *g, int member, const float *in, float *out, int n_blocks, const float *distance_gains, int device_data,
                             uint64_t *ticket) {
  MemberCall c(g, KIND_SOFA, member);
  if (c.rc) return c.rc;
  if (!in || !out || !distance_gains) return afail(g, MI355_ERR_INVALID_ARG, "sofalizer: null argument");
  if (n_blocks < 1 || n_blocks > kSofaMaxBlocks) return afail(g, MI355_ERR_INVALID_ARG, "sofalizer: a member hands over 1..8 whole blocks per submit");
  if (!sofa_group_configured(g->sofa, member)) return afail(g, MI355_ERR_NOT_CONFIGURED, "sofalizer: not configured");
  if (!sofa_group_ready(g->sofa, member)) return afail(g, MI355_ERR_NOT_CONFIGURED, "sofalizer: a channel has no filter yet");
  const size_t C = (size_t)sofa_group_channels(g->sofa, member), frames = (size_t)n_blocks * (size_t)sofa_group_block(g->sofa, member);
  std::memcpy(g->sofa_g.data() + (size_t)member * 64, distance_gains, C * 4);
  Sub &s = g->sub[member];
  s.device = device_data != 0; s.data = (void *)in; s.out = out; s.n = frames; s.n_blocks = n_blocks;
  return stage_and_submit(g, c.lk, member, ticket, in, frames * C * 4, frames * 8);
}

int mi355_agroup_sofa_info(mi355_agroup *g, int member, int *partitions_K, int *fft_n, int *pending_filters) {
  if (!g) return MI355_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(g->mu);
  if (int rc = check_index(g, KIND_SOFA, member)) return rc;
  std::string err;
  return asub(g, sofa_group_info(g->sofa, member, partitions_K, fft_n, pending_filters, &err), err);
}

// kernel launches the group's sofalizer launch sets have made so far (2 per set of uniform members with no filter pending, 3 in the
// interval after a source moved; measurement plumbing)
uint64_t mi355_agroup_sofa_launches(mi355_agroup *g) {
  if (!g || g->kind != KIND_SOFA) return 0;
  std::lock_guard<std::mutex> lk(g->mu);
  return sofa_group_launches(g->sofa);
}

// ---- mixer members (minus1mixer / audiomultimixer, audio/audiomultimixer/src)
mi355_agroup *mi355_agroup_create_mixer(int device, int n_members, int *status) {
  mi355_agroup *g = agroup_new(device, KIND_MIXER, n_members, status);
  if (!g) return nullptr;
  int rc = MI355_OK;
  g->mixer.assign((size_t)n_members, MixerMember{});
  g->mix_tables = mixer_tables_new(&g->last_error, &rc);
  return created(g, rc, status);
}

// the member's contribution matrix (contrib nullptr: minus1mixer's i != o); between intervals only
static int agroup_mixer_setup(mi355_agroup *g, int member, unsigned n_inputs, unsigned n_out, const uint8_t *contrib) {
  MemberCall c(g, KIND_MIXER, member);
  if (c.rc) return c.rc;
  const char *why = "";
  if (int rc = mixer_check_setup(n_inputs, n_out, &why)) return afail(g, rc, why);
  MixerMember &M = g->mixer[(size_t)member];
  M.n_inputs = n_inputs;
  M.n_out = n_out;
  mixer_pack_contrib(n_inputs, n_out, contrib, &M.bits);
  M.configured = true;
  return MI355_OK;
}

// OutputConfiguration::get_output_contributions_for_input_channel of one member (audiomultimixerelement.rs:191-214)
int mi355_agroup_mixer_setup(mi355_agroup *g, int member, unsigned n_inputs, unsigned n_out_channels, const uint8_t *contrib) {
  if (!g) return MI355_ERR_INVALID_ARG;
  if (!contrib) { std::lock_guard<std::mutex> lk(g->mu); return afail(g, MI355_ERR_INVALID_ARG, "mixer: null contribution matrix"); }
  return agroup_mixer_setup(g, member, n_inputs, n_out_channels, contrib);
}

// update_output_config's matrix for one member (minus1mixer.rs:500-537)
int mi355_agroup_mixer_setup_minus1(mi355_agroup *g, int member, unsigned n_streams) { return agroup_mixer_setup(g, member, n_streams, n_streams, nullptr); }

// One interval of one member (aggregate_one_buffer per segment, audiomultimixerelement.rs:606-753, then split_output_buf per output,
// splitter.rs:433-467). The arrays are copied here; a host member's segments go into its input slot now (a 10 ms interval of a
// 256-party room is 240 KB), its outputs come back at wait. wait() answers `frames`.
int mi355_agroup_submit_mixer(mi355_agroup *g, int member, const mi355_mixer_segment *segments, unsigned n_segments, const mi355_mixer_output *outputs,
                              unsigned n_outputs, size_t frames, int device_data, uint64_t *ticket) {
  MemberCall c(g, KIND_MIXER, member);
  if (c.rc) return c.rc;
  MixerMember &M = g->mixer[(size_t)member];
  if (!M.configured) return afail(g, MI355_ERR_NOT_CONFIGURED, "mixer: not configured (setup not called)");
  const char *why = "";
  const bool device = device_data != 0;
  if (int rc = mixer_check(M.n_inputs, M.n_out, segments, n_segments, outputs, n_outputs, frames, device, &why)) return afail(g, rc, why);
  MixerLayout L;
  if (!device) {
    mixer_layout(segments, n_segments, outputs, n_outputs, frames, &L);
    if (int rc = ensure_staging(g, c.lk, L.in_bytes, L.out_bytes_total)) return rc;
  }
  M.segs.assign(segments, segments + n_segments);
  M.outs.assign(outputs, outputs + n_outputs);
  M.layout = std::move(L);
  Sub &s = g->sub[member];
  s.device = device; s.data = nullptr; s.out = nullptr; s.n = frames;
  if (!device && M.layout.in_bytes) {
    // the segments go into the member's slot as submitted() copies a single buffer: a large room (256 parties: 240 KB) outside the
    // lock, the member marked busy before the lock goes away; a small one under it
    char *slot = in_slot(g, member);
    s.state = M_FILLING;
    copy_unlocked(g, c.lk, M.layout.in_bytes, kCopyUnderLock, [&M, slot, n_segments] {
      for (unsigned i = 0; i < n_segments; i++)
        if (M.layout.seg_bytes[i]) std::memcpy(slot + M.layout.seg_off[i], M.segs[i].data, M.layout.seg_bytes[i]);
    });
  }
  submitted(g, c.lk, member, ticket, nullptr, nullptr, 0);
  return MI355_OK;
}

// kernel launches the group's mixer launch sets have made so far (one per set in which a member has a frame; measurement plumbing)
uint64_t mi355_agroup_mixer_launches(mi355_agroup *g) {
  if (!g || g->kind != KIND_MIXER) return 0;
  std::lock_guard<std::mutex> lk(g->mu);
  return g->mix_launches;
}

int mi355_agroup_stats(mi355_agroup *g, uint64_t stats[3]) {
  if (!g || !stats) return MI355_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g->mu);
  stats[0] = g->n_buffers;
  stats[1] = g->n_batches;
  stats[2] = g->n_largest;
  return MI355_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- process-wide groups
// Elements of independent pipelines cannot hand a group to each other; what they share is the process. mi355_agroup_shared_*
// returns THE group of this configuration (kind, device, member count, parameters), creating it at first use, and the next free
// member index; a group whose members have all been handed out is not offered again (the next element of that configuration
// starts a new one). mi355_agroup_release = detach; the last member out destroys the group.
namespace {
std::mutex g_shared_mu;
std::vector<mi355_agroup *> g_shared;

template <typename Make>
mi355_agroup *shared_get(const std::string &key, int *member, int *status, Make make) {
  std::lock_guard<std::mutex> lk(g_shared_mu);
  for (mi355_agroup *g : g_shared)
    if (g->shared_key == key && g->handed_out < g->n_members) {
      if (member) *member = g->handed_out;
      g->handed_out++;
      if (status) *status = MI355_OK;
      return g;
    }
  mi355_agroup *g = make();
  if (!g) return nullptr;
  g->shared_key = key;
  g->handed_out = 1;
  if (member) *member = 0;
  g_shared.push_back(g);
  return g;
}

std::string key_of(const char *kind, int device, int n_members, const double *v, int n) {
  std::string k = std::string(kind) + ":" + std::to_string(device) + ":" + std::to_string(n_members);
  for (int i = 0; i < n; i++) { char b[40]; std::snprintf(b, sizeof b, ":%.17g", v[i]); k += b; }
  return k;
}

// mi355_agroup_loudnorm_push / _drain: the member's adapter and the group's channel count (only the member's thread touches its adapter)
int loudnorm_adapter(mi355_agroup *g, int member, std::vector<double> **ad, size_t *ch) {
  std::unique_lock<std::mutex> lk(g->mu);
  if (g->kind != KIND_LOUDNORM || member < 0 || member >= g->n_members) return afail(g, MI355_ERR_INVALID_ARG, "agroup: not an audioloudnorm member");
  if (g->adapter.empty()) g->adapter.resize((size_t)g->n_members);
  *ad = &g->adapter[(size_t)member];
  *ch = g->channels;
  return MI355_OK;
}
}  // namespace

extern "C" {

mi355_agroup *mi355_agroup_shared_echo(int device, int n_members, size_t ring_len, int *member, int *status) {
  const double v[1] = {(double)ring_len};
  return shared_get(key_of("echo", device, n_members, v, 1), member, status, [&] { return mi355_agroup_create_echo(device, n_members, ring_len, status); });
}

mi355_agroup *mi355_agroup_shared_ebur128(int device, int n_members, unsigned channels, unsigned rate, unsigned mode, const int *channel_class, int *member,
                                          int *status) {
  std::vector<double> v = {(double)channels, (double)rate, (double)mode};
  for (unsigned c = 0; c < channels && c < 64; c++) v.push_back(channel_class ? (double)channel_class[c] : -1.0);
  return shared_get(key_of("ebur128", device, n_members, v.data(), (int)v.size()), member, status,
                    [&] { return mi355_agroup_create_ebur128(device, n_members, channels, rate, mode, channel_class, status); });
}

mi355_agroup *mi355_agroup_shared_loudnorm(int device, int n_members, unsigned channels, double loudness_target, double loudness_range_target,
                                           double max_true_peak, double offset, int *member, int *status) {
  const double v[5] = {(double)channels, loudness_target, loudness_range_target, max_true_peak, offset};
  return shared_get(key_of("loudnorm", device, n_members, v, 5), member, status,
                    [&] { return mi355_agroup_create_loudnorm(device, n_members, channels, loudness_target, loudness_range_target, max_true_peak, offset, status); });
}

// audioloudnorm's sink_chain / drain for a member (audioloudnorm/imp.rs:1545-1586 -> drain_full_frames :226-268, drain :270-310) with
// the adapter on this side: what mi355_loudnorm_push / _drain are for a single-instance context. push appends the buffer and
// hands every whole frame over in lock step with the other members (blocking like wait); drain hands over the rest as the final frame.
int mi355_agroup_loudnorm_push(mi355_agroup *g, int member, const double *data, size_t frames, double *out, size_t out_capacity_frames, size_t *out_frames) {
  if (!g || !out_frames) return MI355_ERR_INVALID_ARG;
  *out_frames = 0;
  std::vector<double> *ad = nullptr;
  size_t ch = 0;
  if (int rc = loudnorm_adapter(g, member, &ad, &ch)) return rc;
  if (frames && !data) { std::lock_guard<std::mutex> lk(g->mu); return afail(g, MI355_ERR_INVALID_ARG, "agroup: null buffer"); }
  ad->insert(ad->end(), data, data + frames * ch);
  for (;;) {
    const size_t fs = mi355_agroup_loudnorm_frame_size(g, member);
    if (fs == 0 || ad->size() / ch < fs) break;
    uint64_t t = 0;
    size_t n = 0;
    int rc = mi355_agroup_submit_loudnorm(g, member, ad->data(), fs, out + *out_frames * ch, out_capacity_frames - *out_frames, 0, 0, &t);
    if (!rc) rc = mi355_agroup_wait(g, t, &n);
    if (rc) return rc;
    ad->erase(ad->begin(), ad->begin() + (std::ptrdiff_t)(fs * ch));
    *out_frames += n;
  }
  return MI355_OK;
}

int mi355_agroup_loudnorm_drain(mi355_agroup *g, int member, double *out, size_t out_capacity_frames, size_t *out_frames, int *eos) {
  if (!g || !out_frames) return MI355_ERR_INVALID_ARG;
  *out_frames = 0;
  if (eos) *eos = 0;
  std::vector<double> *ad = nullptr;
  size_t ch = 0;
  if (int rc = loudnorm_adapter(g, member, &ad, &ch)) return rc;
  const size_t rest = ad->size() / ch;
  uint64_t t = 0;
  int rc = mi355_agroup_submit_loudnorm(g, member, ad->data(), rest, out, out_capacity_frames, 1, 0, &t);
  if (!rc) rc = mi355_agroup_wait(g, t, out_frames);
  if (rc) return rc;
  ad->clear();
  if (eos && rest == 0 && *out_frames == 0) *eos = 1;   // nothing at all to drain: FlowError::Eos (imp.rs:289-293)
  return MI355_OK;
}

mi355_agroup *mi355_agroup_shared_agingradio(int device, int n_members, int *member, int *status) {
  return shared_get(key_of("agingradio", device, n_members, nullptr, 0), member, status, [&] { return mi355_agroup_create_agingradio(device, n_members, status); });
}

mi355_agroup *mi355_agroup_shared_hrtf(int device, int n_members, int *member, int *status) {
  return shared_get(key_of("hrtf", device, n_members, nullptr, 0), member, status, [&] { return mi355_agroup_create_hrtf(device, n_members, status); });
}

mi355_agroup *mi355_agroup_shared_sofa(int device, int n_members, int *member, int *status) {
  return shared_get(key_of("sofa", device, n_members, nullptr, 0), member, status, [&] { return mi355_agroup_create_sofa(device, n_members, status); });
}

mi355_agroup *mi355_agroup_shared_mixer(int device, int n_members, int *member, int *status) {
  return shared_get(key_of("mixer", device, n_members, nullptr, 0), member, status, [&] { return mi355_agroup_create_mixer(device, n_members, status); });
}

void mi355_agroup_release(mi355_agroup *g, int member) {
  if (!g) return;
  (void)mi355_agroup_detach(g, member);
  bool last = false;
  {
    std::lock_guard<std::mutex> lk(g_shared_mu);
    g->released++;
    // members never handed out count as gone once everybody who came has left
    last = g->released >= g->handed_out;
    if (last)
      for (size_t i = 0; i < g_shared.size(); i++)
        if (g_shared[i] == g) { g_shared.erase(g_shared.begin() + (std::ptrdiff_t)i); break; }
  }
  if (last) mi355_agroup_destroy(g);
}

}  // extern "C"

// agingradio_cpu.cpp — one CPU core running AgingRadio::process (audio/audiofx/src/agingradio/imp.rs:94-136) as the reference
// does it: the per-pair click draw, per-sample noise, lowpass-filter 0.4.1's y += alpha * (x - y), quantise, cubic curve. The
// yardstick for tools/bench_agingradio.py, not part of the product. The reference draws from rand's ThreadRng; a xoshiro256++
// generator stands in for it here (comparable cost per 64-bit draw), so the output is not the library's.
//
//   g++ -O3 -std=c++17 -ffp-contract=off tools/agingradio_cpu.cpp -o tools/agingradio_cpu
//   tools/agingradio_cpu [channels=2] [frames_per_buffer=480] [seconds_of_audio=10] [lowpass=2000]
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Xoshiro {
  uint64_t s[4] = {0x9E3779B97F4A7C15ull, 0xBF58476D1CE4E5B9ull, 0x94D049BB133111EBull, 0x2545F4914F6CDD1Dull};
  static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
  uint64_t next() {
    const uint64_t r = rotl(s[0] + s[3], 23) + s[0], t = s[1] << 17;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
    return r;
  }
};

struct Settings { float ampl = 0.011f, clicks = 1.0f / 100000.0f, bits = 4.0f, dist = 1.0f; unsigned passes = 3; };

template <typename F>
static void process(F *data, size_t n, unsigned ch, std::vector<double> *filters, double alpha, const Settings &s, Xoshiro &rng) {
  const double p = s.clicks;
  const uint64_t p_int = p >= 1.0 ? ~0ull : (uint64_t)(p * 18446744073709551616.0);
  for (size_t base = 0; base + 2 * ch <= n; base += 2 * ch) {
    const bool click = s.clicks > 0.0f && (p_int == ~0ull || rng.next() < p_int);
    for (unsigned c = 0; c < 2 * ch; c++) {
      double x = (double)data[base + c];
      if (click) {
        x = 1.0;
      } else {
        const double a = s.ampl;
        if (a > 0.0) {
          uint64_t bits = (rng.next() >> 12) | 0x3FF0000000000000ull;
          double v;
          std::memcpy(&v, &bits, 8);
          x += (v - 1.0) * (a + a) + (-a);
        }
        if (filters) {
          double &y = (*filters)[c % ch];
          const double xc = x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);
          y = y + alpha * (xc - y);
          x = y;
        }
        if (s.bits > 0.0f) {
          const double f = std::pow(2.0, (double)s.bits);
          x = std::round(x * f) / f;
        }
        if (s.dist > 0.0f && s.passes > 0)
          for (unsigned k = 0; k < s.passes; k++) x = x - (double)s.dist * (x * (x * x));
      }
      data[base + c] = (F)x;
    }
  }
}

int main(int argc, char **argv) {
  const unsigned ch = argc > 1 ? (unsigned)atoi(argv[1]) : 2;
  const size_t frames = argc > 2 ? (size_t)atol(argv[2]) : 480;
  const double seconds = argc > 3 ? atof(argv[3]) : 10.0;
  const unsigned lowpass = argc > 4 ? (unsigned)atoi(argv[4]) : 2000;
  const unsigned rate = 48000;
  const double rc = 1.0 / ((double)lowpass * 2.0 * 3.141592653589793), dt = 1.0 / rate, alpha = dt / (rc + dt);
  std::vector<float> buf(frames * ch);
  for (size_t i = 0; i < buf.size(); i++) buf[i] = (float)std::sin(0.001 * (double)i);
  std::vector<double> filters(ch, 0.0);
  Xoshiro rng;
  Settings s;
  const size_t buffers = (size_t)(seconds * rate / (double)frames) + 1;
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t b = 0; b < buffers; b++) process(buf.data(), buf.size(), ch, lowpass ? &filters : nullptr, alpha, s, rng);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  double sum = 0;
  for (float v : buf) sum += v;
  std::printf("{\"channels\": %u, \"frames_per_buffer\": %zu, \"lowpass\": %u, \"buffers\": %zu, \"ms_per_buffer\": %.6f, \"ns_per_sample\": %.3f, \"checksum\": %.6g}\n",
              ch, frames, lowpass, buffers, sec * 1e3 / (double)buffers, sec * 1e9 / ((double)buffers * (double)buf.size()), sum);
  return 0;
}

/* tests/cpu_replay/loudnorm_asan_driver.c — runs oracle/loudnorm_oracle.c + oracle/ebur128_oracle.c over one stream under the
 * host's AddressSanitizer / UBSan (tests/test_loudnorm_cpu.py builds it as a standalone executable and runs it as a child).
 *
 *   loudnorm_asan_driver <channels> <frames> [push_frames]
 *
 * The stream is generated here: a 3 kHz tone near the target loudness with short 9.6 kHz bursts far above the ceiling, the
 * last of them inside the final 100 ms and one ending just before the last, short limiter call begins, so that call detects
 * peaks and multiplies frames. For (19200 - frames % 19200) % channels != 0 that call starts at a ring index that is no
 * multiple of `channels` (imp.rs:766-771), and a frame-wise walk can leave limiter_buf; any such access ends the process
 * with the sanitizer's report. Prints frames out and a checksum. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

typedef struct loudnorm loudnorm;
loudnorm *oracle_loudnorm_new(unsigned channels, double loudness_target, double loudness_range_target, double max_true_peak, double offset_db);
void oracle_loudnorm_free(loudnorm *s);
size_t oracle_loudnorm_push(loudnorm *s, const double *src, size_t frames, double *dst);
size_t oracle_loudnorm_drain(loudnorm *s, double *dst);

static const double PI = 3.14159265358979323846;

static void burst(double *x, size_t ch, size_t n, long start, size_t len, double a) {
  if (start < 0 || (size_t)start + len > n) return;
  for (size_t i = 0; i < len; i++)
    for (size_t c = 0; c < ch; c++) x[((size_t)start + i) * ch + c] = a * (1.0 - 0.07 * (double)c) * sin(2.0 * PI * 0.05 * (double)i + 0.9 * (double)c + 0.4);
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s channels frames [push_frames]\n", argv[0]); return 2; }
  const size_t ch = (size_t)atoi(argv[1]), n = (size_t)atol(argv[2]);
  const size_t push = argc > 3 ? (size_t)atol(argv[3]) : n;
  if (ch < 1 || ch > 64 || n < 1 || push < 1) return 2;
  double *x = (double *)malloc(n * ch * sizeof(double));
  double *y = (double *)malloc((n + 64 * 19200) * ch * sizeof(double));
  if (!x || !y) return 3;
  const double amp = 0.1 / sqrt((double)ch);
  for (size_t i = 0; i < n; i++)
    for (size_t c = 0; c < ch; c++) x[i * ch + c] = amp * sin(2.0 * PI * (3000.0 + 170.0 * (double)c) * (double)i / 192000.0);
  const long N = (long)n, L = (long)(n % 19200);
  burst(x, ch, n, 1000, 40, 4.0);
  burst(x, ch, n, 203000, 40, 5.0);
  burst(x, ch, n, N - 50000, 40, 3.5);
  burst(x, ch, n, N - 30000, 30, 5.0);
  burst(x, ch, n, N - 21000, 60, 3.0);
  burst(x, ch, n, N - 9000, 40, 4.0);
  burst(x, ch, n, N - 2500, 30, 5.0);
  burst(x, ch, n, N - 400, 50, 3.6);
  if (L) burst(x, ch, n, N - L - 340, 40, 4.0);
  loudnorm *s = oracle_loudnorm_new((unsigned)ch, -24.0, 7.0, -2.0, 0.0);
  size_t out = 0;
  for (size_t pos = 0; pos < n; pos += push) out += oracle_loudnorm_push(s, x + pos * ch, n - pos < push ? n - pos : push, y + out * ch);
  const size_t d = oracle_loudnorm_drain(s, y + out * ch);
  if (d != (size_t)-1) out += d;
  double sum = 0.0;
  for (size_t i = 0; i < out * ch; i++) sum += fabs(y[i]);
  printf("frames_out %zu checksum %.17g\n", out, sum);
  oracle_loudnorm_free(s);
  free(x);
  free(y);
  return out == n ? 0 : 4;
}

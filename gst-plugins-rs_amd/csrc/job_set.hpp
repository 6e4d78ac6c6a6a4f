// job_set.hpp — the form the video group's frame queues launch in (hsv_kernels.hip: hsvdetector, hsvfilter; colorlut_group.hip:
// colorlut): a table of up to 32 jobs that travels in the kernel arguments, one job per block found from blockIdx alone, and a
// launch set of two such tables - a vector launch and a literal launch - planned by hsvdetect_plan from the jobs' own units.
// A Table is a struct { Job job[N]; int32_t n_jobs, pad; } whose Job has `units`, `first_block` and `blocks`.
#pragma once
#include "internal.hpp"

#include <string>

namespace mi355 {

// the job of block b: jobs are in first_block order and every job of a table has at least one block
template <class Table>
__device__ __forceinline__ int hsvdetect_job_of(const Table &T, uint32_t b) {
  int j = 0;
  while (j + 1 < T.n_jobs && b >= T.job[j].first_block + T.job[j].blocks) j++;
  return j;
}

enum { kVec = 0, kLit = 1 };

// (units per block, blocks per CU) of the two launches
struct JobGrid {
  unsigned per_block[2];
  int per_cu[2];
};
//   kVec  four pixels per lane: 512 units per block (two groups per lane), 64 blocks per CU - the lone grid_for(ctx, (n_vec + 1) / 2, 256, 64)
//   kLit  one pixel per lane, literally: 256 units per block, 32 blocks per CU - the lone grid_for(ctx, total, 256, 32)
constexpr JobGrid kHsvJobGrid = {{512, 256}, {64, 32}};

// A launch set: the two job tables that a builder classifies frames into and fills, and their grids. Planned and launched here.
template <class Table>
struct JobSet {
  typedef void (*Kernel)(const Table);
  Table table[2];
  uint32_t blocks[2];

  // first_block / blocks of every job, by hsvdetect_plan over the jobs' own units; a table with a job has at least one block
  int plan(int n_cu, const JobGrid &grid = kHsvJobGrid) {
    constexpr int kMax = (int)(sizeof(Table::job) / sizeof(Table::job[0]));
    static_assert(kMax <= kHdSetMax, "hsvdetect_plan takes up to kHdSetMax jobs");
    for (int h = 0; h < 2; h++) {
      Table &T = table[h];
      uint64_t units[kMax];
      uint32_t first[kMax], n[kMax];
      for (int j = 0; j < T.n_jobs; j++) units[j] = T.job[j].units;
      const int rc = hsvdetect_plan(n_cu, grid.per_cu[h], grid.per_block[h], T.n_jobs, units, first, n, &blocks[h]);
      if (rc || (T.n_jobs && !blocks[h])) return rc ? rc : MI355_ERR_INVALID_ARG;
      for (int j = 0; j < T.n_jobs; j++) { T.job[j].first_block = first[j]; T.job[j].blocks = n[j]; }
    }
    return MI355_OK;
  }

  // whichever table has a job goes out on `stream`; *kernel_launches counts on. what[h]: the launch's name in the error text
  int launch(hipStream_t stream, const Kernel (&kernel)[2], const char *const (&what)[2], int *kernel_launches, std::string *err) const {
    for (int h = 0; h < 2; h++) {
      if (!table[h].n_jobs) continue;
      hipLaunchKernelGGL(kernel[h], dim3(blocks[h]), dim3(256), 0, stream, table[h]);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) { *err = std::string(what[h]) + hipGetErrorString(e); return MI355_ERR_HIP; }
      (*kernel_launches)++;
    }
    return MI355_OK;
  }
};

}  // namespace mi355

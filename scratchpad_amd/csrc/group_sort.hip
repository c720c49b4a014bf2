// The stable counting sort of rows by group that sp_moe_route (group = expert) and sp_delta_group (group = adapter
// slot) share: stream_gemm.h states the method and the limits.
#include "stream_gemm.h"

namespace sp {

__global__ __launch_bounds__(kSortThreads) void group_sort_kernel(int32_t* offsets, int32_t* sorted,
                                                                  const int32_t* keys, int N, int G) {
  __shared__ int hist[kMaxGroups * kSortThreads];         // [group][thread]
  __shared__ int part[kSortThreads];
  const int tid = threadIdx.x;
  const int chunk = (N + kSortThreads - 1) / kSortThreads;
  const int c0 = min(tid * chunk, N), c1 = min(c0 + chunk, N);
  for (int g = 0; g < G; ++g) hist[g * kSortThreads + tid] = 0;
  for (int p = c0; p < c1; ++p) {
    const int id = keys[p];
    if ((unsigned)id < (unsigned)G) ++hist[id * kSortThreads + tid];
  }
  __syncthreads();
  // exclusive prefix over the flat [group][thread] order: thread tid owns entries tid G .. tid G + G - 1
  int s = 0;
  for (int j = 0; j < G; ++j) s += hist[tid * G + j];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < kSortThreads; ++i) {
      const int x = part[i];
      part[i] = run;
      run += x;
    }
  }
  __syncthreads();
  int run = part[tid];
  for (int j = 0; j < G; ++j) {
    const int x = hist[tid * G + j];
    hist[tid * G + j] = run;
    run += x;
  }
  if (tid == kSortThreads - 1) offsets[G] = run;          // keys in [0, G)
  __syncthreads();
  if (tid < G) offsets[tid] = hist[tid * kSortThreads];
  __syncthreads();
  for (int p = c0; p < c1; ++p) {
    const int id = keys[p];
    if ((unsigned)id < (unsigned)G) sorted[hist[id * kSortThreads + tid]++] = p;   // < offsets[G] <= N
  }
}

void launch_group_sort(int32_t* offsets, int32_t* sorted, const int32_t* keys, int n, int groups, hipStream_t stream) {
  group_sort_kernel<<<1, kSortThreads, 0, stream>>>(offsets, sorted, keys, n, groups);
}

}  // namespace sp

// What the launch call itself costs the host (profiles/r17): an empty kernel that takes its arguments as the headline
// launch does -- two structs by value, 320 + 72 bytes -- enqueued (a) by hipLaunchKernelGGL, which marshals the structs on
// every call, and (b) by hipModuleLaunchKernel on a hipFunction_t obtained once (hipGetFuncBySymbol) with one prebuilt
// argument buffer (HIP_LAUNCH_PARAM_BUFFER_POINTER).  Only the launch calls are timed: batches of 64 with a stream
// synchronisation between the batches, so the queue never pushes back.  Nanoseconds per call, three repetitions each.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>

struct ArgsA {
  void* p[24];
  long long n[12];
  int k[8];
};  // 320 bytes
struct ArgsB {
  float* bufs[7];
  int n;
  long long off;
};  // 72 bytes

__global__ void k_empty(ArgsA a, ArgsB b) {
  if (a.k[0] == 12345 && b.n == 54321 && a.p[0]) *reinterpret_cast<int*>(a.p[0]) = 1;  // (never: keeps the arguments live)
}

template <class F>
static double ns_per_launch(F launch, hipStream_t st, int batches = 400, int per = 64) {
  for (int i = 0; i < per; ++i) launch();
  (void)hipStreamSynchronize(st);
  double ns = 0;
  for (int b = 0; b < batches; ++b) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < per; ++i) launch();
    ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    (void)hipStreamSynchronize(st);
  }
  return ns / batches / per;
}

int main() {
  hipStream_t st;
  if (hipStreamCreate(&st) != hipSuccess) {
    printf("no device\n");
    return 1;
  }
  ArgsA a;
  ArgsB b;
  memset(&a, 0, sizeof a);
  memset(&b, 0, sizeof b);
  hipFunction_t fn = nullptr;
  if (hipGetFuncBySymbol(&fn, reinterpret_cast<const void*>(&k_empty)) != hipSuccess || !fn) {
    printf("hipGetFuncBySymbol failed\n");
    return 1;
  }
  struct alignas(8) Packed {
    ArgsA a;
    ArgsB b;
  } packed;
  packed.a = a;
  packed.b = b;
  size_t packed_bytes = sizeof packed;
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &packed, HIP_LAUNCH_PARAM_BUFFER_SIZE, &packed_bytes, HIP_LAUNCH_PARAM_END};
  int failed = 0;
  for (int rep = 0; rep < 3; ++rep) {
    const double t_ggl = ns_per_launch([&] { hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, st, a, b); }, st);
    const double t_mod = ns_per_launch(
        [&] { failed += hipModuleLaunchKernel(fn, 1, 1, 1, 64, 1, 1, 0, st, nullptr, config) != hipSuccess; }, st);
    printf("hipLaunchKernelGGL (392 bytes by value) %7.1f ns   hipModuleLaunchKernel (prebuilt buffer) %7.1f ns   difference %+7.1f ns\n",
           t_ggl, t_mod, t_ggl - t_mod);
  }
  failed += hipGetLastError() != hipSuccess;
  printf("failed launches: %d\n", failed);
  (void)hipStreamDestroy(st);
  return failed ? 1 : 0;
}

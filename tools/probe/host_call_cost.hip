// What the per-call host checks in front of a resident launch cost (profiles/r11): hipGetDevice, the stream-capture
// query and an uncontended std::mutex, one million calls each, nanoseconds per call.  Host code only; it needs a device
// because the runtime answers both queries from its own per-thread / per-stream state.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <mutex>

template <class F>
static double ns_per_call(F f, int n = 1000000) {
  for (int i = 0; i < 1000; ++i) f();
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < n; ++i) f();
  return std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n;
}

int main() {
  hipStream_t st;
  if (hipStreamCreate(&st) != hipSuccess) {
    printf("no device\n");
    return 1;
  }
  int sink = 0;
  std::mutex mu;
  const double t_clock = ns_per_call([&] { sink += (int)std::chrono::steady_clock::now().time_since_epoch().count(); });
  const double t_dev = ns_per_call([&] {
    int dev = 0;
    sink += hipGetDevice(&dev) == hipSuccess ? dev : 1;
  });
  const double t_cap = ns_per_call([&] {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    sink += hipStreamIsCapturing(st, &cap) == hipSuccess ? (int)cap : 1;
  });
  const double t_cap0 = ns_per_call([&] {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    sink += hipStreamIsCapturing(nullptr, &cap) == hipSuccess ? (int)cap : 1;
  });
  const double t_mu = ns_per_call([&] {
    std::lock_guard<std::mutex> lk(mu);
    ++sink;
  });
  printf("steady_clock::now            %7.1f ns\n", t_clock);
  printf("hipGetDevice                 %7.1f ns\n", t_dev);
  printf("hipStreamIsCapturing(stream) %7.1f ns\n", t_cap);
  printf("hipStreamIsCapturing(null)   %7.1f ns\n", t_cap0);
  printf("std::mutex lock + unlock     %7.1f ns\n", t_mu);
  printf("two hipGetDevice + one capture query + one mutex: %.3f us per solve (sink %d)\n",
         (2 * t_dev + t_cap + t_mu) * 1e-3, sink & 1);
  (void)hipStreamDestroy(st);
  return 0;
}

// Host -> device uploads as a kernel: the call's packed inputs read over PCIe from host-mapped pinned
// staging memory (its device pointer) by 16-byte loads, written to device memory -- no copy engine.
// hipMemcpyAsync's H2D path stalled the first BA calls after the bench warmup by 7-10 ms each
// (profiles/r05_bench_20step_before.json); for the small per-call uploads of the BA, PnP and
// FrameOptimization handles a kernel on the call's own stream is also the shorter path.
// Device -> device copies on one device (rspl_memcpy_d2d) take a kernel too: a runtime copy is a blit launch with
// the runtime's bookkeeping around it and system-scope cache maintenance at its end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.hpp"

namespace rspl {

__global__ __launch_bounds__(256) void upload_kernel(uint4* dst, const uint4* src, size_t n16, uint8_t* dtail,
                                                     const uint8_t* stail, int ntail) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t i = t; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
  if (t < (size_t)ntail) dtail[t] = stail[t];
}

hipError_t upload_mapped(void* dst, const void* src_mapped, size_t bytes, hipStream_t s) {
  const size_t n16 = bytes / 16;
  const int ntail = (int)(bytes - 16 * n16);
  if (!bytes) return hipSuccess;
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n16 + 255) / 256, 1024));
  hipLaunchKernelGGL(upload_kernel, dim3(blocks), dim3(256), 0, s, static_cast<uint4*>(dst),
                     static_cast<const uint4*>(src_mapped), n16, static_cast<uint8_t*>(dst) + 16 * n16,
                     static_cast<const uint8_t*>(src_mapped) + 16 * n16, ntail);
  return hipGetLastError();
}

// Device -> device: V-byte accesses over the body, where V is the widest width at which dst and src are
// misaligned alike (so that one head of < V bytes aligns both); head and tail byte by byte.
template <typename V>
__global__ __launch_bounds__(256) void copy_kernel(uint8_t* dst, const uint8_t* src, size_t head, size_t nv,
                                                   size_t ntail) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  V* dv = reinterpret_cast<V*>(dst + head);
  const V* sv = reinterpret_cast<const V*>(src + head);
  for (size_t i = t; i < nv; i += (size_t)gridDim.x * 256) dv[i] = sv[i];
  if (t < head) dst[t] = src[t];
  if (t < ntail) dst[head + sizeof(V) * nv + t] = src[head + sizeof(V) * nv + t];
}

template <typename V>
static hipError_t copy_launch(uint8_t* dst, const uint8_t* src, size_t bytes, hipStream_t s) {
  constexpr size_t w = sizeof(V);
  const size_t head = std::min<size_t>((w - reinterpret_cast<uintptr_t>(dst) % w) % w, bytes);
  const size_t nv = (bytes - head) / w, ntail = bytes - head - w * nv;  // head, ntail < w <= 256
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((nv + 255) / 256, 1024));
  hipLaunchKernelGGL(copy_kernel<V>, dim3(blocks), dim3(256), 0, s, dst, src, head, nv, ntail);
  return hipGetLastError();
}

hipError_t copy_device(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (!bytes) return hipSuccess;
  uint8_t* d = static_cast<uint8_t*>(dst);
  const uint8_t* c = static_cast<const uint8_t*>(src);
  const uintptr_t skew = reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src);
  if (skew % 16 == 0) return copy_launch<uint4>(d, c, bytes, s);
  if (skew % 8 == 0) return copy_launch<uint2>(d, c, bytes, s);
  if (skew % 4 == 0) return copy_launch<uint32_t>(d, c, bytes, s);
  return copy_launch<uint8_t>(d, c, bytes, s);
}

}  // namespace rspl

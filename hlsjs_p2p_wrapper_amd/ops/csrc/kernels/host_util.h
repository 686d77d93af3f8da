// Helpers of the host binding files (torch + pybind: not for the .hip translation units).
#pragma once
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>
#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include <cstring>
#include <vector>

#include "launch.h"

namespace hlsp2p {
namespace host {

// compute units of a device (cached: the attribute query costs microseconds per call)
inline int num_cus(int device) {
  static int cached[64] = {0};
  if (device >= 0 && device < 64 && cached[device]) return cached[device];
  int n = 0;
  (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device);
  if (n <= 0) n = 256;  // also when the query fails
  if (device >= 0 && device < 64) cached[device] = n;
  return n;
}

inline void hip_ok(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, what, " failed: ", hipGetErrorString(e));
}

// Many small host arrays, each appended at a 16-byte aligned offset, to go to the device in ONE
// H2D: callers keep the offsets, copy the block into pinned memory and upload it their own way.
struct Staging {
  std::vector<uint8_t> bytes;
  static int64_t aligned(int64_t nbytes) { return (nbytes + 15) & ~int64_t(15); }
  int64_t add(const void* p, int64_t nbytes) {
    const int64_t off = static_cast<int64_t>(bytes.size());
    bytes.resize(off + aligned(nbytes), 0);
    if (nbytes) std::memcpy(bytes.data() + off, p, static_cast<size_t>(nbytes));
    return off;
  }
  template <typename T>
  int64_t add(const std::vector<T>& v) { return add(v.data(), static_cast<int64_t>(v.size() * sizeof(T))); }
  int64_t size() const { return static_cast<int64_t>(bytes.size()); }
  void copy_to(const torch::Tensor& pinned) const {
    if (!bytes.empty()) std::memcpy(pinned.data_ptr(), bytes.data(), bytes.size());
  }
};

// uint8 block from the caching pinned-host allocator (it records the stream of a copy out of it)
inline torch::Tensor pinned_bytes(int64_t n) {
  return torch::empty({n}, torch::TensorOptions().dtype(torch::kUInt8).pinned_memory(true));
}

}  // namespace host
}  // namespace hlsp2p

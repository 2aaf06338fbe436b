// The one allocation point of libtvfem's device memory, with an optional red
// zone around every allocation (a test mode: GPU AddressSanitizer is not
// available where this library runs).
//
// TVFEM_ALLOC_GUARD unset (or 0): tv_dev_alloc is hipMalloc and tv_dev_free is
// hipFree -- same sizes, same addresses, nothing recorded.
//
// TVFEM_ALLOC_GUARD=<KiB> (read at every allocation): the allocation becomes
//   [ front guard | data (bytes) | back guard ]
// inside ONE hipMalloc.  The front guard is the guard size rounded up to 4 KiB,
// so the data keeps its alignment and its offset within a page; the back guard
// starts at the very byte where the data ends and is at least the guard size.
// Both are filled before the call returns:
//   kMemDoubles  all-ones bytes: read as a double that is a NaN, so a kernel
//                that reads past a vector of doubles poisons its result (a test
//                sees it as a bitwise difference from an unguarded run);
//   kMemOther    zero bytes (indices, flags, structs): an index read past its
//                array under a mask then is the valid index 0, never a wild one
//                -- the red zone must not turn a harmless over-read into a
//                fault.  The price: OVER-READS OF NON-DOUBLE ARRAYS ARE NOT
//                DETECTED, only over-writes.
// tv_guard_check compares every live guard with its fill (writes outside an
// allocation).  The guards lie inside the library's own allocation: nothing in
// this mode touches memory that is not mapped.  Not seen: accesses further out
// than the guard, LDS, memory allocated by the caller (torch, RCCL).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "tv_ctx.h"

namespace tv {
namespace {

struct GuardRec {
  void* base;
  size_t bytes, front, back;
  int fill;    // byte value of both guards
  int device;
};
std::mutex g_guard_mu;
std::map<const void*, GuardRec> g_guard;  // keyed by the data pointer

size_t guard_bytes_env() {
  const char* e = std::getenv("TVFEM_ALLOC_GUARD");
  if (!e || !*e) return 0;
  const long long kib = std::atoll(e);
  return kib > 0 ? (size_t)kib * 1024 : 0;
}

}  // namespace

hipError_t tv_dev_alloc(void** p, size_t bytes, int kind) {
  const size_t g = guard_bytes_env();
  if (g == 0) return hipMalloc(p, bytes);
  GuardRec r{};
  r.bytes = bytes;
  r.front = (g + 4095) / 4096 * 4096;
  r.back = g;
  r.fill = kind == kMemDoubles ? 0xFF : 0x00;
  if (hipError_t e = hipGetDevice(&r.device)) return e;
  if (hipError_t e = hipMalloc(&r.base, r.front + bytes + r.back)) return e;
  char* data = static_cast<char*>(r.base) + r.front;
  hipError_t e = hipMemset(r.base, r.fill, r.front);
  if (e == hipSuccess) e = hipMemset(data + bytes, r.fill, r.back);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // the fills are in place when the call returns
  if (e != hipSuccess) {
    hipFree(r.base);
    return e;
  }
  {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guard[data] = r;
  }
  *p = data;
  return hipSuccess;
}

hipError_t tv_dev_free(void* p) {
  if (p != nullptr) {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    auto it = g_guard.find(p);
    if (it != g_guard.end()) {
      void* base = it->second.base;
      g_guard.erase(it);
      return hipFree(base);
    }
  }
  return hipFree(p);
}

}  // namespace tv

extern "C" int tv_guard_check(int64_t* n_guarded, int64_t* n_damaged, int64_t* guard_bytes) {
  using namespace tv;
  if (!n_guarded || !n_damaged || !guard_bytes) {
    set_global_error("tv_guard_check: null argument");
    return TV_ERR_ARG;
  }
  *n_guarded = *n_damaged = *guard_bytes = 0;
  std::lock_guard<std::mutex> lk(g_guard_mu);
  if (g_guard.empty()) return TV_OK;  // (no HIP call: the mode is off or nothing is live)
  int dev0 = 0;
  auto hip_fail = [&](hipError_t e) {
    set_global_error(std::string("tv_guard_check: HIP error ") + hipGetErrorString(e));
    return TV_ERR_HIP;
  };
  if (hipError_t e = hipGetDevice(&dev0)) return hip_fail(e);
  std::vector<unsigned char> h;
  int cur = dev0;
  size_t smallest = SIZE_MAX;
  std::string first;
  for (const auto& kv : g_guard) {
    const GuardRec& r = kv.second;
    if (r.device != cur) {
      if (hipError_t e = hipSetDevice(r.device)) return hip_fail(e);
      cur = r.device;
    }
    if (hipError_t e = hipDeviceSynchronize()) return hip_fail(e);
    smallest = std::min(smallest, r.back);
    h.resize(r.front + r.back);
    const char* data = static_cast<const char*>(kv.first);
    if (hipError_t e = hipMemcpy(h.data(), r.base, r.front, hipMemcpyDeviceToHost)) return hip_fail(e);
    if (hipError_t e = hipMemcpy(h.data() + r.front, data + r.bytes, r.back, hipMemcpyDeviceToHost))
      return hip_fail(e);
    // the damaged byte nearest to the data: the back guard from its start, the front guard from its end
    int64_t at = -1;
    bool behind = false;
    for (size_t i = 0; i < r.back && at < 0; ++i)
      if (h[r.front + i] != (unsigned char)r.fill) at = (int64_t)i, behind = true;
    for (size_t i = r.front; i-- > 0 && at < 0;)
      if (h[i] != (unsigned char)r.fill) at = (int64_t)(r.front - i);
    ++*n_guarded;
    if (at < 0) continue;
    ++*n_damaged;
    if (first.empty())
      first = "tv_guard_check: guard damaged around an allocation of " + std::to_string(r.bytes) + " bytes (fill " +
              (r.fill ? "0xFF, doubles" : "0x00") + "): first damaged byte at offset " +
              (behind ? std::to_string(at) + " past the data" : std::to_string(at) + " before the data");
  }
  if (cur != dev0) hipSetDevice(dev0);
  *guard_bytes = (int64_t)smallest;
  if (!first.empty()) set_global_error(first);
  return TV_OK;
}

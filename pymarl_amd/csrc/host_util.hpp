// Host plumbing shared by the learners' host code: the last-error string, the HIP and LDS checks, the owner of a device
// allocation, and the workspace table that carves one allocation into named buffers.
#pragma once
#include <cstdint>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>
#include "../../include/mq_learner.h"

namespace {

std::mutex g_err_mu;
std::string g_err;

int set_err(int code, const std::string& msg) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = msg;
  return code;
}

// A kernel's static LDS plus a launch's dynamic LDS against the CU's LDS (160 KB on gfx950), checked before the
// launch (the static size is looked up once per kernel). A dispatch past it aborts the whole queue
// (HSA_STATUS_ERROR_INVALID_ALLOCATION), which HIP then reports at the next runtime call as "an illegal memory access
// was encountered", far from its cause: the round-5 fault of a stamped BPTT build was exactly that.
int lds_fits(const void* fn, size_t dyn, const char* what) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, size_t>> known;
  static int limit = 0;
  size_t st = 0;
  bool found = false;
  {
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& k : known)
      if (k.first == fn) { st = k.second; found = true; break; }
  }
  if (!found) {
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return set_err(MQ_ERR_HIP, std::string(what) + ": hipFuncGetAttributes");
    st = fa.sharedSizeBytes;
    std::lock_guard<std::mutex> lk(mu);
    known.emplace_back(fn, st);
    if (limit == 0) {
      int dev = 0, v = 0;
      limit = (hipGetDevice(&dev) == hipSuccess &&
               hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess && v > 0)
                  ? v : 160 * 1024;
    }
  }
  if (st + dyn > (size_t)limit)
    return set_err(MQ_ERR_ARG, std::string(what) + " needs " + std::to_string(st) + " B of static + " +
                                   std::to_string(dyn) + " B of dynamic LDS, past the " + std::to_string(limit) +
                                   " B a workgroup can have");
  return MQ_OK;
}
#define MQ_LDS(fn, dyn)                                                        \
  do {                                                                         \
    const int _rc = lds_fits((const void*)(fn), (size_t)(dyn), #fn);          \
    if (_rc) return _rc;                                                       \
  } while (0)

#define MQ_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return set_err(MQ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

// The one owner of a device allocation: freed when its handle is deleted, whichever path led there. Reads as the
// pointer it holds (null until alloc succeeds).
template <class T = float>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }   // move-only: the copy operations are implicitly deleted
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  operator T*() const { return p; }
  // `count` elements, once: a buffer that is already there stays. A failure is "<what>: <HIP's reason>".
  int alloc(int64_t count, const std::string& what) {
    if (p) return MQ_OK;
    const hipError_t e = hipMalloc((void**)&p, (size_t)count * sizeof(T));
    if (e == hipSuccess) return MQ_OK;
    p = nullptr;
    return set_err(MQ_ERR_HIP, what + ": " + hipGetErrorString(e));
  }
};

inline int64_t align_up(int64_t x) { return (x + 63) & ~int64_t(63); }

// One buffer of a workspace: its name, its floats, and the pointer that receives its place (f, or i for an int32 one).
struct WsRow {
  const char* name;
  int64_t count;
  float** f;
  int32_t** i = nullptr;
};
using WsTable = std::vector<WsRow>;

// The buffers in table order, each at a multiple of 64 floats (an empty one still takes 64): returns the floats in
// all and, given a base, assigns every row's pointer. No HIP call: tests/host/ws_probe.cpp lays a table out over a
// made-up base.
inline int64_t ws_assign(const WsTable& t, float* base) {
  int64_t total = 0;
  for (const WsRow& r : t) {
    if (base && r.f) *r.f = base + total;
    if (base && r.i) *r.i = (int32_t*)(base + total);
    total += align_up(r.count > 1 ? r.count : 1);
  }
  return total;
}

// The table's single allocation, and every row's pointer into it.
inline int ws_carve(DevBuf<float>& ws, const WsTable& t, const std::string& what) {
  const int rc = ws.alloc(ws_assign(t, nullptr), what);
  if (rc) return rc;
  ws_assign(t, ws);
  return MQ_OK;
}

}  // namespace

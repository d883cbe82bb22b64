// uc_host.hpp -- host-side helpers that the C-ABI files of libuchirp_link.so (uc_link_api.cpp), libuchirp_scene.so
// (uc_scene_api.cpp), libuchirp_array.so (uc_array_api.cpp) and libuchirp_align.so (uc_align_api.cpp) share, so that their contracts cannot drift apart: the
// thread's last error, the guard that restores the caller's HIP device, the test for device memory and the pinned + device
// staging pair.  Nothing here knows a frame format (that part: uc_link_host.hpp).  Header-only and in an anonymous
// namespace: every library gets its own copy (its own last error) and no symbol crosses a library boundary.
// RESTRICTION: exactly ONE translation unit per library may include this header.  The anonymous namespace gives every
// includer its own g_err: a second includer in the same library would record errors that uc_*_last_error() of the first
// never shows, and nothing would warn about it.
#pragma once
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace {

// one staging pair: pinned on the host and its twin on the device
struct StagingSlot {
  void* pinned = nullptr;
  void* dev = nullptr;
  size_t cap = 0;
  hipEvent_t copied = nullptr;   // this slot's last host-to-device copy has read the pinned buffer
  hipEvent_t done = nullptr;     // this slot's last kernel has read the device buffer
  bool in_flight = false;
};

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int hip_fail(hipError_t e, const char* what) { return fail(-EIO, "%s: %s", what, hipGetErrorString(e)); }

// the calling thread's current device, put back when the entry point returns
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) {
      prev = -1;
      (void)hipGetLastError();
    }
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// the device whose memory p is (device or managed memory), -1 for anything else
int device_of(const void* p) {
  hipPointerAttribute_t attr;
  memset(&attr, 0, sizeof(attr));
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // clear the sticky "invalid value" of a plain host pointer
    return -1;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged ? attr.device : -1;
}

// the slot's staging pair holds at least `bytes`; called before anything of the call is enqueued
int reserve(StagingSlot* l, size_t bytes, const char* who) {
  if (bytes <= l->cap) return 0;
  size_t cap = l->cap ? l->cap : 4096;
  while (cap < bytes) cap *= 2;
  void *p = nullptr, *d = nullptr;
  hipError_t e = hipHostMalloc(&p, cap, hipHostMallocDefault);
  if (e != hipSuccess) return fail(-ENOMEM, "%s: %zu bytes of pinned staging: %s", who, cap, hipGetErrorString(e));
  e = hipMalloc(&d, cap);
  if (e != hipSuccess) {
    (void)hipHostFree(p);
    return fail(-ENOMEM, "%s: %zu bytes of device staging: %s", who, cap, hipGetErrorString(e));
  }
  if (l->in_flight) (void)hipEventSynchronize(l->done);  // the old pair may still be read
  if (l->pinned) (void)hipHostFree(l->pinned);
  if (l->dev) (void)hipFree(l->dev);
  l->pinned = p;
  l->dev = d;
  l->cap = cap;
  l->in_flight = false;
  return 0;
}

}  // namespace

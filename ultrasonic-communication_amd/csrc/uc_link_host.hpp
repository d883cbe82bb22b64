// uc_link_host.hpp -- host-side helpers that the C-ABI files of libuchirp_link.so (uc_link_api.cpp) and
// libuchirp_scene.so (uc_scene_api.cpp) share, so that the two contracts cannot drift apart: the thread's last error,
// the guard that restores the caller's HIP device, the argument checks, the reference format and the pinned + device
// staging pair.  Header-only and in an anonymous namespace: every library gets its own copy (its own last error) and no
// symbol crosses a library boundary.
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

#include "../../include/uchirp_link.h"

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

bool is_device_ptr(const void* p) {
  hipPointerAttribute_t attr;
  memset(&attr, 0, sizeof(attr));
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // clear the sticky "invalid value" of a plain host pointer
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

size_t elem_size(int dtype) {
  switch (dtype) {
    case UC_LINK_DTYPE_I32:
    case UC_LINK_DTYPE_F32: return 4;
    case UC_LINK_DTYPE_I16: return 2;
    default: return 0;
  }
}

bool config_ok(const uc_link_config* c) {
  if (!(c->fs_tx > 0.0) || !(c->t_symbol > 0.0) || !std::isfinite(c->fs_tx) || !std::isfinite(c->t_symbol)) return false;
  if (!std::isfinite(c->f0) || !std::isfinite(c->f1)) return false;
  const double n = c->t_symbol * c->fs_tx;
  return n >= 2.0 && n < 1e9 && c->n_preamble < (1u << 20) && c->n_guard < (1u << 20);
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

// the format of the reference transmission: 44100 Hz, 0.0262 s, 16000 .. 19000 Hz, 7 preamble symbols, 12 guard symbols
void reference_config(uc_link_config* cfg) {
  memset(cfg, 0, sizeof(*cfg));
  cfg->fs_tx = 44100.0;
  cfg->t_symbol = 0.0262;
  cfg->f0 = 16000.0;
  cfg->f1 = 19000.0;
  cfg->n_preamble = 7;
  cfg->n_guard = 12;
}

}  // namespace

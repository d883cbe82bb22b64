// uc_host.hpp -- the host layer that the C-ABI files of the sixteen sibling libraries share (uc_<name>_api.cpp for link,
// scene, array, align, xcorr, wcorr, track, retime, rate, spec, mic, iir, scan, ddc, mf and duc), so that their contracts
// cannot drift apart:
//   errors     the thread's last error (fail, hip_fail) and the guard that restores the caller's HIP device
//   the object HostBase, which every struct uc_<name> derives from; open() and close_base(), what every uc_*_create and
//              uc_*_destroy does; DeviceBuffer, a device buffer per staging slot that grows; the transform's twiddles
//   staging    stage_begin / stage_copy / stage_end: the ONLY place that knows the order of the events around a launch
//   the grid   persistent_grid: the workgroups the chip holds at once
//   checks     of the row-matrix arguments, with the entry point's name formatted into the one text each has
// Nothing here knows a frame format (that part: uc_link_host.hpp) or a kernel.  Header-only and in an anonymous
// namespace: every library gets its own copy (its own last error) and no symbol crosses a library boundary.
// RESTRICTION: exactly ONE translation unit per library may include this header.  The anonymous namespace gives every
// includer its own g_err: a second includer in the same library would record errors that uc_*_last_error() of the first
// never shows, and nothing would warn about it.
//
// An entry point that launches reads, top to bottom:
//   checks of the arguments alone; DeviceGuard + hipSetDevice; checks that need the device (on_device);
//   stage_begin -> fill sl->pinned, Params and the grid -> stage_copy -> the launches -> return stage_end(...).
// Nothing is enqueued before stage_copy, and an error before it leaves the object as it was.
#pragma once
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------------------------- errors

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

// `who` is the entry point's name in every function below: the first word of each message
int hip_fail(hipError_t e, const char* who, const char* what) { return fail(-EIO, "%s: %s: %s", who, what, hipGetErrorString(e)); }

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

// ------------------------------------------------------------------------------------------------------------ the object

// one staging pair: pinned on the host and its twin on the device
struct StagingSlot {
  void* pinned = nullptr;
  void* dev = nullptr;
  size_t cap = 0;
  hipEvent_t copied = nullptr;   // this slot's last host-to-device copy has read the pinned buffer
  hipEvent_t done = nullptr;     // this slot's last kernel has read the device buffer
  bool in_flight = false;
};

// what every struct uc_<name> starts with; a library adds only what is its own (a table, a format, per-slot buffers)
struct HostBase {
  int device = 0;
  int cus = 0;
  unsigned grid_override = 0;      // UC_<NAME>_GRID under UC_TUNING=1
  int resident[4] = {0, 0, 0, 0};  // by dtype (the link's formats go up to 3): workgroups one CU holds at once (asked once per format)
  // staging: the call's argument tables, pinned on the host and their twin on the device.  Two such pairs, used in turn:
  // call k stages while call k - 1's copy still waits in its stream, so that a loop of calls blocks the host only on the
  // copy of two calls back.
  StagingSlot slot[2];
  unsigned next = 0;
};

// uc_*_destroy: wait for what is in flight, free the staging pairs and their events.  The caller holds a DeviceGuard and
// frees what it added AFTER this (nothing of the object is read by the device any more).
void close_base(HostBase* b) {
  (void)hipSetDevice(b->device);
  for (StagingSlot& sl : b->slot) {
    if (sl.in_flight) (void)hipEventSynchronize(sl.done);
    if (sl.pinned) (void)hipHostFree(sl.pinned);
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.copied) (void)hipEventDestroy(sl.copied);
    if (sl.done) (void)hipEventDestroy(sl.done);
  }
}

// uc_*_create: is there a device, is `device` one, is it a gfx950 (in this order); then a new T (derived from HostBase)
// with the base filled and the events made.  `grid_var` names UC_<NAME>_GRID.  The caller holds a DeviceGuard; on success
// `device` is current, so that the caller can go on to allocate what it adds.
template <class T>
int open(const char* who, const char* grid_var, int device, T** out) {
  if (!out) return fail(-EINVAL, "%s: out is NULL", who);
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(-ENODEV, "%s: no HIP device (%s); this library has no CPU path", who, e != hipSuccess ? hipGetErrorString(e) : "0 devices");
  }
  if (device < 0 || device >= ndev) return fail(-ENODEV, "%s: device %d out of range [0,%d)", who, device, ndev);
  if ((e = hipSetDevice(device)) != hipSuccess) return hip_fail(e, who, "hipSetDevice");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hip_fail(e, who, "hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(-ENODEV, "%s: device %d is %s; the kernels are built for gfx950 only", who, device, prop.gcnArchName);
  T* l = new T();
  l->device = device;
  l->cus = prop.multiProcessorCount;
  // experiment switches are read only under UC_TUNING=1, so that a stray variable in a production environment changes nothing
  const char* tuning = getenv("UC_TUNING");
  if (tuning && !strcmp(tuning, "1")) {
    const char* g = getenv(grid_var);
    if (g && atoi(g) > 0) l->grid_override = (unsigned)atoi(g);
  }
  for (StagingSlot& sl : l->slot)
    if ((e = hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)) != hipSuccess) {
      close_base(l);
      delete l;
      return hip_fail(e, who, "hipEventCreate");
    }
  *out = l;
  return 0;
}

// device memory that belongs to one staging slot (the unit sums of a call) and grows like it
struct DeviceBuffer {
  void* dev = nullptr;
  size_t cap = 0;   // bytes
};

// b holds at least `bytes` (`what` names them in the message); sl is the slot whose kernels read b
int reserve_device(DeviceBuffer* b, StagingSlot* sl, size_t bytes, const char* who, const char* what) {
  if (bytes <= b->cap) return 0;
  size_t cap = b->cap ? b->cap : (size_t)1 << 16;
  while (cap < bytes) cap *= 2;
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, cap);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(-ENOMEM, "%s: %zu bytes of %s: %s", who, cap, what, hipGetErrorString(e));
  }
  if (sl->in_flight) (void)hipEventSynchronize(sl->done);  // the old buffer may still be read
  if (b->dev) (void)hipFree(b->dev);
  b->dev = d;
  b->cap = cap;
  return 0;
}

// exp(-2 pi i k / points), k < points, on the current device: cosine and sine in double, rounded once (as libuchirp.so
// builds its own).  On an error *dev is NULL or what the caller's destroy frees.
inline int device_twiddles(float** dev, int points, const char* who) {
  std::vector<float> tw(2 * (size_t)points);
  for (int k = 0; k < points; ++k) {
    const double a = -2.0 * 3.14159265358979323846 * (double)k / (double)points;
    tw[2 * k] = (float)std::cos(a);
    tw[2 * k + 1] = (float)std::sin(a);
  }
  hipError_t e = hipMalloc((void**)dev, tw.size() * sizeof(float));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *dev = nullptr;
    return fail(-ENOMEM, "%s: the twiddle table: %s", who, hipGetErrorString(e));
  }
  if ((e = hipMemcpy(*dev, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return hip_fail(e, who, "hipMemcpy");
  return 0;
}

// --------------------------------------------------------------------------------------------------------------- staging

// the slot's staging pair holds at least `bytes`
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

// Step 1, after the last check and before anything of the call is enqueued: this call's slot holds `bytes` (and its
// device buffer `extra`, if the library has one, `extra_bytes` of `extra_what`), and its pinned buffer may be written: the
// copy of two calls back has run.  An error leaves `next` as it was.
int stage_begin(HostBase* b, size_t bytes, const char* who, StagingSlot** slot, DeviceBuffer* extra = nullptr, size_t extra_bytes = 0,
                const char* extra_what = "") {
  StagingSlot* sl = &b->slot[b->next];
  int rc = reserve(sl, bytes, who);
  if (rc) return rc;
  if (extra && (rc = reserve_device(extra, sl, extra_bytes, who, extra_what)) != 0) return rc;
  if (sl->in_flight) (void)hipEventSynchronize(sl->copied);
  *slot = sl;
  return 0;
}

// Step 2, with sl->pinned filled: behind the slot's last kernel, the copy to sl->dev, and the mark that it has run
int stage_copy(StagingSlot* sl, size_t bytes, hipStream_t hs, const char* who) {
  hipError_t e;
  if (sl->in_flight && (e = hipStreamWaitEvent(hs, sl->done, 0)) != hipSuccess) return hip_fail(e, who, "hipStreamWaitEvent");
  if ((e = hipMemcpyAsync(sl->dev, sl->pinned, bytes, hipMemcpyHostToDevice, hs)) != hipSuccess) return hip_fail(e, who, "hipMemcpyAsync");
  (void)hipEventRecord(sl->copied, hs);
  return 0;
}

// Step 3, behind the launches, whatever they returned (`launched`: the first error among them): the mark that the slot's
// kernels have run, the slot is in flight, the next call takes the other one; only then the launch error is reported
int stage_end(HostBase* b, StagingSlot* sl, hipStream_t hs, hipError_t launched, const char* who) {
  (void)hipEventRecord(sl->done, hs);
  sl->in_flight = true;
  b->next ^= 1u;
  if (launched != hipSuccess) return hip_fail(launched, who, "launch");
  return 0;
}

// -------------------------------------------------------------------------------------------------------------- the grid

// a persistent grid of exactly the workgroups the chip holds at once (the work is dealt statically, so a workgroup that had
// to wait for a slot would run its whole share alone after the others), at most `cap`.  The runtime's occupancy figure is
// asked (`resident_blocks_per_cu` of the library's kernel file, once per format), not assumed; `fallback` stands in if it
// gives none.
inline uint64_t persistent_grid(HostBase* b, int dtype, int (*resident_blocks_per_cu)(int), int fallback, uint64_t cap) {
  if (!b->resident[dtype]) {
    const int r = resident_blocks_per_cu(dtype);
    b->resident[dtype] = r > 0 ? r : fallback;
  }
  uint64_t grid = (uint64_t)b->cus * (uint64_t)b->resident[dtype];
  if (b->grid_override) grid = b->grid_override;
  return grid > cap ? cap : grid;
}

// ---------------------------------------------------------------------------------------------------------------- checks
// Each returns 0 or the code of fail().  A check that only one entry point makes stays there.  (`inline`, like the grid and
// the twiddles: a library that needs only some of them is not warned about the rest.)

constexpr uint64_t COUNT_MAX = 0xFFFFFFFFull;     // records, rows
constexpr uint64_t STRIDE_MAX = 1ull << 40;       // elements between rows, elements in a row

// the sample formats of the row matrices: UC_*_DTYPE_I32 = 0, UC_*_DTYPE_F32 = 1 in every header (asserted by the includer)
inline int check_dtype(const char* who, int dtype) { return dtype == 0 || dtype == 1 ? 0 : fail(-EINVAL, "%s: unknown dtype %d", who, dtype); }

inline int check_count(const char* who, const char* name, size_t n) {
  return n == 0 || n > COUNT_MAX ? fail(-EINVAL, "%s: %s %zu out of range", who, name, n) : 0;
}

inline int check_max_lag(const char* who, uint32_t max_lag, int limit) {
  return max_lag < 1 || max_lag > (uint32_t)limit ? fail(-EINVAL, "%s: max_lag %u not in 1 .. %d", who, max_lag, limit) : 0;
}

// a stride of 0 stands for rows without a gap
inline size_t stride_or(size_t stride, size_t n) { return stride ? stride : n; }

inline int check_stride(const char* who, const char* name, size_t stride, const char* n_name, size_t n) {
  return stride_or(stride, n) < n ? fail(-EINVAL, "%s: %s %zu < %s %zu", who, name, stride, n_name, n) : 0;
}

// the correlations' rows hold 2 max_lag + 1 values
inline int check_corr_stride(const char* who, size_t corr_stride, size_t lags) {
  return stride_or(corr_stride, lags) < lags ? fail(-EINVAL, "%s: corr_stride %zu < 2 max_lag + 1 = %zu", who, corr_stride, lags) : 0;
}

// the two (defaulted) strides of a call
inline int check_strides_max(const char* who, size_t istride, size_t ostride) {
  return istride > STRIDE_MAX || ostride > STRIDE_MAX ? fail(-EINVAL, "%s: stride too large", who) : 0;
}

// rows * stride of the input (4-byte samples: 2^58) and of the output (`out_limit`): a buffer of 2^60 bytes is no buffer.
// By division, so that nothing wraps.  `out_product` names the output's product in the message.
inline int check_extent(const char* who, size_t n_mics, size_t istride, uint64_t out_rows, size_t ostride, uint64_t out_limit, const char* out_product) {
  return n_mics > (1ull << 58) / istride || out_rows > out_limit / ostride
             ? fail(-EINVAL, "%s: n_mics * in_stride or %s too large", who, out_product)
             : 0;
}

// (ref, mic) rows of uchirp_align.h / uchirp_xcorr.h / uchirp_track.h (one layout): both below n_mics
template <class Pair>
int check_pairs(const char* who, const Pair* pairs, size_t n_pairs, size_t n_mics) {
  for (size_t k = 0; k < n_pairs; ++k)
    if (pairs[k].ref >= n_mics || pairs[k].mic >= n_mics)
      return fail(-EINVAL, "%s: pair %zu: rows %u, %u; n_mics %zu", who, k, pairs[k].ref, pairs[k].mic, n_mics);
  return 0;
}

// the kernels' pair records: where the two rows start, in samples
template <class Rec, class Pair>
void stage_pairs(Rec* rec, const Pair* pairs, size_t n_pairs, size_t istride) {
  for (size_t k = 0; k < n_pairs; ++k) {
    rec[k].ref = (uint64_t)pairs[k].ref * istride;
    rec[k].mic = (uint64_t)pairs[k].mic * istride;
  }
}

// the bytes from the first element of a row matrix to its last
inline size_t span_bytes(uint64_t rows, size_t stride, size_t n, size_t elem) { return ((rows - 1) * stride + n) * elem; }

inline int check_disjoint(const char* who, const char* a_name, const void* a, size_t a_bytes, const char* b_name, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes ? fail(-EINVAL, "%s: %s overlaps %s", who, a_name, b_name) : 0;
}

// with `device` current
inline int check_on_device(const char* who, const char* name, const void* p, int device) {
  return device_of(p) != device ? fail(-EINVAL, "%s: %s is not device memory of device %d", who, name, device) : 0;
}

}  // namespace

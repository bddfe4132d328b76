// What surrounds a handle's device blocks, written once: the device check, the handle's stream and two timing events, one call's scratch, the
// event timer and the wall clock.  The rule of resource_pool.hpp is the contract here as well: THE STREAM HAS DRAINED BEFORE ANY BLOCK GOES BACK -
// ~DeviceHandle and ~CallScratch are where that happens, no destroy function and no call repeats it.
#pragma once
#include <algorithm>
#include <chrono>

#include "resource_pool.hpp"

namespace ppsfm {

using Clock = std::chrono::steady_clock;
inline double MsSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// `device` is one of this process's devices (`where` = the entry point, for the message) and becomes the current one
inline int UseDevice(const char* where, int device) {
  int ndev = 0;
  PP_HIP_TRY(hipGetDeviceCount(&ndev));
  PP_REQUIRE(device >= 0 && device < ndev, "%s: device %d of %d", where, device, ndev);
  PP_HIP_TRY(hipSetDevice(device));
  return PP_OK;
}

// The base of a handle, or one call's resources on the stack: a stream, the two events that bracket its device time, its blocks.  pooled = false:
// plain hipStreamCreate / hipEventCreate / hipMalloc (resources the pool never sees).  The destructor closes it from any state construction reached,
// null members included: set the device, drain the stream, release the blocks, then the events, then the stream.  It runs after the derived members'
// destructors, so a derived handle keeps its device memory in `blocks` and nowhere else.
struct DeviceHandle {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DeviceBlocks blocks;
  explicit DeviceHandle(bool pooled = true) : blocks(pooled) {}
  DeviceHandle(const DeviceHandle&) = delete;
  DeviceHandle& operator=(const DeviceHandle&) = delete;
  int Open(int dev) {      // on the current device (UseDevice, or the hipSetDevice of a caller that was given a checked device)
    device = dev;
    if (blocks.pooled()) {
      PP_TRY(PoolStreamAcquire(&stream));
      PP_TRY(PoolEventAcquire(&ev0, true)); PP_TRY(PoolEventAcquire(&ev1, true));
    } else {
      PP_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      PP_HIP_TRY(hipEventCreate(&ev0)); PP_HIP_TRY(hipEventCreate(&ev1));
    }
    return PP_OK;
  }
  ~DeviceHandle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    blocks.Release();
    for (hipEvent_t e : {ev0, ev1}) {
      if (!e) continue;
      if (blocks.pooled()) PoolEventRelease(e, true); else (void)hipEventDestroy(e);
    }
    if (!stream) return;
    if (blocks.pooled()) PoolStreamRelease(stream); else (void)hipStreamDestroy(stream);
  }
};

// pool blocks of one call (at least one element each), returned after the stream has drained on every way out (`b` is destroyed after the body)
struct CallScratch {
  hipStream_t s;
  DeviceBlocks b;
  explicit CallScratch(hipStream_t stream) : s(stream) {}
  ~CallScratch() { (void)hipStreamSynchronize(s); }
  template <typename T> int Alloc(T** p, size_t count) { return b.Alloc(p, std::max<size_t>(count, 1)); }
  template <typename T> int Zeros(T** p, size_t count) {
    PP_TRY(Alloc(p, count));
    PP_HIP_TRY(hipMemsetAsync(*p, 0, std::max<size_t>(count, 1) * sizeof(T), s));
    return PP_OK;
  }
  template <typename T> int Put(T** p, const T* src, size_t count) { return b.Put(p, src, count, s, 1); }
};

// HIP-event time of the spans between Begin() and End() on a stream, summed
struct StreamTimer {
  hipStream_t stream;
  hipEvent_t ev0, ev1;
  float ms = 0.f;
  explicit StreamTimer(const DeviceHandle& h) : stream(h.stream), ev0(h.ev0), ev1(h.ev1) {}
  int Begin() { PP_HIP_TRY(hipEventRecord(ev0, stream)); return PP_OK; }
  int End() { PP_HIP_TRY(hipEventRecord(ev1, stream)); return PP_OK; }
  int Add() {      // after the stream has drained
    float t = 0.f;
    PP_HIP_TRY(hipEventElapsedTime(&t, ev0, ev1));
    ms += t;
    return PP_OK;
  }
};

}  // namespace ppsfm

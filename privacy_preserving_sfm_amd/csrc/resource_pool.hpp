// Recycled HIP resources of the handles and of the calls without one: device blocks, pinned host blocks, streams and events.
//
// The mapper builds a NEW BundleAdjuster for every image it registers (src/sfm/incremental_mapper.cc:813-858, 6 images; the global one at
// controllers/incremental_mapper.cc:497-504 as the model grows): pp_ba_create / pp_ba_destroy sit in its inner loop.  Measured on MI355X for a
// 6-image / 2004-observation problem: create 0.40 ms, destroy 0.75 ms against 2.2 ms for a 25-iteration solve - ~70 hipMalloc / hipFree (a hipFree
// synchronises the device), a pinned allocation, a stream and 13 events per handle.  Blocks are kept by (device, size class) and handed out
// again; a handle synchronises its stream before it returns anything, so a block is never reused under a kernel that still reads it.
// PPSFM_POOL_MAX_MB (default 1024) caps the cached device bytes per process - beyond it a returned block is freed at once; 0 disables the pool.
#pragma once
#include "common.hpp"

namespace ppsfm {

int PoolDeviceAlloc(void** p, size_t bytes);      // on the CURRENT device
void PoolDeviceFree(void* p);                     // (a pointer the pool does not know is hipFree'd)
int PoolPinnedAlloc(void** p, size_t bytes);
void PoolPinnedFree(void* p);
int PoolStreamAcquire(hipStream_t* s);            // non-blocking stream of the current device
void PoolStreamRelease(hipStream_t s);
int PoolEventAcquire(hipEvent_t* e, bool timing);
void PoolEventRelease(hipEvent_t e, bool timing);
void PoolTrim();                                  // frees everything cached (tests; pp_pool_trim)

// The device and pinned blocks of one owner - a handle, or one call's scratch: what Alloc / Put / AllocPinned hand out is recorded and goes back in
// Release() (the destructor), so "allocated" means "owned" and no destroy function lists buffers.  pooled = false: plain hipMalloc / hipHostMalloc
// (memory the pool never sees; freeing it waits for the device).  The owner NEVER synchronises: the rule above holds - whoever owns it drains its stream
// before it lets the owner release anything.
class DeviceBlocks {
 public:
  explicit DeviceBlocks(bool pooled = true) : pooled_(pooled) {}
  DeviceBlocks(const DeviceBlocks&) = delete;
  DeviceBlocks& operator=(const DeviceBlocks&) = delete;
  ~DeviceBlocks() { Release(); }
  // count == 0: *p = nullptr, PP_OK, nothing recorded; nothing is recorded on failure either
  template <class T> int Alloc(T** p, size_t count) { return AllocBytes(reinterpret_cast<void**>(p), count * sizeof(T), false); }
  // max(count, min_count) elements, the first `count` of them uploaded from src (when not null) on `s`
  template <class T> int Put(T** p, const T* src, size_t count, hipStream_t s, size_t min_count = 0) {
    PP_TRY(Alloc(p, count > min_count ? count : min_count));
    return src ? Upload(*p, src, count, s) : PP_OK;
  }
  int AllocPinned(void** p, size_t bytes) { return AllocBytes(p, bytes, true); }
  // one block back early (a buffer that is regrown); *p = nullptr.  A pointer this owner does not hold is a programming error.
  template <class T> void Free(T** p) { FreeBlock(*p); *p = nullptr; }
  void Release();      // everything, in allocation order
  bool pooled() const { return pooled_; }

 private:
  int AllocBytes(void** p, size_t bytes, bool pinned);
  void FreeBlock(void* p);
  struct Block { void* p; bool pinned; };
  std::vector<Block> blocks_;
  bool pooled_;
};

}  // namespace ppsfm

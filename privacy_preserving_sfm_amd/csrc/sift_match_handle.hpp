// pp_sift_handle as the units that fill one see it: sift_match.hip uploads uint8 rows and prepares them (pp_sift_create), sift_extract.hip writes the
// prepared rows from its descriptor kernel (pp_sift_extract_to_matcher).  Both allocate the store through AllocSiftStore, so a handle is the same
// object whichever way it came to be.
#pragma once
#include <vector>

#include "device_handle.hpp"
#include "sift_match_replay.hpp"

struct pp_sift_impl : ppsfm::DeviceHandle {      // blocks: the descriptors, their offsets and the threshold table
  int32_t num_images = 0;
  std::vector<int64_t> desc_start;      // num_images + 1
  int8_t* d_desc = nullptr;             // total x 128, d - 128
  int32_t* d_off = nullptr;             // total
  // the thresholds of the last options used, on the host and on the device
  bool have_thresholds = false;
  float key_ratio = 0.f, key_distance = 0.f;
  ppsfm::SiftThresholds thresholds;
  int32_t* d_table = nullptr;
  int32_t Rows(int32_t image) const { return (int32_t)(desc_start[(size_t)image + 1] - desc_start[(size_t)image]); }
};

namespace ppsfm {

constexpr int kSiftRowTile = 128;       // query rows per workgroup of k_sift_top2: 4 wavefronts x the MFMA's 32

// what a handle can index: k_sift_top2 addresses rows in int32, a tile past the last one included
inline bool SiftRowsFit(int64_t rows) { return rows >= 0 && rows < 0x7FFFFFFFll - kSiftRowTile; }

// A store of `rows` descriptor rows and their offsets, never less than 16 bytes and one offset (a handle without a row still has both blocks)
inline int AllocSiftStore(DeviceBlocks& b, int64_t rows, int8_t** desc, int32_t** off) {
  PP_TRY(b.Alloc(desc, std::max<size_t>((size_t)rows * kSiftDim, 16)));
  return b.Alloc(off, std::max<size_t>((size_t)rows, 1));
}

}  // namespace ppsfm

// Stand-alone driver of the wavefront descriptor (K23: DescriptorSample, DescriptorFold and the norms by parts in csrc/sift_core.hpp; DescriptorByWave,
// ExtractOnHost's wave route and PlanSiftBatches in csrc/sift_extract_replay.hpp) for tests/test_sift_describe_wave_host.py: no device, built with
// g++ -fsanitize=address,undefined -ffp-contract=off.  One command per line on stdin, the options as tests/sift_extract_host_driver.cpp reads them:
//   wave image_file width height <options>   both descriptor routes of ExtractOnHost on the image, compared by their bits
//        -> same|differs features F raw R bytes B windows W min_pixels A max_pixels Z not_multiple_of_64 N below_64 M cut C two_orientations T
//           (R, B, W: how many raw values, bytes and windows differ)
//   fold binx biny bint rbinx rbiny rbint win mod   one constructed pixel through DescriptorFold on the 64 bin owners against the inner loop of
//                                                   Descriptor(), restated here   -> same|differs touched T  (T: bins that received an addition)
//   frame width height x y sigma is     a keypoint on a synthetic gradient level: DescriptorByWave against Descriptor() + FinishDescriptor()
//        -> same|differs computed C pixels P nonzero Z
//   plan target b0 b1 ...               -> the first image of every sub-batch, then the number of images
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../privacy_preserving_sfm_amd/csrc/sift_extract_replay.hpp"

using namespace ppsfm::sift;

static double ReadDouble(std::istream& in) {
  std::string s;
  in >> s;
  return std::strtod(s.c_str(), nullptr);
}

static Options ReadOptions(std::istream& in) {
  Options o;
  in >> o.max_num_features >> o.first_octave >> o.num_octaves >> o.octave_resolution;
  o.peak_threshold = ReadDouble(in);
  o.edge_threshold = ReadDouble(in);
  in >> o.max_num_orientations >> o.upright >> o.normalization;
  return o;
}

template <class T>
static size_t Differing(const std::vector<T>& a, const std::vector<T>& b) {
  if (a.size() != b.size()) return a.size() + b.size() + 1;
  size_t n = 0;
  for (size_t i = 0; i < a.size(); ++i) n += std::memcmp(&a[i], &b[i], sizeof(T)) != 0;
  return n;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "wave") {
      std::string image_file;
      int w = 0, h = 0;
      in >> image_file >> w >> h;
      const Options o = ReadOptions(in);
      const std::string why = CheckOptions(o, w, h);
      if (!why.empty()) { std::printf("refused %s\n", why.c_str()); continue; }
      std::vector<uint8_t> grey((size_t)w * h);
      std::ifstream f(image_file, std::ios::binary);
      f.read(reinterpret_cast<char*>(grey.data()), (std::streamsize)grey.size());
      if (!f) { std::printf("refused cannot read %s\n", image_file.c_str()); continue; }
      const HostResult A = ExtractOnHost(o, w, h, grey.data(), true, StageSink());
      const HostResult B = ExtractOnHost(o, w, h, grey.data(), true, StageSink(), DescriptorRoute::kWave);
      const size_t raw = Differing(A.raw, B.raw), bytes = Differing(A.descriptors, B.descriptors), windows = Differing(A.windows, B.windows);
      const bool rest = A.keypoints == B.keypoints && A.angles == B.angles && A.octave_level == B.octave_level && A.windows.size() == A.angles.size();
      int32_t lo = 0, hi = 0;
      long odd = 0, small = 0, cut = 0;
      for (size_t i = 0; i < B.window_pixels.size(); ++i) {
        const int32_t p = B.window_pixels[i];
        lo = i == 0 || p < lo ? p : lo; hi = i == 0 || p > hi ? p : hi;
        odd += p % 64 != 0; small += p < 64; cut += B.windows[i].cut;
      }
      std::printf("%s features %zu raw %zu bytes %zu windows %zu min_pixels %d max_pixels %d not_multiple_of_64 %ld below_64 %ld cut %ld two_orientations %lld\n",
                  raw + bytes + windows == 0 && rest ? "same" : "differs", B.angles.size(), raw, bytes, windows, lo, hi, odd, small, cut,
                  (long long)B.two_orientations);
    } else if (cmd == "fold") {
      int binx = 0, biny = 0, bint = 0;
      in >> binx >> biny >> bint;
      const float rbinx = (float)ReadDouble(in), rbiny = (float)ReadDouble(in), rbint = (float)ReadDouble(in), win = (float)ReadDouble(in), mod = (float)ReadDouble(in);
      // the inner loop of Descriptor(), from a zero histogram
      float want[kDescBins], got[kDescBins];
      for (int i = 0; i < kDescBins; ++i) want[i] = got[i] = 0.f;
      bool touched[kDescBins] = {};
      float* dpt = want + 2 * 32 + 2 * 8;
      for (int dbinx = 0; dbinx < 2; ++dbinx)
        for (int dbiny = 0; dbiny < 2; ++dbiny)
          for (int dbint = 0; dbint < 2; ++dbint) {
            if (binx + dbinx >= -2 && binx + dbinx < 2 && biny + dbiny >= -2 && biny + dbiny < 2) {
              const float weight = win * mod * AbsF((float)(1 - dbinx) - rbinx) * AbsF((float)(1 - dbiny) - rbiny) * AbsF((float)(1 - dbint) - rbint);
              const int at = ((bint + dbint) % 8) + (biny + dbiny) * 32 + (binx + dbinx) * 8;
              dpt[at] += weight;
              touched[2 * 32 + 2 * 8 + at] = true;
            }
          }
      DescriptorTap t;
      t.wm = win * mod; t.rbinx = rbinx; t.rbiny = rbiny; t.rbint = rbint; t.binx = binx; t.biny = biny; t.bint = bint; t.pad_ = 0;
      for (int lane = 0; lane < kWaveLanes; ++lane) DescriptorFold(t, ((lane >> 2) & 3) - 2, (lane >> 4) - 2, 2 * (lane & 3), &got[2 * lane], &got[2 * lane + 1]);
      int n = 0;
      for (int i = 0; i < kDescBins; ++i) n += touched[i];
      std::printf("%s touched %d\n", std::memcmp(want, got, sizeof(want)) == 0 ? "same" : "differs", n);
    } else if (cmd == "frame") {
      int w = 0, h = 0, is = 0;
      in >> w >> h;
      Keypoint k{};
      k.x = (float)ReadDouble(in); k.y = (float)ReadDouble(in); k.sigma = (float)ReadDouble(in);
      in >> is;
      k.is = is; k.s = (float)is; k.ix = (int)k.x; k.iy = (int)k.y; k.o = 0;
      std::vector<float> grad(2 * (size_t)w * h);      // level 0 of an octave with s_min = -1, s_max = 4
      for (size_t i = 0; i < grad.size() / 2; ++i) { grad[2 * i] = 0.25f + 0.001f * (float)(i % 97); grad[2 * i + 1] = 0.061f * (float)(i % 103); }
      const std::vector<double> expn = ExpnTable();
      const double angle = 0.7;
      float a[kDescBins], b[kDescBins];
      uint8_t ua[kDescBins], ub[kDescBins];
      const DescriptorWindow wa = Descriptor(grad.data(), w, h, -1, 4, k, 1.0, angle, std::sin(angle), std::cos(angle), expn.data(), a);
      FinishDescriptor(a, 0, ua);
      const DescriptorWindow wb = DescriptorByWave(grad.data(), w, h, -1, 4, k, 1.0, angle, std::sin(angle), std::cos(angle), expn.data(), 0, b, ub);
      const bool same = std::memcmp(a, b, sizeof(a)) == 0 && std::memcmp(ua, ub, sizeof(ua)) == 0 && wa.computed == wb.computed && wa.cut == wb.cut;
      int nonzero = 0;
      for (int i = 0; i < kDescBins; ++i) nonzero += b[i] != 0.f || ub[i] != 0;
      std::printf("%s computed %d pixels %d nonzero %d\n", same ? "same" : "differs", wb.computed, DescriptorWindowPixels(MakeDescriptorFrame(w, h, -1, 4, k, 1.0)), nonzero);
    } else if (cmd == "plan") {
      long long target = 0, v = 0;
      in >> target;
      std::vector<int64_t> bytes;
      while (in >> v) bytes.push_back(v);
      const std::vector<int32_t> plan = PlanSiftBatches(bytes, target);
      for (size_t i = 0; i < plan.size(); ++i) std::printf(i ? " %d" : "%d", plan[i]);
      std::printf("\n");
    } else if (!cmd.empty()) {
      std::printf("refused unknown command %s\n", cmd.c_str());
    }
    std::fflush(stdout);
  }
  return 0;
}

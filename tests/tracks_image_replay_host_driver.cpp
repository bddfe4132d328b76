// Stand-alone driver of csrc/tracks_image_replay.hpp (std only, no HIP) for tests/test_tracks_image_replay_host.py: built with plain
// g++ -fsanitize=address,undefined.  It reads a state and, per line of the image, a canned speculative answer and the answer on the state the
// sequential loop meets (what a fresh launch would return), runs ReplayTriangulateImage and prints the events and the counters.
//   input (whitespace separated):  L  line_image[L]  corr_start[L+1]  corr_line[E]  C  image_registered[C]
//                                  P  then per point: x y z n line[n]
//                                  N  then per line of the image: line, the speculative answer, the fresh answer
//   an answer: nlist list[nlist]  num_triangulated  continue_point  nset set[nset] round_of[nset]  nrounds xyz[3 nrounds]
#include <cstdio>
#include <iostream>

#include "tracks_image_replay.hpp"

using namespace ppsfm;

static ImageLineResult ReadAnswer(std::istream& in) {
  ImageLineResult r;
  size_t n = 0;
  in >> n;
  r.list.resize(n);
  for (auto& v : r.list) in >> v;
  in >> r.num_triangulated >> r.continue_point >> n;
  r.set.resize(n); r.round_of.resize(n);
  for (auto& v : r.set) in >> v;
  for (auto& v : r.round_of) in >> v;
  in >> n;
  r.xyz.resize(3 * n);
  for (auto& v : r.xyz) in >> v;
  return r;
}

int main() {
  std::istream& in = std::cin;
  TrackState st;
  in >> st.L;
  st.line_image.resize((size_t)st.L);
  for (auto& v : st.line_image) in >> v;
  st.corr_start.resize((size_t)st.L + 1);
  for (auto& v : st.corr_start) in >> v;
  st.corr_line.resize((size_t)st.corr_start.back());
  for (auto& v : st.corr_line) in >> v;
  size_t C = 0, P = 0, N = 0;
  in >> C;
  st.image_registered.resize(C);
  for (auto& v : st.image_registered) { int b; in >> b; v = (uint8_t)b; }
  in >> P;
  st.line_point.assign((size_t)st.L, -1);
  st.tracks.resize(P); st.deleted.assign(P, 0); st.points.resize(3 * P);
  for (size_t p = 0; p < P; ++p) {
    size_t n = 0;
    in >> st.points[3 * p] >> st.points[3 * p + 1] >> st.points[3 * p + 2] >> n;
    st.tracks[p].resize(n);
    for (auto& l : st.tracks[p]) { in >> l; st.line_point[(size_t)l] = (int32_t)p; }
  }
  in >> N;
  std::vector<int32_t> lines(N);
  std::vector<ImageLineResult> spec(N), fresh(N);
  for (size_t i = 0; i < N; ++i) { in >> lines[i]; spec[i] = ReadAnswer(in); fresh[i] = ReadAnswer(in); }
  if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }
  std::vector<std::pair<int, int>> events;
  const ImageCounters cnt = ReplayTriangulateImage(
      st, lines, [&](size_t i) -> const ImageLineResult& { return spec[i]; },
      [&](int32_t line) -> const ImageLineResult* {
        for (size_t i = 0; i < N; ++i) if (lines[i] == line) return &fresh[i];
        return nullptr;
      },
      [&](int p, int32_t l) { events.emplace_back(p, l); });
  std::printf("%d %lld %d %d %d %zu\n", cnt.error, (long long)cnt.num_tris, cnt.points_created, cnt.lines_continued, cnt.lines_redone, events.size());
  for (const auto& e : events) std::printf("%d %d\n", e.first, e.second);
  std::printf("%d\n", st.NumPoints());
  for (int p = 0; p < st.NumPoints(); ++p) {
    std::printf("%zu", st.tracks[(size_t)p].size());
    for (const int32_t l : st.tracks[(size_t)p]) std::printf(" %d", l);
    std::printf("\n");
  }
  return 0;
}

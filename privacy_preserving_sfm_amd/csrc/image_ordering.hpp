// The image order pp_ba_create gives the reduced camera system - host code, std only: tests/image_ordering_host_driver.cpp runs its stages under ASan/UBSan.
//
// Ceres' SPARSE_SCHUR reorders the cameras before it factorises the reduced system (the solver the reference selects for 50 < images <= 1000,
// src/optim/bundle_adjustment.cc:279-282).  Here the reduced system is one dense array whose empty 64x64 tiles are skipped and whose independent
// sub-trees of the elimination tree are factorised side by side by several chain workgroups (chol_plan.hpp "ChainRanges"), so what an ordering has to
// deliver is (a) few non-zero tiles and (b) a short longest dependency path over the block columns:
//   * reverse Cuthill-McKee on the co-visibility graph: a band (a sequence whose image ids are not in capture order gets its block-banded system back);
//   * nested dissection of that band (BandDissector): [part | part | the images that couple them], cuts at tile boundaries;
//   * nested dissection of the GRAPH itself (GraphDissector): a vertex separator from a level structure, for co-visibility that no order makes a
//     narrow band - photo collections: clusters joined by a few images, a hub with satellites -, the components a separator leaves as parts of their own.
// The candidates are compared by the number of chain steps of their one-launch factorisation (PlanStepsOf: the chain plan alone, no task list), and
// the winner's task list is verified once (the `verify` callable: plan + list + replay) before it is taken.
//
// Cost (the mapper builds a new BundleAdjuster per global BA, src/sfm/incremental_mapper.cc:893-936, so this runs per call): the co-visibility is a
// bit matrix filled point by point, and the fill STOPS as soon as the graph is too dense for any order to remove a tenth of the tiles (a clique - the
// headline scene - leaves after ~0.3 ms).
//
// ChooseImageOrdering's stages, in its order: SetupOf | CoVisibilityGraph | (TileMapOf, PlanStepsOf: what an order costs) BandCandidate |
// DissectionCandidates | VerifiedWinner.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <numeric>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/ppsfm_hip.h"
#include "ba_structure.hpp"
#include "chol_plan.hpp"
#include "switches.hpp"

namespace ppsfm {

using Adjacency = std::vector<std::vector<int32_t>>;      // neighbours of every image, ascending, no self loops

// Reverse Cuthill-McKee order of the images on their co-visibility graph.  Per connected component: a pseudo-peripheral start (repeated breadth-first
// searches from a minimum-degree node of the last level), breadth-first numbering with the neighbours by increasing degree, the whole order reversed.
// Images without neighbours (constant poses, unobserved images) keep their relative order at the end.  Returns old_of_new.
// (G: the graph as begin(u) / end(u) / degree(u) - the whole graph's neighbour lists, or a part's sub-graph in two flat arrays)
struct ListsGraph {
  const Adjacency& adj;
  int size() const { return (int)adj.size(); }
  const int32_t* begin(int u) const { return adj[u].data(); }
  const int32_t* end(int u) const { return adj[u].data() + adj[u].size(); }
  size_t degree(int u) const { return adj[u].size(); }
};
struct FlatGraph {
  std::vector<int32_t> off, nb;
  int size() const { return (int)off.size() - 1; }
  const int32_t* begin(int u) const { return nb.data() + off[u]; }
  const int32_t* end(int u) const { return nb.data() + off[u + 1]; }
  size_t degree(int u) const { return (size_t)(off[u + 1] - off[u]); }
};
template <class G>
std::vector<int32_t> ReverseCuthillMcKeeOf(const G& g) {
  const int C = g.size();
  std::vector<int32_t> order; order.reserve(C);
  std::vector<int32_t> level(C, -1);
  std::vector<char> placed(C, 0);
  auto bfs = [&](int start, std::vector<int32_t>* visit) {      // levels from `start` over unplaced nodes; returns the last node of minimum degree in the deepest level
    visit->clear();
    visit->push_back(start); level[start] = 0;
    for (size_t q = 0; q < visit->size(); ++q) {
      const int u = (*visit)[q];
      for (const int32_t* p = g.begin(u); p != g.end(u); ++p) { const int v = *p; if (!placed[v] && level[v] < 0) { level[v] = level[u] + 1; visit->push_back(v); } }
    }
    const int depth = level[visit->back()];
    int best = visit->back();
    for (int v : *visit) if (level[v] == depth && g.degree(v) < g.degree(best)) best = v;
    for (int v : *visit) level[v] = -1;
    return std::make_pair(best, depth);
  };
  std::vector<int32_t> by_degree(C);
  std::iota(by_degree.begin(), by_degree.end(), 0);
  std::stable_sort(by_degree.begin(), by_degree.end(), [&](int a, int b) { return g.degree(a) < g.degree(b); });
  std::vector<int32_t> visit, nb;
  for (int seed : by_degree) {
    if (placed[seed] || g.degree(seed) == 0) continue;
    int start = seed, ecc = -1;
    for (int round = 0; round < 4; ++round) {      // pseudo-peripheral node (two or three searches settle it on these graphs)
      const auto far = bfs(start, &visit);
      if (far.second <= ecc) break;
      ecc = far.second; start = far.first;
    }
    const size_t first = order.size();
    order.push_back(start); placed[start] = 1;
    for (size_t q = first; q < order.size(); ++q) {
      const int u = order[q];
      nb.clear();
      for (const int32_t* p = g.begin(u); p != g.end(u); ++p) { const int v = *p; if (!placed[v]) { placed[v] = 1; nb.push_back(v); } }
      std::stable_sort(nb.begin(), nb.end(), [&](int a, int b) { return g.degree(a) < g.degree(b); });
      order.insert(order.end(), nb.begin(), nb.end());
    }
  }
  std::reverse(order.begin(), order.end());
  for (int c = 0; c < C; ++c) if (!placed[c]) order.push_back(c);
  return order;
}
inline std::vector<int32_t> ReverseCuthillMcKee(const Adjacency& adj) { return ReverseCuthillMcKeeOf(ListsGraph{adj}); }

// a vertex set in a band order of its own (Cuthill-McKee on the sub-graph of the set: its images with neighbours inside the set first, the others behind
// them).  The sub-graph is built with LOCAL indices in two flat arrays (the dissections call this for every part they look at: no per-call array of the whole
// graph's size, no vector per vertex); `loc` is scratch, -1 outside every call.
inline std::vector<int32_t> BandOrderOf(const std::vector<int32_t>& set, const Adjacency& adj, std::vector<int32_t>* loc) {
  const int n = (int)set.size();
  for (int i = 0; i < n; ++i) (*loc)[set[i]] = i;
  FlatGraph sub;
  sub.off.assign((size_t)n + 1, 0);
  size_t bound = 0;
  for (int i = 0; i < n; ++i) bound += adj[set[i]].size();
  sub.nb.resize(bound);
  size_t at = 0;
  for (int i = 0; i < n; ++i) {
    for (int u : adj[set[i]]) if ((*loc)[u] >= 0) sub.nb[at++] = (*loc)[u];
    sub.off[i + 1] = (int32_t)at;
  }
  for (int i = 0; i < n; ++i) (*loc)[set[i]] = -1;
  const std::vector<int32_t> order = ReverseCuthillMcKeeOf(sub);      // (vertices without neighbours inside the set come last, in the set's order)
  std::vector<int32_t> out(n);
  for (int i = 0; i < n; ++i) out[i] = set[order[i]];
  return out;
}

// A chain starts at a 64-column tile boundary and needs three block columns.  With w columns per image (ReducedColumns::W6) a part may start every
// 64 / gcd(64, w) images - 32 for w = 6, 8 for w = 8 - and holds at least 192 columns.
struct Grain {
  int align = 32, min_leaf = 32, min_right = 33;
  explicit Grain(int columns_per_image = 6) {
    int g = 64, b = columns_per_image;
    while (b) { const int t = g % b; g = b; b = t; }      // gcd(64, columns per image)
    align = 64 / g;
    min_leaf = ((192 + columns_per_image - 1) / columns_per_image + align - 1) / align * align;
    min_right = min_leaf + 1;
  }
  int min_cut() const { return min_leaf + min_right + 4; }      // the shortest sequence / set a dissector looks at
};

// ---- nested dissection of a BAND order ------------------------------------------------------------------------------------------------------------
// The one-launch factorisation runs a chain workgroup per independent sub-tree of the elimination tree, so a band of T block columns costs T steps of one
// chain, while [left part | right part | the images that couple them] costs max(left, right) + separator steps of two.  A cut position c of the sequence:
// the separator is every image at a position >= c with a neighbour before c, the right part the rest of [c, n); parts are dissected again (`levels`).
// Cuts are multiples of Grain::align images, and a part starts where its parent started plus such a cut.  A cut is taken when it shortens the sequence's chain
// (max(left, right) + separator) to at most 0.8 of its length.  A PART is first put into a band order of its own when that gives the better cut: the parts
// of a ring folded flat are open bands of half its width.
struct BandCut { int c = -1, cost = 0; std::vector<int32_t> first_nb; };
inline BandCut BestBandCut(const std::vector<int32_t>& seq, const Adjacency& adj, std::vector<int32_t>* pos, int bias, const Grain& gr) {
  const int n = (int)seq.size();
  BandCut cut;
  cut.cost = n;
  for (int i = 0; i < n; ++i) (*pos)[seq[i]] = i;
  cut.first_nb.resize(n);
  for (int i = 0; i < n; ++i) {
    int m = i;
    for (int v : adj[seq[i]]) if ((*pos)[v] >= 0) m = std::min(m, (int)(*pos)[v]);
    cut.first_nb[i] = m;
  }
  for (int i = 0; i < n; ++i) (*pos)[seq[i]] = -1;
  // separator size per cut position by a sweep: image i belongs to the separator of every cut c with first_nb[i] < c <= i
  std::vector<int32_t> diff(n + 2, 0);
  for (int i = 0; i < n; ++i) if (cut.first_nb[i] < i) { diff[cut.first_nb[i] + 1] += 1; diff[i + 1] -= 1; }
  int sep = 0;
  for (int c = 1; c + gr.min_right <= n; ++c) {
    sep += diff[c];
    if (c < gr.min_leaf || c % gr.align) continue;
    const int right = n - c - sep;
    if (right < gr.min_right) continue;
    // (bias: the left part's chain stops and its contributions reach the separator two steps - 21 images - behind its last column, the right part's
    // chain runs on into the separator: an even split makes that chain wait.  Both are tried.)
    const int cost = std::max(c + bias, right) + sep;
    if (cost < cut.cost) { cut.cost = cost; cut.c = c; }
  }
  return cut;
}
// (the eight trials of DissectionCandidates - one to four levels, two balances - look at the same parts again and again: a part's band order and best cut are
// kept per (sequence, re-ordered or not, balance), keyed on the sequence itself; a map's nodes stay where they are when it grows)
struct BandDissector {
  const Adjacency& adj;
  const Grain gr;
  std::vector<int32_t> pos;
  struct Node { std::vector<int32_t> seq; BandCut cut; };      // seq: the order the cut refers to (the part's own band order, or the one it inherited)
  std::map<std::tuple<bool, int, std::vector<int32_t>>, Node, std::less<>> memo;      // (std::less<>: looked up by references, no copy of the sequence)
  BandDissector(const Adjacency& a, const Grain& g) : adj(a), gr(g), pos(a.size(), -1) {}
  const Node& NodeOf(const std::vector<int32_t>& seq_in, bool reorder, int bias) {
    const auto found = memo.find(std::tie(reorder, bias, seq_in));
    if (found != memo.end()) return found->second;
    Node nd;
    nd.cut = BestBandCut(seq_in, adj, &pos, bias, gr);
    if (reorder) {
      std::vector<int32_t> own = BandOrderOf(seq_in, adj, &pos);
      BandCut cut2 = BestBandCut(own, adj, &pos, bias, gr);
      if (cut2.c >= 0 && cut2.cost < nd.cut.cost) { nd.cut = std::move(cut2); nd.seq = std::move(own); }
    }
    if (nd.seq.empty()) nd.seq = seq_in;
    return memo.emplace(std::make_tuple(reorder, bias, seq_in), std::move(nd)).first->second;
  }
  struct Parts { std::vector<int32_t> left, right, sep; };      // of a sequence's cut: [left | right | separator]; left empty = no cut pays
  Parts PartsOf(const std::vector<int32_t>& seq_in, bool reorder, int bias) {
    Parts p;
    const int n = (int)seq_in.size();
    const Node& nd = NodeOf(seq_in, reorder, bias);
    if (nd.cut.c < 0 || nd.cut.cost * 5 > n * 4) return p;
    p.left.assign(nd.seq.begin(), nd.seq.begin() + nd.cut.c);
    for (int i = nd.cut.c; i < n; ++i) (nd.cut.first_nb[i] < nd.cut.c ? p.sep : p.right).push_back(nd.seq[i]);
    return p;
  }
  std::vector<int32_t> Dissect(const std::vector<int32_t>& seq_in, int levels, bool reorder, int bias) {
    if (levels <= 0 || (int)seq_in.size() < gr.min_cut()) return seq_in;
    const Parts p = PartsOf(seq_in, reorder, bias);
    if (p.left.empty()) return seq_in;
    std::vector<int32_t> out = Dissect(p.left, levels - 1, true, bias);
    const std::vector<int32_t> r = Dissect(p.right, levels - 1, true, bias);
    out.insert(out.end(), r.begin(), r.end());
    out.insert(out.end(), p.sep.begin(), p.sep.end());
    return out;
  }
};

// ---- nested dissection of the GRAPH -----------------------------------------------------------------------------------------------------------------
// Order of a vertex set: [part | part | ... | separator].  The set's connected components are parts of their own (nothing couples them: no separator);
// a connected set is cut by a vertex separator taken from the level structure of a pseudo-peripheral vertex: level j, reduced to its vertices with a
// neighbour in level j + 1 (the others join the near side); the far side's components become parts.  The level with the smallest
// max(largest part) + separator is taken if that is at most 0.8 of the set.  Every part but the last must be a multiple of Grain::align images long (the next one
// starts at a tile boundary): the remainder moves into the separator - vertices next to the separator first.  Leaves are put into a band order of their own.
struct GraphDissector {
  const Adjacency& adj;
  const Grain gr;
  std::vector<int32_t> tag, level, comp;      // scratch, -1 outside every call
  GraphDissector(const Adjacency& a, const Grain& g) : adj(a), gr(g), tag(a.size(), -1), level(a.size(), -1), comp(a.size(), -1) {}

  // connected components of a set (tag marks membership during the call)
  std::vector<std::vector<int32_t>> Components(const std::vector<int32_t>& set) {
    std::vector<std::vector<int32_t>> out;
    for (int v : set) tag[v] = 0;
    std::vector<int32_t> stack;
    for (int s : set) {
      if (tag[s] != 0) continue;
      out.emplace_back();
      tag[s] = 1; stack.push_back(s);
      while (!stack.empty()) {
        const int u = stack.back(); stack.pop_back();
        out.back().push_back(u);
        for (int v : adj[u]) if (tag[v] == 0) { tag[v] = 1; stack.push_back(v); }
      }
    }
    for (int v : set) tag[v] = -1;
    return out;
  }
  // breadth-first levels of a connected set from `root`; returns the levels
  std::vector<std::vector<int32_t>> Levels(const std::vector<int32_t>& set, int root) {
    for (int v : set) tag[v] = 0;
    std::vector<std::vector<int32_t>> lv(1, std::vector<int32_t>{root});
    tag[root] = 1;
    for (;;) {
      std::vector<int32_t> next;
      for (int u : lv.back()) for (int v : adj[u]) if (tag[v] == 0) { tag[v] = 1; next.push_back(v); }
      if (next.empty()) break;
      lv.push_back(std::move(next));
    }
    for (int v : set) tag[v] = -1;
    return lv;
  }

  struct Split { std::vector<std::vector<int32_t>> parts; std::vector<int32_t> sep; int cost = 0; };
  // the best level-structure separator of a connected set, or parts.empty()
  Split BestSplit(const std::vector<int32_t>& set) {
    Split best;
    const int n = (int)set.size();
    best.cost = n;
    if (n < gr.min_cut()) return best;
    // pseudo-peripheral root: repeated searches from a minimum-degree vertex of the last level
    int root = set[0];
    for (int v : set) if (adj[v].size() < adj[root].size()) root = v;
    std::vector<std::vector<int32_t>> lv = Levels(set, root);
    for (int round = 0; round < 6; ++round) {
      int far = lv.back()[0];
      for (int v : lv.back()) if (adj[v].size() < adj[far].size()) far = v;
      std::vector<std::vector<int32_t>> lv2 = Levels(set, far);
      if (lv2.size() <= lv.size()) break;
      lv.swap(lv2);
    }
    const int m = (int)lv.size();
    if (m < 3) return best;
    for (size_t j = 0; j < lv.size(); ++j) for (int v : lv[j]) level[v] = (int)j;
    // per vertex: does it touch the next / the previous level (one pass over the edges); per level: how many do
    std::vector<int32_t> below(m + 1, 0), touch_up(m, 0), touch_down(m, 0);
    for (int j = 0; j < m; ++j) below[j + 1] = below[j] + (int)lv[j].size();
    for (int v : set) {
      bool up = false, down = false;
      for (int u : adj[v]) { const int l = level[u]; if (l < 0) continue; up = up || l == level[v] + 1; down = down || l == level[v] - 1; }
      comp[v] = (up ? 1 : 0) | (down ? 2 : 0);
      touch_up[level[v]] += up ? 1 : 0; touch_down[level[v]] += down ? 1 : 0;
    }
    int best_j = -1, best_dir = 0;
    for (int j = 1; j + 1 < m; ++j) {
      // dir 0: the separator is the part of level j that touches level j + 1 (the rest of the level joins the near side); dir 1: the part that touches
      // level j - 1 (the rest joins the far side)
      for (int dir = 0; dir < 2; ++dir) {
        const int sz = (int)lv[j].size(), sep = dir ? touch_down[j] : touch_up[j];
        const int near = below[j] + (dir ? 0 : sz - sep), far = n - below[j + 1] + (dir ? sz - sep : 0);
        if (near < gr.min_leaf || far < gr.min_right) continue;
        const int cost = std::max(near, far) + sep + (near % gr.align);      // (the far side may fall into components: counted whole here, split below)
        if (cost < best.cost) { best.cost = cost; best_j = j; best_dir = dir; }
      }
    }
    if (best_j >= 0) {
      const int j = best_j, dir = best_dir;
      std::vector<int32_t> near, far;
      for (int v : set) {
        const int l = level[v];
        if (l < j) near.push_back(v);
        else if (l > j) far.push_back(v);
        else if (comp[v] & (dir ? 2 : 1)) best.sep.push_back(v);
        else (dir ? far : near).push_back(v);
      }
      best.parts.push_back(std::move(near));
      best.parts.push_back(std::move(far));
    }
    for (int v : set) comp[v] = -1;
    for (int v : set) level[v] = -1;
    return best;
  }

  // parts -> aligned parts: every part but the last gives its remainder (mod Grain::align) to `tail`, vertices adjacent to `tail`/`sep` first; parts that
  // become shorter than a chain join the tail whole
  void Align(std::vector<std::vector<int32_t>>* parts, std::vector<int32_t>* tail) {
    std::vector<std::vector<int32_t>> out;
    for (int v : *tail) tag[v] = 2;
    for (size_t i = 0; i < parts->size(); ++i) {
      std::vector<int32_t>& p = (*parts)[i];
      const bool last = i + 1 == parts->size();
      if ((int)p.size() < (last ? gr.min_right : gr.min_leaf)) { for (int v : p) { tail->push_back(v); tag[v] = 2; } continue; }
      const int rem = last ? 0 : (int)p.size() % gr.align;
      if (rem) {
        // boundary vertices (a neighbour in the tail) first
        std::stable_partition(p.begin(), p.end(), [&](int v) { for (int u : adj[v]) if (tag[u] == 2) return false; return true; });
        for (int r = 0; r < rem; ++r) { const int v = p.back(); p.pop_back(); tail->push_back(v); tag[v] = 2; }
      }
      out.push_back(std::move(p));
    }
    for (int v : *tail) tag[v] = -1;
    parts->swap(out);
  }

  // (DissectionCandidates asks for one to four levels: the deeper calls meet the shallower ones' parts again - a set's cut and its leaf order are kept, keyed on
  // the set itself; a map's nodes stay where they are when the recursion adds to it, so the references below hold across it)
  struct Cut { std::vector<std::vector<int32_t>> parts; std::vector<int32_t> tail; };      // parts empty: the set takes no cut
  std::map<std::vector<int32_t>, Cut> cuts;
  std::map<std::vector<int32_t>, std::vector<int32_t>> leaves;
  const std::vector<int32_t>& LeafOf(const std::vector<int32_t>& set) {
    const auto found = leaves.find(set);
    return found != leaves.end() ? found->second : leaves.emplace(set, BandOrderOf(set, adj, &tag)).first->second;
  }
  const Cut& CutOf(const std::vector<int32_t>& set) {
    const auto found = cuts.find(set);
    if (found != cuts.end()) return found->second;
    Cut c;
    const int n = (int)set.size();
    std::vector<std::vector<int32_t>> parts = Components(set);
    std::vector<int32_t> tail;
    bool cut_found = parts.size() > 1;
    if (!cut_found) {
      Split sp = BestSplit(set);
      if (!sp.parts.empty() && sp.cost * 5 <= n * 4) {
        cut_found = true;
        tail = std::move(sp.sep);
        std::vector<std::vector<int32_t>> far = Components(sp.parts[1]);      // the far side's components are parts of their own
        parts.clear();
        parts.push_back(std::move(sp.parts[0]));
        for (auto& f : far) parts.push_back(std::move(f));
      }
    }
    if (cut_found) {
      // large parts first (their chains are the long ones), the largest LAST: it needs no alignment and its chain runs on into the tail
      std::stable_sort(parts.begin(), parts.end(), [](const std::vector<int32_t>& a, const std::vector<int32_t>& b) { return a.size() > b.size(); });
      if (parts.size() > 1) std::rotate(parts.begin(), parts.begin() + 1, parts.end());
      Align(&parts, &tail);
      if (parts.size() > 1 || (parts.size() == 1 && !tail.empty())) { c.parts = std::move(parts); c.tail = std::move(tail); }
    }
    return cuts.emplace(set, std::move(c)).first->second;
  }
  std::vector<int32_t> Dissect(const std::vector<int32_t>& set, int levels) {
    if (levels <= 0 || (int)set.size() < gr.min_cut()) return LeafOf(set);
    const Cut& cut = CutOf(set);
    if (cut.parts.empty()) return LeafOf(set);
    std::vector<int32_t> out; out.reserve(set.size());
    for (const std::vector<int32_t>& part : cut.parts) {
      const std::vector<int32_t> o = Dissect(part, levels - 1);
      out.insert(out.end(), o.begin(), o.end());
    }
    if (!cut.tail.empty()) { const std::vector<int32_t>& t = LeafOf(cut.tail); out.insert(out.end(), t.begin(), t.end()); }
    return out;
  }
};

// ---- what the problem says before any graph is built ----------------------------------------------------------------------------------------------
// Per-image intrinsics beside their pose columns.  BundleAdjuster::ParameterizeCameras (src/optim/bundle_adjustment.cc:490-528) makes a camera block
// variable under a refine flag; a reconstruction in which every image has its own camera then has C more parameter blocks, each coupled with the same images as
// its own pose.  Behind all pose columns they are 6 C + ... dense-looking block rows that every part of a dissection waits for (500 images, f and k variable:
// 39 chain steps instead of ~25); beside their image's pose columns they belong to that image's part.  Returns n_v > 0 when EVERY image's camera is variable,
// referenced by that image alone, with the same even number n_v of variable parameters (the pose blocks stay 16-byte aligned in the reduced system) - the
// reduced system then has 6 + n_v columns per image and no tail -, 0 otherwise (variable intrinsics, if any, follow the pose columns).  PPSFM_BA_INTR_LAYOUT=tail: 0.
// cam_np: the parameters of every camera's model (CameraNumParams of camera_model).
inline int PrivateIntrinsicsColumns(const pp_ba_problem_desc* d, const int32_t* cam_np, IntrLayout layout) {
  if (!d->camera_const_mask || layout == IntrLayout::Tail) return 0;
  const int C = d->num_poses, K = d->num_cameras;
  std::vector<int32_t> users(K, 0);
  for (int c = 0; c < C; ++c) users[d->pose_camera[c]]++;
  int nv_all = -1;
  for (int c = 0; c < C; ++c) {
    const int k = d->pose_camera[c];
    if (users[k] != 1) return 0;
    int nv = 0;
    for (int j = 0; j < cam_np[k]; ++j) if (!((d->camera_const_mask[k] >> j) & 1)) ++nv;
    if (nv == 0 || (nv & 1) || (nv_all >= 0 && nv != nv_all)) return 0;
    nv_all = nv;
  }
  return nv_all > 0 ? nv_all : 0;
}
// the reduced camera system is solved by conjugate gradients (ba_pcg.hip): the descriptor's linear solver unless PPSFM_BA_LINEAR_SOLVER overrides it -
// ITERATIVE_SCHUR above PP_MAX_NUM_IMAGES_DIRECT_SOLVER images for AUTO (bundle_adjustment.cc:273-286)
inline bool WillIterate(const pp_ba_problem_desc* d, LinearSolverSwitch sw) {
  const int ls = sw == LinearSolverSwitch::Iterative ? PP_LINEAR_SOLVER_ITERATIVE_SCHUR : (sw == LinearSolverSwitch::Direct ? PP_LINEAR_SOLVER_DIRECT : d->linear_solver);
  return ls == PP_LINEAR_SOLVER_ITERATIVE_SCHUR || (ls == PP_LINEAR_SOLVER_AUTO && d->num_poses > PP_MAX_NUM_IMAGES_DIRECT_SOLVER);
}
// what decides whether an order is looked for at all, the column layout and the grain of the cuts.  PPSFM_BA_ORDERING: natural | rcm (forced even where
// it does not pay: tests) | band (no dissection) | unset = by chain steps
struct OrderingSetup { bool will_iterate, forced, candidate; ReducedColumns cols; Grain grain; };
inline OrderingSetup SetupOf(const pp_ba_problem_desc* d, int NI, const int32_t* cam_np, const Switches& sw) {
  const int C = d->num_poses;
  const bool will_iterate = WillIterate(d, sw.ba_linear_solver), forced = sw.ba_ordering == OrderingSwitch::Rcm;
  const ReducedColumns cols(C, NI, will_iterate ? 0 : PrivateIntrinsicsColumns(d, cam_np, sw.ba_intr_layout));
  const bool candidate = d->ordering == PP_ORDERING_AUTO && sw.ba_ordering != OrderingSwitch::Natural && !will_iterate && C >= 3 &&
                         (forced || (sw.ba_sparse && cols.Tt >= 8));
  return OrderingSetup{will_iterate, forced, candidate, cols, Grain(cols.W6)};
}
// true when ChooseImageOrdering will build the co-visibility graph from the observations (pp_ba_create then hands it the graph's bits from the device,
// pair_lists.hip CoVisibilityOnDevice, where the by-point lists are anyway)
inline bool OrderingReadsObservations(const pp_ba_problem_desc* d, int NI, const int32_t* cam_np, const Switches& sw) { return SetupOf(d, NI, cam_np, sw).candidate && !d->covisibility; }

// ---- the co-visibility graph ----------------------------------------------------------------------------------------------------------------------
// Two images are neighbours when a variable point is seen by both and neither is fixed (ImageIsFixed).  As a bit matrix: C rows of BitWords(C) words,
// bit j of row i for j < i.  Three sources: the observations, the caller's matrix, the bits pp_ba_create built on the device.
inline int BitWords(int C) { return (C + 63) / 64; }
// filled point by point from the observations.  `stop_at` > 0: the fill stops once that many distinct edges exist (the caller's "too dense for any order
// to pay"); returns false then.
inline bool FillFromObservations(const pp_ba_problem_desc* d, int nv_private, int64_t stop_at, uint64_t* b) {
  const int C = d->num_poses, P = d->num_points, W = BitWords(C);
  const int64_t M = d->num_obs;
  // observations grouped by point: the caller's arrays as they are when obs_point never decreases (BundleAdjuster::SetUp adds a point's track at a time,
  // src/optim/bundle_adjustment.cc:330-338), a counting sort otherwise
  std::vector<int32_t> ps(P + 1, 0), po_sorted;
  bool grouped = true;
  for (int64_t o = 0; o < M; ++o) { ps[d->obs_point[o] + 1]++; grouped = grouped && (o == 0 || d->obs_point[o] >= d->obs_point[o - 1]); }
  for (int p = 0; p < P; ++p) ps[p + 1] += ps[p];
  if (!grouped) { po_sorted.resize(M); std::vector<int32_t> f(ps.begin(), ps.end() - 1); for (int64_t o = 0; o < M; ++o) po_sorted[f[d->obs_point[o]]++] = d->obs_pose[o]; }
  const int32_t* po_base = grouped ? d->obs_pose : po_sorted.data();
  std::vector<uint8_t> fixed(C, 0);
  for (int c = 0; c < C; ++c) fixed[c] = ImageIsFixed(nv_private, d->pose_const, c) ? 1 : 0;
  int64_t edges = 0;
  std::vector<int32_t> obs;      // the variable observers of one point
  for (int p = 0; p < P; ++p) {
    if (d->point_const && d->point_const[p]) continue;
    obs.clear();
    for (int e = ps[p]; e < ps[p + 1]; ++e) if (!fixed[po_base[e]]) obs.push_back(po_base[e]);
    const int n = (int)obs.size();
    const int32_t* v = obs.data();
    for (int a = 1; a < n; ++a) {
      const int ca = v[a];
      for (int c = 0; c < a; ++c) {
        const int cb = v[c];
        const int hi = ca > cb ? ca : cb, lo = ca > cb ? cb : ca;      // lower triangle only (an image seen twice by a point: a bit on the diagonal, not counted)
        uint64_t& w = b[(size_t)hi * W + (lo >> 6)];
        const uint64_t m = 1ull << (lo & 63);
        edges += (hi != lo) & !(w & m);
        w |= m;
      }
    }
    if (stop_at > 0 && edges >= stop_at) return false;
  }
  return true;
}
// from the caller's (a point-sharded group's UNION) co-visibility: C x C bytes, read as symmetric; returns the edges it found
inline int64_t FillFromMatrix(const pp_ba_problem_desc* d, int nv_private, uint64_t* b) {
  const int C = d->num_poses;
  int64_t edges = 0;
  for (int i = 1; i < C; ++i)
    for (int j = 0; j < i && !ImageIsFixed(nv_private, d->pose_const, i); ++j)
      if ((d->covisibility[(size_t)i * C + j] || d->covisibility[(size_t)j * C + i]) && !ImageIsFixed(nv_private, d->pose_const, j)) { b[(size_t)i * BitWords(C) + (j >> 6)] |= 1ull << (j & 63); ++edges; }
  return edges;
}
// the neighbour lists of a bit matrix (bits on the diagonal are no edges)
inline Adjacency AdjacencyOf(int C, const uint64_t* bits) {
  const int W = BitWords(C);
  Adjacency adj(C);
  for (int i = 0; i < C; ++i) adj[i].reserve(16);
  for (int i = 0; i < C; ++i)
    for (int w = 0; w <= (i >> 6); ++w) {
      uint64_t m = bits[(size_t)i * W + w];
      while (m) { const int j = 64 * w + __builtin_ctzll(m); m &= m - 1; if (j != i) { adj[i].push_back(j); adj[j].push_back(i); } }
    }
  for (int i = 0; i < C; ++i) std::sort(adj[i].begin(), adj[i].end());
  return adj;
}
// The graph ChooseImageOrdering works on: from the caller's matrix when there is one, else from `graph_bits` when given, else from the observations.
// A tile of the reduced system holds at least 10 x 10 image pairs, so an order can empty at most (non-edges / 100) tiles: once fewer than a tenth of the
// tiles could go, no order is taken (BandCandidate's rule) and the fill stops - a clique leaves after a fraction of its pairs.  Returns false then
// (never when the order is forced).
inline bool CoVisibilityGraph(const pp_ba_problem_desc* d, const OrderingSetup& setup, const uint64_t* graph_bits, Adjacency* adj) {
  const int C = d->num_poses, nv_private = setup.cols.nv_private;
  int64_t variable = 0;
  for (int c = 0; c < C; ++c) variable += ImageIsFixed(nv_private, d->pose_const, c) ? 0 : 1;
  const int64_t all_pairs = variable * (variable - 1) / 2, total_tiles = (int64_t)setup.cols.Tt * (setup.cols.Tt + 1) / 2;
  const int64_t stop_at = setup.forced ? 0 : std::max<int64_t>(1, all_pairs - 10 * total_tiles + 1);      // non-edges < total_tiles / 10 * 100
  std::vector<uint64_t> own(d->covisibility || !graph_bits ? (size_t)C * BitWords(C) : 0, 0);      // (the device's bits are read where they are)
  if (d->covisibility) {
    if (FillFromMatrix(d, nv_private, own.data()) >= stop_at && stop_at > 0) return false;
  } else if (graph_bits) {
    int64_t edges = 0;
    for (int i = 1; i < C; ++i) for (int w = 0; w <= (i >> 6); ++w) edges += __builtin_popcountll(graph_bits[(size_t)i * BitWords(C) + w]);
    if (stop_at > 0 && edges >= stop_at) return false;
  } else if (!FillFromObservations(d, nv_private, stop_at, own.data())) return false;
  *adj = AdjacencyOf(C, own.empty() ? graph_bits : own.data());
  return true;
}

// the tile map of an order (image c at position pos[c]; null: the caller's order), closed under fill-in; returns its non-zero tiles
inline int TileMapOf(const ReducedColumns& cols, const Adjacency& adj, const int32_t* pos, std::vector<uint8_t>* nz) {
  const int C = (int)adj.size();
  nz->assign((size_t)cols.Tt * cols.Tt, 0);
  auto at = [&](int c) { return pos ? pos[c] : c; };
  for (int c = 0; c < C; ++c) { MarkImagePair(cols, at(c), at(c), nz->data()); for (int c2 : adj[c]) if (c2 < c) MarkImagePair(cols, at(c), at(c2), nz->data()); }
  MarkTailAndRhs(cols, nz->data());
  return CloseTileMap(cols.Tt, nz->data());
}
// the chain steps of a closed tile map's factorisation (the block columns on the longest dependency path when the block-sparse one-launch mode takes it,
// all of them otherwise) and its chains - from the chain plan alone; the winner's list is verified by VerifiedWinner
struct OrderCost { int nnz = 0, steps = 0, chains = 1; };
inline OrderCost PlanStepsOf(int Tt, const std::vector<uint8_t>& nz, int nnz, const PlanSwitches& ps) {
  if (!BlockSparsePays(Tt, nnz) || !UseTasks(Tt)) return OrderCost{nnz, Tt, 1};
  const ChainPlan plan = PlanChains(Tt, nz.data(), ps);
  return OrderCost{nnz, plan.Steps(), plan.cr.n};
}

// (PPSFM_ORDER_DEBUG: where the time of an ordering goes, on stderr)
struct LapTimer {
  using Clock = std::chrono::steady_clock;
  const bool print;
  const Clock::time_point begin = Clock::now();
  Clock::time_point last = begin;
  double MsSince(Clock::time_point t) const { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }
  void Lap(const char* what) { if (print) { fprintf(stderr, "ppsfm:   %-28s %.3f ms\n", what, MsSince(last)); last = Clock::now(); } }
};

struct Candidate { std::vector<int32_t> oon, noo; OrderCost cost; };      // oon empty: the caller's order
inline std::vector<int32_t> InverseOf(const std::vector<int32_t>& oon) {
  std::vector<int32_t> noo(oon.size());
  for (size_t i = 0; i < oon.size(); ++i) noo[oon[i]] = (int32_t)i;
  return noo;
}
// The band: Cuthill-McKee, taken when it removes at least a tenth of the factor's tiles (a dense co-visibility keeps the caller's order: nothing to gain,
// and the solve stays bit-for-bit what it was) or when forced; the caller's order otherwise.  nnz_natural / nnz_rcm: the tiles of the two orders.
inline Candidate BandCandidate(const OrderingSetup& setup, const Adjacency& adj, const PlanSwitches& ps, int* nnz_natural, int* nnz_rcm) {
  const int Tt = setup.cols.Tt;
  std::vector<uint8_t> nz;
  Candidate rcm;
  rcm.oon = ReverseCuthillMcKee(adj);
  rcm.noo = InverseOf(rcm.oon);
  *nnz_natural = TileMapOf(setup.cols, adj, nullptr, &nz);
  Candidate natural;
  natural.cost = PlanStepsOf(Tt, nz, *nnz_natural, ps);
  natural.cost.chains = 1;      // (the caller's order is reported as one chain, whatever its plan says)
  *nnz_rcm = TileMapOf(setup.cols, adj, rcm.noo.data(), &nz);
  bool identity = true;
  for (size_t i = 0; i < rcm.oon.size(); ++i) identity = identity && rcm.oon[i] == (int32_t)i;
  if (identity || !(setup.forced || (int64_t)*nnz_rcm * 10 <= (int64_t)*nnz_natural * 9)) return natural;
  rcm.cost = PlanStepsOf(Tt, nz, *nnz_rcm, ps);
  return rcm;
}

// The dissections that beat the band, best first: eight trials on the band (one to four levels, cuts balanced evenly / in favour of the part whose chain
// runs on - the bias), then up to four levels on the graph itself (separators from level structures: clusters, hubs - what no band order shows).  The
// graph is asked when the cuts of the band left more than 0.7 of its steps: on sequences, rings and the clustered collections of the tests the band's cuts -
// parts re-ordered by their own Cuthill-McKee - find the same separators, and the graph's would only cost their milliseconds (PPSFM_BA_GRAPH_ND=1 / 0:
// always / never).  A dissection has MORE tiles than its band - the separators' rows fill - and pays when the chain it shortens is what bounds the
// factorisation: taken from 0.95 of the band's steps; among dissections the fewest steps, then the most chains.
struct DissectionTrials {
  const OrderingSetup& setup;
  const Adjacency& adj;
  const Candidate& band;
  const Switches& sw;
  std::vector<int32_t> connected, rest;      // the band's images with neighbours (what is dissected) and those without (they stay behind)
  std::vector<std::vector<int32_t>> tried;
  std::vector<Candidate> ranked;
  std::vector<uint8_t> nz;
  DissectionTrials(const OrderingSetup& u, const Adjacency& a, const Candidate& b, const Switches& s) : setup(u), adj(a), band(b), sw(s) {
    for (int i = 0; i < (int)adj.size(); ++i) { const int c = band.oon.empty() ? i : band.oon[i]; (adj[c].empty() ? rest : connected).push_back(c); }
  }
  // false: the same order as the band or as an earlier trial (deeper levels / the other balance found no new cut)
  bool Consider(std::vector<int32_t> order) {
    if (order == connected || std::find(tried.begin(), tried.end(), order) != tried.end()) return false;
    tried.push_back(order);
    order.insert(order.end(), rest.begin(), rest.end());
    Candidate c;
    c.noo = InverseOf(order);
    c.cost = PlanStepsOf(setup.cols.Tt, nz, TileMapOf(setup.cols, adj, c.noo.data(), &nz), sw.plan);
    c.oon.swap(order);
    if (sw.order_debug) fprintf(stderr, "ppsfm:   candidate: %d tiles, %d chains, %d steps (band: %d tiles, %d steps)\n", c.cost.nnz, c.cost.chains, c.cost.steps, band.cost.nnz, band.cost.steps);
    if (c.cost.chains > 1 && c.cost.steps * 100 <= band.cost.steps * 95) ranked.push_back(std::move(c));
    return true;
  }
};
inline std::vector<Candidate> DissectionCandidates(const OrderingSetup& setup, const Adjacency& adj, const Candidate& band, const Switches& sw, LapTimer* timer) {
  DissectionTrials trials(setup, adj, band, sw);
  const int bias_images = 128 / setup.cols.W6;      // (two chain steps: see BestBandCut)
  BandDissector bd(adj, setup.grain);
  for (int trial = 0; trial < 8; ++trial) {
    std::vector<int32_t> order = bd.Dissect(trials.connected, 1 + trial / 2, false, (trial & 1) ? bias_images : 0);
    if (order == trials.connected) { if (trial & 1) break; continue; }
    trials.Consider(std::move(order));
  }
  timer->Lap("band dissections");
  int best_band_steps = band.cost.steps;
  for (const Candidate& c : trials.ranked) best_band_steps = std::min(best_band_steps, c.cost.steps);
  const bool graph_nd = sw.ba_graph_nd >= 0 ? sw.ba_graph_nd != 0 : best_band_steps * 10 > band.cost.steps * 7;
  GraphDissector gd(adj, setup.grain);
  for (int levels = 1; graph_nd && levels <= 4; ++levels) if (!trials.Consider(gd.Dissect(trials.connected, levels)) && levels > 1) break;
  timer->Lap("graph dissections");
  std::stable_sort(trials.ranked.begin(), trials.ranked.end(), [](const Candidate& a, const Candidate& b) { return a.cost.steps != b.cost.steps ? a.cost.steps < b.cost.steps : a.cost.chains > b.cost.chains; });
  return std::move(trials.ranked);
}

// chain steps and *chains of the factorisation of a closed Tt x Tt tile map from its plan, its task list and the list's replay (the library binds
// cholesky.hip's CholeskyChainSteps, whose process-wide cache then holds the winner's plan for the handle's first solve; a host driver, PlanAndList)
using VerifyPlan = std::function<int(int Tt, const uint8_t* nz, int* chains)>;
// the best dissection whose task list confirms what its plan promised (a list of several chains that fails its replay would run as one chain: the next
// candidate then), or the band.  The winner's list is built and replayed ONCE.
inline Candidate* VerifiedWinner(const OrderingSetup& setup, const Adjacency& adj, Candidate* band, std::vector<Candidate>* ranked, const VerifyPlan& verify) {
  std::vector<uint8_t> nz;
  for (Candidate& c : *ranked) {
    (void)TileMapOf(setup.cols, adj, c.noo.data(), &nz);
    int chains = 1;
    const int steps = verify(setup.cols.Tt, nz.data(), &chains);
    if (chains == c.cost.chains && steps == c.cost.steps) return &c;
  }
  return band;
}

// old_of_new empty = the caller's order.  nnz_*: non-zero tiles of the factor in the caller's order / in the order taken (-1: not computed); dense_exit:
// the co-visibility turned out too dense for any order to pay and was not completed; chains / chain_steps: of the order taken (0: not planned);
// plan_ms: host time spent.
struct ImageOrdering { std::vector<int32_t> old_of_new, new_of_old; int nnz_natural = -1, nnz_ordered = -1, chains = 0, chain_steps = 0; bool dense_exit = false; double plan_ms = 0; };
inline ImageOrdering Finished(ImageOrdering out, const LapTimer& timer, int C) {
  out.plan_ms = timer.MsSince(timer.begin);
  if (timer.print) fprintf(stderr, "ppsfm: image ordering %.3f ms (%d images, %s)\n", out.plan_ms, C, out.dense_exit ? "co-visibility too dense: left early" : (out.old_of_new.empty() ? "caller's order" : "renumbered"));
  return out;
}
// `graph_bits` (the bit matrix above) replaces the walk over the observations when given.
inline ImageOrdering ChooseImageOrdering(const pp_ba_problem_desc* d, int NI, const int32_t* cam_np, const Switches& sw, const uint64_t* graph_bits, const VerifyPlan& verify) {
  LapTimer timer{sw.order_debug};
  const int C = d->num_poses;
  ImageOrdering out;
  const OrderingSetup setup = SetupOf(d, NI, cam_np, sw);
  if (!setup.candidate) return Finished(std::move(out), timer, C);
  Adjacency adj;
  if (!CoVisibilityGraph(d, setup, graph_bits, &adj)) { out.dense_exit = true; return Finished(std::move(out), timer, C); }
  timer.Lap("co-visibility graph");
  Candidate band = BandCandidate(setup, adj, sw.plan, &out.nnz_natural, &out.nnz_ordered);
  timer.Lap("cuthill-mckee + two tile maps");
  std::vector<Candidate> ranked;      // (PPSFM_BA_ORDERING = rcm (forced) / band (by tile count): the band order only; above 128 block columns there are no chains to gain)
  if (sw.ba_ordering != OrderingSwitch::Rcm && sw.ba_ordering != OrderingSwitch::Band && setup.cols.Tt <= 128) ranked = DissectionCandidates(setup, adj, band, sw, &timer);
  Candidate* const chosen = VerifiedWinner(setup, adj, &band, &ranked, verify);
  timer.Lap("winner's list + replay");
  if (!chosen->oon.empty()) { out.nnz_ordered = chosen->cost.nnz; out.old_of_new.swap(chosen->oon); out.new_of_old.swap(chosen->noo); }
  out.chains = chosen->cost.chains; out.chain_steps = chosen->cost.steps;
  return Finished(std::move(out), timer, C);
}

}  // namespace ppsfm

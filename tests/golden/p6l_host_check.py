#!/usr/bin/env python3
"""Re3q3Device / P6LDevice (csrc/p6l_device.hpp) compiled as HOST code behind a stand-alone driver, CPU only - the tool behind two statements of
tests/golden/gen_p6l_golden.py and docs/HISTORY.md:

  python tests/golden/p6l_host_check.py compare [MUTATION]   the comparison of tests/test_gpu_p6l_exact.py with the host build in the kernel's place;
                                                             MUTATION: sign (one PolyMac of row 2 of M(X)), perm (perm[1] where elim == 2), sweeps
                                                             (kAberthSweeps = 6), applied to a temporary copy of the header
  python tests/golden/p6l_host_check.py minor [N]            the search for a p6l_minor set: N (20 000) six-tuples drawn like p6l_clean and
                                                             p6l_outliers, the smallest |m00 m11 - m10 m01| / (|m00 m11| + |m10 m01|) at a returned root

The host build divides where the kernel uses v_rcp and does not contract to FMA: its figures are close to the kernel's, not equal."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

STUB = "#pragma once\n#include <cmath>\n#include <cstdio>\nusing std::isfinite;\n#define PP_HD inline\n"
DRIVER = r"""
#include "p6l_device.hpp"
#include <cstdlib>
#include <cstring>
#include <vector>
int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const bool p6l = !strcmp(argv[1], "p6l");
  const long n = atol(argv[4]);
  const int in_w = p6l ? 37 : 30, out_w = p6l ? 98 : 26;
  std::vector<double> in((size_t)n * in_w), out((size_t)n * out_w, 0.0);
  FILE* f = fopen(argv[2], "rb"); if (!f || fread(in.data(), 8, in.size(), f) != in.size()) return 3; fclose(f);
  for (long i = 0; i < n; ++i) {
    ppsfm::g_minor = 1.0;
    const double* a = &in[i * in_w];
    double* o = &out[i * out_w];
    o[0] = p6l ? ppsfm::P6LDevice(a, a + 18, a[36] != 0.0, o + 1, nullptr, nullptr) : ppsfm::Re3q3Device(a, o + 1, true, nullptr);
    o[out_w - 1] = ppsfm::g_minor;
  }
  f = fopen(argv[3], "wb"); fwrite(out.data(), 8, out.size(), f); fclose(f);
  return 0;
}
"""
MUTATIONS = {
    "sign": ("PolyMac<2, 1>(kz, pa[Z], 1.0, M20);", "PolyMac<2, 1>(kz, pa[Z], -1.0, M20);"),
    "perm": ("(elim == 1 ? c[10 * i + perm[1][j]] : c[10 * i + perm[2][j]]);", "(elim == 1 ? c[10 * i + perm[1][j]] : c[10 * i + perm[1][j]]);"),
    "sweeps": ("constexpr int kAberthSweeps = 40;", "constexpr int kAberthSweeps = 6;"),
}
HOOK = "    const double y = (m12 * m01 - m02 * m11) / (m00 * m11 - m10 * m01);"


def build(tmp, mutation=None):
    src = open(os.path.join(ROOT, "privacy_preserving_sfm_amd", "csrc", "p6l_device.hpp")).read()
    assert src.count(HOOK) == 1
    src = src.replace("namespace ppsfm {\n", "namespace ppsfm {\nstatic double g_minor = 1.0;\n", 1)
    src = src.replace(HOOK, "    { const double r_ = fabs(m00 * m11 - m10 * m01) / (fabs(m00 * m11) + fabs(m10 * m01)); if (r_ < g_minor) g_minor = r_; }\n" + HOOK)
    if mutation:
        old, new = MUTATIONS[mutation]
        assert src.count(old) == 1, mutation
        src = src.replace(old, new)
    for name, text in (("camera_models.hpp", STUB), ("p6l_device.hpp", src), ("driver.cpp", DRIVER)):
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", tmp, os.path.join(tmp, "driver.cpp"), "-o", os.path.join(tmp, "driver")])

    def run(mode, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        rows.tofile(os.path.join(tmp, "in.bin"))
        subprocess.check_call([os.path.join(tmp, "driver"), mode, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), str(len(rows))])
        return np.fromfile(os.path.join(tmp, "out.bin")).reshape(len(rows), -1)
    return run


def compare(run):
    import p6l_reference as ref
    import test_gpu_p6l_exact as T

    def re3q3(systems):
        o = run("re3q3", np.stack([e["c"].ravel() for e in systems]))
        return o[:, 1:25].reshape(-1, 3, 8).copy(), o[:, 0].astype(np.int32)

    def p6l(systems):
        o = run("p6l", np.stack([np.concatenate([e["lines"].ravel(), e["points"].ravel(), [float(e["aligned"].all())]]) for e in systems]))
        return o[:, 1:97].reshape(-1, 8, 3, 4).copy(), o[:, 0].astype(np.int32)
    T._re3q3, T._p6l = re3q3, p6l
    g = ref.load_golden()
    fails = 0
    for names, solve, checks in ((ref.QUADRIC_SETS + (ref.SPECIAL_SET,), re3q3, (T.check_quadrics_decided, T.check_quadrics_invariants)),
                                 (ref.P6L_SETS, p6l, (T.check_p6l_decided, T.check_p6l_invariants))):
        for name in names:
            out = solve(g[name]["systems"])
            for check in checks:
                try:
                    r = check(name, g[name], *out)
                    print("%-22s %-26s ok%s" % (name, check.__name__, "" if r is None else "  max rho / bound %.3g" % r))
                except AssertionError as ex:
                    fails += 1
                    print("%-22s %-26s FAIL %s" % (name, check.__name__, str(ex).replace("\n", " ")[:160]))
    for test in (T.test_scaled_rows_return_the_parents_roots, T.test_lane_position_prefixes_and_repeatability):
        try:
            test(g)
            print("%-49s ok" % test.__name__)
        except AssertionError as ex:
            fails += 1
            print("%-49s FAIL %s" % (test.__name__, str(ex).replace("\n", " ")[:160]))
    print("failed checks:", fails)
    return fails


def minor_search(run, n):
    import gen_p6l_golden as gen
    rng = np.random.default_rng(20261108)
    rows = []
    for i in range(n):
        t = gen.six_tuple(rng, 0.5 if i % 2 else 0.0, int(rng.integers(0, 4)) if i % 2 else 0)
        rows.append(np.concatenate([t["lines"].ravel(), t["points"].ravel(), [0.0]]))
    m = run("p6l", np.array(rows))[:, 97]
    print("%d six-tuples: smallest minor ratio %.3g, %d at or below 1e-6, %d below 1e-4" % (n, m.min(), (m <= 1e-6).sum(), (m < 1e-4).sum()))


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        if len(sys.argv) > 1 and sys.argv[1] == "minor":
            minor_search(build(tmp), int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
        else:
            sys.exit(1 if compare(build(tmp, sys.argv[2] if len(sys.argv) > 2 else None)) else 0)

"""CPU check of csrc/nerf_wgrad_table.h: for every recorded shape and combination of facts the table chooses the instance
and the wave split that wgrad_impl's macro chains chose before they became a table (tests/golden/wgrad_choice.txt, written by
tools/record_wgrad_choice.cpp from those chains).  The header has no HIP in it: any host C++17 compiler builds the program."""
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO

_PROGRAM = r"""
#include <cstdio>
#include "nerf_wgrad_table.h"
int main() {
  using namespace nerf;
  const int sizes[] = {1, 3, 27, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 161, 192, 193, 224, 225, 255, 256};
  for (int n_out : sizes) for (int n_in : sizes) for (int facts = 0; facts < 16; ++facts) {
    const WgChoice c = wg_choose(n_out, n_in, WgFacts{bool(facts & 1), bool(facts & 2), bool(facts & 4), bool(facts & 8)});
    std::printf("%d %d %d ", n_out, n_in, facts);
    if (c.row < 0 || c.form == kWgNoListKernel) { std::printf("none 0 0\n"); continue; }
    const WgRow& r = kWgRows[c.row];
    if (r.outs() < n_out || r.ins() < n_in) { std::printf("does-not-cover 0 0\n"); continue; }
    if (c.form == kWgPlain) std::printf("%s<%d,%d>", r.kind == kWgGeneric ? "f32" : "vec", r.wo, r.wi);
    else std::printf("%s<%d,%d,16>", c.form == kWgList ? "list" : "ring", r.wo, r.wi);
    std::printf(" %d %d\n", r.osplit, r.isplit);
  }
  return 0;
}
"""


def test_table_chooses_what_the_macro_chains_chose(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler available")
    src, exe = tmp_path / "choice.cpp", tmp_path / "choice"
    src.write_text(_PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(REPO, "nerf_replication_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    # the one instance that changed its name: nerf_wgrad256_f32_kernel was nerf_wgrad_vec_f32_kernel<4,4> written out by hand
    want = [l.replace(" w256 ", " vec<4,4> ") for l in open(os.path.join(GOLDEN, "wgrad_choice.txt")).read().splitlines()]
    assert len(want) == 22 * 22 * 16 and len(got) == len(want)
    assert [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:10] == []

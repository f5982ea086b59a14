"""The PROBAV_GEN1 grammar (csrc/w4_switch.h), on the host: a stand-alone program built with the host C++ compiler prints the parser's answer for
each value; the expected masks are the table of the header comment and INTEGRATION.md, written out here."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "proba-v_amd", "csrc")
C, W, F, B = 1, 2, 4, 8                      # conv3_w4, conv3_wgrad_w4, pw_fwd_w4, pw_bwd_w4 disabled (bit = the W4 enumerator)
TABLE = [(None, 0), ("", 0), ("0", 0), ("x", 0), ("p", 0),
         ("1", C | W | F | B), ("1conv", C | W | F | B),
         ("conv", C), ("c", C),
         ("wg", W), ("w", W),
         ("pw", F | B), ("pwx", F | B),
         ("pwf", F), ("pwb", B)]
PROGRAM = r"""
#include "w4_switch.h"
#include <cstdio>
#include <initializer_list>
using namespace probav;
static_assert((int)W4::conv == 0 && (int)W4::wgrad == 1 && (int)W4::pw_fwd == 2 && (int)W4::pw_bwd == 3, "W4");
int main(int argc, char** argv)
{
    printf("%u\n", w4_parse_disabled(nullptr));
    for (int i = 1; i < argc; ++i) printf("%u\n", w4_parse_disabled(argv[i]));
    // the predicate w4_enabled() applies to the parsed mask: none disabled, all disabled, pw_fwd alone disabled
    for (unsigned mask : {0u, 15u, 4u}) for (W4 k : {W4::conv, W4::wgrad, W4::pw_fwd, W4::pw_bwd}) printf("%d\n", (int)w4_mask_enabled(mask, k));
    return 0;
}
"""


def test_gen1_grammar(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "w4.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "w4")
    subprocess.check_call([cxx, "-std=c++17", "-I", CSRC, str(src), "-o", exe])
    values = [v for v, _ in TABLE if v is not None]
    out = subprocess.check_output([exe] + values, text=True).split()
    got = [int(t) for t in out]
    assert got[:len(TABLE)] == [m for _, m in TABLE], list(zip([v for v, _ in TABLE], got))
    assert got[len(TABLE):] == [1, 1, 1, 1,  0, 0, 0, 0,  1, 1, 0, 1]

"""CPU: the rank keys of smatrix_merge_topk / smatrix_merge_topk_by (libsmatrix_amd/csrc/kernels/rank_key.hpp) as host code, under
the undefined-behaviour and address sanitizers.  tests/c/rank_key_select.cpp, a program of its own, runs the selection kernels'
digit loop on both key policies -- seeded random keys, ties, keys that differ in one byte only, all scores 0, the extremes of
both halves, sets of two keys -- and wants the m-th largest key by std::sort for every m, and exactly m keys kept by the
emission's comparison.  A shift by 64 in the key arithmetic is a failure here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_digit_loop_finds_the_mth_largest_key_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rank_key_select")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "libsmatrix_amd", "csrc", "kernels"),
                    os.path.join(ROOT, "tests", "c", "rank_key_select.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RANK_KEY_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]

"""Developer tool (no GPU): the largest error of rk_log2, rk_exp2 and pw (rappas_amd/csrc/rk_divmath.h, through
rk_diversity_math_host) against mpmath at 100 digits on the fixed grids of tests/test_diversity_host.py -> profiles/diversity_math_accuracy.txt.
usage: python scripts/diversity_math_accuracy.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_diversity_host as T  # noqa: E402


def main():
    e_log, e_exp, pw_ratio = T.measure_math()
    text = (
        "rk_log2, rk_exp2 and pw of rappas_amd/csrc/rk_divmath.h against mpmath 1.3.0 at 100 digits (scripts/diversity_math_accuracy.py; the\n"
        "host build of the product library, x86-64, -ffp-contract=off; the device gives the same bits).  Errors in units in the last place\n"
        "of the exact value.\n\n"
        f"rk_log2   {len(T.log2_grid())} points: a / T for T in 3, 7, 1000, 2^30 + 1, 2^62 - 1 and up to 2 000 a spread over 1 .. T, and 2^0 .. 2^-63\n"
        f"          largest error {e_log:.2f} ulps        asserted by tests/test_diversity_host.py: {T.ASSERTED_LOG2_ULPS} ulps; exact on the powers of two\n"
        f"rk_exp2   {len(T.exp2_grid())} points evenly spaced over [-512, 8]\n"
        f"          largest error {e_exp:.2f} ulps        asserted: {T.ASSERTED_EXP2_ULPS} ulps\n"
        f"pw        those x with theta in {', '.join('%g' % t for t in T.PW_THETAS)}\n"
        f"          largest error {pw_ratio:.2f} of the bound 2 (A_exp + (A_log + 0.5) |theta log2 x| ln 2) + 1 ulps the test derives\n")
    with open(os.path.join(ROOT, "profiles", "diversity_math_accuracy.txt"), "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()

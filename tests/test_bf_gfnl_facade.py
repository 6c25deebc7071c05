"""The C++ facade (include/stereo_matching.hpp) with aggregations "BF" and "GFNL".

tests/cpp/bf_gfnl_facade_check.cpp sets the static selector from its first argument and the
facade's bf_ksize_v / bf_ksize_u or gfnl_var_thresh, runs costCalculate -> SolveAll ->
dispOptimize on one pair and writes DP[0].  Here: it compiles against the facade and the library.
Its maps are compared with the Python path's in tests/test_gpu_bf.py and tests/test_gpu_gfnl.py.
"""
import os

from test_cpp_facade import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bf_gfnl_facade_check.cpp")


def test_bf_gfnl_facade_check_compiles(tmp_path):
    _compile(SRC, str(tmp_path / "bf_gfnl_facade_check"))

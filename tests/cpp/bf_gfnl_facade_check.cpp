// bf_gfnl_facade_check.cpp — the C++ facade (include/stereo_matching.hpp) with aggregation "BF" or "GFNL":
//   bf_gfnl_facade_check BF   LEFT.ppm RIGHT.ppm MAXDISP KSIZE_V KSIZE_U OUT.i16
//   bf_gfnl_facade_check GFNL LEFT.ppm RIGHT.ppm MAXDISP VAR_THRESH 0    OUT.i16
// runs costCalculate -> SolveAll(smPsy, 1, 0.3) -> dispOptimize on one pair (main_.cpp:139-163)
// and writes DP[0] as raw little-endian int16, rows x cols.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "stereo_matching.hpp"

using namespace smamd;
using namespace std;

string StereoMatching::costcalculation = "censusGrad";
string StereoMatching::aggregation = "BF";
string StereoMatching::optimization = "sgm";
string StereoMatching::object = "";
const string StereoMatching::root = "";

int main(int argc, char** argv) {
    if (argc != 8) {
        cerr << "usage: bf_gfnl_facade_check BF|GFNL LEFT.ppm RIGHT.ppm MAXDISP A B OUT.i16" << endl;
        return 2;
    }
    StereoMatching::aggregation = argv[1];
    Mat I1_c = imread(argv[2], 1), I2_c = imread(argv[3], 1);
    Mat I1 = imread(argv[2], 0), I2 = imread(argv[3], 0);
    if (I1_c.empty() || I2_c.empty()) {
        cout << "can't read original img" << endl;
        return -1;
    }
    if (StereoMatching::aggregation == "BF") {
        StereoMatching::bf_ksize_v = atoi(argv[5]);
        StereoMatching::bf_ksize_u = atoi(argv[6]);
    } else {
        StereoMatching::gfnl_var_thresh = (float)atof(argv[5]);
    }
    try {
        StereoMatching::Parameters param(atoi(argv[4]), I1_c.rows, I1_c.cols);
        StereoMatching* smPsy[1] = {new StereoMatching(I1_c, I2_c, I1, I2, param)};
        smPsy[0]->costCalculate();
        SolveAll(smPsy, 1, 0.3f);
        smPsy[0]->dispOptimize();
        const Mat& dp = smPsy[0]->DP[0];
        FILE* f = fopen(argv[7], "wb");
        if (!f) return 3;
        for (int r = 0; r < dp.rows; r++) fwrite(dp.ptr<int16_t>(r), sizeof(int16_t), (size_t)dp.cols, f);
        fclose(f);
        delete smPsy[0];
    } catch (const std::exception& e) {
        cerr << e.what() << endl;
        return 4;
    }
    return 0;
}

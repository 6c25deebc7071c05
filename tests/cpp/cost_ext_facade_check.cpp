// cost_ext_facade_check.cpp — the C++ facade (include/stereo_matching.hpp) with one of the cost strings
// "SD", "BT", "grad", "TruncAD", "adGrad", "ADCensusGrad" (or any other, to see it refused):
//   cost_ext_facade_check COST LEFT.ppm RIGHT.ppm MAXDISP OUT.i16
// runs costCalculate -> SolveAll(smPsy, 1, 0.3) -> dispOptimize on one pair (main_.cpp:139-163)
// and writes DP[0] as raw little-endian int16, rows x cols.  Exit status 4 with the exception's text
// on stderr when the facade refuses the string.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "stereo_matching.hpp"

using namespace smamd;
using namespace std;

string StereoMatching::costcalculation = "adGrad";
string StereoMatching::aggregation = "CBCA";
string StereoMatching::optimization = "sgm";
string StereoMatching::object = "";
const string StereoMatching::root = "";

int main(int argc, char** argv) {
    if (argc != 6) {
        cerr << "usage: cost_ext_facade_check COST LEFT.ppm RIGHT.ppm MAXDISP OUT.i16" << endl;
        return 2;
    }
    StereoMatching::costcalculation = argv[1];
    Mat I1_c = imread(argv[2], 1), I2_c = imread(argv[3], 1);
    Mat I1 = imread(argv[2], 0), I2 = imread(argv[3], 0);
    if (I1_c.empty() || I2_c.empty()) {
        cout << "can't read original img" << endl;
        return -1;
    }
    try {
        StereoMatching::Parameters param(atoi(argv[4]), I1_c.rows, I1_c.cols);
        StereoMatching* smPsy[1] = {new StereoMatching(I1_c, I2_c, I1, I2, param)};
        smPsy[0]->costCalculate();
        SolveAll(smPsy, 1, 0.3f);
        smPsy[0]->dispOptimize();
        const Mat& dp = smPsy[0]->DP[0];
        FILE* f = fopen(argv[5], "wb");
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

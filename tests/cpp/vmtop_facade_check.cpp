// vmtop_facade_check.cpp — the C++ facade (include/stereo_matching.hpp) with param.Do_vmTop:
//   vmtop_facade_check LEFT.ppm RIGHT.ppm MAXDISP M LAMC TS METHOD HAS_CIR2 COLOR_LIMIT OUT.i16
// builds Parameters(maxDisp, rows, cols, 13, 1, M, lamc, ts) as main_.cpp:138 does, sets Do_vmTop (METHOD < 0
// leaves it off: the plain WTA), runs costCalculate -> SolveAll(smPsy, 1, 0.3) -> dispOptimize on one pair
// (main_.cpp:139-163) and writes DP[0] as raw little-endian int16, rows x cols.  It prints vmTop_thres's bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "stereo_matching.hpp"

using namespace smamd;
using namespace std;

string StereoMatching::costcalculation = "censusGrad";
string StereoMatching::aggregation = "CBCA";
string StereoMatching::optimization = "sgm";
string StereoMatching::object = "";
const string StereoMatching::root = "";

int main(int argc, char** argv) {
    if (argc != 11) {
        cerr << "usage: vmtop_facade_check LEFT.ppm RIGHT.ppm MAXDISP M LAMC TS METHOD HAS_CIR2 COLOR_LIMIT OUT.i16" << endl;
        return 2;
    }
    Mat I1_c = imread(argv[1], 1), I2_c = imread(argv[2], 1);
    Mat I1 = imread(argv[1], 0), I2 = imread(argv[2], 0);
    if (I1_c.empty() || I2_c.empty()) {
        cout << "can't read original img" << endl;
        return -1;
    }
    try {
        StereoMatching::Parameters param(atoi(argv[3]), I1_c.rows, I1_c.cols, 13, 1, atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
        const int method = atoi(argv[7]);
        param.Do_vmTop = method >= 0;
        param.vmTop_method = method >= 0 ? method : 0;
        param.vmTop_hasCir2 = atoi(argv[8]) != 0;
        param.vmTop_cir3_doColorLimit = atoi(argv[9]) != 0;
        uint32_t tb;
        memcpy(&tb, &param.vmTop_thres, sizeof(tb));
        printf("vmTop_thres_bits %08x\n", tb);
        StereoMatching* smPsy[1] = {new StereoMatching(I1_c, I2_c, I1, I2, param)};
        smPsy[0]->costCalculate();
        SolveAll(smPsy, 1, 0.3f);
        smPsy[0]->dispOptimize();
        const Mat& dp = smPsy[0]->DP[0];
        FILE* f = fopen(argv[10], "wb");
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

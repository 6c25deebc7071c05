// refine_ext_facade_check.cpp — the C++ facade (include/stereo_matching.hpp) with refine()'s extra stages:
//   refine_ext_facade_check LEFT.ppm RIGHT.ppm MAXDISP PKR BG SE SE_FLOAT OUT.i16 OUT_SE.f32 OUT_MASK.u8
// sets Do_refine and the three switches as a main_.cpp would before constructing the object, runs costCalculate ->
// SolveAll(smPsy, 1, 0.3) -> dispOptimize -> refine on one pair (main_.cpp:139-166) and writes DP[0] (int16), SE
// (float32, when SE is on) and PKR_Err_Mask (bytes, when PKR is on), rows x cols each.  It prints DISP_PKR and
// bgIplDepth.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "stereo_matching.hpp"

using namespace smamd;
using namespace std;

string StereoMatching::costcalculation = "censusGrad";
string StereoMatching::aggregation = "CBCA";
string StereoMatching::optimization = "sgm";
string StereoMatching::object = "";
const string StereoMatching::root = "";

template <typename T>
static bool dump(const char* path, const Mat& m) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    for (int r = 0; r < m.rows; r++) fwrite(m.ptr<T>(r), sizeof(T), (size_t)m.cols, f);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 11) {
        cerr << "usage: refine_ext_facade_check LEFT.ppm RIGHT.ppm MAXDISP PKR BG SE SE_FLOAT OUT.i16 OUT_SE.f32 OUT_MASK.u8" << endl;
        return 2;
    }
    Mat I1_c = imread(argv[1], 1), I2_c = imread(argv[2], 1);
    Mat I1 = imread(argv[1], 0), I2 = imread(argv[2], 0);
    if (I1_c.empty() || I2_c.empty()) {
        cout << "can't read original img" << endl;
        return -1;
    }
    try {
        StereoMatching::Do_refine = true;
        StereoMatching::Do_calPKR = atoi(argv[4]) != 0;
        StereoMatching::Do_bgIpol = atoi(argv[5]) != 0;
        StereoMatching::Do_subpixelEnhancement = atoi(argv[6]) != 0;
        StereoMatching::SE_FLOAT = atoi(argv[7]) != 0;
        StereoMatching::Parameters param(atoi(argv[3]), I1_c.rows, I1_c.cols);
        printf("DISP_PKR %d bgIplDepth %d\n", param.DISP_PKR, param.bgIplDepth);
        StereoMatching* smPsy[1] = {new StereoMatching(I1_c, I2_c, I1, I2, param)};
        smPsy[0]->costCalculate();
        SolveAll(smPsy, 1, 0.3f);
        smPsy[0]->dispOptimize();
        if (StereoMatching::Do_refine) smPsy[0]->refine();
        bool ok = dump<int16_t>(argv[8], smPsy[0]->DP[0]);
        if (StereoMatching::Do_subpixelEnhancement) ok = ok && dump<float>(argv[9], smPsy[0]->SE);
        if (StereoMatching::Do_calPKR) ok = ok && dump<uint8_t>(argv[10], smPsy[0]->PKR_Err_Mask);
        delete smPsy[0];
        if (!ok) return 3;
    } catch (const std::exception& e) {
        cerr << e.what() << endl;
        return 4;
    }
    return 0;
}

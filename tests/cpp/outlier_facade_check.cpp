// outlier_facade_check.cpp — the C++ facade (include/stereo_matching.hpp) with refine()'s outlier classification:
//   outlier_facade_check LEFT.ppm RIGHT.ppm MAXDISP CLASSIFY RV_COMBINE TYPE OUT.i16 OUT_MASK.u8
// sets Do_refine, LRC_CLASSIFY and RV_COMBINE_BG as a main_.cpp would before constructing the object and
// Parameters::interpolateType, runs costCalculate -> SolveAll(smPsy, 1, 0.3) -> dispOptimize -> refine on one pair
// (main_.cpp:139-166) and writes DP[0] (int16) and, with the classification on, LRC_Err_Mask (bytes), rows x cols
// each.  It prints the two parameters.
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
    if (argc != 9) {
        cerr << "usage: outlier_facade_check LEFT.ppm RIGHT.ppm MAXDISP CLASSIFY RV_COMBINE TYPE OUT.i16 OUT_MASK.u8" << endl;
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
        StereoMatching::LRC_CLASSIFY = atoi(argv[4]) != 0;
        StereoMatching::RV_COMBINE_BG = atoi(argv[5]) != 0;
        StereoMatching::Parameters param(atoi(argv[3]), I1_c.rows, I1_c.cols);
        param.interpolateType = atoi(argv[6]);
        printf("DISP_MIS %d interpolateType %d\n", param.DISP_MIS, param.interpolateType);
        StereoMatching* smPsy[1] = {new StereoMatching(I1_c, I2_c, I1, I2, param)};
        smPsy[0]->costCalculate();
        SolveAll(smPsy, 1, 0.3f);
        smPsy[0]->dispOptimize();
        smPsy[0]->refine();
        bool ok = dump<int16_t>(argv[7], smPsy[0]->DP[0]);
        if (StereoMatching::LRC_CLASSIFY) ok = ok && dump<uint8_t>(argv[8], smPsy[0]->LRC_Err_Mask);
        else ok = ok && smPsy[0]->LRC_Err_Mask.empty();
        delete smPsy[0];
        if (!ok) return 3;
    } catch (const std::exception& e) {
        cerr << e.what() << endl;
        return 4;
    }
    return 0;
}

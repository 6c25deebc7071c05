// eval_facade_check.cpp — the C++ facade (include/stereo_matching.hpp) with the per-stage error table:
//   eval_facade_check LEFT.ppm RIGHT.ppm MAXDISP GT.pgm NONOCC.pgm DISC.pgm
// sets Do_refine and Do_stageErrors as a main_.cpp would before constructing the object, reads DT as main_.cpp does
// (imread + convertTo CV_32F), passes nonocc and disc and an empty `all` mask, runs costCalculate -> SolveAll(smPsy, 1,
// 0.3) -> dispOptimize -> refine on one pair (main_.cpp:139-166) and prints stageErrorsText(): the err-txt lines.
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

int main(int argc, char** argv) {
    if (argc != 7) {
        cerr << "usage: eval_facade_check LEFT.ppm RIGHT.ppm MAXDISP GT.pgm NONOCC.pgm DISC.pgm" << endl;
        return 2;
    }
    Mat I1_c = imread(argv[1], 1), I2_c = imread(argv[2], 1);
    Mat I1 = imread(argv[1], 0), I2 = imread(argv[2], 0);
    Mat DT = imread(argv[4], 0), nonocc = imread(argv[5], 0), disc = imread(argv[6], 0), all;
    if (I1_c.empty() || I2_c.empty() || DT.empty() || nonocc.empty() || disc.empty()) {
        cout << "can't read original img" << endl;
        return -1;
    }
    try {
        DT.convertTo(DT, CV_32F, 1.0);
        StereoMatching::Do_refine = true;
        StereoMatching::Do_stageErrors = true;
        StereoMatching::Parameters param(atoi(argv[3]), I1_c.rows, I1_c.cols);
        StereoMatching* smPsy[1] = {new StereoMatching(I1_c, I2_c, I1, I2, DT, all, nonocc, disc, param)};
        smPsy[0]->costCalculate();
        SolveAll(smPsy, 1, 0.3f);
        smPsy[0]->dispOptimize();
        smPsy[0]->refine();
        cout << smPsy[0]->stageErrorsText();
        delete smPsy[0];
    } catch (const std::exception& e) {
        cerr << e.what() << endl;
        return 4;
    }
    return 0;
}

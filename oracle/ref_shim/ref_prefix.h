/* Force-included in front of the reference's C++ sources (oracle/ref_nl.mk): the standard headers
   and the namespace MSVC let them leave out, and the two "_s" stdio calls. */
#pragma once
#ifdef __cplusplus
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
using namespace std;
#define fopen_s(pf, path, mode) ((*(pf) = fopen((path), (mode))) == NULL)
#define fscanf_s(f, fmt, str, n) fscanf((f), (fmt), (str))
#endif

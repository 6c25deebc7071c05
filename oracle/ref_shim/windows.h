/* Stand-in for the three Win32 names the reference's qx_timer uses (oracle/ref_nl.mk).  The timer's
   readings are never used by the tests. */
#pragma once
#include <time.h>
struct LARGE_INTEGER { long long QuadPart; };
static inline int QueryPerformanceFrequency(LARGE_INTEGER *li) { li->QuadPart = 1000000000LL; return 1; }
static inline int QueryPerformanceCounter(LARGE_INTEGER *li) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    li->QuadPart = (long long)ts.tv_sec * 1000000000LL + ts.tv_nsec;
    return 1;
}

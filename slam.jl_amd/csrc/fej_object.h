// fej_object.h -- the layout of the first-estimates object, for the two libraries that read it: ekf_fej.hip (libslamhip_fej.so), which
// owns it, and ekf_wide.hip (libslamhip_wide.so), which reads h, N, lin and first and calls nothing of the other library.
#pragma once

#include "common.h"

struct slam_ekf_fej {
    slam_ekf* h;
    int N;             // the landmarks the object knows: h->N, unless the map changed outside (remap)
    int maxN;          // h->maxN at create: the capacity of the arrays below
    double* lin;       // [3]         the vehicle's linearisation pose
    double* first;     // [2 maxN]    every landmark's first estimate
    double* spare;     // [2 maxN]    remap writes here; the two are swapped
    int32_t* ids;      // [maxN]      reset / remap: the ids
};

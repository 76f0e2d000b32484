// mg_contact.h — the staged entry of the rigid contact list,
// written by the reporting builds of the step kernels (template flag CREP) in
// the frame's last substep and packed by k_contact_compact (mg_contact.hip).
#pragma once
#include "mg_internal.h"
#include "mg_math.h"

// Entry k of the staging record whose slot-0 dword is `st` (SoA stride
// `stride`, mg_internal.h). Dwords: body0, body1 (global rigid-body index, -1:
// the ground plane), kind (0: contact point, 1: friction anchor), a spare dword, world
// point, world normal (the direction a positive normal impulse pushes body0),
// separation at the substep's start (as the solver rows hold it: less the rest
// offset), the substep's final normal impulse, its final friction impulse on
// body0 (world vector), the friction coefficient of the row. The impulses are
// the values the kernel adds into the net contact force, stored, not recomputed.
__device__ __forceinline__ void crep_store(float* st, int stride, int k, int body0, int body1, int kind, V3 p, V3 n,
                                           float sep, float lambda, V3 fimp, float mu) {
    float* e = st + (size_t)k * MG_CREP_N * (size_t)stride;
    const size_t s = (size_t)stride;
    e[0 * s] = __int_as_float(body0);
    e[1 * s] = __int_as_float(body1);
    e[2 * s] = __int_as_float(kind);   // dword 3 is spare: reserved, not written
    e[4 * s] = p.x; e[5 * s] = p.y; e[6 * s] = p.z;
    e[7 * s] = n.x; e[8 * s] = n.y; e[9 * s] = n.z;
    e[10 * s] = sep;
    e[11 * s] = lambda;
    e[12 * s] = fimp.x; e[13 * s] = fimp.y; e[14 * s] = fimp.z;
    e[15 * s] = mu;
}

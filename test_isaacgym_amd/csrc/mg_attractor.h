// mg_attractor.h — rigid-body attractors (franka_attractor.py:132): an implicit
// 6-axis pose spring between a frame fixed on a body and a target pose
// (DESIGN.md §3.11). Shared by the articulated-body kernels (mg_env.hip) and
// the free-body kernels (mg_rigid.hip).
//
// A device record is MG_ATTR_N floats: axes (bits 0..5, as a float), stiffness
// K, damping D, the attractor frame in the body frame (p[3], q[4]), the target
// pose in global coordinates (p[3], q[4]). Axis k < 3 acts along the target
// frame's axis k at the attractor point, axis k >= 3 about its axis k - 3.
//
// Each selected axis is one row j (a 6-vector: moment about the reference
// point O, force) with  force_k = K err_k - (D + h K) vel_k+ ,  vel_k+ the
// row's velocity at the end of the substep, vel_k + h j . a. Summed over the
// rows that is a constant wrench  sum_k j_k b_k  (b_k = K err_k - (D + h K)
// vel_k) and an added inertia  h (D + h K) sum_k j_k j_k^T  about O.
#pragma once
#include "mg_spatial.h"

#define MG_ATTR_N 20

struct MgAttrFrame {
    V3 r;         // attractor point - O
    M3 Rt;        // target frame axes (columns, world)
    V3 e, phi;    // position error, rotation error (rotation vector), world
    float K, c1;  // stiffness, D + h K
    int axes;
};

// xb, qb: the body's pose; O: the reference point of the caller's 6-vectors
MG_HD MgAttrFrame attr_frame(const float* a, V3 xb, Q4 qb, V3 O, float h) {
    MgAttrFrame F;
    F.axes = (int)a[0];
    F.K = a[1];
    F.c1 = a[2] + h * a[1];
    const V3 xa = vadd(xb, qrot(qb, v3(a[3], a[4], a[5])));
    const Q4 qa = qmul(qb, q4(a[6], a[7], a[8], a[9]));
    const Q4 qt = qnormalize(q4(a[13], a[14], a[15], a[16]));
    F.r = vsub(xa, O);
    F.Rt = qmat(qt);
    F.e = vsub(v3(a[10], a[11], a[12]), xa);
    F.phi = q_log(qnormalize(qmul(qt, qconj(qa))));   // exp(phi) qa = qt, shortest arc
    return F;
}

// row k (bit k of F.axes): j[6] and b = K err - (D + h K) vel for a body
// turning at w whose point at O moves at vO
MG_HD void attr_row(const MgAttrFrame& F, int k, V3 w, V3 vO, float* j, float& b) {
    const int ax = k < 3 ? k : k - 3;
    const V3 t = ax == 0 ? F.Rt.c0 : (ax == 1 ? F.Rt.c1 : F.Rt.c2);
    if (k < 3) {
        const V3 s = vcross(F.r, t);
        j[0] = s.x; j[1] = s.y; j[2] = s.z; j[3] = t.x; j[4] = t.y; j[5] = t.z;
        b = F.K * vdot(t, F.e) - F.c1 * vdot(t, vadd(vO, vcross(w, F.r)));
    } else {
        j[0] = t.x; j[1] = t.y; j[2] = t.z; j[3] = 0.0f; j[4] = 0.0f; j[5] = 0.0f;
        b = F.K * vdot(t, F.phi) - F.c1 * vdot(t, w);
    }
}

// x = M^-1 b for a symmetric positive definite 6x6 M (row-major): left-looking
// Cholesky, forward and backward substitution (oracle: spd6_solve_)
MG_HD void spd6_solve(const float* M, const float* b, float* x) {
    float Lm[36], y[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float sj = M[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) sj = sj - Lm[j * 6 + k] * Lm[j * 6 + k];
        const float dj = sqrtf(sj);
        const float inv = 1.0f / dj;
        Lm[j * 6 + j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            float t = M[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - Lm[i * 6 + k] * Lm[j * 6 + k];
            Lm[i * 6 + j] = t * inv;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float t = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t = t - Lm[i * 6 + k] * y[k];
        y[i] = t / Lm[i * 6 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        float t = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t = t - Lm[k * 6 + i] * x[k];
        x[i] = t / Lm[i * 6 + i];
    }
}

// A free body's attractor step (mg_rigid.hip): v (COM velocity) and w after the
// gravity / applied-wrench update, solved implicitly against the body's own
// inertia:  (M + h (D + h K) sum j j^T) du = h sum j b,  about the COM xc.
MG_HD void attr_free_body(const float* a, V3 x, Q4 q, V3 xc, float invm, V3 invI, Q4 iq, float h, V3& v, V3& w) {
    const MgAttrFrame F = attr_frame(a, x, q, xc, h);
    // world inertia R diag(1 / invI) R^T (a locked axis: a very large inertia)
    const V3 Id = v3(invI.x > 0.0f ? 1.0f / invI.x : 1e20f, invI.y > 0.0f ? 1.0f / invI.y : 1e20f,
                     invI.z > 0.0f ? 1.0f / invI.z : 1e20f);
    const S3 I = sym_rdrt(qmat(qmul(q, iq)), Id);
    const float m = invm > 0.0f ? 1.0f / invm : 1e20f;
    float M[36], f[6], du[6];
#pragma unroll
    for (int i = 0; i < 36; ++i) M[i] = 0.0f;
    M[0] = I.xx; M[1] = I.xy; M[2] = I.xz;
    M[6] = I.xy; M[7] = I.yy; M[8] = I.yz;
    M[12] = I.xz; M[13] = I.yz; M[14] = I.zz;
    M[21] = m; M[28] = m; M[35] = m;
#pragma unroll
    for (int i = 0; i < 6; ++i) f[i] = 0.0f;
    const float c = h * F.c1;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if ((F.axes >> k) & 1) {
            float j[6], b;
            attr_row(F, k, w, v, j, b);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                f[i] = f[i] + j[i] * (h * b);
#pragma unroll
                for (int n = 0; n < 6; ++n) M[i * 6 + n] = M[i * 6 + n] + j[i] * (c * j[n]);
            }
        }
    }
    spd6_solve(M, f, du);
    w = vadd(w, v3(du[0], du[1], du[2]));
    v = vadd(v, v3(du[3], du[4], du[5]));
}

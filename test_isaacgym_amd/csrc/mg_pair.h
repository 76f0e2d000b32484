// mg_pair.h — mg_math.h's vector / quaternion helpers on pairs of values.
//
// A wave that is alone on its SIMD (the one-round launches of k_rigid_step1,
// DESIGN.md §3.2) is bound by instruction issue, and a packed f32 instruction
// (v_pk_mul_f32, v_pk_add_f32, v_pk_fma_f32) does two lanes' worth of work in
// one issue slot. A V3x2 holds two vectors component by component, each
// component an f2 register pair; every helper here restates its scalar
// original with the same terms in the same order and grouping, so each half of
// every packed operation is the correctly rounded IEEE operation of the scalar
// form and the results are bit for bit the same (tests/test_pair_math.py).
// Products and sums stay separate operations (-ffp-contract=off); a fused
// multiply-add appears only where the scalar code calls fmaf. Selects and
// compares stay per component: there is no packed v_cndmask.
#pragma once
#include "mg_math.h"

typedef float f2 __attribute__((ext_vector_type(2)));
MG_HD f2 pk2(float a, float b) { return f2{a, b}; }
MG_HD f2 bc2(float a) { return f2{a, a}; }
MG_HD f2 pfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

#ifdef __HIP__
// (1.0f / d.x, 1.0f / d.y): the compiler's own expansion of an IEEE f32
// division (v_div_scale of denominator and numerator, v_rcp, six refinement
// steps, v_div_fmas, v_div_fixup; denormals stay enabled, no mode switch), with
// the six steps of the two quotients issued as packed operations. Scaling,
// reciprocal, the final fmas (each half with its own scale flag) and the fixup
// stay per half, so each half is the scalar sequence's value for every float
// (tests/test_rcp_pairs_gpu.py). Device code only (a plain C++ host build of
// this header, tests/pair_math_check.cpp, does not see it).
__device__ __forceinline__ f2 rcp2_ieee(f2 d) {
    bool fx, fy, unused;
    const float dsx = __builtin_amdgcn_div_scalef(1.0f, d.x, false, &unused);
    const float dsy = __builtin_amdgcn_div_scalef(1.0f, d.y, false, &unused);
    const f2 ns = pk2(__builtin_amdgcn_div_scalef(1.0f, d.x, true, &fx),
                      __builtin_amdgcn_div_scalef(1.0f, d.y, true, &fy));
    const f2 nd = -pk2(dsx, dsy);
    const f2 r0 = pk2(__builtin_amdgcn_rcpf(dsx), __builtin_amdgcn_rcpf(dsy));
    const f2 e0 = pfma(nd, r0, bc2(1.0f));
    const f2 r1 = pfma(e0, r0, r0);
    const f2 q0 = ns * r1;
    const f2 e1 = pfma(nd, q0, ns);
    const f2 q1 = pfma(e1, r1, q0);
    const f2 e2 = pfma(nd, q1, ns);
    return pk2(__builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(e2.x, r1.x, q1.x, fx), d.x, 1.0f),
               __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(e2.y, r1.y, q1.y, fy), d.y, 1.0f));
}
#endif

struct V3x2 { f2 x, y, z; };            // (a, b): .x = (a.x, b.x) ...
struct Q4x2 { f2 x, y, z, w; };

MG_HD V3x2 v3x2(V3 a, V3 b) { V3x2 r; r.x = pk2(a.x, b.x); r.y = pk2(a.y, b.y); r.z = pk2(a.z, b.z); return r; }
MG_HD V3x2 v3bc(V3 a) { return v3x2(a, a); }
MG_HD V3x2 v3p(f2 x, f2 y, f2 z) { V3x2 r; r.x = x; r.y = y; r.z = z; return r; }
MG_HD V3 v3lo(V3x2 p) { return v3(p.x.x, p.y.x, p.z.x); }
MG_HD V3 v3hi(V3x2 p) { return v3(p.x.y, p.y.y, p.z.y); }
MG_HD Q4x2 q4x2(Q4 a, Q4 b) {
    Q4x2 r; r.x = pk2(a.x, b.x); r.y = pk2(a.y, b.y); r.z = pk2(a.z, b.z); r.w = pk2(a.w, b.w); return r;
}
MG_HD Q4 q4lo(Q4x2 p) { return q4(p.x.x, p.y.x, p.z.x, p.w.x); }
MG_HD Q4 q4hi(Q4x2 p) { return q4(p.x.y, p.y.y, p.z.y, p.w.y); }

MG_HD V3x2 vadd2(V3x2 a, V3x2 b) { return v3p(a.x + b.x, a.y + b.y, a.z + b.z); }
MG_HD V3x2 vsub2(V3x2 a, V3x2 b) { return v3p(a.x - b.x, a.y - b.y, a.z - b.z); }
MG_HD V3x2 vscale2(V3x2 a, f2 s) { return v3p(a.x * s, a.y * s, a.z * s); }
MG_HD f2 vdot2(V3x2 a, V3x2 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
MG_HD V3x2 vcross2(V3x2 a, V3x2 b) {
    return v3p(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// a + b * s
MG_HD V3x2 vmad2(V3x2 a, V3x2 b, f2 s) { return v3p(a.x + b.x * s, a.y + b.y * s, a.z + b.z * s); }

// qrot of a pair of vectors by a pair of quaternions: (qrot(qa, va), qrot(qb, vb))
MG_HD V3x2 qrotq2(Q4x2 q, V3x2 v) {
    const f2 tx = 2.0f * (q.y * v.z - q.z * v.y);
    const f2 ty = 2.0f * (q.z * v.x - q.x * v.z);
    const f2 tz = 2.0f * (q.x * v.y - q.y * v.x);
    return v3p(v.x + q.w * tx + (q.y * tz - q.z * ty),
               v.y + q.w * ty + (q.z * tx - q.x * tz),
               v.z + q.w * tz + (q.x * ty - q.y * tx));
}
// qrot of two vectors by one quaternion
MG_HD V3x2 qrot2(Q4 q, V3x2 v) { return qrotq2(q4x2(q, q), v); }
MG_HD V3x2 qrot_inv2(Q4 q, V3x2 v) { return qrot2(qconj(q), v); }

// ---- the +Z ground basis (mg_rigid.hip BasisZ: n = z, t1 = y, t2 = -x) ------
// Iw (r x d) and (r x d) . Iw (r x d) of two lever arms, the zero component of
// r x d dropped as in BasisZ (symmul's term order).
MG_HD V3 z_iwn(const S3& I, V3 r) {
    const float a = r.y, b = -r.x;   // r x n = (a, b, 0)
    return v3(I.xx * a + I.xy * b, I.xy * a + I.yy * b, I.xz * a + I.yz * b);
}
MG_HD V3 z_iw1(const S3& I, V3 r) {
    const float a = -r.z, c = r.x;   // r x t1 = (a, 0, c)
    return v3(I.xx * a + I.xz * c, I.xy * a + I.yz * c, I.xz * a + I.zz * c);
}
MG_HD V3 z_iw2(const S3& I, V3 r) {
    const float b = -r.z, c = r.y;   // r x t2 = (0, b, c)
    return v3(I.xy * b + I.xz * c, I.yy * b + I.yz * c, I.yz * b + I.zz * c);
}
MG_HD float z_kn(V3 r, V3 In) { return r.y * In.x + -r.x * In.y; }
MG_HD float z_k1(V3 r, V3 I1) { return -r.z * I1.x + r.x * I1.z; }
MG_HD float z_k2(V3 r, V3 I2) { return -r.z * I2.y + r.y * I2.z; }
// the same on two lever arms
MG_HD V3x2 z_iwn2(const S3& I, V3x2 r) {
    const f2 a = r.y, b = -r.x;   // r x n = (a, b, 0)
    return v3p(I.xx * a + I.xy * b, I.xy * a + I.yy * b, I.xz * a + I.yz * b);
}
MG_HD V3x2 z_iw12(const S3& I, V3x2 r) {
    const f2 a = -r.z, c = r.x;   // r x t1 = (a, 0, c)
    return v3p(I.xx * a + I.xz * c, I.xy * a + I.yz * c, I.xz * a + I.zz * c);
}
MG_HD V3x2 z_iw22(const S3& I, V3x2 r) {
    const f2 b = -r.z, c = r.y;   // r x t2 = (0, b, c)
    return v3p(I.xy * b + I.xz * c, I.yy * b + I.yz * c, I.yz * b + I.zz * c);
}
MG_HD f2 z_kn2(V3x2 r, V3x2 In) { return r.y * In.x + -r.x * In.y; }
MG_HD f2 z_k12(V3x2 r, V3x2 I1) { return -r.z * I1.x + r.x * I1.z; }
MG_HD f2 z_k22(V3x2 r, V3x2 I2) { return -r.z * I2.y + r.y * I2.z; }

// The x and y of Iw (r x d) as one pair from pairs of Iw's entries: the solver
// (mg_rigid.hip tgs_zp) consumes (In.x, In.y), (I1.x, I1.y), (I2.x, I2.y) as
// packed operands, so they are formed as pairs where they are produced; the z
// component stays the scalar z_iwn / z_iw1 / z_iw2 expression.
struct S3P { f2 xx_xy, xy_yy, xz_yz; };
MG_HD S3P s3p(const S3& I) { S3P p; p.xx_xy = pk2(I.xx, I.xy); p.xy_yy = pk2(I.xy, I.yy); p.xz_yz = pk2(I.xz, I.yz); return p; }
// sym_rdrt with its entries formed as the pairs above: (xx, xy) and (xz, yz)
// each by one packed chain over the columns' (x, y), yy and zz scalar; every
// entry the same sum of the same products as sym_rdrt's.
MG_HD S3 sym_rdrt_p(M3 Rp, V3 d, S3P& Ip) {
    const f2 c0 = pk2(Rp.c0.x, Rp.c0.y), c1 = pk2(Rp.c1.x, Rp.c1.y), c2 = pk2(Rp.c2.x, Rp.c2.y);
    const f2 u0 = c0 * bc2(d.x), u1 = c1 * bc2(d.y), u2 = c2 * bc2(d.z);   // (u.x, u.y) of vscale(c, d)
    const float u0z = Rp.c0.z * d.x, u1z = Rp.c1.z * d.y, u2z = Rp.c2.z * d.z;
    const f2 xx_xy = bc2(u0.x) * c0 + bc2(u1.x) * c1 + bc2(u2.x) * c2;
    const f2 xz_yz = u0 * bc2(Rp.c0.z) + u1 * bc2(Rp.c1.z) + u2 * bc2(Rp.c2.z);
    S3 s;
    s.xx = xx_xy.x;
    s.xy = xx_xy.y;
    s.xz = xz_yz.x;
    s.yz = xz_yz.y;
    s.yy = u0.y * Rp.c0.y + u1.y * Rp.c1.y + u2.y * Rp.c2.y;
    s.zz = u0z * Rp.c0.z + u1z * Rp.c1.z + u2z * Rp.c2.z;
    Ip.xx_xy = xx_xy;
    Ip.xy_yy = pk2(s.xy, s.yy);
    Ip.xz_yz = xz_yz;
    return s;
}
MG_HD f2 z_iwn_xy(const S3P& I, V3 r) { return I.xx_xy * bc2(r.y) + I.xy_yy * bc2(-r.x); }
MG_HD f2 z_iw1_xy(const S3P& I, V3 r) { return I.xx_xy * bc2(-r.z) + I.xz_yz * bc2(r.x); }
MG_HD f2 z_iw2_xy(const S3P& I, V3 r) { return I.xy_yy * bc2(-r.z) + I.xz_yz * bc2(r.y); }
MG_HD float z_iwn_z(const S3& I, V3 r) { return I.xz * r.y + I.yz * -r.x; }
MG_HD float z_iw1_z(const S3& I, V3 r) { return I.xz * -r.z + I.zz * r.x; }
MG_HD float z_iw2_z(const S3& I, V3 r) { return I.yz * -r.z + I.zz * r.y; }
// BasisZ::vn of two lever arms: v.z + w.x r.y - w.y r.x by two fused multiply-adds
MG_HD f2 z_vn2(V3 v, V3 w, f2 ry, f2 nrx) { return pfma(bc2(w.y), nrx, pfma(bc2(w.x), ry, bc2(v.z))); }

// pair_math_check.cpp — host check of test_isaacgym_amd/csrc/mg_pair.h: every
// pair helper against its scalar original (mg_math.h, and the +Z row helpers
// of mg_pair.h itself) on the same inputs, both halves compared bit for bit
// (two NaNs compare equal whatever their payloads). Built and run by
// tests/test_pair_math.py; the exit status is the verdict.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mg_pair.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd32() {   // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
float rndf(float scale) { return ((float)rnd32() / 4294967296.0f * 2.0f - 1.0f) * scale; }

const float kInf = std::numeric_limits<float>::infinity();
const float kNan = std::numeric_limits<float>::quiet_NaN();
const float kSpecial[] = {0.0f, -0.0f, 1e-45f, -1e-45f, 1.1e-38f, -5e-39f, kInf, -kInf, kNan, 1.0f, -2.5f, 3.0e38f};
const int kNSpecial = (int)(sizeof(kSpecial) / sizeof(kSpecial[0]));

long g_fail = 0, g_checks = 0;
bool same(float a, float b) {
    if (a != a && b != b) return true;
    uint32_t ua, ub;
    std::memcpy(&ua, &a, 4);
    std::memcpy(&ub, &b, 4);
    return ua == ub;
}
void check1(const char* what, float got, float want) {
    ++g_checks;
    if (!same(got, want)) {
        if (g_fail < 20) std::printf("MISMATCH %s: pair %a, scalar %a\n", what, got, want);
        ++g_fail;
    }
}
void check(const char* what, f2 got, float lo, float hi) {
    check1(what, got.x, lo);
    check1(what, got.y, hi);
}
void check3(const char* what, V3x2 got, V3 lo, V3 hi) {
    check(what, got.x, lo.x, hi.x);
    check(what, got.y, lo.y, hi.y);
    check(what, got.z, lo.z, hi.z);
}

struct In {
    V3 a, b, c, d;   // two pairs of vectors
    Q4 q, p;
    S3 I;
    float s, t;
};

void run(const In& k) {
    const V3x2 A = v3x2(k.a, k.b), C = v3x2(k.c, k.d);
    const f2 S = pk2(k.s, k.t);
    // packing and unpacking
    check3("v3x2/v3lo/v3hi", A, v3lo(A), v3hi(A));
    check3("v3x2", A, k.a, k.b);
    check3("v3bc", v3bc(k.a), k.a, k.a);
    const Q4x2 QP = q4x2(k.q, k.p);
    check("q4x2.x", QP.x, q4lo(QP).x, q4hi(QP).x);
    check("q4x2.w", QP.w, k.q.w, k.p.w);
    check("bc2", bc2(k.s), k.s, k.s);
    check("pfma", pfma(A.x, C.y, S), fmaf(k.a.x, k.c.y, k.s), fmaf(k.b.x, k.d.y, k.t));
    // vectors
    check3("vadd2", vadd2(A, C), vadd(k.a, k.c), vadd(k.b, k.d));
    check3("vsub2", vsub2(A, C), vsub(k.a, k.c), vsub(k.b, k.d));
    check3("vscale2", vscale2(A, S), vscale(k.a, k.s), vscale(k.b, k.t));
    check("vdot2", vdot2(A, C), vdot(k.a, k.c), vdot(k.b, k.d));
    check("vdot2 self", vdot2(A, A), vdot(k.a, k.a), vdot(k.b, k.b));
    check3("vcross2", vcross2(A, C), vcross(k.a, k.c), vcross(k.b, k.d));
    check3("vmad2", vmad2(A, C, S), vmad(k.a, k.c, k.s), vmad(k.b, k.d, k.t));
    // rotations: two vectors by one quaternion, and by a pair of quaternions
    check3("qrot2", qrot2(k.q, A), qrot(k.q, k.a), qrot(k.q, k.b));
    check3("qrot_inv2", qrot_inv2(k.q, A), qrot_inv(k.q, k.a), qrot_inv(k.q, k.b));
    check3("qrotq2", qrotq2(QP, A), qrot(k.q, k.a), qrot(k.p, k.b));
    check3("qrotq2 (q, conj q)", qrotq2(q4x2(k.q, qconj(k.q)), A), qrot(k.q, k.a), qrot_inv(k.q, k.b));
    // +Z rows
    const V3x2 In = z_iwn2(k.I, A), I1 = z_iw12(k.I, A), I2 = z_iw22(k.I, A);
    check3("z_iwn2", In, z_iwn(k.I, k.a), z_iwn(k.I, k.b));
    check3("z_iw12", I1, z_iw1(k.I, k.a), z_iw1(k.I, k.b));
    check3("z_iw22", I2, z_iw2(k.I, k.a), z_iw2(k.I, k.b));
    check("z_kn2", z_kn2(A, C), z_kn(k.a, k.c), z_kn(k.b, k.d));
    check("z_k12", z_k12(A, C), z_k1(k.a, k.c), z_k1(k.b, k.d));
    check("z_k22", z_k22(A, C), z_k2(k.a, k.c), z_k2(k.b, k.d));
    const S3P IP = s3p(k.I);
    check("z_iwn_xy", z_iwn_xy(IP, k.a), z_iwn(k.I, k.a).x, z_iwn(k.I, k.a).y);
    check("z_iw1_xy", z_iw1_xy(IP, k.a), z_iw1(k.I, k.a).x, z_iw1(k.I, k.a).y);
    check("z_iw2_xy", z_iw2_xy(IP, k.a), z_iw2(k.I, k.a).x, z_iw2(k.I, k.a).y);
    check1("z_iwn_z", z_iwn_z(k.I, k.b), z_iwn(k.I, k.b).z);
    check1("z_iw1_z", z_iw1_z(k.I, k.b), z_iw1(k.I, k.b).z);
    check1("z_iw2_z", z_iw2_z(k.I, k.b), z_iw2(k.I, k.b).z);
    // BasisZ::vn (mg_rigid.hip): fmaf(w.y, -r.x, fmaf(w.x, r.y, v.z))
    check("z_vn2", z_vn2(k.c, k.d, A.y, -A.x), fmaf(k.d.y, -k.a.x, fmaf(k.d.x, k.a.y, k.c.z)),
          fmaf(k.d.y, -k.b.x, fmaf(k.d.x, k.b.y, k.c.z)));
    {
        const M3 Rm = qmat(k.p);
        S3P SP;
        const S3 got = sym_rdrt_p(Rm, k.c, SP), want = sym_rdrt(Rm, k.c);
        check("sym_rdrt_p xx,yy", pk2(got.xx, got.yy), want.xx, want.yy);
        check("sym_rdrt_p zz,xy", pk2(got.zz, got.xy), want.zz, want.xy);
        check("sym_rdrt_p xz,yz", pk2(got.xz, got.yz), want.xz, want.yz);
        check("sym_rdrt_p (xx, xy)", SP.xx_xy, want.xx, want.xy);
        check("sym_rdrt_p (xy, yy)", SP.xy_yy, want.xy, want.yy);
        check("sym_rdrt_p (xz, yz)", SP.xz_yz, want.xz, want.yz);
    }
    check("z_kn2 (In)", z_kn2(A, In), z_kn(k.a, z_iwn(k.I, k.a)), z_kn(k.b, z_iwn(k.I, k.b)));
}

V3 rv(float s) { return v3(rndf(s), rndf(s), rndf(s)); }
Q4 rq(bool unit) {
    Q4 q = q4(rndf(1.0f), rndf(1.0f), rndf(1.0f), rndf(1.0f));
    return unit ? qnormalize(q) : q;
}
In random_in(int i) {
    const float scales[] = {1.0f, 1e-3f, 100.0f, 1e-20f, 1e18f};
    const float s = scales[i % 5];
    In k;
    k.a = rv(s); k.b = rv(s); k.c = rv(s); k.d = rv(s);
    k.q = rq(i % 3 != 0); k.p = rq(i % 3 != 1);
    k.I = sym_rdrt(qmat(k.q), v3(1.0f + rndf(0.9f), 1.0f + rndf(0.9f), 1.0f + rndf(0.9f)));
    k.s = rndf(s); k.t = rndf(2.0f);
    return k;
}

}  // namespace

int main() {
    const int kRandom = 100000;
    for (int i = 0; i < kRandom; ++i) run(random_in(i));
    // signed zeros, denormals, infinities and NaN in every component position,
    // in the low half, the high half and both
    float* slots[32];
    for (int i = 0; i < 4000; ++i) {
        In k = random_in(i);
        int n = 0;
        for (V3* v : {&k.a, &k.b, &k.c, &k.d}) { slots[n++] = &v->x; slots[n++] = &v->y; slots[n++] = &v->z; }
        for (Q4* q : {&k.q, &k.p}) { slots[n++] = &q->x; slots[n++] = &q->y; slots[n++] = &q->z; slots[n++] = &q->w; }
        for (float* f : {&k.I.xx, &k.I.yy, &k.I.zz, &k.I.xy, &k.I.xz, &k.I.yz, &k.s, &k.t}) slots[n++] = f;
        const int hits = 1 + (int)(rnd32() % 4);
        for (int h = 0; h < hits; ++h) *slots[rnd32() % n] = kSpecial[rnd32() % kNSpecial];
        run(k);
    }
    for (int a = 0; a < kNSpecial; ++a)
        for (int b = 0; b < kNSpecial; ++b) {   // every special against every special, all components
            In k = random_in(a + b);
            k.a = v3(kSpecial[a], kSpecial[b], kSpecial[a]);
            k.b = v3(kSpecial[b], kSpecial[a], kSpecial[b]);
            k.c = v3(kSpecial[b], kSpecial[b], kSpecial[a]);
            k.d = v3(kSpecial[a], kSpecial[a], kSpecial[b]);
            k.s = kSpecial[a];
            k.t = kSpecial[b];
            run(k);
            k.q = q4(kSpecial[a], kSpecial[b], 0.5f, kSpecial[b]);
            k.I.xy = kSpecial[a];
            k.I.zz = kSpecial[b];
            run(k);
        }
    std::printf("%ld comparisons, %ld mismatches\n", g_checks, g_fail);
    return g_fail == 0 ? 0 : 1;
}

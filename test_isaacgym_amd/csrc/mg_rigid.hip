// mg_rigid.hip — fused free-body step: gym.simulate() for every single-body
// dynamic actor (the servo scene's UAV and ground vehicle).
//
// One lane = one free body for the whole frame: `substeps` TGS substeps, each
//   1. unconstrained velocity: gravity, external force, PhysX-style damping
//      v *= 1 - min(damping*h, 1), max-velocity clamp;
//   2. contact generation against the ground plane (box corners, sphere and
//      capsule end caps within contact_offset), at most MG_MAX_CONTACTS slots;
//   3. TGS: npos position iterations of length h/npos, each a Gauss-Seidel pass
//      over the normal rows (speculative / depenetration target) and the
//      friction rows (Coulomb pyramid, PhysX-style), followed by integrating the
//      body's motion delta; then nvel velocity iterations with the bias removed
//      (single-shape bodies: the patch's anchor rows then the normal rows, the
//      first and the velocity sweeps opening with the normal rows too);
//   4. pose update: com += sum of iteration deltas, q = exp(dtheta) q.
// Envs are independent and (test10_servo_vecenv.py:317,323: group=i, filter=-1)
// the two actors of an env do not collide, so lanes never communicate: no
// atomics, no grid sync. State is SoA [field][body] so every load and store of
// a wavefront is one coalesced 256-B transaction per field.
//
// At the headline size (4096 envs = 128 waves on 1024 SIMDs) the frame time is
// one wave's instruction stream plus its memory round trips
// (tools/kbench_rigid_phases.py: 7.2 us with no contacts, +5.9 us for 10 of the
// 14 solver iterations), so the single-shape kernel k_rigid_step1 is built for
// latency:
//   - template constants (damping, speed limits, gravity flag and the shape
//     record) are one compact MG_TREC_N-float record per template body, staged
//     in LDS by the workgroup while the lanes' state loads are in flight: one
//     HBM round trip instead of body -> template -> shape -> ...;
//   - the 4 static contact slots are processed without branches: an inactive
//     slot has zero effective masses and a zero lever arm, so its rows apply
//     exactly zero impulse; only a wave with no contact at all skips the
//     solver loops (wave-uniform);
//   - the row updates fuse the impulse accumulation (fmaf) and clamp the
//     friction impulse with one v_med3_f32;
//   - the +Z ground (make_step's basis n = z, t1 = y, t2 = -x) is a template
//     specialisation with the cross / dot products written out;
//   - a wave of a one-round launch is alone on its SIMD and bound by
//     instruction issue, where a packed f32 instruction does two lanes' worth
//     of work in one slot: beside the +Z solver (tgs_zp), the patch update,
//     the row constants with the anchor rows, and Iw are formed on f2 pairs
//     (mg_pair.h; MG_RIGID1_PACK_GEOM, builds without attractor or report),
//     and qmat(q) is formed once per substep for Iw and the candidates. Each
//     half is the scalar form's operation, so results are unchanged; the wide
//     forms and k_rigid_step keep the scalar code.
// Multi-shape bodies run k_rigid_step (8 shift-register slots, a second launch).
// The C restatement is oracle/migym_oracle.c:rigid_body_step (same slot order,
// same specialisation, same evaluation order).
#include "mg_internal.h"
#include "mg_math.h"
#include "mg_pair.h"
#include "mg_attractor.h"
#include "mg_contact.h"

#ifdef MG_RIGID1_STAMPS
// diagnostic build only (tools/kbench_rigid_stamps.py): s_memtime stamps of
// each k_rigid_step1 wave at its phase boundaries, lane 0 -> g_rigid_stamp[wave]
#define MG_RIGID1_NSTAMP 18
__device__ unsigned long long g_rigid_stamp[4096][MG_RIGID1_NSTAMP];
extern "C" int mg_debug_rigid_stamps(unsigned long long* out, int nwaves) {
    if (nwaves > 4096) nwaves = 4096;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rigid_stamp), (size_t)nwaves * MG_RIGID1_NSTAMP * 8) == hipSuccess
               ? 0
               : -1;
}
__device__ __forceinline__ unsigned long long rigid_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define RSTAMP(k) do { const unsigned long long t_ = rigid_stamp(); \
    if (threadIdx.x == 0 && blockIdx.x < 4096) g_rigid_stamp[blockIdx.x][k] = t_; } while (0)
#define RUSE(v) asm volatile("" ::"v"(v))
#else
#define RSTAMP(k) do { } while (0)
#define RUSE(v) do { } while (0)
#endif

namespace {

// ---- ground basis: general (n, t1, t2) or the +Z specialisation -----------
// Row kernels of the Gauss-Seidel chain use explicit fused multiply-adds
// (fmaf, correctly rounded like the oracle's C fmaf); everything else is built
// with -ffp-contract=off. vn / v1 / v2: velocity of the contact point along the
// row direction d (d . v + w . (r x d)); ps: separation s0 + n . dx + dth . (r x n).
__device__ __forceinline__ float fdot3(V3 a, V3 b, float acc) {
    return fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc)));
}
__device__ __forceinline__ V3 fmad3(V3 v, V3 d, float s) {
    return v3(fmaf(d.x, s, v.x), fmaf(d.y, s, v.y), fmaf(d.z, s, v.z));
}
struct BasisGen {
    static constexpr bool kPacked = false;
    V3 n, t1, t2;
    __device__ __forceinline__ float dn(V3 v) const { return vdot(n, v); }
    __device__ __forceinline__ float d1(V3 v) const { return vdot(t1, v); }
    __device__ __forceinline__ float d2(V3 v) const { return vdot(t2, v); }
    __device__ __forceinline__ V3 cn(V3 r) const { return vcross(r, n); }
    __device__ __forceinline__ V3 c1(V3 r) const { return vcross(r, t1); }
    __device__ __forceinline__ V3 c2(V3 r) const { return vcross(r, t2); }
    __device__ __forceinline__ V3 addn(V3 v, float s) const { return vmad(v, n, s); }
    __device__ __forceinline__ V3 add1(V3 v, float s) const { return vmad(v, t1, s); }
    __device__ __forceinline__ V3 add2(V3 v, float s) const { return vmad(v, t2, s); }
    __device__ __forceinline__ float vn(V3 v, V3 w, V3 r) const { return fdot3(w, cn(r), vdot(n, v)); }
    __device__ __forceinline__ float v1(V3 v, V3 w, V3 r) const { return fdot3(w, c1(r), vdot(t1, v)); }
    __device__ __forceinline__ float v2(V3 v, V3 w, V3 r) const { return fdot3(w, c2(r), vdot(t2, v)); }
    __device__ __forceinline__ float ps(float s0, V3 dx, V3 dth, V3 r) const {
        return fdot3(dth, cn(r), s0 + vdot(n, dx));
    }
    __device__ __forceinline__ V3 fn(V3 v, float dl, float invm) const { return fmad3(v, n, dl * invm); }
    __device__ __forceinline__ V3 f1(V3 v, float dl, float invm) const { return fmad3(v, t1, dl * invm); }
    __device__ __forceinline__ V3 f2(V3 v, float dl, float invm) const { return fmad3(v, t2, dl * invm); }
    // Iw (r x d) and (r x d) . Iw (r x d) of the three row directions
    __device__ __forceinline__ V3 iwn(const S3& I, V3 r) const { return symmul(I, cn(r)); }
    __device__ __forceinline__ V3 iw1(const S3& I, V3 r) const { return symmul(I, c1(r)); }
    __device__ __forceinline__ V3 iw2(const S3& I, V3 r) const { return symmul(I, c2(r)); }
    __device__ __forceinline__ float kn(V3 r, V3 In) const { return vdot(cn(r), In); }
    __device__ __forceinline__ float k1(V3 r, V3 I1) const { return vdot(c1(r), I1); }
    __device__ __forceinline__ float k2(V3 r, V3 I2) const { return vdot(c2(r), I2); }
};
// n = (0,0,1), t1 = (0,1,0), t2 = (-1,0,0)
struct BasisZ {
    static constexpr bool kPacked = true;   // tgs_z applies (rigid_body1<..., PACK>)
    __device__ __forceinline__ float dn(V3 v) const { return v.z; }
    __device__ __forceinline__ float d1(V3 v) const { return v.y; }
    __device__ __forceinline__ float d2(V3 v) const { return -v.x; }
    __device__ __forceinline__ V3 cn(V3 r) const { return v3(r.y, -r.x, 0.0f); }
    __device__ __forceinline__ V3 c1(V3 r) const { return v3(-r.z, 0.0f, r.x); }
    __device__ __forceinline__ V3 c2(V3 r) const { return v3(0.0f, -r.z, r.y); }
    __device__ __forceinline__ V3 addn(V3 v, float s) const { return v3(v.x, v.y, v.z + s); }
    __device__ __forceinline__ V3 add1(V3 v, float s) const { return v3(v.x, v.y + s, v.z); }
    __device__ __forceinline__ V3 add2(V3 v, float s) const { return v3(v.x - s, v.y, v.z); }
    // r x n = (r.y, -r.x, 0), r x t1 = (-r.z, 0, r.x), r x t2 = (0, -r.z, r.y): zero terms dropped
    __device__ __forceinline__ float vn(V3 v, V3 w, V3 r) const { return fmaf(w.y, -r.x, fmaf(w.x, r.y, v.z)); }
    __device__ __forceinline__ float v1(V3 v, V3 w, V3 r) const { return fmaf(w.z, r.x, fmaf(w.x, -r.z, v.y)); }
    __device__ __forceinline__ float v2(V3 v, V3 w, V3 r) const { return fmaf(w.z, r.y, fmaf(w.y, -r.z, -v.x)); }
    __device__ __forceinline__ float ps(float s0, V3 dx, V3 dth, V3 r) const {
        return fmaf(dth.y, -r.x, fmaf(dth.x, r.y, s0 + dx.z));
    }
    __device__ __forceinline__ V3 fn(V3 v, float dl, float invm) const { return v3(v.x, v.y, fmaf(dl, invm, v.z)); }
    __device__ __forceinline__ V3 f1(V3 v, float dl, float invm) const { return v3(v.x, fmaf(dl, invm, v.y), v.z); }
    __device__ __forceinline__ V3 f2(V3 v, float dl, float invm) const { return v3(fmaf(-dl, invm, v.x), v.y, v.z); }
    // symmul / vdot with the zero component of r x d dropped (mg_pair.h)
    __device__ __forceinline__ V3 iwn(const S3& I, V3 r) const { return z_iwn(I, r); }
    __device__ __forceinline__ V3 iw1(const S3& I, V3 r) const { return z_iw1(I, r); }
    __device__ __forceinline__ V3 iw2(const S3& I, V3 r) const { return z_iw2(I, r); }
    __device__ __forceinline__ float kn(V3 r, V3 In) const { return z_kn(r, In); }
    __device__ __forceinline__ float k1(V3 r, V3 I1) const { return z_k1(r, I1); }
    __device__ __forceinline__ float k2(V3 r, V3 I2) const { return z_k2(r, I2); }
};

// clamp x to [-lim, lim] (lim >= 0): the median of three, one instruction
__device__ __forceinline__ float clamp_sym(float x, float lim) { return __builtin_amdgcn_fmed3f(x, -lim, lim); }

struct Slot {
    V3 r;        // contact point - centre of mass (world)
    float s0;    // separation minus rest offset at substep start
    float mu, e; // combined friction / restitution
    float kn, kt1, kt2;   // effective masses
    float ln, lt1, lt2;   // accumulated impulses
    float vn0;            // pre-solve normal velocity (restitution)
    V3 In, I1, I2;        // Iw (r x n), Iw (r x t1), Iw (r x t2): cached when CACHE
    bool on;
};

// The empty asm makes the lever arm opaque to loop-invariant code motion, so
// (r x n), Iw (r x n) ... are recomputed per row instead of being hoisted for all
// 8 slots out of the iteration loop (which spilled to scratch).
#define MG_OPAQUE3(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z))

template <bool CACHE, class B>
__device__ __forceinline__ void contact_normal(const B& G, Slot& c, V3& v, V3& w, float invm, const S3& Iw,
                                               float tgt) {
    if (!CACHE) MG_OPAQUE3(c.r);
    const float vn = G.vn(v, w, c.r);
    const float nl = fmaxf(fmaf(c.kn, tgt - vn, c.ln), 0.0f);
    const float dl = nl - c.ln;
    c.ln = nl;
    v = G.fn(v, dl, invm);
    w = fmad3(w, CACHE ? c.In : G.iwn(Iw, c.r), dl);
}

// Coulomb friction, PhysX-style pyramid: the two tangent rows are solved one
// after the other, each accumulated impulse clamped to [-mu ln, mu ln]
// (no sqrt / divide on the Gauss-Seidel chain).
template <bool CACHE, class B>
__device__ __forceinline__ void contact_friction(const B& G, Slot& c, V3& v, V3& w, float invm, const S3& Iw) {
    if (!CACHE) MG_OPAQUE3(c.r);
    const float lim = c.mu * c.ln;
    const float vt1 = G.v1(v, w, c.r);
    const float n1 = clamp_sym(fmaf(-c.kt1, vt1, c.lt1), lim);
    const float d1 = n1 - c.lt1;
    c.lt1 = n1;
    v = G.f1(v, d1, invm);
    w = fmad3(w, CACHE ? c.I1 : G.iw1(Iw, c.r), d1);
    const float vt2 = G.v2(v, w, c.r);
    const float n2 = clamp_sym(fmaf(-c.kt2, vt2, c.lt2), lim);
    const float d2 = n2 - c.lt2;
    c.lt2 = n2;
    v = G.f2(v, d2, invm);
    w = fmad3(w, CACHE ? c.I2 : G.iw2(Iw, c.r), d2);
}

// Row targets. Position iterations: v_n >= -s / sub, capped at the maximum
// depenetration velocity (the cap only binds while penetrating: for s >= 0 the
// target is <= 0 <= max_depen). Velocity iterations: v_n >= -s / h while
// separated, else 0, raised to the restitution bounce -e v_n0 above the
// bounce threshold.
__device__ __forceinline__ float pos_target(const MgStep& P, float s) { return fminf(-s * P.inv_sub, P.max_depen); }
__device__ __forceinline__ float vel_target(const MgStep& P, float s, float e, float vn0) {
    float tgt = fminf(-s * P.inv_h, 0.0f);
    if (e > 0.0f && vn0 < -P.bounce_thresh) tgt = fmaxf(tgt, -e * vn0);
    return tgt;
}

// Identity skips shared by both kernels and the oracle (the skipped
// composition with an identity pose / a zero offset returns its input up to
// the sign of zero terms).
__device__ __forceinline__ bool shape_pose_identity(const float* sh) {
    return sh[4] == 0.0f && sh[5] == 0.0f && sh[6] == 0.0f && sh[7] == 0.0f && sh[8] == 0.0f && sh[9] == 0.0f &&
           sh[10] == 1.0f;
}
// orientation of the principal inertia frame: q iq
__device__ __forceinline__ Q4 inertia_frame(Q4 q, Q4 iq) {
    if (iq.x == 0.0f && iq.y == 0.0f && iq.z == 0.0f && iq.w == 1.0f) return q;
    return qmul(q, iq);
}
// centre of mass in the world: x + q com
__device__ __forceinline__ V3 com_world(V3 x, Q4 q, V3 com) {
    if (com.x == 0.0f && com.y == 0.0f && com.z == 0.0f) return x;
    return vadd(x, qrot(q, com));
}
// body origin from the centre of mass: xc - q com
__device__ __forceinline__ V3 origin_from_com(V3 xc, Q4 q, V3 com) {
    if (com.x == 0.0f && com.y == 0.0f && com.z == 0.0f) return xc;
    return vsub(xc, qrot(q, com));
}

// Candidates of one shape: emit(k, point, separation, mu, e) with k the static
// candidate index within the shape (box corner bits zyx, capsule end 0/1, the
// k-th deepest hull vertex). BOX: the caller's shapes are all boxes at the body
// origin with the body's orientation (MgRigidArgs::box_only): only that branch
// is compiled, the same operations on a box as in the general build.
// PK (the one-round builds with their geometry on packed pairs, mg_pair.h): Rq
// is qmat(q), formed once per substep by the caller; a box with the body's
// orientation takes it as its own matrix.
template <bool BOX = false, bool PK = false, class B, class F>
__device__ __forceinline__ void shape_candidates(const B& G, const MgStep& P, const float* sh, Q4 q, V3 x,
                                                 const float* hulls, F&& emit, const M3* Rq = nullptr) {
    const int type = BOX ? MG_SHAPE_BOX : (int)sh[0];
    // shape pose in the world: a shape at the body origin with the body's
    // orientation (the usual URDF box / sphere) skips the composition
    Q4 qs = q;
    V3 cs = x;
    if constexpr (!BOX) {
        if (!shape_pose_identity(sh)) {
            qs = qmul(q, q4(sh[7], sh[8], sh[9], sh[10]));
            cs = vadd(x, qrot(q, v3(sh[4], sh[5], sh[6])));
        }
    }
    const float mu = 0.5f * (sh[11] + P.mu_ground);
    const float e = 0.5f * (sh[12] + P.e_ground);
    if (type == MG_SHAPE_BOX) {
        // the face whose outward normal is most opposed to n: axis i* maximises
        // |n . axis_i| (first index on ties), side s* = -sign(n . axis_i*); its 4
        // corners are the candidates k = 0..3 (signs of the two other axes)
        M3 Rs;
        if constexpr (PK) {
            Rs = *Rq;
            if constexpr (!BOX) {
                if (!shape_pose_identity(sh)) Rs = qmat(qs);
            }
        } else {
            Rs = qmat(qs);
        }
        const float d0 = G.dn(Rs.c0), d1 = G.dn(Rs.c1), d2 = G.dn(Rs.c2);
        const float ad0 = fabsf(d0), ad1 = fabsf(d1), ad2 = fabsf(d2);
        int ia = 0;
        float best = ad0;
        if (ad1 > best) { ia = 1; best = ad1; }
        if (ad2 > best) ia = 2;
        const V3 a0 = vscale(Rs.c0, sh[1]);
        const V3 a1 = vscale(Rs.c1, sh[2]);
        const V3 a2 = vscale(Rs.c2, sh[3]);
        const float di = ia == 0 ? d0 : (ia == 1 ? d1 : d2);
        const V3 ai = ia == 0 ? a0 : (ia == 1 ? a1 : a2);
        const V3 e1 = ia == 0 ? a1 : a0;
        const V3 e2 = ia == 2 ? a1 : a2;
        const V3 u = vscale(ai, di > 0.0f ? -1.0f : 1.0f);
        const V3 cu = vadd(cs, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float sx = (k & 1) ? 1.0f : -1.0f;
            const float sy = (k & 2) ? 1.0f : -1.0f;
            const V3 p = vadd(vadd(cu, vscale(e1, sx)), vscale(e2, sy));
            emit(k, p, G.dn(p) + P.pd, mu, e);
        }
    } else if (type == MG_SHAPE_SPHERE) {
        const float rad = sh[1];
        emit(0, G.addn(cs, -rad), G.dn(cs) + P.pd - rad, mu, e);
    } else if (type == MG_SHAPE_CAPSULE) {
        const float rad = sh[1];
        const V3 ax = vscale(qrot(qs, v3(1.0f, 0.0f, 0.0f)), sh[2]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const V3 c = k ? vadd(cs, ax) : vsub(cs, ax);
            emit(k, G.addn(c, -rad), G.dn(c) + P.pd - rad, mu, e);
        }
    } else if (type == MG_SHAPE_CONVEX) {
        // the 4 deepest hull vertices within the contact offset, ascending
        // separation, lower vertex index first on ties
        const float* hv = hulls + (int)sh[2];
        const int nv = (int)hv[0];
        float ks[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        V3 kp[4];
        int kn = 0;
        for (int i = 0; i < nv; ++i) {
            const float* v = hv + MG_HULL_HEADER + 3 * i;
            const V3 p = vadd(cs, qrot(qs, v3(v[0], v[1], v[2])));
            const float sep = G.dn(p) + P.pd;
            if (!(sep < P.contact_offset)) continue;
            if (kn == 4 && !(sep < ks[3])) continue;
            int at = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < kn && ks[k] <= sep) at = k + 1;
#pragma unroll
            for (int k = 3; k > 0; --k)
                if (k > at) { ks[k] = ks[k - 1]; kp[k] = kp[k - 1]; }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k == at) { ks[k] = sep; kp[k] = p; }
            if (kn < 4) kn = kn + 1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < kn) emit(k, kp[k], ks[k], mu, e);
    }
}

// MULTI = false: bodies with one shape, static slots (candidate k -> slot k),
// cached inertia vectors; MULTI = true: several shapes, shift-register slots.
// ATTR: the attractor-aware build (mg_attractor.h), stepped when a free body of
// the sim owns an attractor; a body without one runs the same operations as in
// the plain build. CREP: the reporting build, stepped while
// contact reporting is on: the last substep's slots go to the body's staging
// record, with the impulses that enter fsum.
// unit: the body's index in the launch (its flag word of the capacity report).
template <int MAXC, bool MULTI, bool ATTR, bool CREP, class B>
__device__ __forceinline__ void rigid_body(const B& G, const MgStep& P, const MgRigidArgs& A, int b, int unit) {
    constexpr bool CACHE = !MULTI;
    const int nb = A.nb;
    float* S = A.state;

    V3 x = v3(S[0 * nb + b], S[1 * nb + b], S[2 * nb + b]);
    Q4 q = q4(S[3 * nb + b], S[4 * nb + b], S[5 * nb + b], S[6 * nb + b]);
    V3 v = v3(S[7 * nb + b], S[8 * nb + b], S[9 * nb + b]);
    V3 w = v3(S[10 * nb + b], S[11 * nb + b], S[12 * nb + b]);

    const float* M = A.mass;
    const float invm = M[0 * nb + b];
    const V3 invI = v3(M[1 * nb + b], M[2 * nb + b], M[3 * nb + b]);
    const Q4 iq = q4(M[4 * nb + b], M[5 * nb + b], M[6 * nb + b], M[7 * nb + b]);
    const V3 com = v3(M[8 * nb + b], M[9 * nb + b], M[10 * nb + b]);

    const int tb = A.body_tmpl[b];
    const float lin_damp = A.tbf[tb * MG_TBODY_F_N + 0];
    const float ang_damp = A.tbf[tb * MG_TBODY_F_N + 1];
    const float max_lv = A.tbf[tb * MG_TBODY_F_N + 2];
    const float max_av = A.tbf[tb * MG_TBODY_F_N + 3];
    const float grav_on = A.tbf[tb * MG_TBODY_F_N + 4];
    const int sh0 = A.tbi[tb * MG_TBODY_I_N + 0];
    const int nsh = A.tbi[tb * MG_TBODY_I_N + 1];

    V3 fext = v3(0.0f, 0.0f, 0.0f), text = v3(0.0f, 0.0f, 0.0f);
    if (A.ext) {
        fext = v3(A.ext[0 * nb + b], A.ext[1 * nb + b], A.ext[2 * nb + b]);
        text = v3(A.ext[3 * nb + b], A.ext[4 * nb + b], A.ext[5 * nb + b]);
    }

    const float h = P.h;
    const float lin_keep = 1.0f - fminf(lin_damp * h, 1.0f);
    const float ang_keep = 1.0f - fminf(ang_damp * h, 1.0f);
    const float max_lv2 = max_lv * max_lv;
    const float max_av2 = max_av * max_av;
    const float* at = nullptr;
    if constexpr (ATTR) {
        const int ai = A.attr_idx[b];
        if (ai >= 0) at = A.attr + (size_t)ai * MG_ATTR_N;
    }

    q = qnormalize(q);
    V3 fsum = v3(0.0f, 0.0f, 0.0f);
    int crk = 0;   // CREP: entries staged

    for (int st = 0; st < P.substeps; ++st) {
        const S3 Iw = sym_rdrt(qmat(inertia_frame(q, iq)), invI);
        const V3 xc = com_world(x, q, com);

        // 1. unconstrained velocity
        if (grav_on != 0.0f) v = vmad(v, v3(P.g[0], P.g[1], P.g[2]), h);
        if (A.ext) {   // applied wrench this frame (uniform; none: no update, as the oracle)
            v = vmad(v, fext, invm * h);
            w = vmad(w, symmul(Iw, text), h);
        }
        if constexpr (ATTR) {
            if (at) attr_free_body(at, x, q, xc, invm, invI, iq, h, v, w);
        }
        v = vscale(v, lin_keep);
        w = vscale(w, ang_keep);
        {
            float v2 = vdot(v, v);
            if (v2 > max_lv2) v = vscale(v, sqrtf(max_lv2 / v2));
            float w2 = vdot(w, w);
            if (w2 > max_av2) w = vscale(w, sqrtf(max_av2 / w2));
        }

        // 2. contacts against the ground plane
        Slot sl[MAXC];
#pragma unroll
        for (int j = 0; j < MAXC; ++j) sl[j].on = false;
        if (P.has_ground) {
            if constexpr (!MULTI) {
                // static slots: candidate k of the only shape lives in slot k
                if (nsh == 1)
                shape_candidates(G, P, A.shapes + sh0 * MG_SHAPE_STRIDE, q, x, A.hulls,
                                 [&](int k, V3 p, float sep, float mu, float e) {
                                     if (sep < P.contact_offset) {
                                         sl[k].on = true;
                                         sl[k].r = vsub(p, xc);
                                         sl[k].s0 = sep - P.rest_offset;
                                         sl[k].mu = mu;
                                         sl[k].e = e;
                                     }
                                 });
            } else {
                // several shapes: shift-register insert, newest candidate in slot 0
                // (ncand counts every candidate, without a branch: those past the
                // MAXC slots are ignored)
                int nc = 0, ncand = 0;
                for (int s = sh0; s < sh0 + nsh; ++s) {
                    shape_candidates(G, P, A.shapes + s * MG_SHAPE_STRIDE, q, x, A.hulls,
                                     [&](int, V3 p, float sep, float mu, float e) {
                                         ncand += sep < P.contact_offset ? 1 : 0;
                                         if (sep < P.contact_offset && nc < MAXC) {
#pragma unroll
                                             for (int j = MAXC - 1; j > 0; --j) {
                                                 sl[j].r = sl[j - 1].r; sl[j].s0 = sl[j - 1].s0;
                                                 sl[j].mu = sl[j - 1].mu; sl[j].e = sl[j - 1].e;
                                                 sl[j].on = sl[j - 1].on;
                                             }
                                             sl[0].r = vsub(p, xc); sl[0].s0 = sep - P.rest_offset;
                                             sl[0].mu = mu; sl[0].e = e; sl[0].on = true;
                                             nc = nc + 1;
                                         }
                                     });
                }
                // one atomic per counter for the wave, each such body its own flag word
                const unsigned long long ob = __ballot(ncand > MAXC);
                if (ob) {
                    const int ndrop = mg_cap_wave_sum(ncand > MAXC ? ncand - MAXC : 0);
                    if (ncand > MAXC) atomicOr(A.cap.flags + unit, MG_CAPF_RIGID_SLOTS);
                    if (threadIdx.x == (unsigned)(__ffsll(ob) - 1)) {
                        mg_cap_add(A.cap, MG_CAP_RIGID_OVERFLOW, __popcll(ob));
                        mg_cap_add(A.cap, MG_CAP_RIGID_CANDIDATES_DROPPED, ndrop);
                    }
                }
            }
        }
        // contact constants
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            if (sl[j].on) {
                const V3 In = G.iwn(Iw, sl[j].r), I1 = G.iw1(Iw, sl[j].r), I2 = G.iw2(Iw, sl[j].r);
                if (CACHE) { sl[j].In = In; sl[j].I1 = I1; sl[j].I2 = I2; }
                sl[j].kn = 1.0f / (invm + G.kn(sl[j].r, In));
                sl[j].kt1 = 1.0f / (invm + G.k1(sl[j].r, I1));
                sl[j].kt2 = 1.0f / (invm + G.k2(sl[j].r, I2));
                sl[j].ln = 0.0f; sl[j].lt1 = 0.0f; sl[j].lt2 = 0.0f;
                sl[j].vn0 = G.vn(v, w, sl[j].r);
            }
        }

        // 3. TGS position iterations: every normal row, then every friction row
        V3 dx = v3(0.0f, 0.0f, 0.0f), dth = v3(0.0f, 0.0f, 0.0f);
        for (int it = 0; it < P.npos; ++it) {
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                if (sl[j].on) {
                    const float s = G.ps(sl[j].s0, dx, dth, sl[j].r);
                    contact_normal<CACHE>(G, sl[j], v, w, invm, Iw, pos_target(P, s));
                }
            }
#pragma unroll
            for (int j = 0; j < MAXC; ++j)
                if (sl[j].on) contact_friction<CACHE>(G, sl[j], v, w, invm, Iw);
            dx = fmad3(dx, v, P.sub);
            dth = fmad3(dth, w, P.sub);
        }
        // velocity iterations (bias removed)
        for (int it = 0; it < P.nvel; ++it) {
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                if (sl[j].on) {
                    const float s = G.ps(sl[j].s0, dx, dth, sl[j].r);
                    contact_normal<CACHE>(G, sl[j], v, w, invm, Iw, vel_target(P, s, sl[j].e, sl[j].vn0));
                }
            }
#pragma unroll
            for (int j = 0; j < MAXC; ++j)
                if (sl[j].on) contact_friction<CACHE>(G, sl[j], v, w, invm, Iw);
        }
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            if (sl[j].on) {
                fsum = G.addn(fsum, sl[j].ln);
                fsum = G.add1(fsum, sl[j].lt1);
                fsum = G.add2(fsum, sl[j].lt2);
            }
        }
        if constexpr (CREP) {
            if (st == P.substeps - 1) {
                const V3 z3 = v3(0.0f, 0.0f, 0.0f);
                const int gb = A.crep_body[b];
#pragma unroll
                for (int j = 0; j < MAXC; ++j) {
                    if (sl[j].on && crk < MG_CREP_FREE_CAP) {
                        // per-point friction rows: the point carries its friction impulse
                        crep_store(A.crep + b, A.crep_stride, crk, gb, -1, 0, vadd(xc, sl[j].r), G.addn(z3, 1.0f),
                                   sl[j].s0, sl[j].ln, G.add2(G.add1(z3, sl[j].lt1), sl[j].lt2), sl[j].mu);
                        crk = crk + 1;
                    }
                }
            }
        }

        // 4. pose update (centre of mass moves by the integrated delta)
        const V3 xc1 = vadd(xc, dx);
        q = qintegrate(q, dth);
        x = origin_from_com(xc1, q, com);
    }

    S[0 * nb + b] = x.x; S[1 * nb + b] = x.y; S[2 * nb + b] = x.z;
    S[3 * nb + b] = q.x; S[4 * nb + b] = q.y; S[5 * nb + b] = q.z; S[6 * nb + b] = q.w;
    S[7 * nb + b] = v.x; S[8 * nb + b] = v.y; S[9 * nb + b] = v.z;
    S[10 * nb + b] = w.x; S[11 * nb + b] = w.y; S[12 * nb + b] = w.z;
    A.cforce[0 * nb + b] = fsum.x * P.inv_dt;
    A.cforce[1 * nb + b] = fsum.y * P.inv_dt;
    A.cforce[2 * nb + b] = fsum.z * P.inv_dt;
    if constexpr (CREP) A.crep_n[b] = crk;
}

// ---- single-shape bodies: k_rigid_step1 ------------------------------------
#ifndef MG_RIGID1_SHAPE_REGS
#define MG_RIGID1_SHAPE_REGS 1
#endif
// One-round launches without an attractor or a contact report form their
// geometry on packed f32 pairs (mg_pair.h); 0 builds the scalar form for A/B
// runs (tools/build_variant.sh).
#ifndef MG_RIGID1_PACK_GEOM
#define MG_RIGID1_PACK_GEOM 1
#endif
// The one-round +Z builds with packed geometry (tgs_zp and the packed row
// constants), each 0 for the form before it (A/B runs as above):
// SWEEP_PAIRS: tgs_zp's loops run two sweeps per trip (no impulse copies);
// RECIP_PAIRS: the rows' effective masses by rcp2_ieee (mg_pair.h) on every
// lane with one select each, in place of a division per exec bracket.
#ifndef MG_RIGID1_SWEEP_PAIRS
#define MG_RIGID1_SWEEP_PAIRS 1
#endif
#ifndef MG_RIGID1_RECIP_PAIRS
#define MG_RIGID1_RECIP_PAIRS 1
#endif
// Friction is PhysX's patch friction, as in the coupled
// step (§3.6.1): the body-ground pair's contacts form one patch whose friction
// acts at up to two anchors, each fixed on the body (body frame) and on the
// ground (world point), kept from substep to substep and from step to step
// while the body's copy stays within the correlation distance of the ground's
// and the normal holds (cos >= MG_FP_NORMAL_COS in the body frame); anchors grow
// from this substep's contacts in slot order and spread over the patch
// (ground_patch_update). The record (MG_FP_N floats, the coupled record's layout) lives in
// HBM, SoA [MG_FP_N][nf1]: field 0 (the anchor count) is written every step,
// the rest only while anchors are held; a body that cannot touch the ground at
// the step's start (the far skip below) does not use it — its first substep
// has no contact, which drops any patch (a wide launch does not read it then; a
// one-round launch has fetched it with its other inputs and selects zeros).
struct GPatch {
    int cnt;
    bool dirty;     // anchors / normal differ from the stored record (written back at the step's end)
    V3 nA;          // patch normal in the body frame
    V3 aA[2];       // anchor on the body (body frame)
    V3 aB[2];       // anchor on the ground (world)
};
// Anchors are placed by candidate index during the scan and turned into body
// copies (qrot_inv(q, p - x)) once per slot after it, from the scan points w0 /
// w1 (the candidate each slot ended with): the oracle's gpatch_update_ values.
// The normal test takes only the normal component of the rotated patch normal
// (G.dn: for the +Z ground one component of qrot; the same value as the
// oracle's dot product).
// Branch-free: every candidate value is formed on every lane and the oracle's
// branches become selects (the lanes of a wave hold different contact states,
// so the branches diverged and the wave paid every side plus the exec-mask
// bookkeeping: ~2.9k cycles per substep of a vehicle wave, tools/
// kbench_rigid_stamps.py). The values selected are the ones the branches
// computed, by the same operations, so results are unchanged.
template <class B>
__device__ __forceinline__ void ground_patch_update(const B& G, GPatch& R, V3 x, Q4 q, V3 n0, const V3 (&p)[4],
                                                    const float (&s0)[4], const bool (&on)[4], float fot,
                                                    float corr) {
    const float c2 = corr * corr;
    const V3 z3 = v3(0.0f, 0.0f, 0.0f);
    int cnt = R.cnt;
    const float nd = G.dn(qrot(q, R.nA));
    if (cnt > 0 && nd < MG_FP_NORMAL_COS) cnt = 0;
    // held anchors: kept while the body's copy stays within the correlation
    // distance of the ground's
    const V3 wa0 = vadd(x, qrot(q, R.aA[0]));
    const V3 wa1 = vadd(x, qrot(q, R.aA[1]));
    const V3 d0v = vsub(wa0, R.aB[0]), d1v = vsub(wa1, R.aB[1]);
    const bool k0 = 0 < cnt && vdot(d0v, d0v) <= c2;
    const bool k1 = 1 < cnt && vdot(d1v, d1v) <= c2;
    GPatch N;
    N.aA[0] = vsel(k0, R.aA[0], vsel(k1, R.aA[1], z3));
    N.aB[0] = vsel(k0, R.aB[0], vsel(k1, R.aB[1], z3));
    N.aA[1] = vsel(k0 && k1, R.aA[1], z3);
    N.aB[1] = vsel(k0 && k1, R.aB[1], z3);
    V3 w0 = vsel(k0, wa0, vsel(k1, wa1, z3));
    V3 w1 = z3;
    const int kept = (k0 ? 1 : 0) + (k1 ? 1 : 0);
    // growth from this substep's contacts in slot order (only while fewer than
    // two anchors are held): the first, then one farther than the correlation
    // distance, then a candidate replacing whichever end spreads the pair most
    int nc = kept;
    float dd = 0.0f;
    bool set0 = false, set1 = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool c = kept < 2 && on[j] && s0[j] <= fot;
        const V3 pj = p[j];
        const V3 e0 = vsub(pj, w0), e1 = vsub(pj, w1);
        const float dj0 = vdot(e0, e0), dj1 = vdot(e1, e1);
        const bool a0 = c && nc == 0;
        const bool a1 = c && nc == 1 && dj0 > c2;
        const bool a2 = c && nc == 2 && dj0 > dj1 && dj0 > dd;
        const bool a3 = c && nc == 2 && !(dj0 > dj1) && dj1 > dd;
        const bool to0 = a0 || a3, to1 = a1 || a2;
        dd = (a1 || a2) ? dj0 : (a3 ? dj1 : dd);
        w0 = vsel(to0, pj, w0);
        w1 = vsel(to1, pj, w1);
        set0 = set0 || to0;
        set1 = set1 || to1;
        nc = a0 ? 1 : (a1 ? 2 : nc);
    }
    N.aA[0] = vsel(set0, qrot_inv(q, vsub(w0, x)), N.aA[0]);
    N.aB[0] = vsel(set0, w0, N.aB[0]);
    N.aA[1] = vsel(set1, qrot_inv(q, vsub(w1, x)), N.aA[1]);
    N.aB[1] = vsel(set1, w1, N.aB[1]);
    N.cnt = nc;
    N.nA = vsel(kept > 0, R.nA, qrot_inv(q, n0));
    // the stored record changes unless every held anchor was kept in place and
    // none was placed (a resting body: most steps)
    N.dirty = R.dirty || !(kept == R.cnt && nc == kept);
    R = N;
}

// ground_patch_update on packed f32 pairs (mg_pair.h), for the one-round
// launches (a lone wave is issue-bound: DESIGN.md §3.2). The same values by the
// same operations, two at a time: the held anchors' world copies with their
// distance tests, qrot(q, nA) beside qrot_inv(q, n0) as one rotation by the
// quaternion pair (q, conj q), each scan candidate's e0 / e1 and dj0 / dj1 with
// the scan points kept as the pair (w0, w1), and the two closing qrot_inv.
// Compares and selects act on the halves.
template <class B>
__device__ __forceinline__ void ground_patch_update_pk(const B& G, GPatch& R, V3 x, Q4 q, V3 n0, const V3 (&p)[4],
                                                       const float (&s0)[4], const bool (&on)[4], float fot,
                                                       float corr) {
    const float c2 = corr * corr;
    const V3 z3 = v3(0.0f, 0.0f, 0.0f);
    int cnt = R.cnt;
    // (qrot(q, nA), qrot_inv(q, n0))
    const V3x2 nn = qrotq2(q4x2(q, qconj(q)), v3x2(R.nA, n0));
    const float nd = G.dn(v3lo(nn));
    if (cnt > 0 && nd < MG_FP_NORMAL_COS) cnt = 0;
    const V3x2 X = v3bc(x);
    const V3x2 wa = vadd2(X, qrot2(q, v3x2(R.aA[0], R.aA[1])));
    const V3x2 dv = vsub2(wa, v3x2(R.aB[0], R.aB[1]));
    const f2 dq = vdot2(dv, dv);
    const bool k0 = 0 < cnt && dq.x <= c2;
    const bool k1 = 1 < cnt && dq.y <= c2;
    const V3 wa0 = v3lo(wa), wa1 = v3hi(wa);
    GPatch N;
    N.aA[0] = vsel(k0, R.aA[0], vsel(k1, R.aA[1], z3));
    N.aB[0] = vsel(k0, R.aB[0], vsel(k1, R.aB[1], z3));
    N.aA[1] = vsel(k0 && k1, R.aA[1], z3);
    N.aB[1] = vsel(k0 && k1, R.aB[1], z3);
    V3x2 W = v3x2(vsel(k0, wa0, vsel(k1, wa1, z3)), z3);   // (w0, w1)
    const int kept = (k0 ? 1 : 0) + (k1 ? 1 : 0);
    int nc = kept;
    float dd = 0.0f;
    bool set0 = false, set1 = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool c = kept < 2 && on[j] && s0[j] <= fot;
        const V3 pj = p[j];
        const V3x2 E = vsub2(v3bc(pj), W);   // (e0, e1)
        const f2 dj = vdot2(E, E);
        const float dj0 = dj.x, dj1 = dj.y;
        const bool a0 = c && nc == 0;
        const bool a1 = c && nc == 1 && dj0 > c2;
        const bool a2 = c && nc == 2 && dj0 > dj1 && dj0 > dd;
        const bool a3 = c && nc == 2 && !(dj0 > dj1) && dj1 > dd;
        const bool to0 = a0 || a3, to1 = a1 || a2;
        dd = (a1 || a2) ? dj0 : (a3 ? dj1 : dd);
        W.x = pk2(to0 ? pj.x : W.x.x, to1 ? pj.x : W.x.y);
        W.y = pk2(to0 ? pj.y : W.y.x, to1 ? pj.y : W.y.y);
        W.z = pk2(to0 ? pj.z : W.z.x, to1 ? pj.z : W.z.y);
        set0 = set0 || to0;
        set1 = set1 || to1;
        nc = a0 ? 1 : (a1 ? 2 : nc);
    }
    const V3x2 bA = qrot_inv2(q, vsub2(W, X));
    N.aA[0] = vsel(set0, v3lo(bA), N.aA[0]);
    N.aB[0] = vsel(set0, v3lo(W), N.aB[0]);
    N.aA[1] = vsel(set1, v3hi(bA), N.aA[1]);
    N.aB[1] = vsel(set1, v3hi(W), N.aB[1]);
    N.cnt = nc;
    N.nA = vsel(kept > 0, R.nA, v3hi(nn));
    N.dirty = R.dirty || !(kept == R.cnt && nc == kept);
    R = N;
}

// Normal row of the branch-free solver: an inactive slot holds r = 0, s0 = 0
// and kn = 0, so it computes ln = max(0 + 0 (tgt - vn), 0) = 0 and applies a
// zero impulse. Anchor rows likewise (k = 0, r = 0: raw 0 within any bound).
struct NRow {
    V3 r, In;                 // contact point - COM; Iw (r x n)
    float s0, kn, ln, vn0;
};
struct ARow {
    V3 r, I1, I2;             // anchor (body copy) - COM; Iw (r x t1), Iw (r x t2)
    float k1, k2, l1, l2;     // effective masses, accumulated impulses along t1, t2
    float e1, e2;             // position-sweep target velocities (drift closing)
};

template <class B>
__device__ __forceinline__ void row_normal1(const B& G, NRow& c, V3& v, V3& w, float invm, float tgt) {
    const float vn = G.vn(v, w, c.r);
    const float nl = fmaxf(fmaf(c.kn, tgt - vn, c.ln), 0.0f);
    const float dl = nl - c.ln;
    c.ln = nl;
    v = G.fn(v, dl, invm);
    w = fmad3(w, c.In, dl);
}

// ---- +Z ground: the solver on packed f32 pairs -------------------------------
// The same sweeps as rigid_body1's scalar loop with BasisZ (normal rows, the
// patch's anchor rows t1 = +y, t2 = -x, the closing normal pass of the last
// position sweep and the velocity sweeps), but the velocity state lives in
// register pairs W = (w.x, w.y), Z = (w.z, v.z), V = (v.x, v.y) (the motion
// delta in DW = (dth.x, dth.y), DZ = (dth.z, dx.z), DV = (dx.x, dx.y)), so one
// v_pk_fma_f32 applies two of a row's impulse updates and the separations of two
// slots share one packed chain. Each half of a packed op is the same correctly
// rounded fma / add / mul as the scalar form, so results are bit-identical to
// the scalar loop and to the oracle; only the issue count drops. Used by
// launches that fit in one resident round (the latency regime: DESIGN.md §3.2).
// (f2, pk2, bc2, pfma: mg_pair.h)

// lim1 = share * mu: an anchor row's bound per unit of the patch's normal impulse
// PAIRS (rigid_body1's PKG builds, MG_RIGID1_SWEEP_PAIRS): two sweeps per loop trip
template <bool PAIRS>
__device__ __forceinline__ void tgs_zp(const MgStep& P, NRow (&sl)[4], ARow (&an)[2], float lim1, float e, V3& v,
                                       V3& w, V3& dx, V3& dth, float invm, bool& c01, bool& c02, bool& c11,
                                       bool& c12) {
    f2 W = pk2(w.x, w.y), Z = pk2(w.z, v.z), V = pk2(v.x, v.y);
    f2 DW = pk2(dth.x, dth.y), DZ = pk2(dth.z, dx.z), DV = pk2(dx.x, dx.y);
    // the packed operands are named values, not arrays: an array of pairs built
    // lane by lane was kept in scratch (a memory round trip per substep)
    float s0r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // register copies: the pairs of loads were built through scratch
        s0r[j] = sl[j].s0;
        asm volatile("" : "+v"(s0r[j]));
    }
    const f2 S0a = pk2(s0r[0], s0r[1]), S0b = pk2(s0r[2], s0r[3]);
    const f2 RYa = pk2(sl[0].r.y, sl[1].r.y), RYb = pk2(sl[2].r.y, sl[3].r.y);
    const f2 NRXa = pk2(-sl[0].r.x, -sl[1].r.x), NRXb = pk2(-sl[2].r.x, -sl[3].r.x);
    // separations of slots (2h, 2h+1): s0 + dx.z + dth.x r.y - dth.y r.x (BasisZ::ps)
    auto sep = [&](int h) {
        f2 a = (h ? S0b : S0a) + bc2(DZ.y);
        a = pfma(bc2(DW.x), h ? RYb : RYa, a);
        return pfma(bc2(DW.y), h ? NRXb : NRXa, a);
    };
    auto normal = [&](int j, float tgt) {
        const float nrx = -sl[j].r.x, ry = sl[j].r.y;
        const float vn = fmaf(W.y, nrx, fmaf(W.x, ry, Z.y));
        const float nl = fmaxf(fmaf(sl[j].kn, tgt - vn, sl[j].ln), 0.0f);
        const float dl = nl - sl[j].ln;
        sl[j].ln = nl;
        W = pfma(pk2(sl[j].In.x, sl[j].In.y), bc2(dl), W);
        Z = pfma(pk2(sl[j].In.z, invm), bc2(dl), Z);   // Z = (w.z, v.z): In.z and 1/m (BasisZ::fn)
    };
    // the anchors' rows: t1 = +y (BasisZ::v1 / f1), t2 = -x (v2 / f2)
    auto anchors = [&](bool pos, bool last) {
        const float lim = lim1 * (((sl[0].ln + sl[1].ln) + sl[2].ln) + sl[3].ln);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float rx = an[a].r.x, ry = an[a].r.y, nrz = -an[a].r.z;
            {
                const float v1 = fmaf(Z.x, rx, fmaf(W.x, nrz, V.y));
                const float raw = fmaf(an[a].k1, (pos ? an[a].e1 : 0.0f) - v1, an[a].l1);
                const float nl = clamp_sym(raw, lim);
                const float dl = nl - an[a].l1;
                const bool cl = last && (raw > lim || raw < -lim);
                if (a == 0) c01 = cl; else c11 = cl;
                an[a].l1 = nl;
                V.y = fmaf(dl, invm, V.y);
                W = pfma(pk2(an[a].I1.x, an[a].I1.y), bc2(dl), W);
                Z.x = fmaf(an[a].I1.z, dl, Z.x);
            }
            {
                const float v2 = fmaf(Z.x, ry, fmaf(W.y, nrz, -V.x));
                const float raw = fmaf(an[a].k2, (pos ? an[a].e2 : 0.0f) - v2, an[a].l2);
                const float nl = clamp_sym(raw, lim);
                const float dl = nl - an[a].l2;
                const bool cl = last && (raw > lim || raw < -lim);
                if (a == 0) c02 = cl; else c12 = cl;
                an[a].l2 = nl;
                V.x = fmaf(-dl, invm, V.x);
                W = pfma(pk2(an[a].I2.x, an[a].I2.y), bc2(dl), W);
                Z.x = fmaf(an[a].I2.z, dl, Z.x);
            }
        }
    };
    const f2 nsub = bc2(-P.inv_sub), psub = bc2(P.sub);
    const int nit = P.npos + P.nvel;
    if constexpr (PAIRS) {
        // sweep order (round 6, as the oracle): a position sweep is the anchors'
        // rows then the normal rows (non-penetration has the last word before the
        // velocity is integrated); only the first opens with the normal rows.
        // The first sweep stands in front of the loop, the rest run two per trip
        // and an odd one after it: a row's new impulse is formed from the old one
        // and both are read once more (dl = nl - ln), so a loop of one sweep per
        // trip copied all eight accumulated impulses at its head; with two sweeps
        // per trip the second writes the registers the first read.
        auto pos_sweep = [&](bool first, bool last) {
            const f2 t0 = sep(0) * nsub, t1 = sep(1) * nsub;   // -s / sub of each slot
            const float tg[4] = {fminf(t0.x, P.max_depen), fminf(t0.y, P.max_depen), fminf(t1.x, P.max_depen),
                                 fminf(t1.y, P.max_depen)};
            if (first) {
#pragma unroll
                for (int j = 0; j < 4; ++j) normal(j, tg[j]);
            }
            anchors(true, last);
#pragma unroll
            for (int j = 0; j < 4; ++j) normal(j, tg[j]);   // same targets: dx, dth unchanged
            DV = pfma(V, psub, DV);
            DW = pfma(W, psub, DW);
            DZ = pfma(Z, psub, DZ);
        };
        auto vel_sweep = [&](const float (&tg)[4], bool last) {
#pragma unroll
            for (int j = 0; j < 4; ++j) normal(j, tg[j]);
            anchors(false, last);
#pragma unroll
            for (int j = 0; j < 4; ++j) normal(j, tg[j]);
        };
        if (P.npos > 0) {
            pos_sweep(true, nit == 1);
            int it = 1;
            for (; it + 2 <= P.npos; it += 2) {
                pos_sweep(false, false);   // a sweep followed by another is never the last
                pos_sweep(false, it + 1 == nit - 1);
            }
            if (it < P.npos) pos_sweep(false, it == nit - 1);
        }
        if (P.nvel > 0) {
            const f2 s01 = sep(0), s23 = sep(1);
            const float sj[4] = {s01.x, s01.y, s23.x, s23.y};
            float tg[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) tg[j] = vel_target(P, sj[j], e, sl[j].vn0);
            int it = P.npos;
            for (; it + 2 <= nit; it += 2) {
                vel_sweep(tg, false);
                vel_sweep(tg, it + 1 == nit - 1);
            }
            if (it < nit) vel_sweep(tg, true);
        }
    } else {
        // sweep order (round 6, as the oracle): a position sweep is the anchors'
        // rows then the normal rows (non-penetration has the last word before the
        // velocity is integrated); only the first opens with the normal rows
        for (int it = 0; it < P.npos; ++it) {
            const f2 t0 = sep(0) * nsub, t1 = sep(1) * nsub;   // -s / sub of each slot
            const float tg[4] = {fminf(t0.x, P.max_depen), fminf(t0.y, P.max_depen), fminf(t1.x, P.max_depen),
                                 fminf(t1.y, P.max_depen)};
            if (it == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) normal(j, tg[j]);
            }
            anchors(true, it == nit - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) normal(j, tg[j]);   // same targets: dx, dth unchanged
            DV = pfma(V, psub, DV);
            DW = pfma(W, psub, DW);
            DZ = pfma(Z, psub, DZ);
        }
        if (P.nvel > 0) {
            const f2 s01 = sep(0), s23 = sep(1);
            const float sj[4] = {s01.x, s01.y, s23.x, s23.y};
            float tg[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) tg[j] = vel_target(P, sj[j], e, sl[j].vn0);
            for (int it = P.npos; it < nit; ++it) {
#pragma unroll
                for (int j = 0; j < 4; ++j) normal(j, tg[j]);
                anchors(false, it == nit - 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) normal(j, tg[j]);
            }
        }
    }
    v = v3(V.x, V.y, Z.y);
    w = v3(W.x, W.y, Z.x);
    dx = v3(DV.x, DV.y, DZ.y);
    dth = v3(DW.x, DW.y, DZ.x);
}

// T: this body's compact template record (MG_TREC_N floats: MG_TBODY_F_N
// template floats, then the shape record; shape type < 0 when it has none).
// R: the ground patch at the step's start (cnt 0: none), at its end on return.
// at (ATTR builds): this body's attractor record, or null.
// CREP (the reporting builds): cr is the body's staging record
// (null: a dead lane), crs its stride, gbody the body's global index; the last
// substep's points and anchors are stored there with the impulses that enter
// fsum. Returns the number of entries staged. BOX: shape_candidates' box build.
template <bool PACK, bool ATTR, bool CREP, bool BOX = false, class B>
__device__ __forceinline__ int rigid_body1(const B& G, const MgStep& P, const float* T, V3& x, Q4& q, V3& v,
                                           V3& w, V3& fsum, float invm, V3 invI, Q4 iq, V3 com, bool has_ext,
                                           V3 fext, V3 text, const float* hulls, float* gp, int gstride,
                                           const float (&pr)[MG_FP_N], const float* at, float* cr = nullptr,
                                           int crs = 0, int gbody = 0) {
    int crk = 0;
    // geometry on packed pairs: the one-round builds without attractor or report
    constexpr bool PKG = PACK && !ATTR && !CREP && MG_RIGID1_PACK_GEOM;
    const float lin_damp = T[0], ang_damp = T[1], max_lv = T[2], max_av = T[3], grav_on = T[4];
    // the shape record: wide launches read it from the template record (LDS
    // when staged) in each substep's candidate search — registers are scarcer
    // than LDS reads at three waves per SIMD; a one-round launch (PACK) keeps it
    // in registers (the LDS reads were on each substep's dependency chain)
    float shr[MG_SHAPE_STRIDE];
    const float* sh = T + MG_TBODY_F_N;
    if constexpr (PACK && MG_RIGID1_SHAPE_REGS) {
#pragma unroll
        for (int k = 0; k < 14; ++k) shr[k] = sh[k];
        sh = shr;
    }
    const bool has_shape = P.has_ground && sh[0] >= 0.0f;
    const float rho = sh[13];   // bounding radius about the body origin (< 0: none)
    const float h = P.h;
    const float lin_keep = 1.0f - fminf(lin_damp * h, 1.0f);
    const float ang_keep = 1.0f - fminf(ang_damp * h, 1.0f);
    const float max_lv2 = max_lv * max_lv;
    const float max_av2 = max_av * max_av;
    const float mu = 0.5f * (sh[11] + P.mu_ground);
    const float e = 0.5f * (sh[12] + P.e_ground);
    const V3 n0 = v3(P.n[0], P.n[1], P.n[2]);
    // the ground patch kept from the last step: read only by a body that can
    // touch the ground at this step's start (otherwise its first substep has no
    // contact and drops the patch, whatever the record holds)
    GPatch R;
    R.cnt = 0;
    R.dirty = false;
    R.nA = R.aA[0] = R.aA[1] = R.aB[0] = R.aB[1] = v3(0.0f, 0.0f, 0.0f);
    {
        const float clear = G.dn(x) + P.pd;
        const bool far = rho >= 0.0f && clear - rho > P.contact_offset + 1e-3f * (1.0f + fabsf(clear) + rho);
        const bool use = gp && has_shape && !far;
        if constexpr (PACK) {
            // a one-round launch loaded the record beside its other inputs
            // (pr, k_rigid_step1): selected here, not read — the same values
            // for a body that reads it, the same zeros for one that does not
            R.cnt = (int)(use ? pr[0] : 0.0f);
            R.nA = vsel(use, v3(pr[1], pr[2], pr[3]), R.nA);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                R.aA[k] = vsel(use, v3(pr[4 + 6 * k], pr[5 + 6 * k], pr[6 + 6 * k]), R.aA[k]);
                R.aB[k] = vsel(use, v3(pr[7 + 6 * k], pr[8 + 6 * k], pr[9 + 6 * k]), R.aB[k]);
            }
        } else if (use) {
            float r[MG_FP_N];
#pragma unroll
            for (int k = 0; k < MG_FP_N; ++k) r[k] = gp[(size_t)k * gstride];
            R.cnt = (int)r[0];
            R.nA = v3(r[1], r[2], r[3]);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                R.aA[k] = v3(r[4 + 6 * k], r[5 + 6 * k], r[6 + 6 * k]);
                R.aB[k] = v3(r[7 + 6 * k], r[8 + 6 * k], r[9 + 6 * k]);
            }
        }
    }

    RUSE(R.cnt); RUSE(R.aA[1].z);
    RSTAMP(2);   // patch record read
    q = qnormalize(q);
    for (int st = 0; st < P.substeps; ++st) {
        // PKG: qmat(q) is formed once per substep, for the candidates and, when
        // the principal frame is the body's (inertia_frame's identity skip), for
        // Iw: the same function of the same input; Iw's entries as pairs
        M3 Rq;
        S3P Ip;
        S3 Iw;
        if constexpr (PKG) {
            Rq = qmat(q);
            M3 Rp = Rq;
            if (!(iq.x == 0.0f && iq.y == 0.0f && iq.z == 0.0f && iq.w == 1.0f)) Rp = qmat(qmul(q, iq));
            Iw = sym_rdrt_p(Rp, invI, Ip);
        } else {
            Iw = sym_rdrt(qmat(inertia_frame(q, iq)), invI);
        }
        const V3 xc = com_world(x, q, com);

        // 1. unconstrained velocity
        if (grav_on != 0.0f) v = vmad(v, v3(P.g[0], P.g[1], P.g[2]), h);
        if (has_ext) {   // applied wrench this frame (uniform; none: no update, as the oracle)
            v = vmad(v, fext, invm * h);
            w = vmad(w, symmul(Iw, text), h);
        }
        if constexpr (ATTR) {
            if (at) attr_free_body(at, x, q, xc, invm, invI, iq, h, v, w);
        }
        v = vscale(v, lin_keep);
        w = vscale(w, ang_keep);
        {
            float v2 = vdot(v, v);
            if (v2 > max_lv2) v = vscale(v, sqrtf(max_lv2 / v2));
            float w2 = vdot(w, w);
            if (w2 > max_av2) w = vscale(w, sqrtf(max_av2 / w2));
        }

        RUSE(v.x); RUSE(w.z); RUSE(xc.x);
        if (st < 2) RSTAMP(3 + 6 * st);   // free-flight velocity, Iw, COM
        // 2. ground contacts: candidate k of the shape -> slot k
        NRow sl[4];
        bool on[4];
        V3 cp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            on[j] = false;
            sl[j].r = v3(0.0f, 0.0f, 0.0f);
            sl[j].s0 = 0.0f;
            cp[j] = v3(0.0f, 0.0f, 0.0f);
        }
        // a body clearing the plane by more than its bounding radius (plus a
        // rounding margin far above the candidates' own error) has no candidate
        // within contact_offset: a wave of only such bodies skips the search
        const float clear = G.dn(x) + P.pd;
        const bool far = rho >= 0.0f && clear - rho > P.contact_offset + 1e-3f * (1.0f + fabsf(clear) + rho);
        if (__any(has_shape && !far) && has_shape)
            shape_candidates<BOX, PKG>(G, P, sh, q, x, hulls, [&](int k, V3 p, float sep, float, float) {
                // selects, not a branch: the candidates of a wave's bodies pass
                // the test on different lanes
                const bool c = sep < P.contact_offset;
                on[k] = on[k] || c;
                sl[k].r = vsel(c, vsub(p, xc), sl[k].r);
                sl[k].s0 = c ? sep - P.rest_offset : sl[k].s0;
                cp[k] = vsel(c, p, cp[k]);
            }, &Rq);
        RUSE(sl[0].s0); RUSE(sl[3].r.z);
        if (st < 2) RSTAMP(4 + 6 * st);   // candidates
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) any = any || on[j];
        // the friction patch of this substep (no contact: none)
        if (any) {
            float cs0[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) cs0[j] = sl[j].s0;
            if constexpr (PKG)
                ground_patch_update_pk(G, R, x, q, n0, cp, cs0, on, P.fric_offset, P.fric_corr);
            else
                ground_patch_update(G, R, x, q, n0, cp, cs0, on, P.fric_offset, P.fric_corr);
        } else {
            R.cnt = 0;
        }

        RUSE(R.cnt);
        if (st < 2) RSTAMP(5 + 6 * st);   // patch update
        // 3. TGS (skipped by a wave in which no body touches the ground)
        V3 dx = v3(0.0f, 0.0f, 0.0f), dth = v3(0.0f, 0.0f, 0.0f);
        if (__any(any)) {
            ARow an[2];
            V3 awp[2];   // CREP: the anchors' body copies in the world
            if constexpr (PKG && B::kPacked) {
                // the same constants on packed pairs (mg_pair.h): the x, y of
                // every Iw (r x d) as the pair the solver consumes, the slots'
                // pre-solve normal velocities two at a time, the anchors' world
                // copies, drifts and lever arms as one pair of vectors
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f2 Ixy = z_iwn_xy(Ip, sl[j].r);
                    sl[j].In = v3(Ixy.x, Ixy.y, z_iwn_z(Iw, sl[j].r));
                    if constexpr (!MG_RIGID1_RECIP_PAIRS)
                        sl[j].kn = on[j] ? 1.0f / (invm + G.kn(sl[j].r, sl[j].In)) : 0.0f;
                    sl[j].ln = 0.0f;
                }
                if constexpr (MG_RIGID1_RECIP_PAIRS) {
                    // two slots' denominators as one pair, both reciprocals on
                    // every lane (an inactive slot has r = 0: 1 / invm, unused)
#pragma unroll
                    for (int j = 0; j < 4; j += 2) {
                        const f2 kn = rcp2_ieee(bc2(invm) + z_kn2(v3x2(sl[j].r, sl[j + 1].r),
                                                                   v3x2(sl[j].In, sl[j + 1].In)));
                        sl[j].kn = on[j] ? kn.x : 0.0f;
                        sl[j + 1].kn = on[j + 1] ? kn.y : 0.0f;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    const f2 vn0 = z_vn2(v, w, pk2(sl[j].r.y, sl[j + 1].r.y), pk2(-sl[j].r.x, -sl[j + 1].r.x));
                    sl[j].vn0 = vn0.x;
                    sl[j + 1].vn0 = vn0.y;
                }
                const V3x2 WA = vadd2(v3bc(x), qrot2(q, v3x2(R.aA[0], R.aA[1])));
                const V3x2 DR = vsub2(WA, v3x2(R.aB[0], R.aB[1]));
                const V3x2 RR = vsub2(WA, v3bc(xc));
                const f2 kd2 = bc2(0.8f * P.inv_h);
                const f2 E1 = -DR.y * kd2, E2 = -(-DR.x) * kd2;   // -d1(dr) kd, -d2(dr) kd
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const bool act = a < R.cnt;
                    const V3 r = vsel(act, a ? v3hi(RR) : v3lo(RR), v3(0.0f, 0.0f, 0.0f));
                    const f2 I1xy = z_iw1_xy(Ip, r), I2xy = z_iw2_xy(Ip, r);
                    an[a].r = r;
                    an[a].I1 = v3(I1xy.x, I1xy.y, z_iw1_z(Iw, r));
                    an[a].I2 = v3(I2xy.x, I2xy.y, z_iw2_z(Iw, r));
                    if constexpr (MG_RIGID1_RECIP_PAIRS) {
                        // (k1, k2): z_k1 and z_k2 (mg_pair.h) term by term as one pair
                        const f2 k = rcp2_ieee(bc2(invm) + (bc2(-r.z) * pk2(an[a].I1.x, an[a].I2.y) +
                                                            pk2(r.x, r.y) * pk2(an[a].I1.z, an[a].I2.z)));
                        an[a].k1 = act ? k.x : 0.0f;
                        an[a].k2 = act ? k.y : 0.0f;
                    } else {
                        an[a].k1 = act ? 1.0f / (invm + G.k1(r, an[a].I1)) : 0.0f;
                        an[a].k2 = act ? 1.0f / (invm + G.k2(r, an[a].I2)) : 0.0f;
                    }
                    an[a].l1 = 0.0f;
                    an[a].l2 = 0.0f;
                    an[a].e1 = act ? fminf(fmaxf(a ? E1.y : E1.x, -P.max_depen), P.max_depen) : 0.0f;
                    an[a].e2 = act ? fminf(fmaxf(a ? E2.y : E2.x, -P.max_depen), P.max_depen) : 0.0f;
                }
            } else {
                // contact constants (inactive slots: r = 0, so In = 0, kn = 0)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sl[j].In = G.iwn(Iw, sl[j].r);
                    sl[j].kn = on[j] ? 1.0f / (invm + G.kn(sl[j].r, sl[j].In)) : 0.0f;
                    sl[j].ln = 0.0f;
                    sl[j].vn0 = G.vn(v, w, sl[j].r);
                }
                // anchor rows at the anchors' body copies; the position sweeps close
                // 80 % of the substep-start drift of their two copies
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const bool act = a < R.cnt;
                    // formed on every lane, selected (a divergent branch cost more)
                    const V3 wa = vadd(x, qrot(q, R.aA[a]));
                    if constexpr (CREP) awp[a] = wa;
                    const V3 dr = vsub(wa, R.aB[a]);
                    const float kd = 0.8f * P.inv_h;
                    const V3 r = vsel(act, vsub(wa, xc), v3(0.0f, 0.0f, 0.0f));
                    const float e1 = act ? fminf(fmaxf(-G.d1(dr) * kd, -P.max_depen), P.max_depen) : 0.0f;
                    const float e2 = act ? fminf(fmaxf(-G.d2(dr) * kd, -P.max_depen), P.max_depen) : 0.0f;
                    an[a].r = r;
                    an[a].I1 = G.iw1(Iw, r);
                    an[a].I2 = G.iw2(Iw, r);
                    an[a].k1 = act ? 1.0f / (invm + G.k1(r, an[a].I1)) : 0.0f;
                    an[a].k2 = act ? 1.0f / (invm + G.k2(r, an[a].I2)) : 0.0f;
                    an[a].l1 = 0.0f;
                    an[a].l2 = 0.0f;
                    an[a].e1 = e1;
                    an[a].e2 = e2;
                }
            }
            // the anchors whose bound clamped a row in the last iteration, per
            // anchor and direction: the patch slips when every anchor it holds is
            // clamped along one direction (the Gauss-Seidel sweep may leave one of
            // two anchors at its half budget while the other still holds)
            bool c01 = false, c02 = false, c11 = false, c12 = false;
            // each anchor of a two-anchor patch holds half of the patch's Coulomb
            // budget mu N per direction: symmetric (a box sliding on its diagonal
            // anchors exerts no yaw torque), and the two saturate at mu N together
            const float share = R.cnt == 2 ? 0.5f : 1.0f;
            const int nit = P.npos + P.nvel;
            RUSE(an[1].k2); RUSE(sl[3].kn);
            if (st < 2) RSTAMP(6 + 6 * st);   // row constants, anchor rows
            if constexpr (B::kPacked && PACK) {
                tgs_zp<PKG && MG_RIGID1_SWEEP_PAIRS>(P, sl, an, share * mu, e, v, w, dx, dth, invm, c01, c02, c11, c12);
            } else
            for (int it = 0; it < nit; ++it) {
                const bool pos = it < P.npos, last = it == nit - 1;
                auto normals = [&]() {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float sj = G.ps(sl[j].s0, dx, dth, sl[j].r);
                        row_normal1(G, sl[j], v, w, invm, pos ? pos_target(P, sj) : vel_target(P, sj, e, sl[j].vn0));
                    }
                };
                // sweep order (round 6, oracle rigid_body_step): a position
                // sweep is the anchors' rows then the normal rows; the first
                // and the velocity sweeps open with the normal rows as well
                if (it == 0 || !pos) normals();
                // the patch's normal impulse (slot order)
                const float mun = mu * (((sl[0].ln + sl[1].ln) + sl[2].ln) + sl[3].ln);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    {
                        const float lim = share * mun;
                        const float raw = fmaf(an[a].k1, (pos ? an[a].e1 : 0.0f) - G.v1(v, w, an[a].r), an[a].l1);
                        const float nl = clamp_sym(raw, lim);
                        const float dl = nl - an[a].l1;
                        const bool cl = last && (raw > lim || raw < -lim);
                        if (a == 0) c01 = cl; else c11 = cl;
                        an[a].l1 = nl;
                        v = G.f1(v, dl, invm);
                        w = fmad3(w, an[a].I1, dl);
                    }
                    {
                        const float lim = share * mun;
                        const float raw = fmaf(an[a].k2, (pos ? an[a].e2 : 0.0f) - G.v2(v, w, an[a].r), an[a].l2);
                        const float nl = clamp_sym(raw, lim);
                        const float dl = nl - an[a].l2;
                        const bool cl = last && (raw > lim || raw < -lim);
                        if (a == 0) c02 = cl; else c12 = cl;
                        an[a].l2 = nl;
                        v = G.f2(v, dl, invm);
                        w = fmad3(w, an[a].I2, dl);
                    }
                }
                normals();   // every sweep ends with the normal rows
                if (pos) {
                    dx = fmad3(dx, v, P.sub);
                    dth = fmad3(dth, w, P.sub);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) fsum = G.addn(fsum, sl[j].ln);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                fsum = G.add1(fsum, an[a].l1);
                fsum = G.add2(fsum, an[a].l2);
            }
            if constexpr (CREP) {
                if (cr && st == P.substeps - 1) {
                    const V3 z3 = v3(0.0f, 0.0f, 0.0f);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (on[j]) {
                            crep_store(cr, crs, crk, gbody, -1, 0, cp[j], n0, sl[j].s0, sl[j].ln, z3, mu);
                            crk = crk + 1;
                        }
                    }
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        if (a < R.cnt) {
                            crep_store(cr, crs, crk, gbody, -1, 1, awp[a], n0, 0.0f, 0.0f,
                                       G.add2(G.add1(z3, an[a].l1), an[a].l2), mu);
                            crk = crk + 1;
                        }
                    }
                }
            }
            // a slipping patch lets go (regrown at the next substep)
            const bool one = R.cnt < 2;
            if ((c01 && (c11 || one)) || (c02 && (c12 || one))) R.cnt = 0;
        } else {
            // no solver pass: the motion delta is the substep's free flight
            for (int it = 0; it < P.npos; ++it) {
                dx = fmad3(dx, v, P.sub);
                dth = fmad3(dth, w, P.sub);
            }
        }

        RUSE(dx.x); RUSE(dth.z);
        if (st < 2) RSTAMP(7 + 6 * st);   // solver sweeps (or free flight)
        // 4. pose update (centre of mass moves by the integrated delta)
        const V3 xc1 = vadd(xc, dx);
        q = qintegrate(q, dth);
        x = origin_from_com(xc1, q, com);
        RUSE(x.x); RUSE(q.w);
        if (st < 2) RSTAMP(8 + 6 * st);   // pose update
    }
    // the patch for the next step: the anchor count always, the anchors while held
    if (gp && has_shape) {
        gp[0] = (float)R.cnt;
        if (R.cnt > 0 && R.dirty) {
            const float r[MG_FP_N] = {0.0f, R.nA.x, R.nA.y, R.nA.z,
                                      R.aA[0].x, R.aA[0].y, R.aA[0].z, R.aB[0].x, R.aB[0].y, R.aB[0].z,
                                      R.aA[1].x, R.aA[1].y, R.aA[1].z, R.aB[1].x, R.aB[1].y, R.aB[1].z};
#pragma unroll
            for (int k = 1; k < MG_FP_N; ++k) gp[(size_t)k * gstride] = r[k];
        }
    }
    return crk;
}

// Wide launches: __launch_bounds__(64, 3), at most 168 VGPRs, so three waves
// share a SIMD (the Gauss-Seidel chains are latency-bound: more resident waves,
// not more lanes, fill the SIMD); free of scratch at that budget. One-round
// launches (the packed solver, the shape record in registers): two waves, 175
// VGPRs and no scratch — at three waves the shape record spilled 36 B/lane
// (4096 envs: 13.2 us against 13.5 with the record in LDS and 13.5 at either
// budget, same-box A/B, profiles/r05_ab_rigid_shape_regs.jsonl). The general
// ground basis needs more registers: two waves. So do the reporting builds
// (CREP): at three waves their staging stores spilled 25 to 47 registers.
// (MG_RIGID1_ROUND_WAVES = 2, MG_RIGID1_WIDE_WAVES = 3: mg_forms.h.) BOX (one-round launches with the slot record whose shapes are all plain
// boxes, MgRigidArgs::box_only): the candidates are compiled for the box alone.
template <unsigned F>
__global__ void __launch_bounds__(64, (F & RF_UPZ) && (F & RF_WIDE) && !(F & RF_CREP) ? MG_RIGID1_WIDE_WAVES
                                                                                     : ((F & RF_UPZ) ? MG_RIGID1_ROUND_WAVES : 2))
k_rigid_step1(MgStep P, MgRigidArgs A) {
    static_assert(k_rigid_step1_built(F), "not a build of k_rigid_step1 (mg_forms.h)");
    constexpr bool UPZ = F & RF_UPZ, LDS_T = F & RF_LDS, WIDE = F & RF_WIDE, ATTR = F & RF_ATTR, REC = F & RF_REC,
                   CREP = F & RF_CREP, BOX = F & RF_BOX;
    extern __shared__ float s_trec[];
    const int i = (WIDE ? gridDim.x - 1 - blockIdx.x : blockIdx.x) * 64 + threadIdx.x;
    RSTAMP(0);
    if constexpr (!WIDE) {
        // the kernel arguments the entry needs, as one batch of scalar loads: left
        // to the compiler they came in three dependent batches, each in front of
        // the vector loads it feeds (three scalar-cache trips before the first wait)
        asm volatile("" ::"s"(A.nf), "s"(A.free_ids), "s"(A.nb), "s"(A.slot_rec), "s"(A.gpatch), "s"(A.gstride),
                     "s"(A.trec), "s"(A.ntb), "s"(A.ext), "s"(A.root_src), "s"(A.state), "s"(P.h));
    }
    const bool live = i < A.nf;
    const int b = A.free_ids ? A.free_ids[live ? i : A.nf - 1] : (live ? i : A.nf - 1);
    const int nb = A.nb;
    V3 x, v, w;
    Q4 q;
    int tb;
    V3 fext = v3(0.0f, 0.0f, 0.0f), text = v3(0.0f, 0.0f, 0.0f);
    const float* T;
    // one-round launches: the fused refresh's rows and the ground-patch record at
    // the step's start, loaded with the other inputs (below)
    int pre_ob = -1, pre_or = -1;
    float pr[MG_FP_N];
    if constexpr (WIDE) {
        // this lane's inputs first, so they are in flight with the template staging;
        // a fused root-state set (migym_capi.cpp) supplies them from the actor's row
        // of the user tensor instead (the scatter that would have written them)
        const float* Si = A.state + b;
        int si = nb;
        if (A.root_src) {
            const int rr = A.root_row[b];
            if (rr >= 0) {
                Si = A.root_src + (size_t)rr * MG_STATE_N;
                si = 1;
            }
        }
        x = v3(Si[0 * si], Si[1 * si], Si[2 * si]);
        q = q4(Si[3 * si], Si[4 * si], Si[5 * si], Si[6 * si]);
        v = v3(Si[7 * si], Si[8 * si], Si[9 * si]);
        w = v3(Si[10 * si], Si[11 * si], Si[12 * si]);
        tb = A.body_tmpl[b];
        if (A.ext) {
            fext = v3(A.ext[0 * nb + b], A.ext[1 * nb + b], A.ext[2 * nb + b]);
            text = v3(A.ext[3 * nb + b], A.ext[4 * nb + b], A.ext[5 * nb + b]);
        }
        if constexpr (LDS_T) {
            for (int k = threadIdx.x; k < A.ntb * MG_TREC_N; k += 64) s_trec[k] = A.trec[k];
            __syncthreads();
            T = s_trec + tb * MG_TREC_N;
        } else {
            T = A.trec + tb * MG_TREC_N;
        }
#pragma unroll
        for (int k = 0; k < MG_FP_N; ++k) pr[k] = 0.0f;   // unused: a wide launch reads the record when near
    } else {
        // A one-round launch's time is one wave's memory round trips and its
        // instruction stream, so everything whose address
        // depends on the slot alone is issued here, back to back, before the
        // first wait: the slot's indices as one 16-byte record, the ground-patch
        // record (selected, not read, in rigid_body1: a far body never uses what
        // it fetched), the first two rounds of the template staging, the applied
        // wrench and, with no fused root set, the SoA state. Only the rows of a
        // fused root set (52-byte records at the record's root_row) and a
        // template record read from global memory are a second trip. A dead lane
        // holds the slot of the launch's last body: every address is a live one.
        MgSlotRec rec;
        if constexpr (REC) {
            rec = A.slot_rec[b];
        } else {   // no record (callers with free_ids): the separate arrays, the same values
            rec.root_row = A.root_src ? A.root_row[b] : -1;
            rec.body_tmpl = A.body_tmpl[b];
            rec.out_body = A.out_rb ? A.out_body[b] : -1;
            rec.out_root_row = A.out_root ? A.out_root_row[b] : -1;
        }
        if (A.gpatch) {
#pragma unroll
            for (int k = 0; k < MG_FP_N; ++k) pr[k] = A.gpatch[(size_t)k * A.gstride + b];
        } else {
#pragma unroll
            for (int k = 0; k < MG_FP_N; ++k) pr[k] = 0.0f;
        }
        const int nt = A.ntb * MG_TREC_N, l = threadIdx.x;
        float t0 = 0.0f, t1 = 0.0f;
        if constexpr (LDS_T) {   // clamped, not branched: the store below is the conditional one
            t0 = A.trec[min(l, nt - 1)];
            t1 = A.trec[min(l + 64, nt - 1)];
        }
        if (A.ext) {
            fext = v3(A.ext[0 * nb + b], A.ext[1 * nb + b], A.ext[2 * nb + b]);
            text = v3(A.ext[3 * nb + b], A.ext[4 * nb + b], A.ext[5 * nb + b]);
        }
        float s[MG_STATE_N];
        if (!A.root_src) {
#pragma unroll
            for (int k = 0; k < MG_STATE_N; ++k) s[k] = A.state[k * nb + b];
        }
        // keeps the loads above where they are (as one if-else chain with the
        // same loads below, they were placed behind the wait for the record)
        asm volatile("" ::: "memory");
        // the staged template values go to LDS before the second trip is issued:
        // they arrive with the record (loads return in order), and the reads of
        // the template record then overlap the root rows' flight
        if constexpr (LDS_T) {
            if (l < nt) s_trec[l] = t0;
            if (l + 64 < nt) s_trec[l + 64] = t1;
            for (int k = l + 128; k < nt; k += 64) s_trec[k] = A.trec[k];
            asm volatile("" ::: "memory");
        }
        if (!A.root_src) {
        } else if (rec.root_row >= 0) {
            // the actor's row of the user tensor (the scatter that would have
            // written the SoA state): consecutive floats, loaded four at a time
            const float* Rr = A.root_src + (size_t)rec.root_row * MG_STATE_N;
#pragma unroll
            for (int k = 0; k < MG_STATE_N; ++k) s[k] = Rr[k];
        } else {
#pragma unroll
            for (int k = 0; k < MG_STATE_N; ++k) s[k] = A.state[k * nb + b];
        }
        x = v3(s[0], s[1], s[2]);
        q = q4(s[3], s[4], s[5], s[6]);
        v = v3(s[7], s[8], s[9]);
        w = v3(s[10], s[11], s[12]);
        tb = rec.body_tmpl;
        pre_ob = rec.out_body;
        pre_or = A.out_root ? rec.out_root_row : -1;
        if constexpr (LDS_T) {
            __syncthreads();
            T = s_trec + tb * MG_TREC_N;
        } else {
            T = A.trec + tb * MG_TREC_N;
        }
    }
    // mass row: the template's own when all its bodies share it (the servo scene:
    // no per-body loads), else the body's SoA row (migym_capi.cpp upload)
    float mr[11];
    if (T[5] != 0.0f) {
#pragma unroll
        for (int k = 0; k < 11; ++k) mr[k] = T[MG_TREC_MASS + k];
    } else {
#pragma unroll
        for (int k = 0; k < 11; ++k) mr[k] = A.mass[k * nb + b];
    }
    const float invm = mr[0];
    const V3 invI = v3(mr[1], mr[2], mr[3]);
    const Q4 iq = q4(mr[4], mr[5], mr[6], mr[7]);
    const V3 com = v3(mr[8], mr[9], mr[10]);
    V3 fsum = v3(0.0f, 0.0f, 0.0f);
    RUSE(x.x); RUSE(q.w); RUSE(w.z); RUSE(invm); RUSE(com.z); RUSE(T[4]);
    if constexpr (!WIDE) {
        RUSE(pre_ob); RUSE(pre_or); RUSE(pr[0]); RUSE(pr[MG_FP_N - 1]);
    }
    RSTAMP(1);   // state, template record, mass row (one-round: slot and patch records too) in registers
    // this body's ground-patch record (slot b of the SoA [MG_FP_N][gstride] table)
    // and its LDS copy during the frame
    float* gp = live && A.gpatch ? A.gpatch + b : nullptr;
    const float* at = nullptr;
    if constexpr (ATTR) {
        const int ai = A.attr_idx[b];
        if (live && ai >= 0) at = A.attr + (size_t)ai * MG_ATTR_N;
    }
    // reporting builds: this body's staging record and its global index
    float* cr = nullptr;
    int gbody = 0, crk = 0;
    if constexpr (CREP) {
        if (live) {
            cr = A.crep + b;
            gbody = A.crep_body[b];
        }
    }
    if constexpr (UPZ) {
        crk = rigid_body1<!WIDE, ATTR, CREP, BOX>(BasisZ{}, P, T, x, q, v, w, fsum, invm, invI, iq, com,
                                                  A.ext != nullptr, fext, text, A.hulls, gp, A.gstride, pr, at, cr,
                                                  A.crep_stride, gbody);
    } else {
        BasisGen G;
        G.n = v3(P.n[0], P.n[1], P.n[2]);
        G.t1 = v3(P.t1[0], P.t1[1], P.t1[2]);
        G.t2 = v3(P.t2[0], P.t2[1], P.t2[2]);
        crk = rigid_body1<!WIDE, ATTR, CREP, BOX>(G, P, T, x, q, v, w, fsum, invm, invI, iq, com, A.ext != nullptr,
                                                  fext, text, A.hulls, gp, A.gstride, pr, at, cr, A.crep_stride,
                                                  gbody);
    }
    if constexpr (CREP) {
        if (live) A.crep_n[b] = crk;
    }
    // the output addresses are recomputed here (an opaque copy of the slot)
    // rather than kept live in registers across the frame
    int bo = b;
    asm volatile("" : "+v"(bo));
    if (live) {
        float* So = A.state;
        So[0 * nb + bo] = x.x; So[1 * nb + bo] = x.y; So[2 * nb + bo] = x.z;
        So[3 * nb + bo] = q.x; So[4 * nb + bo] = q.y; So[5 * nb + bo] = q.z; So[6 * nb + bo] = q.w;
        So[7 * nb + bo] = v.x; So[8 * nb + bo] = v.y; So[9 * nb + bo] = v.z;
        So[10 * nb + bo] = w.x; So[11 * nb + bo] = w.y; So[12 * nb + bo] = w.z;
        A.cforce[0 * nb + bo] = fsum.x * P.inv_dt;
        A.cforce[1 * nb + bo] = fsum.y * P.inv_dt;
        A.cforce[2 * nb + bo] = fsum.z * P.inv_dt;
    }
    if ((A.out_rb || A.out_root) && !WIDE) {
        // the refresh fused into the step: the same 13 values into the bound
        // rigid-body row and, for a root body, its actor's root row (the rows the
        // paired gather k_gather_rb_root would write from the SoA state)
        if (live) {
            const float o[MG_STATE_N] = {x.x, x.y, x.z, q.x, q.y, q.z, q.w, v.x, v.y, v.z, w.x, w.y, w.z};
            // the rows came with the slot record at entry: no load, and so no
            // wait, stands between the stores above and these
            const int ob = pre_ob;
            const int rr = pre_or;
            if (A.out_rb) {
                float* R = A.out_rb + (size_t)ob * MG_STATE_N;
#pragma unroll
                for (int k = 0; k < MG_STATE_N; ++k) R[k] = o[k];
            }
            if (rr >= 0) {
                float* Ro = A.out_root + (size_t)rr * MG_STATE_N;
#pragma unroll
                for (int k = 0; k < MG_STATE_N; ++k) Ro[k] = o[k];
            }
        }
        RSTAMP(15);   // all stores issued
#ifdef MG_RIGID1_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        RSTAMP(16);   // stores complete
#endif
    } else if (A.out_rb || A.out_root) {   // launch-uniform
        // Wide launches are issue-bound, and the rows are 52-B AoS records, every
        // other one per wave (the wave holds one template: UAVs or cars): written
        // lane by lane, each store instruction touches 64 rows 104 B apart. The
        // wave's rows are transposed through LDS instead, so that store k writes
        // elements k*64 .. k*64+63 of the wave's 64 x 13 block — runs of
        // consecutive floats, five rows each (262k envs: 46.9 -> 45.6 us; a
        // one-round launch is latency-bound and pays the LDS round trip: 10.2 ->
        // 11.3 us at 4096, so it keeps the direct stores).
        __shared__ float s_out[64 * 16];
        __shared__ int s_dst[2][64];
        const int l = threadIdx.x;
        const float o[MG_STATE_N] = {x.x, x.y, x.z, q.x, q.y, q.z, q.w, v.x, v.y, v.z, w.x, w.y, w.z};
#pragma unroll
        for (int k = 0; k < MG_STATE_N; ++k) s_out[l * 16 + k] = o[k];
        s_dst[0][l] = live && A.out_rb ? A.out_body[bo] : -1;
        s_dst[1][l] = live && A.out_root ? A.out_root_row[bo] : -1;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MG_STATE_N; ++k) {
            const int e = k * 64 + l;
            const int row = e / MG_STATE_N, col = e - row * MG_STATE_N;
            const float val = s_out[row * 16 + col];
            const int d0 = s_dst[0][row], d1 = s_dst[1][row];
            if (d0 >= 0) A.out_rb[(size_t)d0 * MG_STATE_N + col] = val;
            if (d1 >= 0) A.out_root[(size_t)d1 * MG_STATE_N + col] = val;
        }
    }
}

template <unsigned F, int MAXC, bool MULTI>
__global__ void __launch_bounds__(64) k_rigid_step(MgStep P, MgRigidArgs A) {
    static_assert(k_rigid_step_built(F, MAXC, MULTI), "not a build of k_rigid_step (mg_forms.h)");
    constexpr bool UPZ = F & RF_UPZ, ATTR = F & RF_ATTR, CREP = F & RF_CREP;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= A.nf) return;
    const int b = A.free_ids ? A.free_ids[i] : i;
    if constexpr (UPZ) {
        rigid_body<MAXC, MULTI, ATTR, CREP>(BasisZ{}, P, A, b, i);
    } else {
        BasisGen G;
        G.n = v3(P.n[0], P.n[1], P.n[2]);
        G.t1 = v3(P.t1[0], P.t1[1], P.t1[2]);
        G.t2 = v3(P.t2[0], P.t2[1], P.t2[2]);
        rigid_body<MAXC, MULTI, ATTR, CREP>(G, P, A, b, i);
    }
}

// rcp2_ieee (mg_pair.h) over an array, a pair per lane; an odd count's last
// pair takes 1 for its missing half (tests/test_rcp_pairs_gpu.py)
__global__ void __launch_bounds__(256) k_rcp_pairs(const float* d, float* out, int n) {
    const int i = 2 * (blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const bool two = i + 1 < n;
    const f2 r = rcp2_ieee(pk2(d[i], two ? d[i + 1] : 1.0f));
    out[i] = r.x;
    if (two) out[i + 1] = r.y;
}

}  // namespace

hipError_t mg_launch_rcp_pairs(const float* d, float* out, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int pairs = (n + 1) / 2;
    hipLaunchKernelGGL(k_rcp_pairs, dim3((pairs + 255) / 256), dim3(256), 0, s, d, out, n);
    return hipGetLastError();
}

// A.free_ids lists the single-shape bodies first (A.nf1 of them), then the
// multi-shape ones; each group is its own launch, of the build b holds for it
// (mg_forms.h mg_choose_free: the slot record goes to the one-round builds that read it).
hipError_t mg_launch_rigid_step(const MgStep& P, const MgRigidArgs& A, const MgBuilds& b, hipStream_t s) {
    if (A.nf <= 0) return hipSuccess;
    MgRigidArgs A1 = A, A2 = A;
    A2.root_src = nullptr;   // fused root sets only with single-shape bodies (migym_capi.cpp)
    A2.out_rb = nullptr;     // so is the fused refresh (MG_FUSE_STEP_OUT)
    A2.out_root = nullptr;
    A2.gpatch = nullptr;     // ground patches: single-shape bodies (multi-shape ones keep per-point rows)
    A2.slot_rec = nullptr;   // the packed slot record: one-round single-shape launches by slot only
    A1.nf = A.nf1;
    A2.nf = A.nf - A.nf1;
    if (A.free_ids) {
        A2.free_ids = A.free_ids + A.nf1;
    } else {   // bodies in storage slots 0..nf-1: the second group starts at slot nf1
        A2.state = A.state + A.nf1;
        A2.mass = A.mass + A.nf1;
        A2.body_tmpl = A.body_tmpl + A.nf1;
        A2.ext = A.ext ? A.ext + A.nf1 : nullptr;
        A2.cforce = A.cforce + A.nf1;
        A2.attr_idx = A.attr_idx ? A.attr_idx + A.nf1 : nullptr;
        A2.crep = A.crep ? A.crep + A.nf1 : nullptr;
        A2.crep_n = A.crep_n ? A.crep_n + A.nf1 : nullptr;
        A2.crep_body = A.crep_body ? A.crep_body + A.nf1 : nullptr;
    }
    if ((A1.nf > 0 && !mg_build_fits(b.one, mg_args_have(A1), MG_K_RIGID_STEP1)) ||
        (A2.nf > 0 && !mg_build_fits(b.multi, mg_args_have(A2), MG_K_RIGID_STEP)))
        return hipErrorInvalidValue;
    bool ok = true;
    if (A1.nf > 0) {
        // a wide launch is issue-bound, not latency-bound: it dispatches
        // longest-first (back to front: the free-body order, migym_capi.cpp) and
        // solves with the scalar rows (tgs_z's packed pairs are fewer
        // instructions for a wave alone on its SIMD, but each holds the issue
        // slots of two scalar ones when waves share it: DESIGN.md §3.2).
        const int blocks = (A1.nf + 63) / 64;
        const size_t lds = (size_t)A.ntb * MG_TREC_N * sizeof(float);
        ok = MG_LAUNCH_FORM(RF_BITS, b.one.form, k_rigid_step1_built(F), k_rigid_step1<F>, dim3(blocks),
                            (F & RF_LDS) ? lds : 0, s, P, A1);
    }
    if (A2.nf > 0) {
        const int blocks = (A2.nf + 63) / 64;
        ok = MG_LAUNCH_FORM(RF_BITS, b.multi.form, k_rigid_step_built(F, MG_MAX_CONTACTS, true),
                            (k_rigid_step<F, MG_MAX_CONTACTS, true>), dim3(blocks), 0, s, P, A2) && ok;
    }
    return ok ? hipGetLastError() : hipErrorNotSupported;
}
